"""hipfuse regions with symbolic dims (``cache="symbolic values"``): elementwise ops, broadcasts, unit reshapes,
transposes, ``full``, Philox draws and row reductions over constant extents fuse into kernels that take their
extents and strides as arguments, so one program and a handful of code objects serve every size.

Numerics yardstick: the static-shape program of the same function on the same inputs (``thunder.jit`` with the
default cache), bit for bit, plus eager within the tolerances of tests/test_hipfuse.py.
"""
import os
import re

import pytest
import torch

import lightning_thunder_amd as thunder
from lightning_thunder_amd.core.prims import PrimIDs
from lightning_thunder_amd.core.proxies import TensorProxy
from lightning_thunder_amd.core.symbolic import SymInt
from lightning_thunder_amd.executors import hipfuse
from lightning_thunder_amd.executors import hipfuse_codegen as cg
from kernel_checks import bits_equal

LIB = os.path.join(os.path.dirname(thunder.__file__), "ops", "_lta_kernels.so")
EX = ["hipfuse", "torch"]


@pytest.fixture
def cpu_fusion():
    old = hipfuse.ex.allow_cpu
    hipfuse.ex.allow_cpu = True
    yield
    hipfuse.ex.allow_cpu = old


def _tup(x):
    return x if isinstance(x, tuple) else (x,)


def _regions(jf, backward=False):
    tr = (thunder.last_backward_traces(jf) if backward else thunder.last_traces(jf))[-1]
    return [fb._call_ctx[fb.sym.name] for fb in hipfuse.fusions(tr)]


def _has_symbolic_input(f) -> bool:
    return any(isinstance(p, TensorProxy) and any(isinstance(d, SymInt) for d in p.shape) for p in f.inputs)


def _gelu_res(x, b, r):
    y = torch.nn.functional.gelu(x + b, approximate="tanh") * 0.5 + r
    return y, y.transpose(1, 2).exp()


class _BiasSoftmax(torch.nn.Module):
    """The bias is a parameter, so the last dim is a constant of the program."""

    def __init__(self, C):
        super().__init__()
        self.b = torch.nn.Parameter(torch.randn(C))

    def forward(self, x, r):
        y = torch.nn.functional.gelu(x + self.b, approximate="tanh") * 0.5 + r
        return torch.softmax(y, -1)


def _softmax_args(x, b, r):
    y = torch.nn.functional.gelu(x + b, approximate="tanh") * 0.5 + r
    return torch.softmax(y, -1)


def _guards(jf) -> str:
    return thunder.compile_stats(jf).interpreter_cache[-1].shape_guards.source


def _targs(f, sizes: dict, dtype=None):
    """Dense, aligned TensorArgs of region ``f`` with every symbolic dim whose traced value is a key of
    ``sizes`` replaced by its value there."""
    from lightning_thunder_amd.core import dtypes as _dt

    out = {}
    for p in f.inputs:
        if isinstance(p, TensorProxy):
            shape = tuple(sizes.get(d.value, d.value) if isinstance(d, SymInt) else int(d) for d in p.shape)
            out[p.name] = cg.TensorArg(shape, cg._contig_strides(shape), dtype or _dt.to_torch_dtype(p.dtype), True)
    return out


# ------------------------------------------------------------------------------------------
# CPU: admission, guards, one source for all sizes
# ------------------------------------------------------------------------------------------
def test_symbolic_regions_form_cpu(cpu_fusion):
    """1. Elementwise + broadcast + transpose under symbolic values: one region with symbolic inputs serves
    three lengths through one cache entry (the parent commit forms no region here)."""
    jf = thunder.jit(_gelu_res, executors=EX, cache="symbolic values")
    for T in (3, 5, 9):
        args = (torch.randn(2, T, 24), torch.randn(24), torch.randn(2, T, 24))
        for o, e in zip(jf(*args), _gelu_res(*args)):
            torch.testing.assert_close(o, e, rtol=1e-5, atol=1e-5)
    tr = thunder.last_traces(jf)[-1]
    fus = hipfuse.fusions(tr)
    assert len(fus) >= 1
    assert any(_has_symbolic_input(f) for f in _regions(jf))
    assert re.search(r'f32\[[^\]]*\bs\d+\b', str(tr))
    assert thunder.cache_misses(jf) == 1 and thunder.cache_hits(jf) == 2


def test_constant_reduced_extent_fuses_cpu(cpu_fusion):
    """2. A softmax over a dim a parameter pins to a constant joins a row-mode region; one entry."""
    torch.manual_seed(0)
    m = _BiasSoftmax(24)
    jm = thunder.jit(m, executors=EX, cache="symbolic values")
    with torch.no_grad():
        for T in (3, 5, 9):
            x, r = torch.randn(2, T, 24), torch.randn(2, T, 24)
            torch.testing.assert_close(jm(x, r), m(x, r), rtol=1e-5, atol=1e-5)
    regs = [f for f in _regions(jm) if f.plan.red > 0]
    assert regs and regs[0].symbolic
    assert any(b.sym.id in (PrimIDs.AMAX, PrimIDs.SUM) for b in regs[0].nodes)
    assert thunder.cache_misses(jm) == 1 and thunder.cache_hits(jm) == 2


def test_symbolic_reduced_extent_stays_per_op_cpu(cpu_fusion):
    """3. The same softmax over a bare symbol: the reduction stays out of every region, the program is right
    through one entry, and fusing specialises no size the program without hipfuse does not specialise."""
    jf = thunder.jit(_softmax_args, executors=EX, cache="symbolic values")
    jt = thunder.jit(_softmax_args, executors=["torch"], cache="symbolic values")
    for T in (3, 5, 9):
        args = (torch.randn(2, T, 24), torch.randn(24), torch.randn(2, T, 24))
        torch.testing.assert_close(jf(*args), _softmax_args(*args), rtol=1e-5, atol=1e-5)
        jt(*args)
    for f in _regions(jf):
        assert f.plan.red == 0 and not any(b.sym.id in cg.REDUCTIONS for b in f.nodes)
    assert thunder.cache_misses(jf) == 1 and thunder.cache_hits(jf) == 2
    spec = re.compile(r"\(?\b[s\d+*/% ()-]*s\d+[s\d+*/% ()-]*\)? == \d+")
    mine = {m.group(0) for m in spec.finditer(_guards(jf))}
    theirs = {m.group(0) for m in spec.finditer(_guards(jt))}
    assert mine <= theirs, (mine - theirs, _guards(jf))


@pytest.mark.skipif(not os.path.exists(LIB), reason="native library not built")
def test_one_source_for_all_sizes_cpu(cpu_fusion, monkeypatch, tmp_path):
    """4. The region's source does not depend on the sizes (same alignment and stride classes), precompile
    builds it with hiprtc, and no later size compiles anything."""
    monkeypatch.setenv("LTA_CACHE_DIR", str(tmp_path))
    jf = thunder.jit(_gelu_res, executors=EX, cache="symbolic values")
    for T in (3, 5, 9):
        jf(torch.randn(2, T, 24), torch.randn(24), torch.randn(2, T, 24))
    (f,) = _regions(jf)
    assert f.symbolic
    a = cg.generate(f.plan, f.inputs, f.outputs, _targs(f, {}))
    b = cg.generate(f.plan, f.inputs, f.outputs, _targs(f, {3: 130, 2: 5}))
    assert a.name == b.name and a.src == b.src
    assert "A.ext[" in a.src and a.sym_mode == ("pointwise", 8)
    before = hipfuse.RTC_STATS["compiled"]
    assert hipfuse.precompile(thunder.last_traces(jf)[-1]) == 1
    assert hipfuse.RTC_STATS["compiled"] == before + 1
    hipfuse.precompile(thunder.last_traces(jf)[-1])
    hipfuse.compile_source(b)
    assert hipfuse.RTC_STATS["compiled"] == before + 1


@pytest.mark.skipif(not os.path.exists(LIB), reason="native library not built")
def test_dense_region_needs_no_decomposition_and_wide_indices_compile_cpu(cpu_fusion, monkeypatch, tmp_path):
    """A region whose operands are all identity-mapped and dense addresses by the flat index alone; above
    2^31 elements the same region is generated with 64-bit indices and compiles (that variant never ran on a
    GPU: such tensors do not fit a test)."""
    monkeypatch.setenv("LTA_CACHE_DIR", str(tmp_path))

    def f(x, r):
        return torch.tanh(x) * r + 1.0

    jf = thunder.jit(f, executors=EX, cache="symbolic values")
    x, r = torch.randn(2, 5, 24), torch.randn(2, 5, 24)
    torch.testing.assert_close(jf(x, r), f(x, r), rtol=1e-5, atol=1e-5)
    (reg,) = _regions(jf)
    ks = cg.generate(reg.plan, reg.inputs, reg.outputs, _targs(reg, {}))
    assert not re.search(r"\bi\d+\b", ks.src.split("__launch_bounds__")[1]), ks.src
    assert "const unsigned E0" in ks.src
    big = cg.generate(reg.plan, reg.inputs, reg.outputs, _targs(reg, {2: 8, 5: 2 ** 20, 24: 264}))
    assert "const unsigned long long E0" in big.src and big.name != ks.name
    assert len(hipfuse.compile_source(big)) > 1000
    # a strided operand of the same region: decomposed, runtime strides, scalar loads
    ta = _targs(reg, {})
    first = next(iter(ta))
    ta[first] = cg.TensorArg(ta[first].shape, (240, 48, 2), ta[first].dtype, True)
    st = cg.generate(reg.plan, reg.inputs, reg.outputs, ta)
    assert "A.str[" in st.src and re.search(r"\bi1\b", st.src)
    assert len(hipfuse.compile_source(st)) > 1000


# kernel names of three default-cache regions of tests/test_hipfuse.py's CASES (fp32, dense, aligned) as the
# commit before symbolic regions generated them: a pointwise, a row and a column region
_PARENT_NAMES = {
    "pointwise_bcast": "lta_fused_09a4a1d84d903215",
    "ln_gelu_softmax": "lta_fused_492ae4e7cc9b4627",
    "bias_grad": "lta_fused_191e285ff9f83692",
}


@pytest.mark.parametrize("case", sorted(_PARENT_NAMES))
def test_static_regions_unchanged_cpu(case, cpu_fusion):
    """5. Regions without a symbolic dim generate byte-identical source (the name is its hash)."""
    import test_hipfuse as th

    fn, mk = th.CASES[case]
    jf = thunder.jit(fn, executors=EX)
    jf(*mk(torch.float32, "cpu"))
    (f,) = _regions(jf)
    assert not f.symbolic
    targs = {p.name: cg.TensorArg(tuple(p.shape), tuple(torch.empty(tuple(p.shape)).stride()), p.dtype, True)
             for p in f.inputs if isinstance(p, TensorProxy)}
    assert cg.generate(f.plan, f.inputs, f.outputs, targs).name == _PARENT_NAMES[case]


def _embed_add(idx, w, p):
    return torch.nn.functional.embedding(idx, w) + p


def _reshape_work(x):
    return torch.tanh(x.reshape(x.shape[0] * x.shape[1], x.shape[2])) * 2.0 + 1.0


def _lead_sum(x):
    return (x * 0.5).sum(0)


_NOT_ADMITTED = {
    "gather": (_embed_add, lambda T: (torch.randint(0, 50, (2, T)), torch.randn(50, 24), torch.randn(2, T, 24))),
    "reshape": (_reshape_work, lambda T: (torch.randn(2, T, 24),)),
    "leading_sum": (_lead_sum, lambda T: (torch.randn(T, 24),)),
}


@pytest.mark.parametrize("case", sorted(_NOT_ADMITTED))
def test_not_admitted_ops_keep_working_cpu(case, cpu_fusion):
    """6. Gathers, general reshapes and leading-dim reductions stay out of symbolic regions and stay right."""
    fn, mk = _NOT_ADMITTED[case]
    jf = thunder.jit(fn, executors=EX, cache="symbolic values")
    for T in (5, 9):
        args = mk(T)
        torch.testing.assert_close(jf(*args), fn(*args), rtol=1e-5, atol=1e-5)
    assert thunder.cache_misses(jf) == 1 and thunder.cache_hits(jf) == 1
    bad = {PrimIDs.EMBEDDING, PrimIDs.TAKE}
    for f in _regions(jf):
        assert not f.plan.colred and not f.plan.has_pad
        assert not any(b.sym.id in bad for b in f.nodes)


def test_empty_batch_cpu(cpu_fusion):
    """7. B = 0 through the program traced at B = 2: correctly shaped empty outputs when the guards admit the
    call, an ordinary guarded miss (a second entry) when they do not."""
    jf = thunder.jit(_gelu_res, executors=EX, cache="symbolic values")
    jf(torch.randn(2, 5, 24), torch.randn(24), torch.randn(2, 5, 24))
    y, z = jf(torch.randn(0, 5, 24), torch.randn(24), torch.randn(0, 5, 24))
    assert y.shape == (0, 5, 24) and z.shape == (0, 24, 5)
    assert thunder.cache_misses(jf) + thunder.cache_hits(jf) == 2


def test_unbindable_extent_forms_no_region_cpu(cpu_fusion):
    """A region whose symbolic extent no tensor input carries (a ``full`` of a symbolic shape and work on it
    alone) is not formed."""

    def f(x):
        z = torch.full((x.shape[0], x.shape[1]), 2.0)
        return torch.tanh(z) * 3.0 + 1.0, x.sum()

    jf = thunder.jit(f, executors=EX, cache="symbolic values")
    for T in (5, 9):
        x = torch.randn(3, T)
        for o, e in zip(jf(x), f(x)):
            torch.testing.assert_close(o, e, rtol=1e-5, atol=1e-5)
    for reg in _regions(jf):
        assert not any(b.sym.id == PrimIDs.FULL for b in reg.nodes)


# ------------------------------------------------------------------------------------------
# GPU: bit for bit against the static-shape program
# ------------------------------------------------------------------------------------------
def _to64(x):
    return x.double() if isinstance(x, torch.Tensor) and x.is_floating_point() else x


def _check(out, static, eager, ref64, dtype, what):
    """Bit for bit against the static program; against eager as tests/test_hipfuse.py does for the dtype."""
    for o, s, e, r in zip(_tup(out), _tup(static), _tup(eager), _tup(ref64)):
        assert o.shape == e.shape and o.dtype == e.dtype, (what, o.shape, e.shape)
        assert bits_equal(o, s), (what, (o.float() - s.float()).abs().max().item())
        if dtype == torch.float32:
            torch.testing.assert_close(o, e, rtol=1e-5, atol=1e-5)
        else:  # test_fused_numerics_gpu
            err = (o.double() - r).abs().max().item()
            err_e = (e.double() - r).abs().max().item()
            assert err <= 2 * err_e + 1e-5, (what, err, err_e)


def _run_pair(fn, mk_args, sizes, dtype, what, module=False, expect_generated=None):
    """``fn`` under symbolic values at every size (through ONE entry) against the default-cache program, eager
    and fp64.  ``expect_generated``: RTC_STATS["generated"] growth of the symbolic program after each size
    (default: only the first size generates)."""
    sym = thunder.jit(fn, executors=EX, cache="symbolic values")
    static = thunder.jit(fn, executors=EX)
    fn64 = fn
    if module:
        import copy

        fn64 = copy.deepcopy(fn).double()
    base = dict(hipfuse.RTC_STATS)
    first = None
    with torch.no_grad():
        for n, size in enumerate(sizes):
            args = mk_args(size, dtype)
            out = sym(*args)
            torch.cuda.synchronize()
            grown = hipfuse.RTC_STATS["generated"] - base["generated"]
            if expect_generated is not None:
                assert grown == expect_generated[n], (what, size, grown, expect_generated)
            elif first is None:
                first = grown
            else:
                assert grown == first, (what, size, grown, first)
            snap = dict(hipfuse.RTC_STATS)
            ref = static(*args)
            hipfuse.RTC_STATS.update(snap)  # the static program's kernels are not the symbolic program's
            _check(out, ref, fn(*args), fn64(*[_to64(a) for a in args]), dtype, (what, size))
    assert thunder.cache_misses(sym) == 1 and thunder.cache_hits(sym) == len(sizes) - 1
    regs = _regions(sym)
    assert regs and any(f.symbolic for f in regs), what
    return sym


class _GeluRes(torch.nn.Module):
    def __init__(self, C, dtype):
        super().__init__()
        self.b = torch.nn.Parameter(torch.randn(C, device="cuda", dtype=dtype))

    def forward(self, x, r):
        return _gelu_res(x, self.b, r)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_pointwise_constant_inner_dim_gpu(dtype):
    """a. C = 24 is a constant (vector width 8); (B, T) vary.  One kernel serves every size."""
    torch.manual_seed(0)
    m = _GeluRes(24, dtype)
    mk = lambda s, dt: (torch.randn(s[0], s[1], 24, device="cuda", dtype=dt), torch.randn(s[0], s[1], 24, device="cuda", dtype=dt))
    sym = _run_pair(m, mk, [(2, 3), (2, 5), (3, 130)], dtype, "pointwise-const-inner", module=True)
    (f,) = [f for f in _regions(sym) if f.symbolic]
    assert len(f._variants) == 1 and next(iter(f._variants.values()))[1].vec == 8


@pytest.mark.gpu
def test_pointwise_symbolic_inner_dim_gpu():
    """b. The innermost dim is a symbol: the call's value picks the vector width by divisibility, 7 -> 1,
    8 -> 8, 12 -> 4, and 9 -> 1 again (the kernel built for 7).  One region, so ``generated`` reads 1, 2, 3, 3."""
    torch.manual_seed(0)
    mk = lambda C, dt: (torch.randn(2, 5, C, device="cuda", dtype=dt), torch.randn(C, device="cuda", dtype=dt),
                        torch.randn(2, 5, C, device="cuda", dtype=dt))
    sym = _run_pair(_gelu_res, mk, [7, 8, 12, 9], torch.float32, "pointwise-symbolic-inner", expect_generated=[1, 2, 3, 3])
    (f,) = _regions(sym)
    assert sorted(v[1].vec for v in f._variants.values()) == [1, 4, 8]


def _bcast_transposed(x, w, m):
    return (x * w + m).transpose(1, 2) + 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_broadcast_transpose_strided_input_gpu(dtype):
    """c. x[B, T, C] * w[C] + m[B, 1, 1] stored transposed [B, C, T]; x is a non-contiguous view made outside
    the region (every other row of a base tensor): runtime strides, scalar stores."""
    torch.manual_seed(0)

    def mk(T, dt):
        base = torch.randn(3, 2 * T, 24, device="cuda", dtype=dt)
        return base[:, ::2], torch.randn(24, device="cuda", dtype=dt), torch.randn(3, 1, 1, device="cuda", dtype=dt)

    _run_pair(_bcast_transposed, mk, [5, 64, 67], dtype, "bcast-transpose")


class _RowSoftmax(torch.nn.Module):
    def __init__(self, R, dtype):
        super().__init__()
        self.b = torch.nn.Parameter(torch.randn(R, device="cuda", dtype=dtype))

    def forward(self, x):
        return torch.softmax(x + self.b, -1)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("R,rows", [(40, (6, 70, 128)), (1000, (3, 9, 8)), (4104, (3, 9))])
def test_row_softmax_constant_last_dim_gpu(R, rows, dtype):
    """d. Row mode over a constant last dim with a symbolic row count, at row counts that are and are not
    multiples of the rows per workgroup: R = 40 (4 lanes per row, 64 rows per workgroup), R = 1000 (one
    wave per row, 4 rows per workgroup) and R = 4104 (256 lanes per row, the LDS exchange between waves)."""
    torch.manual_seed(0)
    m = _RowSoftmax(R, dtype)
    sym = _run_pair(m, lambda n, dt: (torch.randn(n, R, device="cuda", dtype=dt),), list(rows), dtype, f"softmax-{R}",
                    module=True)
    (f,) = [f for f in _regions(sym) if f.symbolic]
    assert f.plan.red == 1
    mode = next(iter(f._variants.values()))[1].mode
    assert mode == {40: "row(T=4)", 1000: "row(T=64)", 4104: "row(T=256)"}[R], mode


class _LayerNorm(torch.nn.Module):
    def __init__(self, R, dtype):
        super().__init__()
        self.w = torch.nn.Parameter(torch.randn(R, device="cuda", dtype=dtype))
        self.b = torch.nn.Parameter(torch.randn(R, device="cuda", dtype=dtype))

    def forward(self, x):
        var, mean = torch.var_mean(x, -1, keepdim=True, correction=0)
        return (x - mean) * torch.rsqrt(var + 1e-5) * self.w + self.b


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_var_mean_layer_norm_gpu(dtype):
    """e. LayerNorm written out over ``var_mean`` (the two-pass path), R = 96, symbolic T."""
    torch.manual_seed(0)
    m = _LayerNorm(96, dtype)
    sym = _run_pair(m, lambda T, dt: (torch.randn(2, T, 96, device="cuda", dtype=dt),), [3, 33], dtype, "layernorm", module=True)
    assert any(b.sym.id == PrimIDs.VAR_MEAN for f in _regions(sym) if f.symbolic for b in f.nodes)


class _BiasGeluDropout(torch.nn.Module):
    def __init__(self, C):
        super().__init__()
        self.b = torch.nn.Parameter(torch.randn(C, device="cuda"))

    def forward(self, x):
        return torch.nn.functional.dropout(torch.nn.functional.gelu(x + self.b, approximate="tanh"), 0.25)


@pytest.mark.gpu
def test_dropout_same_mask_as_static_gpu():
    """f. dropout(gelu(x + b), 0.25) forward and backward under the same seed as the static program.  The kept
    elements are exactly the static program's in the output and in the input gradient, so the Philox index (the
    flat position in the domain) has not moved, and the forward output is bit for bit the static program's.
    The gradients are NOT bit for bit, the one such case of this file: the static backward is ONE column-mode
    region (dx and the bias gradient sum(dx, (0, 1)) together), column mode is out of scope for symbolic
    regions, so the symbolic backward is a pointwise region plus ATen's sum.  hipcc contracts the two kernels'
    multiply-adds differently and the sums run in another order: on an MI355X dx differs by one fp32 ulp
    (2.4e-7 at T = 4, 4.8e-7 at T = 36) and db by up to 1.9e-6.  Both programs' gradients are therefore held to
    the fp64 evaluation (kernel_checks tolerance, ref32 = the eager fp32 evaluation with the same mask): the
    worst err / tol measured is 0.10 for the symbolic and 0.14 for the static program."""
    from kernel_checks import F32, assert_within

    torch.manual_seed(0)
    m = _BiasGeluDropout(24)
    sym = thunder.jit(m, executors=EX, cache="symbolic values")
    static = thunder.jit(m, executors=EX)

    def reference(x, b, g, mask, dt):
        x, b = x.detach().to(dt).requires_grad_(True), b.detach().to(dt).requires_grad_(True)
        y = torch.nn.functional.gelu(x + b, approximate="tanh") * mask.to(dt) * (1.0 / 0.75)
        y.backward(g.to(dt))
        return y.detach(), x.grad, b.grad

    for T in (4, 36):
        x = torch.randn(2, T, 24, device="cuda")
        g = torch.randn(2, T, 24, device="cuda")
        res = []
        for jm in (sym, static):
            xi = x.clone().requires_grad_(True)
            torch.manual_seed(1)
            out = jm(xi)
            out.backward(g)
            res.append((out.detach(), xi.grad.clone(), m.b.grad.clone()))
            m.zero_grad()
        for a, b in zip(res[0][:2], res[1][:2]):
            assert torch.equal(a == 0, b == 0), T  # the same elements dropped
        assert (res[0][0] == 0).any() and (res[0][0] != 0).any()
        assert bits_equal(res[0][0], res[1][0]), (T, (res[0][0] - res[1][0]).abs().max().item())
        mask = res[1][0] != 0
        ref64, ref32 = reference(x, m.b, g, mask, torch.float64), reference(x, m.b, g, mask, torch.float32)
        for who, r in zip(("symbolic", "static"), res):
            for what, o, r64, r32 in zip(("out", "dx", "db"), r, ref64, ref32):
                print(f"T={T} {who} {what}: max |symbolic - static| = {(o - res[1][('out', 'dx', 'db').index(what)]).abs().max().item():.3e}")
                assert_within(o, r64, r32, F32, "symbolic-dropout", f"T={T} {who} {what}")
    assert thunder.cache_misses(sym) == 1 and thunder.cache_hits(sym) == 1
    assert any(f.symbolic and any(b.sym.id == PrimIDs.UNIFORM_PHILOX for b in f.nodes)
               for f in _regions(sym) + _regions(sym, backward=True))


@pytest.mark.gpu
def test_empty_extent_gpu():
    """A call whose bound extent is 0 returns correctly shaped empty outputs without a launch."""
    jf = thunder.jit(_gelu_res, executors=EX, cache="symbolic values")
    mk = lambda B: (torch.randn(B, 5, 24, device="cuda"), torch.randn(24, device="cuda"), torch.randn(B, 5, 24, device="cuda"))
    jf(*mk(2))
    y, z = jf(*mk(0))
    assert y.shape == (0, 5, 24) and z.shape == (0, 24, 5)


class _MLPBlock(torch.nn.Module):
    """A GPT-2-style MLP block: Linear -> bias -> GELU(tanh) -> Linear -> dropout -> residual."""

    def __init__(self, d=64, hidden=256, p=0.1):
        super().__init__()
        self.fc = torch.nn.Linear(d, hidden, bias=False)
        self.b = torch.nn.Parameter(torch.zeros(hidden))
        self.proj = torch.nn.Linear(hidden, d)
        self.p = p

    def forward(self, x):
        h = torch.nn.functional.gelu(self.fc(x) + self.b, approximate="tanh")
        return x + torch.nn.functional.dropout(self.proj(h), self.p, self.training)


def _rel(a, b):
    return ((a.float() - b.float()).norm() / (b.float().norm() + 1e-12)).item()


@pytest.mark.gpu
def test_training_mlp_block_one_entry_gpu():
    """g. The non-vacuous counterpart of test_symbolic_litgpt_three_lengths_one_entry_gpu: a bf16 MLP block
    trains at three lengths through ONE entry whose forward and backward traces hold hipFusion regions with
    symbolic inputs, and nothing is generated or compiled after the first length.  The dropout mask is the
    program's own Philox draw, which eager cannot reproduce, so the numbers are compared with dropout switched
    off (``eval()``; a second symbolic program, also one entry): loss and parameter gradients within 3x the
    error of eager bf16 against an fp32 model."""
    torch.manual_seed(0)
    dev = torch.device("cuda")
    m32 = _MLPBlock().to(dev)
    with torch.no_grad():
        m32.b.normal_(std=0.5)
    m = _MLPBlock().to(dev)
    m.load_state_dict(m32.state_dict())
    m = m.to(torch.bfloat16)
    jm = thunder.jit(m, cache="symbolic values")
    counts = None
    for T in (128, 256, 384):
        x = torch.randn(2, T, 64, device=dev, dtype=torch.bfloat16)
        loss = jm(x).float().pow(2).mean()
        loss.backward()
        assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.parameters())
        m.zero_grad()
        if counts is None:
            counts = dict(hipfuse.RTC_STATS)
    assert thunder.cache_misses(jm) == 1 and thunder.cache_hits(jm) == 2
    assert hipfuse.RTC_STATS == counts, (hipfuse.RTC_STATS, counts)
    assert any(f.symbolic and _has_symbolic_input(f) for f in _regions(jm)), thunder.last_traces(jm)[-1]
    assert any(f.symbolic and _has_symbolic_input(f) for f in _regions(jm, backward=True)), thunder.last_backward_traces(jm)[-1]

    m.eval(), m32.eval()
    je = thunder.jit(m, cache="symbolic values")
    for T in (128, 256, 384):
        x = torch.randn(2, T, 64, device=dev, dtype=torch.bfloat16)
        got, eag, ref = {}, {}, {}
        for fn, xin, store in ((je, x, got), (m, x, eag), (m32, x.float(), ref)):
            mod = m32 if fn is m32 else m
            loss = fn(xin).float().pow(2).mean()
            loss.backward()
            store["loss"] = loss.detach()
            store.update({n: p.grad.float().clone() for n, p in mod.named_parameters()})
            mod.zero_grad()
        for n in ref:
            base = max(_rel(eag[n], ref[n]), 1e-6)
            assert _rel(got[n], ref[n]) <= 3 * base + 1e-5, (T, n, _rel(got[n], ref[n]), base)
    assert thunder.cache_misses(je) == 1 and thunder.cache_hits(je) == 2
