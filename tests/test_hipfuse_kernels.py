"""The kernels hipfuse generates at run time (executors/hipfuse_codegen.py), mode by mode, vector width by
vector width and tail by tail, against fp64 references of the same functions:

* one table (``CASES``) maps every (function, shape) to the ``(mode, vec, grid)`` the generator must pick for
  it: pointwise at every vector width and at the grid cap, row mode at every lane count ``T`` with and without
  a tail, one to three passes and two reduced dims, column mode with one split, several, a short last split,
  more splits than the last workgroup has waves for, masked column tails and every partial hand-off.  The
  table is asserted on the CPU (where every source is also compiled for gfx950) and again by every GPU case, so
  a retuned heuristic fails here instead of silently uncovering a branch;
* numerics in fp32, bf16 and fp16: the functions upcast once, compute in fp32 and round once to ``T``, so
  ``kernel_checks.assert_within`` applies as it stands: ``ulp(T) |ref64| + 8 e32 + floor`` per element, with
  ``ref64`` the same function on the inputs upcast (exactly) to fp64 and ``e32`` the error of plain torch fp32.
  Column sums take the floor relative to the largest reference (``rel_floor``).  The only ``extra`` term is
  the documented error of the 16-bit fast exp (``|x| 6e-8`` relative) where softmax arguments reach 160;
* edge inputs (``-inf`` next to finite values, constant rows, one NaN, softmax arguments of +-80);
* operand layouts: the same values through a padded pitch, an address that is no multiple of 16 bytes, an
  odd pitch and (pointwise) a transposed operand must give the same bits as the contiguous operand: only the
  load instructions differ, not the order of arithmetic;
* data movement (slice, cat, pad, a transposed store, index_select / gather / embedding, a reshape that
  copies) followed only by multiplications by 2.0, bit for bit against eager torch;
* the column hand-off between workgroups: repeated calls, two kernels with different numbers of column
  groups interleaved on the shared arrival counters, a graph replay, and the ``fence`` / ``twopass`` variants
  of ``LTA_HIPFUSE_COL_SYNC``.

Every line ``[group dtype] ... err/tol=`` is printed with ``-s``.
"""
import os
import zlib

import pytest
import torch
import torch.nn.functional as F

import lightning_thunder_amd as thunder
from lightning_thunder_amd.core.proxies import TensorProxy
from lightning_thunder_amd.executors import hipfuse
from lightning_thunder_amd.executors import hipfuse_codegen as cg

from kernel_checks import _WORST, BF16, F16, F32, assert_within_finite, bits_equal, nan_padded, odd_pitch, offset_by_one

gpu = pytest.mark.gpu
F64 = torch.float64
DTYPES = [F32, BF16, F16]
LIB = os.path.join(os.path.dirname(thunder.__file__), "ops", "_lta_kernels.so")

# Largest err / tol measured on MI355X per group, fp32 / bf16 / fp16 (every run prints them with -s):
#   pointwise       0.15 / 0.99 / 0.50   (fp32: pw_3x1000; bf16: pw_1031x2049; fp16: the int64 operand)
#   row softmax     0.07 / 0.97 / 0.49   (sm_257x8; bf16: sm_65x40)
#   row reduce      0.10 / 0.80 / 0.45   (row4_37x50: the product; bf16: the sum)
#   layernorm       0.07 / 0.99 / 0.49   (bf16 / fp16: the constant row)
#   column          0.06 / 0.99 / 0.49   (fp32: col_130x520; 16-bit: the full-domain output of full_and_col)
# A correctly rounded bf16 output reaches 1.0 of the rounding term alone and fp16 0.5, as in the other
# batteries; the fp32 figures are the share of 8 e32 + floor the kernels use.  No case needed more than the
# base formula; the ``extra`` of the |x| = 80 softmax is at most 2e-5 of an element.  Every bit-identity
# held: layouts against the contiguous run, data movement against eager torch, repeated / interleaved /
# replayed column kernels, ``fence`` against the coherent hand-off.  The GPU tests take 30 s (183 tests, the
# slowest 1.7 s: the first launch), nearly all of it hiprtc.


# ------------------------------------------------------------------------------------------------
# the functions: ``up`` is the compute type (fp32 in the kernel and in the fp32 evaluation, fp64 in the
# reference), ``out`` the type of the one rounding at the end
# ------------------------------------------------------------------------------------------------
def _pw(x, b, up, out):
    return (F.silu(x.to(up) + b.to(up)) * 2.0).to(out)


def _softmax(x, b, up, out):
    return torch.softmax(x.to(up) + b.to(up), -1).to(out)


def _layer_norm(corr):
    def fn(x, w, b, up, out):
        xf = x.to(up)
        var, mean = torch.var_mean(xf, -1, correction=corr, keepdim=True)
        return ((xf - mean) * torch.rsqrt(var + 1e-5) * w.to(up) + b.to(up)).to(out)

    return fn


def _row4(x, up, out):
    xf = x.to(up)
    return xf.sum(-1).to(out), xf.amax(-1).to(out), xf.amin(-1).to(out), (xf * 0.125 + 1.0).prod(-1).to(out)


def _row_minmax(x, up, out):
    xf = x.to(up)
    return xf.amax(-1).to(out), xf.amin(-1).to(out)


def _sumsq2(x, up, out):
    xf = x.to(up)
    return (xf * xf).sum((-2, -1)).to(out)


def _colsum(x, up, out):
    return (x.to(up) * 0.5).sum(0).to(out)


def _col3(x, up, out):
    xf = x.to(up)
    return xf.sum(0).to(out), xf.amax(0).to(out), xf.amin(0).to(out)


def _col_minmax(x, up, out):
    xf = x.to(up)
    return xf.amax(0).to(out), xf.amin(0).to(out)


def _full_and_col(a, b, up, out):
    y = torch.tanh(a.to(up)) * b.to(up)
    return y.to(out), y.sum(0).to(out)


def _col_amax_epilogue(x, up, out):
    return (x.to(up).abs().amax((0, 1)) * 0.5 + 1.0).to(out)


def _int64_operand(x, m, up, out):
    return (x.to(up) * m.to(up)).to(out)


def _tanh_exp(x, up, out):
    # every output 16-bit for a 16-bit T: the hardware exp / tanh forms
    xf = x.to(up)
    return (torch.tanh(xf) * torch.exp(-xf.abs())).to(out)


def _tanh_exp_mixed(x, up, out):
    # an fp32 output next to the T one: the library exp / tanh
    xf = x.to(up)
    t = torch.tanh(xf)
    return (t * torch.exp(-xf.abs())).to(out), t


# data movement, then only multiplications by 2.0: eager torch is bit-exact in every dtype (two of them after
# a view: a region is formed from two computing prims on, and slice / pad / reshape are none)
def _mv_slice8(x, up, out):
    return x[:, 8:72] * 2.0 * 2.0


def _mv_slice5(x, up, out):
    return x[:, 5:69] * 2.0 * 2.0


def _mv_slice_step(x, up, out):
    return x[:, 1::3] * 2.0 * 2.0


def _mv_cat(a, b, up, out):
    return torch.cat([a, b], -1) * 2.0


def _mv_cat_rows(a, b, up, out):
    return torch.cat([a, b, a], 0) * 2.0


def _mv_pad8(x, up, out):
    return F.pad(x, (8, 8)) * 2.0 * 2.0


def _mv_pad5(x, up, out):
    return F.pad(x, (5, 3)) * 2.0 * 2.0


def _mv_transposed_store(x, up, out):
    return (x * 2.0).t() * 2.0


def _mv_index_select(w, idx, up, out):
    return torch.index_select(w, 0, idx) * 2.0


def _mv_gather(x, idx, up, out):
    return torch.gather(x, 1, idx) * 2.0


def _mv_embedding(ids, w, up, out):
    return F.embedding(ids, w) * 2.0


def _mv_reshape_copy(yt, up, out):
    return yt.reshape(8, 4, 24) * 2.0 * 2.0


def i64(shape, hi, lo=0):
    """An int64 operand with values in [lo, hi)."""
    return ("i64", tuple(shape), lo, hi)


def tr(shape):
    """A floating-point operand of ``shape`` that is the transpose of a contiguous tensor."""
    return ("t", tuple(shape))


class Case:
    def __init__(self, fn, shapes, mode, vec, grid, group, rel_floor=False, kind=None, f32_outs=()):
        self.fn, self.shapes, self.expect, self.group = fn, shapes, (mode, vec, grid), group
        self.rel_floor, self.kind, self.f32_outs = rel_floor, kind, f32_outs  # f32_outs: outputs that stay fp32


PW, SM, RR, LN, COL, MV = "pointwise", "row softmax", "row reduce", "layernorm", "column", "movement"
# name -> function, operand shapes, (mode, vec, grid) of contiguous 16-byte aligned operands
CASES = {
    # pointwise: every vector width, one element, the grid cap (the stride loop wraps)
    "pw_3x1000": Case(_pw, [(3, 1000), (1000,)], "pointwise", 8, (2, 1, 1), PW),
    "pw_5x36": Case(_pw, [(5, 36), (36,)], "pointwise", 4, (1, 1, 1), PW),
    "pw_7x30": Case(_pw, [(7, 30), (30,)], "pointwise", 2, (1, 1, 1), PW),
    "pw_33x7": Case(_pw, [(33, 7), (7,)], "pointwise", 1, (1, 1, 1), PW),
    "pw_1x1": Case(_pw, [(1, 1), (1,)], "pointwise", 1, (1, 1, 1), PW),
    "pw_1031x2049": Case(_pw, [(1031, 2049), (2049,)], "pointwise", 1, (8192, 1, 1), PW),
    "pw_int64_5x40": Case(_int64_operand, [(5, 40), i64((5, 40), 4, -3)], "pointwise", 4, (1, 1, 1), PW),
    "pw_tanh_exp_9x40": Case(_tanh_exp, [(9, 40)], "pointwise", 8, (1, 1, 1), PW),
    "pw_tanh_exp_mixed_9x40": Case(_tanh_exp_mixed, [(9, 40)], "pointwise", 8, (1, 1, 1), PW, f32_outs=(1,)),
    # row mode: softmax (three passes) at every T; rows past the end, a loop tail, W > 1, V = 1
    "sm_257x8": Case(_softmax, [(257, 8), (8,)], "row(T=1)", 8, (2, 1, 1), SM),
    "sm_65x40": Case(_softmax, [(65, 40), (40,)], "row(T=4)", 8, (2, 1, 1), SM),
    "sm_9x264": Case(_softmax, [(9, 264), (264,)], "row(T=32)", 8, (2, 1, 1), SM),
    "sm_5x1000": Case(_softmax, [(5, 1000), (1000,)], "row(T=64)", 8, (2, 1, 1), SM),
    "sm_3x1032": Case(_softmax, [(3, 1032), (1032,)], "row(T=128)", 8, (2, 1, 1), SM),
    "sm_2x2056": Case(_softmax, [(2, 2056), (2056,)], "row(T=256)", 8, (2, 1, 1), SM),
    "sm_3x4104": Case(_softmax, [(3, 4104), (4104,)], "row(T=256)", 8, (3, 1, 1), SM),
    "sm_65x7": Case(_softmax, [(65, 7), (7,)], "row(T=4)", 1, (2, 1, 1), SM),
    "sm_3x33": Case(_softmax, [(3, 33), (33,)], "row(T=32)", 1, (1, 1, 1), SM),
    "sm_5x1": Case(_softmax, [(5, 1), (1,)], "row(T=1)", 1, (1, 1, 1), SM),
    "ln_corr0_2x33x96": Case(_layer_norm(0), [(2, 33, 96), (96,), (96,)], "row(T=8)", 8, (3, 1, 1), LN),
    "ln_corr1_2x33x96": Case(_layer_norm(1), [(2, 33, 96), (96,), (96,)], "row(T=8)", 8, (3, 1, 1), LN),
    "row4_37x50": Case(_row4, [(37, 50)], "row(T=16)", 2, (3, 1, 1), RR, rel_floor=True),
    "row_minmax_37x50": Case(_row_minmax, [(37, 50)], "row(T=16)", 2, (3, 1, 1), RR),
    "sumsq2_5x6x20": Case(_sumsq2, [(5, 6, 20)], "row(T=16)", 4, (1, 1, 1), RR, rel_floor=True),
    # column mode: one split, two, a short last split, masked column tails, scalar partials, idle waves,
    # more splits than 8 x the waves of the last workgroup
    "col_64x512": Case(_colsum, [(64, 512)], "col(S=1)", 8, (1, 1, 1), COL, rel_floor=True),
    "col_65x512": Case(_colsum, [(65, 512)], "col(S=2)", 8, (1, 2, 1), COL, rel_floor=True),
    "col_130x520": Case(_colsum, [(130, 520)], "col(S=3)", 8, (2, 3, 1), COL, rel_floor=True),
    "col_130x1002": Case(_colsum, [(130, 1002)], "col(S=3)", 2, (8, 3, 1), COL, rel_floor=True),
    "col_130x7": Case(_colsum, [(130, 7)], "col(S=3)", 1, (1, 3, 1), COL, rel_floor=True),
    "col_5x24": Case(_colsum, [(5, 24)], "col(S=1)", 8, (1, 1, 1), COL, rel_floor=True),
    "col_1x64": Case(_colsum, [(1, 64)], "col(S=1)", 8, (1, 1, 1), COL, rel_floor=True),
    "col_1000x8": Case(_colsum, [(1000, 8)], "col(S=16)", 8, (1, 16, 1), COL, rel_floor=True),
    "col_4096x4": Case(_colsum, [(4096, 4)], "col(S=64)", 4, (1, 64, 1), COL, rel_floor=True),
    "col3_130x36": Case(_col3, [(130, 36)], "col(S=3)", 4, (1, 3, 1), COL, rel_floor=True),
    "col_minmax_130x36": Case(_col_minmax, [(130, 36)], "col(S=3)", 4, (1, 3, 1), COL),
    "full_and_col_300x200": Case(_full_and_col, [(300, 200), (300, 200)], "col(S=5)", 8, (1, 5, 1), COL, rel_floor=True),
    "col_amax_epilogue_8x17x96": Case(_col_amax_epilogue, [(8, 17, 96)], "col(S=3)", 8, (1, 3, 1), COL),
    # data movement: vector-aligned offsets / piece bounds and misaligned ones
    "mv_slice8": Case(_mv_slice8, [(6, 96)], "pointwise", 8, (1, 1, 1), MV, kind="slice"),
    "mv_slice5": Case(_mv_slice5, [(6, 96)], "pointwise", 8, (1, 1, 1), MV, kind="slice"),
    "mv_slice_step": Case(_mv_slice_step, [(6, 96)], "pointwise", 8, (1, 1, 1), MV, kind="slice"),
    "mv_cat_16_24": Case(_mv_cat, [(6, 16), (6, 24)], "pointwise", 8, (1, 1, 1), MV, kind="cat"),
    "mv_cat_5_11": Case(_mv_cat, [(6, 5), (6, 11)], "pointwise", 8, (1, 1, 1), MV, kind="cat"),
    "mv_cat_rows": Case(_mv_cat_rows, [(6, 16), (3, 16)], "pointwise", 8, (1, 1, 1), MV, kind="cat"),
    "mv_pad8": Case(_mv_pad8, [(6, 16)], "pointwise", 8, (1, 1, 1), MV, kind="pad"),
    "mv_pad5": Case(_mv_pad5, [(6, 16)], "pointwise", 8, (1, 1, 1), MV, kind="pad"),
    "mv_transposed_store": Case(_mv_transposed_store, [(6, 40)], "pointwise", 8, (1, 1, 1), MV),
    "mv_index_select_48": Case(_mv_index_select, [(20, 48), i64((13,), 20)], "pointwise", 4, (1, 1, 1), MV, kind="gather"),
    "mv_index_select_45": Case(_mv_index_select, [(20, 45), i64((13,), 20)], "pointwise", 1, (3, 1, 1), MV, kind="gather"),
    "mv_gather": Case(_mv_gather, [(16, 40), i64((16, 24), 40)], "pointwise", 4, (1, 1, 1), MV, kind="gather"),
    "mv_embedding": Case(_mv_embedding, [i64((4, 9), 20), (20, 48)], "pointwise", 4, (2, 1, 1), MV, kind="gather"),
    "mv_reshape_copy": Case(_mv_reshape_copy, [tr((32, 24))], "pointwise", 8, (1, 1, 1), MV, kind="reshape"),
}
NUMERIC = [n for n, c in CASES.items() if c.group != MV]
MOVEMENT = [n for n, c in CASES.items() if c.group == MV]


def make_inputs(name, T, device):
    """The operands of a case: the same values on every device and, up to their rounding, in every dtype."""
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    args = []
    for s in CASES[name].shapes:
        if s and s[0] == "i64":
            args.append(torch.randint(s[2], s[3], s[1], generator=g).to(device))
        elif s and s[0] == "t":
            args.append(torch.randn(s[1][::-1], generator=g).to(T).to(device).t())
        else:
            args.append(torch.randn(s, generator=g).to(T).to(device))
    return args


def compile_fn(fn, T):
    """``fn`` at compute type fp32 and output type ``T`` through the fusion executor."""
    n = fn.__code__.co_argcount - 2
    if n == 1:
        return thunder.jit(lambda a: fn(a, F32, T), executors=["hipfuse", "torch"])
    if n == 2:
        return thunder.jit(lambda a, b: fn(a, b, F32, T), executors=["hipfuse", "torch"])
    assert n == 3
    return thunder.jit(lambda a, b, c: fn(a, b, c, F32, T), executors=["hipfuse", "torch"])


def as_tuple(x):
    return tuple(x) if isinstance(x, (tuple, list)) else (x,)


def the_region(jf, args):
    """The one fusion region of the last call of ``jf`` and its tensor operands in the region's order."""
    trace = thunder.last_traces(jf)[-1]
    fus = hipfuse.fusions(trace)
    assert len(fus) == 1, f"expected one fusion region, found {len(fus)}:\n{trace}"
    left = [b.sym.name for b in trace.bound_symbols if not b.sym.is_fusion]
    assert all(n in ("python_return", "python_del", "unpack_trivial") for n in left), left
    hf = fus[0]._call_ctx[fus[0].sym.name]
    by_name = {p.name: a for p, a in zip(trace.args, args)}
    return hf, [by_name[hf.inputs[i].name] for i in hf.tensor_pos]


def variant(jf, args):
    """The kernel source ``jf`` ran for ``args`` (the variant of their strides and alignment, already built)."""
    hf, tensors = the_region(jf, args)
    n = len(hf._variants)
    ks = hf._variant(tensors)[1]
    assert len(hf._variants) == n, "the call did not run the variant of these operands"
    return ks


def assert_table(name, ks):
    got = (ks.mode, ks.vec, tuple(ks.grid))
    assert got == CASES[name].expect, f"{name}: the generator chose {got}, the table says {CASES[name].expect}"


# ------------------------------------------------------------------------------------------------
# 1. the shape table on the CPU; every source compiles for gfx950
# ------------------------------------------------------------------------------------------------
@pytest.fixture
def cpu_fusion():
    old = hipfuse.ex.allow_cpu
    hipfuse.ex.allow_cpu = True
    yield
    hipfuse.ex.allow_cpu = old


@pytest.mark.skipif(not os.path.exists(LIB), reason="native library not built")
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_mode_table_and_compile_cpu(name, dtype, cpu_fusion):
    """Each (function, shape) forms one region whose kernel has the mode, vector width and grid of the table,
    and its source compiles.  The reference path of the region (CPU tensors) agrees with the function."""
    case = CASES[name]
    args = make_inputs(name, dtype, "cpu")
    jf = compile_fn(case.fn, dtype)
    outs = as_tuple(jf(*args))
    for o, r in zip(outs, as_tuple(case.fn(*args, F32, dtype))):
        assert o.dtype == r.dtype and o.shape == r.shape
        torch.testing.assert_close(o.float(), r.float(), rtol=2e-2, atol=1e-5)
    hf, tensors = the_region(jf, args)
    if case.kind is not None:
        kinds = {cg._kind(m) for am in hf.plan.arg_maps for m in am.values()}
        assert case.kind in kinds, (name, kinds)
    targs = {hf.inputs[i].name: cg.TensorArg(tuple(t.shape), tuple(t.stride()), t.dtype, True)
             for i, t in zip(hf.tensor_pos, tensors)}
    assert all(isinstance(hf.inputs[i], TensorProxy) for i in hf.tensor_pos)
    ks = cg.generate(hf.plan, hf.inputs, hf.outputs, targs)
    assert_table(name, ks)
    assert len(hipfuse.compile_source(ks)) > 1000


# ------------------------------------------------------------------------------------------------
# 2. numerics on the GPU
# ------------------------------------------------------------------------------------------------
_RUNS: dict = {}


def run_case(name, T):
    """(args, compiled function, outputs, fp64 reference, fp32 evaluation) of a case on the GPU: computed
    once per process and shared (nothing modifies them)."""
    key = (name, T)
    if key not in _RUNS:
        case = CASES[name]
        args = make_inputs(name, T, "cuda")
        jf = compile_fn(case.fn, T)
        outs = as_tuple(jf(*args))
        assert_table(name, variant(jf, args))
        r64 = as_tuple(case.fn(*args, F64, F64))
        r32 = as_tuple(case.fn(*args, F32, F32))
        _RUNS[key] = (args, jf, outs, r64, r32)
    return _RUNS[key]


def check_outputs(name, T, outs, r64, r32, what=None, extra=None):
    case = CASES[name]
    assert len(outs) == len(r64) == len(r32)
    for i, (o, a, b) in enumerate(zip(outs, r64, r32)):
        To = F32 if i in case.f32_outs else T
        assert o.dtype == To, (name, i, o.dtype, To)
        assert_within_finite(o, a.double(), b, To, case.group, f"{what or name} out{i}", rel_floor=case.rel_floor,
                             extra=extra)


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("name", NUMERIC)
def test_numerics_gpu(name, dtype):
    """Every row of the table in every dtype: mode / vec / grid as tabulated, every element within
    ulp(T) |ref64| + 8 e32 + floor."""
    args, jf, outs, r64, r32 = run_case(name, dtype)
    check_outputs(name, dtype, outs, r64, r32)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("name", NUMERIC)
def test_tolerance_is_met_by_fp32_and_sharp_cpu(name, dtype):
    """The plain fp32 evaluation, rounded once to T, stands in for the kernel and passes every case: none relies
    on leniency.  The same evaluation of operands whose last vector (the final 8 elements of the first
    operand's last row: one tail lane of one workgroup) is wrong fails every case but the softmax of one
    element, which is 1 whatever the operand."""
    case = CASES[name]
    args = make_inputs(name, dtype, "cpu")
    r64 = as_tuple(case.fn(*args, F64, F64))
    r32 = as_tuple(case.fn(*args, F32, F32))
    check_outputs(name, dtype, as_tuple(case.fn(*args, F32, dtype)), r64, r32)
    if name == "sm_5x1":
        return
    x = args[0].clone()
    x.view(-1, x.shape[-1])[-1, -8:] = 1000.0
    worst = dict(_WORST)
    try:
        with pytest.raises(AssertionError):
            check_outputs(name, dtype, as_tuple(case.fn(x, *args[1:], F32, dtype)), r64, r32)
    finally:  # the wrong outputs' ratios are no measurement: the record other batteries read stays as it was
        _WORST.clear()
        _WORST.update(worst)


def _edge_row(x):
    """-inf next to finite values (rows 1, 2), a row that is -inf but for one element (3), a constant row (0)."""
    x = x.clone()
    x[0] = 0.75
    x[1, ::3] = float("-inf")
    x[2, -1] = float("-inf")
    x[3] = float("-inf")
    x[3, 5] = 1.5
    return x


def run_edge(name, T, args):
    case = CASES[name]
    jf = compile_fn(case.fn, T)
    outs = as_tuple(jf(*args))
    assert_table(name, variant(jf, args))
    return outs, as_tuple(case.fn(*args, F64, F64)), as_tuple(case.fn(*args, F32, F32))


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16", "fp16"])
def test_softmax_edges_gpu(dtype):
    """Softmax (row mode, T = 32, a tail) of rows that hold -inf but are not all -inf, of a row with one finite
    element and of a constant row; then of arguments of +-80.  There the 16-bit regions' fast exp rounds
    x log2(e): |x| 6e-8 relative per exponential (the comment of ``fast_expf``), so with a = x - max <= 0 and
    p the reference, an element may be off by p (|a| + sum_j p_j |a_j|) 6e-8 more: numerator and denominator."""
    name = "sm_9x264"
    x, b = make_inputs(name, dtype, "cuda")
    b = torch.zeros_like(b)
    outs, r64, r32 = run_edge(name, dtype, [_edge_row(x), b])
    check_outputs(name, dtype, outs, r64, r32, what=f"{name} -inf/constant")
    assert bits_equal(outs[0][3, :5], torch.zeros_like(outs[0][3, :5])) and outs[0][3, 5].item() == 1.0
    g = torch.Generator().manual_seed(5)
    x80 = ((torch.rand(x.shape, generator=g) * 2 - 1) * 80).to(dtype).cuda()
    outs, r64, r32 = run_edge(name, dtype, [x80, b])
    extra = None
    if dtype != F32:
        a = x80.double() - x80.double().amax(-1, keepdim=True)
        extra = r64[0] * (a.abs() + (r64[0] * a.abs()).sum(-1, keepdim=True)) * 6e-8
    check_outputs(name, dtype, outs, r64, r32, what=f"{name} |x|=80", extra=extra)


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("name", ["row_minmax_37x50", "col_minmax_130x36"])
def test_amax_amin_edges_gpu(name, dtype):
    """amax / amin over rows (row mode) and over columns (column mode, three splits): -inf next to finite
    values, an all-but-one -inf line, a constant line; then one NaN, which torch and the kernels propagate:
    the NaN and -inf positions equal the reference's, the finite remainder is within tolerance."""
    (x,) = make_inputs(name, dtype, "cuda")
    col = name.startswith("col")
    e = _edge_row(x.t() if col else x)
    e = e.t().contiguous() if col else e
    outs, r64, r32 = run_edge(name, dtype, [e])
    check_outputs(name, dtype, outs, r64, r32, what=f"{name} -inf/constant")
    n = x.clone()
    n[17, 21] = float("nan")
    outs, r64, r32 = run_edge(name, dtype, [n])
    assert int(torch.isnan(r64[0]).sum()) == 1 and int(torch.isnan(r64[1]).sum()) == 1
    check_outputs(name, dtype, outs, r64, r32, what=f"{name} NaN")


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16", "fp16"])
def test_layer_norm_constant_row_gpu(dtype):
    """var_mean of a constant row: the variance is exactly zero and the output is the bias."""
    name = "ln_corr1_2x33x96"
    x, w, b = make_inputs(name, dtype, "cuda")
    x = x.clone()
    x[1, 7] = -1.25
    outs, r64, r32 = run_edge(name, dtype, [x, w, b])
    check_outputs(name, dtype, outs, r64, r32, what=f"{name} constant row")
    assert bits_equal(outs[0][1, 7], b)


# ------------------------------------------------------------------------------------------------
# 3. operand layouts
# ------------------------------------------------------------------------------------------------
def _transposed(t):
    return t.t().contiguous().t()


LAYOUTS = [("padded pitch", nan_padded), ("address % 16 != 0", offset_by_one), ("odd pitch", odd_pitch),
           ("transposed", _transposed)]


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("name", ["pw_3x1000", "pw_7x30", "sm_5x1000", "row4_37x50", "col_130x520", "col_130x1002"])
def test_operand_layouts_gpu(name, dtype):
    """The first operand of a V = 8 and a V = 2 case of every mode through (b) a NaN-padded wider pitch with
    extra rows, (c) a view one element into its buffer, (d) the leading columns of a base one element wider
    and (e, pointwise) a transposed tensor.  Every layout is a variant of its own; (c) and (d) cannot use
    the 16-byte loads, so their source differs from the contiguous one; the outputs have the bits of the
    contiguous run (only the loads differ), so nothing outside the operand was consumed."""
    args, jf, outs, _, _ = run_case(name, dtype)
    assert all(bits_equal(o, c) for o, c in zip(as_tuple(jf(*args)), outs))
    seen = {id(variant(jf, args)): "contiguous"}
    src = variant(jf, args).src
    for what, lay in LAYOUTS:
        if what == "transposed" and not name.startswith("pw"):
            continue
        x = lay(args[0])
        assert torch.equal(x, args[0]) and (x.stride() != args[0].stride() or x.data_ptr() % 16 != 0)
        largs = [x] + args[1:]
        louts = as_tuple(jf(*largs))
        ks = variant(jf, largs)
        assert id(ks) not in seen, f"{name} {what}: ran the variant of {seen.get(id(ks))}"
        seen[id(ks)] = what
        assert (ks.mode, ks.vec) == CASES[name].expect[:2]
        if what in ("address % 16 != 0", "odd pitch"):
            assert ks.src != src, f"{name} {what}: the source of the aligned contiguous operand"
        for i, (o, c) in enumerate(zip(louts, outs)):
            assert not torch.isnan(o).any(), f"{name} {what} out{i}: NaN (padding was consumed)"
            assert bits_equal(o, c), f"{name} {what} out{i}: differs from the contiguous run"


# ------------------------------------------------------------------------------------------------
# 4. data movement against an exact oracle
# ------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("name", MOVEMENT)
def test_data_movement_exact_gpu(name, dtype):
    """Slices, concatenations, pads, a transposed store, indexed loads and a copying reshape at aligned and
    misaligned positions, followed only by multiplications by 2.0: the bits of eager torch."""
    case = CASES[name]
    args = make_inputs(name, dtype, "cuda")
    jf = compile_fn(case.fn, dtype)
    out = jf(*args)
    assert_table(name, variant(jf, args))
    ref = case.fn(*args, F32, dtype)
    assert out.shape == ref.shape and out.dtype == ref.dtype == dtype
    assert bits_equal(out, ref), f"{name}: {(out != ref).sum().item()} of {out.numel()} elements differ"


# ------------------------------------------------------------------------------------------------
# 5. the column hand-off
# ------------------------------------------------------------------------------------------------
HANDOFF_A, HANDOFF_B = "col_130x1002", "col_1000x8"  # 8 column groups of 3 splits; 1 group of 16


@gpu
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_column_handoff_repeat_interleave_graph_gpu(dtype):
    """Two column kernels with different numbers of column groups share the arrival counters of their stream:
    repeated and interleaved (A, B, A, B) launches give the bits each gives alone (fixed combine order, every
    launch leaves the counters at zero), and so does a captured graph of A then B, replayed twice."""
    xa, fa, oa, _, _ = run_case(HANDOFF_A, dtype)
    xb, fb, ob, _, _ = run_case(HANDOFF_B, dtype)
    assert variant(fa, xa).counters == 8 and variant(fb, xb).counters == 1
    for _ in range(3):
        assert bits_equal(fa(*xa), oa[0])
    for _ in range(3):
        assert bits_equal(fb(*xb), ob[0])
    for _ in range(2):
        ra, rb = fa(*xa), fb(*xb)
        assert bits_equal(ra, oa[0]) and bits_equal(rb, ob[0])
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fa(*xa), fb(*xb)  # counters / kernels of the capture stream exist before the capture
        with torch.cuda.graph(g, stream=s):
            ga, gb = fa(*xa), fb(*xb)
    torch.cuda.current_stream().wait_stream(s)
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        assert bits_equal(ga, oa[0]) and bits_equal(gb, ob[0])


@gpu
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("name", ["col_130x520", "col_130x1002", "full_and_col_300x200"])
@pytest.mark.parametrize("sync", ["fence", "twopass"])
def test_column_sync_variants_gpu(sync, name, dtype, monkeypatch):
    """``LTA_HIPFUSE_COL_SYNC=fence`` hands the partials over with ``__threadfence`` in place of the coherent
    memory operations: same grid, same combine order, so the bits of the default.  ``twopass`` is a second
    builder: two launches, workgroups of 4 waves and splits of its own (>= 32 rows each, up to 512 workgroups),
    so its sums associate differently and are held to the fp64 tolerance only; the elementwise full-domain
    output of ``full_and_col`` has the default's bits there too."""
    args, _, outs, r64, r32 = run_case(name, dtype)
    monkeypatch.setattr(cg, "COL_SYNC", sync)
    jf = compile_fn(CASES[name].fn, dtype)
    souts = as_tuple(jf(*args))
    ks = variant(jf, args)
    assert ks.mode.startswith("col") and ks.grid[1] > 1 and ks.vec == CASES[name].expect[1]
    assert bool(ks.extra) == (sync == "twopass") and bool(ks.counters) == (sync == "fence")
    check_outputs(name, dtype, souts, r64, r32, what=f"{name} {sync}")
    for i, (o, c) in enumerate(zip(souts, outs)):
        if sync == "fence" or (name.startswith("full_and_col") and i == 0):
            assert bits_equal(o, c), f"{name} {sync} out{i}: differs from the coherent hand-off"
    assert bits_equal(as_tuple(jf(*args))[-1], souts[-1])
