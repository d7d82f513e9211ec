"""The trace rewrites of ``hipex._post_claim``, pinned at the pass level on hand-built traces.

Every case builds a small program of bound symbols over symbolic proxies (no GPU, no kernels), runs
``hipex._post_claim`` and compares the whole resulting program: operator names, argument names and
literals, output names, and the provenance of the last pass that rewrote it.  A refusal is a program
that comes back as the same object (or, where another pass still applies, with only that rewrite).
"""
import pytest
import torch

import lightning_thunder_amd as thunder
from lightning_thunder_amd import torch as lt
from lightning_thunder_amd.core import prims
from lightning_thunder_amd.core.proxies import Proxy, TensorProxy
from lightning_thunder_amd.core.trace import TraceCtx, tracectx
from lightning_thunder_amd.executors import hipex
from lightning_thunder_amd.transforms.inplace_index_copy import index_copy_inplace

BF16, U8, F32, I64, I32 = torch.bfloat16, torch.uint8, torch.float32, torch.int64, torch.int32
K, N = 256, 512


def _fmt(v):
    if isinstance(v, Proxy):
        return v.name
    if isinstance(v, tuple):
        return "(" + ", ".join(_fmt(x) for x in v) + ")"
    if isinstance(v, list):
        return "[" + ", ".join(_fmt(x) for x in v) + "]"
    return repr(v)


def _line(b):
    call = ", ".join([_fmt(a) for a in b.args] + [f"{k}={_fmt(v)}" for k, v in b.kwargs.items()])
    outs = b.output if isinstance(b.output, (tuple, list)) else (b.output,)
    lhs = ", ".join(_fmt(o) for o in outs) + " = " if b.output is not None else ""
    return f"{lhs}{b.sym.name}({call})"


class Program:
    """A trace under construction: ``t`` declares a tensor, calling the object appends ``sym(*args)``."""

    def __init__(self):
        self.trace = TraceCtx()

    def t(self, name, *shape, dtype=BF16, device="cuda", requires_grad=False):
        with tracectx(self.trace):
            return TensorProxy(name=name, shape=shape, device=device, dtype=dtype, requires_grad=requires_grad)

    def ts(self, names, *shape, **kw):
        return tuple(self.t(n, *shape, **kw) for n in names.split())

    def __call__(self, sym, *args, out, **kwargs):
        self.trace.bound_symbols.append(sym.bind(*args, output=out, **kwargs))
        return out

    def run(self, *outs):
        """Returns ``(rewritten program as lines without the return, provenance or None)``."""
        self.trace.bound_symbols.append(prims.python_return.bind(*outs, output=None))
        before = [_line(b) for b in self.trace.bound_symbols]
        new = hipex._post_claim(self.trace)
        assert [_line(b) for b in self.trace.bound_symbols] == before, "the input trace was modified"
        lines = [_line(b) for b in new.bound_symbols]
        assert lines[-1] == before[-1]
        if new is self.trace:
            return None, None
        assert new.scopes == [new.bound_symbols] and new.names == self.trace.names
        assert all(b._call_ctx for b in new.bound_symbols if b.sym.name.startswith("hip_") and b not in self.trace.bound_symbols)
        return lines[:-1], str(new.get_provenance().pss)


def unchanged(result):
    assert result == (None, None), result


# ------------------------------------------------------------------------------------------------
# the two decode weight kinds
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mxfp4_sym():
    from lightning_thunder_amd.transforms.mxfp4_inference import MXFP4InferenceTransform

    m = torch.nn.Sequential(torch.nn.Linear(64, 32))
    m.requires_grad_(False)
    jm = thunder.jit(m, transforms=[MXFP4InferenceTransform()])
    jm(torch.randn(2, 64))
    (sym,) = {b.sym for b in thunder.last_traces(jm)[-1].bound_symbols if b.sym.id in hipex._MXFP4_LINEAR_IDS}
    return sym


class Bf16:
    name = "bf16"
    norm_rows = 8

    def weight(self, p, tag, n=N, k=K):
        return (p.t(tag, n, k),)

    def proj(self, p, x, w, out, bias=None):
        return p(hipex.hip_linear, x, *w, bias, out=out)

    def w(self, tag):
        return tag

    def lowered(self, x, tag, out, bias="None"):  # a candidate no fold took
        return f"{out} = hip_linear({x}, {tag}, {bias})"

    def fused(self, x, tag, out, bias="None", residual="None", act="None", gate=None, norm=False, g="None", eps="1e-05"):
        return (f"{out} = hip_decode_linear({x}, {tag}, {bias}, {residual}, {act}, {gate}, {norm}, {g}, {eps})")

    def group(self, x, tags, outs, norm=False, g="None", eps="1e-05", packed=False):
        ws = "(" + ", ".join(tags) + ")"
        return f"{outs} = hip_decode_linear_group({x}, {ws}, {norm}, {g}, {eps}{', True' if packed else ''})"

    def provenance(self, gated=0, act=0, res=0, norm=0):
        return f"hipex: decode GEMV fusion ({gated} gated pair(s), {norm} norm prologue(s))"

    def group_provenance(self, n, **folds):
        return f"hipex: {n} grouped decode projection launch(es)"


class Mxfp4:
    name = "mxfp4"
    norm_rows = 1

    def __init__(self, sym):
        self.sym = sym

    def weight(self, p, tag, n=N, k=K):
        return p.t(tag + "_q", n, k // 2, dtype=U8), p.t(tag + "_s", n, k // 32, dtype=U8)

    def proj(self, p, x, w, out, bias=None):
        return p(self.sym, x, *w, bias, False, out=out)

    def w(self, tag):
        return f"{tag}_q, {tag}_s"

    def lowered(self, x, tag, out, bias="None"):
        return self.fused(x, tag, out, bias=bias)

    def fused(self, x, tag, out, bias="None", residual="None", act="None", gate=None, norm=False, g="None", eps="1e-05"):
        gate = "None, None" if gate is None else self.w(gate)
        return (f"{out} = hip_mxfp4_decode_linear({x}, {self.w(tag)}, {bias}, {residual}, {act}, {gate}, {norm}, {g}, "
                f"{eps})")

    def group(self, x, tags, outs, norm=False, g="None", eps="1e-05", packed=False):
        ws = "(" + ", ".join(f"({self.w(t)})" for t in tags) + ")"
        return f"{outs} = hip_mxfp4_decode_linear_group({x}, {ws}, {norm}, {g}, {eps}{', True' if packed else ''})"

    def provenance(self, gated=0, act=0, res=0, norm=0, group=0):
        return (f"hipex: MXFP4 decode GEMV fusion ({gated} gated pair(s), {act} activation(s), {res} residual(s), "
                f"{norm} norm prologue(s), {group} group(s))")

    def group_provenance(self, n, **folds):
        return self.provenance(group=n, **folds)


@pytest.fixture(params=["bf16", "mxfp4"])
def kind(request, mxfp4_sym):
    return Bf16() if request.param == "bf16" else Mxfp4(mxfp4_sym)


def _pair(p, kind, rows=1, x2=False, n2=N, bias=None):
    """``a = proj(x, w1[, bias]); b = proj(x or x2, w2)``."""
    x = p.t("x", rows, K)
    xb = p.t("x2", rows, K) if x2 else x
    a, b, y = p.ts("a b y", rows, N)
    kind.proj(p, x, kind.weight(p, "w1"), a, bias)
    kind.proj(p, xb, kind.weight(p, "w2", n2), b)
    return x, a, b, y


# ------------------------------------------------------------------------------------------------
# decode: the gated pair
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 2, 8])
def test_decode_swiglu_pair(kind, rows):
    p = Program()
    x, a, b, y = _pair(p, kind, rows)
    p(hipex.hip_swiglu, a, b, out=y)
    assert p.run(y) == ([kind.fused("x", "w1", "y", act="'silu'", gate="w2")], kind.provenance(gated=1))


@pytest.mark.parametrize("silu_first", [True, False])
@pytest.mark.parametrize("silu_args", [(), (False,)])
def test_decode_mul_silu_pair(kind, silu_first, silu_args):
    p = Program()
    x, a, b, y = _pair(p, kind)
    s = p.t("s", 1, N)
    p(lt.silu, a, *silu_args, out=s)
    p(lt.mul, *((s, b) if silu_first else (b, s)), out=y)
    assert p.run(y) == ([kind.fused("x", "w1", "y", act="'silu'", gate="w2")], kind.provenance(gated=1))


def _torch_op(name):
    from lightning_thunder_amd.executors import torchex

    return torchex.ex.opmap[name]


def test_decode_mul_silu_pair_claimed_by_the_torch_executor(kind):
    """The bf16 pass matches ``mul`` / ``silu`` only under their ltorch names, the MXFP4 pass under the torch
    executor's names as well (pinned as found; the packed ``cat`` is matched under both by both)."""
    p = Program()
    x, a, b, y = _pair(p, kind)
    s = p.t("s", 1, N)
    p(_torch_op("torch_silu"), a, out=s)
    p(_torch_op("torch_mul"), s, b, out=y)
    if kind.name == "bf16":
        assert p.run(y) == ([kind.group("x", ["w1", "w2"], "a, b"), "s = torch_silu(a)", "y = torch_mul(s, b)"],
                            kind.group_provenance(1))
    else:
        assert p.run(y) == ([kind.fused("x", "w1", "y", act="'silu'", gate="w2")], kind.provenance(gated=1))


def test_decode_packed_cat_claimed_by_the_torch_executor(kind):
    p = Program()
    x, outs = _siblings(p, kind, 2)
    c = p.t("c", 1, 2 * N)
    p(_torch_op("torch_cat"), outs, -1, out=c)
    assert p.run(c) == ([kind.group("x", ["w0", "w1"], "c", packed=True)], kind.group_provenance(1))


def test_decode_mul_silu_inplace_refused(kind):
    p = Program()
    x, a, b, y = _pair(p, kind)
    s = p.t("s", 1, N)
    p(lt.silu, a, True, out=s)
    p(lt.mul, s, b, out=y)
    assert p.run(y) == ([kind.group("x", ["w1", "w2"], "a, b"), "s = silu(a, True)", "y = mul(s, b)"],
                        kind.group_provenance(1))


def test_decode_pair_refused_a_read_twice(kind):
    p = Program()
    x, a, b, y = _pair(p, kind)
    z = p.t("z", 1, N)
    p(hipex.hip_swiglu, a, b, out=y)
    p(lt.silu, a, out=z)
    # the pair stays; the two projections are still siblings of one x
    assert p.run(y, z) == ([kind.group("x", ["w1", "w2"], "a, b"), "y = hip_swiglu(a, b)", "z = silu(a)"],
                           kind.group_provenance(1))


def test_decode_pair_refused_value_returned(kind):
    p = Program()
    x, a, b, y = _pair(p, kind)
    p(hipex.hip_swiglu, a, b, out=y)
    assert p.run(y, a) == ([kind.group("x", ["w1", "w2"], "a, b"), "y = hip_swiglu(a, b)"], kind.group_provenance(1))


def test_decode_pair_refused_different_x(kind):
    p = Program()
    x, a, b, y = _pair(p, kind, x2=True)
    p(hipex.hip_swiglu, a, b, out=y)
    result = p.run(y)
    if kind.name == "bf16":
        unchanged(result)
    else:  # each candidate is still lowered on its own
        assert result == ([kind.lowered("x", "w1", "a"), kind.lowered("x2", "w2", "b"), "y = hip_swiglu(a, b)"],
                          kind.provenance())


def test_decode_pair_refused_different_weight_shapes(kind):
    p = Program()
    x, a, b, y = _pair(p, kind, n2=N // 2)
    p(hipex.hip_swiglu, a, b, out=y)
    assert p.run(y) == ([kind.group("x", ["w1", "w2"], "a, b"), "y = hip_swiglu(a, b)"], kind.group_provenance(1))


def test_decode_pair_refused_nine_rows(kind):
    p = Program()
    x, a, b, y = _pair(p, kind, rows=9)
    p(hipex.hip_swiglu, a, b, out=y)
    unchanged(p.run(y))


def test_decode_pair_refused_member_with_bias(kind):
    p = Program()
    bias = p.t("bias", N)
    x, a, b, y = _pair(p, kind, bias=bias)
    p(hipex.hip_swiglu, a, b, out=y)
    result = p.run(y)
    if kind.name == "bf16":
        unchanged(result)
    else:
        assert result == ([kind.lowered("x", "w1", "a", bias="bias"), kind.lowered("x", "w2", "b"), "y = hip_swiglu(a, b)"],
                          kind.provenance())


@pytest.mark.parametrize("extra", ["residual", "act"])
def test_bf16_pair_refused_member_with_residual_or_act(extra):
    p = Program()
    x, r = p.t("x", 1, K), p.t("r", 1, N)
    w1, w2 = p.ts("w1 w2", N, K)
    a, b, y = p.ts("a b y", 1, N)
    p(hipex.hip_linear, x, w1, None, *((r,) if extra == "residual" else (None, "silu")), out=a)
    p(hipex.hip_linear, x, w2, None, out=b)
    p(hipex.hip_swiglu, a, b, out=y)
    unchanged(p.run(y))


def test_bf16_pair_reads_operands_by_keyword():
    p = Program()
    x = p.t("x", 1, K)
    w1, w2 = p.ts("w1 w2", N, K)
    a, b, y = p.ts("a b y", 1, N)
    p(hipex.hip_linear, x, w1, bias=None, out=a)
    p(hipex.hip_linear, x, w2, out=b)
    p(hipex.hip_swiglu, a, b, out=y)
    assert p.run(y) == ([Bf16().fused("x", "w1", "y", act="'silu'", gate="w2")], Bf16().provenance(gated=1))


# ------------------------------------------------------------------------------------------------
# decode: the RMSNorm prologue
# ------------------------------------------------------------------------------------------------
def _norm(p, rows, eps=1e-6):
    x, g = p.t("x", rows, K), p.t("g", K)
    h, rstd = p.t("h", rows, K), p.t("rstd", rows, dtype=F32)
    p(hipex.hip_rms_norm_fwd, x, g, eps, out=(h, rstd))
    return x, h, rstd


def test_decode_norm_into_projection(kind):
    p = Program()
    x, h, rstd = _norm(p, kind.norm_rows)
    bias, o = p.t("bias", N), p.t("o", kind.norm_rows, N)
    kind.proj(p, h, kind.weight(p, "w1"), o, bias)
    assert p.run(o) == ([kind.fused("x", "w1", "o", bias="bias", norm=True, g="g", eps="1e-06")],
                        kind.provenance(norm=1))


def test_bf16_norm_keeps_bias_residual_act_of_its_consumers():
    p = Program()
    x, h, rstd = _norm(p, 8)
    bias, r = p.t("bias", N), p.t("r", 8, N)
    w1, w2, w3 = p.ts("w1 w2 w3", N, K)
    o1, o2, o3 = p.ts("o1 o2 o3", 8, N)
    p(hipex.hip_linear, h, w1, bias, out=o1)
    p(hipex.hip_linear, h, w2, None, r, out=o2)
    p(hipex.hip_linear, h, w3, None, None, "silu", out=o3)
    k = Bf16()
    assert p.run(o1, o2, o3) == ([k.fused("x", "w1", "o1", bias="bias", norm=True, g="g", eps="1e-06"),
                                  k.fused("x", "w2", "o2", residual="r", norm=True, g="g", eps="1e-06"),
                                  k.fused("x", "w3", "o3", act="'silu'", norm=True, g="g", eps="1e-06")],
                                 k.provenance(norm=1))


def test_decode_norm_into_gated_pair(kind):
    p = Program()
    rows = kind.norm_rows
    x, h, rstd = _norm(p, rows, eps=1)
    a, b, y = p.ts("a b y", rows, N)
    kind.proj(p, h, kind.weight(p, "w1"), a)
    kind.proj(p, h, kind.weight(p, "w2"), b)
    p(hipex.hip_swiglu, a, b, out=y)
    assert p.run(y) == ([kind.fused("x", "w1", "y", act="'silu'", gate="w2", norm=True, g="g", eps="1.0")],
                        kind.provenance(gated=1, norm=1))


def _norm_refusal(p, kind, result, rest, lowered_bias="None"):
    """The norm stays; MXFP4 still lowers the projection ``o = proj(h, w1)``, bf16 leaves everything."""
    if kind.name == "bf16":
        unchanged(result)
    else:
        assert result == (["h, rstd = hip_rms_norm_fwd(x, g, 1e-06)", kind.lowered("h", "w1", "o", bias=lowered_bias)] + rest,
                          kind.provenance())


def test_decode_norm_refused_rstd_read(kind):
    p = Program()
    x, h, rstd = _norm(p, 1)
    o = p.t("o", 1, N)
    kind.proj(p, h, kind.weight(p, "w1"), o)
    _norm_refusal(p, kind, p.run(o, rstd), [])


def test_decode_norm_refused_other_consumer(kind):
    p = Program()
    x, h, rstd = _norm(p, 1)
    o, z = p.t("o", 1, N), p.t("z", 1, K)
    kind.proj(p, h, kind.weight(p, "w1"), o)
    p(lt.silu, h, out=z)
    _norm_refusal(p, kind, p.run(o, z), ["z = silu(h)"])


def test_decode_norm_refused_y_returned(kind):
    p = Program()
    x, h, rstd = _norm(p, 1)
    o = p.t("o", 1, N)
    kind.proj(p, h, kind.weight(p, "w1"), o)
    _norm_refusal(p, kind, p.run(o, h), [])


def test_bf16_norm_refused_y_used_as_weight():
    p = Program()
    x, h, rstd = _norm(p, 1)
    o = p.t("o", 1, 1)
    p(hipex.hip_linear, h, h, None, out=o)
    unchanged(p.run(o))


def test_mxfp4_norm_refused_y_used_as_other_operand(mxfp4_sym):
    kind = Mxfp4(mxfp4_sym)
    p = Program()
    x, g = p.t("x", 1, K), p.t("g", K)
    h, rstd = p.t("h", 1, K), p.t("rstd", 1, dtype=F32)
    p(hipex.hip_rms_norm_fwd, x, g, 1e-6, out=(h, rstd))
    o = p.t("o", 1, K)
    kind.proj(p, h, kind.weight(p, "w1", K), o, h)
    _norm_refusal(p, kind, p.run(o), [], lowered_bias="h")


def test_decode_norm_refused_nine_rows(kind):
    p = Program()
    x, h, rstd = _norm(p, 9)
    o = p.t("o", 9, N)
    kind.proj(p, h, kind.weight(p, "w1"), o)
    unchanged(p.run(o))


def test_decode_norm_refused_non_literal_eps(kind):
    p = Program()
    x, g, eps = p.t("x", 1, K), p.t("g", K), p.t("eps", dtype=F32)
    h, rstd, o = p.t("h", 1, K), p.t("rstd", 1, dtype=F32), p.t("o", 1, N)
    p(hipex.hip_rms_norm_fwd, x, g, eps, out=(h, rstd))
    kind.proj(p, h, kind.weight(p, "w1"), o)
    result = p.run(o)
    if kind.name == "bf16":
        unchanged(result)
    else:
        assert result == (["h, rstd = hip_rms_norm_fwd(x, g, eps)", kind.lowered("h", "w1", "o")], kind.provenance())


@pytest.mark.parametrize("rows", [2, 8])
def test_mxfp4_norm_cap_of_one_row(mxfp4_sym, rows):
    kind = Mxfp4(mxfp4_sym)
    p = Program()
    x, h, rstd = _norm(p, rows)
    o = p.t("o", rows, N)
    kind.proj(p, h, kind.weight(p, "w1"), o)
    _norm_refusal(p, kind, p.run(o), [])


# ------------------------------------------------------------------------------------------------
# decode: sibling projections
# ------------------------------------------------------------------------------------------------
def _siblings(p, kind, n, shape=(1, K)):
    x = p.t("x", *shape)
    outs = [p.t(f"p{i}", *shape[:-1], N) for i in range(n)]
    for i, o in enumerate(outs):
        kind.proj(p, x, kind.weight(p, f"w{i}"), o)
    return x, outs


@pytest.mark.parametrize("n,expect", [(2, [(0, 1)]), (3, [(0, 1, 2)]), (4, [(0, 1, 2), (3,)]), (5, [(0, 1, 2), (3, 4)])])
def test_decode_groups_of_siblings(kind, n, expect):
    p = Program()
    x, outs = _siblings(p, kind, n)
    lines = [kind.group("x", [f"w{i}" for i in c], ", ".join(f"p{i}" for i in c)) if len(c) > 1
             else kind.lowered("x", f"w{c[0]}", f"p{c[0]}") for c in expect]
    assert p.run(*outs) == (lines, kind.group_provenance(sum(len(c) > 1 for c in expect)))


def test_decode_single_projection_is_not_grouped(kind):
    p = Program()
    x, outs = _siblings(p, kind, 1)
    result = p.run(*outs)
    if kind.name == "bf16":
        unchanged(result)
    else:
        assert result == ([kind.lowered("x", "w0", "p0")], kind.provenance())


def test_decode_differing_norm_keys_are_not_grouped(kind):
    p = Program()
    x, g1, g2 = p.t("x", 1, K), p.t("g1", K), p.t("g2", K)
    h1, h2 = p.ts("h1 h2", 1, K)
    r1, r2 = p.ts("r1 r2", 1, dtype=F32)
    o1, o2, o3, o4 = p.ts("o1 o2 o3 o4", 1, N)
    p(hipex.hip_rms_norm_fwd, x, g1, 1e-6, out=(h1, r1))
    p(hipex.hip_rms_norm_fwd, x, g2, 1e-6, out=(h2, r2))
    kind.proj(p, h1, kind.weight(p, "w1"), o1)
    kind.proj(p, h2, kind.weight(p, "w2"), o2)
    kind.proj(p, x, kind.weight(p, "w3"), o3)
    kind.proj(p, h1, kind.weight(p, "w4"), o4)
    norm = dict(norm=True, eps="1e-06")
    assert p.run(o1, o2, o3, o4) == (
        [kind.group("x", ["w1", "w4"], "o1, o4", g="g1", **norm), kind.fused("x", "w2", "o2", g="g2", **norm),
         kind.lowered("x", "w3", "o3")],
        kind.group_provenance(1, norm=2))


@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("dim", [-1, 2])
def test_decode_packed_cat(kind, n, dim):
    p = Program()
    x, outs = _siblings(p, kind, n, shape=(1, 1, K))
    c = p.t("c", 1, 1, n * N)
    p(lt.cat, outs, dim, out=c)
    assert p.run(c) == ([kind.group("x", [f"w{i}" for i in range(n)], "c", packed=True)], kind.group_provenance(1))


def test_decode_packed_cat_with_dim_keyword_and_norm(kind):
    p = Program()
    x, g = p.t("x", 1, 1, K), p.t("g", K)
    h, rstd = p.t("h", 1, 1, K), p.t("rstd", 1, dtype=F32)
    p(hipex.hip_rms_norm_fwd, x, g, 1e-5, out=(h, rstd))
    p0, p1 = p.ts("p0 p1", 1, 1, N)
    kind.proj(p, h, kind.weight(p, "w0"), p0)
    kind.proj(p, h, kind.weight(p, "w1"), p1)
    c = p.t("c", 1, 1, 2 * N)
    p(lt.cat, [p0, p1], dim=-1, out=c)
    assert p.run(c) == ([kind.group("x", ["w0", "w1"], "c", norm=True, g="g", packed=True)],
                        kind.group_provenance(1, norm=1))


def test_decode_cat_on_another_dim_is_not_packed(kind):
    p = Program()
    x, outs = _siblings(p, kind, 2, shape=(1, 1, K))
    c = p.t("c", 1, 2, N)
    p(lt.cat, outs, 1, out=c)
    assert p.run(c) == ([kind.group("x", ["w0", "w1"], "p0, p1"), "c = cat([p0, p1], 1)"], kind.group_provenance(1))


def test_decode_cat_of_four_is_not_packed(kind):
    p = Program()
    x, outs = _siblings(p, kind, 4, shape=(1, 1, K))
    c = p.t("c", 1, 1, 4 * N)
    p(lt.cat, outs, -1, out=c)
    assert p.run(c) == ([kind.group("x", ["w0", "w1", "w2"], "p0, p1, p2"), kind.lowered("x", "w3", "p3"),
                         "c = cat([p0, p1, p2, p3], -1)"], kind.group_provenance(1))


def test_decode_cat_part_read_twice_is_not_packed(kind):
    p = Program()
    x, outs = _siblings(p, kind, 2, shape=(1, 1, K))
    c, z = p.t("c", 1, 1, 2 * N), p.t("z", 1, 1, N)
    p(lt.cat, outs, -1, out=c)
    p(lt.silu, outs[0], out=z) if kind.name == "bf16" else p(lt.mul, outs[0], outs[0], out=z)
    tail = "z = silu(p0)" if kind.name == "bf16" else "z = mul(p0, p0)"
    assert p.run(c, z) == ([kind.group("x", ["w0", "w1"], "p0, p1"), "c = cat([p0, p1], -1)", tail],
                           kind.group_provenance(1))


def test_decode_packed_cat_leaves_other_siblings_grouped(kind):
    p = Program()
    x, outs = _siblings(p, kind, 4, shape=(1, 1, K))
    c = p.t("c", 1, 1, 2 * N)
    p(lt.cat, [outs[1], outs[2]], -1, out=c)
    assert p.run(c, outs[0], outs[3]) == (
        [kind.group("x", ["w0", "w3"], "p0, p3"), kind.group("x", ["w1", "w2"], "c", packed=True)],
        kind.group_provenance(2))


# ------------------------------------------------------------------------------------------------
# decode: what only the MXFP4 pass folds, and what it leaves alone
# ------------------------------------------------------------------------------------------------
@pytest.fixture
def mx(mxfp4_sym):
    return Mxfp4(mxfp4_sym)


def test_mxfp4_silu_becomes_act(mx):
    p = Program()
    x, a, y = p.t("x", 2, K), p.t("a", 2, N), p.t("y", 2, N)
    mx.proj(p, x, mx.weight(p, "w1"), a)
    p(lt.silu, a, out=y)
    assert p.run(y) == ([mx.fused("x", "w1", "y", act="'silu'")], mx.provenance(act=1))


@pytest.mark.parametrize("claimed", [False, True])
@pytest.mark.parametrize("op_first", [True, False])
def test_mxfp4_residual_is_emitted_at_the_add(mx, op_first, claimed):
    add = _torch_op("torch_add") if claimed else lt.add
    p = Program()
    x, x0, a, r, y = p.t("x", 2, K), p.t("x0", 2, N), p.t("a", 2, N), p.t("r", 2, N), p.t("y", 2, N)
    bias = p.t("bias", N)
    mx.proj(p, x, mx.weight(p, "w1"), a, bias)
    p(lt.silu, x0, out=r)  # the residual is produced after the projection
    p(add, *((a, r) if op_first else (r, a)), out=y)
    assert p.run(y) == (["r = silu(x0)", mx.fused("x", "w1", "y", bias="bias", residual="r")], mx.provenance(res=1))


def test_mxfp4_silu_then_residual(mx):
    p = Program()
    x, a, s, r, y = p.t("x", 1, K), p.t("a", 1, N), p.t("s", 1, N), p.t("r", 1, N), p.t("y", 1, N)
    mx.proj(p, x, mx.weight(p, "w1"), a)
    p(lt.silu, a, out=s)
    p(lt.add, s, r, out=y)
    assert p.run(y) == ([mx.fused("x", "w1", "y", residual="r", act="'silu'")], mx.provenance(act=1, res=1))


def test_mxfp4_residual_refusals(mx):
    p = Program()
    x, r = p.t("x", 1, K), p.t("r", 1, N)
    a, b, y1, y2, y3 = p.ts("a b y1 y2 y3", 1, N)
    wide = p.t("wide", 2, N)
    mx.proj(p, x, mx.weight(p, "w1"), a)
    mx.proj(p, x, mx.weight(p, "w2"), b)
    p(lt.add, a, r, alpha=2, out=y1)
    p(lt.add, b, b, out=y2)
    p(lt.add, y1, wide, out=y3)
    assert p.run(y2, y3) == ([mx.group("x", ["w1", "w2"], "a, b"), "y1 = add(a, r, alpha=2)", "y2 = add(b, b)",
                              "y3 = add(y1, wide)"], mx.provenance(group=1))


def test_mxfp4_gated_pair_takes_no_residual_or_act(mx):
    p = Program()
    x, r = p.t("x", 1, K), p.t("r", 1, N)
    a, b, y, s, z = p.ts("a b y s z", 1, N)
    mx.proj(p, x, mx.weight(p, "w1"), a)
    mx.proj(p, x, mx.weight(p, "w2"), b)
    p(hipex.hip_swiglu, a, b, out=y)
    p(lt.silu, y, out=s)
    p(lt.add, s, r, out=z)
    assert p.run(z) == ([mx.fused("x", "w1", "y", act="'silu'", gate="w2"), "s = silu(y)", "z = add(s, r)"],
                        mx.provenance(gated=1))


@pytest.mark.parametrize("case", ["requires_grad", "bias_requires_grad", "float32", "cpu", "nine_rows"])
def test_mxfp4_left_alone(mx, case):
    p = Program()
    rows = 9 if case == "nine_rows" else 1
    x = p.t("x", rows, K, requires_grad=case == "requires_grad", dtype=F32 if case == "float32" else BF16,
            device="cpu" if case == "cpu" else "cuda")
    bias = p.t("bias", N, requires_grad=True) if case == "bias_requires_grad" else None
    y = p.t("y", rows, N, dtype=x.dtype, device=str(x.device))
    mx.proj(p, x, mx.weight(p, "w1"), y, bias)
    unchanged(p.run(y))


def test_mxfp4_switch_leaves_everything_in_place(mx, monkeypatch):
    monkeypatch.setenv("LTA_MXFP4_DECODE_FUSION", "0")
    p = Program()
    x, a, b, y = _pair(p, mx)
    p(hipex.hip_swiglu, a, b, out=y)
    unchanged(p.run(y))


def test_mxfp4_unfused_candidate_is_lowered_with_its_bias(mx):
    p = Program()
    x, bias, y = p.t("x", 8, K), p.t("bias", N), p.t("y", 8, N)
    p(mx.sym, x, *mx.weight(p, "w1"), bias=bias, out=y)
    assert p.run(y) == ([mx.lowered("x", "w1", "y", bias="bias")], mx.provenance())


# ------------------------------------------------------------------------------------------------
# residual adds into the GEMM epilogues
# ------------------------------------------------------------------------------------------------
M = 16


def _gemm(p, which, *, at=False, residual=None):
    """``y = <gemm>(...)`` of M rows; returns (y, the expected call without its closing residual)."""
    y = p.t("y", M, N)
    if which == "hip_linear":
        x, w, b = p.t("x", M, K), p.t("w", N, K), p.t("b", N)
        p(hipex.hip_linear, x, w, b, out=y)
        return y, "hip_linear(x, w, b, "
    if which == "hip_matmul":
        x, w = p.t("x", M, K), p.t("w", K, N)
        p(hipex.hip_matmul, x, w, out=y)
        return y, "hip_matmul(x, w, "
    qa, qb = p.t("qa", M, K, dtype=U8), p.t("qb", N, K, dtype=U8)
    sa, sb = p.ts("sa sb", dtype=F32)
    if which == "hip_fp8_gemm":
        p(hipex.hip_fp8_gemm, qa, qb, sa, sb, 0, 0, None, (M, N), *(() if residual is None else (residual,)), out=y)
        return y, "hip_fp8_gemm(qa, qb, sa, sb, 0, 0, None, (16, 512), "
    p(hipex.hip_fp8_gemm_layout, qa, qb, sa, sb, 1, at, (M, N), out=y)
    return y, "hip_fp8_gemm_layout(qa, qb, sa, sb, 1, False, (16, 512), "


_GEMMS = ["hip_linear", "hip_matmul", "hip_fp8_gemm", "hip_fp8_gemm_layout"]
_EPILOGUE = "hipex: 1 residual add(s) fused into GEMM epilogues"


@pytest.mark.parametrize("y_first", [True, False])
@pytest.mark.parametrize("claimed", [False, True])
@pytest.mark.parametrize("which", _GEMMS)
def test_residual_add_into_gemm(which, claimed, y_first):
    add = _torch_op("torch_add") if claimed else lt.add
    p = Program()
    r, z, u, u0 = p.t("r", M, N), p.t("z", M, N), p.t("u", M, K), p.t("u0", M, K)
    y, call = _gemm(p, which)
    p(lt.silu, u0, out=u)  # stands between the GEMM and the add: shows where the fused op is emitted
    p(add, *((y, r) if y_first else (r, y)), out=z)
    fused = f"z = {call}r)"
    # hip_matmul is computed where the GEMM was, the others where the add was
    lines = [fused, "u = silu(u0)"] if which == "hip_matmul" else ["u = silu(u0)", fused]
    assert p.run(z, u) == (lines, _EPILOGUE)


@pytest.mark.parametrize("which", _GEMMS)
def test_residual_produced_after_the_gemm(which):
    p = Program()
    r0, r, z = p.ts("r0 r z", M, N)
    y, call = _gemm(p, which)
    p(lt.silu, r0, out=r)
    p(lt.add, y, r, out=z)
    result = p.run(z)
    if which in ("hip_linear", "hip_matmul"):  # emitted (or checked) at the GEMM: the residual is not there yet
        unchanged(result)
    else:
        assert result == (["r = silu(r0)", f"z = {call}r)"], _EPILOGUE)


@pytest.mark.parametrize("which", _GEMMS)
def test_residual_add_refused_gemm_read_twice(which):
    p = Program()
    r, z, z2 = p.ts("r z z2", M, N)
    y, _ = _gemm(p, which)
    p(lt.add, y, r, out=z)
    p(lt.silu, y, out=z2)
    unchanged(p.run(z, z2))


def test_residual_add_refused_layout_at_flag():
    p = Program()
    r, z = p.ts("r z", M, N)
    y, _ = _gemm(p, "hip_fp8_gemm_layout", at=True)
    p(lt.add, y, r, out=z)
    unchanged(p.run(z))


def test_residual_add_refusals():
    p = Program()
    r, r2, z = p.ts("r r2 z", M, N)
    y, _ = _gemm(p, "hip_fp8_gemm", residual=r)
    p(lt.add, y, r2, out=z)  # the GEMM already has a residual
    unchanged(p.run(z))
    p = Program()
    r, z = p.ts("r z", M, N)
    small = p.t("small", N)
    y, _ = _gemm(p, "hip_linear")
    p(lt.add, y, small, out=z)  # a broadcast add is no residual
    unchanged(p.run(z))
    p = Program()
    r, z = p.ts("r z", M, N)
    y, _ = _gemm(p, "hip_matmul")
    p(lt.add, y, r, alpha=2, out=z)
    unchanged(p.run(z))


def test_residual_add_into_linear_that_has_a_residual_is_refused():
    p = Program()
    x, w, r, r2, y, z = p.t("x", M, K), p.t("w", N, K), *p.ts("r r2 y z", M, N)
    p(hipex.hip_linear, x, w, None, r, out=y)
    p(lt.add, y, r2, out=z)
    unchanged(p.run(z))


# ------------------------------------------------------------------------------------------------
# residual-gradient adds into the normalisation backwards
# ------------------------------------------------------------------------------------------------
def _norm_bwd(p, which):
    dy, x, dx = p.ts("dy x dx", M, K)
    w, dw, db = p.ts("w dw db", K)
    mean, rstd = p.ts("mean rstd", M, dtype=F32)
    if which == "rms":
        p(hipex.hip_rms_norm_bwd, dy, x, w, rstd, out=(dx, dw))
        return dx, (dw,), "z, dw = hip_rms_norm_bwd(dy, x, w, rstd, r)"
    p(hipex.hip_layer_norm_bwd, dy, x, w, mean, rstd, True, out=(dx, dw, db))
    return dx, (dw, db), "z, dw, db = hip_layer_norm_bwd(dy, x, w, mean, rstd, True, r)"


@pytest.mark.parametrize("dx_first", [True, False])
@pytest.mark.parametrize("which", ["rms", "layer"])
def test_residual_gradient_into_norm_backward(which, dx_first):
    p = Program()
    r, z, u, u0 = p.ts("r z u u0", M, K)
    dx, rest, fused = _norm_bwd(p, which)
    p(lt.silu, u0, out=u)
    p(lt.add, *((dx, r) if dx_first else (r, dx)), out=z)
    assert p.run(z, u, *rest) == ([fused, "u = silu(u0)"],
                                  "hipex: 1 residual-gradient add(s) fused into a normalisation backward")


@pytest.mark.parametrize("which", ["rms", "layer"])
@pytest.mark.parametrize("case", ["dx_read_twice", "residual_produced_later", "dw_added"])
def test_residual_gradient_refused(which, case):
    p = Program()
    r0, r, z, z2 = p.ts("r0 r z z2", M, K)
    dx, rest, _ = _norm_bwd(p, which)
    if case == "dx_read_twice":
        p(lt.add, dx, r, out=z)
        p(lt.silu, dx, out=z2)
        unchanged(p.run(z, z2, *rest))
    elif case == "residual_produced_later":
        p(lt.silu, r0, out=r)
        p(lt.add, dx, r, out=z)
        unchanged(p.run(z, *rest))
    else:
        g, zw = p.ts("g zw", K)
        p(lt.add, rest[0], g, out=zw)
        unchanged(p.run(dx, zw))


# ------------------------------------------------------------------------------------------------
# KV-cache writes into the RoPE
# ------------------------------------------------------------------------------------------------
def _rope(p):
    qkv, cos, sin = p.t("qkv", 1, 1, 3 * 4 * 64), p.t("cos", 1, 64), p.t("sin", 1, 64)
    q, k, v = p.ts("q k v", 1, 4, 1, 64)
    kc, vc, kc2, vc2 = p.ts("kc vc kc2 vc2", 1, 4, 32, 64)
    p(hipex.hip_qkv_rope, qkv, cos, sin, 4, 4, 64, 64, out=(q, k, v))
    return q, k, v, kc, vc, kc2, vc2


_ROPE_CACHE = "q, kc2, vc2 = hip_qkv_rope_cache(qkv, cos, sin, 4, 4, 64, 64, kc, vc, pos)"
_KV = "hipex: 1 KV-cache write pair(s) fused into RoPE"


def test_kv_cache_writes_emitted_at_the_rope():
    p = Program()
    pos = p.t("pos", 1, dtype=I64)
    q, k, v, kc, vc, kc2, vc2 = _rope(p)
    s = p.t("s", 1, 4, 1, 64)
    p(lt.silu, q, out=s)
    p(index_copy_inplace, kc, 2, pos, k, out=kc2)
    p(index_copy_inplace, vc, 2, pos, v, out=vc2)
    assert p.run(s, kc2, vc2) == ([_ROPE_CACHE, "s = silu(q)"], _KV)


def _hf_order(p, between_rope_and_writes=None, between_writes=None, pos_dtype=I64):
    p0, pos = p.ts("p0 pos", 1, dtype=pos_dtype)
    q, k, v, kc, vc, kc2, vc2 = _rope(p)
    s = p.t("s", 1, 4, 32, 64)
    if between_rope_and_writes == "q":
        s = p.t("sq", 1, 4, 1, 64)
        p(lt.silu, q, out=s)
    p(lt.silu, p0, out=pos)  # the positions are computed after the RoPE
    p(index_copy_inplace, kc, 2, pos, k, out=kc2)
    if between_writes is not None:
        p(lt.silu, {"kc2": kc2, "vc": vc}[between_writes], out=s)
    p(index_copy_inplace, vc, 2, pos, v, out=vc2)
    return q, kc2, vc2, s


def test_kv_cache_writes_emitted_at_the_later_write():
    p = Program()
    q, kc2, vc2, _ = _hf_order(p)
    assert p.run(q, kc2, vc2) == (["pos = silu(p0)", _ROPE_CACHE], _KV)


@pytest.mark.parametrize("case", ["q_read_in_between", "cache_result_read_in_between", "cache_read_in_between", "int32"])
def test_kv_cache_writes_refused(case):
    p = Program()
    if case == "q_read_in_between":
        q, kc2, vc2, s = _hf_order(p, between_rope_and_writes="q")
    elif case == "cache_result_read_in_between":
        q, kc2, vc2, s = _hf_order(p, between_writes="kc2")
    elif case == "cache_read_in_between":
        q, kc2, vc2, s = _hf_order(p, between_writes="vc")
    else:
        q, kc2, vc2, s = _hf_order(p, pos_dtype=I32)
    unchanged(p.run(q, kc2, vc2, s))


@pytest.mark.parametrize("case", ["k_returned", "k_read_twice", "other_dim", "other_positions", "plain_index_copy"])
def test_kv_cache_writes_refused_at_the_rope(case):
    p = Program()
    pos, pos2 = p.ts("pos pos2", 1, dtype=I64)
    q, k, v, kc, vc, kc2, vc2 = _rope(p)
    s = p.t("s", 1, 4, 1, 64)
    if case == "k_read_twice":
        p(lt.silu, k, out=s)
    write = lt.index_copy if case == "plain_index_copy" else index_copy_inplace
    p(write, kc, 1 if case == "other_dim" else 2, pos, k, out=kc2)
    p(index_copy_inplace, vc, 2, pos2 if case == "other_positions" else pos, v, out=vc2)
    unchanged(p.run(q, kc2, vc2, *((k,) if case == "k_returned" else ()), *((s,) if case == "k_read_twice" else ())))


# ------------------------------------------------------------------------------------------------
# fp8 input casts into their producers
# ------------------------------------------------------------------------------------------------
_CASTS = "hipex: 1 fp8 input cast(s) fused into their producers"


def _cast(p, t, e5m2, slot, tag):
    q, s = p.t("q" + tag, M, t.shape[-1], dtype=U8), p.t("s" + tag, dtype=F32)
    p(hipex.hip_fp8_cast_delayed, t, e5m2, "key", slot, out=(q, s))
    return q, s


def _norm_cast(p, weight=True):
    x, g = p.t("x", M, K), p.t("g", K)
    h, rstd = p.t("h", M, K), p.t("rstd", M, dtype=F32)
    p(hipex.hip_rms_norm_fwd, x, g if weight else None, 1e-5, out=(h, rstd))
    return h, rstd


def test_fp8_cast_into_norm():
    p = Program()
    h, rstd = _norm_cast(p)
    q, s = _cast(p, h, False, 3, "")
    assert p.run(q, s, rstd) == (["q, s, rstd = hip_rms_norm_fwd_fp8(x, g, 1e-05, 'key', 3)"], _CASTS)


def test_fp8_cast_into_swiglu():
    p = Program()
    a, b, y = p.ts("a b y", M, N)
    p(hipex.hip_swiglu, a, b, out=y)
    q, s = _cast(p, y, False, 4, "")
    assert p.run(q, s) == (["q, s = hip_swiglu_fp8(a, b, 'key', 4)"], _CASTS)


def test_fp8_casts_into_swiglu_backward():
    p = Program()
    g, a, b, da, db = p.ts("g a b da db", M, N)
    p(hipex.hip_swiglu_bwd, g, a, b, out=(da, db))
    qa, sa = _cast(p, da, True, 5, "a")
    qb, sb = _cast(p, db, True, 6, "b")
    assert p.run(qa, sa, qb, sb) == (["qa, sa, qb, sb = hip_swiglu_bwd_fp8(g, a, b, 'key', 5, 6)"], _CASTS)


@pytest.mark.parametrize("case", ["switch", "read_twice", "e5m2", "no_weight", "returned"])
def test_fp8_cast_into_norm_refused(case, monkeypatch):
    p = Program()
    if case == "switch":
        monkeypatch.setenv("LTA_FP8_FUSE_PRODUCERS", "0")
    h, rstd = _norm_cast(p, weight=case != "no_weight")
    q, s = _cast(p, h, case == "e5m2", 3, "")
    z = p.t("z", M, K)
    if case == "read_twice":
        p(lt.silu, h, out=z)
    # "returned": the return symbol is a reader like any other in this pass's count
    unchanged(p.run(q, s, *((z,) if case == "read_twice" else ()), *((h,) if case == "returned" else ())))


def test_fp8_casts_into_swiglu_backward_refused():
    p = Program()
    g, a, b, da, db = p.ts("g a b da db", M, N)
    p(hipex.hip_swiglu_bwd, g, a, b, out=(da, db))
    qa, sa = _cast(p, da, True, 5, "a")
    unchanged(p.run(qa, sa, db))  # only one of the two gradients is cast


# ------------------------------------------------------------------------------------------------
# the opt-in SwiGLU GEMM epilogues
# ------------------------------------------------------------------------------------------------
def _gate_up(p, rows=M):
    x, w1, w2 = p.t("x", rows, K), p.t("w1", N, K), p.t("w2", N, K)
    a, b, y = p.ts("a b y", rows, N)
    p(hipex.hip_linear, x, w1, None, out=a)
    p(hipex.hip_linear, x, w2, None, out=b)
    p(hipex.hip_swiglu, a, b, out=y)
    return a, b, y


_SWIGLU_FWD = "hipex: 1 gate-up SwiGLU GEMM(s), 0 SwiGLU-backward GEMM epilogue(s)"


def test_swiglu_gemm_forward(monkeypatch):
    monkeypatch.setenv("LTA_FUSED_SWIGLU", "1")
    p = Program()
    a, b, y = _gate_up(p)
    assert p.run(y) == (["y = hip_gate_up_y(x, w1, w2)"], _SWIGLU_FWD)


def test_swiglu_gemm_forward_keeps_a_and_b_for_later_readers(monkeypatch):
    monkeypatch.setenv("LTA_FUSED_SWIGLU", "1")
    p = Program()
    a, b, y = _gate_up(p)
    assert p.run(y, a) == (["a, b, y = hip_gate_up(x, w1, w2)"], _SWIGLU_FWD)


def test_swiglu_gemm_is_opt_in(monkeypatch):
    monkeypatch.delenv("LTA_FUSED_SWIGLU", raising=False)
    p = Program()
    a, b, y = _gate_up(p)
    unchanged(p.run(y))


def test_swiglu_gemm_leaves_decode_rows_to_the_gemv(monkeypatch):
    monkeypatch.setenv("LTA_FUSED_SWIGLU", "1")
    p = Program()
    a, b, y = _gate_up(p, rows=8)
    assert p.run(y) == ([Bf16().fused("x", "w1", "y", act="'silu'", gate="w2")], Bf16().provenance(gated=1))


def _swiglu_bwd(p):
    dy, w = p.t("dy", M, K), p.t("w", K, N)
    g, a, b, da, db = p.ts("g a b da db", M, N)
    p(hipex.hip_matmul, dy, w, out=g)
    p(hipex.hip_swiglu_bwd, g, a, b, out=(da, db))
    return g, da, db


def test_swiglu_gemm_backward(monkeypatch):
    monkeypatch.setenv("LTA_FUSED_SWIGLU", "1")
    p = Program()
    g, da, db = _swiglu_bwd(p)
    assert p.run(da, db) == (["da, db = hip_matmul_swiglu_bwd(dy, w, a, b)"],
                             "hipex: 0 gate-up SwiGLU GEMM(s), 1 SwiGLU-backward GEMM epilogue(s)")


def test_swiglu_gemm_backward_refused_g_returned(monkeypatch):
    monkeypatch.setenv("LTA_FUSED_SWIGLU", "1")
    p = Program()
    g, da, db = _swiglu_bwd(p)
    unchanged(p.run(da, db, g))


# ------------------------------------------------------------------------------------------------
# the RoPE split in the qkv GEMM epilogues (bf16 and fp8), the RoPE backward in the attention backward
# ------------------------------------------------------------------------------------------------
B_, T_, NH, NG, HS = 2, 16, 2, 2, 128
_QKV_N = (NH + 2 * NG) * HS


def _rope_outs(p):
    return p.t("q", B_, NH, T_, HS), p.t("k", B_, NG, T_, HS), p.t("v", B_, NG, T_, HS)


@pytest.mark.parametrize("switch", [None, "0"])
def test_qkv_rope_into_gemm(switch, monkeypatch):
    # LTA_FUSED_QKV_ROPE is read by the launcher, not by the pass: the program is the same either way
    monkeypatch.delenv("LTA_FUSED_QKV_ROPE", raising=False) if switch is None else monkeypatch.setenv("LTA_FUSED_QKV_ROPE", switch)
    p = Program()
    x, w, qkv = p.t("x", B_, T_, K), p.t("w", _QKV_N, K), p.t("qkv", B_, T_, _QKV_N)
    cos, sin = p.ts("cos sin", T_, HS, dtype=F32)
    p(hipex.hip_linear, x, w, None, out=qkv)
    q, k, v = p(hipex.hip_qkv_rope, qkv, cos, sin, NH, NG, HS, HS, out=_rope_outs(p))
    assert p.run(q, k, v) == (["q, k, v = hip_linear_qkv_rope(x, w, cos, sin, 2, 2, 128, 128)"],
                              "hipex: 1 qkv projection(s) with the RoPE split in the GEMM epilogue")


@pytest.mark.parametrize("case", ["qkv_returned", "bias", "decode_rows", "cos_produced_later"])
def test_qkv_rope_into_gemm_refused(case):
    p = Program()
    T = 1 if case == "decode_rows" else T_
    x, w, qkv = p.t("x", 1 if case == "decode_rows" else B_, T, K), p.t("w", _QKV_N, K), p.t("qkv", B_, T, _QKV_N)
    cos0, cos, sin = p.ts("cos0 cos sin", T, HS, dtype=F32)
    bias = p.t("bias", _QKV_N) if case == "bias" else None
    p(hipex.hip_linear, x, w, bias, out=qkv)
    if case == "cos_produced_later":
        p(lt.silu, cos0, out=cos)
    q, k, v = p(hipex.hip_qkv_rope, qkv, cos, sin, NH, NG, HS, HS, out=_rope_outs(p))
    unchanged(p.run(q, k, v, *((qkv,) if case == "qkv_returned" else ())))


def _fp8_qkv(p, bias=None, fmt_b=0):
    qx, qw = p.t("qx", B_ * T_, K, dtype=U8), p.t("qw", _QKV_N, K, dtype=U8)
    sx, sw = p.ts("sx sw", dtype=F32)
    qkv = p.t("qkv", B_, T_, _QKV_N)
    cos, sin = p.ts("cos sin", T_, HS, dtype=F32)
    p(hipex.hip_fp8_gemm, qx, qw, sx, sw, 0, fmt_b, bias, (B_, T_, _QKV_N), out=qkv)
    return p(hipex.hip_qkv_rope, qkv, cos, sin, NH, NG, HS, HS, out=_rope_outs(p)), qkv


def test_fp8_qkv_rope_into_gemm():
    p = Program()
    (q, k, v), _ = _fp8_qkv(p)
    assert p.run(q, k, v) == (["q, k, v = hip_fp8_gemm_qkv_rope(qx, qw, sx, sw, (2, 16, 768), cos, sin, 2, 2, 128, 128)"],
                              "hipex: 1 fp8 qkv projection(s) with the RoPE split in the GEMM epilogue")


@pytest.mark.parametrize("case", ["bias", "e5m2_weight", "qkv_returned"])
def test_fp8_qkv_rope_into_gemm_refused(case):
    p = Program()
    bias = p.t("bias", _QKV_N) if case == "bias" else None
    (q, k, v), qkv = _fp8_qkv(p, bias=bias, fmt_b=1 if case == "e5m2_weight" else 0)
    unchanged(p.run(q, k, v, *((qkv,) if case == "qkv_returned" else ())))


def _attn_bwd(p, hs=HS, rope_n=None):
    g, q, o = p.ts("g q o", B_, NH, T_, hs)
    k, v = p.ts("k v", B_, NG, T_, hs)
    lse = p.t("lse", B_, NH, T_, dtype=F32)
    cos, sin = p.ts("cos sin", T_, hs, dtype=F32)
    dq, dk, dv = p.t("dq", B_, NH, T_, hs), p.t("dk", B_, NG, T_, hs), p.t("dv", B_, NG, T_, hs)
    dqkv = p.t("dqkv", B_, T_, (NH + 2 * NG) * hs)
    p(hipex.hip_attn_bwd, g, q, k, v, o, lse, True, 0.25, out=(dq, dk, dv))
    return (dq, dk, dv), dqkv, (cos, sin, NH, NG, hs, hs if rope_n is None else rope_n)


def test_rope_backward_into_attention_backward():
    p = Program()
    grads, dqkv, rope = _attn_bwd(p)
    p(hipex.hip_qkv_rope_bwd, *grads, *rope, out=dqkv)
    assert p.run(dqkv) == (["dqkv = hip_flash_attn_bwd_rope(g, q, k, v, o, lse, True, 0.25, cos, sin, 2, 2)"],
                           "hipex: 1 RoPE backward(s) fused into the attention backward")


@pytest.mark.parametrize("case", ["head_size_64", "partial_rope", "dk_read_twice"])
def test_rope_backward_into_attention_backward_refused(case):
    p = Program()
    grads, dqkv, rope = _attn_bwd(p, hs=64 if case == "head_size_64" else HS, rope_n=64 if case == "partial_rope" else None)
    p(hipex.hip_qkv_rope_bwd, *grads, *rope, out=dqkv)
    z = p.t("z", *grads[1].shape)
    if case == "dk_read_twice":
        p(lt.silu, grads[1], out=z)
    unchanged(p.run(dqkv, *((z,) if case == "dk_read_twice" else ())))


# ------------------------------------------------------------------------------------------------
# e5m2 gradient casts into the RMSNorm backward, e4m3 casts into the attention epilogue
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("residual", [False, True])
def test_fp8_gradient_cast_into_rms_backward(residual):
    p = Program()
    dy, x, dx, r = p.ts("dy x dx r", M, K)
    w, dw = p.ts("w dw", K)
    rstd = p.t("rstd", M, dtype=F32)
    p(hipex.hip_rms_norm_bwd, dy, x, w, rstd, *((r,) if residual else ()), out=(dx, dw))
    q, s = _cast(p, dx, True, 7, "")
    # dx keeps its other readers (here: the return)
    assert p.run(dx, dw, q, s) == (
        [f"dx, dw, q, s = hip_rms_norm_bwd_fp8(dy, x, w, rstd, {'r' if residual else 'None'}, 'key', 7)"],
        "hipex: 1 e5m2 gradient cast(s) fused into RMSNorm backwards")


def test_fp8_gradient_cast_follows_the_residual_gradient_add():
    p = Program()
    dy, x, dx, r, z = p.ts("dy x dx r z", M, K)
    w, dw = p.ts("w dw", K)
    rstd = p.t("rstd", M, dtype=F32)
    p(hipex.hip_rms_norm_bwd, dy, x, w, rstd, out=(dx, dw))
    p(lt.add, dx, r, out=z)
    q, s = _cast(p, z, True, 7, "")
    assert p.run(z, dw, q, s) == (["z, dw, q, s = hip_rms_norm_bwd_fp8(dy, x, w, rstd, r, 'key', 7)"],
                                  "hipex: 1 e5m2 gradient cast(s) fused into RMSNorm backwards")


@pytest.mark.parametrize("case", ["e4m3", "dw_cast", "second_cast", "switch"])
def test_fp8_gradient_cast_into_rms_backward_refused(case, monkeypatch):
    if case == "switch":
        monkeypatch.setenv("LTA_FP8_FUSE_PRODUCERS", "0")
    p = Program()
    dy, x, dx = p.ts("dy x dx", M, K)
    w, dw = p.ts("w dw", 1, K)
    rstd = p.t("rstd", M, dtype=F32)
    p(hipex.hip_rms_norm_bwd, dy, x, w, rstd, out=(dx, dw))
    if case == "second_cast":
        q, s = _cast(p, dx, True, 7, "")
        q2, s2 = _cast(p, dx, True, 8, "2")
        assert p.run(dx, dw, q, s, q2, s2) == (
            ["dx, dw, q, s = hip_rms_norm_bwd_fp8(dy, x, w, rstd, None, 'key', 7)",
             "q2, s2 = hip_fp8_cast_delayed(dx, True, 'key', 8)"],
            "hipex: 1 e5m2 gradient cast(s) fused into RMSNorm backwards")
        return
    q, s = _cast(p, dw if case == "dw_cast" else dx, case != "e4m3", 7, "")
    unchanged(p.run(dx, dw, q, s))


def _attn_out(p, view, hs=HS):
    q, o = p.ts("q o", B_, NH, T_, hs)
    k, v = p.ts("k v", B_, NG, T_, hs)
    lse = p.t("lse", B_, NH, T_, dtype=F32)
    p(hipex.hip_attn_fwd, q, k, v, True, 0.25, out=(o, lse))
    t = p.t("t", B_, T_, NH, hs)
    y = p.t("y", B_, T_, NH * hs)
    if view == "transpose":
        p(lt.transpose, o, 1, 2, out=t)
    elif view == "negative_dims":
        p(lt.transpose, o, -2, -3, out=t)
    elif view == "permute":
        p(lt.permute, o, (0, 2, 1, 3), out=t)
    elif view == "permute_varargs":
        p(lt.permute, o, 0, 2, 1, 3, out=t)
    elif view == "wrong_transpose":
        p(lt.transpose, o, 0, 1, out=t)
    elif view == "wrong_permute":
        p(lt.permute, o, (0, 1, 2, 3), out=t)
    elif view == "reshape_first":
        p(lt.reshape, o, (B_, T_, NH, hs), out=t)
    if view == "two_transposes":
        t0 = p.t("t0", B_, T_, NH, hs)
        p(lt.transpose, o, 1, 2, out=t0)
        p(lt.transpose, t0, 1, 2, out=t)
    if view == "no_view":
        return o, lse, o
    p(lt.reshape, t, (B_, T_, NH * hs) if view != "unmerged" else (B_, T_ * NH, hs), out=y)
    return o, lse, y


_ATTN_CAST = "hipex: 1 e4m3 attention-output cast(s) fused into the attention epilogue"


@pytest.mark.parametrize("view", ["transpose", "negative_dims", "permute", "permute_varargs"])
def test_fp8_cast_into_attention_epilogue(view):
    p = Program()
    o, lse, y = _attn_out(p, view)
    q, s = _cast(p, y, False, 9, "y")
    lines, prov = p.run(o, lse, q, s)
    assert lines[0] == "o, lse, qy, sy = hip_flash_attn_fwd_fp8(q, k, v, True, 0.25, 'key', 9)"
    assert [ln.split(" = ")[0] for ln in lines[1:]] == ["t", "y"] and prov == _ATTN_CAST  # the view chain stays


@pytest.mark.parametrize("view", ["wrong_transpose", "wrong_permute", "reshape_first", "two_transposes", "no_view"])
def test_fp8_cast_into_attention_epilogue_refused_views(view):
    p = Program()
    o, lse, y = _attn_out(p, view)
    q, s = _cast(p, y, False, 9, "y")
    unchanged(p.run(o, lse, q, s))


@pytest.mark.parametrize("case", ["head_size_64", "e5m2", "switch"])
def test_fp8_cast_into_attention_epilogue_refused(case, monkeypatch):
    if case == "switch":
        monkeypatch.setenv("LTA_FP8_FUSE_PRODUCERS", "0")
    p = Program()
    o, lse, y = _attn_out(p, "transpose", hs=64 if case == "head_size_64" else HS)
    q, s = _cast(p, y, case == "e5m2", 9, "y")
    unchanged(p.run(o, lse, q, s))


def test_merges_heads_refuses_a_chain_that_does_not_merge_heads():
    p = Program()
    o, lse, y = _attn_out(p, "unmerged")
    q, s = _cast(p, y, False, 9, "y")
    unchanged(p.run(o, lse, q, s))


# ------------------------------------------------------------------------------------------------
# the order of the passes
# ------------------------------------------------------------------------------------------------
def test_bf16_grouping_runs_after_the_kv_cache_pass_and_mxfp4_before(mx):
    """One decode attention block per weight kind: both programs fuse the same way, but the bf16 siblings are
    grouped after the KV-cache pass (the last provenance is the grouping's) and the MXFP4 ones before it."""
    for kind, last in ((Bf16(), Bf16().group_provenance(1)), (mx, _KV)):
        p = Program()
        pos = p.t("pos", 1, dtype=I64)
        x, outs = _siblings(p, kind, 3, shape=(1, 1, K))
        qkv = p.t("qkv", 1, 1, 3 * 4 * 64)
        p(lt.cat, outs, -1, out=qkv)
        cos, sin = p.t("cos", 1, 64), p.t("sin", 1, 64)
        q, k, v = p.ts("q k v", 1, 4, 1, 64)
        kc, vc, kc2, vc2 = p.ts("kc vc kc2 vc2", 1, 4, 32, 64)
        p(hipex.hip_qkv_rope, qkv, cos, sin, 4, 4, 64, 64, out=(q, k, v))
        p(index_copy_inplace, kc, 2, pos, k, out=kc2)
        p(index_copy_inplace, vc, 2, pos, v, out=vc2)
        assert p.run(q, kc2, vc2) == ([kind.group("x", ["w0", "w1", "w2"], "qkv", packed=True), _ROPE_CACHE], last)


def test_a_norm_read_by_both_weight_kinds_stays(mx):
    p = Program()
    x, h, rstd = _norm(p, 1)
    o1, o2 = p.ts("o1 o2", 1, N)
    Bf16().proj(p, h, Bf16().weight(p, "w1"), o1)
    mx.proj(p, h, mx.weight(p, "w2"), o2)
    assert p.run(o1, o2) == (["h, rstd = hip_rms_norm_fwd(x, g, 1e-06)", "o1 = hip_linear(h, w1, None)",
                              mx.lowered("h", "w2", "o2")], mx.provenance())


def test_nothing_to_rewrite_returns_the_same_object():
    p = Program()
    x, y, z = p.ts("x y z", 4, K)
    p(lt.silu, x, out=y)
    p(lt.mul, y, x, out=z)
    new = hipex._post_claim(p.trace)  # without a return
    assert new is p.trace
    unchanged(p.run(z))
