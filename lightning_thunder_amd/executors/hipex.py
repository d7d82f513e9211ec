"""hipex: the hand-written CDNA4 kernel executor (replaces the reference's cuDNN / sdpa / apex / TE /
Triton-CE executors: ``thunder/executors/{cudnnex,sdpaex,apexex,triton_crossentropy,transformer_engineex}.py``).

It claims high-level ltorch ops whole (RMSNorm, SDPA, cross-entropy, RoPE/qkv-split,
SwiGLU, ...) on HIP devices and provides *grad transforms* so autodiff saves exactly
what the fused backward kernels need (e.g. RMSNorm's per-row rstd, attention's LSE).
"""
from __future__ import annotations

import math
import os
from functools import partial
from typing import Callable, NamedTuple

import torch

from ..core.prims import OpTags
from ..core.proxies import Proxy, TensorProxy, pyval
from ..core import dtypes
from ..extend import OperatorExecutor, register_executor, add_default_executor
from ..ops.kv8 import E4M3_MAX
from .rewrite import Rewrite, operands

ex = OperatorExecutor("hipex", version="0.1")
register_executor(ex)
add_default_executor(ex)

hipex = ex


def _gpu(*ts) -> bool:
    return all(t is None or (isinstance(t, TensorProxy) and t.device.type == "cuda") for t in ts)


_FLOAT16ISH = (torch.bfloat16, torch.float16, torch.float32)


# =========================================================================================
# K2 GEMM: linear forward (+ fused epilogues) on the hand-written MFMA kernel
# =========================================================================================
def _linear_meta(x, w, bias=None, residual=None, act=None):
    return TensorProxy(like=x, shape=tuple(x.shape[:-1]) + (w.shape[0],))


def _linear_impl(x, w, bias=None, residual=None, act=None):
    from ..ops.gemm import linear

    return linear(x, w, bias, residual, act)


hip_linear = ex.register_operator("hip_linear", meta=_linear_meta, fn=_linear_impl)


def _linear_checker(a, w, bias=None):
    from ..ops.gemm import _hand_gemm_shape

    if not _gpu(a, w, bias) or a.dtype != torch.bfloat16 or w.dtype != torch.bfloat16 or w.ndim != 2:
        return False
    if bias is not None and (bias.dtype != torch.bfloat16 or bias.ndim != 1):
        return False
    if a.ndim < 2:
        return False
    M = 1
    for s in a.shape[:-1]:
        M *= s
    N, K = w.shape
    if a.shape[-1] != K:
        return False
    if M <= 8:  # decode: the weight-streaming GEMV (csrc/gemv.hip)
        return K % 8 == 0
    return _hand_gemm_shape(M, N, K)


def _linear_exec(a, w, bias=None):
    return hip_linear(a, w, bias)


def _register_linear():
    from .. import torch as ltorch

    ex.register_implementation(ltorch.linear, checker=_linear_checker, execution_transform=_linear_exec)


_register_linear()


# K2 GEMM for the prim matmul: the backward's dgrad (g @ W) and wgrad (g^T @ x) read their
# transposed operands through the transposing LDS read (csrc/gemm.hip, MN-major images)
def _mm_impl(a, b, residual=None):
    from ..ops.gemm import matmul

    return matmul(a, b, residual)


def _mm_checker(a, b):
    from ..ops.gemm import _hand_gemm_shape

    if not _gpu(a, b) or a.dtype != torch.bfloat16 or b.dtype != torch.bfloat16 or b.ndim != 2 or a.ndim < 2:
        return False
    M = 1
    for s in a.shape[:-1]:
        M *= s
    K, N = b.shape
    return a.shape[-1] == K and _hand_gemm_shape(M, N, K)


def _mm_meta(a, b, residual=None):
    return TensorProxy(like=a, shape=tuple(a.shape[:-1]) + (b.shape[1],))


hip_matmul = ex.register_operator("hip_matmul", meta=_mm_meta, fn=_mm_impl)


def _register_matmul():
    from ..core import prims as P

    ex.register_implementation(P.matmul, checker=_mm_checker, execution_transform=lambda a, b: hip_matmul(a, b))


_register_matmul()


# =========================================================================================
# K8 FP8 linear (fwd/bwd on the block-scaled MFMA GEMM)
# =========================================================================================
def _fp8_quant_meta(t, e5m2):
    C = t.shape[-1]
    R = 1
    for d in t.shape[:-1]:
        R *= d
    u8 = torch.uint8
    return (TensorProxy(like=t, shape=(R, C), dtype=u8, requires_grad=False),
            TensorProxy(like=t, shape=(C, R), dtype=u8, requires_grad=False),
            TensorProxy(like=t, shape=(), dtype=torch.float32, requires_grad=False))


def _fp8_quant_impl(t, e5m2):
    from ..ops.fp8 import quantize

    return quantize(t, e5m2)


def _fp8_gemm_meta(qa, qb, sa, sb, fmt_a, fmt_b, bias, out_shape, residual=None):
    return TensorProxy(like=qa, shape=tuple(out_shape), dtype=torch.bfloat16)


def _fp8_gemm_impl(qa, qb, sa, sb, fmt_a, fmt_b, bias, out_shape, residual=None):
    from ..ops.fp8 import gemm

    return gemm(qa, qb, sa, sb, fmt_a, fmt_b, bias, out_shape, residual)


# quantize = amax + cast(+transpose) (pure: CSE shares one quantisation of x between the sibling
# fc_1 / fc_2 linears); gemm = the block-scaled-MFMA NT kernel
hip_fp8_quantize = ex.register_operator("hip_fp8_quantize", meta=_fp8_quant_meta, fn=_fp8_quant_impl)
hip_fp8_gemm = ex.register_operator("hip_fp8_gemm", meta=_fp8_gemm_meta, fn=_fp8_gemm_impl)


def _fp8_quant_delayed_meta(t, e5m2, key, slot):
    return _fp8_quant_meta(t, e5m2)


def _fp8_quant_delayed_impl(t, e5m2, key, slot):
    from ..ops.fp8 import quantize_delayed

    return quantize_delayed(t, e5m2, key, slot)


def _fp8_update_impl(key):
    from ..ops.fp8 import delayed_update

    delayed_update(key)


# delayed scaling: quantize against the slot's amax history (its own amax recorded while casting);
# the history advances once per forward (first op of the program), after an amax all-reduce
hip_fp8_quantize_delayed = ex.register_operator("hip_fp8_quantize_delayed", meta=_fp8_quant_delayed_meta,
                                                fn=_fp8_quant_delayed_impl)
hip_fp8_delayed_update = ex.register_operator("hip_fp8_delayed_update", meta=lambda key: None, fn=_fp8_update_impl,
                                              tags=(OpTags.DONT_DCE,))
hip_fp8_delayed_update.not_capturable = True  # may all-reduce over the data-parallel group


def _fp8_cast_meta(t, e5m2, key=None, slot=None):
    C = t.shape[-1]
    R = 1
    for d in t.shape[:-1]:
        R *= d
    return (TensorProxy(like=t, shape=(R, C), dtype=torch.uint8, requires_grad=False),
            TensorProxy(like=t, shape=(), dtype=torch.float32, requires_grad=False))


def _fp8_cast_impl(t, e5m2):
    from ..ops.fp8 import quantize_rows

    return quantize_rows(t, e5m2)


def _fp8_cast_delayed_impl(t, e5m2, key, slot):
    from ..ops.fp8 import quantize_delayed_rows

    return quantize_delayed_rows(t, e5m2, key, slot)


def _fp8_gemm_layout_meta(qa, qb, sa, sb, fmt_a, at, out_shape, residual=None):
    return TensorProxy(like=qa, shape=tuple(out_shape), dtype=torch.bfloat16)


def _fp8_gemm_layout_impl(qa, qb, sa, sb, fmt_a, at, out_shape, residual=None):
    from ..ops.fp8 import gemm_fp8_layout

    return gemm_fp8_layout(qa, qb, sa, sb, fmt_a, at, residual).reshape(out_shape)


# row-major fp8 copies only: the backward GEMMs read the saved e4m3 activation / weight and the e5m2
# gradient in place (MN-major operands through ds_read_b64_tr_b8, csrc/gemm4_fp8.hip), so no
# transposed copy is ever written (LTA_FP8_TRANSPOSED=1: the cast_transpose path, A/B)
hip_fp8_cast = ex.register_operator("hip_fp8_cast", meta=_fp8_cast_meta, fn=_fp8_cast_impl)
hip_fp8_cast_delayed = ex.register_operator("hip_fp8_cast_delayed", meta=_fp8_cast_meta, fn=_fp8_cast_delayed_impl)
hip_fp8_gemm_layout = ex.register_operator("hip_fp8_gemm_layout", meta=_fp8_gemm_layout_meta,
                                           fn=_fp8_gemm_layout_impl)


def _rms_fp8_meta(x, w, eps, key, slot):
    q, sc = _fp8_cast_meta(x, False)
    return q, sc, TensorProxy(like=x, shape=(q.shape[0],), dtype=torch.float32, requires_grad=False)


def _rms_fp8_impl(x, w, eps, key, slot):
    from ..ops.fp8 import rms_norm_fwd_fp8_delayed

    return rms_norm_fwd_fp8_delayed(x, w, eps, key, slot)


def _swiglu_fp8_impl(a, b, key, slot):
    from ..ops.fp8 import swiglu_fwd_fp8_delayed

    return swiglu_fwd_fp8_delayed(a, b, key, slot)


def _swiglu_bwd_fp8_meta(g, a, b, key, slot_a, slot_b):
    qa, sa = _fp8_cast_meta(a, True)
    qb, sb = _fp8_cast_meta(b, True)
    return qa, sa, qb, sb


def _swiglu_bwd_fp8_impl(g, a, b, key, slot_a, slot_b):
    from ..ops.fp8 import swiglu_bwd_fp8_delayed

    return swiglu_bwd_fp8_delayed(g, a, b, key, slot_a, slot_b)


hip_swiglu_bwd_fp8 = ex.register_operator("hip_swiglu_bwd_fp8", meta=_swiglu_bwd_fp8_meta, fn=_swiglu_bwd_fp8_impl)

# producer-fused input casts of the fp8 linears (delayed scaling; _fuse_fp8_cast_producers)
hip_rms_norm_fwd_fp8 = ex.register_operator("hip_rms_norm_fwd_fp8", meta=_rms_fp8_meta, fn=_rms_fp8_impl)
hip_swiglu_fp8 = ex.register_operator("hip_swiglu_fp8", meta=lambda a, b, key, slot: _fp8_cast_meta(a, False),
                                      fn=_swiglu_fp8_impl)


def _delayed_cast(b, e5m2: bool):
    """The operands of ``b`` when it is the delayed-scaling row cast to e5m2 (gradients) / e4m3, else None."""
    if b.sym is not hip_fp8_cast_delayed:
        return None
    c = operands(b)
    return c if bool(c["e5m2"]) == e5m2 and c["key"] is not None else None


def _fp8_producer_fusion_off() -> bool:
    import os

    return os.environ.get("LTA_FP8_FUSE_PRODUCERS", "1") == "0"  # A/B hook


def _fuse_fp8_cast_producers(trace):
    """``y, rstd = hip_rms_norm_fwd(x, w, eps); q, s = hip_fp8_cast_delayed(y, False, key, slot)`` ->
    ``q, s, rstd = hip_rms_norm_fwd_fp8(x, w, eps, key, slot)``, and ``y = hip_swiglu(a, b)`` + its
    cast -> ``q, s = hip_swiglu_fp8(a, b, key, slot)`` when the cast is y's only use: the activation
    leaves the producing kernel as e4m3 (no bf16 round trip, no separate cast launch).  Parity: the
    reference's TransformerEngine layers quantise inside their fused norm / activation kernels
    (thunder/executors/transformer_engineex_impl.py)."""
    if _fp8_producer_fusion_off():
        return trace
    rw = Rewrite(trace, ex)
    for i, b in enumerate(rw.bsyms):
        c = _delayed_cast(b, e5m2=False)
        if c is None:
            continue
        y = c["t"]
        j = rw.producer(y)
        if j is None or rw.touched(j) or rw.uses(y) != 1:
            continue
        pb = rw.bsyms[j]
        p = operands(pb)
        if pb.sym is hip_rms_norm_fwd and p["weight"] is not None and pb.output[0].name == y.name:
            nb = hip_rms_norm_fwd_fp8.bind(p["x"], p["weight"], p["eps"], c["key"], c["slot"],
                                           output=(b.output[0], b.output[1], pb.output[1]))
        elif pb.sym is hip_swiglu:
            nb = hip_swiglu_fp8.bind(p["a"], p["b"], c["key"], c["slot"], output=b.output)
        else:
            continue
        rw.replace(j, nb)
        rw.drop(i)
    # backward: da, db = hip_swiglu_bwd(g, a, b) whose only uses are their e5m2 casts
    casts = {}
    for i, b in enumerate(rw.bsyms):
        c = _delayed_cast(b, e5m2=True)
        if c is not None:
            casts[c["t"].name] = (i, c)
    for j, pb in enumerate(rw.bsyms):
        if pb.sym is not hip_swiglu_bwd or rw.touched(j):
            continue
        da, db = pb.output
        if da.name not in casts or db.name not in casts or rw.uses(da) != 1 or rw.uses(db) != 1:
            continue
        (ia, ca), (ib, cb) = casts[da.name], casts[db.name]
        if ca["key"] != cb["key"]:
            continue
        p = operands(pb)
        rw.replace(j, hip_swiglu_bwd_fp8.bind(p["g"], p["a"], p["b"], ca["key"], ca["slot"], cb["slot"],
                                              output=(*rw.bsyms[ia].output, *rw.bsyms[ib].output)))
        rw.drop(ia, ib)
    return rw.finish(f"hipex: {rw.replaced} fp8 input cast(s) fused into their producers")


def _fp8_transposed() -> bool:
    import os

    return os.environ.get("LTA_FP8_TRANSPOSED", "0") == "1"


def _mx_quant_meta(t, e5m2):
    C = t.shape[-1]
    R = 1
    for d in t.shape[:-1]:
        R *= d
    u8 = torch.uint8
    mk = lambda shape: TensorProxy(like=t, shape=shape, dtype=u8, requires_grad=False)  # noqa: E731
    return mk((R, C)), mk((R, C // 32)), mk((C, R)), mk((C, R // 32))


def _mx_quant_impl(t, e5m2):
    from ..ops.fp8 import mx_quantize

    return mx_quantize(t, e5m2)


def _mx_gemm_meta(qa, sa, qb, sb, fmt_a, fmt_b, bias, out_shape):
    return TensorProxy(like=qa, shape=tuple(out_shape), dtype=torch.bfloat16)


def _mx_gemm_impl(qa, sa, qb, sb, fmt_a, fmt_b, bias, out_shape):
    from ..ops.fp8 import gemm_nt_mx

    return gemm_nt_mx(qa, sa, qb, sb, fmt_a, fmt_b, bias).reshape(out_shape)


# MXFP8: one pass emits both orientations with their 32-block E8M0 scales; the GEMM feeds the scales
# to the block-scaled MFMA per lane
hip_mx_quantize = ex.register_operator("hip_mx_quantize", meta=_mx_quant_meta, fn=_mx_quant_impl)
hip_mx_gemm = ex.register_operator("hip_mx_gemm", meta=_mx_gemm_meta, fn=_mx_gemm_impl)


def _mx_vjp(x, w, bias=None):
    from .. import torch as ltorch

    qx, sx, qxT, sxT = hip_mx_quantize(x, False)
    qw, sw, qwT, swT = hip_mx_quantize(w, False)
    y = hip_mx_gemm(qx, sx, qw, sw, 0, 0, bias, tuple(x.shape[:-1]) + (w.shape[0],))

    def bwd(g):
        qg, sg, qgT, sgT = hip_mx_quantize(g, True)
        dx = hip_mx_gemm(qg, sg, qwT, swT, 1, 0, None, tuple(x.shape))
        dw = hip_mx_gemm(qgT, sgT, qxT, sxT, 1, 0, None, tuple(w.shape))
        if bias is None:
            return dx, dw
        return dx, dw, ltorch.sum(g, tuple(range(g.ndim - 1)))

    return y, bwd


def _mx4_quant_meta(t):
    C = t.shape[-1]
    R = 1
    for d in t.shape[:-1]:
        R *= d
    u8 = torch.uint8
    return (TensorProxy(like=t, shape=(R, C // 2), dtype=u8, requires_grad=False),
            TensorProxy(like=t, shape=(R, C // 32), dtype=u8, requires_grad=False))


def _mx4_quant_impl(t):
    from ..ops.mxfp4 import quantize

    return quantize(t)


def _mx4_gemm_impl(qa, sa, qb, sb, bias, out_shape):
    from ..ops.mxfp4 import gemm_nt

    return gemm_nt(qa, sa, qb, sb, bias).reshape(out_shape)


# MXFP4 recipe: packed e2m1 + E8M0/32 operands of the forward GEMM (csrc/fp8.hip mx4 cast,
# csrc/gemm.hip gemm_nt_mxfp4_kernel)
hip_mx4_quantize = ex.register_operator("hip_mx4_quantize", meta=_mx4_quant_meta, fn=_mx4_quant_impl)
hip_mx4_gemm = ex.register_operator(
    "hip_mx4_gemm", meta=lambda qa, sa, qb, sb, bias, out_shape: TensorProxy(like=qa, shape=tuple(out_shape),
                                                                            dtype=torch.bfloat16),
    fn=_mx4_gemm_impl)


def _mx4_fwd(x, w, bias):
    qx4, sx4 = hip_mx4_quantize(x)
    qw4, sw4 = hip_mx4_quantize(w)
    return hip_mx4_gemm(qx4, sx4, qw4, sw4, bias, tuple(x.shape[:-1]) + (w.shape[0],))


def _mx4_vjp(x, w, bias=None):
    """MXFP4 forward, MXFP8 backward: the backward reads e4m3 MX copies of x^T and w^T."""
    from .. import torch as ltorch

    y = _mx4_fwd(x, w, bias)
    _, _, qxT, sxT = hip_mx_quantize(x, False)
    _, _, qwT, swT = hip_mx_quantize(w, False)

    def bwd(g):
        qg, sg, qgT, sgT = hip_mx_quantize(g, True)
        dx = hip_mx_gemm(qg, sg, qwT, swT, 1, 0, None, tuple(x.shape))
        dw = hip_mx_gemm(qgT, sgT, qxT, sxT, 1, 0, None, tuple(w.shape))
        if bias is None:
            return dx, dw
        return dx, dw, ltorch.sum(g, tuple(range(g.ndim - 1)))

    return y, bwd


def _quant(t, e5m2, key, slot):
    if key is None:
        return hip_fp8_quantize(t, e5m2)
    return hip_fp8_quantize_delayed(t, e5m2, key, slot)


def _cast(t, e5m2, key, slot):
    if key is None:
        return hip_fp8_cast(t, e5m2)
    return hip_fp8_cast_delayed(t, e5m2, key, slot)


def _fp8_vjp(x, w, bias=None, key=None, slots=None):
    from .. import torch as ltorch

    if key == "mxfp8":
        return _mx_vjp(x, w, bias)
    if key == "mxfp4":
        return _mx4_vjp(x, w, bias)
    sl = slots or (None, None, None)
    out_shape = tuple(x.shape[:-1]) + (w.shape[0],)
    if not _fp8_transposed():
        qx, sx = _cast(x, False, key, sl[0])
        qw, sw = _cast(w, False, key, sl[1])
        y = hip_fp8_gemm(qx, qw, sx, sw, 0, 0, bias, out_shape)

        def bwd_rows(g):
            qg, sg = _cast(g, True, key, sl[2])
            dx = hip_fp8_gemm_layout(qg, qw, sg, sw, 1, False, tuple(x.shape))  # dY [M, out] . W [out][in]
            dw = hip_fp8_gemm_layout(qg, qx, sg, sx, 1, True, tuple(w.shape))   # dY^T . X, both [tokens][.]
            if bias is None:
                return dx, dw
            return dx, dw, ltorch.sum(g, tuple(range(g.ndim - 1)))

        return y, bwd_rows
    qx, qxT, sx = _quant(x, False, key, sl[0])
    qw, qwT, sw = _quant(w, False, key, sl[1])
    y = hip_fp8_gemm(qx, qw, sx, sw, 0, 0, bias, out_shape)

    def bwd(g):
        qg, qgT, sg = _quant(g, True, key, sl[2])
        dx = hip_fp8_gemm(qg, qwT, sg, sw, 1, 0, None, tuple(x.shape))
        dw = hip_fp8_gemm(qgT, qxT, sg, sx, 1, 0, None, tuple(w.shape))
        if bias is None:
            return dx, dw
        db = ltorch.sum(g, tuple(range(g.ndim - 1)))
        return dx, dw, db

    return y, bwd


def _fp8_exec(x, w, bias=None, key=None, slots=None):
    if key == "mxfp8":
        qx, sx, _, _ = hip_mx_quantize(x, False)
        qw, sw, _, _ = hip_mx_quantize(w, False)
        return hip_mx_gemm(qx, sx, qw, sw, 0, 0, bias, tuple(x.shape[:-1]) + (w.shape[0],))
    if key == "mxfp4":
        return _mx4_fwd(x, w, bias)
    sl = slots or (None, None, None)
    qx, sx = _cast(x, False, key, sl[0])
    qw, sw = _cast(w, False, key, sl[1])
    return hip_fp8_gemm(qx, qw, sx, sw, 0, 0, bias, tuple(x.shape[:-1]) + (w.shape[0],))


def _register_fp8():
    from ..transforms.fp8 import fp8_linear, fp8_delayed_update, eligible
    from ..core.transforms import register_vjp

    ex.register_implementation(fp8_linear, checker=eligible, execution_transform=_fp8_exec)
    register_vjp(fp8_linear)(_fp8_vjp)
    ex.register_implementation(fp8_delayed_update, hip_fp8_delayed_update)


_register_fp8()


def _residual_adds(b):
    """``(y, r)`` and ``(r, y)`` when ``b`` is ``y + r`` of two tensors of its output's shape (no alpha)."""
    if b.sym.name not in ("torch_add", "add") or b.kwargs.get("alpha") not in (None, 1):
        return ()
    if len(b.args) < 2 or not all(isinstance(a, TensorProxy) for a in b.args[:2]):
        return ()
    y, r = b.args[:2]
    if tuple(r.shape) != tuple(y.shape) or r.dtype != y.dtype or tuple(b.output.shape) != tuple(y.shape):
        return ()
    return (y, r), (r, y)


def _fuse_linear_epilogues(trace):
    """``y = hip_linear(x, w, b); z = y + r`` (y used nowhere else) -> ``z = hip_linear(x, w, b, r)``:
    the residual add runs in the GEMM's epilogue (one HBM round trip of y saved)."""
    rw = Rewrite(trace, ex)
    for i, b in enumerate(rw.bsyms):
        for y, r in _residual_adds(b):
            j = rw.producer(y)
            if j is None or rw.touched(j) or rw.uses(y) != 1:
                continue
            lb = rw.bsyms[j]
            if lb.sym not in (hip_linear, hip_matmul, hip_fp8_gemm, hip_fp8_gemm_layout):
                continue
            p = operands(lb)
            if p["residual"] is not None or p.get("act") is not None or p.get("at"):
                continue  # the fp8 layout GEMM has its residual epilogue for the dgrad layout (A [M][K]) only
            # hip_matmul is computed where the GEMM was (the add's consumers come later), the others where
            # the add was (every input of the GEMM exists there); the residual must exist at that place
            at, gone = (j, i) if lb.sym is hip_matmul else (i, j)
            if rw.producer(r, -1) > (i if lb.sym in (hip_fp8_gemm, hip_fp8_gemm_layout) else j):
                continue
            head = list(p.values())[:list(p).index("residual")]
            rw.replace(at, lb.sym.bind(*head, r, output=b.output))
            rw.drop(gone)
            break
    return rw.finish(f"hipex: {rw.replaced} residual add(s) fused into GEMM epilogues")


# =========================================================================================
# K2b decode GEMV with fused prologues (rmsnorm) / gated epilogues (SwiGLU up-projection pair)
# =========================================================================================
def _as_rows(x, residual=None):
    """x as [rows, K] and the residual, if any, as [rows, N]: what the decode launchers take."""
    return x.reshape(-1, x.shape[-1]), None if residual is None else residual.reshape(-1, residual.shape[-1])


def _like(x, outs, packed=True):
    """Row results back under x's leading dims: one tensor (a single or packed launch) or one per weight."""
    if packed:
        return outs.reshape(*x.shape[:-1], outs.shape[-1])
    return tuple(o.reshape(*x.shape[:-1], o.shape[-1]) for o in outs)


def _decode_linear_meta(x, w, bias=None, residual=None, act=None, gate_weight=None, norm=False, norm_weight=None,
                        eps=1e-5):
    return TensorProxy(like=x, shape=tuple(x.shape[:-1]) + (w.shape[0],))


def _decode_linear_impl(x, w, bias=None, residual=None, act=None, gate_weight=None, norm=False, norm_weight=None,
                        eps=1e-5):
    from ..ops.gemm import gemv_nt, gemv_supported, _torch_linear

    x2, r2 = _as_rows(x, residual)
    ok = gemv_supported(x2, w, bias, r2) and (gate_weight is None or gate_weight.stride() == w.stride())
    if ok and norm_weight is not None:
        ok = norm_weight.is_contiguous() and norm_weight.dtype == x.dtype
    if ok:
        return _like(x, gemv_nt(x2, w, bias=bias, residual=r2, act=act, gate_weight=gate_weight, norm=norm,
                                norm_weight=norm_weight, eps=eps))
    if norm:  # unaligned operands: the same math on the library path
        from ..ops.rmsnorm import rms_norm_fwd

        x2, _ = rms_norm_fwd(x2, norm_weight, eps)
    if gate_weight is not None:
        y = _torch_linear(x2, w, None, None, act) * torch.nn.functional.linear(x2, gate_weight)
    else:
        y = _torch_linear(x2, w, bias, r2, act)
    return _like(x, y)


hip_decode_linear = ex.register_operator("hip_decode_linear", meta=_decode_linear_meta, fn=_decode_linear_impl)
_GEMV_MAX_ROWS = 8


def _rows(t) -> int:
    r = 1
    for d in t.shape[:-1]:
        r *= d
    return r


def _decode_group_meta(x, weights, norm=False, norm_weight=None, eps=1e-5, packed=False):
    if packed:
        return TensorProxy(like=x, shape=tuple(x.shape[:-1]) + (sum(w.shape[0] for w in weights),))
    return tuple(TensorProxy(like=x, shape=tuple(x.shape[:-1]) + (w.shape[0],)) for w in weights)


def _decode_group_impl(x, weights, norm=False, norm_weight=None, eps=1e-5, packed=False):
    from ..ops.gemm import gemv_group, gemv_supported

    x2, _ = _as_rows(x)
    ok = all(gemv_supported(x2, w) for w in weights)
    if ok and norm_weight is not None:
        ok = norm_weight.is_contiguous() and norm_weight.dtype == x.dtype
    if ok:
        outs = gemv_group(x2, list(weights), norm=norm, norm_weight=norm_weight, eps=eps, packed=packed)
    else:
        if norm:
            from ..ops.rmsnorm import rms_norm_fwd

            x2, _ = rms_norm_fwd(x2, norm_weight, eps)
        outs = [torch.nn.functional.linear(x2, w) for w in weights]
        if packed:
            outs = torch.cat(outs, -1)
    return _like(x, outs, packed)


hip_decode_linear_group = ex.register_operator("hip_decode_linear_group", meta=_decode_group_meta,
                                               fn=_decode_group_impl)


# =========================================================================================
# MXFP4 decode GEMV (lta::mxfp4_linear with <= 8 rows) with the same prologue / epilogues / groups
# =========================================================================================
def _mxfp4_decode_linear_meta(x, q, s, bias=None, residual=None, act=None, gate_q=None, gate_s=None, norm=False,
                              norm_weight=None, eps=1e-5):
    return TensorProxy(like=x, shape=tuple(x.shape[:-1]) + (q.shape[0],))


def _mxfp4_decode_linear_impl(x, q, s, bias=None, residual=None, act=None, gate_q=None, gate_s=None, norm=False,
                              norm_weight=None, eps=1e-5):
    from ..ops import mxfp4 as mx

    x2, r2 = _as_rows(x, residual)
    kw = dict(bias=bias, residual=r2, act=act, gate_q=gate_q, gate_s=gate_s)
    if mx.gemv_fused_supported(x2, q, s, norm_weight=norm_weight, **kw):
        y = mx.gemv_fused(x2, q, s, norm=norm, norm_weight=norm_weight, eps=eps, **kw)
    else:  # operands the kernel does not take (alignment, > 8 rows): the same math in torch
        y = mx.gemv_fused_reference(x2, q, s, norm=norm, norm_weight=norm_weight, eps=eps, **kw)
    return _like(x, y)


def _mxfp4_decode_group_meta(x, weights, norm=False, norm_weight=None, eps=1e-5, packed=False):
    if packed:
        return TensorProxy(like=x, shape=tuple(x.shape[:-1]) + (sum(q.shape[0] for q, _ in weights),))
    return tuple(TensorProxy(like=x, shape=tuple(x.shape[:-1]) + (q.shape[0],)) for q, _ in weights)


def _mxfp4_decode_group_impl(x, weights, norm=False, norm_weight=None, eps=1e-5, packed=False):
    from ..ops import mxfp4 as mx

    x2, _ = _as_rows(x)
    if all(mx.gemv_fused_supported(x2, q, s, norm_weight=norm_weight) for q, s in weights):
        outs = mx.gemv_group(x2, list(weights), norm=norm, norm_weight=norm_weight, eps=eps, packed=packed)
    else:
        outs = [mx.gemv_fused_reference(x2, q, s, norm=norm, norm_weight=norm_weight, eps=eps) for q, s in weights]
        if packed:
            outs = torch.cat(outs, -1)
    return _like(x, outs, packed)


hip_mxfp4_decode_linear = ex.register_operator("hip_mxfp4_decode_linear", meta=_mxfp4_decode_linear_meta,
                                               fn=_mxfp4_decode_linear_impl)
hip_mxfp4_decode_linear_group = ex.register_operator("hip_mxfp4_decode_linear_group", meta=_mxfp4_decode_group_meta,
                                                     fn=_mxfp4_decode_group_impl)
# The norm prologue is recomputed by every wave of the 4-bit GEMV; it pays only while the launch is
# weight-bound (profiles/mxfp4_decode_fusion.txt: a win at 1 row, a loss from 2 rows on the 12288 x
# 4096 qkv weight and at 8 rows on every site), so the pass folds the norm for single-row decode only.
_MXFP4_NORM_MAX_ROWS = 1
_MXFP4_LINEAR_IDS = ("custom_op.lta::mxfp4_linear", "custom_op.custom_op_impl_custom_op_lta_mxfp4_linear")


# =========================================================================================
# Decode fusion: one rewrite for both weight kinds, over operand records of the candidate projections
# =========================================================================================
def _decode_record(b, x, w, bias=None, residual=None, act=None, gate=None, norm=False, norm_weight=None, eps=1e-5):
    """The operands of a decode projection, or None unless it runs <= 8 rows against a 2-D weight."""
    if not all(isinstance(v, TensorProxy) for v in (x, *w, b.output)) or _rows(x) > _GEMV_MAX_ROWS or w[0].ndim != 2:
        return None
    return dict(x=x, w=w, bias=bias, residual=residual, act=act, gate=gate, norm=bool(norm), norm_weight=norm_weight,
                eps=eps, out=b.output, fused=False)


def _bf16_decode_candidate(b):
    if b.sym is hip_linear:
        p = operands(b)
        return _decode_record(b, p["x"], (p["w"],), p["bias"], p["residual"], p["act"])
    if b.sym is hip_decode_linear:
        p = operands(b)
        gate = None if p["gate_weight"] is None else (p["gate_weight"],)
        return _decode_record(b, p["x"], (p["w"],), p["bias"], p["residual"], p["act"], gate, p["norm"],
                              p["norm_weight"], p["eps"])
    return None


def _mxfp4_decode_candidate(b):
    if b.sym.id not in _MXFP4_LINEAR_IDS:
        return None
    p = operands(b, ("x", "q", "s", "bias", "fp4_activations"))
    x, bias = p["x"], p["bias"]
    if not isinstance(x, TensorProxy) or x.device.type != "cuda" or x.dtype != torch.bfloat16:
        return None
    if any(getattr(v, "requires_grad", False) for v in (x, bias, b.output)):
        return None  # the op's autograd stays with the custom op
    return _decode_record(b, x, (p["q"], p["s"]), bias)


class _DecodeKind(NamedTuple):
    """What the decode fusion needs to know about a weight format."""
    candidate: Callable  # bound symbol -> operand record, or None
    linear: object  # the operator emitted for one record: (x, *w, bias, residual, act, *gate, norm, norm_weight, eps)
    group: object  # ... and for 2-3 sibling records: (x, weights, norm, norm_weight, eps[, packed])
    norm_max_rows: int
    lower: bool  # emit the records no fold touched as well (else their bound symbol stays)
    mul: tuple  # the names under which the written-out gate's mul / silu are matched
    silu: tuple
    switch: str | None = None  # environment variable that turns the pass off with "0" (A/B)


_BF16_DECODE = _DecodeKind(_bf16_decode_candidate, hip_decode_linear, hip_decode_linear_group, _GEMV_MAX_ROWS,
                           lower=False, mul=("mul",), silu=("silu",))
_MXFP4_DECODE = _DecodeKind(_mxfp4_decode_candidate, hip_mxfp4_decode_linear, hip_mxfp4_decode_linear_group,
                            _MXFP4_NORM_MAX_ROWS, lower=True, mul=("mul", "torch_mul"), silu=("silu", "torch_silu"),
                            switch="LTA_MXFP4_DECODE_FUSION")


def _silu_arg(b, names):
    """``a`` when ``b`` is the out-of-place ``silu(a)`` of a tensor, else None."""
    if b.sym.name not in names or not b.args or (len(b.args) > 1 and b.args[1] not in (False, None)):
        return None
    return b.args[0] if isinstance(b.args[0], TensorProxy) else None


def _last_dim_cat_parts(b):
    """The two or three tensors of a ``cat`` along the last dim, else None."""
    if b.sym.name not in ("cat", "torch_cat", "cat_prim") or not b.args or not isinstance(b.args[0], (list, tuple)):
        return None
    parts = b.args[0]
    dim = b.args[1] if len(b.args) > 1 else b.kwargs.get("dim", 0)
    if not 2 <= len(parts) <= 3 or not all(isinstance(p, TensorProxy) for p in parts) or dim not in (-1, parts[0].ndim - 1):
        return None
    return parts


def _fuse_decode(trace, kind: _DecodeKind, folds, message: str):
    """Decode projections (<= 8 rows: the weight-streaming GEMVs) with what stands around them folded
    into the launch.  Every candidate becomes an operand record; a fold moves the record to the position
    of the consumer it absorbs, and the records are emitted at the end.  ``folds`` names the ones to run:

    * ``gate``: ``hip_swiglu(p(x, W1), p(x, W3))``, or written out ``mul(silu(a), b)`` (HF LlamaMLP), both
      projections plain and read nowhere else -> one record with ``act="silu"`` and W3 as its gate;
    * ``act``: ``silu(p(...))`` -> ``act="silu"``; ``residual``: ``p(...) + r`` -> the residual epilogue,
      emitted where the add was (r exists there);
    * ``norm``: ``hip_rms_norm_fwd`` of at most ``kind.norm_max_rows`` rows that feeds only records, as
      their x (rstd unused, literal eps) -> their norm prologue;
    * ``group``: two or three plain sibling records of one x and norm (attention q / k / v) -> one group
      launch, ``packed`` when a trailing ``cat(..., -1)`` is their only reader.
    Every launch removed is ~5 us of a ~1 ms decode step on MI355X (kernel floor + boundary)."""
    if kind.switch is not None and os.environ.get(kind.switch, "1") == "0":
        return trace
    rw = Rewrite(trace, ex)
    bsyms = rw.bsyms
    cand = {i: c for i, b in enumerate(bsyms) if (c := kind.candidate(b)) is not None}
    if not cand:
        return trace
    at = {c["out"].name: i for i, c in cand.items()}  # where the record that makes a value stands now
    group: dict[int, tuple] = {}  # position -> (member records, packed output or None)
    n = dict.fromkeys(("gate", "act", "residual", "norm", "group"), 0)

    def reads(c):
        return [v.name for v in (c["x"], *c["w"], c["bias"], c["residual"], *(c["gate"] or ()), c["norm_weight"])
                if isinstance(v, TensorProxy)]

    def plain(c):
        return c["gate"] is None and c["bias"] is None and c["residual"] is None and c["act"] is None

    def move(j, i, out, **changes):  # the record of position j is emitted at i (a consumer it absorbs)
        c = cand.pop(j)
        del at[c["out"].name]
        c.update(changes, out=out, fused=True)
        cand[i] = c
        at[out.name] = i
        rw.drop(j)

    def gate_pair(i, a, g, out):
        ja, jg = at.get(a.name), at.get(g.name)
        if ja is None or jg is None or ja == jg or rw.uses(a) != 1 or rw.uses(g) != 1:
            return False
        ca, cg = cand[ja], cand[jg]
        if ca["x"].name != cg["x"].name or not plain(ca) or not plain(cg) or ca["norm"] or cg["norm"]:
            return False
        if tuple(ca["w"][0].shape) != tuple(cg["w"][0].shape) or out.dtype != a.dtype:
            return False
        del cand[jg], at[g.name]
        rw.drop(jg)
        move(ja, i, out, act="silu", gate=cg["w"])
        n["gate"] += 1
        return True

    def untouched(i):
        return i not in cand and not rw.dropped(i)

    if "gate" in folds:
        for i, b in enumerate(bsyms):
            if not untouched(i) or len(b.args) != 2 or not all(isinstance(a, TensorProxy) for a in b.args):
                continue
            if b.sym is hip_swiglu:
                gate_pair(i, b.args[0], b.args[1], b.output)
            elif b.sym.name in kind.mul:
                for s_arg, g_arg in (b.args, b.args[::-1]):
                    js = rw.producer(s_arg)
                    if js is None or not untouched(js) or rw.uses(s_arg) != 1:
                        continue
                    a = _silu_arg(bsyms[js], kind.silu)
                    if a is not None and gate_pair(i, a, g_arg, b.output):
                        rw.drop(js)
                        break
    if "act" in folds:
        for i, b in enumerate(bsyms):
            a = _silu_arg(b, kind.silu) if untouched(i) else None
            j = at.get(a.name) if a is not None else None
            if j is None or rw.uses(a) != 1 or b.output.dtype != a.dtype:
                continue
            c = cand[j]
            if c["gate"] is None and c["act"] is None and c["residual"] is None:
                move(j, i, b.output, act="silu")
                n["act"] += 1
    if "residual" in folds:
        for i, b in enumerate(bsyms):
            for y, r in _residual_adds(b) if untouched(i) else ():
                j = at.get(y.name)
                if j is None or rw.uses(y) != 1 or y.name == r.name:
                    continue
                if cand[j]["gate"] is None and cand[j]["residual"] is None:
                    move(j, i, b.output, residual=r)
                    n["residual"] += 1
                    break
    if "norm" in folds:
        for i, b in enumerate(bsyms):
            if b.sym is not hip_rms_norm_fwd:
                continue
            p = operands(b)
            y, rstd = b.output
            if rw.uses(rstd) or not isinstance(p["eps"], (int, float)) or _rows(p["x"]) > kind.norm_max_rows:
                continue
            if any(untouched(k) for k in rw.consumers(y)):
                continue  # read by something that is no record
            readers = [c for c in cand.values() if y.name in reads(c)]
            if not readers or any(c["norm"] or c["x"].name != y.name or reads(c).count(y.name) != 1 for c in readers):
                continue
            for c in readers:
                c.update(x=p["x"], norm=True, norm_weight=p["weight"], eps=float(p["eps"]), fused=True)
            rw.drop(i)
            n["norm"] += 1
    if "group" in folds:
        sibs: dict = {}  # (x, norm) -> positions of the plain records, in program order
        for i in sorted(cand):
            c = cand[i]
            if plain(c):
                sibs.setdefault((c["x"].name, c["norm"], getattr(c["norm_weight"], "name", None), c["eps"]), []).append(i)
        for ci, cb in enumerate(bsyms):
            parts = _last_dim_cat_parts(cb) if untouched(ci) else None
            if parts is None:
                continue
            js = [at.get(p.name) for p in parts]
            if any(j is None or rw.uses(p) != 1 for j, p in zip(js, parts)) or len(set(js)) != len(js):
                continue
            key = next((k for k, idxs in sibs.items() if js[0] in idxs), None)
            if key is None or any(j not in sibs[key] for j in js):
                continue
            group[ci] = ([cand.pop(j) for j in js], cb.output)
            rw.drop(*js)
            sibs[key] = [j for j in sibs[key] if j not in js]
        for idxs in sibs.values():
            for c0 in range(0, len(idxs) - 1, 3):
                chunk = idxs[c0:c0 + 3]
                group[chunk[0]] = ([cand.pop(j) for j in chunk], None)  # x and the norm weight exist there
                rw.drop(*chunk[1:])
        n["group"] = len(group)

    for i, (members, packed_out) in group.items():
        c = members[0]
        ws = tuple(m["w"] if len(m["w"]) > 1 else m["w"][0] for m in members)
        if packed_out is not None:
            rw.replace(i, kind.group.bind(c["x"], ws, c["norm"], c["norm_weight"], c["eps"], True, output=packed_out))
        else:
            rw.replace(i, kind.group.bind(c["x"], ws, c["norm"], c["norm_weight"], c["eps"],
                                          output=tuple(m["out"] for m in members)))
    for i, c in cand.items():
        if kind.lower or c["fused"]:
            gate = c["gate"] or (None,) * len(c["w"])
            rw.replace(i, kind.linear.bind(c["x"], *c["w"], c["bias"], c["residual"], c["act"], *gate, c["norm"],
                                           c["norm_weight"], c["eps"], output=c["out"]))
    return rw.finish(message.format(**n))


def _qkv_rope_cache_meta(qkv, cos, sin, n_head, n_query_groups, head_size, rope_n, kc, vc, pos):
    B, T, _ = qkv.shape
    return TensorProxy(like=qkv, shape=(B, n_head, T, head_size)), TensorProxy(like=kc), TensorProxy(like=vc)


def _qkv_rope_cache_run(rope_args, caches, pos, stored, rows=False):
    """The cache-writing RoPE over ``caches`` in operator order (kc, vc, then scale caches): the kernel where its
    ``*_supported`` takes the operands, else the program as the model spells it (RoPE, then one write per buffer),
    with ``stored(t)`` the tensors k (or v) goes into its caches as.  ``rows``: ``pos`` is per token, int64 [B, T];
    ``rows="slots"``: the caches are the pools of a paged cache and ``pos`` holds every token's pool row."""
    from ..ops import fused
    from ..ops.kv_pages import write_slots
    from ..ops.kv_rows import write_rows

    qkv, cos, sin, _, *shape = rope_args
    if rows == "slots":
        ok = fused.qkv_rope_cache_slots_supported(qkv, cos, sin, *caches[:2], pos, *shape, *caches[2:])
        native, write = fused.qkv_rope_cache_slots_fwd, write_slots
    elif rows:
        ok = fused.qkv_rope_cache_rows_supported(qkv, cos, sin, *caches[:2], pos, *shape, *caches[2:])
        native, write = fused.qkv_rope_cache_rows_fwd, write_rows
    else:
        supported = fused.qkv_rope_cache_scaled_supported if len(caches) == 4 else fused.qkv_rope_cache_supported
        ok, native = supported(qkv, *caches, pos, *shape), fused.qkv_rope_cache_fwd
        write = lambda c, p, t: c.index_copy_(2, p if p.dtype == torch.int64 else p.long(), t)  # int64 indices only
    if ok:
        return native(*rope_args, *caches[:2], pos, *caches[2:])
    q, k, v = _qkv_rope_impl(*rope_args)
    srcs = (t for pair in zip(stored(k), stored(v)) for t in pair)
    return (q, *(write(c, pos, t) for c, t in zip(caches, srcs)))


def _unscaled_stored(op: str, kc, vc):
    """``stored`` of ``_qkv_rope_cache_run`` for unscaled caches: k / v as they are, or their e4m3 bytes for uint8
    caches (models/litgpt.py KVCache); operator ``op`` refuses one of each."""
    from ..ops.kv8 import e4m3_bytes

    kv8 = kc.dtype == torch.uint8
    if kv8 != (vc.dtype == torch.uint8):
        raise ValueError(f"{op}: one of the two caches is uint8 (e4m3), the other is not")
    return (lambda t: (e4m3_bytes(t),)) if kv8 else (lambda t: (t,))


def _qkv_rope_cache_impl(qkv, cos, sin, n_head, n_query_groups, head_size, rope_n, kc, vc, pos):
    return _qkv_rope_cache_run((qkv, cos, sin, n_head, n_query_groups, head_size, rope_n), (kc, vc), pos,
                               _unscaled_stored("hip_qkv_rope_cache", kc, vc))


hip_qkv_rope_cache = ex.register_operator("hip_qkv_rope_cache", meta=_qkv_rope_cache_meta, fn=_qkv_rope_cache_impl,
                                          tags=(OpTags.DONT_DCE, OpTags.IN_PLACE))
hip_qkv_rope_cache.written_args = (7, 8)  # kc, vc; qkv/cos/sin/pos are only read


# the scaled e4m3 cache (ops/kv8.py): bytes and one scale byte per (token, kv head) row, all four written
def _qkv_rope_cache_s8_meta(qkv, cos, sin, n_head, n_query_groups, head_size, rope_n, kc, vc, k_scale, v_scale, pos):
    B, T, _ = qkv.shape
    return (TensorProxy(like=qkv, shape=(B, n_head, T, head_size)), TensorProxy(like=kc), TensorProxy(like=vc),
            TensorProxy(like=k_scale), TensorProxy(like=v_scale))


def _qkv_rope_cache_s8_impl(qkv, cos, sin, n_head, n_query_groups, head_size, rope_n, kc, vc, k_scale, v_scale, pos):
    from ..ops.kv8 import quantise_rows

    return _qkv_rope_cache_run((qkv, cos, sin, n_head, n_query_groups, head_size, rope_n),
                               (kc, vc, k_scale, v_scale), pos, quantise_rows)


hip_qkv_rope_cache_s8 = ex.register_operator("hip_qkv_rope_cache_s8", meta=_qkv_rope_cache_s8_meta,
                                             fn=_qkv_rope_cache_s8_impl, tags=(OpTags.DONT_DCE, OpTags.IN_PLACE))
hip_qkv_rope_cache_s8.written_args = (7, 8, 9, 10)  # kc, vc, k_scale, v_scale


# Ragged batches: one int64 position per (sequence, token), ``pos`` [B, T], with cos / sin [B, T, rope_n] gathered per
# token (ops/kv_rows.py).  The operators mirror the two above, over the per-row entries of csrc/rope.hip.
def _qkv_rope_cache_rows_impl(qkv, cos, sin, n_head, n_query_groups, head_size, rope_n, kc, vc, pos):
    return _qkv_rope_cache_run((qkv, cos, sin, n_head, n_query_groups, head_size, rope_n), (kc, vc), pos,
                               _unscaled_stored("hip_qkv_rope_cache_rows", kc, vc), rows=True)


def _qkv_rope_cache_rows_s8_impl(qkv, cos, sin, n_head, n_query_groups, head_size, rope_n, kc, vc, k_scale, v_scale,
                                 pos):
    from ..ops.kv8 import quantise_rows

    return _qkv_rope_cache_run((qkv, cos, sin, n_head, n_query_groups, head_size, rope_n),
                               (kc, vc, k_scale, v_scale), pos, quantise_rows, rows=True)


hip_qkv_rope_cache_rows = ex.register_operator("hip_qkv_rope_cache_rows", meta=_qkv_rope_cache_meta,
                                               fn=_qkv_rope_cache_rows_impl, tags=(OpTags.DONT_DCE, OpTags.IN_PLACE))
hip_qkv_rope_cache_rows.written_args = (7, 8)
hip_qkv_rope_cache_rows_s8 = ex.register_operator("hip_qkv_rope_cache_rows_s8", meta=_qkv_rope_cache_s8_meta,
                                                  fn=_qkv_rope_cache_rows_s8_impl,
                                                  tags=(OpTags.DONT_DCE, OpTags.IN_PLACE))
hip_qkv_rope_cache_rows_s8.written_args = (7, 8, 9, 10)
# A paged cache (ops/kv_pages.py): the caches are pools [ng, R + 1, hs] and ``slots`` int64 [B, T] holds every token's
# pool row; the same per-row entries of csrc/rope.hip, with the pools' (0, head, row) strides and the capacity R.
def _qkv_rope_cache_slots_meta(qkv, cos, sin, n_head, n_query_groups, head_size, rope_n, kp, vp, slots):
    return _qkv_rope_cache_meta(qkv, cos, sin, n_head, n_query_groups, head_size, rope_n, kp, vp, slots)


def _qkv_rope_cache_slots_impl(qkv, cos, sin, n_head, n_query_groups, head_size, rope_n, kp, vp, slots):
    return _qkv_rope_cache_run((qkv, cos, sin, n_head, n_query_groups, head_size, rope_n), (kp, vp), slots,
                               _unscaled_stored("hip_qkv_rope_cache_slots", kp, vp), rows="slots")


def _qkv_rope_cache_slots_s8_impl(qkv, cos, sin, n_head, n_query_groups, head_size, rope_n, kp, vp, k_scale, v_scale,
                                  slots):
    from ..ops.kv8 import quantise_rows

    return _qkv_rope_cache_run((qkv, cos, sin, n_head, n_query_groups, head_size, rope_n),
                               (kp, vp, k_scale, v_scale), slots, quantise_rows, rows="slots")


hip_qkv_rope_cache_slots = ex.register_operator("hip_qkv_rope_cache_slots", meta=_qkv_rope_cache_slots_meta,
                                                fn=_qkv_rope_cache_slots_impl, tags=(OpTags.DONT_DCE, OpTags.IN_PLACE))
hip_qkv_rope_cache_slots.written_args = (7, 8)
hip_qkv_rope_cache_slots_s8 = ex.register_operator("hip_qkv_rope_cache_slots_s8", meta=_qkv_rope_cache_s8_meta,
                                                   fn=_qkv_rope_cache_slots_s8_impl,
                                                   tags=(OpTags.DONT_DCE, OpTags.IN_PLACE))
hip_qkv_rope_cache_slots_s8.written_args = (7, 8, 9, 10)
_KV_PAGED_GATHER_IDS = ("custom_op.lta::kv_paged_gather", "custom_op.custom_op_impl_custom_op_lta_kv_paged_gather")
_KV_PAGED_MASK_IDS = ("custom_op.lta::kv_paged_mask", "custom_op.custom_op_impl_custom_op_lta_kv_paged_mask")
_KV_POSITION_MASK_IDS = ("custom_op.lta::kv_position_mask", "custom_op.custom_op_impl_custom_op_lta_kv_position_mask")
# the same two masks under a sliding window (a trailing ``window``): read wherever those are
_KV_WINDOW_MASK_IDS = ("custom_op.lta::kv_window_mask", "custom_op.custom_op_impl_custom_op_lta_kv_window_mask")
_KV_PAGED_WINDOW_MASK_IDS = ("custom_op.lta::kv_paged_window_mask",
                             "custom_op.custom_op_impl_custom_op_lta_kv_paged_window_mask")
_CACHE_WRITES = ("index_copy_inplace", "scatter_rows_inplace")  # shared positions / one position per token
_KV8_QUANTISE_IDS = ("custom_op.lta::kv8_quantise_rows", "custom_op.custom_op_impl_custom_op_lta_kv8_quantise_rows")
_KV8_DEQUANTISE_IDS = ("custom_op.lta::kv8_dequantise_rows",
                       "custom_op.custom_op_impl_custom_op_lta_kv8_dequantise_rows")


def _kv8_fusion_off() -> bool:
    """LTA_KV8_FUSION=0 keeps the e4m3 KV cache's quantising writes and dequantising reads as the
    separate operations the model spells (A/B against the two fused kernels)."""
    return os.environ.get("LTA_KV8_FUSION", "1") == "0"


def _kv_pos_fusion_off() -> bool:
    """LTA_KV_POS_FUSION=0 keeps a ragged batch's position mask and per-row cache writes as the separate operations
    the model spells (A/B against the per-row RoPE write and the position mode of the decode kernels)."""
    return os.environ.get("LTA_KV_POS_FUSION", "1") == "0"


def _kv_paged_fusion_off() -> bool:
    """LTA_KV_PAGED_FUSION=0 keeps a paged cache's slot writes, page gathers and mask as the separate operations the
    model spells (A/B against the slot-writing RoPE and the paged mode of the decode kernels)."""
    return os.environ.get("LTA_KV_PAGED_FUSION", "1") == "0"


def _kv_window_fusion_off() -> bool:
    """LTA_KV_WINDOW_FUSION=0 keeps the masks of a model's sliding-window layers (``lta::kv_window_mask``,
    ``lta::kv_paged_window_mask``) and the masked kernels that read them (A/B against the window mode of the decode
    and prefill kernels); the layers without a window are fused as ever."""
    return os.environ.get("LTA_KV_WINDOW_FUSION", "1") == "0"


def _window_of(mask_bsym, names):
    """``(operands by name, window)`` of a position or paged mask: window None for the plain mask; None instead of
    the pair for a window mask that is switched off or whose window is not a plain int >= 1."""
    if mask_bsym.sym.id not in (*_KV_WINDOW_MASK_IDS, *_KV_PAGED_WINDOW_MASK_IDS):
        return operands(mask_bsym, names), None
    p = operands(mask_bsym, (*names, "window"))
    w = p["window"]
    if _kv_window_fusion_off() or isinstance(w, (Proxy, bool)) or not isinstance(w, int) or w < 1:
        return None
    return p, w


def _window_form(op, window):
    """``(operator, its operands between the key selector and scale)`` for a fused form under ``window``."""
    return (op, ()) if window is None else (_WINDOW_FORMS[op], (window,))


def _ints_of(args):
    """The ints of ``f(x, 1, 0, 2)`` or ``f(x, (1, 0, 2))`` after the tensor, None for anything else."""
    rest = args[1:]
    if len(rest) == 1 and isinstance(rest[0], (tuple, list)):
        rest = rest[0]
    return tuple(rest) if all(isinstance(n, int) and not isinstance(n, bool) for n in rest) else None


def _slot_relayout(rw, t):
    """``(permute position, reshape position, the [H, B * T, D] tensor)`` when ``t`` [B, H, T, D] is read once, by
    ``permute(t, 1, 0, 2, 3)``, whose result is read once by ``reshape(., H, B * T, D)`` (the layout a paged
    cache's pools are written in, ops/kv_pages.py ``write_slots``); None for anything else."""
    if getattr(t, "ndim", 0) != 4:
        return None
    B, H, T, D = t.shape
    found = []
    for names, ints, shape in ((("permute", "torch_permute"), (1, 0, 2, 3), (H, B, T, D)),
                               (("reshape", "torch_reshape"), (H, B * T, D), (H, B * T, D))):
        if rw.uses(t) != 1:
            return None
        (j,) = rw.consumers(t)
        b = rw.bsyms[j]
        if rw.touched(j) or b.sym.name not in names or b.kwargs or not b.args or b.args[0] is not t:
            return None
        if _ints_of(b.args) != ints or not isinstance(b.output, TensorProxy) or tuple(b.output.shape) != shape:
            return None
        found.append(j)
        t = b.output
    return (*found, t)


def _flat_slots(rw, index):
    """``(slots, reshape position)`` when ``index = reshape(slots, -1)`` of int64 ``slots`` [B, T], else None."""
    j = rw.producer(index)
    if j is None or rw.touched(j):
        return None
    b = rw.bsyms[j]
    if b.sym.name not in ("reshape", "torch_reshape") or b.kwargs or not b.args or _ints_of(b.args) != (-1,):
        return None
    slots = b.args[0]
    if not isinstance(slots, TensorProxy) or slots.dtype != torch.int64 or slots.ndim != 2:
        return None
    return slots, j


def _only_tensor_arg(b, rest=0):
    """``b``'s tensor operand when it is called as ``op(tensor, <rest literals>)`` with no keywords."""
    if b.kwargs or len(b.args) != 1 + rest or not isinstance(b.args[0], TensorProxy):
        return None
    return b.args[0]


def _e4m3_quantise_chain(rw, t):
    """``[clamp, to, view]`` positions when ``t`` is read once, by ``clamp(t, -448.0, 448.0)``, whose
    result is read once by ``to(float8_e4m3fn)``, whose result is read once by ``view(uint8)``; the
    uint8 tensor is the last one's output.  None for anything else: other bounds, no clamp or another
    fp8 format would give other bytes than the kernel's saturating e4m3 conversion."""
    chain = []
    for names, rest in ((("clamp", "torch_clamp"), (-E4M3_MAX, E4M3_MAX)),
                        (("to", "torch_to"), (torch.float8_e4m3fn,)),
                        (("view", "torch_view"), (torch.uint8,))):
        if rw.uses(t) != 1:
            return None
        (j,) = rw.consumers(t)
        b = rw.bsyms[j]
        if rw.touched(j) or b.sym.name not in names or _only_tensor_arg(b, len(rest)) is not t:
            return None
        for got, want in zip(b.args[1:], rest):
            if isinstance(want, float):
                if isinstance(got, bool) or not isinstance(got, (int, float)) or float(got) != want:
                    return None
            elif got is not want:
                return None
        if not isinstance(b.output, TensorProxy):
            return None
        chain.append(j)
        t = b.output
    return chain


def _cache_sources(rw, t):
    """How the ``hip_qkv_rope`` result ``t`` (read once) reaches its cache, as ``(kind, the tensors that
    are copied, the links to drop)``: "plain", ``t`` itself; "e4m3", the uint8 end of
    ``_e4m3_quantise_chain``; "scaled", the two outputs of ``kv8_quantise_rows``.  None for anything
    else, and for both e4m3 kinds under LTA_KV8_FUSION=0."""
    (j,) = rw.consumers(t)
    b = rw.bsyms[j]
    if b.sym.name in _CACHE_WRITES or _slot_relayout(rw, t) is not None:  # written as it is (a paged cache: relaid)
        return "plain", (t,), ()
    if _kv8_fusion_off():
        return None
    if b.sym.id in _KV8_QUANTISE_IDS:
        outs = b.output
        if rw.touched(j) or _only_tensor_arg(b) is not t or not isinstance(outs, (tuple, list)) or len(outs) != 2:
            return None
        return ("scaled", tuple(outs), (j,)) if all(isinstance(o, TensorProxy) for o in outs) else None
    chain = _e4m3_quantise_chain(rw, t)
    return None if chain is None else ("e4m3", (rw.bsyms[chain[-1]].output,), tuple(chain))


def _fuse_kv_cache_writes(trace):
    """``q, k, v = hip_qkv_rope(...); kc = index_copy_inplace(cache_k, 2, pos, k);
    vc = index_copy_inplace(cache_v, 2, pos, v)`` (k, v used nowhere else) ->
    ``q, kc, vc = hip_qkv_rope_cache(..., cache_k, cache_v, pos)``: the rotated keys and the values
    are stored straight into the static caches by the RoPE kernel (two launches fewer per layer).

    With uint8 (unscaled e4m3) caches k and v reach their write through
    ``clamp(-448, 448) -> to(float8_e4m3fn) -> view(uint8)``, every link read once; the kernel
    converts in the same launch (eight launches fewer per layer).

    With the scaled e4m3 cache k and v each pass through ``kv8_quantise_rows`` and their bytes and scale
    bytes through four ``index_copy_inplace``: ``hip_qkv_rope_cache_s8``.

    k and v must reach their caches the same way (``_cache_sources``), and every copied tensor is read
    once, by an ``index_copy_inplace`` along dim 2 at one int64 ``pos`` into a buffer of its dtype.
    Anything else (a result read twice, another position, v through another format) stays.

    A ragged batch the same way: the RoPE takes cos / sin ``[B, T, rope_n]``, every copied tensor is read once by a
    ``scatter_rows_inplace`` at one int64 ``pos`` ``[B, T]``, and the result is ``hip_qkv_rope_cache_rows`` (or
    ``hip_qkv_rope_cache_rows_s8``).  LTA_KV_POS_FUSION=0 leaves those writes alone.

    A paged cache (ops/kv_pages.py), again with cos / sin ``[B, T, rope_n]``: every copied tensor is read once by the
    ``[H, B * T, D]`` relayout (``_slot_relayout``), and that once by ``index_copy_inplace(pool, 1, reshape(slots,
    -1), .)`` into a 3-D pool of its dtype, all at one int64 ``slots`` ``[B, T]``: ``hip_qkv_rope_cache_slots`` (or
    ``hip_qkv_rope_cache_slots_s8``).  The relayouts go; ``reshape(slots, -1)`` goes with its last reader.
    LTA_KV_PAGED_FUSION=0 leaves those writes alone."""
    rw = Rewrite(trace, ex)
    flats = set()  # positions of the reshape(slots, -1) whose writes were folded
    for i, b in enumerate(rw.bsyms):
        if b.sym is not hip_qkv_rope:
            continue
        q, k, v = b.output
        if rw.uses(k) != 1 or rw.uses(v) != 1:
            continue
        sk, sv = _cache_sources(rw, k), _cache_sources(rw, v)
        if sk is None or sv is None or sk[0] != sv[0]:
            continue
        srcs = [t for pair in zip(sk[1], sv[1]) for t in pair]  # the operators' order: k, v, then their scales
        copies, pos = [], None
        rows = getattr(b.args[1], "ndim", 2) == 3  # cos [B, T, rope_n]: one position per token
        relayouts = [_slot_relayout(rw, t) if rows else None for t in srcs]
        paged = relayouts[0] is not None  # the writes of a paged cache: all of one kind, or nothing is folded
        if any((r is not None) != paged for r in relayouts):
            continue
        if rows and (_kv_paged_fusion_off() if paged else _kv_pos_fusion_off()):
            continue
        links, flat_at = [], set()
        for t, relayout in zip(srcs, relayouts):
            if paged:
                *hops, t = relayout
                links += hops
            if rw.uses(t) != 1:
                break
            (j,) = rw.consumers(t)
            c = rw.bsyms[j]
            if rw.touched(j) or c.sym.name != _CACHE_WRITES[rows and not paged]:
                break
            w = operands(c)
            buf, index = w["buf"], w["pos" if rows and not paged else "index"]
            if not (rows and not paged) and w["dim"] != (1 if paged else 2):
                break
            if w["src"] is not t or not isinstance(buf, TensorProxy) or buf.dtype != t.dtype:
                break
            if paged:  # a pool [ng, R + 1, hs], written at reshape(slots, -1)
                flat = _flat_slots(rw, index) if isinstance(index, TensorProxy) else None
                if flat is None or buf.ndim != 3:
                    break
                index = flat[0]
                flat_at.add(flat[1])
            if pos is None:
                pos = index
                if not isinstance(pos, TensorProxy) or pos.dtype != torch.int64 or (rows and pos.ndim != 2):
                    break
            elif getattr(index, "name", None) != pos.name:
                break
            copies.append((j, c.output, buf))
        if len(copies) != len(srcs):
            continue
        at_copies, outs, bufs = zip(*copies)
        # the fused op needs the caches and positions: emit it where the RoPE was when they exist
        # there (LitGPT), else at the last cache write (HF computes the positions after the RoPE),
        # provided nothing in between reads q and, as the earlier writes move later, nothing but the
        # writes themselves reads a written cache or a write's result
        ready = max(rw.producer(t, -1) for t in (*bufs, pos))
        at = i
        if ready >= i:
            at = max(at_copies)
            if any(i < j < at for j in rw.consumers(q)) or ready >= at:
                continue
            lo = min(at_copies)
            if any(lo < j < at and j not in at_copies for t in (*outs, *bufs) for j in rw.consumers(t)):
                continue
        op = ((hip_qkv_rope_cache, hip_qkv_rope_cache_s8), (hip_qkv_rope_cache_rows, hip_qkv_rope_cache_rows_s8),
              (hip_qkv_rope_cache_slots, hip_qkv_rope_cache_slots_s8))[rows + paged][sk[0] == "scaled"]
        rw.replace(at, op.bind(*b.args, *bufs, pos, output=(q, *outs)))
        rw.drop(*({i, *sk[2], *sv[2], *at_copies, *links} - {at}))
        flats |= flat_at
    for j in flats:  # reshape(slots, -1) is shared by the layers of a step: it goes with its last reader
        if all(rw.touched(c) for c in rw.consumers(rw.bsyms[j].output)):
            rw.drop(j)
    return rw.finish(f"hipex: {rw.replaced} KV-cache write pair(s) fused into RoPE")


def _e4m3_dequantised(rw, t, dtype):
    """``((cache,), view position, (to position, view position))`` when
    ``t = to(view(cache, float8_e4m3fn), dtype)`` of a uint8 ``cache``, else None: the caches read, where
    the first link stands, and the links to drop when nothing else reads them, innermost last."""
    j = rw.producer(t)
    if j is None or rw.touched(j):
        return None
    b = rw.bsyms[j]
    if b.sym.name not in ("to", "torch_to") or _only_tensor_arg(b, 1) is None or b.args[1] is not dtype:
        return None
    f = b.args[0]
    jv = rw.producer(f)
    if f.dtype != torch.float8_e4m3fn or jv is None or rw.touched(jv):
        return None
    bv = rw.bsyms[jv]
    if bv.sym.name not in ("view", "torch_view") or _only_tensor_arg(bv, 1) is None:
        return None
    if bv.args[1] is not torch.float8_e4m3fn or bv.args[0].dtype != torch.uint8:
        return None
    return (bv.args[0],), jv, (j, jv)


def _kv8_rows_dequantised(rw, t, dtype):
    """``((cache, scale cache), position, (position,))`` when ``t = kv8_dequantise_rows(cache, scales, dtype)``
    of uint8 operands, else None (the shape of ``_e4m3_dequantised``)."""
    j = rw.producer(t)
    if j is None or rw.touched(j):
        return None
    b = rw.bsyms[j]
    if b.sym.id not in _KV8_DEQUANTISE_IDS:
        return None
    p = operands(b, ("b", "scales", "dtype"))
    c, s = p["b"], p["scales"]
    if p["dtype"] is not dtype or not all(isinstance(x, TensorProxy) and x.dtype == torch.uint8 for x in (c, s)):
        return None
    return (c, s), j, (j,)


def _fuse_kv_position_reads(trace):
    """``mask = kv_position_mask(pos, S); hip_decode_attn(q, k, v, mask, False, scale)`` with ``S`` the keys' and
    ``pos`` int64 ``[B, T]`` -> ``hip_decode_attn_pos(q, k, v, pos, scale)``: the kernel takes every row's key count
    from its position, reads no mask and splits the row's live keys over all of its workgroups.  The mask is shared
    by the layers of a step: it must be read by such attentions only, and is dropped with the last of them.

    ``mask = kv_window_mask(pos, S, window)`` (the sliding-window layers of a step; a model with both kinds of layer
    holds both masks, each dropped with its own readers) -> ``hip_decode_attn_pos_win(q, k, v, pos, window, scale)``;
    LTA_KV_WINDOW_FUSION=0 leaves that mask and its readers alone."""
    if _kv_pos_fusion_off():
        return trace
    rw = Rewrite(trace, ex)
    for m, b in enumerate(rw.bsyms):
        if b.sym.id not in (*_KV_POSITION_MASK_IDS, *_KV_WINDOW_MASK_IDS) or rw.touched(m):
            continue
        pw = _window_of(b, ("input_pos", "S"))
        if pw is None:
            continue
        p, window = pw
        pos, S, mask = p["input_pos"], p["S"], b.output
        if not isinstance(pos, TensorProxy) or pos.dtype != torch.int64 or pos.ndim != 2 or isinstance(S, TensorProxy):
            continue
        readers = rw.consumers(mask)
        found = []
        for i in readers:
            a = rw.bsyms[i]
            if a.sym is not hip_decode_attn or rw.touched(i) or readers.count(i) != 1:
                break
            o = operands(a)
            q, k = o["q"], o["k"]
            if o["mask"] is not mask or o["causal"] or k.shape[2] != int(S):
                break
            if tuple(pos.shape) != (q.shape[0], q.shape[2]):
                break
            found.append((i, a, o))
        if not found or len(found) != len(readers):
            continue
        op, win = _window_form(hip_decode_attn_pos, window)
        for i, a, o in found:
            rw.replace(i, op.bind(o["q"], o["k"], o["v"], pos, *win, o["scale"], output=a.output))
        rw.drop(m)
    return rw.finish(f"hipex: {rw.replaced} decode attention(s) take their key counts from the positions")


def _fuse_kv8_reads(trace):
    """``hip_decode_attn(q, to(view(kc, float8_e4m3fn), q.dtype), to(view(vc, float8_e4m3fn), q.dtype), ...)``
    over uint8 caches -> ``hip_decode_attn_kv8(q, kc, vc, ...)``: the decode kernel unpacks the e4m3
    bytes itself, so a decode step neither converts nor re-reads the whole cache at 16 bits.  The
    dequantising view / to are dropped when nothing else reads them.

    The scaled cache the same way: ``hip_decode_attn(q, kv8_dequantise_rows(kc, ks, q.dtype),
    kv8_dequantise_rows(vc, vs, q.dtype), ...)`` -> ``hip_decode_attn_kv8s(q, kc, vc, ks, vs, ...)``.  k and v
    must be of one kind, and nothing may write a byte or scale cache in place between its dequantise and
    the attention.

    ``hip_decode_attn_pos`` folds the same chains into ``hip_decode_attn_kv8_pos`` / ``hip_decode_attn_kv8s_pos``,
    ``hip_decode_attn_pos_win`` into their ``_win`` forms."""
    if _kv8_fusion_off():
        return trace
    rw = Rewrite(trace, ex)
    for i, b in enumerate(rw.bsyms):
        if b.sym not in (hip_decode_attn, hip_decode_attn_pos, hip_decode_attn_pos_win):
            continue
        by_pos = b.sym is not hip_decode_attn
        p = operands(b)
        q = p["q"]
        win = (p["window"],) if b.sym is hip_decode_attn_pos_win else ()
        for op, resolve in (((hip_decode_attn_kv8s, hip_decode_attn_kv8s_pos)[by_pos], _kv8_rows_dequantised),
                            ((hip_decode_attn_kv8, hip_decode_attn_kv8_pos)[by_pos], _e4m3_dequantised)):
            rk, rv = resolve(rw, p["k"], q.dtype), resolve(rw, p["v"], q.dtype)
            if rk is not None and rv is not None:
                break
        else:
            continue
        caches = [c for pair in zip(rk[0], rv[0]) for c in pair]  # the operators' order: k, v, then their scales
        # the kernel reads the caches where the attention stands: nothing may write them after the first link
        first = min(rk[1], rv[1])
        if any(first < j < i and OpTags.IN_PLACE in (rw.bsyms[j].sym.tags or ())
               for c in caches for j in rw.consumers(c)):
            continue
        rest = (p["pos"], *win, p["scale"]) if by_pos else (p["mask"], p["causal"], p["scale"])
        if win:
            op = _WINDOW_FORMS[op]
        rw.replace(i, op.bind(q, *caches, *rest, output=b.output))
        for _, _, links in (rk, rv):
            for j in links:
                if rw.uses(rw.bsyms[j].output) != 1:
                    break
                rw.drop(j)
    return rw.finish(f"hipex: {rw.replaced} decode attention(s) read their e4m3 KV cache directly")


def _paged_gather(rw, t):
    """``(pool, table, page_size, position)`` when ``t = kv_paged_gather(pool, table, page_size)`` is read once,
    else None."""
    j = rw.producer(t)
    if j is None or rw.touched(j) or rw.bsyms[j].sym.id not in _KV_PAGED_GATHER_IDS or rw.uses(t) != 1:
        return None
    p = operands(rw.bsyms[j], ("pool", "table", "page_size"))
    if not all(isinstance(p[n], TensorProxy) for n in ("pool", "table")) or isinstance(p["page_size"], Proxy):
        return None
    return p["pool"], p["table"], p["page_size"], j


def _fuse_kv_paged_reads(trace):
    """``hip_decode_attn(q, kv_paged_gather(kp, table, page), kv_paged_gather(vp, table, page),
    kv_paged_mask(pos, table, page, num_pages), False, scale)`` -> ``hip_decode_attn_paged(q, kp, vp, pos, table, page,
    num_pages, scale)``: the kernel takes every key's pool row from the block table and every row's key count from its
    position, so a decode step neither gathers the logical cache nor builds a mask.  The same over
    ``hip_decode_attn_kv8`` / ``hip_decode_attn_kv8s``, whose byte (and scale) operands are gathers of the byte (and
    scale) pools: ``hip_decode_attn_kv8_paged`` / ``hip_decode_attn_kv8s_paged``.

    Every cache operand must be a gather read once, all at one table and page size, the mask a ``kv_paged_mask`` of
    that table, page size and int64 ``pos`` ``[B, T]``, and ``causal`` false; nothing may write a pool in place
    between its gather and the attention.  The gathers are dropped, and the mask with its last reader, when nothing
    else reads it.  LTA_KV_PAGED_FUSION=0 turns the pass off.

    Under ``kv_paged_window_mask(pos, table, page, num_pages, window)`` the same, into the ``_win`` forms with
    ``window`` ahead of ``scale``; LTA_KV_WINDOW_FUSION=0 leaves those attentions and their mask alone."""
    if _kv_paged_fusion_off():
        return trace
    rw = Rewrite(trace, ex)
    forms = {hip_decode_attn: (hip_decode_attn_paged, ("k", "v")),
             hip_decode_attn_kv8: (hip_decode_attn_kv8_paged, ("k8", "v8")),
             hip_decode_attn_kv8s: (hip_decode_attn_kv8s_paged, ("k8", "v8", "k_scale", "v_scale"))}
    masks = set()
    for i, b in enumerate(rw.bsyms):
        if b.sym not in forms or rw.touched(i):
            continue
        op, names = forms[b.sym]
        p = operands(b)
        q, mask = p["q"], p["mask"]
        if p["causal"] or not isinstance(mask, TensorProxy):
            continue
        m = rw.producer(mask)
        if m is None or rw.touched(m) or rw.bsyms[m].sym.id not in (*_KV_PAGED_MASK_IDS, *_KV_PAGED_WINDOW_MASK_IDS):
            continue
        pw = _window_of(rw.bsyms[m], ("pos", "table", "page_size", "num_pages"))
        if pw is None:
            continue
        pm, window = pw
        op, win = _window_form(op, window)
        pos, table = pm["pos"], pm["table"]
        if not isinstance(pos, TensorProxy) or pos.dtype != torch.int64 or not isinstance(table, TensorProxy):
            continue
        if any(isinstance(pm[n], Proxy) for n in ("page_size", "num_pages")):
            continue
        if tuple(pos.shape) != (q.shape[0], q.shape[2]):
            continue
        gathers = [_paged_gather(rw, p[n]) if isinstance(p[n], TensorProxy) else None for n in names]
        if any(g is None or g[1].name != table.name or g[2] != pm["page_size"] for g in gathers):
            continue
        # the kernel reads the pools where the attention stands: nothing may write them after their gather
        if any(g[3] < j < i and OpTags.IN_PLACE in (rw.bsyms[j].sym.tags or ())
               for g in gathers for j in rw.consumers(g[0])):
            continue
        rw.replace(i, op.bind(q, *(g[0] for g in gathers), pos, table, pm["page_size"], pm["num_pages"], *win,
                              p["scale"], output=b.output))
        rw.drop(*(g[3] for g in gathers))
        masks.add(m)
    for m in masks:  # one mask serves the layers of a step
        if all(rw.touched(j) and not rw.dropped(j) for j in rw.consumers(rw.bsyms[m].output)):
            rw.drop(m)
    return rw.finish(f"hipex: {rw.replaced} decode attention(s) read their paged KV cache through the block table")


def _kv_prefill_fusion_off() -> bool:
    """LTA_KV_PREFILL_FUSION=0 keeps a prefill against the KV cache (more than 16 query rows at 2-D positions) as the
    masked flash attention over the gathered / dequantised cache that the model spells (A/B against the prefill
    kernel).  The switches of the cache kinds hold here too: LTA_KV_POS_FUSION=0, LTA_KV_PAGED_FUSION=0 and
    LTA_KV8_FUSION=0 leave the prefill of their kind alone."""
    return os.environ.get("LTA_KV_PREFILL_FUSION", "1") == "0"


def _fuse_kv_prefill_reads(trace):
    """``hip_flash_attn_fwd_ex(q, k, v, mask, False, scale, 0.0, ...)`` whose LSE nobody reads, at head dim 64 / 128,
    with ``mask = kv_position_mask(pos, S)`` (``S`` the keys' length) or ``kv_paged_mask(pos, table, page, num_pages)``
    and ``pos`` int64 ``[B, T]`` -> ``hip_prefill_attn_pos(q, k, v, pos, scale)`` / ``hip_prefill_attn_paged(q, kp, vp,
    pos, table, page, num_pages, scale)``: the kernel takes every row's key count from its position (and every key's
    pool row from the block table), so a prefill builds no ``[B, 1, T, S]`` mask image, sweeps no key tile beyond its
    rows' positions, and neither gathers nor dequantises the cache.

    k / v are the raw cache, ``to(view(cache, float8_e4m3fn), q.dtype)`` of a uint8 cache (``_kv8`` forms) or
    ``kv8_dequantise_rows(cache, scales, q.dtype)`` (``_kv8s`` forms), both of one kind; under the paged mask every
    cache operand is a ``kv_paged_gather`` read once, all at the mask's table and page size (``PagedKVCache.forward``
    dequantises the gather of a pool).  Nothing may write a cache or pool in place between the first of those links
    and the attention.  The links are dropped when nothing else reads them, the mask (one serves the layers of a
    step) with its last reader.  Anything else stays as it is: a read LSE, ``causal``, dropout, a float mask, another
    head dim, k and v of different kinds, the 1-D ``input_pos`` route (``mask_cache.index_select``).

    ``kv_window_mask`` / ``kv_paged_window_mask`` (the sliding-window layers) are read the same way, into the ``_win``
    forms with ``window`` ahead of ``scale``; LTA_KV_WINDOW_FUSION=0 leaves those attentions and their masks alone."""
    if _kv_prefill_fusion_off():
        return trace
    rw = Rewrite(trace, ex)
    ops = {"16bit": (hip_prefill_attn_pos, hip_prefill_attn_paged),
           "kv8": (hip_prefill_attn_kv8_pos, hip_prefill_attn_kv8_paged),
           "kv8s": (hip_prefill_attn_kv8s_pos, hip_prefill_attn_kv8s_paged)}
    masks = set()
    for i, b in enumerate(rw.bsyms):
        if b.sym is not hip_attn_fwd_ex or rw.touched(i):
            continue
        p = operands(b)
        q, k, v, mask = p["q"], p["k"], p["v"], p["mask"]
        if not isinstance(b.output, (tuple, list)) or len(b.output) != 2 or rw.uses(b.output[1]):
            continue
        if p["causal"] or isinstance(p["dropout_p"], Proxy) or p["dropout_p"] or q.shape[-1] not in (64, 128):
            continue
        if not all(isinstance(t, TensorProxy) for t in (k, v, mask)) or mask.dtype != torch.bool:
            continue
        m = rw.producer(mask)
        if m is None or rw.touched(m):
            continue
        mb = rw.bsyms[m]
        paged = mb.sym.id in (*_KV_PAGED_MASK_IDS, *_KV_PAGED_WINDOW_MASK_IDS)
        if not paged and mb.sym.id not in (*_KV_POSITION_MASK_IDS, *_KV_WINDOW_MASK_IDS):
            continue
        pw = _window_of(mb, ("pos", "table", "page_size", "num_pages") if paged else ("input_pos", "S"))
        if pw is None:
            continue
        pm, window = pw
        if paged:
            pos, table = pm["pos"], pm["table"]
            if _kv_paged_fusion_off() or not isinstance(table, TensorProxy):
                continue
            if any(isinstance(pm[n], Proxy) for n in ("page_size", "num_pages")):
                continue
        else:
            pos = pm["input_pos"]
            if _kv_pos_fusion_off() or isinstance(pm["S"], Proxy) or k.ndim != 4 or k.shape[2] != int(pm["S"]):
                continue
        if not isinstance(pos, TensorProxy) or pos.dtype != torch.int64 or pos.ndim != 2:
            continue
        if tuple(pos.shape) != (q.shape[0], q.shape[2]):
            continue
        # the cache kind: k and v through the same dequantise, or both as they are stored
        kinds = (("kv8s", _kv8_rows_dequantised), ("kv8", _e4m3_dequantised))
        found = [(kind, resolve(rw, k, q.dtype), resolve(rw, v, q.dtype)) for kind, resolve in kinds]
        hit = [f for f in found if f[1] is not None and f[2] is not None]
        if hit:
            kind, rk, rv = hit[0]
            if _kv8_fusion_off():
                continue
        elif any(f[1] is not None or f[2] is not None for f in found) or k.dtype != q.dtype or v.dtype != q.dtype:
            continue
        else:
            kind, rk, rv = "16bit", ((k,), i, ()), ((v,), i, ())
        caches = [c for pair in zip(rk[0], rv[0]) for c in pair]  # the operators' order: k, v, then their scales
        chains = [list(rk[2]), list(rv[2])]  # per operand: the links to drop, outermost first
        first = min(rk[1], rv[1])
        if paged:
            gathers = [_paged_gather(rw, c) for c in caches]
            if any(g is None or g[1].name != table.name or g[2] != pm["page_size"] for g in gathers):
                continue
            for n, g in enumerate(gathers):
                chains[n % 2].append(g[3])
            caches = [g[0] for g in gathers]
            first = min(first, *(g[3] for g in gathers))
        # the kernel reads the caches where the attention stands: nothing may write them after the first link
        if any(first < j < i and OpTags.IN_PLACE in (rw.bsyms[j].sym.tags or ())
               for c in caches for j in rw.consumers(c)):
            continue
        rest = (pos, table, pm["page_size"], pm["num_pages"]) if paged else (pos,)
        op, win = _window_form(ops[kind][paged], window)
        rw.replace(i, op.bind(q, *caches, *rest, *win, p["scale"], output=b.output[0]))
        for chain in chains:
            for j in chain:
                # a link goes when its only reader was the attention or a link just dropped (a scaled paged cache has
                # two gathers under one dequantise)
                link = rw.bsyms[j].output
                if rw.uses(link) != 1 or not all(c == i or rw.dropped(c) for c in rw.consumers(link)):
                    break
                rw.drop(j)
        masks.add(m)
    for m in masks:  # one mask serves the layers of a step
        if all(rw.touched(j) and not rw.dropped(j) for j in rw.consumers(rw.bsyms[m].output)):
            rw.drop(m)
    return rw.finish(f"hipex: {rw.replaced} prefill attention(s) read their KV cache by positions")


def _fuse_rms_bwd_residual(trace):
    """``(dx, dw) = hip_rms_norm_bwd(g, x, w, rstd); z = dx + r`` (dx used nowhere else) ->
    ``(z, dw) = hip_rms_norm_bwd(g, x, w, rstd, r)``: the residual stream's gradient is added in the
    normalisation backward's store pass instead of a separate elementwise launch.  The same for
    ``hip_layer_norm_bwd`` (GPT-2 / NeoX blocks)."""
    rw = Rewrite(trace, ex)
    for i, b in enumerate(rw.bsyms):
        for y, r in _residual_adds(b):
            j = rw.producer(y)
            if j is None or rw.touched(j) or rw.uses(y) != 1:
                continue
            rb = rw.bsyms[j]
            if rb.sym is not hip_rms_norm_bwd and rb.sym is not hip_layer_norm_bwd:
                continue
            p = operands(rb)
            if p["residual"] is not None or rb.output[0] is not y or b.output.dtype != y.dtype or rw.producer(r, -1) > j:
                continue
            p["residual"] = r  # the last parameter of both
            rw.replace(j, rb.sym.bind(*p.values(), output=(b.output, *rb.output[1:])))
            rw.drop(i)
            break
    return rw.finish(f"hipex: {rw.replaced} residual-gradient add(s) fused into a normalisation backward")


# ---- fused SwiGLU GEMMs (csrc/gemm4.hip EPI 1 / 2) ---------------------------------------
def _gate_up_meta(x, w1, w2):
    shp = tuple(x.shape[:-1]) + (w1.shape[0],)
    return TensorProxy(like=x, shape=shp), TensorProxy(like=x, shape=shp), TensorProxy(like=x, shape=shp)


def _gate_up_impl(x, w1, w2):
    from ..ops.gemm import gate_up_swiglu

    return gate_up_swiglu(x, w1, w2, need_ab=True)


def _gate_up_y_impl(x, w1, w2):
    from ..ops.gemm import gate_up_swiglu

    return gate_up_swiglu(x, w1, w2, need_ab=False)[2]


hip_gate_up = ex.register_operator("hip_gate_up", meta=_gate_up_meta, fn=_gate_up_impl)
hip_gate_up_y = ex.register_operator("hip_gate_up_y", meta=lambda x, w1, w2: _gate_up_meta(x, w1, w2)[2],
                                     fn=_gate_up_y_impl)


def _mm_swiglu_bwd_impl(dy, w, a, b):
    from ..ops.gemm import matmul_swiglu_bwd

    return matmul_swiglu_bwd(dy, w, a, b)


hip_matmul_swiglu_bwd = ex.register_operator(
    "hip_matmul_swiglu_bwd", meta=lambda dy, w, a, b: (TensorProxy(like=a), TensorProxy(like=b)), fn=_mm_swiglu_bwd_impl)


def _plain_linear(b):
    """The operands of ``b`` when it is a ``hip_linear`` without bias, residual or activation, else None."""
    if b.sym is not hip_linear:
        return None
    p = operands(b)
    return p if p["bias"] is None and p["residual"] is None and p["act"] is None else None


def _fuse_swiglu_gemms(trace):
    """LLaMA-MLP SwiGLU chains onto the GEMM epilogues (prefill / training shapes; decode rows go to
    the gated GEMV of :func:`_fuse_decode`):

    * forward: ``a = hip_linear(x, w1); b = hip_linear(x, w2); y = hip_swiglu(a, b)`` ->
      ``a, b, y = hip_gate_up(x, w1, w2)`` (one launch; ``hip_gate_up_y`` when nothing else reads
      a / b, e.g. inference);
    * backward: ``g = hip_matmul(dy, w); da, db = hip_swiglu_bwd(g, a, b)`` (g read nowhere else) ->
      ``da, db = hip_matmul_swiglu_bwd(dy, w, a, b)``.
    Reference counterpart: nvFuser fusing the pointwise SwiGLU into its matmul segments
    (thunder/executors/nvfuserex_impl.py:2437-2488)."""
    from ..ops.gemm import _fused_swiglu_on

    if not _fused_swiglu_on():
        return trace
    rw = Rewrite(trace, ex)
    n_fwd = n_bwd = 0
    for i, b in enumerate(rw.bsyms):
        if b.sym is hip_swiglu:
            a, g = operands(b).values()
            ja, jg = rw.producer(a), rw.producer(g)
            if ja is None or jg is None or ja == jg or rw.touched(ja) or rw.touched(jg):
                continue
            pa, pg = _plain_linear(rw.bsyms[ja]), _plain_linear(rw.bsyms[jg])
            if pa is None or pg is None or pa["x"].name != pg["x"].name:
                continue
            x, w1, w2 = pa["x"], pa["w"], pg["w"]
            if tuple(w1.shape) != tuple(w2.shape) or _rows(x) <= _GEMV_MAX_ROWS or x.dtype != torch.bfloat16:
                continue
            at = max(ja, jg)
            # every other reader of a / b (the return included) must come after the fused op's position
            others = [k for k in rw.consumers(a) + rw.consumers(g) if k != i]
            if any(k <= at for k in others):
                continue
            if others:
                rw.replace(at, hip_gate_up.bind(x, w1, w2, output=(a, g, b.output)))
            else:
                rw.replace(at, hip_gate_up_y.bind(x, w1, w2, output=b.output))
            rw.drop(min(ja, jg), i)
            n_fwd += 1
        elif b.sym is hip_swiglu_bwd:
            g, a, bb = operands(b).values()
            j = rw.producer(g)
            if j is None or rw.touched(j) or rw.bsyms[j].sym is not hip_matmul:
                continue
            m = operands(rw.bsyms[j])
            if m["residual"] is not None or rw.consumers(g) != [i]:
                continue
            if m["b"].ndim != 2 or tuple(a.shape) != tuple(g.shape) or tuple(bb.shape) != tuple(g.shape):
                continue
            rw.replace(i, hip_matmul_swiglu_bwd.bind(m["a"], m["b"], a, bb, output=b.output))
            rw.drop(j)
            n_bwd += 1
    return rw.finish(f"hipex: {n_fwd} gate-up SwiGLU GEMM(s), {n_bwd} SwiGLU-backward GEMM epilogue(s)")


def _linear_qkv_rope_impl(x, w, cos, sin, n_head, n_query_groups, head_size, rope_n):
    from ..ops.gemm import linear_qkv_rope

    return linear_qkv_rope(x, w, cos, sin, n_head, n_query_groups, head_size, rope_n)


def _linear_qkv_rope_meta(x, w, cos, sin, n_head, n_query_groups, head_size, rope_n):
    B, T = x.shape[0], x.shape[1]
    return (TensorProxy(like=x, shape=(B, n_head, T, head_size)),
            TensorProxy(like=x, shape=(B, n_query_groups, T, head_size)),
            TensorProxy(like=x, shape=(B, n_query_groups, T, head_size)))


hip_linear_qkv_rope = ex.register_operator("hip_linear_qkv_rope", meta=_linear_qkv_rope_meta, fn=_linear_qkv_rope_impl)


def _rope_of_gemm(rw, i, b, gemm):
    """``(j, rope operands)`` when ``b`` (at i) is the ``hip_qkv_rope`` of a ``gemm`` output at j that nothing
    else reads, with literal head geometry and cos / sin that exist where the GEMM runs; else None."""
    if b.sym is not hip_qkv_rope:
        return None
    r = operands(b)
    j = rw.producer(r["qkv"])
    if j is None or rw.touched(j) or rw.bsyms[j].sym is not gemm or rw.consumers(r["qkv"]) != [i]:
        return None
    if not all(isinstance(r[k], int) for k in ("n_head", "n_query_groups", "head_size", "rope_n")):
        return None
    if rw.producer(r["cos"], -1) > j or rw.producer(r["sin"], -1) > j:
        return None
    if getattr(r["cos"], "ndim", 2) != 2:  # per-token rotations (a ragged batch): the epilogue indexes cos by t
        return None
    return j, r


def _fuse_qkv_rope_gemm(trace):
    """``qkv = hip_linear(x, w); q, k, v = hip_qkv_rope(qkv, cos, sin, ...)`` (qkv read nowhere else,
    prefill / training rows) -> ``q, k, v = hip_linear_qkv_rope(x, w, cos, sin, ...)``: the attention
    input projection stores the RoPE'd head layouts from its epilogue (csrc/gemm4.hip EPI 3), so the
    [B, T, (nh + 2 ng) D] projection output never goes to HBM.  Reference counterpart: the
    torch.compile / nvFuser cat+RoPE fusion of thunder/executors/torch_compile.py (rope) — here it
    lands in the GEMM itself."""
    rw = Rewrite(trace, ex)
    for i, b in enumerate(rw.bsyms):
        m = _rope_of_gemm(rw, i, b, hip_linear)
        if m is None:
            continue
        j, r = m
        p = _plain_linear(rw.bsyms[j])
        if p is None or p["x"].ndim != 3 or _rows(p["x"]) <= _GEMV_MAX_ROWS:
            continue
        rw.replace(j, hip_linear_qkv_rope.bind(p["x"], p["w"], r["cos"], r["sin"], r["n_head"], r["n_query_groups"],
                                               r["head_size"], r["rope_n"], output=b.output))
        rw.drop(i)
    return rw.finish(f"hipex: {rw.replaced} qkv projection(s) with the RoPE split in the GEMM epilogue")


def _fp8_gemm_qkv_rope_impl(qa, qb, sa, sb, out_shape, cos, sin, n_head, n_query_groups, head_size, rope_n):
    from ..ops.fp8 import gemm_qkv_rope

    return gemm_qkv_rope(qa, qb, sa, sb, out_shape, cos, sin, n_head, n_query_groups, head_size, rope_n)


def _fp8_gemm_qkv_rope_meta(qa, qb, sa, sb, out_shape, cos, sin, n_head, n_query_groups, head_size, rope_n):
    B, T = out_shape[0], out_shape[1]
    mk = lambda h: TensorProxy(like=sa, shape=(B, h, T, head_size), dtype=torch.bfloat16)  # noqa: E731
    return mk(n_head), mk(n_query_groups), mk(n_query_groups)


hip_fp8_gemm_qkv_rope = ex.register_operator("hip_fp8_gemm_qkv_rope", meta=_fp8_gemm_qkv_rope_meta,
                                             fn=_fp8_gemm_qkv_rope_impl)


def _fuse_fp8_qkv_rope_gemm(trace):
    """``qkv = hip_fp8_gemm(qx, qw, sx, sw, 0, 0, None, shape); q, k, v = hip_qkv_rope(qkv, ...)`` (qkv
    read nowhere else) -> ``q, k, v = hip_fp8_gemm_qkv_rope(...)``: the FP8 path's counterpart of
    :func:`_fuse_qkv_rope_gemm` (csrc/gemm4_fp8.hip QKV epilogue; reference: TransformerEngine's fused
    attention input projection, thunder/executors/transformer_engineex_impl.py)."""
    rw = Rewrite(trace, ex)
    for i, b in enumerate(rw.bsyms):
        m = _rope_of_gemm(rw, i, b, hip_fp8_gemm)
        if m is None:
            continue
        j, r = m
        g = operands(rw.bsyms[j])
        if g["out_shape"] is None or g["residual"] is not None or g["fmt_a"] != 0 or g["fmt_b"] != 0 or g["bias"] is not None:
            continue
        out_shape = tuple(g["out_shape"])
        if len(out_shape) != 3 or not all(isinstance(v, int) for v in out_shape):
            continue
        rw.replace(j, hip_fp8_gemm_qkv_rope.bind(g["qa"], g["qb"], g["sa"], g["sb"], out_shape, r["cos"], r["sin"],
                                                 r["n_head"], r["n_query_groups"], r["head_size"], r["rope_n"],
                                                 output=b.output))
        rw.drop(i)
    return rw.finish(f"hipex: {rw.replaced} fp8 qkv projection(s) with the RoPE split in the GEMM epilogue")


def _attn_bwd_rope_meta(g, q, k, v, o, lse, causal, scale, cos, sin, n_head, n_query_groups):
    B, _, T, D = q.shape
    return TensorProxy(like=g, shape=(B, T, (n_head + 2 * n_query_groups) * D))


def _attn_bwd_rope_impl(g, q, k, v, o, lse, causal, scale, cos, sin, n_head, n_query_groups):
    from ..ops.attention import attn_bwd_rope

    return attn_bwd_rope(g, q, k, v, o, lse, causal, scale, cos, sin, n_head, n_query_groups)


hip_attn_bwd_rope = ex.register_operator("hip_flash_attn_bwd_rope", meta=_attn_bwd_rope_meta, fn=_attn_bwd_rope_impl)


def _fuse_attn_bwd_rope(trace):
    """``dq, dk, dv = hip_flash_attn_bwd(...); dqkv = hip_qkv_rope_bwd(dq, dk, dv, cos, sin, ...)``
    (dq / dk / dv read nowhere else, full-width rotate-half RoPE on 128-wide heads) ->
    ``dqkv = hip_flash_attn_bwd_rope(..., cos, sin, n_head, n_query_groups)``: the RoPE backward
    runs in the attention backward's dQ / dK epilogues and the three gradients are stored straight
    into the fused projection's gradient (the mirror of the qkv-RoPE GEMM epilogue of the forward)."""
    rw = Rewrite(trace, ex)
    for i, b in enumerate(rw.bsyms):
        if b.sym is not hip_qkv_rope_bwd:
            continue
        r = operands(b)
        grads = (r["dq"], r["dk"], r["dv"])
        if not all(isinstance(t, TensorProxy) for t in (*grads, r["cos"], r["sin"])):
            continue
        if r["head_size"] != 128 or r["rope_n"] != r["head_size"]:
            continue
        j = rw.producer(grads[0])
        if j is None or rw.touched(j) or rw.bsyms[j].sym is not hip_attn_bwd:
            continue
        ab = rw.bsyms[j]
        if tuple(o.name for o in ab.flat_proxy_outs) != tuple(t.name for t in grads) or any(rw.uses(t) != 1 for t in grads):
            continue
        a = operands(ab)
        nh, ng = r["n_head"], r["n_query_groups"]
        if a["q"].shape[1] != nh or a["k"].shape[1] != ng or a["q"].shape[2] != a["k"].shape[2]:
            continue
        rw.replace(i, hip_attn_bwd_rope.bind(*a.values(), r["cos"], r["sin"], nh, ng, output=b.output))
        rw.drop(j)
    return rw.finish(f"hipex: {rw.replaced} RoPE backward(s) fused into the attention backward")


def _rms_bwd_fp8_meta(dy, x, weight, rstd, residual, key, slot):
    q, sc = _fp8_cast_meta(x, True)
    return TensorProxy(like=x), (None if weight is None else TensorProxy(like=weight)), q, sc


def _rms_bwd_fp8_impl(dy, x, weight, rstd, residual, key, slot):
    from ..ops.fp8 import rms_norm_bwd_fp8_delayed

    return rms_norm_bwd_fp8_delayed(dy, x, weight, rstd, residual, key, slot)


hip_rms_norm_bwd_fp8 = ex.register_operator("hip_rms_norm_bwd_fp8", meta=_rms_bwd_fp8_meta, fn=_rms_bwd_fp8_impl)


def _fuse_fp8_rms_bwd_casts(trace):
    """``dx, dw = hip_rms_norm_bwd(g, x, w, rstd[, r]); q, s = hip_fp8_cast_delayed(dx, True, key, slot)``
    -> ``dx, dw, q, s = hip_rms_norm_bwd_fp8(g, x, w, rstd, r, key, slot)``: a LLaMA block's residual-
    stream gradient is the output gradient of the preceding fp8 linear (the attention projection after
    norm_2's backward, the previous block's MLP projection after norm_1's), so its e5m2 copy leaves the
    norm backward's store pass (dx keeps its other uses; the cast launch re-reading dx disappears).
    Runs after :func:`_fuse_rms_bwd_residual`, so the residual add is already in the norm backward."""
    if _fp8_producer_fusion_off():
        return trace
    rw = Rewrite(trace, ex)
    for i, b in enumerate(rw.bsyms):
        c = _delayed_cast(b, e5m2=True)
        j = rw.producer(c["t"]) if c is not None else None
        if j is None or rw.touched(j):
            continue
        pb = rw.bsyms[j]
        if pb.sym is not hip_rms_norm_bwd or pb.output[0].name != c["t"].name:
            continue
        rw.replace(j, hip_rms_norm_bwd_fp8.bind(*operands(pb).values(), c["key"], c["slot"],
                                                output=(*pb.output[:2], *b.output)))
        rw.drop(i)
    return rw.finish(f"hipex: {rw.replaced} e5m2 gradient cast(s) fused into RMSNorm backwards")


def _attn_fwd_fp8_meta(q, k, v, causal, scale, key, slot):
    B, H, L, E = q.shape
    return (TensorProxy(like=q), TensorProxy(like=q, shape=(B, H, L), dtype=torch.float32, requires_grad=False),
            TensorProxy(like=q, shape=(B * L, H * E), dtype=torch.uint8, requires_grad=False),
            TensorProxy(like=q, shape=(), dtype=torch.float32, requires_grad=False))


def _attn_fwd_fp8_impl(q, k, v, causal, scale, key, slot):
    from ..ops.fp8 import attn_fwd_fp8_delayed

    return attn_fwd_fp8_delayed(q, k, v, causal, scale, key, slot)


hip_attn_fwd_fp8 = ex.register_operator("hip_flash_attn_fwd_fp8", meta=_attn_fwd_fp8_meta, fn=_attn_fwd_fp8_impl)

# the view ops of o.transpose(1, 2).reshape(B, T, H D) at every level a trace can hold them (ltorch symbols
# before flattening, their torch-executor operators, the prims)
_HEAD_MERGE_VIEWS = {"transpose", "permute", "reshape", "view", "torch_transpose", "torch_permute", "torch_reshape",
                     "torch_view", "transpose_prim", "reshape_prim"}


def _merges_heads(chain, out) -> bool:
    """``chain`` (producer order) turns the attention output [B, H, T, D] into its [B, T, H D] (or
    [B T, H D]) rows: one (1, 2) transpose / permute, then reshapes only."""
    B, H, T, D = out.shape
    swapped = False
    for b in chain:
        n = b.sym.name
        if n in ("transpose", "torch_transpose"):
            dims = {int(pyval(d)) % 4 for d in b.args[1:3]}
            if swapped or dims != {1, 2}:
                return False
            swapped = True
        elif n in ("permute", "torch_permute", "transpose_prim"):
            perm = (b.args[1] if len(b.args) == 2 else b.args[1:]) if len(b.args) > 1 else \
                b.kwargs.get("permutation", b.kwargs.get("dims"))
            try:
                perm = tuple(int(pyval(d)) % 4 for d in perm)
            except TypeError:
                return False
            if swapped or perm != (0, 2, 1, 3):
                return False
            swapped = True
        elif not swapped:
            return False
    y = chain[-1].output
    return swapped and tuple(y.shape) in ((B, T, H * D), (B * T, H * D))


def _fuse_fp8_attn_out_casts(trace):
    """``o, lse = hip_flash_attn_fwd(q, k, v, ...); y = o.transpose(1, 2).reshape(B, T, H D);
    qy, sy = hip_fp8_cast_delayed(y, False, key, slot)`` -> ``o, lse, qy, sy = hip_flash_attn_fwd_fp8(q, k,
    v, ..., key, slot)``: the e4m3 input of the FP8 output projection leaves the attention epilogue
    (O is stored [B, T, H, D], so its rows are the projection's rows); O itself is still written for the
    backward.  The view chain stays for its other readers."""
    if _fp8_producer_fusion_off():
        return trace
    rw = Rewrite(trace, ex)
    for i, b in enumerate(rw.bsyms):
        c = _delayed_cast(b, e5m2=False)
        if c is None:
            continue
        chain, cur = [], c["t"]
        j = rw.producer(cur)
        while j is not None and rw.bsyms[j].sym.name in _HEAD_MERGE_VIEWS and len(chain) < 4:
            chain.append(rw.bsyms[j])
            cur = rw.bsyms[j].args[0]
            j = rw.producer(cur)
        if j is None or rw.touched(j) or not chain or rw.bsyms[j].sym is not hip_attn_fwd:
            continue
        ab = rw.bsyms[j]
        out = ab.output[0]
        if cur.name != out.name or out.dtype != torch.bfloat16 or out.shape[-1] != 128:
            continue
        if not _merges_heads(chain[::-1], out):
            continue
        rw.replace(j, hip_attn_fwd_fp8.bind(*operands(ab).values(), c["key"], c["slot"], output=(*ab.output[:2], *b.output)))
        rw.drop(i)
    return rw.finish(f"hipex: {rw.replaced} e4m3 attention-output cast(s) fused into the attention epilogue")


_PASSES = (
    _fuse_fp8_cast_producers, _fuse_fp8_attn_out_casts, _fuse_linear_epilogues, _fuse_rms_bwd_residual,
    _fuse_fp8_rms_bwd_casts,
    partial(_fuse_decode, kind=_BF16_DECODE, folds=("gate", "norm"),
            message="hipex: decode GEMV fusion ({gate} gated pair(s), {norm} norm prologue(s))"),
    partial(_fuse_decode, kind=_MXFP4_DECODE, folds=("gate", "act", "residual", "norm", "group"),
            message="hipex: MXFP4 decode GEMV fusion ({gate} gated pair(s), {act} activation(s), {residual} residual(s), "
                    "{norm} norm prologue(s), {group} group(s))"),
    _fuse_swiglu_gemms, _fuse_kv_cache_writes, _fuse_kv_position_reads, _fuse_kv8_reads, _fuse_kv_paged_reads,
    _fuse_kv_prefill_reads,
    partial(_fuse_decode, kind=_BF16_DECODE, folds=("group",), message="hipex: {group} grouped decode projection launch(es)"),
    _fuse_qkv_rope_gemm, _fuse_fp8_qkv_rope_gemm, _fuse_attn_bwd_rope,
)


def _post_claim(trace):
    for rewrite in _PASSES:
        trace = rewrite(trace)
    return trace


ex.post_claim_pass = _post_claim


# =========================================================================================
# K4 RMSNorm
# =========================================================================================
def _rms_fwd_meta(x, weight, eps):
    rows = 1
    for s in x.shape[:-1]:
        rows *= s
    return TensorProxy(like=x), TensorProxy(like=x, shape=(rows,), dtype=torch.float32, requires_grad=False)


def _rms_fwd_impl(x, weight, eps):
    from ..ops.rmsnorm import rms_norm_fwd

    return rms_norm_fwd(x, weight, eps)


def _rms_bwd_meta(dy, x, weight, rstd, residual=None):
    return TensorProxy(like=x), (None if weight is None else TensorProxy(like=weight))


def _rms_bwd_impl(dy, x, weight, rstd, residual=None):
    from ..ops.rmsnorm import rms_norm_bwd

    return rms_norm_bwd(dy, x, weight, rstd, residual)


hip_rms_norm_fwd = ex.register_operator("hip_rms_norm_fwd", meta=_rms_fwd_meta, fn=_rms_fwd_impl)
hip_rms_norm_bwd = ex.register_operator("hip_rms_norm_bwd", meta=_rms_bwd_meta, fn=_rms_bwd_impl)


def _rms_checker(a, normalized_shape, weight=None, eps=None):
    if not _gpu(a, weight) or a.dtype not in _FLOAT16ISH:
        return False
    if len(normalized_shape) != 1 or normalized_shape[0] != a.shape[-1]:
        return False
    if weight is not None and (weight.dtype != a.dtype or tuple(weight.shape) != (a.shape[-1],)):
        return False
    return True


def _eps(a, eps):
    return torch.finfo(a.dtype).eps if eps is None else eps


def _rms_exec(a, normalized_shape, weight=None, eps=None):
    y, _ = hip_rms_norm_fwd(a, weight, _eps(a, eps))
    return y


def _rms_grad(a, normalized_shape, weight=None, eps=None):
    y, rstd = hip_rms_norm_fwd(a, weight, _eps(a, eps))

    def bwd(g):
        dx, dw = hip_rms_norm_bwd(g, a, weight, rstd)
        return dx, None, dw

    return y, bwd


# =========================================================================================
# K10 grouped GEMM (MoE experts)
# =========================================================================================
def _gmm_meta(a, b, offs):
    if a.ndim == 2 and b.ndim == 2:  # the wgrad form: [G, K, N]
        return TensorProxy(like=a, shape=(offs.shape[0], a.shape[0], b.shape[1]))
    return TensorProxy(like=a, shape=(a.shape[0], b.shape[2]))


def _gmm_impl(a, b, offs):
    from ..ops.gemm import grouped_mm

    return grouped_mm(a, b, offs)


hip_grouped_mm = ex.register_operator("hip_grouped_mm", meta=_gmm_meta, fn=_gmm_impl)


def _gmm_checker(a, b, offs=None, bias=None, out_dtype=None):
    """Forward / dgrad (2-D x 3-D) and wgrad (2-D x 2-D, reduction over each group's rows) forms:
    the VJP of _grouped_mm (transforms/autodiff.py) emits all three, so MoE training runs every
    expert GEMM on the hand kernels (csrc/gemm4.hip grouped modes)."""
    return (_gpu(a, b, offs) and offs is not None and bias is None and out_dtype is None and a.ndim == 2
            and b.ndim in (2, 3) and a.dtype == torch.bfloat16 and b.dtype == torch.bfloat16)


def _gmm_exec(a, b, offs=None, bias=None, out_dtype=None):
    return hip_grouped_mm(a, b, offs)


# =========================================================================================
# K5 LayerNorm
# =========================================================================================
def _ln_fwd_meta(x, weight, bias, eps):
    rows = 1
    for d in x.shape[:-1]:
        rows *= d
    st = TensorProxy(like=x, shape=(rows,), dtype=torch.float32, requires_grad=False)
    return TensorProxy(like=x), st, TensorProxy(like=st)


def _ln_fwd_impl(x, weight, bias, eps):
    from ..ops.rmsnorm import layer_norm_fwd

    return layer_norm_fwd(x, weight, bias, eps)


def _ln_bwd_meta(dy, x, weight, mean, rstd, has_bias, residual=None):
    return (TensorProxy(like=x), None if weight is None else TensorProxy(like=weight),
            TensorProxy(like=x, shape=(x.shape[-1],)) if has_bias else None)


def _ln_bwd_impl(dy, x, weight, mean, rstd, has_bias, residual=None):
    from ..ops.rmsnorm import layer_norm_bwd

    return layer_norm_bwd(dy, x, weight, mean, rstd, has_bias, residual)


hip_layer_norm_fwd = ex.register_operator("hip_layer_norm_fwd", meta=_ln_fwd_meta, fn=_ln_fwd_impl)
hip_layer_norm_bwd = ex.register_operator("hip_layer_norm_bwd", meta=_ln_bwd_meta, fn=_ln_bwd_impl)


def _ln_checker(a, normalized_shape, weight=None, bias=None, eps=1e-5):
    if not _gpu(a, weight, bias) or a.dtype not in _FLOAT16ISH:
        return False
    if len(normalized_shape) != 1 or normalized_shape[0] != a.shape[-1]:
        return False
    for t in (weight, bias):
        if t is not None and (t.dtype != a.dtype or tuple(t.shape) != (a.shape[-1],)):
            return False
    return True


def _ln_exec(a, normalized_shape, weight=None, bias=None, eps=1e-5):
    y, _, _ = hip_layer_norm_fwd(a, weight, bias, eps)
    return y


def _ln_grad(a, normalized_shape, weight=None, bias=None, eps=1e-5):
    y, mean, rstd = hip_layer_norm_fwd(a, weight, bias, eps)

    def bwd(g):
        dx, dw, db = hip_layer_norm_bwd(g, a, weight, mean, rstd, bias is not None)
        return dx, None, dw, db

    return y, bwd


# =========================================================================================
# K6 fused qkv split + RoPE (lookaside for the LitGPT helper `qkv_split_rope`)
# =========================================================================================
def _qkv_rope_meta(qkv, cos, sin, n_head, n_query_groups, head_size, rope_n):
    B, T, _ = qkv.shape
    q = TensorProxy(like=qkv, shape=(B, n_head, T, head_size))
    k = TensorProxy(like=qkv, shape=(B, n_query_groups, T, head_size))
    v = TensorProxy(like=qkv, shape=(B, n_query_groups, T, head_size))
    return q, k, v


def _qkv_rope_impl(qkv, cos, sin, n_head, n_query_groups, head_size, rope_n):
    from ..ops.fused import qkv_rope_fwd, qkv_rope_rows_fwd

    if cos.dim() == 3:  # one rotation per (sequence, token): a ragged batch
        return qkv_rope_rows_fwd(qkv, cos, sin, n_head, n_query_groups, head_size, rope_n)
    return qkv_rope_fwd(qkv, cos, sin, n_head, n_query_groups, head_size, rope_n)


def _qkv_rope_bwd_meta(dq, dk, dv, cos, sin, n_head, n_query_groups, head_size, rope_n):
    B, _, T, _ = dq.shape
    return TensorProxy(like=dq, shape=(B, T, (n_head + 2 * n_query_groups) * head_size))


def _qkv_rope_bwd_impl(dq, dk, dv, cos, sin, n_head, n_query_groups, head_size, rope_n):
    from ..ops.fused import qkv_rope_bwd

    return qkv_rope_bwd(dq, dk, dv, cos, sin, n_head, n_query_groups, head_size, rope_n)


hip_qkv_rope = ex.register_operator("hip_qkv_rope", meta=_qkv_rope_meta, fn=_qkv_rope_impl)
hip_qkv_rope_bwd = ex.register_operator("hip_qkv_rope_bwd", meta=_qkv_rope_bwd_meta, fn=_qkv_rope_bwd_impl)


def _qkv_rope_vjp(qkv, cos, sin, n_head, n_query_groups, head_size, rope_n):
    q, k, v = hip_qkv_rope(qkv, cos, sin, n_head, n_query_groups, head_size, rope_n)

    def bwd(gq, gk, gv):
        return (hip_qkv_rope_bwd(gq, gk, gv, cos, sin, n_head, n_query_groups, head_size, rope_n),)

    return (q, k, v), bwd


def qkv_split_rope_lookaside(qkv, cos, sin, n_head, n_query_groups, head_size, rope_n_elem):
    ok = (
        _gpu(qkv, cos, sin)
        and qkv.dtype in _FLOAT16ISH
        and qkv.ndim == 3
        and head_size % 8 == 0
        and rope_n_elem % 16 == 0
        and rope_n_elem <= head_size
        and cos.ndim in (2, 3)
        and cos.shape[-2] >= qkv.shape[1]
        and cos.shape[-1] == rope_n_elem
        and cos.dtype in (torch.float32, qkv.dtype)
    )
    if ok and cos.ndim == 3:  # [B, T, rope_n], one rotation per token (a ragged batch): forward only
        ok = (tuple(cos.shape) == (qkv.shape[0], qkv.shape[1], rope_n_elem) and tuple(sin.shape) == tuple(cos.shape)
              and not qkv.requires_grad)
    if not ok:
        return qkv_split_rope_lookaside.__wrapped_original__(qkv, cos, sin, n_head, n_query_groups, head_size, rope_n_elem)
    return hip_qkv_rope(qkv, cos, sin, n_head, n_query_groups, head_size, rope_n_elem)


# =========================================================================================
# SwiGLU (lookaside for the LitGPT helper `swiglu`)
# =========================================================================================
hip_swiglu = ex.register_operator("hip_swiglu", meta=lambda a, b: TensorProxy(like=a),
                                  fn=lambda a, b: __import__("lightning_thunder_amd.ops.fused", fromlist=["x"]).swiglu_fwd(a, b))
hip_swiglu_bwd = ex.register_operator(
    "hip_swiglu_bwd", meta=lambda g, a, b: (TensorProxy(like=a), TensorProxy(like=b)),
    fn=lambda g, a, b: __import__("lightning_thunder_amd.ops.fused", fromlist=["x"]).swiglu_bwd(g, a, b),
)


def _swiglu_vjp(a, b):
    y = hip_swiglu(a, b)

    def bwd(g):
        da, db = hip_swiglu_bwd(g, a, b)
        return da, db

    return y, bwd


def swiglu_lookaside(a, b):
    if _gpu(a, b) and a.dtype in _FLOAT16ISH and a.dtype == b.dtype and tuple(a.shape) == tuple(b.shape):
        return hip_swiglu(a, b)
    return swiglu_lookaside.__wrapped_original__(a, b)


# =========================================================================================
# K7 softmax cross-entropy
# =========================================================================================
def _ce_fwd_meta(logits, target, ignore_index, reduction, label_smoothing, weight=None):
    rows = logits.shape[0]
    loss = TensorProxy(like=logits, shape=(rows,) if reduction == "none" else ())
    lse = TensorProxy(like=logits, shape=(rows,), dtype=torch.float32, requires_grad=False)
    stats = TensorProxy(like=logits, shape=(2,), dtype=torch.float32, requires_grad=False)
    return loss, lse, stats


def _ce_fwd_impl(logits, target, ignore_index, reduction, label_smoothing, weight=None):
    from ..ops.fused import cross_entropy_fwd

    return cross_entropy_fwd(logits, target, ignore_index, reduction, label_smoothing, weight)


def _ce_bwd_impl(g, logits, target, lse, stats, ignore_index, reduction, label_smoothing, weight=None):
    from ..ops.fused import cross_entropy_bwd

    return cross_entropy_bwd(g, logits, target, lse, stats, ignore_index, reduction, label_smoothing, weight)


hip_cross_entropy_fwd = ex.register_operator("hip_cross_entropy_fwd", meta=_ce_fwd_meta, fn=_ce_fwd_impl)
hip_cross_entropy_bwd = ex.register_operator(
    "hip_cross_entropy_bwd", meta=lambda g, logits, *a, **k: TensorProxy(like=logits), fn=_ce_bwd_impl
)


def _ce_checker(a, target, weight=None, size_average=None, ignore_index=-100, reduce=None, reduction="mean", label_smoothing=0.0):
    return (
        _gpu(a, target, weight)
        and a.ndim == 2
        and target.ndim == 1
        and (weight is None or (weight.ndim == 1 and weight.shape[0] == a.shape[1]
                                and weight.dtype in (torch.float32, torch.bfloat16, torch.float16)))
        and size_average is None
        and reduce is None
        and reduction in ("mean", "sum", "none")
        and a.dtype in _FLOAT16ISH
        and target.dtype in (torch.int64, torch.int32)
    )


def _ce_exec(a, target, weight=None, size_average=None, ignore_index=-100, reduce=None, reduction="mean", label_smoothing=0.0):
    if weight is None:
        loss, _, _ = hip_cross_entropy_fwd(a, target, ignore_index, reduction, label_smoothing)
    else:
        loss, _, _ = hip_cross_entropy_fwd(a, target, ignore_index, reduction, label_smoothing, weight)
    return loss


def _ce_grad(a, target, weight=None, size_average=None, ignore_index=-100, reduce=None, reduction="mean", label_smoothing=0.0):
    # class weights (reference: triton_crossentropy_impl.py:49-151) are a constant of the loss: no grad
    extra = () if weight is None else (weight,)
    loss, lse, stats = hip_cross_entropy_fwd(a, target, ignore_index, reduction, label_smoothing, *extra)

    def bwd(g):
        return (hip_cross_entropy_bwd(g, a, target, lse, stats, ignore_index, reduction, label_smoothing, *extra),)

    return loss, bwd


# =========================================================================================
# K3 flash attention (claims ltorch.scaled_dot_product_attention; saves O and LSE for backward)
# =========================================================================================
def _attn_fwd_meta(q, k, v, causal, scale):
    B, H, L, E = q.shape
    return TensorProxy(like=q), TensorProxy(like=q, shape=(B, H, L), dtype=torch.float32, requires_grad=False)


def _attn_fwd_impl(q, k, v, causal, scale):
    from ..ops.attention import attn_fwd

    return attn_fwd(q, k, v, causal, scale)


def _attn_bwd_impl(g, q, k, v, o, lse, causal, scale):
    from ..ops.attention import attn_bwd

    return attn_bwd(g, q, k, v, o, lse, causal, scale)


hip_attn_fwd = ex.register_operator("hip_flash_attn_fwd", meta=_attn_fwd_meta, fn=_attn_fwd_impl)
hip_attn_bwd = ex.register_operator(
    "hip_flash_attn_bwd",
    meta=lambda g, q, k, v, o, lse, causal, scale: (TensorProxy(like=q), TensorProxy(like=k), TensorProxy(like=v)),
    fn=_attn_bwd_impl,
)


# masked / dropout variant (additive or boolean mask, counter-based dropout of P, optional mask
# gradient): the same kernels with the extra terms compiled in (ops/attention.py: lta_attn_*_ex)
def _attn_fwd_ex_meta(q, k, v, mask, causal, scale, dropout_p, seed, offset):
    B, H, L, E = q.shape
    return TensorProxy(like=q), TensorProxy(like=q, shape=(B, H, L), dtype=torch.float32, requires_grad=False)


def _attn_fwd_ex_impl(q, k, v, mask, causal, scale, dropout_p, seed, offset):
    from ..ops.attention import attn_fwd

    return attn_fwd(q, k, v, causal, scale, mask=mask, dropout_p=dropout_p, seed=seed, offset=offset)


def _attn_bwd_ex_meta(g, q, k, v, o, lse, mask, causal, scale, dropout_p, seed, offset, mask_grad):
    outs = (TensorProxy(like=q), TensorProxy(like=k), TensorProxy(like=v))
    return outs + ((TensorProxy(like=mask),) if mask_grad else ())


def _attn_bwd_ex_impl(g, q, k, v, o, lse, mask, causal, scale, dropout_p, seed, offset, mask_grad):
    from ..ops.attention import attn_bwd

    return attn_bwd(g, q, k, v, o, lse, causal, scale, mask=mask, dropout_p=dropout_p, seed=seed, offset=offset,
                    mask_grad=mask_grad)


hip_attn_fwd_ex = ex.register_operator("hip_flash_attn_fwd_ex", meta=_attn_fwd_ex_meta, fn=_attn_fwd_ex_impl)
hip_attn_bwd_ex = ex.register_operator("hip_flash_attn_bwd_ex", meta=_attn_bwd_ex_meta, fn=_attn_bwd_ex_impl)


def _decode_attn_meta(q, k, v, mask, causal, scale):
    return TensorProxy(like=q)


def _decode_attn_impl(q, k, v, mask, causal, scale):
    from ..ops.attention import decode_attn

    return decode_attn(q, k, v, mask, causal, scale)


hip_decode_attn = ex.register_operator("hip_decode_attn", meta=_decode_attn_meta, fn=_decode_attn_impl)


def _decode_attn_kv8_meta(q, k8, v8, mask, causal, scale):
    return TensorProxy(like=q)


def _decode_attn_e4m3_run(q, caches, selector, scale, supported, kernel, dequantise, window=None):
    """Decode attention over e4m3 ``caches`` in operator order (k8, v8, then scale caches), for keys chosen by
    ``selector`` = (mask, causal) or (pos,): ``kernel`` where ``supported`` takes the operands, else (more query
    rows or a head dim the e4m3 kernel does not take) the program as the model spells it,
    ``dequantise(<a cache's operands>, dtype)`` and the 16-bit operator.  ``window``: the position forms' sliding
    window."""
    by_pos = len(selector) == 1
    win = {} if window is None else {"window": window}
    if supported(q, *caches, *(selector if by_pos else ())):
        return kernel(q, *caches, *selector, scale, **win)
    plain = _decode_attn_pos_impl if by_pos else _decode_attn_impl
    return plain(q, dequantise(*caches[0::2], q.dtype), dequantise(*caches[1::2], q.dtype), *selector, scale, **win)


def _decode_attn_kv8_impl(q, k8, v8, mask, causal, scale):
    from ..ops.attention import decode_attn_kv8, decode_attn_kv8_supported
    from ..ops.kv8 import e4m3_values

    return _decode_attn_e4m3_run(q, (k8, v8), (mask, causal), scale, decode_attn_kv8_supported, decode_attn_kv8,
                                 e4m3_values)


hip_decode_attn_kv8 = ex.register_operator("hip_decode_attn_kv8", meta=_decode_attn_kv8_meta, fn=_decode_attn_kv8_impl)


def _decode_attn_kv8s_meta(q, k8, v8, k_scale, v_scale, mask, causal, scale):
    return TensorProxy(like=q)


def _decode_attn_kv8s_impl(q, k8, v8, k_scale, v_scale, mask, causal, scale):
    from ..ops.attention import decode_attn_kv8s, decode_attn_kv8s_supported
    from ..ops.kv8 import dequantise_rows

    return _decode_attn_e4m3_run(q, (k8, v8, k_scale, v_scale), (mask, causal), scale, decode_attn_kv8s_supported,
                                 decode_attn_kv8s, dequantise_rows)


hip_decode_attn_kv8s = ex.register_operator("hip_decode_attn_kv8s", meta=_decode_attn_kv8s_meta,
                                            fn=_decode_attn_kv8s_impl)


# The position forms (a ragged batch): ``pos`` int64 [B, T] in place of mask and causal flag.
def _decode_attn_pos_meta(q, k, v, pos, scale):
    return TensorProxy(like=q)


def _position_mask(pos, S, window=None):
    """The mask the position forms stand for: ``position_mask``, under a sliding window ``window_mask``."""
    from ..ops.kv_rows import position_mask, window_mask

    return position_mask(pos, S) if window is None else window_mask(pos, S, window)


def _decode_attn_pos_impl(q, k, v, pos, scale, window=None):
    from ..ops.attention import decode_attn, decode_attn_pos, decode_attn_pos_supported

    if decode_attn_pos_supported(q, k, v, pos):
        return decode_attn_pos(q, k, v, pos, scale, window=window)
    return decode_attn(q, k, v, _position_mask(pos, k.shape[2], window), False, scale)


def _decode_attn_kv8_pos_impl(q, k8, v8, pos, scale, window=None):
    from ..ops.attention import decode_attn_kv8_pos, decode_attn_kv8_pos_supported
    from ..ops.kv8 import e4m3_values

    return _decode_attn_e4m3_run(q, (k8, v8), (pos,), scale, decode_attn_kv8_pos_supported, decode_attn_kv8_pos,
                                 e4m3_values, window)


def _decode_attn_kv8s_pos_impl(q, k8, v8, k_scale, v_scale, pos, scale, window=None):
    from ..ops.attention import decode_attn_kv8s_pos, decode_attn_kv8s_pos_supported
    from ..ops.kv8 import dequantise_rows

    return _decode_attn_e4m3_run(q, (k8, v8, k_scale, v_scale), (pos,), scale, decode_attn_kv8s_pos_supported,
                                 decode_attn_kv8s_pos, dequantise_rows, window)


hip_decode_attn_pos = ex.register_operator("hip_decode_attn_pos", meta=_decode_attn_pos_meta, fn=_decode_attn_pos_impl)
hip_decode_attn_kv8_pos = ex.register_operator("hip_decode_attn_kv8_pos", meta=_decode_attn_pos_meta,
                                               fn=_decode_attn_kv8_pos_impl)
hip_decode_attn_kv8s_pos = ex.register_operator(
    "hip_decode_attn_kv8s_pos", meta=lambda q, k8, v8, k_scale, v_scale, pos, scale: TensorProxy(like=q),
    fn=_decode_attn_kv8s_pos_impl)


# The paged forms (ops/kv_pages.py): pools [Hkv, R + 1, D] read through the block table, key counts from ``pos``.
def _decode_attn_paged_meta(q, k, v, pos, table, page_size, num_pages, scale):
    return TensorProxy(like=q)


def _paged_selector(caches, pos, table, page_size, num_pages, window=None):
    """The operands of the mask form: every pool's logical cache and the paged mask (under a sliding window the paged
    window mask)."""
    from ..ops.kv_pages import gather_pages, paged_mask, paged_window_mask

    mask = paged_mask(pos, table, page_size, num_pages) if window is None else \
        paged_window_mask(pos, table, page_size, num_pages, window)
    return [gather_pages(c, table, page_size) for c in caches], mask


def _decode_attn_paged_impl(q, k, v, pos, table, page_size, num_pages, scale, window=None):
    from ..ops.attention import decode_attn_paged, decode_attn_paged_supported

    if decode_attn_paged_supported(q, k, v, pos, table, page_size, num_pages):
        return decode_attn_paged(q, k, v, pos, table, page_size, num_pages, scale, window=window)
    caches, mask = _paged_selector((k, v), pos, table, page_size, num_pages, window)
    return _decode_attn_impl(q, *caches, mask, False, scale)


def _decode_attn_kv8_paged_impl(q, k8, v8, pos, table, page_size, num_pages, scale, window=None):
    from ..ops.attention import decode_attn_kv8_paged, decode_attn_kv8_paged_supported

    if decode_attn_kv8_paged_supported(q, k8, v8, pos, table, page_size, num_pages):
        return decode_attn_kv8_paged(q, k8, v8, pos, table, page_size, num_pages, scale, window=window)
    caches, mask = _paged_selector((k8, v8), pos, table, page_size, num_pages, window)
    return _decode_attn_kv8_impl(q, *caches, mask, False, scale)


def _decode_attn_kv8s_paged_impl(q, k8, v8, k_scale, v_scale, pos, table, page_size, num_pages, scale, window=None):
    from ..ops.attention import decode_attn_kv8s_paged, decode_attn_kv8s_paged_supported

    if decode_attn_kv8s_paged_supported(q, k8, v8, k_scale, v_scale, pos, table, page_size, num_pages):
        return decode_attn_kv8s_paged(q, k8, v8, k_scale, v_scale, pos, table, page_size, num_pages, scale,
                                      window=window)
    caches, mask = _paged_selector((k8, v8, k_scale, v_scale), pos, table, page_size, num_pages, window)
    return _decode_attn_kv8s_impl(q, *caches, mask, False, scale)


hip_decode_attn_paged = ex.register_operator("hip_decode_attn_paged", meta=_decode_attn_paged_meta,
                                             fn=_decode_attn_paged_impl)
hip_decode_attn_kv8_paged = ex.register_operator("hip_decode_attn_kv8_paged", meta=_decode_attn_paged_meta,
                                                 fn=_decode_attn_kv8_paged_impl)
hip_decode_attn_kv8s_paged = ex.register_operator(
    "hip_decode_attn_kv8s_paged",
    meta=lambda q, k8, v8, k_scale, v_scale, pos, table, page_size, num_pages, scale: TensorProxy(like=q),
    fn=_decode_attn_kv8s_paged_impl)


# The prefill forms (csrc/prefill_attention.hip): the position and paged forms above for any number of query rows, in
# place of the masked flash attention over the gathered / dequantised cache.  Each runs its kernel where
# ``*_supported`` takes the operands, else the program as the model spells it.
def _prefill_attn_pos_impl(q, k, v, pos, scale, window=None):
    from ..ops.attention import attn_fwd, prefill_attn_pos, prefill_attn_pos_supported

    if prefill_attn_pos_supported(q, k, v, pos):
        return prefill_attn_pos(q, k, v, pos, scale, window=window)
    return attn_fwd(q, k, v, False, scale, mask=_position_mask(pos, k.shape[2], window))[0]


def _prefill_attn_kv8_pos_impl(q, k8, v8, pos, scale, window=None):
    from ..ops.attention import prefill_attn_kv8_pos, prefill_attn_kv8_pos_supported
    from ..ops.kv8 import e4m3_values

    if prefill_attn_kv8_pos_supported(q, k8, v8, pos):
        return prefill_attn_kv8_pos(q, k8, v8, pos, scale, window=window)
    return _prefill_attn_pos_impl(q, e4m3_values(k8, q.dtype), e4m3_values(v8, q.dtype), pos, scale, window)


def _prefill_attn_kv8s_pos_impl(q, k8, v8, k_scale, v_scale, pos, scale, window=None):
    from ..ops.attention import prefill_attn_kv8s_pos, prefill_attn_kv8s_pos_supported
    from ..ops.kv8 import dequantise_rows

    if prefill_attn_kv8s_pos_supported(q, k8, v8, k_scale, v_scale, pos):
        return prefill_attn_kv8s_pos(q, k8, v8, k_scale, v_scale, pos, scale, window=window)
    return _prefill_attn_pos_impl(q, dequantise_rows(k8, k_scale, q.dtype), dequantise_rows(v8, v_scale, q.dtype), pos,
                                  scale, window)


def _prefill_attn_unpaged(q, caches, mask, scale):
    """The masked flash attention over gathered ``caches`` in operator order (k, v, then scale caches)."""
    from ..ops.attention import attn_fwd
    from ..ops.kv8 import dequantise_rows, e4m3_values

    if len(caches) == 4:
        k, v = dequantise_rows(caches[0], caches[2], q.dtype), dequantise_rows(caches[1], caches[3], q.dtype)
    elif caches[0].dtype == torch.uint8:
        k, v = e4m3_values(caches[0], q.dtype), e4m3_values(caches[1], q.dtype)
    else:
        k, v = caches
    return attn_fwd(q, k, v, False, scale, mask=mask)[0]


def _prefill_attn_paged_impl(q, k, v, pos, table, page_size, num_pages, scale, window=None):
    from ..ops.attention import prefill_attn_paged, prefill_attn_paged_supported

    if prefill_attn_paged_supported(q, k, v, pos, table, page_size, num_pages):
        return prefill_attn_paged(q, k, v, pos, table, page_size, num_pages, scale, window=window)
    return _prefill_attn_unpaged(q, *_paged_selector((k, v), pos, table, page_size, num_pages, window), scale)


def _prefill_attn_kv8_paged_impl(q, k8, v8, pos, table, page_size, num_pages, scale, window=None):
    from ..ops.attention import prefill_attn_kv8_paged, prefill_attn_kv8_paged_supported

    if prefill_attn_kv8_paged_supported(q, k8, v8, pos, table, page_size, num_pages):
        return prefill_attn_kv8_paged(q, k8, v8, pos, table, page_size, num_pages, scale, window=window)
    return _prefill_attn_unpaged(q, *_paged_selector((k8, v8), pos, table, page_size, num_pages, window), scale)


def _prefill_attn_kv8s_paged_impl(q, k8, v8, k_scale, v_scale, pos, table, page_size, num_pages, scale, window=None):
    from ..ops.attention import prefill_attn_kv8s_paged, prefill_attn_kv8s_paged_supported

    if prefill_attn_kv8s_paged_supported(q, k8, v8, k_scale, v_scale, pos, table, page_size, num_pages):
        return prefill_attn_kv8s_paged(q, k8, v8, k_scale, v_scale, pos, table, page_size, num_pages, scale,
                                       window=window)
    caches, mask = _paged_selector((k8, v8, k_scale, v_scale), pos, table, page_size, num_pages, window)
    return _prefill_attn_unpaged(q, caches, mask, scale)


hip_prefill_attn_pos = ex.register_operator("hip_prefill_attn_pos", meta=_decode_attn_pos_meta,
                                            fn=_prefill_attn_pos_impl)
hip_prefill_attn_kv8_pos = ex.register_operator("hip_prefill_attn_kv8_pos", meta=_decode_attn_pos_meta,
                                                fn=_prefill_attn_kv8_pos_impl)
hip_prefill_attn_kv8s_pos = ex.register_operator(
    "hip_prefill_attn_kv8s_pos", meta=lambda q, k8, v8, k_scale, v_scale, pos, scale: TensorProxy(like=q),
    fn=_prefill_attn_kv8s_pos_impl)
hip_prefill_attn_paged = ex.register_operator("hip_prefill_attn_paged", meta=_decode_attn_paged_meta,
                                              fn=_prefill_attn_paged_impl)
hip_prefill_attn_kv8_paged = ex.register_operator("hip_prefill_attn_kv8_paged", meta=_decode_attn_paged_meta,
                                                  fn=_prefill_attn_kv8_paged_impl)
hip_prefill_attn_kv8s_paged = ex.register_operator(
    "hip_prefill_attn_kv8s_paged",
    meta=lambda q, k8, v8, k_scale, v_scale, pos, table, page_size, num_pages, scale: TensorProxy(like=q),
    fn=_prefill_attn_kv8s_paged_impl)


# The window forms (a sliding window of ``window`` keys per row, its own included): every position / paged form above
# with ``window`` ahead of ``scale``, on the ``*_win`` entries of the two kernels.
def _pos_win_meta(q, k, v, pos, window, scale):
    return TensorProxy(like=q)


def _kv8s_pos_win_meta(q, k8, v8, k_scale, v_scale, pos, window, scale):
    return TensorProxy(like=q)


def _paged_win_meta(q, k, v, pos, table, page_size, num_pages, window, scale):
    return TensorProxy(like=q)


def _kv8s_paged_win_meta(q, k8, v8, k_scale, v_scale, pos, table, page_size, num_pages, window, scale):
    return TensorProxy(like=q)


def _windowed(impl):
    """``impl(..., scale, window)`` as the operator orders its operands: ``(..., window, scale)``."""
    def run(*a):
        return impl(*a[:-2], a[-1], a[-2])

    return run


_WINDOW_FORMS = {}  # a position / paged operator -> its window form
for _kind, _impls in (("decode", (_decode_attn_pos_impl, _decode_attn_kv8_pos_impl, _decode_attn_kv8s_pos_impl,
                                  _decode_attn_paged_impl, _decode_attn_kv8_paged_impl, _decode_attn_kv8s_paged_impl)),
                      ("prefill", (_prefill_attn_pos_impl, _prefill_attn_kv8_pos_impl, _prefill_attn_kv8s_pos_impl,
                                   _prefill_attn_paged_impl, _prefill_attn_kv8_paged_impl,
                                   _prefill_attn_kv8s_paged_impl))):
    for _form, _meta, _impl in zip(("pos", "kv8_pos", "kv8s_pos", "paged", "kv8_paged", "kv8s_paged"),
                                   (_pos_win_meta, _pos_win_meta, _kv8s_pos_win_meta, _paged_win_meta, _paged_win_meta,
                                    _kv8s_paged_win_meta), _impls):
        _name = f"hip_{_kind}_attn_{_form}"
        _WINDOW_FORMS[globals()[_name]] = globals()[_name + "_win"] = ex.register_operator(
            _name + "_win", meta=_meta, fn=_windowed(_impl))


def _broadcastable(shape, target) -> bool:
    if len(shape) > len(target):
        return False
    for a, b in zip(reversed(shape), reversed(target)):
        if a != 1 and a != b:
            return False
    return True


def _is_decode_shape(query, key, attn_mask) -> bool:
    from ..ops.attention import DECODE_MAX_QUERIES

    if attn_mask is None or not isinstance(attn_mask, TensorProxy) or attn_mask.dtype != torch.bool:
        return False
    B, Hq, T, _ = query.shape
    return T <= DECODE_MAX_QUERIES and _broadcastable(tuple(attn_mask.shape), (B, Hq, T, key.shape[2]))


def _is_decode(query, key, attn_mask) -> bool:
    """Few query rows against a KV cache with a boolean mask: the K3d decode kernel."""
    from ..ops.attention import DECODE_MAX_QUERIES

    if attn_mask is None or not isinstance(attn_mask, TensorProxy) or attn_mask.dtype != torch.bool:
        return False
    B, Hq, T, D = query.shape
    if D not in (64, 128):  # the decode kernel's head dims (others take the padded flash path)
        return False
    return T <= DECODE_MAX_QUERIES and _broadcastable(tuple(attn_mask.shape), (B, Hq, T, key.shape[2]))


def _sdpa_checker(query, key, value, attn_mask=None, dropout_p=0.0, is_causal=False, *, scale=None, enable_gqa=False):
    if not _gpu(query, key, value):
        return False
    if query.ndim != 4 or key.ndim != 4 or value.ndim != 4:
        return False
    try:
        p = float(pyval(dropout_p))
    except Exception:  # a symbolic dropout probability: let the decomposition run
        return False
    if not 0.0 <= p < 1.0:
        return False
    if attn_mask is not None:
        if not isinstance(attn_mask, TensorProxy) or attn_mask.device.type != "cuda":
            return False
        if attn_mask.dtype != torch.bool and not dtypes.is_float_dtype(attn_mask.dtype):
            return False
        if not _broadcastable(tuple(attn_mask.shape), (query.shape[0], query.shape[1], query.shape[2], key.shape[2])):
            return False
        if is_causal and attn_mask is not None:
            return False  # torch rejects the combination as well
    if query.dtype not in (torch.bfloat16, torch.float16) or key.dtype != query.dtype or value.dtype != query.dtype:
        return False
    D = query.shape[-1]
    from ..ops.attention import padded_head_dim, PLAIN_ONLY_HEAD_DIM

    if padded_head_dim(D) is None or key.shape[-1] != D or value.shape[-1] != D:
        return False
    if D > PLAIN_ONLY_HEAD_DIM and (attn_mask is not None or p > 0.0):
        return False
    if D not in (64, 128) and _is_decode_shape(query, key, attn_mask):
        return False  # decode steps at head dims without a decode kernel stay on ATen (padding buys nothing there)
    if key.shape[1] != value.shape[1] or query.shape[1] % key.shape[1] != 0:
        return False
    if key.shape[1] != query.shape[1] and not enable_gqa:
        return False
    return query.shape[0] == key.shape[0] == value.shape[0] and key.shape[2] == value.shape[2]


def _sc(q, scale):
    return scale if scale is not None else 1.0 / math.sqrt(q.shape[-1])


def _p(dropout_p) -> float:
    return float(pyval(dropout_p))


def _rng(query, key, p):
    """(seed, offset) of the framework's Philox stream, advanced by one draw per score."""
    if not p:
        return 0, 0
    from ..core import prims as P

    B, H, L, _ = query.shape
    return P.get_rng_seed_offset(B * H * L * key.shape[2])


def _sdpa_exec(query, key, value, attn_mask=None, dropout_p=0.0, is_causal=False, *, scale=None, enable_gqa=False):
    p = _p(dropout_p)
    if attn_mask is not None and not p and _is_decode(query, key, attn_mask):
        return hip_decode_attn(query, key, value, attn_mask, bool(is_causal), _sc(query, scale))
    if attn_mask is None and not p:
        out, _ = hip_attn_fwd(query, key, value, bool(is_causal), _sc(query, scale))
        return out
    seed, offset = _rng(query, key, p)
    out, _ = hip_attn_fwd_ex(query, key, value, attn_mask, bool(is_causal), _sc(query, scale), p, seed, offset)
    return out


def _sdpa_grad(query, key, value, attn_mask=None, dropout_p=0.0, is_causal=False, *, scale=None, enable_gqa=False):
    sc = _sc(query, scale)
    p = _p(dropout_p)
    if attn_mask is None and not p:
        out, lse = hip_attn_fwd(query, key, value, bool(is_causal), sc)

        def bwd(g):
            dq, dk, dv = hip_attn_bwd(g, query, key, value, out, lse, bool(is_causal), sc)
            return dq, dk, dv

        return out, bwd
    seed, offset = _rng(query, key, p)
    out, lse = hip_attn_fwd_ex(query, key, value, attn_mask, bool(is_causal), sc, p, seed, offset)
    mask_grad = bool(attn_mask is not None and attn_mask.dtype != torch.bool and attn_mask.requires_grad)

    def bwd(g):
        res = hip_attn_bwd_ex(g, query, key, value, out, lse, attn_mask, bool(is_causal), sc, p, seed, offset, mask_grad)
        if mask_grad:
            return res[0], res[1], res[2], res[3]
        return res[0], res[1], res[2]

    return out, bwd


# =========================================================================================
# K11 embedding backward / index_add, K12 topk / sort / cumsum (csrc/index_ops.hip)
# =========================================================================================
_SORT_DT = (torch.float32, torch.float16, torch.bfloat16, torch.int32)
_ROW_DT = (torch.float32, torch.float16, torch.bfloat16)
_SORT_MAX = 16384


def _topk_meta(a, k, dim, largest, sorted):
    shape = list(a.shape)
    shape[dim] = k
    return TensorProxy(like=a, shape=tuple(shape)), TensorProxy(like=a, shape=tuple(shape), dtype=torch.int64,
                                                                requires_grad=False)


def _topk_impl(a, k, dim, largest, sorted):
    from ..ops import index_ops

    return index_ops.topk(a, k, dim, largest, sorted)


def _sort_meta(a, dim, descending, stable):
    return TensorProxy(like=a), TensorProxy(like=a, dtype=torch.int64, requires_grad=False)


def _sort_impl(a, dim, descending, stable):
    from ..ops import index_ops

    return index_ops.sort(a, dim, descending, stable)


def _cumsum_meta(a, dim, out_i32=False):
    if a.dtype in (torch.int32, torch.int64):
        return TensorProxy(like=a, dtype=torch.int32 if out_i32 else torch.int64)
    return TensorProxy(like=a)


def _cumsum_impl(a, dim, out_i32=False):
    from ..ops import index_ops

    return index_ops.cumsum(a, dim, torch.int32 if out_i32 else None)


def _emb_bwd_meta(grad, indices, num_weights, padding_idx, scale_grad_by_freq):
    return TensorProxy(like=grad, shape=(num_weights, grad.shape[-1]))


def _emb_bwd_impl(grad, indices, num_weights, padding_idx, scale_grad_by_freq):
    from ..ops import index_ops

    return index_ops.embedding_backward(grad, indices, num_weights, padding_idx, scale_grad_by_freq)


def _index_add_meta(a, index, src):
    return TensorProxy(like=a)


def _index_add_impl(a, index, src):
    from ..ops import index_ops

    return index_ops.index_add(a, index, src)


hip_topk = ex.register_operator("hip_topk", meta=_topk_meta, fn=_topk_impl)
hip_sort = ex.register_operator("hip_sort", meta=_sort_meta, fn=_sort_impl)
hip_cumsum = ex.register_operator("hip_cumsum", meta=_cumsum_meta, fn=_cumsum_impl)
hip_embedding_backward = ex.register_operator("hip_embedding_backward", meta=_emb_bwd_meta, fn=_emb_bwd_impl)
hip_index_add = ex.register_operator("hip_index_add", meta=_index_add_meta, fn=_index_add_impl)


def _numel(shape) -> int:
    n = 1
    for d in shape:
        n = n * d  # symbolic dims stay symbolic (core/symbolic.py)
    return n


def _topk_checker(a, k, dim, largest, sorted):
    if not (_gpu(a) and a.dtype in _SORT_DT and a.ndim >= 1 and _numel(a.shape) > 0):
        return False
    n = a.shape[dim]
    return 1 <= pyval(k) <= n <= _SORT_MAX


def _topk_exec(a, k, dim, largest, sorted):
    return hip_topk(a, pyval(k), dim, bool(largest), bool(sorted))


def _sort_checker(a, dim, descending, stable):
    if a.dtype == torch.int64:  # 64-bit keys + separate positions: half the LDS capacity
        return _gpu(a) and a.ndim >= 1 and _numel(a.shape) > 0 and a.shape[dim] <= _SORT_MAX // 2
    return (_gpu(a) and a.dtype in _SORT_DT and a.ndim >= 1 and _numel(a.shape) > 0
            and a.shape[dim] <= _SORT_MAX)


def _sort_exec(a, dim, descending, stable):
    return hip_sort(a, dim, bool(descending), bool(stable))


def _cumsum_checker(a, dim, *, dtype=None):
    if not (_gpu(a) and a.ndim >= 1 and 0 < _numel(a.shape) < 2**31):
        return False
    if a.dtype in _ROW_DT:
        return dtype is None or dtype == a.dtype
    # integer scans accumulate in int64; the output dtype is the prim's (int64, or int32 for an
    # int32 scan, which is what ltorch.cumsum(..., dtype=torch.int32) lowers to)
    return a.dtype in (torch.int32, torch.int64) and dtype in (None, torch.int64, torch.int32)


def _cumsum_exec(a, dim, *, dtype=None):
    out = dtype or a.dtype
    return hip_cumsum(a, dim, out == torch.int32)


def _emb_bwd_checker(grad, indices, num_weights, padding_idx, scale_grad_by_freq, sparse):
    if sparse or not _gpu(grad, indices) or grad.dtype not in _ROW_DT or indices.dtype not in (torch.int32, torch.int64):
        return False
    D = grad.shape[-1]
    return (D % (16 // grad.dtype.itemsize) == 0 and 0 < pyval(num_weights) < 2**31
            and _numel(indices.shape) * D == _numel(grad.shape))


def _emb_bwd_exec(grad, indices, num_weights, padding_idx, scale_grad_by_freq, sparse):
    pidx = pyval(padding_idx)
    return hip_embedding_backward(grad, indices, pyval(num_weights), -1 if pidx is None else pidx,
                                  bool(scale_grad_by_freq))


def _index_add_checker(a, indices, value, dim):
    if not (_gpu(a, indices, value) and a.ndim >= 1 and dim == 0 and a.dtype in _ROW_DT and value.dtype == a.dtype):
        return False
    if indices.dtype not in (torch.int32, torch.int64) or indices.ndim > 1 or value.ndim != a.ndim:
        return False
    D = _numel(a.shape[1:])
    return (D > 0 and D % (16 // a.dtype.itemsize) == 0 and tuple(value.shape[1:]) == tuple(a.shape[1:])
            and value.shape[0] == _numel(indices.shape))


def _index_add_exec(a, indices, value, dim):
    return hip_index_add(a, indices, value)


def _cdim(a, dim):
    d = pyval(dim)
    return d % a.ndim if a.ndim else 0


# ltorch-level claims (the torch executor would otherwise take ltorch.argsort / cumsum whole)
def _lt_topk_checker(a, k, dim=-1, largest=True, sorted=True):
    return a.ndim >= 1 and _topk_checker(a, k, _cdim(a, dim), largest, sorted)


def _lt_topk_exec(a, k, dim=-1, largest=True, sorted=True):
    return hip_topk(a, pyval(k), _cdim(a, dim), bool(pyval(largest)), bool(pyval(sorted)))


def _lt_sort_checker(a, dim=-1, descending=False, stable=False):
    return a.ndim >= 1 and _sort_checker(a, _cdim(a, dim), descending, stable)


def _lt_sort_exec(a, dim=-1, descending=False, stable=False):
    return hip_sort(a, _cdim(a, dim), bool(pyval(descending)), bool(pyval(stable)))


def _lt_argsort_exec(a, dim=-1, descending=False, stable=False):
    return hip_sort(a, _cdim(a, dim), bool(pyval(descending)), bool(pyval(stable)))[1]


def _lt_cumsum_checker(a, dim, *, dtype=None):
    if not (_gpu(a) and a.ndim >= 1 and 0 < _numel(a.shape) < 2**31):
        return False
    if a.dtype in _ROW_DT:
        return dtype is None or dtype == a.dtype
    return a.dtype in (torch.int32, torch.int64, torch.bool, torch.uint8, torch.int8, torch.int16) and \
        dtype in (None, torch.int64, torch.int32) and a.dtype in (torch.int32, torch.int64)


def _lt_cumsum_exec(a, dim, *, dtype=None):
    # torch: integer cumsum promotes to int64 unless dtype says otherwise
    return hip_cumsum(a, _cdim(a, dim), dtype == torch.int32)


def _register_all():
    from .. import torch as ltorch
    from ..core import prims as P

    ex.register_implementation(ltorch.topk, checker=_lt_topk_checker, execution_transform=_lt_topk_exec)
    ex.register_implementation(ltorch.sort, checker=_lt_sort_checker, execution_transform=_lt_sort_exec)
    ex.register_implementation(ltorch.argsort, checker=_lt_sort_checker, execution_transform=_lt_argsort_exec)
    ex.register_implementation(ltorch.cumsum, checker=_lt_cumsum_checker, execution_transform=_lt_cumsum_exec)

    ex.register_implementation(P.topk, checker=_topk_checker, execution_transform=_topk_exec)
    ex.register_implementation(P.sort, checker=_sort_checker, execution_transform=_sort_exec)
    ex.register_implementation(P.cumsum, checker=_cumsum_checker, execution_transform=_cumsum_exec)
    ex.register_implementation(P.embedding_backward, checker=_emb_bwd_checker, execution_transform=_emb_bwd_exec)
    ex.register_implementation(P.index_add, checker=_index_add_checker, execution_transform=_index_add_exec)
    from ..core.transforms import register_vjp
    from ..models import litgpt

    ex.register_implementation(ltorch.rms_norm, checker=_rms_checker, execution_transform=_rms_exec, grad_transform=_rms_grad)
    ex.register_implementation(ltorch.layer_norm, checker=_ln_checker, execution_transform=_ln_exec, grad_transform=_ln_grad)
    ex.register_implementation(ltorch._grouped_mm, checker=_gmm_checker, execution_transform=_gmm_exec)
    ex.register_implementation(ltorch.cross_entropy, checker=_ce_checker, execution_transform=_ce_exec, grad_transform=_ce_grad)
    ex.register_implementation(ltorch.scaled_dot_product_attention, checker=_sdpa_checker, execution_transform=_sdpa_exec,
                               grad_transform=_sdpa_grad)
    register_vjp(hip_qkv_rope)(_qkv_rope_vjp)
    register_vjp(hip_swiglu)(_swiglu_vjp)
    ex.register_python_lookaside(litgpt, "qkv_split_rope", qkv_split_rope_lookaside)
    ex.register_python_lookaside(litgpt, "swiglu", swiglu_lookaside)


_register_all()
