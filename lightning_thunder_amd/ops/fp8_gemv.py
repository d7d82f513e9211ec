"""Weight-only e4m3 decode GEMV (W8A16): bf16 activations against a per-tensor-scaled OCP e4m3 weight.

The weight is what ``transforms/fp8_inference.py`` ``quantize_weight_e4m3`` stores: ``q = e4m3(w * scale)``
as uint8 [N, K] plus one fp32 device scalar ``scale``.  ``csrc/gemv_fp8.hip`` streams the bytes once for up
to 8 activation rows, unpacks them with the hardware conversion, accumulates ``x . q`` in fp32 and applies
``1 / scale`` once, with the RMSNorm prologue, the gated (SwiGLU) pair, the bias / activation / residual
epilogue and up to three grouped projections that ``csrc/gemv.hip`` and ``csrc/mxfp4.hip`` carry.  The
scale is read in the kernel, so nothing here synchronises with the host.
"""
from __future__ import annotations

import ctypes

import torch

from ._lib import require, stream_ptr, check, register_signature, c_int, c_float, c_void_p
from .mxfp4 import _FUSED_ACT, _act_reference, _ptr

register_signature("lta_gemv_e4m3_fused", [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_float,
                                           c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int,
                                           c_int, c_void_p])
register_signature("lta_gemv_e4m3_group", [c_void_p, c_void_p, c_int, c_float, c_int, c_void_p, c_void_p, c_void_p,
                                           c_void_p, c_void_p, c_int, c_int, c_int, c_void_p])
GEMV_MAX_ROWS = 8
PIECE = 16  # weights per 16-byte load: K must be a multiple


def dequantize(q: torch.Tensor, scale: torch.Tensor, dtype=torch.float32) -> torch.Tensor:
    """``q / scale`` (``dequantize_e4m3`` of the transform, fp32 by default)."""
    return (q.view(torch.float8_e4m3fn).float() / scale).to(dtype)


def gemv_fused_reference(x: torch.Tensor, q: torch.Tensor, scale: torch.Tensor, *, bias=None, residual=None, act=None,
                         gate_q=None, gate_scale=None, norm: bool = False, norm_weight=None,
                         eps: float = 1e-5) -> torch.Tensor:
    """Pure-torch specification of ``gemv_fused`` (and its fallback for operands the kernel does not
    take): RMSNorm rounded to x's dtype; the product against ``dequantize(q, scale)`` in fp32; with a gate
    weight both products rounded to x's dtype and ``act(a) * b``, otherwise ``act(a + bias) + residual``
    in fp32; one final rounding."""
    dt = x.dtype
    xf = x.float()
    if norm:
        xf = xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)
        if norm_weight is not None:
            xf = xf * norm_weight.float()
        xf = xf.to(dt).float()
    v = xf @ dequantize(q, scale).T
    if gate_q is not None:
        if bias is not None or residual is not None:
            raise ValueError("gemv_fused: a gated pair takes no bias or residual")
        b = (xf @ dequantize(gate_q, gate_scale).T).to(dt).float()
        v = _act_reference(v.to(dt).float(), act) * b
    else:
        if bias is not None:
            v = v + bias.float()
        v = _act_reference(v, act)
        if residual is not None:
            v = v + residual.float()
    return v.to(dt)


def _weight_ok(q, scale, K: int) -> bool:
    return (q.dim() == 2 and q.dtype == torch.uint8 and q.is_cuda and q.shape[1] == K and q.is_contiguous()
            and q.data_ptr() % 16 == 0 and scale.is_cuda and scale.dtype == torch.float32 and scale.numel() == 1)


def gemv_fused_supported(x: torch.Tensor, q: torch.Tensor, scale: torch.Tensor, *, bias=None, residual=None, act=None,
                         gate_q=None, gate_scale=None, norm_weight=None) -> bool:
    """Whether ``gemv_fused`` / ``gemv_group`` take these operands: x [1..8, K] bf16 on the GPU with
    K % 16 == 0, unit element stride, a row stride that is a multiple of 8 and a 16-byte aligned base;
    a contiguous uint8 weight with an fp32 scalar scale on the device; bf16 bias / residual / norm weight."""
    if not x.is_cuda or x.dtype != torch.bfloat16 or x.dim() != 2 or act not in _FUSED_ACT:
        return False
    M, K = x.shape
    if not 1 <= M <= GEMV_MAX_ROWS or K < PIECE or K % PIECE or x.stride(1) != 1 or x.stride(0) % 8 or x.data_ptr() % 16:
        return False
    if not _weight_ok(q, scale, K):
        return False
    N = q.shape[0]
    if (gate_q is None) != (gate_scale is None):
        return False
    if gate_q is not None and (bias is not None or residual is not None or not _weight_ok(gate_q, gate_scale, K)
                               or gate_q.shape != q.shape):
        return False
    if bias is not None and (bias.dtype != x.dtype or bias.numel() != N or not bias.is_contiguous()):
        return False
    if residual is not None and (residual.dtype != x.dtype or tuple(residual.shape) != (M, N)
                                 or residual.stride(1) != 1):
        return False
    if norm_weight is not None and (norm_weight.dtype != x.dtype or norm_weight.numel() != K
                                    or not norm_weight.is_contiguous() or norm_weight.data_ptr() % 16):
        return False
    return True


def gemv_fused(x: torch.Tensor, q: torch.Tensor, scale: torch.Tensor, *, bias=None, residual=None, act=None,
               gate_q=None, gate_scale=None, norm: bool = False, norm_weight=None, eps: float = 1e-5,
               out: torch.Tensor | None = None) -> torch.Tensor:
    """``act(x' . (q / scale)^T + bias) + residual`` for x [M <= 8, K] bf16 in one launch of the e4m3
    weight-streaming kernel (``csrc/gemv_fp8.hip``).  ``norm=True``: ``x' = rmsnorm(x) * norm_weight``;
    ``gate_q`` / ``gate_scale`` (q's shape): ``act(x' W^T) * (x' Wg^T)``, the SwiGLU up-projection pair.
    ``out``: a bf16 [M, N] view with unit element stride to write into.  Operands must satisfy
    ``gemv_fused_supported``."""
    if not gemv_fused_supported(x, q, scale, bias=bias, residual=residual, act=act, gate_q=gate_q,
                                gate_scale=gate_scale, norm_weight=norm_weight):
        raise ValueError(f"gemv_fused: unsupported operands x {tuple(x.shape)} {x.dtype}, q {tuple(q.shape)}")
    M, K = x.shape
    N = q.shape[0]
    y = torch.empty((M, N), dtype=x.dtype, device=x.device) if out is None else out
    if tuple(y.shape) != (M, N) or y.dtype != x.dtype or y.stride(1) != 1:
        raise ValueError("gemv_fused: out must be a bf16 [M, N] tensor with unit element stride")
    check(require().lta_gemv_e4m3_fused(x.data_ptr(), q.data_ptr(), scale.data_ptr(), _ptr(gate_q), _ptr(gate_scale),
                                        _ptr(norm_weight), int(norm), float(eps), _ptr(bias), _ptr(residual),
                                        y.data_ptr(), M, N, K, x.stride(0), y.stride(0),
                                        0 if residual is None else residual.stride(0), _FUSED_ACT[act],
                                        stream_ptr(x.device)), "lta_gemv_e4m3_fused")
    return y


def gemv(x: torch.Tensor, q: torch.Tensor, scale: torch.Tensor, bias: torch.Tensor | None = None) -> torch.Tensor:
    """Weight-only e4m3 decode product: bf16 [..., N] = x [..., K] (bf16, <= 8 rows) . (q / scale)^T (+ bias)."""
    x2 = x.reshape(-1, x.shape[-1])
    if x2.stride(-1) != 1 or x2.stride(0) % 8 or x2.data_ptr() % 16:
        x2 = x2.contiguous()  # the kernel reads x with 16-byte vector loads
        if x2.data_ptr() % 16:
            x2 = x2.clone()
    if bias is not None:
        bias = bias.to(torch.bfloat16).contiguous()
    return gemv_fused(x2, q, scale, bias=bias).reshape(*x.shape[:-1], q.shape[0])


def gemv_group(x: torch.Tensor, weights, *, norm: bool = False, norm_weight=None, eps: float = 1e-5,
               packed: bool = False):
    """``[x' . (q / scale)^T for (q, scale) in weights]`` (<= 3 weights sharing x and the norm, e.g.
    attention q / k / v) in ONE launch.  ``packed``: the outputs are adjacent column ranges of one
    [M, sum N] tensor, returned alone."""
    if not 1 <= len(weights) <= 3:
        raise ValueError("gemv_group takes 1 to 3 weights")
    for q, s in weights:
        if not gemv_fused_supported(x, q, s, norm_weight=norm_weight):
            raise ValueError(f"gemv_group: unsupported operands x {tuple(x.shape)} {x.dtype}, q {tuple(q.shape)}")
    M, K = x.shape
    ns = [q.shape[0] for q, _ in weights]
    if packed:
        buf = torch.empty((M, sum(ns)), dtype=x.dtype, device=x.device)
        outs = list(buf.split(ns, dim=1))
    else:
        outs = [torch.empty((M, n), dtype=x.dtype, device=x.device) for n in ns]
    n = len(weights)
    pad = [None] * (3 - n)
    qs = (ctypes.c_void_p * 3)(*[q.data_ptr() for q, _ in weights], *pad)
    ss = (ctypes.c_void_p * 3)(*[s.data_ptr() for _, s in weights], *pad)
    ys = (ctypes.c_void_p * 3)(*[o.data_ptr() for o in outs], *pad)
    nn = (ctypes.c_int * 3)(*ns, *([0] * (3 - n)))
    ldy = (ctypes.c_int * 3)(*[o.stride(0) for o in outs], *([0] * (3 - n)))
    check(require().lta_gemv_e4m3_group(x.data_ptr(), _ptr(norm_weight), int(norm), float(eps), n,
                                        ctypes.cast(qs, c_void_p), ctypes.cast(ss, c_void_p),
                                        ctypes.cast(ys, c_void_p), ctypes.cast(nn, c_void_p),
                                        ctypes.cast(ldy, c_void_p), M, K, x.stride(0), stream_ptr(x.device)),
          "lta_gemv_e4m3_group")
    return buf if packed else outs
