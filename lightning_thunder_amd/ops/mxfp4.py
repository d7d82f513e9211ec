"""MXFP4 (OCP microscaling, e2m1 elements, one E8M0 scale per 32 along the reduction dim) on CDNA4.

gfx950's block-scaled MFMA (``v_mfma_scale_f32_16x16x128_f8f6f4``, format 4) multiplies e2m1
operands at 4x the bf16 rate per clock with the E8M0 scales applied in hardware, so an MXFP4 GEMM
reads a quarter of the bf16 operand bytes and needs no dequantisation pass.  Storage: two
elements per byte (low nibble = even index, ``torch.float4_e2m1fn_x2`` layout), scales as uint8
(``torch.float8_e8m0fnu`` layout).  Kernels: ``csrc/fp8.hip`` ``mx4_cast_kernel`` (quantise) and
``csrc/gemm.hip`` ``gemm_nt_mxfp4_kernel`` (NT GEMM, bf16 out, optional bias).

The reference has no MXFP4 path (its fp4 support is the dtype, ``thunder/core/dtypes.py``); this
is the MI355X-native counterpart of its MXFP8 TransformerEngine recipe for 4-bit inference.
"""
from __future__ import annotations

import torch

import ctypes

from ._lib import require, stream_ptr, check, register_signature, c_int, c_int64, c_float, c_void_p, DTYPE_CODE

register_signature("lta_mxfp4_cast", [c_int, c_void_p, c_void_p, c_void_p, c_int64, c_void_p])
register_signature("lta_gemm_nt_mxfp4", [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int,
                                         c_int, c_int, c_int, c_int, c_void_p])
register_signature("lta_gemv_mxfp4", [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                                      c_int, c_void_p])
register_signature("lta_gemv_mxfp4_fused", [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_float,
                                            c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int,
                                            c_int, c_void_p])
register_signature("lta_gemv_mxfp4_group", [c_void_p, c_void_p, c_int, c_float, c_int, c_void_p, c_void_p, c_void_p,
                                            c_void_p, c_void_p, c_int, c_int, c_int, c_void_p])
GEMV_MAX_ROWS = 8

BLOCK = 32
E2M1_MAX = 6.0


def _e8m0_exponent(amax: torch.Tensor) -> torch.Tensor:
    """Biased E8M0 exponent per block: the smallest 2^s with amax / 2^s <= 6 (mantissa > 1.5 rounds
    the exponent up), 0 for an all-zero block (as ``mx4_exp`` in csrc/fp8.hip)."""
    m, e = torch.frexp(amax)  # amax = m * 2^e, m in [0.5, 1)
    e = e - 1  # floor(log2 amax)
    above = (m * 2) > 1.5
    s = e - 2 + above.to(e.dtype)
    be = torch.clamp(s + 127, 0, 254)
    return torch.where(amax > 0, be, torch.zeros_like(be)).to(torch.uint8)


def _e2m1_codes(v: torch.Tensor) -> torch.Tensor:
    """Round-to-nearest-even e2m1 codes (4-bit, sign in bit 3) of |v| <= 6."""
    a = v.abs()
    code = torch.zeros_like(a, dtype=torch.int32)
    # thresholds: (value, inclusive) — ties go to the even code
    for i, (t, incl) in enumerate(((0.25, False), (0.75, True), (1.25, False), (1.75, True), (2.5, False),
                                   (3.5, True), (5.0, False))):
        code += (a >= t if incl else a > t).to(torch.int32)
    neg = (v < 0) & (code != 0)
    return code | (neg.to(torch.int32) << 3)


def quantize_reference(x: torch.Tensor):
    """Pure-torch MXFP4 quantisation of ``x [..., C]`` along the last dim: (q [R, C/2] uint8,
    s [R, C/32] uint8) — the specification the HIP kernel is tested against."""
    x2 = x.reshape(-1, x.shape[-1]).float()
    R, C = x2.shape
    xb = x2.reshape(R, C // BLOCK, BLOCK)
    be = _e8m0_exponent(xb.abs().amax(-1))
    scale = torch.exp2(127.0 - be.float()).unsqueeze(-1)
    codes = _e2m1_codes(xb * scale).reshape(R, C)
    q = (codes[:, 0::2] | (codes[:, 1::2] << 4)).to(torch.uint8)
    return q, be


def _e2m1_value(c: torch.Tensor) -> torch.Tensor:
    """fp32 value of 4-bit e2m1 codes, computed elementwise (no host tensors: usable while a
    graph is being captured)."""
    c = c.to(torch.int32)
    e = (c >> 1) & 3
    m = (c & 1).to(torch.float32)
    mag = torch.where(e == 0, 0.5 * m, torch.exp2((e - 1).to(torch.float32)) * (1.0 + 0.5 * m))
    return torch.where((c & 8) != 0, -mag, mag)


def dequantize(q: torch.Tensor, s: torch.Tensor, dtype=torch.float32) -> torch.Tensor:
    """(q [R, C/2], s [R, C/32]) -> [R, C] (exact: every e2m1 value times a power of two)."""
    vals = torch.stack([_e2m1_value(q & 0xF), _e2m1_value(q >> 4)], -1).reshape(q.shape[0], -1)
    scale = torch.exp2(s.float() - 127.0).repeat_interleave(BLOCK, dim=1)
    return (vals * scale).to(dtype)


def quantize(x: torch.Tensor):
    """MXFP4-quantise ``x [..., C]`` (bf16 / fp32, C % 32 == 0) along the last dim on the GPU."""
    x2 = x.reshape(-1, x.shape[-1])
    if not x2.is_contiguous():
        x2 = x2.contiguous()
    R, C = x2.shape
    if C % BLOCK:
        raise ValueError(f"MXFP4 needs the last dim to be a multiple of {BLOCK}, got {C}")
    if not x2.is_cuda:
        return quantize_reference(x2)
    q = torch.empty((R, C // 2), dtype=torch.uint8, device=x.device)
    s = torch.empty((R, C // BLOCK), dtype=torch.uint8, device=x.device)
    check(require().lta_mxfp4_cast(DTYPE_CODE[x2.dtype], x2.data_ptr(), q.data_ptr(), s.data_ptr(), x2.numel(),
                                   stream_ptr(x.device)), "lta_mxfp4_cast")
    return q, s


def gemm_nt(a: torch.Tensor, sa: torch.Tensor, b: torch.Tensor, sb: torch.Tensor,
            bias: torch.Tensor | None = None) -> torch.Tensor:
    """bf16 [M, N] = dequant(a) [M, K] . dequant(b) [N, K]^T (+ bias) on the block-scaled MFMA:
    a [M, K/2], b [N, K/2] packed e2m1; sa [M, K/32], sb [N, K/32] E8M0.  M, N % 256, K % 256."""
    M, K = a.shape[0], a.shape[1] * 2
    N = b.shape[0]
    if M % 256 or N % 256 or K % 256 or b.shape[1] * 2 != K:
        raise ValueError(f"gemm_nt_mxfp4: unsupported shape M={M} N={N} K={K}")
    if sa.shape != (M, K // BLOCK) or sb.shape != (N, K // BLOCK):
        raise ValueError("gemm_nt_mxfp4: scale shapes must be [M, K/32] and [N, K/32]")
    for t in (a, b, sa, sb):
        if not t.is_contiguous() or t.dtype != torch.uint8:
            raise ValueError("gemm_nt_mxfp4: operands and scales must be contiguous uint8")
    out = torch.empty((M, N), dtype=torch.bfloat16, device=a.device)
    if bias is not None:
        bias = bias.to(torch.bfloat16).contiguous()
    check(require().lta_gemm_nt_mxfp4(a.data_ptr(), b.data_ptr(), out.data_ptr(),
                                      None if bias is None else bias.data_ptr(), sa.data_ptr(), sb.data_ptr(), M, N,
                                      K, a.stride(0), b.stride(0), out.stride(0), stream_ptr(a.device)),
          "lta_gemm_nt_mxfp4")
    return out


def gemv(x: torch.Tensor, q: torch.Tensor, s: torch.Tensor, bias: torch.Tensor | None = None) -> torch.Tensor:
    """Weight-only MXFP4 decode product: bf16 [M, N] = x [M, K] (bf16, M <= 8) . dequant(q, s)^T (+ bias),
    streaming the 4-bit weight once (``csrc/mxfp4.hip``)."""
    x2 = x.reshape(-1, x.shape[-1])
    M, K = x2.shape
    N = q.shape[0]
    if M > GEMV_MAX_ROWS or q.shape[1] * 2 != K or s.shape != (N, K // BLOCK) or x2.dtype != torch.bfloat16:
        raise ValueError(f"gemv_mxfp4: unsupported operands x {tuple(x2.shape)} {x2.dtype}, q {tuple(q.shape)}")
    if x2.stride(-1) != 1 or x2.stride(0) % 8 or x2.data_ptr() % 16:
        x2 = x2.contiguous()  # the kernel reads x with 16-B vector loads
        if x2.data_ptr() % 16:
            x2 = x2.clone()
    y = torch.empty((M, N), dtype=torch.bfloat16, device=x.device)
    if bias is not None:
        bias = bias.to(torch.bfloat16).contiguous()
    check(require().lta_gemv_mxfp4(x2.data_ptr(), q.data_ptr(), s.data_ptr(), None if bias is None else bias.data_ptr(),
                                   y.data_ptr(), M, N, K, x2.stride(0), y.stride(0), stream_ptr(x.device)),
          "lta_gemv_mxfp4")
    return y.reshape(*x.shape[:-1], N)


# ---- decode GEMV with the norm prologue / gated pair / bias-activation-residual epilogue ------------
_FUSED_ACT = {None: 0, "none": 0, "gelu_tanh": 1, "silu": 3, "relu": 4}  # codes of ops/gemm.py ACT


def _act_reference(v: torch.Tensor, act) -> torch.Tensor:
    if act in (None, "none"):
        return v
    if act == "silu":
        return torch.nn.functional.silu(v)
    if act == "gelu_tanh":
        return torch.nn.functional.gelu(v, approximate="tanh")
    if act == "relu":
        return torch.relu(v)
    raise ValueError(f"gemv_fused: unsupported activation {act!r}")


def gemv_fused_reference(x: torch.Tensor, q: torch.Tensor, s: torch.Tensor, *, bias=None, residual=None, act=None,
                         gate_q=None, gate_s=None, norm: bool = False, norm_weight=None,
                         eps: float = 1e-5) -> torch.Tensor:
    """Pure-torch specification of ``gemv_fused`` (and its fallback for operands the kernel does
    not take): RMSNorm rounded to x's dtype; the product against ``dequantize(q, s)`` in fp32; with
    a gate weight both products rounded to x's dtype and ``act(a) * b``, otherwise ``act(a + bias)
    + residual`` in fp32; one final rounding."""
    dt = x.dtype
    xf = x.float()
    if norm:
        xf = xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)
        if norm_weight is not None:
            xf = xf * norm_weight.float()
        xf = xf.to(dt).float()
    v = xf @ dequantize(q, s).T
    if gate_q is not None:
        if bias is not None or residual is not None:
            raise ValueError("gemv_fused: a gated pair takes no bias or residual")
        b = (xf @ dequantize(gate_q, gate_s).T).to(dt).float()
        v = _act_reference(v.to(dt).float(), act) * b
    else:
        if bias is not None:
            v = v + bias.float()
        v = _act_reference(v, act)
        if residual is not None:
            v = v + residual.float()
    return v.to(dt)


def _weight_ok(q, s, K: int) -> bool:
    return (q.dim() == 2 and q.dtype == torch.uint8 and s.dtype == torch.uint8 and q.is_cuda and s.is_cuda
            and q.shape[1] * 2 == K and tuple(s.shape) == (q.shape[0], K // BLOCK) and q.is_contiguous()
            and s.is_contiguous())


def gemv_fused_supported(x: torch.Tensor, q: torch.Tensor, s: torch.Tensor, *, bias=None, residual=None, act=None,
                         gate_q=None, gate_s=None, norm_weight=None) -> bool:
    """Whether ``gemv_fused`` / ``gemv_group`` take these operands: x [1..8, K] bf16 on the GPU with
    K % 32 == 0, unit element stride, a row stride that is a multiple of 8 and a 16-byte aligned
    base; contiguous packed weights and scales; bf16 bias / residual / norm weight."""
    if not x.is_cuda or x.dtype != torch.bfloat16 or x.dim() != 2 or act not in _FUSED_ACT:
        return False
    M, K = x.shape
    if not 1 <= M <= GEMV_MAX_ROWS or K < BLOCK or K % BLOCK or x.stride(1) != 1 or x.stride(0) % 8 or x.data_ptr() % 16:
        return False
    if not _weight_ok(q, s, K):
        return False
    N = q.shape[0]
    if (gate_q is None) != (gate_s is None):
        return False
    if gate_q is not None and (bias is not None or residual is not None or not _weight_ok(gate_q, gate_s, K)
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


def _ptr(t):
    return None if t is None else t.data_ptr()


def gemv_fused(x: torch.Tensor, q: torch.Tensor, s: torch.Tensor, *, bias=None, residual=None, act=None, gate_q=None,
               gate_s=None, norm: bool = False, norm_weight=None, eps: float = 1e-5) -> torch.Tensor:
    """``act(x' . dequant(q, s)^T + bias) + residual`` for x [M <= 8, K] bf16 in one launch of the
    4-bit weight-streaming kernel (``csrc/mxfp4.hip``).  ``norm=True``: ``x' = rmsnorm(x) *
    norm_weight``; ``gate_q`` / ``gate_s`` (same shape as q / s): ``act(x' W^T) * (x' Wg^T)``, the
    SwiGLU up-projection pair.  Operands must satisfy ``gemv_fused_supported``."""
    if not gemv_fused_supported(x, q, s, bias=bias, residual=residual, act=act, gate_q=gate_q, gate_s=gate_s,
                                norm_weight=norm_weight):
        raise ValueError(f"gemv_fused: unsupported operands x {tuple(x.shape)} {x.dtype}, q {tuple(q.shape)}")
    M, K = x.shape
    N = q.shape[0]
    y = torch.empty((M, N), dtype=x.dtype, device=x.device)
    check(require().lta_gemv_mxfp4_fused(x.data_ptr(), q.data_ptr(), s.data_ptr(), _ptr(gate_q), _ptr(gate_s),
                                         _ptr(norm_weight), int(norm), float(eps), _ptr(bias), _ptr(residual),
                                         y.data_ptr(), M, N, K, x.stride(0), y.stride(0),
                                         0 if residual is None else residual.stride(0), _FUSED_ACT[act],
                                         stream_ptr(x.device)), "lta_gemv_mxfp4_fused")
    return y


def gemv_group(x: torch.Tensor, weights, *, norm: bool = False, norm_weight=None, eps: float = 1e-5,
               packed: bool = False):
    """``[x' . dequant(q, s)^T for (q, s) in weights]`` (<= 3 weights sharing x and the norm, e.g.
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
    check(require().lta_gemv_mxfp4_group(x.data_ptr(), _ptr(norm_weight), int(norm), float(eps), n,
                                         ctypes.cast(qs, c_void_p), ctypes.cast(ss, c_void_p),
                                         ctypes.cast(ys, c_void_p), ctypes.cast(nn, c_void_p),
                                         ctypes.cast(ldy, c_void_p), M, K, x.stride(0), stream_ptr(x.device)),
          "lta_gemv_mxfp4_group")
    return buf if packed else outs
