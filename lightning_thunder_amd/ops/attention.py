"""K3 flash attention wrappers (kernels in ``csrc/attention_fwd.hip`` / ``attention_bwd.hip``)."""
from __future__ import annotations

import ctypes
import math
import os

import torch

from ._lib import require, dcode, ptr, stream_ptr, check, register_signature, c_int, c_int64, c_void_p, c_float

register_signature("lta_attn_fwd", [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                                    c_int, c_int, c_float, c_int, c_void_p])
register_signature("lta_attn_bwd", [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                    c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int,
                                    c_float, c_int, c_void_p])
register_signature("lta_attn_fwd_s", [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
                                      c_int, c_int, c_int, c_float, c_int, c_void_p, c_void_p])
register_signature("lta_attn_bwd_s", [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                      c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int,
                                      c_float, c_int, c_void_p, c_void_p])

register_signature("lta_attn_fwd_ex", [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
                                       c_int, c_int, c_int, c_float, c_int, c_void_p, c_void_p, c_int, c_int, c_float,
                                       ctypes.c_uint64, ctypes.c_uint64, c_void_p])
register_signature("lta_attn_bwd_ex", [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                       c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_float,
                                       c_int, c_void_p, c_void_p, c_int, c_int, c_void_p, c_float, ctypes.c_uint64,
                                       ctypes.c_uint64, c_void_p])

register_signature("lta_attn_fwd_ex2", [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
                                        c_int, c_int, c_int, c_float, c_int, c_void_p, c_void_p, c_int, c_int, c_float,
                                        ctypes.c_uint64, ctypes.c_uint64, c_void_p, c_void_p])
register_signature("lta_attn_bwd_ex2", [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                        c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_float,
                                        c_int, c_void_p, c_void_p, c_int, c_int, c_void_p, c_float, ctypes.c_uint64,
                                        ctypes.c_uint64, c_void_p, c_void_p])
register_signature("lta_attn_bwd_rope", [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                         c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_float,
                                         c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                         ctypes.c_int64, c_int, c_void_p])
register_signature("lta_attn_bwd_rope_ds", [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                            c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int,
                                            c_int, c_float, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                            c_void_p, ctypes.c_int64, c_void_p, ctypes.c_int64, c_int, c_void_p])
register_signature("lta_attn_bwd_ex3", [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                        c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_float,
                                        c_int, c_void_p, c_void_p, c_int, c_int, c_void_p, c_float, ctypes.c_uint64,
                                        ctypes.c_uint64, c_void_p, c_void_p, c_void_p])

SUPPORTED_HEAD_DIMS = (64, 96, 128, 256)  # the kernels' compile-time head dims
# Other head dims up to 256 (multiples of 8) run zero-padded to the next kernel head dim, as the
# reference pads for aten flash (thunder/executors/sdpaex.py:45-59): zero columns of Q / K leave
# Q K^T unchanged, zero columns of V give zero columns of O (sliced off), the scale stays the
# caller's (1 / sqrt(D) of the real D), and the padded gradient columns are exactly zero.
# D = 256 (Gemma; cuDNN's limit, thunder/executors/cudnn_sdpa.py:339-363) runs 32-key tiles at one
# workgroup per CU with the accumulators in the AGPR file; additive / boolean masks and dropout are
# compiled into those kernels as for the smaller head dims (no spills: 248-256 VGPRs + AGPRs).
MAX_PADDED_HEAD_DIM = 256
PLAIN_ONLY_HEAD_DIM = 256  # above this head dim the kernels would take no additive mask / dropout


def padded_head_dim(D: int) -> int | None:
    if D in SUPPORTED_HEAD_DIMS:
        return D
    if D % 8 or D <= 0 or D > MAX_PADDED_HEAD_DIM:
        return None
    return next(d for d in SUPPORTED_HEAD_DIMS if d >= D)


def _pad_d(t: torch.Tensor, Dp: int) -> torch.Tensor:
    return t if t.shape[-1] == Dp else torch.nn.functional.pad(t, (0, Dp - t.shape[-1]))


def prepare_mask(mask: torch.Tensor, B: int, Hq: int, Tq: int, Sk: int):
    """Additive fp32 image of an SDPA mask for the kernels: ``[Bm, Hm, Tq, Skp]`` (Bm in {1, B},
    Hm in {1, Hq}, key dim padded to a multiple of 64 with -inf).  A boolean mask (True = attend)
    becomes 0 / -inf.  Returns (image, mask_b, mask_h)."""
    m = mask
    while m.dim() < 4:
        m = m.unsqueeze(0)
    mb = m.shape[0] == B and B > 1
    mh = m.shape[1] == Hq and Hq > 1
    m = m.expand(B if mb else 1, Hq if mh else 1, Tq, Sk)
    skp = (Sk + 63) // 64 * 64
    out = torch.full((m.shape[0], m.shape[1], Tq, skp), float("-inf"), device=m.device, dtype=torch.float32)
    if m.dtype == torch.bool:
        out[..., :Sk].masked_fill_(m, 0.0)
    else:
        out[..., :Sk].copy_(m)
    return out, int(mb), int(mh)


def supported(q, k, v) -> bool:
    return (
        q.dtype in (torch.bfloat16, torch.float16)
        and k.dtype == q.dtype
        and v.dtype == q.dtype
        and q.ndim == 4
        and padded_head_dim(q.shape[-1]) is not None
        and k.shape[-1] == q.shape[-1]
        and v.shape[-1] == q.shape[-1]
        and q.shape[1] % k.shape[1] == 0
        and k.shape[1] == v.shape[1]
    )


def _c(t):
    return t if t.is_contiguous() else t.contiguous()


def _strides3(t):
    return (ctypes.c_int64 * 3)(*t.stride()[:3])


def _qkv_in_place(q, k, v):
    """q / k / v as the kernels read them: any [B, H, T] strides with the head dim contiguous and
    16-byte aligned rows in place (e.g. views into a fused qkv projection), else a contiguous copy;
    plus their (batch, head, token) strides for the kernels."""
    q, k, v = (_rows_in_place(t) for t in (q, k, v))
    st = (ctypes.c_int64 * 9)(*q.stride()[:3], *k.stride()[:3], *v.stride()[:3])
    return q, k, v, st


def _grad_like(t):
    """An empty [B, H, T, D] gradient for ``t``: [B, T, H, D] memory (transposed view) when ``t`` is a
    head split of a token-major tensor (token stride > head stride), dense [B, H, T, D] otherwise."""
    B, H, T, D = t.shape
    if H > 1 and T > 1 and t.stride(2) > t.stride(1):
        return torch.empty((B, T, H, D), device=t.device, dtype=t.dtype).transpose(1, 2)
    return torch.empty((B, H, T, D), device=t.device, dtype=t.dtype)


def _rows_ok(t) -> bool:
    """Head dim contiguous, 16-byte aligned rows: any [B, H, T] strides are read in place."""
    return t.stride(-1) == 1 and all(s % 8 == 0 for s in t.stride()[:-1]) and t.data_ptr() % 16 == 0


def _rows_in_place(t):
    """``t`` itself when the kernels can read it in place, else a dense copy in fresh (aligned) memory:
    ``contiguous()`` alone hands a dense tensor at a misaligned address back as it is."""
    if _rows_ok(t):
        return t
    return t.clone(memory_format=torch.contiguous_format) if t.is_contiguous() else t.contiguous()


register_signature("lta_attn_set_rng_state", [c_void_p])
register_signature("lta_attn_set_fp8_out", [c_void_p, c_void_p, c_float, c_void_p, c_void_p])
register_signature("lta_attn_fp8_out_used", [])


def _graph_rng(lib, dropout_p, seed, offset):
    """Dropout seeds drawn inside a hipGraph capture (core/rng.py GraphRngInt): hand the kernel the
    region's device RNG state; the offset stays relative to its base."""
    from ..core.rng import GraphRngInt

    if dropout_p > 0 and (type(seed) is GraphRngInt or type(offset) is GraphRngInt):
        st = (seed if type(seed) is GraphRngInt else offset).state
        lib.lta_attn_set_rng_state(st.data_ptr())
        return 0, int(offset)
    return seed, offset


def attn_fwd(q, k, v, causal: bool, scale: float | None = None, out_layout: str = "bshd", mask=None,
             dropout_p: float = 0.0, seed: int = 0, offset: int = 0, fp8_out=None):
    """q [B, Hq, T, D], k/v [B, Hkv, S, D] -> (o [B, Hq, T, D], lse [B, Hq, T] fp32).

    ``out_layout="bshd"`` (default) stores O as [B, T, Hq, D] and returns its [B, Hq, T, D]
    transposed view: the usual ``o.transpose(1, 2).reshape(B, T, Hq * D)`` before the output
    projection is then a view instead of a copy, and the backward reads it (and dO) in place.

    ``fp8_out`` = (q8 uint8 [B, T, Hq, D], amax_in, fmax, scale_out, amax_out): ask the kernel for an
    e4m3 copy of O as well (the FP8 output projection's input, delayed scaling; csrc AttnQ8).  Returns
    (o, lse, written) then; ``written`` is False when the launched kernel has no such output (the caller
    casts separately)."""
    if fp8_out is not None:
        lib = require()
        if out_layout != "bshd" or q.shape[-1] != 128 or mask is not None or dropout_p:
            return attn_fwd(q, k, v, causal, scale, out_layout, mask, dropout_p, seed, offset) + (False,)
        q8, amax_in, fmax, scale_out, amax_out = fp8_out
        lib.lta_attn_set_fp8_out(q8.data_ptr(), amax_in.data_ptr(), float(fmax), scale_out.data_ptr(),
                                 amax_out.data_ptr())
        try:
            o, lse = attn_fwd(q, k, v, causal, scale, out_layout)
        finally:
            used = bool(lib.lta_attn_fp8_out_used())
            lib.lta_attn_set_fp8_out(None, None, 0.0, None, None)  # never left armed for another call
        return o, lse, used
    lib = require()
    D0 = q.shape[-1]
    Dp = padded_head_dim(D0)
    if Dp is not None and Dp != D0:
        sc = scale if scale is not None else 1.0 / math.sqrt(D0)
        o, lse = attn_fwd(_pad_d(q, Dp), _pad_d(k, Dp), _pad_d(v, Dp), causal, sc, out_layout, mask, dropout_p, seed,
                          offset)
        return o[..., :D0], lse
    q, k, v, qkv_st = _qkv_in_place(q, k, v)
    B, Hq, T, D = q.shape
    Hkv, S = k.shape[1], k.shape[2]
    sc = scale if scale is not None else 1.0 / math.sqrt(D)
    if out_layout == "bshd":
        o = torch.empty((B, T, Hq, D), device=q.device, dtype=q.dtype).transpose(1, 2)
    else:
        o = torch.empty((B, Hq, T, D), device=q.device, dtype=q.dtype)
    lse = torch.empty((B, Hq, T), device=q.device, dtype=torch.float32)
    mimg, mb, mh = (None, 0, 0) if mask is None else prepare_mask(mask, B, Hq, T, S)
    seed, offset = _graph_rng(lib, dropout_p, seed, offset)
    rc = lib.lta_attn_fwd_ex2(dcode(q), ptr(q), ptr(k), ptr(v), ptr(o), ptr(lse), B, Hq, Hkv, T, S, D, float(sc),
                              int(causal), ctypes.cast(_strides3(o), c_void_p), ptr(mimg), mb, mh, float(dropout_p),
                              int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1), ctypes.cast(qkv_st, c_void_p),
                              stream_ptr(q.device))
    check(rc, "lta_attn_fwd")
    return o, lse


def attn_bwd(do, q, k, v, o, lse, causal: bool, scale: float | None = None, mask=None, dropout_p: float = 0.0,
             seed: int = 0, offset: int = 0, mask_grad: bool = False):
    """Returns (dq, dk, dv) with dk/dv summed over the query heads of each kv group; with
    ``mask_grad`` (a float mask) a 4th result: the mask's gradient, reduced to its shape."""
    lib = require()
    D0 = q.shape[-1]
    Dp = padded_head_dim(D0)
    if Dp is not None and Dp != D0:
        sc = scale if scale is not None else 1.0 / math.sqrt(D0)
        res = attn_bwd(_pad_d(do, Dp), _pad_d(q, Dp), _pad_d(k, Dp), _pad_d(v, Dp), _pad_d(o, Dp), lse, causal, sc, mask,
                       dropout_p, seed, offset, mask_grad)
        return (res[0][..., :D0], res[1][..., :D0], res[2][..., :D0]) + tuple(res[3:])
    q, k, v, qkv_st = _qkv_in_place(q, k, v)
    do, o = _rows_in_place(do), _rows_in_place(o)
    B, Hq, T, D = q.shape
    Hkv, S = k.shape[1], k.shape[2]
    sc = scale if scale is not None else 1.0 / math.sqrt(D)
    # gradients take their operand's (head, token) order: heads split from a [B, T, H*D] projection
    # get [B, T, H, D] gradients, so the transpose + reshape back to [B, T, H*D] is a view
    dq, dk, dv = _grad_like(q), _grad_like(k), _grad_like(v)
    gst = (ctypes.c_int64 * 9)(*dq.stride()[:3], *dk.stride()[:3], *dv.stride()[:3])
    delta = torch.empty((B, Hq, T), device=q.device, dtype=torch.float32)
    st = (ctypes.c_int64 * 6)(*do.stride()[:3], *o.stride()[:3])
    mimg, mb, mh = (None, 0, 0) if mask is None else prepare_mask(mask, B, Hq, T, S)
    dmask = None
    if mask_grad:
        assert mask is not None and mask.dtype != torch.bool
        # causal: the dK/dV kernel skips the query tiles wholly above the diagonal and never stores their
        # (zero) dS, so those entries must not be left uninitialised
        dmask = (torch.zeros if causal else torch.empty)((B, Hq, T, S), device=q.device, dtype=torch.float32)
    seed, offset = _graph_rng(lib, dropout_p, seed, offset)
    part = None
    if Hq > Hkv and mask is None and dropout_p == 0:
        # GQA / MQA: the dK/dV pass splits each kv group's query heads over workgroups (D = 128 runs the
        # v4 kernel's 256-key blocks, other head dims the v1 kernel's 128-key blocks)
        part, nbytes, hs = _gqa_workspace(B, Hq, Hkv, S, q.device, D, 256 if D == 128 else 128)
        if part is not None:
            lib.lta_attn_set_gqa_workspace(part.data_ptr(), nbytes, hs)
    rc = lib.lta_attn_bwd_ex3(dcode(q), ptr(do), ptr(q), ptr(k), ptr(v), ptr(o), ptr(lse), ptr(delta), ptr(dq), ptr(dk),
                              ptr(dv), B, Hq, Hkv, T, S, D, float(sc), int(causal), ctypes.cast(st, c_void_p), ptr(mimg),
                              mb, mh, ptr(dmask), float(dropout_p), int(seed) & (2 ** 64 - 1),
                              int(offset) & (2 ** 64 - 1), ctypes.cast(qkv_st, c_void_p), ctypes.cast(gst, c_void_p),
                              stream_ptr(q.device))
    check(rc, "lta_attn_bwd")
    if not mask_grad:
        return dq, dk, dv
    # the mask broadcasts over some dims: its gradient is dS summed over them
    g = dmask
    shape = tuple(mask.shape)
    lead = g.dim() - len(shape)
    g = g.sum(tuple(range(lead))) if lead else g
    dims = tuple(i for i, n in enumerate(shape) if n == 1 and g.shape[i] != 1)
    if dims:
        g = g.sum(dims, keepdim=True)
    return dq, dk, dv, g.to(mask.dtype)


def _dq_from_ds(ws_bytes: int, device: torch.device | None = None) -> bool:
    """The RoPE'd backward computes dQ from the dS the dK/dV kernel stores (one B Hq T^2 bf16
    workspace, 1 GiB for a Llama-2-7B layer at T = 4096) instead of the dQ kernel's S / P / dP
    recompute: 59 us less per layer there (profiles/attn_dq_from_ds.txt).  On by default while the
    workspace fits LTA_ATTN_DS_MAX_GB (default 4) and at most half of what the device can still
    hand out (driver-free plus the caching allocator's unused reserve), so a run near the memory
    limit keeps the workspace-free recompute path; LTA_ATTN_DQ_FROM_DS=0 / 1 forces it off / on."""
    mode = os.environ.get("LTA_ATTN_DQ_FROM_DS", "auto")
    if mode in ("0", "1"):
        return mode == "1"
    if ws_bytes > float(os.environ.get("LTA_ATTN_DS_MAX_GB", "4")) * 2 ** 30:
        return False
    if device is None or device.type != "cuda":
        return True
    free, _ = torch.cuda.mem_get_info(device)
    spare = torch.cuda.memory_reserved(device) - torch.cuda.memory_allocated(device)
    return 2 * ws_bytes <= free + spare


def gqa_split(B: int, Hq: int, Hkv: int, S: int, keys_per_wg: int = 256) -> int:
    """How many workgroups share one kv group's query heads in the dK/dV pass.  The pass runs one
    workgroup per (batch, kv head, 256 keys): for GQA models (Mistral / Llama-3: 8 kv heads) that is
    128 workgroups at T = 4096, half of the 256 CUs, each sweeping 4 query heads.  Splitting the heads
    over workgroups (fp32 partial dK / dV rows, summed by one reduce launch) targets >= 2 waves of
    workgroups; LTA_ATTN_GQA_SPLIT caps it (1 = off)."""
    group = Hq // Hkv
    if group <= 1:
        return 1
    cap = int(os.environ.get("LTA_ATTN_GQA_SPLIT", "8"))
    n_wg = B * Hkv * ((S + keys_per_wg - 1) // keys_per_wg)
    best = 1
    for d in range(2, group + 1):
        if group % d or d > cap:
            continue
        best = d
        if n_wg * d >= 512:
            break
    return best if n_wg < 512 else 1


def _gqa_workspace(B, Hq, Hkv, S, device, D: int = 128, keys_per_wg: int = 256):
    hs = gqa_split(B, Hq, Hkv, S, keys_per_wg)
    if hs <= 1:
        return None, 0, 1
    ws = torch.empty(hs * B * Hkv * S * 2 * D, device=device, dtype=torch.float32)
    return ws, ws.numel() * 4, hs


register_signature("lta_attn_set_gqa_workspace", [c_void_p, c_int64, c_int])


def attn_bwd_rope(do, q, k, v, o, lse, causal: bool, scale, cos, sin, n_head: int, n_query_groups: int):
    """The attention backward and the backward of the rotate-half RoPE + qkv split in one pass:
    returns d(qkv) [B, T, (n_head + 2 n_query_groups) * 128], with dQ / dK rotated back in the
    dK/dV and dQ kernels' epilogues and stored (like dV) straight into their columns of the fused
    projection's gradient (no dq / dk / dv tensors, no separate RoPE-backward pass).  Falls back to
    ``attn_bwd`` + ``ops.fused.qkv_rope_bwd`` when the kernels do not cover the case."""
    lib = require()
    B, Hq, T, D = q.shape
    Hkv, S = k.shape[1], k.shape[2]
    sc = scale if scale is not None else 1.0 / math.sqrt(D)
    if D == 128 and S == T and Hq == n_head and Hkv == n_query_groups:
        qq, kk, vv, qkv_st = _qkv_in_place(q, k, v)
        dd, oo = _rows_in_place(do), _rows_in_place(o)
        cs = cos[:T].float().contiguous()
        sn = sin[:T].float().contiguous()
        W = (Hq + 2 * Hkv) * D
        dqkv = torch.empty((B, T, W), device=q.device, dtype=q.dtype)
        gst = (ctypes.c_int64 * 9)(T * W, D, W, T * W, D, W, T * W, D, W)
        delta = torch.empty((B, Hq, T), device=q.device, dtype=torch.float32)
        st = (ctypes.c_int64 * 6)(*dd.stride()[:3], *oo.stride()[:3])
        esz = dqkv.element_size()
        rc = -1
        n_ws = B * Hq * S * ((T + 255) // 256 * 256)
        part, part_bytes, hsplit = _gqa_workspace(B, Hq, Hkv, S, q.device)
        # the kernel's own shape rules (T == S checked above, T % 64) before the workspace is allocated
        if T > 0 and T % 64 == 0 and Hq % Hkv == 0 and _dq_from_ds(n_ws * esz, q.device):
            ws = torch.empty(n_ws, device=q.device, dtype=q.dtype)
            rc = lib.lta_attn_bwd_rope_ds(dcode(qq), ptr(dd), ptr(qq), ptr(kk), ptr(vv), ptr(oo), ptr(lse), ptr(delta),
                                          ptr(dqkv), ptr(dqkv) + Hq * D * esz, ptr(dqkv) + (Hq + Hkv) * D * esz, B, Hq,
                                          Hkv, T, S, D, float(sc), int(causal), ctypes.cast(st, c_void_p),
                                          ctypes.cast(qkv_st, c_void_p), ctypes.cast(gst, c_void_p), ptr(cs), ptr(sn),
                                          ptr(ws), ws.numel() * ws.element_size(), ptr(part), part_bytes, hsplit,
                                          stream_ptr(q.device))
            if rc != -1:
                check(rc, "lta_attn_bwd_rope_ds")
                return dqkv
        rc = lib.lta_attn_bwd_rope(dcode(qq), ptr(dd), ptr(qq), ptr(kk), ptr(vv), ptr(oo), ptr(lse), ptr(delta),
                                   ptr(dqkv), ptr(dqkv) + Hq * D * esz, ptr(dqkv) + (Hq + Hkv) * D * esz, B, Hq, Hkv, T,
                                   S, D, float(sc), int(causal), ctypes.cast(st, c_void_p), ctypes.cast(qkv_st, c_void_p),
                                   ctypes.cast(gst, c_void_p), ptr(cs), ptr(sn), ptr(part), part_bytes, hsplit,
                                   stream_ptr(q.device))
        if rc != -1:
            check(rc, "lta_attn_bwd_rope")
            return dqkv
    from .fused import qkv_rope_bwd

    dq, dk, dv = attn_bwd(do, q, k, v, o, lse, causal, sc)
    return qkv_rope_bwd(dq, dk, dv, cos, sin, n_head, n_query_groups, D, D)


# ------------------------------------------------------------------------------------------------
# K3d decode attention (csrc/decode_attention.hip): T <= 16 query rows against a long KV cache
# ------------------------------------------------------------------------------------------------
import ctypes  # noqa: E402

from ._lib import c_int64  # noqa: E402
from .kv8 import scale_caches_of  # noqa: E402

# the decode entries: pointers q, k, v, <scale caches>, mask (or pos), o, ws_acc, ws_ml, then the sizes and strides; the
# mask entries go on with chunk, nsplit, causal, the position entries with nsplit alone
for _entry, _scale_ptrs in (("lta_decode_attn", 0), ("lta_decode_attn_kv8", 0), ("lta_decode_attn_kv8s", 2)):
    _head = [c_int, *[c_void_p] * (7 + _scale_ptrs), *[c_int] * 6, c_void_p]
    register_signature(_entry, [*_head, c_int, c_int, c_int, c_float, c_int, c_void_p])
    register_signature(_entry + "_pos", [*_head, c_int, c_float, c_int, c_void_p])
    # the paged entries: the position entries', then the block table, log2 of the page size and the page count
    register_signature(_entry + "_paged", [*_head, c_int, c_float, c_int, c_void_p, c_int, c_int, c_void_p])
    # the window entries: the position / paged entries', then the window
    register_signature(_entry + "_pos_win", [*_head, c_int, c_float, c_int, c_void_p, c_int])
    register_signature(_entry + "_paged_win", [*_head, c_int, c_float, c_int, c_void_p, c_int, c_int, c_void_p, c_int])

DECODE_MAX_QUERIES = 16


def decode_launch_shape(rows: int, S: int):
    """(wsplit, nsplit, chunk) of a decode launch over ``rows`` query rows and ``S`` keys: the same
    for every cache element type."""
    # few rows (batch-1 decode): one row per workgroup with its 4 waves splitting the keys
    wsplit = rows < 256
    blocks = rows if wsplit else (rows + 3) // 4
    # split the cache so that a decode step still launches >= ~256 workgroups (flash-decoding)
    nsplit = max(1, min((256 + blocks - 1) // blocks, S // 256))  # a split is worth a combine launch from ~256 keys
    chunk = ((S + nsplit - 1) // nsplit + 63) // 64 * 64
    nsplit = (S + chunk - 1) // chunk
    return wsplit, nsplit, chunk


def _window_arg(fn: str, window) -> tuple:
    """The trailing argument of a ``*_win`` entry: ``()`` without a window, else ``(window,)`` for an int >= 1
    (``ValueError`` for anything else)."""
    if window is None:
        return ()
    if isinstance(window, bool) or not isinstance(window, int) or window < 1:
        raise ValueError(f"{fn}: window must be an int >= 1 or None, got {window!r}")
    return (min(window, 2 ** 31 - 1),)


def _decode_launch(entry: str, q, k, v, scale: float | None, mask=None, causal: bool = False, pos=None, scales=(),
                   pages=None, window: int | None = None):
    """One launch of ``entry``: a mask entry with (``mask``, ``causal``), a position entry with ``pos``.  ``scales`` =
    (k_scale, v_scale) for the scaled-e4m3 entries, whose argument list carries the two pointers after v.  The
    stride record is q, k, v (b, h, t each), then the selector's (mask b, h, t, s or pos b, t), then the scales'.

    ``pages`` = (table, page_size, num_pages) for the paged entries (``ops/kv_pages.py``): k / v (and the scales) are
    pools ``[Hkv, R + 1, D]`` whose batch stride goes on as 0, ``S`` is the table's logical capacity, the table's two
    strides end the stride record, and the table, log2(page_size) and num_pages follow ``wsplit``.

    The grid comes from the capacity S in both modes (``decode_launch_shape``): positions stay on the device, so a
    hipGraph replays the launch while they advance; the kernel splits each row's live range over the ``nsplit``
    workgroups itself.

    ``window`` (position and paged entries only) launches ``entry + "_win"`` with the window after the stream: row
    (b, hq, t) attends its last ``window`` live positions only.  Without it the launch is ``entry``'s, argument for
    argument."""
    win = _window_arg(entry, window)
    if win:
        entry += "_win"
    lib = require()
    B, Hq, T, D = q.shape
    if pages is not None:
        table, page_size, num_pages = pages
        Hkv, S = k.shape[0], table.shape[1] * page_size
        cache_st = lambda c: (0, *c.stride()[:2])
        tail = (*table.stride(), ptr(table), page_size.bit_length() - 1, num_pages)
    else:
        Hkv, S = k.shape[1], k.shape[2]
        cache_st = lambda c: c.stride()[:3]
        tail = ()
    sc = scale if scale is not None else 1.0 / math.sqrt(D)
    rows = B * Hq * T
    wsplit, nsplit, chunk = decode_launch_shape(rows, S)
    o = torch.empty((B, Hq, T, D), device=q.device, dtype=q.dtype)
    ws_acc = ws_ml = None
    if nsplit > 1:
        ws_acc = torch.empty((nsplit, rows, D), device=q.device, dtype=torch.float32)
        ws_ml = torch.empty((nsplit, rows, 2), device=q.device, dtype=torch.float32)
    if pos is not None:
        sel, sel_st, split = pos, pos.stride(), (nsplit,)
    else:
        sel = mask if mask is None else torch.broadcast_to(mask, (B, Hq, T, S))
        sel_st, split = (0, 0, 0, 0) if mask is None else sel.stride(), (chunk, nsplit, int(causal))
    st = (*q.stride()[:3], *cache_st(k), *cache_st(v), *sel_st, *(s for c in scales for s in cache_st(c)), *tail[:2])
    st = (ctypes.c_int64 * len(st))(*st)
    rc = getattr(lib, entry)(dcode(q), ptr(q), ptr(k), ptr(v), *map(ptr, scales), ptr(sel), ptr(o), ptr(ws_acc),
                             ptr(ws_ml), B, Hq, Hkv, T, S, D, ctypes.cast(st, ctypes.c_void_p), *split, float(sc),
                             int(wsplit), *tail[2:], stream_ptr(q.device), *win)
    check(rc, entry)
    return o


def _refusal(fn: str, **operands) -> ValueError:
    """The error of a wrapper whose ``*_supported`` said no: ``fn`` and every operand's dtype and shape."""
    return ValueError(f"{fn}: unsupported operands " + ", ".join(
        f"{name} {None if t is None else (t.dtype, tuple(t.shape))}" for name, t in operands.items()))


def _cache_operands_ok(q, k, v, cache_dtype, max_queries: int | None = DECODE_MAX_QUERIES) -> bool:
    """The shape rule of every kernel that checks its operands: 16-bit q [B, Hq, T, D] with D 64 / 128 and at most
    ``max_queries`` rows (the decode kernels' DECODE_MAX_QUERIES; None for the prefill kernel: any number), k / v
    [B, Hkv, S, D] of ``cache_dtype`` with Hkv dividing Hq."""
    return (q.dtype in (torch.bfloat16, torch.float16) and q.dim() == 4 and q.shape[-1] in (64, 128)
            and (max_queries is None or q.shape[2] <= max_queries) and k.dtype == cache_dtype and v.dtype == cache_dtype
            and k.dim() == 4 and k.shape == v.shape and k.shape[-1] == q.shape[-1] and k.shape[0] == q.shape[0]
            and k.shape[1] > 0 and q.shape[1] % k.shape[1] == 0)


def _e4m3_in_place(q, k8, v8):
    return _rows_in_place(q), _rows8_in_place(k8), _rows8_in_place(v8)


def decode_attn(q, k, v, mask=None, causal: bool = False, scale: float | None = None):
    """q [B, Hq, T, D] (T <= 16), k/v [B, Hkv, S, D], mask bool broadcastable to [B, Hq, T, S] -> [B, Hq, T, D]."""
    q, k, v = _rows_in_place(q), _rows_in_place(k), _rows_in_place(v)
    return _decode_launch("lta_decode_attn", q, k, v, scale, mask, causal)


def decode_attn_kv8_supported(q, k8, v8) -> bool:
    """What the e4m3-cache decode kernel takes: 16-bit q of head dim 64 / 128, uint8 k / v."""
    return _cache_operands_ok(q, k8, v8, torch.uint8)


def _rows8_in_place(t):
    """A uint8 cache as the kernel reads it (head dim contiguous, 16-byte aligned rows, strides a
    multiple of 16 bytes) in place, else a dense copy in fresh memory."""
    if t.stride(-1) == 1 and all(s % 16 == 0 for s in t.stride()[:-1]) and t.data_ptr() % 16 == 0:
        return t
    return t.clone(memory_format=torch.contiguous_format) if t.is_contiguous() else t.contiguous()


def decode_attn_kv8(q, k8, v8, mask=None, causal: bool = False, scale: float | None = None):
    """``decode_attn`` over an unscaled OCP e4m3 cache: k8 / v8 uint8 [B, Hkv, S, D] (the bytes of
    ``float8_e4m3fn``), unpacked in the kernel; q and the result are bf16 / fp16."""
    if not decode_attn_kv8_supported(q, k8, v8):
        raise _refusal("decode_attn_kv8", q=q, k=k8, v=v8)
    return _decode_launch("lta_decode_attn_kv8", *_e4m3_in_place(q, k8, v8), scale, mask, causal)


def decode_attn_kv8s_supported(q, k8, v8, k_scale, v_scale) -> bool:
    """What the scaled-e4m3 decode kernel takes: the operands of ``decode_attn_kv8`` plus uint8 scale
    caches [B, Hkv, S, 1] on the same device (any strides: a lane loads single bytes)."""
    return decode_attn_kv8_supported(q, k8, v8) and scale_caches_of((k_scale, v_scale), (k8, v8))


def decode_attn_kv8s(q, k8, v8, k_scale, v_scale, mask=None, causal: bool = False, scale: float | None = None):
    """``decode_attn`` over the scaled e4m3 cache of ``ops/kv8.py``: k8 / v8 uint8 [B, Hkv, S, D], k_scale /
    v_scale uint8 [B, Hkv, S, 1] (``e + 127`` per row).  Equals ``decode_attn`` over
    ``dequantise_rows(k8, k_scale, q.dtype)`` / ``dequantise_rows(v8, v_scale, q.dtype)`` bit for bit (fp32
    subnormal or overflowing partial sums aside); the scales are read in place."""
    if not decode_attn_kv8s_supported(q, k8, v8, k_scale, v_scale):
        raise _refusal("decode_attn_kv8s", q=q, k=k8, v=v8, k_scale=k_scale, v_scale=v_scale)
    return _decode_launch("lta_decode_attn_kv8s", *_e4m3_in_place(q, k8, v8), scale, mask, causal,
                          scales=(k_scale, v_scale))


# ------------------------------------------------------------------------------------------------
# Position mode of the decode kernels (ragged batches): every row's key count from pos[b, t], no mask
# ------------------------------------------------------------------------------------------------
def _pos_ok(q, k, pos, max_queries: int | None = DECODE_MAX_QUERIES) -> bool:
    """int64 positions [B, T] (any strides) on q's device, at most ``max_queries`` query rows (None: any number)."""
    return (pos is not None and pos.dtype == torch.int64 and pos.dim() == 2 and q.dim() == 4 and k.dim() == 4
            and tuple(pos.shape) == (q.shape[0], q.shape[2]) and pos.device == q.device
            and 0 < q.shape[2] and (max_queries is None or q.shape[2] <= max_queries))


def decode_attn_pos_supported(q, k, v, pos) -> bool:
    """What the 16-bit position kernel takes: bf16 / fp16 q, k, v of one dtype and head dim 64 / 128, GQA
    head counts, int64 ``pos`` [B, T] with T <= 16."""
    return _pos_ok(q, k, pos) and _cache_operands_ok(q, k, v, q.dtype)


def decode_attn_kv8_pos_supported(q, k8, v8, pos) -> bool:
    return _pos_ok(q, k8, pos) and decode_attn_kv8_supported(q, k8, v8)


def decode_attn_kv8s_pos_supported(q, k8, v8, k_scale, v_scale, pos) -> bool:
    return _pos_ok(q, k8, pos) and decode_attn_kv8s_supported(q, k8, v8, k_scale, v_scale)


def decode_attn_pos(q, k, v, pos, scale: float | None = None, window: int | None = None):
    """Decode attention of a ragged batch: q [B, Hq, T, D] (T <= 16), k / v [B, Hkv, S, D], ``pos`` int64
    [B, T].  Row (b, hq, t) attends keys ``0 .. n-1`` with ``n = clamp(pos[b, t] + 1, 0, S)``: what
    ``decode_attn`` computes under the mask ``arange(S) <= pos[b, t]``, without the mask tensor and with the
    row's live keys split over all of its workgroups.  ``n = 0`` gives a NaN row, like a fully masked one.

    ``window`` (an int >= 1; here and on the other position / paged wrappers) is a sliding window: the row attends keys
    ``max(0, n - window) .. n-1``, that is ``window`` keys with its own (the Mistral / HF convention; LitGPT's own mask
    keeps ``window + 1``), what ``decode_attn`` computes under ``window_mask(pos, S, window)``; only those keys are
    read, and on a paged cache only their table entries.  Where ``window >= n`` for every row the result is the
    call's without a window, bit for bit.  ``None`` launches the entry without a window."""
    if not decode_attn_pos_supported(q, k, v, pos):
        raise _refusal("decode_attn_pos", q=q, k=k, v=v, pos=pos)
    q, k, v = _rows_in_place(q), _rows_in_place(k), _rows_in_place(v)
    return _decode_launch("lta_decode_attn_pos", q, k, v, scale, pos=pos, window=window)


def decode_attn_kv8_pos(q, k8, v8, pos, scale: float | None = None, window: int | None = None):
    """``decode_attn_pos`` over an unscaled e4m3 cache (the operands of ``decode_attn_kv8``)."""
    if not decode_attn_kv8_pos_supported(q, k8, v8, pos):
        raise _refusal("decode_attn_kv8_pos", q=q, k=k8, v=v8, pos=pos)
    return _decode_launch("lta_decode_attn_kv8_pos", *_e4m3_in_place(q, k8, v8), scale, pos=pos, window=window)


def decode_attn_kv8s_pos(q, k8, v8, k_scale, v_scale, pos, scale: float | None = None, window: int | None = None):
    """``decode_attn_pos`` over the scaled e4m3 cache (the operands of ``decode_attn_kv8s``): equals
    ``decode_attn_pos`` over the dequantised cache bit for bit, with that kernel's exclusions."""
    if not decode_attn_kv8s_pos_supported(q, k8, v8, k_scale, v_scale, pos):
        raise _refusal("decode_attn_kv8s_pos", q=q, k=k8, v=v8, k_scale=k_scale, v_scale=v_scale, pos=pos)
    return _decode_launch("lta_decode_attn_kv8s_pos", *_e4m3_in_place(q, k8, v8), scale, pos=pos,
                          scales=(k_scale, v_scale), window=window)


# ------------------------------------------------------------------------------------------------
# Paged mode of the decode kernels (ops/kv_pages.py): the position mode with every key's row taken from a block table
# ------------------------------------------------------------------------------------------------
def _paged_ok(q, k, v, pos, table, page_size, num_pages, cache_dtype, scales=(),
              max_queries: int | None = DECODE_MAX_QUERIES) -> bool:
    """16-bit q [B, Hq, T, D] with D 64 / 128 and at most ``max_queries`` rows (None: any number); pools k / v
    [Hkv, rows, D] of ``cache_dtype`` read in place (head dim contiguous, 16-byte aligned rows and heads) with Hkv dividing Hq and
    ``rows >= num_pages * page_size``; scale pools uint8 [Hkv, rows, 1]; int64 ``pos`` [B, T] and ``table``
    [B, max_pages >= 1] on q's device; ``page_size`` a power of two >= 16 and ``num_pages`` >= 1, both ints."""
    if not all(isinstance(n, int) and not isinstance(n, bool) for n in (page_size, num_pages)):
        return False
    if page_size < 16 or page_size & (page_size - 1) or num_pages < 1 or num_pages * page_size >= 2 ** 31:
        return False
    if not (q.dtype in (torch.bfloat16, torch.float16) and q.dim() == 4 and q.shape[-1] in (64, 128)
            and 0 < q.shape[2] and (max_queries is None or q.shape[2] <= max_queries)):
        return False
    unit = 16 // k.element_size()  # elements per 16 bytes
    for c in (k, v):
        if c.dtype != cache_dtype or c.dim() != 3 or c.shape != k.shape or c.device != q.device:
            return False
        if c.stride(2) != 1 or c.stride(0) % unit or c.stride(1) % unit or c.data_ptr() % 16:
            return False
    Hkv, rows, D = k.shape
    if D != q.shape[-1] or Hkv < 1 or q.shape[1] % Hkv or rows < num_pages * page_size:
        return False
    if any(s is None or s.dtype != torch.uint8 or s.device != q.device or tuple(s.shape) != (Hkv, rows, 1)
           for s in scales):
        return False
    return all(t is not None and t.dtype == torch.int64 and t.dim() == 2 and t.device == q.device
               and t.shape[0] == q.shape[0] for t in (pos, table)) and pos.shape[1] == q.shape[2] \
        and table.shape[1] >= 1 and table.shape[1] * page_size < 2 ** 31


def decode_attn_paged_supported(q, k, v, pos, table, page_size, num_pages) -> bool:
    """What the 16-bit paged kernel takes: see ``_paged_ok``, with pools of q's dtype."""
    return _paged_ok(q, k, v, pos, table, page_size, num_pages, q.dtype)


def decode_attn_kv8_paged_supported(q, k8, v8, pos, table, page_size, num_pages) -> bool:
    return _paged_ok(q, k8, v8, pos, table, page_size, num_pages, torch.uint8)


def decode_attn_kv8s_paged_supported(q, k8, v8, k_scale, v_scale, pos, table, page_size, num_pages) -> bool:
    return _paged_ok(q, k8, v8, pos, table, page_size, num_pages, torch.uint8, (k_scale, v_scale))


def decode_attn_paged(q, k, v, pos, table, page_size: int, num_pages: int, scale: float | None = None,
                      window: int | None = None):
    """``decode_attn_pos`` over a paged cache: k / v pools ``[Hkv, R + 1, D]``, ``table`` int64 ``[B, max_pages]``.
    Row (b, hq, t) attends the keys ``j <= pos[b, t]`` (clamped to the capacity ``S = max_pages * page_size``) whose
    table entry lies in ``[0, num_pages)``, each read at pool row ``table[b, j // page_size] * page_size + j %
    page_size``: what ``decode_attn`` computes over ``gather_pages`` under ``paged_mask``.  No key gives a NaN row."""
    if not decode_attn_paged_supported(q, k, v, pos, table, page_size, num_pages):
        raise _refusal("decode_attn_paged", q=q, k=k, v=v, pos=pos, table=table)
    return _decode_launch("lta_decode_attn_paged", _rows_in_place(q), k, v, scale, pos=pos,
                          pages=(table, page_size, num_pages), window=window)


def decode_attn_kv8_paged(q, k8, v8, pos, table, page_size: int, num_pages: int, scale: float | None = None,
                          window: int | None = None):
    """``decode_attn_paged`` over unscaled e4m3 pools (uint8)."""
    if not decode_attn_kv8_paged_supported(q, k8, v8, pos, table, page_size, num_pages):
        raise _refusal("decode_attn_kv8_paged", q=q, k=k8, v=v8, pos=pos, table=table)
    return _decode_launch("lta_decode_attn_kv8_paged", _rows_in_place(q), k8, v8, scale, pos=pos,
                          pages=(table, page_size, num_pages), window=window)


def decode_attn_kv8s_paged(q, k8, v8, k_scale, v_scale, pos, table, page_size: int, num_pages: int,
                           scale: float | None = None, window: int | None = None):
    """``decode_attn_paged`` over the scaled e4m3 pools: bytes ``[Hkv, R + 1, D]`` and scale bytes ``[Hkv, R + 1, 1]``."""
    if not decode_attn_kv8s_paged_supported(q, k8, v8, k_scale, v_scale, pos, table, page_size, num_pages):
        raise _refusal("decode_attn_kv8s_paged", q=q, k=k8, v=v8, k_scale=k_scale, v_scale=v_scale, pos=pos,
                       table=table)
    return _decode_launch("lta_decode_attn_kv8s_paged", _rows_in_place(q), k8, v8, scale, pos=pos,
                          scales=(k_scale, v_scale), pages=(table, page_size, num_pages), window=window)


# ------------------------------------------------------------------------------------------------
# K3p prefill attention by positions (csrc/prefill_attention.hip): the flash forward for any number of query rows
# that sit at positions of a KV cache; the position and paged modes of the decode kernels above, past 16 rows
# ------------------------------------------------------------------------------------------------
# the prefill entries: pointers q, k, v, <scale caches>, pos, o, then the sizes, the stride record, O's strides and the
# softmax scale; the paged entries go on with the block table, log2 of the page size and the page count
for _entry, _scale_ptrs in (("lta_prefill_attn", 0), ("lta_prefill_attn_kv8", 0), ("lta_prefill_attn_kv8s", 2)):
    _head = [c_int, *[c_void_p] * (5 + _scale_ptrs), *[c_int] * 6, c_void_p, c_void_p, c_float]
    register_signature(_entry + "_pos", [*_head, c_void_p])
    register_signature(_entry + "_paged", [*_head, c_void_p, c_int, c_int, c_void_p])
    register_signature(_entry + "_pos_win", [*_head, c_void_p, c_int])
    register_signature(_entry + "_paged_win", [*_head, c_void_p, c_int, c_int, c_void_p, c_int])


def _prefill_launch(entry: str, q, k, v, pos, scale: float | None, scales=(), pages=None, window: int | None = None):
    """One launch of the prefill entry ``entry`` (operands as ``_decode_launch`` takes them in its position mode).  O
    is stored ``[B, T, Hq, D]`` and returned as its ``[B, Hq, T, D]`` view, as ``attn_fwd`` does.  The grid comes from
    the shapes alone: positions and table stay on the device, so the launch is capturable.  ``window`` launches
    ``entry + "_win"`` with the window after the stream, as ``_decode_launch`` does."""
    win = _window_arg(entry, window)
    if win:
        entry += "_win"
    lib = require()
    B, Hq, T, D = q.shape
    if pages is not None:
        table, page_size, num_pages = pages
        Hkv, S = k.shape[0], table.shape[1] * page_size
        cache_st = lambda c: (0, *c.stride()[:2])
        tail = (*table.stride(), ptr(table), page_size.bit_length() - 1, num_pages)
    else:
        Hkv, S = k.shape[1], k.shape[2]
        cache_st = lambda c: c.stride()[:3]
        tail = ()
    sc = scale if scale is not None else 1.0 / math.sqrt(D)
    o = torch.empty((B, T, Hq, D), device=q.device, dtype=q.dtype).transpose(1, 2)
    st = (*q.stride()[:3], *cache_st(k), *cache_st(v), *pos.stride(), *(s for c in scales for s in cache_st(c)), *tail[:2])
    st = (ctypes.c_int64 * len(st))(*st)
    rc = getattr(lib, entry)(dcode(q), ptr(q), ptr(k), ptr(v), *map(ptr, scales), ptr(pos), ptr(o), B, Hq, Hkv, T, S, D,
                             ctypes.cast(st, c_void_p), ctypes.cast(_strides3(o), c_void_p), float(sc), *tail[2:],
                             stream_ptr(q.device), *win)
    check(rc, entry)
    return o


def prefill_attn_pos_supported(q, k, v, pos) -> bool:
    """What the 16-bit prefill kernel takes: bf16 / fp16 q, k, v of one dtype and head dim 64 / 128, GQA head counts,
    int64 ``pos`` [B, T] with any T >= 1, a cache of at least one key."""
    return _pos_ok(q, k, pos, None) and _cache_operands_ok(q, k, v, q.dtype, None) and k.shape[2] > 0


def prefill_attn_kv8_pos_supported(q, k8, v8, pos) -> bool:
    return _pos_ok(q, k8, pos, None) and _cache_operands_ok(q, k8, v8, torch.uint8, None) and k8.shape[2] > 0


def prefill_attn_kv8s_pos_supported(q, k8, v8, k_scale, v_scale, pos) -> bool:
    return prefill_attn_kv8_pos_supported(q, k8, v8, pos) and scale_caches_of((k_scale, v_scale), (k8, v8))


def prefill_attn_pos(q, k, v, pos, scale: float | None = None, window: int | None = None):
    """Attention of query rows at positions of a KV cache: q [B, Hq, T, D] (any T >= 1), k / v [B, Hkv, S, D], ``pos``
    int64 [B, T] (need not be monotone).  Row (b, hq, t) attends keys ``0 .. n-1`` with ``n = clamp(pos[b, t] + 1, 0,
    S)``: what ``attn_fwd(q, k, v, causal=False, mask=position_mask(pos, S))[0]`` computes, bit for bit, without the
    mask image and over the key tiles some row can see only.  ``n = 0`` gives a row of zeros, as there.

    ``window`` as ``decode_attn_pos`` takes it: the row attends keys ``max(0, n - window) .. n-1``, what ``attn_fwd``
    computes under ``window_mask(pos, S, window)`` bit for bit, over the key tiles between the workgroup's lowest window
    and its highest position only."""
    if not prefill_attn_pos_supported(q, k, v, pos):
        raise _refusal("prefill_attn_pos", q=q, k=k, v=v, pos=pos)
    q, k, v = _rows_in_place(q), _rows_in_place(k), _rows_in_place(v)
    return _prefill_launch("lta_prefill_attn_pos", q, k, v, pos, scale, window=window)


def prefill_attn_kv8_pos(q, k8, v8, pos, scale: float | None = None, window: int | None = None):
    """``prefill_attn_pos`` over an unscaled e4m3 cache (uint8 bytes of ``float8_e4m3fn``): equals it over
    ``e4m3_values(k8, q.dtype)`` / ``e4m3_values(v8, q.dtype)`` bit for bit."""
    if not prefill_attn_kv8_pos_supported(q, k8, v8, pos):
        raise _refusal("prefill_attn_kv8_pos", q=q, k=k8, v=v8, pos=pos)
    return _prefill_launch("lta_prefill_attn_kv8_pos", *_e4m3_in_place(q, k8, v8), pos, scale, window=window)


def prefill_attn_kv8s_pos(q, k8, v8, k_scale, v_scale, pos, scale: float | None = None, window: int | None = None):
    """``prefill_attn_pos`` over the scaled e4m3 cache of ``ops/kv8.py``: equals it over ``dequantise_rows`` of the
    caches bit for bit; the scales are read in place."""
    if not prefill_attn_kv8s_pos_supported(q, k8, v8, k_scale, v_scale, pos):
        raise _refusal("prefill_attn_kv8s_pos", q=q, k=k8, v=v8, k_scale=k_scale, v_scale=v_scale, pos=pos)
    return _prefill_launch("lta_prefill_attn_kv8s_pos", *_e4m3_in_place(q, k8, v8), pos, scale,
                           scales=(k_scale, v_scale), window=window)


def prefill_attn_paged_supported(q, k, v, pos, table, page_size, num_pages) -> bool:
    """What the 16-bit paged prefill kernel takes: see ``_paged_ok``, with pools of q's dtype and any T >= 1."""
    return _paged_ok(q, k, v, pos, table, page_size, num_pages, q.dtype, max_queries=None)


def prefill_attn_kv8_paged_supported(q, k8, v8, pos, table, page_size, num_pages) -> bool:
    return _paged_ok(q, k8, v8, pos, table, page_size, num_pages, torch.uint8, max_queries=None)


def prefill_attn_kv8s_paged_supported(q, k8, v8, k_scale, v_scale, pos, table, page_size, num_pages) -> bool:
    return _paged_ok(q, k8, v8, pos, table, page_size, num_pages, torch.uint8, (k_scale, v_scale), max_queries=None)


def prefill_attn_paged(q, k, v, pos, table, page_size: int, num_pages: int, scale: float | None = None,
                       window: int | None = None):
    """``prefill_attn_pos`` over a paged cache: k / v pools ``[Hkv, R + 1, D]``, ``table`` int64 ``[B, max_pages]``.
    Row (b, hq, t) attends the keys ``j <= pos[b, t]`` (clamped to the capacity ``S = max_pages * page_size``) whose
    table entry lies in ``[0, num_pages)``, each read at pool row ``table[b, j // page_size] * page_size + j %
    page_size``: what ``attn_fwd`` computes over ``gather_pages`` under ``paged_mask``, bit for bit.  A row without a
    live key is zeros."""
    if not prefill_attn_paged_supported(q, k, v, pos, table, page_size, num_pages):
        raise _refusal("prefill_attn_paged", q=q, k=k, v=v, pos=pos, table=table)
    return _prefill_launch("lta_prefill_attn_paged", _rows_in_place(q), k, v, pos, scale,
                           pages=(table, page_size, num_pages), window=window)


def prefill_attn_kv8_paged(q, k8, v8, pos, table, page_size: int, num_pages: int, scale: float | None = None,
                           window: int | None = None):
    """``prefill_attn_paged`` over unscaled e4m3 pools (uint8)."""
    if not prefill_attn_kv8_paged_supported(q, k8, v8, pos, table, page_size, num_pages):
        raise _refusal("prefill_attn_kv8_paged", q=q, k=k8, v=v8, pos=pos, table=table)
    return _prefill_launch("lta_prefill_attn_kv8_paged", _rows_in_place(q), k8, v8, pos, scale,
                           pages=(table, page_size, num_pages), window=window)


def prefill_attn_kv8s_paged(q, k8, v8, k_scale, v_scale, pos, table, page_size: int, num_pages: int,
                            scale: float | None = None, window: int | None = None):
    """``prefill_attn_paged`` over the scaled e4m3 pools: bytes ``[Hkv, R + 1, D]`` and scale bytes ``[Hkv, R + 1, 1]``."""
    if not prefill_attn_kv8s_paged_supported(q, k8, v8, k_scale, v_scale, pos, table, page_size, num_pages):
        raise _refusal("prefill_attn_kv8s_paged", q=q, k=k8, v=v8, k_scale=k_scale, v_scale=v_scale, pos=pos,
                       table=table)
    return _prefill_launch("lta_prefill_attn_kv8s_paged", _rows_in_place(q), k8, v8, pos, scale,
                           scales=(k_scale, v_scale), pages=(table, page_size, num_pages), window=window)
