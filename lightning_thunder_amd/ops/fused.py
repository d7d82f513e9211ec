"""Wrappers for K6 (qkv split + RoPE), SwiGLU and K7 (cross entropy) kernels."""
from __future__ import annotations

import ctypes

import torch

from ._lib import require, dcode, ptr, stream_ptr, check, register_signature, c_int, c_int64, c_void_p, c_float
from .kv8 import scale_caches_of

register_signature("lta_qkv_rope_fwd", [c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                        c_int, c_int, c_int, c_int, c_int, c_int, c_void_p])
# the cache-writing entries: pointers qkv, cos, sin, q, kc, vc, <scale caches>, pos, strides; the per-row entries
# take the caches' capacity S after rope_n
for _entry, _scale_ptrs in (("lta_qkv_rope_cache_fwd", 0), ("lta_qkv_rope_cache_fwd_kv8", 0),
                            ("lta_qkv_rope_cache_fwd_kv8s", 2)):
    register_signature(_entry, [c_int, c_int, *[c_void_p] * (8 + _scale_ptrs), *[c_int] * 6, c_void_p])
    register_signature(_entry + "_rows", [c_int, c_int, *[c_void_p] * (8 + _scale_ptrs), *[c_int] * 7, c_void_p])
register_signature("lta_qkv_rope_bwd", [c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                        c_int, c_int, c_int, c_int, c_int, c_int, c_void_p])
register_signature("lta_swiglu_fwd", [c_int, c_void_p, c_void_p, c_void_p, c_int64, c_void_p])
register_signature("lta_swiglu_bwd", [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p])
register_signature("lta_ce_fwd", [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int64,
                                  c_int, c_float, c_void_p])
register_signature("lta_ce_bwd", [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64,
                                  c_int64, c_int, c_float, c_void_p])
register_signature("lta_ce_fwd_w", [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64,
                                    c_int64, c_int, c_float, c_void_p])
register_signature("lta_ce_bwd_w", [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64,
                                    c_int64, c_int64, c_int, c_float, c_void_p])


def _c(t):
    return t if t.is_contiguous() else t.contiguous()


def qkv_rope_fwd(qkv, cos, sin, n_head: int, n_query_groups: int, head_size: int, rope_n: int):
    lib = require()
    qkv = _c(qkv)
    B, T, _ = qkv.shape
    cos = _c(cos[:T])
    sin = _c(sin[:T])
    if cos.dtype != sin.dtype:
        sin = sin.to(cos.dtype)
    if cos.dtype not in (torch.float32, qkv.dtype):
        cos, sin = cos.float(), sin.float()
    q = torch.empty((B, n_head, T, head_size), device=qkv.device, dtype=qkv.dtype)
    k = torch.empty((B, n_query_groups, T, head_size), device=qkv.device, dtype=qkv.dtype)
    v = torch.empty_like(k)
    rc = lib.lta_qkv_rope_fwd(dcode(qkv), dcode(cos), ptr(qkv), ptr(cos), ptr(sin), ptr(q), ptr(k), ptr(v), B, T,
                              n_head, n_query_groups, head_size, rope_n, stream_ptr(qkv.device))
    check(rc, "lta_qkv_rope_fwd")
    return q, k, v


def _row_kernel_shape(dtype, head_size: int, rope_n: int) -> bool:
    """What csrc/rope.hip's one-row-per-workgroup kernel takes (its ``row_pair_shift >= 0``)."""
    pairs = head_size // 16
    return (dtype in (torch.bfloat16, torch.float16) and rope_n == head_size and head_size % 16 == 0
            and pairs > 0 and pairs & (pairs - 1) == 0)


def qkv_rope_cache_supported(qkv, kc, vc, pos, n_query_groups: int, head_size: int, rope_n: int | None = None) -> bool:
    """Static caches [B, ng, S, hs] (head dim contiguous, 16-byte aligned rows) and int64 positions.
    uint8 caches (unscaled e4m3, 8-byte aligned rows) only at the row kernel's shapes: full rotation
    (``rope_n``, taken as ``head_size`` when not given) and ``head_size / 16`` a power of two."""
    B, T, _ = qkv.shape
    kv8 = kc.dtype == torch.uint8 and vc.dtype == torch.uint8
    if kv8 and not _row_kernel_shape(qkv.dtype, head_size, head_size if rope_n is None else rope_n):
        return False
    for c in (kc, vc):
        if c.dtype != (torch.uint8 if kv8 else qkv.dtype) or c.dim() != 4:
            return False
        if tuple(c.shape[:2]) != (B, n_query_groups) or c.shape[3] != head_size:
            return False
        if c.stride(3) != 1 or any(st % 8 for st in c.stride()[:3]) or c.data_ptr() % (8 if kv8 else 16):
            return False
    return pos.dtype == torch.int64 and pos.dim() == 1 and pos.numel() == T and pos.is_contiguous()


def qkv_rope_cache_scaled_supported(qkv, kc, vc, k_scale, v_scale, pos, n_query_groups: int, head_size: int,
                                    rope_n: int | None = None) -> bool:
    """What the scaled e4m3 write takes: uint8 caches as ``qkv_rope_cache_supported`` has them, a head row
    within one wave (``head_size <= 1024``), and uint8 scale caches [B, ng, S, 1] over the same rows."""
    if kc.dtype != torch.uint8 or vc.dtype != torch.uint8 or head_size > 1024:
        return False
    return (qkv_rope_cache_supported(qkv, kc, vc, pos, n_query_groups, head_size, rope_n)
            and scale_caches_of((k_scale, v_scale), (kc, vc)))


def _qkv_rope_cache_launch(qkv, cos, sin, n_head, n_query_groups, head_size, rope_n, caches, pos, suffix="", *capacity,
                           pooled: bool = False):
    """One launch of the cache-writing entry for ``caches`` = (kc, vc) or (kc, vc, k_scale, v_scale), over contiguous
    qkv / cos / sin / pos; the per-row entries have the ``suffix`` "_rows" and take the caches' ``capacity`` after
    rope_n.  ``pooled``: the caches are the ``[ng, rows, hs]`` pools of a paged cache, shared by the batch (batch
    stride 0).  Returns (q, *caches)."""
    lib = require()
    B, T, _ = qkv.shape
    if cos.dtype != sin.dtype:
        sin = sin.to(cos.dtype)
    if cos.dtype not in (torch.float32, qkv.dtype):
        cos, sin = cos.float(), sin.float()
    q = torch.empty((B, n_head, T, head_size), device=qkv.device, dtype=qkv.dtype)
    st = (ctypes.c_int64 * (3 * len(caches)))(*(s for c in caches
                                                for s in ((0, *c.stride()[:2]) if pooled else c.stride()[:3])))
    entry = ("lta_qkv_rope_cache_fwd" + ("_kv8s" if len(caches) == 4 else "_kv8" if caches[0].dtype == torch.uint8 else "")
             + suffix)
    rc = getattr(lib, entry)(dcode(qkv), dcode(cos), ptr(qkv), ptr(cos), ptr(sin), ptr(q), *map(ptr, caches), ptr(pos),
                             st, B, T, n_head, n_query_groups, head_size, rope_n, *capacity, stream_ptr(qkv.device))
    check(rc, entry)
    return (q, *caches)


def qkv_rope_cache_fwd(qkv, cos, sin, n_head: int, n_query_groups: int, head_size: int, rope_n: int, kc, vc, pos,
                       k_scale=None, v_scale=None):
    """qkv split + RoPE with k / v written in place into the static caches ``kc`` / ``vc`` at rows
    ``pos`` (the decode step's ``index_copy_`` fused into the same launch).  Returns (q, kc, vc).
    uint8 caches receive the rows as unscaled saturating e4m3: bit for bit ``ops/kv8.py``'s ``e4m3_bytes``
    of ``qkv_rope_fwd``'s k (and v).
    With ``k_scale`` / ``v_scale`` (uint8 [B, ng, S, 1]) the caches are the scaled ones of ``ops/kv8.py``:
    bytes and scale bytes equal ``quantise_rows`` of ``qkv_rope_fwd``'s k (and v) bit for bit, and the
    result is (q, kc, vc, k_scale, v_scale)."""
    if (k_scale is None) != (v_scale is None):
        raise ValueError("qkv_rope_cache_fwd: k_scale and v_scale come together")
    scales = () if k_scale is None else (k_scale, v_scale)
    if scales and not qkv_rope_cache_scaled_supported(qkv, kc, vc, k_scale, v_scale, pos, n_query_groups, head_size,
                                                      rope_n):
        raise ValueError("qkv_rope_cache_fwd: operands the scaled e4m3 write does not take "
                         "(see qkv_rope_cache_scaled_supported)")
    T = qkv.shape[1]
    return _qkv_rope_cache_launch(_c(qkv), _c(cos[:T]), _c(sin[:T]), n_head, n_query_groups, head_size, rope_n,
                                  (kc, vc, *scales), pos)


def qkv_rope_cache_rows_supported(qkv, cos, sin, kc, vc, pos, n_query_groups: int, head_size: int,
                                  rope_n: int | None = None, k_scale=None, v_scale=None) -> bool:
    """What the per-row write takes: the caches of ``qkv_rope_cache_supported`` (or, with scale caches, of
    ``qkv_rope_cache_scaled_supported``), one int64 position per token ``[B, T]`` and cos / sin ``[B, T, rope_n]``
    gathered per token."""
    if (k_scale is None) != (v_scale is None) or qkv.dim() != 3 or pos.dim() != 2:
        return False
    B, T, _ = qkv.shape
    rn = head_size if rope_n is None else rope_n
    if B == 0 or pos.dtype != torch.int64 or tuple(pos.shape) != (B, T) or pos.device != qkv.device:
        return False
    if head_size % 8 or rn % 16 or rn > head_size:
        return False
    if kc.dim() != 4 or vc.dim() != 4 or kc.shape[2] != vc.shape[2]:  # one capacity bounds every write
        return False
    if any(t.dim() != 3 or tuple(t.shape) != (B, T, rn) or not t.is_floating_point() for t in (cos, sin)):
        return False
    flat = _c(pos[0])  # the cache rules want T int64 positions; which ones does not matter to them
    if k_scale is not None:
        return qkv_rope_cache_scaled_supported(qkv, kc, vc, k_scale, v_scale, flat, n_query_groups, head_size, rn)
    return qkv_rope_cache_supported(qkv, kc, vc, flat, n_query_groups, head_size, rn)


def qkv_rope_cache_rows_fwd(qkv, cos, sin, n_head: int, n_query_groups: int, head_size: int, rope_n: int, kc, vc, pos,
                            k_scale=None, v_scale=None):
    """``qkv_rope_cache_fwd`` for a ragged batch: ``pos`` int64 ``[B, T]`` and cos / sin ``[B, T, rope_n]`` hold
    every token's own position and rotation; token (b, t) writes row ``pos[b, t]`` of sequence b's caches.  A
    position outside ``[0, S)`` writes nothing (q is still returned for it).  Same bytes as the shared-position
    write otherwise; returns (q, kc, vc) or (q, kc, vc, k_scale, v_scale)."""
    if not qkv_rope_cache_rows_supported(qkv, cos, sin, kc, vc, pos, n_query_groups, head_size, rope_n, k_scale,
                                         v_scale):
        raise ValueError("qkv_rope_cache_rows_fwd: operands the per-row write does not take "
                         "(see qkv_rope_cache_rows_supported)")
    scales = () if k_scale is None else (k_scale, v_scale)
    return _qkv_rope_cache_launch(_c(qkv), _c(cos), _c(sin), n_head, n_query_groups, head_size, rope_n,
                                  (kc, vc, *scales), _c(pos), "_rows", kc.shape[2])


def qkv_rope_cache_slots_supported(qkv, cos, sin, kp, vp, slots, n_query_groups: int, head_size: int,
                                   rope_n: int | None = None, k_scale=None, v_scale=None) -> bool:
    """``qkv_rope_cache_rows_supported`` for the pools of a paged cache (``ops/kv_pages.py``): kp / vp
    ``[ng, R + 1, hs]`` under the same dtype, layout and alignment rules, scale pools uint8 ``[ng, R + 1, 1]``, one
    int64 pool row per token ``slots`` ``[B, T]`` and cos / sin ``[B, T, rope_n]``."""
    if (k_scale is None) != (v_scale is None) or qkv.dim() != 3 or slots.dim() != 2:
        return False
    B, T, _ = qkv.shape
    rn = head_size if rope_n is None else rope_n
    if B == 0 or slots.dtype != torch.int64 or tuple(slots.shape) != (B, T) or slots.device != qkv.device:
        return False
    if head_size % 8 or rn % 16 or rn > head_size:
        return False
    if any(t.dim() != 3 or tuple(t.shape) != (B, T, rn) or not t.is_floating_point() for t in (cos, sin)):
        return False
    kv8 = kp.dtype == torch.uint8 and vp.dtype == torch.uint8
    if kv8 and not _row_kernel_shape(qkv.dtype, head_size, rn):
        return False
    if kp.dim() != 3 or vp.dim() != 3 or kp.shape[1] != vp.shape[1] or kp.shape[1] < 1:  # one capacity bounds every write
        return False
    for c in (kp, vp):
        if c.dtype != (torch.uint8 if kv8 else qkv.dtype) or c.device != qkv.device:
            return False
        if c.shape[0] != n_query_groups or c.shape[2] != head_size:
            return False
        if c.stride(2) != 1 or any(st % 8 for st in c.stride()[:2]) or c.data_ptr() % (8 if kv8 else 16):
            return False
    if k_scale is None:
        return True
    return kv8 and head_size <= 1024 and all(
        s.dtype == torch.uint8 and s.device == qkv.device and tuple(s.shape) == (n_query_groups, kp.shape[1], 1)
        for s in (k_scale, v_scale))


def qkv_rope_cache_slots_fwd(qkv, cos, sin, n_head: int, n_query_groups: int, head_size: int, rope_n: int, kp, vp,
                             slots, k_scale=None, v_scale=None):
    """``qkv_rope_cache_rows_fwd`` into the pools of a paged cache: token (b, t) writes pool row ``slots[b, t]``
    (``ops/kv_pages.py`` ``page_slots``) of kp / vp ``[ng, R + 1, hs]`` through the per-row entries, with the pools'
    (0, head, row) strides and the capacity ``R``: a token whose slot is the sink row ``R`` (or any row outside
    ``[0, R)``) writes nothing.  Returns (q, kp, vp) or (q, kp, vp, k_scale, v_scale)."""
    if not qkv_rope_cache_slots_supported(qkv, cos, sin, kp, vp, slots, n_query_groups, head_size, rope_n, k_scale,
                                          v_scale):
        raise ValueError("qkv_rope_cache_slots_fwd: operands the slot write does not take "
                         "(see qkv_rope_cache_slots_supported)")
    scales = () if k_scale is None else (k_scale, v_scale)
    return _qkv_rope_cache_launch(_c(qkv), _c(cos), _c(sin), n_head, n_query_groups, head_size, rope_n,
                                  (kp, vp, *scales), _c(slots), "_rows", kp.shape[1] - 1, pooled=True)


def qkv_rope_rows_fwd(qkv, cos, sin, n_head: int, n_query_groups: int, head_size: int, rope_n: int):
    """``qkv_rope_fwd`` with one rotation per token, cos / sin ``[B, T, rope_n]``: the per-row kernels writing fresh
    k / v ``[B, ng, T, hs]`` at rows ``0 .. T-1``.  Returns (q, k, v)."""
    B, T, _ = qkv.shape
    k = torch.empty((B, n_query_groups, T, head_size), device=qkv.device, dtype=qkv.dtype)
    v = torch.empty_like(k)
    pos = torch.arange(T, device=qkv.device).expand(B, T).contiguous()
    return qkv_rope_cache_rows_fwd(qkv, cos, sin, n_head, n_query_groups, head_size, rope_n, k, v, pos)


def qkv_rope_bwd(dq, dk, dv, cos, sin, n_head: int, n_query_groups: int, head_size: int, rope_n: int):
    lib = require()
    dq, dk, dv = _c(dq), _c(dk), _c(dv)
    B, _, T, _ = dq.shape
    cos = _c(cos[:T])
    sin = _c(sin[:T])
    if cos.dtype != sin.dtype:
        sin = sin.to(cos.dtype)
    if cos.dtype not in (torch.float32, dq.dtype):
        cos, sin = cos.float(), sin.float()
    dqkv = torch.empty((B, T, (n_head + 2 * n_query_groups) * head_size), device=dq.device, dtype=dq.dtype)
    rc = lib.lta_qkv_rope_bwd(dcode(dq), dcode(cos), ptr(dq), ptr(dk), ptr(dv), ptr(cos), ptr(sin), ptr(dqkv), B, T,
                              n_head, n_query_groups, head_size, rope_n, stream_ptr(dq.device))
    check(rc, "lta_qkv_rope_bwd")
    return dqkv


def swiglu_fwd(a, b):
    lib = require()
    a, b = _c(a), _c(b)
    y = torch.empty_like(a)
    check(lib.lta_swiglu_fwd(dcode(a), ptr(a), ptr(b), ptr(y), a.numel(), stream_ptr(a.device)), "lta_swiglu_fwd")
    return y


def swiglu_bwd(g, a, b):
    lib = require()
    g, a, b = _c(g), _c(a), _c(b)
    da = torch.empty_like(a)
    db = torch.empty_like(b)
    check(lib.lta_swiglu_bwd(dcode(a), ptr(g), ptr(a), ptr(b), ptr(da), ptr(db), a.numel(), stream_ptr(a.device)),
          "lta_swiglu_bwd")
    return da, db


_REDUCTION = {"none": 0, "mean": 1, "sum": 2}


def _ce_weight(weight):
    return None if weight is None else _c(weight.to(torch.float32))


def cross_entropy_fwd(logits, target, ignore_index: int = -100, reduction: str = "mean", label_smoothing: float = 0.0,
                      weight=None):
    """Returns (loss [in logits dtype; per-row when reduction='none'], lse [rows] fp32, stats [2] fp32).
    ``weight``: optional [V] class weights (torch semantics: 'mean' divides by the kept rows' target
    weights; stats[1] holds that sum)."""
    lib = require()
    logits = _c(logits)
    target = _c(target.to(torch.int64))
    rows, V = logits.shape
    loss_rows = torch.empty(rows, device=logits.device, dtype=torch.float32)
    lse = torch.empty(rows, device=logits.device, dtype=torch.float32)
    stats = torch.empty(2, device=logits.device, dtype=torch.float32)
    r = _REDUCTION[reduction]
    w = _ce_weight(weight)
    check(lib.lta_ce_fwd_w(dcode(logits), ptr(logits), ptr(target), ptr(w), ptr(loss_rows), ptr(lse), ptr(stats), rows,
                           V, int(ignore_index), r, float(label_smoothing), stream_ptr(logits.device)), "lta_ce_fwd")
    if r == 0:
        loss = loss_rows.to(logits.dtype)
    else:
        loss = stats[0].to(logits.dtype)
    return loss, lse, stats


def ce_row_stats(logits, target_local, ignore_index: int = -100):
    """Per-row fp32 ``(lse, lse - x[target])`` of ``logits`` [rows, V] in ONE pass of the hand CE kernel
    (rows whose ``target_local`` is ``ignore_index`` get 0 in the second output) — the local half of
    a vocab-parallel cross-entropy."""
    lib = require()
    logits = _c(logits)
    target = _c(target_local.to(torch.int64))
    rows, V = logits.shape
    loss_rows = torch.empty(rows, device=logits.device, dtype=torch.float32)
    lse = torch.empty(rows, device=logits.device, dtype=torch.float32)
    check(lib.lta_ce_fwd_w(dcode(logits), ptr(logits), ptr(target), None, ptr(loss_rows), ptr(lse), None, rows, V,
                           int(ignore_index), 0, 0.0, stream_ptr(logits.device)), "lta_ce_fwd")
    return lse, loss_rows


def cross_entropy_bwd(g, logits, target, lse, stats, ignore_index: int = -100, reduction: str = "mean",
                      label_smoothing: float = 0.0, weight=None):
    lib = require()
    logits = _c(logits)
    target = _c(target.to(torch.int64))
    rows, V = logits.shape
    gs = _c(g.float().reshape(-1))
    dl = torch.empty_like(logits)
    w = _ce_weight(weight)
    check(lib.lta_ce_bwd_w(dcode(logits), ptr(logits), ptr(target), ptr(w), ptr(lse), ptr(gs), ptr(stats), ptr(dl), rows,
                           V, int(ignore_index), _REDUCTION[reduction], float(label_smoothing),
                           stream_ptr(logits.device)), "lta_ce_bwd")
    return dl
