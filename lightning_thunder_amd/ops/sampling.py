"""Sampling kernels (``csrc/sampling.hip``): row-wise argmax of decode logits (greedy) and
temperature / top-k / top-p sampling from the project's Philox stream.

The definition of :func:`sample_last`, shared by the kernel, the torch fallback and the tests.  For a
row ``x[0..V)`` of logits in its storage dtype, ``temperature T > 0``, optional ``top_k >= 1``, optional
``top_p`` in (0, 1], Philox ``(seed, offset)`` and row index ``r``:

1. *top-k.*  If ``top_k < V``: ``t_k`` is the ``top_k``-th largest logit and ``K = {i : x_i >= t_k}``
   (ties at ``t_k`` are all kept; values compare as floats, so ``-0.0 == +0.0``).  Otherwise K is everything.
2. *top-p.*  If ``top_p < 1``: with ``z_i = x_i / T`` and ``m_i = exp(z_i - max_K z)``, ``t_p`` is the largest
   logit value ``v`` occurring in K with ``sum_{i in K, x_i >= v} m_i >= top_p * sum_K m_i`` and
   ``K <- {i in K : x_i >= t_p}``.  A tie group is never split and the maximum is always kept.
3. *draw* (Gumbel-max).  ``V4 = ceil(V / 4) * 4``, ``e = r * V4 + i``; ``w`` is word ``e % 4`` of
   ``philox4x32(counter=(blk_lo, blk_hi, off_lo, off_hi), key=(seed, 0))``, ``blk = e // 4`` (the convention of
   ``core/rng.py``); ``u_i = (2 * (w >> 9) + 1) * 2^-24`` (exact in fp32, strictly inside (0, 1)).  The token is
   ``argmax_{i in K} (z_i - log(-log(u_i)))``, the smallest index on ties.  One call consumes ``R * V4`` counters.
4. *special rows*, as :func:`argmax_last`: any NaN gives the index of the first NaN; else any ``+inf`` the
   smallest index holding ``+inf``; all ``-inf`` gives 0; ``-inf`` entries are otherwise never drawn.

Arithmetic is fp32 on the exactly upcast logits; only the top-p masses are summed wider (2^-40 fixed point in
the kernel, fp64 in the fallback), so that the sum does not depend on its order.
"""
from __future__ import annotations

import math
from typing import Optional

import torch

from ..core import rng
from ._lib import require, dcode, stream_ptr, check, register_signature, c_int, c_int64, c_void_p, c_float

register_signature("lta_argmax_rows", [c_int, c_void_p, c_void_p, c_int, c_int64, c_int64, c_void_p])
register_signature("lta_sample_rows", [c_int, c_void_p, c_void_p, c_int, c_int64, c_int64, c_float, c_int64, c_float,
                                       c_int64, c_int64, c_void_p])


def _kernel_ok(x: torch.Tensor, x2: torch.Tensor) -> bool:
    return (x.is_cuda and x.dtype in (torch.bfloat16, torch.float16, torch.float32)
            and x2.stride(-1) == 1 and x2.stride(0) % 8 == 0 and x2.data_ptr() % 16 == 0 and x2.shape[0] > 0)


def argmax_last(x: torch.Tensor, keepdim: bool = False) -> torch.Tensor:
    """``x.argmax(-1)`` for [..., V] logits; the HIP kernel on MI355X, torch elsewhere."""
    V = x.shape[-1]
    x2 = x.reshape(-1, V) if x.dim() != 2 else x
    if not _kernel_ok(x, x2):
        return x.argmax(-1, keepdim=keepdim)
    out = torch.empty(x2.shape[0], dtype=torch.int64, device=x.device)
    check(require().lta_argmax_rows(dcode(x2), x2.data_ptr(), out.data_ptr(), x2.shape[0], V, x2.stride(0),
                                    stream_ptr(x.device)), "lta_argmax_rows")
    out = out.reshape(x.shape[:-1])
    return out.unsqueeze(-1) if keepdim else out


def _f32(v: float) -> float:
    """``v`` rounded to fp32, as the kernel receives its scalar arguments."""
    return torch.tensor(v, dtype=torch.float32).item()


def _kept_mask(xf: torch.Tensor, temperature: float, top_k: Optional[int], top_p: Optional[float]) -> torch.Tensor:
    """Points 1 and 2 of the definition for [R, V] logits ``xf`` (fp32, or fp64 for a reference): the kept
    set as a bool mask.  Rows with a NaN are the caller's business (point 4)."""
    R, V = xf.shape
    keep = torch.ones_like(xf, dtype=torch.bool)
    if top_k is not None and top_k < V:
        keep = xf >= torch.topk(xf, top_k, dim=-1).values[:, -1:]
    if top_p is not None and top_p < 1:
        z = (xf / temperature).masked_fill(~keep, -math.inf)
        xs, order = torch.sort(xf.masked_fill(~keep, -math.inf), dim=-1, descending=True)
        ms = torch.exp(z - z.max(-1, keepdim=True).values).gather(-1, order).double()  # 0 outside K
        before = ms.cumsum(-1) - ms  # mass sorted ahead of j; for a tie group, take it at the group's first member
        j = torch.arange(V, device=xf.device).expand(R, V)
        first = torch.ones_like(keep)
        first[:, 1:] = xs[:, 1:] != xs[:, :-1]
        start = torch.cummax(torch.where(first, j, torch.zeros_like(j)), dim=-1).values
        above = before.gather(-1, start)  # mass of the kept logits strictly larger than this one
        keep_sorted = above < top_p * ms.sum(-1, keepdim=True)
        keep = keep & torch.zeros_like(keep).scatter_(-1, order, keep_sorted)
    return keep


def _gumbel_uniforms(R: int, V: int, seed: int, offset: int, device) -> torch.Tensor:
    """Point 3 of the definition: ``u`` [R, V] in fp32."""
    V4 = (V + 3) // 4 * 4
    blk = torch.arange(R * V4 // 4, device=device, dtype=torch.int64)
    m = 0xFFFFFFFF
    c2 = torch.full_like(blk, offset & m)
    c3 = torch.full_like(blk, (offset >> 32) & m)
    w = torch.stack(rng.philox4x32(blk & m, (blk >> 32) & m, c2, c3, seed & m, 0), dim=1).reshape(R, V4)[:, :V]
    return (2 * (w >> 9) + 1).to(torch.float32) * 2.0 ** -24


def _sample_rows_torch(x2: torch.Tensor, temperature: float, top_k, top_p, seed: int, offset: int) -> torch.Tensor:
    """The definition in torch, for calls the kernel does not take (CPU, misaligned rows, other dtypes)."""
    R, V = x2.shape
    xf = x2.float()
    T = _f32(temperature)
    keep = _kept_mask(xf, T, top_k, None if top_p is None else _f32(top_p)) & (xf != -math.inf)
    u = _gumbel_uniforms(R, V, seed, offset, x2.device)
    score = (xf / T - torch.log(-torch.log(u))).masked_fill(~keep, -math.inf)
    tok = score.argmax(-1)
    nan, pinf = xf.isnan(), xf == math.inf
    tok = torch.where(pinf.any(-1), pinf.int().argmax(-1), tok)
    tok = torch.where((xf == -math.inf).all(-1), torch.zeros_like(tok), tok)
    return torch.where(nan.any(-1), nan.int().argmax(-1), tok)


def sample_last(x: torch.Tensor, temperature: float, top_k: Optional[int] = None, top_p: Optional[float] = None, *,
                seed: Optional[int] = None, offset: Optional[int] = None, keepdim: bool = False) -> torch.Tensor:
    """One token per row of [..., V] logits, drawn after temperature, top-k and top-p filtering (the module
    docstring has the definition); int64.  ``temperature == 0`` is :func:`argmax_last`.

    Without ``seed`` and ``offset`` the call takes the next ``R * ceil(V / 4) * 4`` counters of the project's
    Philox stream (``core.rng``), which follows ``torch.manual_seed``.  The HIP kernel runs under the
    conditions of :func:`argmax_last`; every other call runs the same definition in torch and returns the same
    token unless two scores of a row are closer than fp32 rounding."""
    if not (math.isfinite(temperature) and temperature >= 0):
        raise ValueError(f"temperature must be finite and >= 0, got {temperature}")
    if top_k is not None and top_k < 1:
        raise ValueError(f"top_k must be >= 1, got {top_k}")
    if top_p is not None and not 0 < top_p <= 1:
        raise ValueError(f"top_p must lie in (0, 1], got {top_p}")
    if temperature == 0:
        return argmax_last(x, keepdim=keepdim)
    V = x.shape[-1]
    x2 = x.reshape(-1, V) if x.dim() != 2 else x
    R = x2.shape[0]
    if seed is None or offset is None:
        seed, offset = rng.next_seed_offset(R * ((V + 3) // 4 * 4))
    seed, offset = int(seed), int(offset)
    if _kernel_ok(x, x2):
        out = torch.empty(R, dtype=torch.int64, device=x.device)
        k = 0 if top_k is None or top_k >= V else int(top_k)
        check(require().lta_sample_rows(dcode(x2), x2.data_ptr(), out.data_ptr(), R, V, x2.stride(0), temperature, k,
                                        1.0 if top_p is None else top_p, seed, offset, stream_ptr(x.device)),
              "lta_sample_rows")
    else:
        out = _sample_rows_torch(x2, temperature, top_k, top_p, seed, offset)
    out = out.reshape(x.shape[:-1])
    return out.unsqueeze(-1) if keepdim else out
