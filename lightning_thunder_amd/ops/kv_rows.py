"""Ragged batches against the static KV cache, in plain torch: every sequence of a batch sits at its own
position, so token ``(b, t)`` carries ``input_pos[b, t]`` (LitGPT's batched ``input_pos``).

``position_mask`` is the attention mask of such a step (``window_mask`` under a sliding window) and ``write_rows`` its
cache write; they are the definition the kernels follow (``csrc/decode_attention.hip`` position and window modes,
``csrc/rope.hip`` per-row mode).
The masks are also ``torch.library`` custom ops (``lta::kv_position_mask``, ``lta::kv_window_mask``), so a traced
program holds each as one symbol that the HIP executor can drop once the decode kernels read the positions themselves.
"""
from __future__ import annotations

import torch


def position_mask(input_pos: torch.Tensor, S: int) -> torch.Tensor:
    """bool ``[B, 1, T, S]``: ``mask[b, 0, t, j] = j <= input_pos[b, t]`` (key j is visible to the token at
    position ``input_pos[b, t]`` of sequence b)."""
    j = torch.arange(S, device=input_pos.device)
    return (j <= input_pos[:, None, :, None])


@torch.library.custom_op("lta::kv_position_mask", mutates_args=())
def kv_position_mask(input_pos: torch.Tensor, S: int) -> torch.Tensor:
    return position_mask(input_pos, S)


@kv_position_mask.register_fake
def _kv_position_mask_fake(input_pos, S):
    B, T = input_pos.shape
    return input_pos.new_empty((B, 1, T, S), dtype=torch.bool)


def window_mask(input_pos: torch.Tensor, S: int, window: int) -> torch.Tensor:
    """bool ``[B, 1, T, S]``: ``position_mask`` under a sliding window, ``mask[b, 0, t, j] = input_pos[b, t] - window
    < j <= input_pos[b, t]``.  The token at position p sees ``window`` keys, itself included (the Mistral / HF
    convention; LitGPT's own mask keeps ``window + 1``).  ``window >= S`` is ``position_mask``."""
    j = torch.arange(S, device=input_pos.device)
    p = input_pos[:, None, :, None]
    return (j <= p) & (j > p - window)


@torch.library.custom_op("lta::kv_window_mask", mutates_args=())
def kv_window_mask(input_pos: torch.Tensor, S: int, window: int) -> torch.Tensor:
    return window_mask(input_pos, S, window)


@kv_window_mask.register_fake
def _kv_window_mask_fake(input_pos, S, window):
    B, T = input_pos.shape
    return input_pos.new_empty((B, 1, T, S), dtype=torch.bool)


def write_rows(cache: torch.Tensor, input_pos: torch.Tensor, src: torch.Tensor) -> torch.Tensor:
    """``cache[b, :, input_pos[b, t], :] = src[b, :, t, :]`` in place (cache ``[B, H, S, D]``, src
    ``[B, H, T, D]``, input_pos int64 ``[B, T]``); O(tokens) work.  Returns ``cache``."""
    return cache.scatter_(2, input_pos[:, None, :, None].expand_as(src), src)
