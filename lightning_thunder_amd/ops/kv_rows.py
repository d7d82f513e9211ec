"""Ragged batches against the static KV cache, in plain torch: every sequence of a batch sits at its own
position, so token ``(b, t)`` carries ``input_pos[b, t]`` (LitGPT's batched ``input_pos``).

``position_mask`` is the attention mask of such a step and ``write_rows`` its cache write; they are the
definition the kernels follow (``csrc/decode_attention.hip`` position mode, ``csrc/rope.hip`` per-row mode).
The mask is also a ``torch.library`` custom op (``lta::kv_position_mask``), so a traced program holds it as
one symbol that the HIP executor can drop once the decode kernels read the positions themselves.
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


def write_rows(cache: torch.Tensor, input_pos: torch.Tensor, src: torch.Tensor) -> torch.Tensor:
    """``cache[b, :, input_pos[b, t], :] = src[b, :, t, :]`` in place (cache ``[B, H, S, D]``, src
    ``[B, H, T, D]``, input_pos int64 ``[B, T]``); O(tokens) work.  Returns ``cache``."""
    return cache.scatter_(2, input_pos[:, None, :, None].expand_as(src), src)
