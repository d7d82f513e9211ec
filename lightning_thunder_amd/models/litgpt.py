"""LitGPT-architecture decoder models in plain PyTorch (parity: the LitGPT configs/model used by the
reference's ``thunder/benchmarks/benchmark_litgpt.py:295,335`` and ``thunder/tests/litgpt_model.py:1-131``).

LitGPT itself is not installed in this image, so the architecture is defined
here with LitGPT's module names (``transformer.wte``, ``transformer.h[i].attn.attn``,
``mlp.fc_1/fc_2/proj``, ``lm_head`` …) so checkpoints and traces line up.

Hot spots live in small module-level helpers (``apply_rope``, ``qkv_split_rope``)
written in plain torch; the HIP executor registers lookasides for them so a
compiled model runs the fused CDNA4 kernels while eager PyTorch runs the same
math unfused (that is the "speedup vs eager" baseline).
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field, replace
from typing import List, Optional

import torch
import torch.nn as nn
import torch.utils.checkpoint
import torch.nn.functional as F

from ..ops.kv8 import kv8_dequantise_rows, kv8_quantise_rows
from ..ops.kv_pages import (PageTable, check_page_size, kv_page_slots, kv_paged_gather, kv_paged_mask,
                            kv_paged_window_mask)
from ..ops.kv_rows import kv_position_mask, kv_window_mask


@dataclass
class Config:
    name: str = ""
    block_size: int = 4096
    vocab_size: int = 32000
    padded_vocab_size: Optional[int] = None
    padding_multiple: int = 512
    n_layer: int = 32
    n_head: int = 32
    n_embd: int = 4096
    head_size: Optional[int] = None
    n_query_groups: Optional[int] = None
    rotary_percentage: float = 1.0
    parallel_residual: bool = False
    bias: bool = False
    norm_class_name: str = "RMSNorm"
    norm_eps: float = 1e-5
    mlp_class_name: str = "LLaMAMLP"
    intermediate_size: Optional[int] = None
    rope_base: int = 10000
    rope_condense_ratio: int = 1
    shared_attention_norm: bool = False
    gelu_approximate: str = "none"
    tie_embeddings: bool = False
    n_expert: int = 0
    n_expert_per_token: int = 0
    # Gemma: token embeddings scaled by sqrt(n_embd), RMSNorm scale (1 + weight)
    scale_embeddings: bool = False
    norm_unit_offset: bool = False
    # Sliding-window attention (Mistral, Phi-3, Gemma-2): the token at position p sees key j iff p - W < j <= p, that
    # is W keys, itself included (the Mistral / HF convention; LitGPT's own mask keeps W + 1).
    # ``sliding_window_indices`` holds one 0 / 1 per layer (1: the layer is windowed); all ones when only the size is set.
    sliding_window_size: Optional[int] = None
    sliding_window_indices: Optional[List[int]] = None

    def __post_init__(self):
        if self.sliding_window_indices is not None and len(self.sliding_window_indices) != self.n_layer:
            raise ValueError(f"Config: sliding_window_indices has {len(self.sliding_window_indices)} entries for "
                             f"{self.n_layer} layers")
        if self.sliding_window_size is None:
            self.sliding_window_indices = None
        else:
            W = self.sliding_window_size
            if isinstance(W, bool) or not isinstance(W, int) or W < 1:
                raise ValueError(f"Config: sliding_window_size must be an int >= 1 or None, got {W!r}")
            if self.sliding_window_indices is None:
                self.sliding_window_indices = [1] * self.n_layer
        if self.head_size is None:
            self.head_size = self.n_embd // self.n_head
        if self.padded_vocab_size is None:
            self.padded_vocab_size = ((self.vocab_size + self.padding_multiple - 1) // self.padding_multiple) * self.padding_multiple
        if self.n_query_groups is None:
            self.n_query_groups = self.n_head
        if self.intermediate_size is None:
            self.intermediate_size = 4 * self.n_embd
        self.rope_n_elem = int(self.rotary_percentage * self.head_size)

    @classmethod
    def from_name(cls, name: str, **kwargs) -> "Config":
        base = name_to_config[name]
        if "sliding_window_indices" not in kwargs and base.sliding_window_indices is not None \
                and all(base.sliding_window_indices):
            kwargs["sliding_window_indices"] = None  # "every layer" follows an n_layer given here
        return replace(base, **kwargs)

    def layer_window(self, block_idx: int) -> Optional[int]:
        """The window of layer ``block_idx``, None for a layer that attends every earlier key."""
        if self.sliding_window_size is None or not self.sliding_window_indices[block_idx]:
            return None
        return self.sliding_window_size

    @property
    def uniform_window(self) -> Optional[int]:
        """The window when every layer has it (only then may a paged cache give up the pages below it), else None."""
        if self.sliding_window_size is None or not all(self.sliding_window_indices):
            return None
        return self.sliding_window_size

    @property
    def qkv_size(self) -> int:
        return (self.n_head + 2 * self.n_query_groups) * self.head_size


configs = [
    # Meta Llama 2
    Config(name="Llama-2-7b-hf", vocab_size=32000, padding_multiple=64, n_layer=32, n_head=32, n_embd=4096,
           intermediate_size=11008, norm_eps=1e-5),
    Config(name="Llama-2-13b-hf", vocab_size=32000, padding_multiple=64, n_layer=40, n_head=40, n_embd=5120,
           intermediate_size=13824, norm_eps=1e-5),
    Config(name="Llama-2-70b-hf", vocab_size=32000, padding_multiple=64, n_layer=80, n_head=64, n_embd=8192,
           n_query_groups=8, intermediate_size=28672, norm_eps=1e-5),
    # Meta Llama 3
    Config(name="Llama-3-8B", block_size=8192, vocab_size=128000, padded_vocab_size=128256, n_layer=32, n_head=32,
           n_embd=4096, n_query_groups=8, intermediate_size=14336, rope_base=500000),
    Config(name="Llama-3-70B", block_size=8192, vocab_size=128000, padded_vocab_size=128256, n_layer=80, n_head=64,
           n_embd=8192, n_query_groups=8, intermediate_size=28672, rope_base=500000),
    Config(name="Llama-3.2-1B", block_size=8192, vocab_size=128000, padded_vocab_size=128256, n_layer=16, n_head=32,
           n_embd=2048, n_query_groups=8, intermediate_size=8192, rope_base=500000, tie_embeddings=True),
    # Mistral
    Config(name="Mistral-7B-v0.1", block_size=4096, vocab_size=32000, padded_vocab_size=32000, n_layer=32, n_head=32,
           n_embd=4096, n_query_groups=8, intermediate_size=14336, sliding_window_size=4096),
    Config(name="Mistral-7B-v0.2", block_size=32768, vocab_size=32000, padded_vocab_size=32000, n_layer=32, n_head=32,
           n_embd=4096, n_query_groups=8, intermediate_size=14336, rope_base=1000000),
    # Google Gemma (the reference's multi-model chart and GemmaMLP target, BASELINE.md:26):
    # head_size 256 (n_head * head_size != n_embd), GeGLU (tanh) MLP, scaled embeddings, (1 + w) RMSNorm
    Config(name="Gemma-2b", block_size=8192, vocab_size=256000, padding_multiple=64, n_layer=18, n_head=8,
           n_query_groups=1, n_embd=2048, head_size=256, intermediate_size=16384, mlp_class_name="GemmaMLP",
           gelu_approximate="tanh", scale_embeddings=True, norm_unit_offset=True, norm_eps=1e-6, tie_embeddings=True),
    Config(name="Gemma-7b", block_size=8192, vocab_size=256000, padding_multiple=64, n_layer=28, n_head=16,
           n_query_groups=16, n_embd=3072, head_size=256, intermediate_size=24576, mlp_class_name="GemmaMLP",
           gelu_approximate="tanh", scale_embeddings=True, norm_unit_offset=True, norm_eps=1e-6, tie_embeddings=True),
    # Microsoft Phi-3
    Config(name="Phi-3-mini-4k-instruct", block_size=4096, vocab_size=32064, padded_vocab_size=32064, n_layer=32,
           n_head=32, n_embd=3072, intermediate_size=8192, norm_eps=1e-5),
    # Llama-1-architecture fine-tunes of the chart
    Config(name="Nous-Hermes-13b", block_size=2048, vocab_size=32000, padded_vocab_size=32001, n_layer=40, n_head=40,
           n_embd=5120, intermediate_size=13824, norm_eps=1e-6),
    Config(name="Platypus-30B", block_size=2048, vocab_size=32000, padded_vocab_size=32000, n_layer=60, n_head=52,
           n_embd=6656, intermediate_size=17920, norm_eps=1e-6),
    # CodeLlama
    Config(name="CodeLlama-34b-hf", block_size=16384, vocab_size=32000, padded_vocab_size=32000, n_layer=48, n_head=64,
           n_embd=8192, n_query_groups=8, intermediate_size=22016, rope_base=1000000),
    # Small test configs (reference thunder/tests/litgpt_model.py)
    Config(name="llama2-like", vocab_size=320, padding_multiple=64, n_layer=2, n_head=4, n_embd=64, intermediate_size=86,
           block_size=128),
    Config(name="llama3-like", vocab_size=320, padded_vocab_size=320, n_layer=2, n_head=4, n_embd=64, n_query_groups=2,
           intermediate_size=96, block_size=128, rope_base=500000),
    # llama3-like under a 24-key sliding window: on every layer (Mistral), on the even layers only (Gemma-2)
    Config(name="mistral-like", vocab_size=320, padded_vocab_size=320, n_layer=2, n_head=4, n_embd=64, n_query_groups=2,
           intermediate_size=96, block_size=128, rope_base=500000, sliding_window_size=24),
    Config(name="gemma2-like", vocab_size=320, padded_vocab_size=320, n_layer=2, n_head=4, n_embd=64, n_query_groups=2,
           intermediate_size=96, block_size=128, rope_base=500000, sliding_window_size=24,
           sliding_window_indices=[1, 0]),
    Config(name="gpt-neox-like", vocab_size=320, padding_multiple=64, n_layer=2, n_head=4, n_embd=64, block_size=128,
           norm_class_name="LayerNorm", mlp_class_name="GptNeoxMLP", bias=True, parallel_residual=True,
           rotary_percentage=0.25),
    # Mixtral-style sparse MoE (litgpt "LLaMAMoE"): 8 experts, top-2 routing
    Config(name="Mixtral-8x7B-v0.1", vocab_size=32000, padding_multiple=512, n_layer=32, n_head=32, n_embd=4096,
           n_query_groups=8, intermediate_size=14336, mlp_class_name="LLaMAMoE", n_expert=8, n_expert_per_token=2,
           rope_base=1000000, norm_eps=1e-5),
    Config(name="mixtral-like", vocab_size=320, padding_multiple=64, n_layer=2, n_head=4, n_embd=256, n_query_groups=2,
           intermediate_size=512, mlp_class_name="LLaMAMoE", n_expert=4, n_expert_per_token=2),
    Config(name="llama2-7b-shape-2l", vocab_size=32000, padding_multiple=64, n_layer=2, n_head=32, n_embd=4096,
           intermediate_size=11008),
    Config(name="gemma-like", vocab_size=320, padding_multiple=64, n_layer=2, n_head=2, n_query_groups=1, n_embd=64,
           head_size=256, intermediate_size=128, block_size=128, mlp_class_name="GemmaMLP", gelu_approximate="tanh",
           scale_embeddings=True, norm_unit_offset=True, norm_eps=1e-6, tie_embeddings=True),
]
name_to_config = {c.name: c for c in configs}


def build_rope_cache(seq_len: int, n_elem: int, device=None, base: int = 10000, condense_ratio: int = 1):
    theta = 1.0 / (base ** (torch.arange(0, n_elem, 2, device=device).float() / n_elem))
    seq_idx = torch.arange(seq_len, device=device) / condense_ratio
    idx_theta = torch.outer(seq_idx, theta).repeat(1, 2)
    return torch.cos(idx_theta), torch.sin(idx_theta)


def apply_rope(x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor) -> torch.Tensor:
    """x: [B, H, T, hs]; cos/sin: [T, hs], or [B, T, hs] gathered per sequence (a ragged batch), which
    broadcast over the heads  (LitGPT's rotate-half formulation)."""
    if cos.dim() == 3:
        cos = cos.unsqueeze(1)
        sin = sin.unsqueeze(1)
    head_size = x.size(-1)
    x1 = x[..., : head_size // 2]
    x2 = x[..., head_size // 2:]
    rotated = torch.cat((-x2, x1), dim=-1)
    roped = (x * cos) + (rotated * sin)
    return roped.to(dtype=x.dtype)


def qkv_split_rope(qkv: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, n_head: int, n_query_groups: int,
                   head_size: int, rope_n_elem: int):
    """Splits fused qkv [B, T, (nh+2*ng)*hs] into q [B, nh, T, hs], k/v [B, ng, T, hs] and applies RoPE to q, k."""
    B, T, _ = qkv.shape
    q_size = n_head * head_size
    kv_size = n_query_groups * head_size
    q, k, v = qkv.split((q_size, kv_size, kv_size), dim=-1)
    q = q.view(B, T, n_head, head_size).transpose(1, 2)
    k = k.view(B, T, n_query_groups, head_size).transpose(1, 2)
    v = v.view(B, T, n_query_groups, head_size).transpose(1, 2)
    if rope_n_elem == head_size:
        q = apply_rope(q, cos, sin)
        k = apply_rope(k, cos, sin)
    else:
        q = torch.cat((apply_rope(q[..., :rope_n_elem], cos, sin), q[..., rope_n_elem:]), dim=-1)
        k = torch.cat((apply_rope(k[..., :rope_n_elem], cos, sin), k[..., rope_n_elem:]), dim=-1)
    return q, k, v


def swiglu(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """LLaMA MLP gate: silu(a) * b."""
    return F.silu(a) * b


class RMSNorm(nn.Module):
    """RMSNorm; ``add_unit_offset`` (Gemma) scales by ``1 + weight`` with the weight initialised to
    zero, so the stored parameter is the deviation from identity."""

    def __init__(self, size: int, dim: int = -1, eps: float = 1e-6, add_unit_offset: bool = False):
        super().__init__()
        self.add_unit_offset = add_unit_offset
        self.weight = nn.Parameter(torch.zeros(size) if add_unit_offset else torch.ones(size))
        self.eps = eps
        self.dim = dim

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        w = self.weight + 1.0 if self.add_unit_offset else self.weight
        return F.rms_norm(x, (x.shape[-1],), w, self.eps)

    def reset_parameters(self) -> None:
        (nn.init.zeros_ if self.add_unit_offset else nn.init.ones_)(self.weight)


def _norm(config: Config, size: int) -> nn.Module:
    if config.norm_class_name == "RMSNorm":
        return RMSNorm(size, eps=config.norm_eps, add_unit_offset=config.norm_unit_offset)
    return nn.LayerNorm(size, eps=config.norm_eps)


class KVCache(nn.Module):
    """Static key/value cache (LitGPT ``KVCache``): [B, n_query_groups, max_seq, head_size] buffers
    updated in place at ``input_pos``.  Static storage keeps the decode step's addresses fixed, so
    a compiled decode step is a cache hit every token and can be replayed as one hipGraph.

    ``dtype=torch.float8_e4m3fn`` keeps the cache as unscaled, saturating OCP e4m3 in ``uint8``
    buffers (the stored-fp8 convention of ``transforms/fp8_inference.py``): half the bytes per token.
    Writes clamp to +-448 before the cast (torch's cast alone turns larger magnitudes into NaN, the
    kernels saturate); reads dequantise exactly to the dtype of the incoming k / v.

    ``scale="row"`` (e4m3 only) adds one power-of-two scale per (token, kv head) row, the format of
    ``ops/kv8.py``: the buffers ``k_scale`` / ``v_scale`` (uint8 ``[B, n_query_groups, max_seq, 1]``,
    ``e + 127``, initialised to 127) hold the rows' exponents and the bytes hold ``x * 2^-e``, so the e4m3
    rounding error is the same relative 2^-4 at every magnitude from 2^-24 to 57344 and no calibration is
    needed.  ``scale=None`` is the unscaled cache.

    ``input_pos`` is the shared 1-D ``[T]`` (every sequence writes rows ``input_pos``), or int64 ``[B, T]`` for
    a ragged batch: token (b, t) writes row ``input_pos[b, t]`` of sequence b, in every buffer of the format."""

    def __init__(self, k_shape, v_shape, device=None, dtype=None, scale: Optional[str] = None):
        super().__init__()
        if scale not in (None, "row"):
            raise ValueError(f"KV cache: scale must be None or 'row', got {scale!r}")
        if scale is not None and dtype != torch.float8_e4m3fn:
            raise ValueError(f"KV cache: scale={scale!r} needs dtype=torch.float8_e4m3fn, got {dtype}")
        self.scale = scale
        if dtype == torch.float8_e4m3fn:
            dtype = torch.uint8
        elif dtype is not None and dtype.is_floating_point and dtype.itemsize == 1:
            raise ValueError(f"KV cache: the only 8-bit float cache is torch.float8_e4m3fn, got {dtype}")
        self.register_buffer("k", torch.zeros(k_shape, device=device, dtype=dtype), persistent=False)
        self.register_buffer("v", torch.zeros(v_shape, device=device, dtype=dtype), persistent=False)
        if scale is not None:
            for name, shape in (("k_scale", k_shape), ("v_scale", v_shape)):
                self.register_buffer(name, torch.full((*shape[:-1], 1), 127, device=device, dtype=torch.uint8),
                                     persistent=False)

    def forward(self, input_pos: torch.Tensor, k: torch.Tensor, v: torch.Tensor):
        if input_pos.dim() == 2:  # per-sequence positions: one O(tokens) ``scatter_`` along the key dim per buffer
            def put(cache, src):  # (LitGPT's spelling of the batched write)
                return cache.scatter_(2, input_pos[:, None, :, None].expand_as(src), src)
        else:
            def put(cache, src):
                return cache.index_copy_(2, input_pos, src)

        if self.scale is not None:
            k8, ks = kv8_quantise_rows(k)
            v8, vs = kv8_quantise_rows(v)
            k_all, v_all = put(self.k, k8), put(self.v, v8)
            ks_all, vs_all = put(self.k_scale, ks), put(self.v_scale, vs)
            return kv8_dequantise_rows(k_all, ks_all, k.dtype), kv8_dequantise_rows(v_all, vs_all, v.dtype)
        if self.k.dtype == torch.uint8:
            f8 = torch.float8_e4m3fn
            k8 = k.clamp(-448.0, 448.0).to(f8).view(torch.uint8)
            v8 = v.clamp(-448.0, 448.0).to(f8).view(torch.uint8)
            k_all, v_all = put(self.k, k8), put(self.v, v8)
            return k_all.view(f8).to(k.dtype), v_all.view(f8).to(v.dtype)
        return put(self.k, k.to(self.k.dtype)), put(self.v, v.to(self.v.dtype))

    def reset_parameters(self) -> None:
        torch.nn.init.zeros_(self.k)
        torch.nn.init.zeros_(self.v)
        if self.scale is not None:
            torch.nn.init.constant_(self.k_scale, 127)
            torch.nn.init.constant_(self.v_scale, 127)


class PagedKVCache(nn.Module):
    """Paged key/value cache (``ops/kv_pages.py``): pools ``[n_query_groups, num_pages * page_size + 1, head_size]``
    whose rows are handed out in pages through the model's block table; the last row is the sink for tokens without
    a page.  ``dtype`` and ``scale`` as :class:`KVCache` has them; the scale pools are
    ``[n_query_groups, num_pages * page_size + 1, 1]``.

    ``forward(slots, table, k, v)`` writes token (b, t) at pool row ``slots[b, t]`` and returns every sequence's
    logical cache ``[B, n_query_groups, max_pages * page_size, head_size]``, dequantised as ``KVCache.forward``
    does."""

    def __init__(self, n_query_groups: int, head_size: int, page_size: int, num_pages: int, device=None, dtype=None,
                 scale: Optional[str] = None):
        super().__init__()
        if scale not in (None, "row"):
            raise ValueError(f"KV cache: scale must be None or 'row', got {scale!r}")
        if scale is not None and dtype != torch.float8_e4m3fn:
            raise ValueError(f"KV cache: scale={scale!r} needs dtype=torch.float8_e4m3fn, got {dtype}")
        self.scale = scale
        self.page_size = check_page_size(page_size)
        self.num_pages = num_pages
        if dtype == torch.float8_e4m3fn:
            dtype = torch.uint8
        elif dtype is not None and dtype.is_floating_point and dtype.itemsize == 1:
            raise ValueError(f"KV cache: the only 8-bit float cache is torch.float8_e4m3fn, got {dtype}")
        rows = num_pages * page_size + 1
        self.register_buffer("k", torch.zeros((n_query_groups, rows, head_size), device=device, dtype=dtype),
                             persistent=False)
        self.register_buffer("v", torch.zeros((n_query_groups, rows, head_size), device=device, dtype=dtype),
                             persistent=False)
        if scale is not None:
            for name in ("k_scale", "v_scale"):
                self.register_buffer(name, torch.full((n_query_groups, rows, 1), 127, device=device, dtype=torch.uint8),
                                     persistent=False)

    def forward(self, slots: torch.Tensor, table: torch.Tensor, k: torch.Tensor, v: torch.Tensor):
        B, H, T, _ = k.shape
        flat = slots.reshape(-1)

        def put(pool, src):  # [B, H, T, D] laid out as [H, B * T, D], one row per token
            return pool.index_copy_(1, flat, src.permute(1, 0, 2, 3).reshape(H, B * T, src.shape[-1]))

        def get(pool):
            return kv_paged_gather(pool, table, self.page_size)

        if self.scale is not None:
            k8, ks = kv8_quantise_rows(k)
            v8, vs = kv8_quantise_rows(v)
            k_all, v_all = put(self.k, k8), put(self.v, v8)
            ks_all, vs_all = put(self.k_scale, ks), put(self.v_scale, vs)
            return (kv8_dequantise_rows(get(k_all), get(ks_all), k.dtype),
                    kv8_dequantise_rows(get(v_all), get(vs_all), v.dtype))
        if self.k.dtype == torch.uint8:
            f8 = torch.float8_e4m3fn
            k8 = k.clamp(-448.0, 448.0).to(f8).view(torch.uint8)
            v8 = v.clamp(-448.0, 448.0).to(f8).view(torch.uint8)
            k_all, v_all = put(self.k, k8), put(self.v, v8)
            return get(k_all).view(f8).to(k.dtype), get(v_all).view(f8).to(v.dtype)
        return get(put(self.k, k.to(self.k.dtype))), get(put(self.v, v.to(self.v.dtype)))

    def reset_parameters(self) -> None:
        torch.nn.init.zeros_(self.k)
        torch.nn.init.zeros_(self.v)
        if self.scale is not None:
            torch.nn.init.constant_(self.k_scale, 127)
            torch.nn.init.constant_(self.v_scale, 127)

    def nbytes(self) -> int:
        return sum(b.numel() * b.element_size() for b in self.buffers())


class CausalSelfAttention(nn.Module):
    def __init__(self, config: Config):
        super().__init__()
        self.attn = nn.Linear(config.n_embd, config.qkv_size, bias=config.bias)
        self.proj = nn.Linear(config.n_head * config.head_size, config.n_embd, bias=config.bias)
        self.config = config
        self.kv_cache: Optional[KVCache] = None

    def forward(self, x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, mask: Optional[torch.Tensor] = None,
                input_pos: Optional[torch.Tensor] = None, pages=None) -> torch.Tensor:
        B, T, C = x.shape
        c = self.config
        qkv = self.attn(x)
        q, k, v = qkv_split_rope(qkv, cos, sin, c.n_head, c.n_query_groups, c.head_size, c.rope_n_elem)
        if pages is not None:  # a paged cache: (slots [B, T], the block table), computed once per step by GPT.forward
            k, v = self.kv_cache(pages[0], pages[1], k, v)
            y = F.scaled_dot_product_attention(q, k, v, attn_mask=mask, enable_gqa=c.n_query_groups != c.n_head)
        elif input_pos is not None:
            if self.kv_cache is None:
                raise TypeError("call model.set_kv_cache(...) before passing input_pos")
            k, v = self.kv_cache(input_pos, k, v)
            y = F.scaled_dot_product_attention(q, k, v, attn_mask=mask, enable_gqa=c.n_query_groups != c.n_head)
        elif mask is not None:  # a windowed layer over more tokens than its window: the band mask
            y = F.scaled_dot_product_attention(q, k, v, attn_mask=mask, enable_gqa=c.n_query_groups != c.n_head)
        else:
            y = F.scaled_dot_product_attention(q, k, v, is_causal=True, enable_gqa=c.n_query_groups != c.n_head)
        y = y.transpose(1, 2).reshape(B, T, c.n_head * c.head_size)
        return self.proj(y)


class LLaMAMLP(nn.Module):
    def __init__(self, config: Config):
        super().__init__()
        self.fc_1 = nn.Linear(config.n_embd, config.intermediate_size, bias=config.bias)
        self.fc_2 = nn.Linear(config.n_embd, config.intermediate_size, bias=config.bias)
        self.proj = nn.Linear(config.intermediate_size, config.n_embd, bias=config.bias)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        x_fc_1 = self.fc_1(x)
        x_fc_2 = self.fc_2(x)
        return self.proj(swiglu(x_fc_1, x_fc_2))


def geglu(a: torch.Tensor, b: torch.Tensor, approximate: str = "tanh") -> torch.Tensor:
    """Gemma MLP gate: gelu(a) * b."""
    return F.gelu(a, approximate=approximate) * b


class GemmaMLP(nn.Module):
    """LitGPT ``GemmaMLP`` (the reference benchmarks it, thunder/benchmarks/targets.py:578): the
    LLaMA MLP layout with a GeGLU gate."""

    def __init__(self, config: Config):
        super().__init__()
        self.fc_1 = nn.Linear(config.n_embd, config.intermediate_size, bias=config.bias)
        self.fc_2 = nn.Linear(config.n_embd, config.intermediate_size, bias=config.bias)
        self.proj = nn.Linear(config.intermediate_size, config.n_embd, bias=config.bias)
        self.config = config

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self.proj(geglu(self.fc_1(x), self.fc_2(x), self.config.gelu_approximate))


class GptNeoxMLP(nn.Module):
    def __init__(self, config: Config):
        super().__init__()
        self.fc = nn.Linear(config.n_embd, config.intermediate_size, bias=config.bias)
        self.proj = nn.Linear(config.intermediate_size, config.n_embd, bias=config.bias)
        self.config = config

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        x = self.fc(x)
        x = F.gelu(x, approximate=self.config.gelu_approximate)
        return self.proj(x)


class LLaMAMoE(nn.Module):
    """Sparse MoE MLP (litgpt ``LLaMAMoE``): softmax top-k router, tokens sorted by expert and run
    through *grouped* GEMMs (``torch._grouped_mm`` -> the K10 HIP kernel on MI355X), combined with
    the routing weights.  Expert weights are stored [E, out, in] like ``nn.Linear``."""

    def __init__(self, config: Config):
        super().__init__()
        E, D, I = config.n_expert, config.n_embd, config.intermediate_size
        self.gate = nn.Linear(D, E, bias=False)
        self.fc_1 = nn.Parameter(torch.empty(E, I, D))
        self.fc_2 = nn.Parameter(torch.empty(E, I, D))
        self.proj = nn.Parameter(torch.empty(E, D, I))
        self.config = config
        self.reset_parameters()

    def reset_parameters(self, std: float = 0.02) -> None:
        for w in (self.fc_1, self.fc_2, self.proj):
            nn.init.normal_(w, std=std)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        B, T, D = x.shape
        E, k = self.config.n_expert, self.config.n_expert_per_token
        xf = x.reshape(-1, D)
        probs = torch.softmax(self.gate(xf).float(), dim=-1)
        weights, experts = torch.topk(probs, k, dim=-1)                       # [N, k]
        weights = (weights / weights.sum(-1, keepdim=True)).to(x.dtype)
        flat_e = experts.reshape(-1)                                          # [N*k]
        order = torch.argsort(flat_e, stable=True)
        token = torch.div(order, k, rounding_mode="floor")
        counts = torch.nn.functional.one_hot(flat_e, E).sum(0)
        offs = torch.cumsum(counts, 0).to(torch.int32)
        xs = xf[token]                                                        # [N*k, D] sorted by expert
        a = torch._grouped_mm(xs, self.fc_1.transpose(1, 2), offs)
        b = torch._grouped_mm(xs, self.fc_2.transpose(1, 2), offs)
        h = swiglu(a, b)
        ys = torch._grouped_mm(h, self.proj.transpose(1, 2), offs)            # [N*k, D]
        ys = ys * weights.reshape(-1)[order].unsqueeze(-1)
        out = torch.zeros_like(xf).index_add(0, token, ys)
        return out.reshape(B, T, D)


class Block(nn.Module):
    def __init__(self, config: Config, block_idx: int = 0):
        super().__init__()
        self.sliding_window = config.layer_window(block_idx)  # None: the layer attends every earlier key
        self.norm_1 = _norm(config, config.n_embd)
        self.attn = CausalSelfAttention(config)
        self.norm_2 = None if config.shared_attention_norm else _norm(config, config.n_embd)
        if config.mlp_class_name == "LLaMAMLP":
            self.mlp = LLaMAMLP(config)
        elif config.mlp_class_name == "LLaMAMoE":
            self.mlp = LLaMAMoE(config)
        elif config.mlp_class_name == "GemmaMLP":
            self.mlp = GemmaMLP(config)
        else:
            self.mlp = GptNeoxMLP(config)
        self.config = config

    def forward(self, x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, mask: Optional[torch.Tensor] = None,
                input_pos: Optional[torch.Tensor] = None, pages=None) -> torch.Tensor:
        x_normed = self.norm_1(x)
        h = self.attn(x_normed, cos, sin, mask, input_pos) if pages is None else \
            self.attn(x_normed, cos, sin, mask, input_pos, pages)
        if self.config.parallel_residual:
            n2 = x_normed if self.norm_2 is None else self.norm_2(x)
            return self.mlp(n2) + h + x
        x = h + x
        return self.mlp(self.norm_2(x)) + x


class GPT(nn.Module):
    def __init__(self, config: Config):
        super().__init__()
        self.config = config
        self.activation_checkpointing = False  # per-Block torch.utils.checkpoint in training forwards
        self.lm_head = nn.Linear(config.n_embd, config.padded_vocab_size, bias=config.lm_head_bias if hasattr(config, "lm_head_bias") else False)
        self.transformer = nn.ModuleDict(
            dict(
                wte=nn.Embedding(config.padded_vocab_size, config.n_embd),
                h=nn.ModuleList(Block(config, i) for i in range(config.n_layer)),
                ln_f=_norm(config, config.n_embd),
            )
        )
        if config.tie_embeddings:
            self.lm_head.weight = self.transformer.wte.weight
        self.max_seq_length = config.block_size
        self.register_buffer("cos", torch.empty(0), persistent=False)
        self.register_buffer("sin", torch.empty(0), persistent=False)
        self.mask_cache: Optional[torch.Tensor] = None
        self.window_mask_cache: Optional[torch.Tensor] = None  # the band mask of the windowed layers (1-D input_pos)
        self.kv_pages: Optional[PageTable] = None  # the allocator of a paged KV cache (set_kv_cache(page_size=...))
        self.page_table: Optional[torch.Tensor] = None  # its device block table, shared by all layers
        self._rope_seq = 0

    def set_rope_cache(self, seq_len: int, device=None) -> None:
        cos, sin = build_rope_cache(seq_len, self.config.rope_n_elem, device=device, base=self.config.rope_base,
                                    condense_ratio=self.config.rope_condense_ratio)
        self.cos = cos
        self.sin = sin
        self._rope_seq = seq_len

    def set_kv_cache(self, batch_size: int, max_seq_length: Optional[int] = None, device=None,
                     dtype: Optional[torch.dtype] = None, scale: Optional[str] = None,
                     page_size: Optional[int] = None, num_pages: Optional[int] = None) -> None:
        """Allocates a static KV cache in every block and the causal mask for incremental decoding.
        ``dtype=torch.float8_e4m3fn`` stores the caches as unscaled, saturating e4m3 in ``uint8`` buffers
        (see :class:`KVCache`); any other 8-bit float dtype raises ``ValueError``.  ``scale="row"`` with
        that dtype adds one power-of-two scale byte per (token, kv head) row; with any other dtype it
        raises ``ValueError``.

        ``page_size`` (a power of two >= 16, else ``ValueError``) makes the cache a paged one (``ops/kv_pages.py``):
        every block gets a :class:`PagedKVCache` of ``num_pages`` pages (default ``batch_size * max_pages``, what
        the static cache would hold) in the same ``dtype`` / ``scale`` formats, the model gets the allocator
        ``self.kv_pages`` with ``max_pages = ceil(max_seq_length / page_size)`` table entries per sequence, and
        ``self.max_seq_length`` becomes ``max_pages * page_size``.  Such a model takes the 2-D ``input_pos`` only."""
        if scale is not None and dtype != torch.float8_e4m3fn:
            raise ValueError(f"set_kv_cache: scale={scale!r} needs dtype=torch.float8_e4m3fn, got {dtype}")
        c = self.config
        max_seq_length = max_seq_length or c.block_size
        dtype = dtype or self.lm_head.weight.dtype
        device = device or self.lm_head.weight.device
        if page_size is None:
            if num_pages is not None:
                raise ValueError("set_kv_cache: num_pages needs a page_size")
            self.kv_pages = self.page_table = None
        else:
            check_page_size(page_size)
            max_pages = -(-max_seq_length // page_size)
            num_pages = batch_size * max_pages if num_pages is None else num_pages
            self.kv_pages = PageTable(batch_size, max_pages, page_size, num_pages, device=device)
            self.page_table = self.kv_pages.table
            for block in self.transformer.h:
                ac = getattr(block.attn, "config", c)
                block.attn.kv_cache = PagedKVCache(ac.n_query_groups, ac.head_size, page_size, num_pages, device=device,
                                                   dtype=dtype, scale=scale)
            max_seq_length = max_pages * page_size
            if self.cos.numel() == 0 or self.cos.shape[0] < max_seq_length:
                self.set_rope_cache(max_seq_length, device=device)
            self.mask_cache = self.window_mask_cache = None
            self.max_seq_length = max_seq_length
            return
        for block in self.transformer.h:
            # sized from the attention module's own config: under head-parallel TP it holds only
            # this rank's kv groups (distributed/tensor_parallel swaps in a localized config)
            ac = getattr(block.attn, "config", c)
            shape = (batch_size, ac.n_query_groups, max_seq_length, ac.head_size)
            block.attn.kv_cache = KVCache(shape, shape, device=device, dtype=dtype, scale=scale)
        if self.cos.numel() == 0 or self.cos.shape[0] < max_seq_length:
            self.set_rope_cache(max_seq_length, device=device)
        ones = torch.ones((max_seq_length, max_seq_length), device=device, dtype=torch.bool)
        self.mask_cache = torch.tril(ones).unsqueeze(0).unsqueeze(0)
        W = c.sliding_window_size
        self.window_mask_cache = None
        if W is not None and W < max_seq_length:  # row p: keys p - W + 1 .. p
            self.window_mask_cache = torch.triu(torch.tril(ones), diagonal=1 - W).unsqueeze(0).unsqueeze(0)
        self.max_seq_length = max_seq_length

    def clear_kv_cache(self) -> None:
        for block in self.transformer.h:
            block.attn.kv_cache = None
        self.mask_cache = self.window_mask_cache = None
        self.kv_pages = self.page_table = None

    def forward(self, idx: torch.Tensor, input_pos: Optional[torch.Tensor] = None) -> torch.Tensor:
        T = idx.size(1)
        if self.cos.numel() == 0 or self.cos.shape[0] < T:
            raise RuntimeError("call model.set_rope_cache(seq_len, device) before forward")
        pages = None
        # the windowed layers' mask, next to the global one: only where the window hides a key some row could see (a
        # cache of more than W positions, more than W tokens without a cache); else every layer runs the global code
        W = self.config.sliding_window_size
        wmask = None
        if input_pos is not None and self.kv_pages is not None:  # a paged cache: slots and mask once per step
            if input_pos.dim() != 2:
                raise TypeError("a paged KV cache takes the 2-D input_pos [B, T] (one position per token) only, "
                                f"got {input_pos.dim()}-D")
            B = idx.size(0)
            flat = input_pos.reshape(-1)
            cos = self.cos.index_select(0, flat).view(B, T, -1)
            sin = self.sin.index_select(0, flat).view(B, T, -1)
            pt = self.kv_pages
            table = self.page_table
            slots = kv_page_slots(table, input_pos, pt.page_size, pt.num_pages * pt.page_size)
            mask = kv_paged_mask(input_pos, table, pt.page_size, pt.num_pages)
            if W is not None and W < self.max_seq_length:
                wmask = kv_paged_window_mask(input_pos, table, pt.page_size, pt.num_pages, W)
            pages = (slots, table)
        elif input_pos is not None and input_pos.dim() == 2:  # a ragged batch: one position per (sequence, token)
            B = idx.size(0)
            flat = input_pos.reshape(-1)
            cos = self.cos.index_select(0, flat).view(B, T, -1)
            sin = self.sin.index_select(0, flat).view(B, T, -1)
            mask = kv_position_mask(input_pos, self.max_seq_length)
            if W is not None and W < self.max_seq_length:
                wmask = kv_window_mask(input_pos, self.max_seq_length, W)
        elif input_pos is not None:  # incremental decoding against the KV cache
            cos = self.cos.index_select(0, input_pos)
            sin = self.sin.index_select(0, input_pos)
            mask = self.mask_cache.index_select(2, input_pos)
            if self.window_mask_cache is not None:
                wmask = self.window_mask_cache.index_select(2, input_pos)
        else:
            cos = self.cos[:T]
            sin = self.sin[:T]
            mask = None
            if W is not None and T > W:
                ones = torch.ones((T, T), device=idx.device, dtype=torch.bool)
                wmask = torch.triu(torch.tril(ones), diagonal=1 - W).unsqueeze(0).unsqueeze(0)
        x = self.transformer.wte(idx)
        if self.config.scale_embeddings:
            x = x * math.sqrt(self.config.n_embd)
        global_mask = mask
        for block in self.transformer.h:
            mask = wmask if wmask is not None and block.sliding_window is not None else global_mask
            if self.activation_checkpointing and input_pos is None:
                # recompute the block's intermediates in the backward (LitGPT / benchmark_litgpt
                # ``--checkpoint_activations``); traced as ltorch.checkpoint
                x = torch.utils.checkpoint.checkpoint(block, x, cos, sin, mask, None, use_reentrant=False)
            elif pages is not None:
                x = block(x, cos, sin, mask, input_pos, pages)
            else:
                x = block(x, cos, sin, mask, input_pos)
        x = self.transformer.ln_f(x)
        return self.lm_head(x)

    @classmethod
    def from_name(cls, name: str, **kwargs) -> "GPT":
        return cls(Config.from_name(name, **kwargs))


def init_weights(model: GPT, std: float = 0.02) -> None:
    """Random init (synthetic benchmark weights; no checkpoints are available offline).

    Every parameter and buffer is initialised — a model materialised with ``to_empty`` holds
    uninitialised memory otherwise: Linear/Embedding weights N(0, std), biases zero, and every other
    module with a ``reset_parameters`` (RMSNorm/LayerNorm weights to one, KV caches to zero, MoE
    routers) through it."""
    for m in model.modules():
        if isinstance(m, nn.Linear):
            nn.init.normal_(m.weight, mean=0.0, std=std)
            if m.bias is not None:
                nn.init.zeros_(m.bias)
        elif isinstance(m, nn.Embedding):
            nn.init.normal_(m.weight, mean=0.0, std=std)
        elif isinstance(m, nn.LayerNorm):
            if m.weight is not None:
                nn.init.ones_(m.weight)
            if m.bias is not None:
                nn.init.zeros_(m.bias)
        elif hasattr(m, "reset_parameters"):
            m.reset_parameters()


def flops_per_token(config: Config, seq_len: int, training: bool = True) -> float:
    """Model FLOPs per token (matmuls + attention), as used for MFU/TFLOP/s reporting."""
    c = config
    n_params_linear = c.n_layer * (c.n_embd * c.qkv_size + c.n_head * c.head_size * c.n_embd
                                   + 3 * c.n_embd * c.intermediate_size) + c.n_embd * c.padded_vocab_size
    attn = c.n_layer * 2 * 2 * seq_len * c.n_head * c.head_size / 2  # causal: half of QK^T and PV
    fwd = 2 * n_params_linear + attn
    return fwd * (3 if training else 1)


@torch.no_grad()
def generate(model, prompt: torch.Tensor, max_new_tokens: int, *, forward=None, temperature: float = 0.0,
             top_k: Optional[int] = None, top_p: Optional[float] = None, eos_id: Optional[int] = None,
             prompt_lengths: Optional[torch.Tensor] = None, pad_id: int = 0,
             prefill_chunk: Optional[int] = None) -> torch.Tensor:
    """Autoregressive generation with the static KV cache (LitGPT ``generate``).

    ``forward`` is the callable used for every step (default: ``model``; pass ``thunder.jit(model)``).
    Prefill runs the prompt with ``input_pos = arange(T)``; every decode step feeds one token with
    the *same* ``input_pos`` tensor advanced in place, so a compiled decode step keeps its input
    addresses (hipGraph-replayable) and is a cache hit after the first token.
    Greedy when ``temperature == 0``.  With ``temperature > 0`` every token is drawn by
    ``ops.sampling.sample_last``: temperature, then ``top_k`` (ties at the k-th logit all stay drawable),
    then the nucleus ``top_p``, then one draw from the softmax of what is left.  The draws come from the
    project's Philox counter stream (``core.rng``), not from ATen's generator: ``torch.manual_seed(s)``
    before the call reproduces the tokens.  Returns ``[B, T + max_new_tokens]`` token ids.

    ``prompt_lengths`` (int64 ``[B]``, ``1 <= len_b <= T``) makes the batch ragged: ``prompt`` is right-padded
    and row b holds ``len_b`` real tokens; see :func:`_generate_ragged`.  ``pad_id`` is only used there.

    ``prefill_chunk`` (a positive int, else ``ValueError``) runs the prompt in slices of at most that many columns,
    each one ``forward(prompt[:, c0:c1], pos2d)`` at the int64 ``[B, c1 - c0]`` positions ``arange(c0, c1)``, on every
    route (plain, ragged, paged): a prompt longer than one forward's activations allow still prefills, and every
    chunk attends the cache by positions (``hip_prefill_attn_*`` under the HIP executor).  A value ``>= T`` is one
    chunk: the whole prompt by positions.  ``None`` prefills as before; the decode loop is the same either way.
    """
    from ..ops.sampling import argmax_last, sample_last

    if prefill_chunk is not None and (isinstance(prefill_chunk, bool) or not isinstance(prefill_chunk, int)
                                      or prefill_chunk < 1):
        raise ValueError(f"generate: prefill_chunk must be a positive int or None, got {prefill_chunk!r}")
    forward = forward or model
    if prompt_lengths is None and getattr(model, "kv_pages", None) is not None:  # a paged cache: always the ragged route
        prompt_lengths = torch.full((prompt.shape[0],), prompt.shape[1], device=prompt.device, dtype=torch.int64)
    if prompt_lengths is not None:
        return _generate_ragged(model, prompt, max_new_tokens, forward, temperature, top_k, top_p, eos_id,
                                prompt_lengths, pad_id, prefill_chunk)
    B, T = prompt.shape
    if model.transformer.h[0].attn.kv_cache is None:
        raise RuntimeError("call model.set_kv_cache(batch_size, max_seq_length) first")
    device = prompt.device
    if prefill_chunk is None:
        input_pos = torch.arange(T, device=device)
        logits = forward(prompt, input_pos)
    else:
        logits = _chunked_prefill(forward, prompt, prefill_chunk)[:, None]
    out = [prompt]
    pos = torch.tensor([T], device=device, dtype=torch.int64)
    for i in range(max_new_tokens):
        last = logits[:, -1]
        if temperature > 0:
            nxt = sample_last(last, temperature, top_k, top_p, keepdim=True)
        else:
            nxt = argmax_last(last, keepdim=True)
        out.append(nxt)
        if eos_id is not None and bool((nxt == eos_id).all()):
            break
        if i + 1 < max_new_tokens:
            logits = forward(nxt, pos)
            pos.add_(1)
    return torch.cat(out, dim=1)


def _chunked_prefill(forward, prompt, chunk: int, lengths: Optional[torch.Tensor] = None,
                     before_chunk=None) -> torch.Tensor:
    """The prompt ``[B, T]`` through ``forward`` in slices of at most ``chunk`` columns at the 2-D positions
    ``arange(c0, c1)``.  Returns the logits ``[B, V]`` every sequence's first new token is drawn from: those of column
    ``lengths[b] - 1`` (``T - 1`` without ``lengths``), picked out of the chunk that holds it; no other logits are kept.
    ``before_chunk(c0, c1)`` runs ahead of every slice (a paged cache under a sliding window moves its pages there)."""
    B, T = prompt.shape
    device = prompt.device
    rows = torch.arange(B, device=device)
    last = None
    for c0 in range(0, T, chunk):
        c1 = min(T, c0 + chunk)
        if before_chunk is not None:
            before_chunk(c0, c1)
        pos2d = torch.arange(c0, c1, device=device, dtype=torch.int64).expand(B, c1 - c0).contiguous()
        logits = forward(prompt[:, c0:c1], pos2d)
        if lengths is None:
            if c1 == T:
                last = logits[:, -1]
            continue
        col = lengths - 1 - c0  # the column of this chunk that holds a sequence's last prompt token, if any does
        here = (col >= 0) & (col < c1 - c0)
        picked = logits[rows, col.clamp(0, c1 - c0 - 1)]
        last = picked if last is None else torch.where(here[:, None], picked, last)
    return last


def _generate_ragged(model, prompt, max_new_tokens, forward, temperature, top_k, top_p, eos_id, prompt_lengths,
                     pad_id, prefill_chunk=None) -> torch.Tensor:
    """``generate`` for a right-padded ``[B, Tmax]`` prompt whose row b holds ``prompt_lengths[b]`` tokens.

    Prefill runs the padded prompt at the shared ``arange(Tmax)``: a pad token writes K/V rows at positions
    ``>= len_b``, and each of those is overwritten by the sequence's own token before any row can attend to it,
    because a row at position p sees keys ``<= p`` only.  The first token of row b comes from
    ``logits[b, len_b - 1]``.  Every decode step feeds ``[B, 1]`` tokens with one int64 ``[B, 1]`` position
    tensor that starts at ``prompt_lengths`` and is advanced in place (fixed addresses: a hipGraph replays).
    A sequence that has produced ``eos_id`` keeps riding in the batch, its later tokens are ``pad_id``; the
    loop ends when all are done.

    On a paged cache (``set_kv_cache(page_size=...)``) the prefill runs at ``arange(Tmax)`` expanded to ``[B, Tmax]``
    after ``model.kv_pages.reserve(prompt_lengths)``, and before every decode step the sequences that are not
    finished get room for one more token, from host-side counters; a finished sequence receives no further page.

    With ``prefill_chunk`` the prefill is ``_chunked_prefill`` on either cache: slices of the padded prompt at 2-D
    positions, after the prompts' pages are reserved; a pad token's K/V row is overwritten as above.

    When every layer of the model has one sliding window ``W`` (``Config.uniform_window``), a paged cache gives up the
    pages no later row can see: before every ``reserve`` the table is trimmed to ``len_b - W + 1`` (floored at 0), with
    ``len_b`` the position the sequence's next row sits at, per decode step and per prefill chunk, and a chunked prefill
    reserves its pages chunk by chunk.  A sequence then holds about ``W / page_size`` pages however long it grows.  A
    model with any global layer never trims.

    Returns ``[B, Tmax + max_new_tokens]``: row b is its prompt, the new tokens
    from column ``len_b`` on, then ``pad_id``."""
    from ..ops.sampling import argmax_last, sample_last

    B, T = prompt.shape
    cache = model.transformer.h[0].attn.kv_cache
    if cache is None:
        raise RuntimeError("call model.set_kv_cache(batch_size, max_seq_length) first")
    device = prompt.device
    lengths = torch.as_tensor(prompt_lengths, device=device).to(torch.int64).reshape(-1)
    if lengths.numel() != B:
        raise ValueError(f"generate: prompt_lengths has {lengths.numel()} entries for a batch of {B}")
    lo, hi = int(lengths.min()), int(lengths.max())
    if lo < 1 or hi > T:
        raise ValueError(f"generate: prompt_lengths must lie in [1, {T}], got {lo} .. {hi}")
    pages = getattr(model, "kv_pages", None)
    capacity = cache.k.shape[2] if pages is None else pages.capacity
    if hi + max_new_tokens > capacity:
        raise ValueError(f"generate: the longest prompt ({hi}) plus {max_new_tokens} new tokens exceeds the KV "
                         f"cache of {capacity} positions")
    out = torch.full((B, T + max_new_tokens), pad_id, device=device, dtype=prompt.dtype)
    cols = torch.arange(T, device=device)
    out[:, :T] = torch.where(cols[None, :] < lengths[:, None], prompt, torch.full_like(prompt, pad_id))
    if max_new_tokens <= 0:
        return out
    if pages is None:
        if prefill_chunk is None:
            logits = forward(prompt, torch.arange(T, device=device))
    else:
        # pages for the prompts; a pad token beyond its sequence's last page has no slot and falls to the sink row
        held = lengths.tolist()  # host-side counters from here on
        live = [True] * B
        trim = getattr(getattr(model, "config", None), "uniform_window", None)  # the window pages may fall out of
        pages.reset()  # a generation starts from an empty table, as it overwrites a static cache
        if trim is None or prefill_chunk is None:
            pages.reserve(held)
        if prefill_chunk is None:
            logits = forward(prompt, torch.arange(T, device=device).expand(B, T).contiguous())
    if prefill_chunk is None:
        last = logits[torch.arange(B, device=device), lengths - 1]
    elif pages is not None and trim is not None:
        def move_pages(c0, c1):  # the chunk's rows sit at c0 .. c1 - 1; a sequence that ended earlier waits at len_b
            pages.trim([max(0, min(c0, n) - trim + 1) for n in held])
            pages.reserve([min(c1, n) for n in held])

        last = _chunked_prefill(forward, prompt, prefill_chunk, lengths, move_pages)
    else:
        last = _chunked_prefill(forward, prompt, prefill_chunk, lengths)
    pos = lengths.clone().view(B, 1)  # where the next token of every sequence goes; advanced in place
    done = torch.zeros(B, 1, device=device, dtype=torch.bool)
    for i in range(max_new_tokens):
        if temperature > 0:
            nxt = sample_last(last, temperature, top_k, top_p, keepdim=True)
        else:
            nxt = argmax_last(last, keepdim=True)
        nxt = torch.where(done, torch.full_like(nxt, pad_id), nxt)
        out.scatter_(1, pos, nxt.to(out.dtype))
        if eos_id is not None:
            done = done | (nxt == eos_id)
            if bool(done.all()):
                break
            if pages is not None:
                live = [not d for d in done.view(-1).tolist()]
        if i + 1 < max_new_tokens:
            if pages is not None:  # room for this step's token; a finished sequence gets no further page
                if trim is not None:  # the step's row sits at position n and sees keys n - W + 1 .. n
                    pages.trim([max(0, n - trim + 1) for n in held])
                held = [n + 1 if alive else n for n, alive in zip(held, live)]
                pages.reserve(held)
            logits = forward(nxt, pos)
            last = logits[:, -1]
            pos.add_(1)
    return out
