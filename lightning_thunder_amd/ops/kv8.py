"""The two e4m3 KV cache formats in plain torch: unscaled, and one power-of-two scale per row.

``e4m3_bytes`` / ``e4m3_values`` (unscaled) and ``quantise_rows`` / ``dequantise_rows`` (scaled) are the
definition; the kernels (``csrc/rope.hip`` row kernel, ``csrc/decode_attention.hip``) equal them bit for
bit.  A scaled row ``x[..., :]`` is stored as ``D`` bytes of OCP
e4m3 (``float8_e4m3fn``) of ``x * 2^-e`` plus one byte ``e + 127`` (E8M0 style), where ``e`` is the
smallest exponent in [-15, 7] with ``amax * 2^-e <= 448``.  Multiplying by a power of two is exact, so the
only rounding is the e4m3 conversion, whose error is relative: the same 2^-4 at every magnitude from
2^-24 to 57344.  Larger values saturate; an all-zero row takes ``e = -15`` by the clamp.  With ``e`` in that
range every dequantised value is exact in bf16 and in fp16.

A row that holds a NaN is outside the bit-for-bit contract between this definition and the kernels:
``torch.amax`` propagates the NaN (its fp32 bits then give ``e = 7``), a kernel's maximum need not, so the
scale byte and the finite elements' bytes may differ.  Neither faults or writes outside the row.

Both functions are also ``torch.library`` custom ops (``lta::kv8_quantise_rows``,
``lta::kv8_dequantise_rows``), so a traced program holds each as one symbol.
"""
from __future__ import annotations

import torch

E4M3_MAX = 448.0
E_MIN, E_MAX = -15, 7
SCALE_BIAS = 127
_F8 = torch.float8_e4m3fn


def e4m3_bytes(x: torch.Tensor) -> torch.Tensor:
    """The stored form of an unscaled e4m3 value: saturate, round to nearest even, as uint8."""
    return x.clamp(-E4M3_MAX, E4M3_MAX).to(_F8).view(torch.uint8)


def e4m3_values(b: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """The values of e4m3 bytes in ``dtype`` (exact for bf16 / fp16 / fp32)."""
    return b.view(_F8).to(dtype)


def scale_caches_of(scales, caches) -> bool:
    """Every ``scales[i]`` holds the scale bytes of the byte cache ``caches[i]`` [B, H, S, D]: uint8
    [B, H, S, 1] on its device (any strides)."""
    return all(s is not None and s.dtype == torch.uint8 and s.device == c.device and s.dim() == 4
               and tuple(s.shape) == (*c.shape[:3], 1) for s, c in zip(scales, caches))


def pow2(n: torch.Tensor) -> torch.Tensor:
    """fp32 ``2^n`` for integer ``n`` in [-126, 127], built from bits (exact on every backend)."""
    return ((n.to(torch.int32) + 127) << 23).view(torch.float32)


def row_exponent(x: torch.Tensor) -> torch.Tensor:
    """int32 ``[..., 1]``: the smallest ``e`` in [-15, 7] with ``amax(|x|) * 2^-e <= 448 = 1.75 * 2^8``."""
    amax = x.abs().amax(-1, keepdim=True).float()
    bits = amax.view(torch.int32)
    ex = (bits >> 23) & 0xFF
    man = bits & 0x7FFFFF
    return (ex - 135 + (man > 0x600000).to(torch.int32)).clamp(E_MIN, E_MAX)


def quantise_rows(x: torch.Tensor):
    """``x [..., D]`` float -> ``(bytes uint8 [..., D], scales uint8 [..., 1])``."""
    e = row_exponent(x)
    return e4m3_bytes(x.float() * pow2(-e)), (e + SCALE_BIAS).to(torch.uint8)


def dequantise_rows(b: torch.Tensor, scales: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """``bytes * 2^(scales - 127)`` in ``dtype``; exact for bf16 / fp16 / fp32 with scales in [112, 134]."""
    return e4m3_values(b, dtype) * pow2(scales.to(torch.int32) - SCALE_BIAS).to(dtype)


@torch.library.custom_op("lta::kv8_quantise_rows", mutates_args=())
def kv8_quantise_rows(x: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    return quantise_rows(x)


@kv8_quantise_rows.register_fake
def _kv8_quantise_rows_fake(x):
    return (x.new_empty(x.shape, dtype=torch.uint8), x.new_empty((*x.shape[:-1], 1), dtype=torch.uint8))


@torch.library.custom_op("lta::kv8_dequantise_rows", mutates_args=())
def kv8_dequantise_rows(b: torch.Tensor, scales: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    return dequantise_rows(b, scales, dtype)


@kv8_dequantise_rows.register_fake
def _kv8_dequantise_rows_fake(b, scales, dtype):
    return b.new_empty(b.shape, dtype=dtype)
