"""Shared assertions of the kernel-against-fp64 batteries (test_decode_kernels.py, test_train_row_kernels.py,
test_attention_kernels.py, test_gemm_kernels.py, test_hipfuse_kernels.py), the mirror of the attention kernels' dropout hash, and the
guard / poison buffers that show a kernel writing outside its result or reading outside its operands.

Tolerance of every rounded output, per element:  ulp(T) * |ref64| + 8 * e32 + floor.
``ulp`` is the spacing of T at 1 (2^-8 bf16, 2^-10 fp16, 2^-23 fp32): the single rounding of the
output.  ``e32`` is the largest error of a plain torch fp32 evaluation of the same reference formula on
the same inputs; the kernels accumulate in fp32, and the factor 8 covers their fast exp and their
summation order.  ``floor`` is 1e-6, or with ``rel_floor`` 1e-6 * max |ref64| (outputs that are small
as a whole: Adam second moments, gradients under a mean); a reference that is zero everywhere then
asks for exact zeros (unless the caller's error model adds an ``extra`` term: that is then the tolerance), and the rounding term is at least half the subnormal spacing of T (fp16: 2^-25 =
3e-8; without it a correctly rounded fp16 value below 6e-5 fails ulp(T) |ref64|).
"""
import torch

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
ULP = {BF16: 2.0 ** -8, F16: 2.0 ** -10, F32: 2.0 ** -23}
HALF_SUBNORMAL = {BF16: 2.0 ** -134, F16: 2.0 ** -25, F32: 2.0 ** -150}  # half the spacing of T next to zero
E32_FACTOR = 8.0
ABS_FLOOR = 1e-6
_INT_VIEW = {BF16: torch.int16, F16: torch.int16, F32: torch.int32}

# (group, dtype) -> largest err / tol seen in this process
_WORST: dict = {}


def _dt_id(d):
    return str(d).replace("torch.", "")


def assert_within(out, ref64, ref32, dtype, group, what="", rel_floor=False, extra=None):
    """|out - ref64| <= ulp(T) |ref64| + 8 e32 + floor (+ ``extra``, a per-element term of the caller's
    error model) for every element; records the worst ratio."""
    assert out.shape == ref64.shape, (out.shape, ref64.shape)
    assert torch.isfinite(ref64).all(), f"{what}: reference is not finite"
    if out.numel() == 0:
        return
    if rel_floor and extra is None and not ref64.any():
        assert not out.double().abs().any(), f"{what}: the reference is zero everywhere, the output is not"
        print(f"[{group} {_dt_id(dtype)}] {what} exact zeros")
        return
    e32 = (ref32.double() - ref64).abs().max().item()
    floor = ABS_FLOOR * ref64.abs().max().item() if rel_floor else ABS_FLOOR
    rounding = ULP[dtype] * ref64.abs()
    if rel_floor:  # below its smallest normal T is spaced absolutely: a correctly rounded fp16 is off by up to 2^-25
        rounding = rounding.clamp(min=HALF_SUBNORMAL[dtype])
    tol = rounding + E32_FACTOR * e32 + floor
    if extra is not None:
        assert extra.shape == ref64.shape and (extra >= 0).all(), f"{what}: malformed extra tolerance term"
        tol = tol + extra.double()
    err = (out.double() - ref64).abs()
    assert not torch.isnan(err).any(), f"{what}: NaN in the kernel output"
    ratio = (err / tol).max().item()
    key = (group, _dt_id(dtype))
    _WORST[key] = max(_WORST.get(key, 0.0), ratio)
    off = (out != ref64.to(dtype)).sum().item()  # elements that are not the correctly rounded reference
    print(f"[{group} {_dt_id(dtype)}] {what} err/tol={ratio:.3f} max_err={err.max().item():.3e} e32={e32:.3e}"
          f" off_by_rounding={off}/{out.numel()} (worst so far {_WORST[key]:.3f})")
    assert ratio <= 1.0, f"{what}: err/tol = {ratio:.3f} (max err {err.max().item():.3e}, e32 {e32:.3e})"


M32 = 0xFFFFFFFF


def _fmix32(h):
    h = h & M32
    h = h ^ (h >> 16)
    h = (h * 0x85EBCA6B) & M32
    h = h ^ (h >> 13)
    h = (h * 0xC2B2AE35) & M32
    h = h ^ (h >> 16)
    return h


def keep_mask(seed, offset, B, H, T, S, p, device):
    """The attention kernels' dropout keep mask [B, H, T, S] (True = kept): a mirror of attention.h
    rng_head / rng_q / rng_k / rng_keep in int64 torch arithmetic."""
    lo, hi = seed & M32, (seed >> 32) & M32
    base = _fmix32(torch.tensor(lo ^ ((offset * 0x27D4EB2F) & M32), dtype=torch.int64, device=device)) ^ hi
    bh = torch.arange(B * H, dtype=torch.int64, device=device)
    head = _fmix32(((bh * 0x9E3779B9) & M32) ^ base)  # [BH]
    q = torch.arange(T, dtype=torch.int64, device=device)
    k = torch.arange(S, dtype=torch.int64, device=device)
    qterm = _fmix32(((q[None, :] * 0x61C88647) & M32) + head[:, None])  # [BH, T]
    kterm = _fmix32(((k * 0x7FEB352D) & M32) + 0x3C6EF372)  # [S]
    h = _fmix32(qterm[:, :, None] ^ kterm[None, None, :])
    p32 = float(torch.tensor(p, dtype=torch.float32))  # the kernels receive p as fp32
    thresh = min(int(p32 * 4294967296.0), 4294967295)
    return (h >= thresh).reshape(B, H, T, S)


def bits_equal(a, b):
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    it = _INT_VIEW[a.dtype]
    return torch.equal(a.contiguous().view(it), b.contiguous().view(it))


# ------------------------------------------------------------------------------------------------
# guards and poison: results as views of sentinel-filled buffers, operands as views of NaN-filled ones
# ------------------------------------------------------------------------------------------------
SENTINEL = 0x5A3C  # int16 pattern of every 16-bit word around a guarded result (a finite bf16, 1.3e16)


def guarded(shape, device, pads=None, dtype=BF16):
    """(buf, view): ``view`` is a 16-bit tensor of ``shape``, the leading corner of the int16 buffer ``buf``
    whose every word is SENTINEL.  ``pads`` are the extra elements per dim (default: 8 more rows and a
    pitch 64 elements longer on the last two dims, nothing on the leading ones)."""
    assert dtype in (BF16, F16)
    shape = tuple(shape)
    if pads is None:
        pads = (0,) * (len(shape) - 2) + (8, 64)
    assert len(pads) == len(shape)
    buf = torch.full(tuple(s + p for s, p in zip(shape, pads)), SENTINEL, dtype=torch.int16, device=device)
    return buf, buf.view(dtype)[tuple(slice(0, s) for s in shape)]


def assert_guard_intact(buf, shape, what=""):
    """Every word of ``buf`` (from :func:`guarded`) outside its leading ``shape`` corner is still SENTINEL."""
    rest = buf.clone()
    rest[tuple(slice(0, s) for s in shape)] = SENTINEL
    bad = rest != SENTINEL
    n = int(bad.sum().item())
    assert n == 0, (f"{what}: {n} words outside the {tuple(shape)} result were overwritten, the first at "
                    f"{tuple(int(i) for i in bad.nonzero()[0])}")


def nan_padded(t, pad_rows=8, pad_cols=8):
    """A view equal to ``t`` (floating point, >= 2-D) inside a NaN-filled buffer: ``pad_rows`` more rows and
    a pitch of the columns rounded up to 8 elements plus ``pad_cols`` on the last two dims (16-byte aligned
    rows for 16-bit types).  A kernel that consumes a padding column or a row past the end yields NaN."""
    assert t.dim() >= 2 and t.is_floating_point() and pad_cols % 8 == 0
    *lead, R, C = t.shape
    buf = torch.full((*lead, R + pad_rows, (C + 7) // 8 * 8 + pad_cols), float("nan"), dtype=t.dtype, device=t.device)
    view = buf[..., :R, :C]
    view.copy_(t)
    return view


def offset_by_one(t):
    """A contiguous copy of ``t`` that starts one element into its buffer: on the GPU its address is no
    multiple of 16 bytes."""
    buf = torch.full((t.numel() + 1,), float("nan"), dtype=t.dtype, device=t.device)
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and (t.device.type == "cpu" or view.data_ptr() % 16 != 0)
    return view


def odd_pitch(t):
    """A view equal to ``t`` (>= 2-D): the leading columns of a NaN-filled base one element wider, so the
    stride of the second-to-last dim is the column count plus one."""
    *lead, R, C = t.shape
    base = torch.full((*lead, R, C + 1), float("nan"), dtype=t.dtype, device=t.device)
    view = base[..., :C]
    view.copy_(t)
    return view


def assert_within_finite(out, ref64, ref32, dtype, group, what="", rel_floor=False, extra=None):
    """:func:`assert_within` for a reference with NaN or infinite elements: those must sit at the same
    positions of ``out`` (infinities with their sign), the finite remainder is held to the tolerance."""
    assert out.shape == ref64.shape, (out.shape, ref64.shape)
    nan, inf = torch.isnan(ref64), torch.isinf(ref64)
    assert torch.equal(torch.isnan(out), nan), f"{what}: NaN at other positions than the reference's"
    assert torch.equal(out[inf].double(), ref64[inf]), f"{what}: infinities differ from the reference's"
    fin = ~(nan | inf)
    assert fin.any(), f"{what}: nothing finite is left to compare"
    assert_within(out[fin], ref64[fin], ref32[fin], dtype, group, what, rel_floor=rel_floor,
                  extra=None if extra is None else extra[fin])


def poison(t):
    """Fill a scratch buffer with NaN in place (stale contents that nothing may consume)."""
    return t.fill_(float("nan"))
