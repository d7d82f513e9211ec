"""Shared assertions of the kernel-against-fp64 batteries (test_decode_kernels.py, test_train_row_kernels.py).

Tolerance of every rounded output, per element:  ulp(T) * |ref64| + 8 * e32 + floor.
``ulp`` is the spacing of T at 1 (2^-8 bf16, 2^-10 fp16, 2^-23 fp32): the single rounding of the
output.  ``e32`` is the largest error of a plain torch fp32 evaluation of the same reference formula on
the same inputs; the kernels accumulate in fp32, and the factor 8 covers their fast exp and their
summation order.  ``floor`` is 1e-6, or with ``rel_floor`` 1e-6 * max |ref64| (outputs that are small
as a whole: Adam second moments, gradients under a mean); a reference that is zero everywhere then
asks for exact zeros, and the rounding term is at least half the subnormal spacing of T (fp16: 2^-25 =
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


def assert_within(out, ref64, ref32, dtype, group, what="", rel_floor=False):
    """|out - ref64| <= ulp(T) |ref64| + 8 e32 + floor for every element; records the worst ratio."""
    assert out.shape == ref64.shape, (out.shape, ref64.shape)
    assert torch.isfinite(ref64).all(), f"{what}: reference is not finite"
    if out.numel() == 0:
        return
    if rel_floor and not ref64.any():
        assert not out.double().abs().any(), f"{what}: the reference is zero everywhere, the output is not"
        print(f"[{group} {_dt_id(dtype)}] {what} exact zeros")
        return
    e32 = (ref32.double() - ref64).abs().max().item()
    floor = ABS_FLOOR * ref64.abs().max().item() if rel_floor else ABS_FLOOR
    rounding = ULP[dtype] * ref64.abs()
    if rel_floor:  # below its smallest normal T is spaced absolutely: a correctly rounded fp16 is off by up to 2^-25
        rounding = rounding.clamp(min=HALF_SUBNORMAL[dtype])
    tol = rounding + E32_FACTOR * e32 + floor
    err = (out.double() - ref64).abs()
    assert not torch.isnan(err).any(), f"{what}: NaN in the kernel output"
    ratio = (err / tol).max().item()
    key = (group, _dt_id(dtype))
    _WORST[key] = max(_WORST.get(key, 0.0), ratio)
    off = (out != ref64.to(dtype)).sum().item()  # elements that are not the correctly rounded reference
    print(f"[{group} {_dt_id(dtype)}] {what} err/tol={ratio:.3f} max_err={err.max().item():.3e} e32={e32:.3e}"
          f" off_by_rounding={off}/{out.numel()} (worst so far {_WORST[key]:.3f})")
    assert ratio <= 1.0, f"{what}: err/tol = {ratio:.3f} (max err {err.max().item():.3e}, e32 {e32:.3e})"


def bits_equal(a, b):
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    it = _INT_VIEW[a.dtype]
    return torch.equal(a.contiguous().view(it), b.contiguous().view(it))
