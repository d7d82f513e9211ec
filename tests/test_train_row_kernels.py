"""The row kernels of every training step, branch by branch, against fp64 references written here:

* ``rms_norm_fwd`` / ``rms_norm_bwd`` (csrc/rmsnorm.hip) and ``layer_norm_fwd`` / ``layer_norm_bwd``
  (csrc/layernorm.hip): every CHUNKS count the issue of the vector kernels names, the generic kernels
  (odd column counts, too many chunks, misaligned pointers), both column reductions of csrc/colreduce.h
  and the scalar ones, odd rows per workgroup, workgroups without rows, empty input;
* ``swiglu_fwd`` / ``swiglu_bwd`` (csrc/swiglu_ce.hip): scalar tail, grid-stride loop, saturated
  sigmoid arguments, misaligned views (the host-side guard);
* ``cross_entropy_fwd`` / ``cross_entropy_bwd`` / ``ce_row_stats``: vector and scalar paths, more than
  one trip, every reduction, smoothing, class weights, ignored rows, -inf logits;
* ``optim.AdamW._fused`` (csrc/adamw.hip): single steps from constructed states, vector and scalar
  chunks, and the bitwise identities its comment promises.

Tolerance of every rounded output, per element:  ulp(T) |ref64| + 8 e32 + 1e-6 max |ref64|
(kernel_checks.assert_within with rel_floor).  The references take 16-bit inputs upcast exactly;
``e32`` is the error of the same formula evaluated by plain torch in fp32 on the same inputs.  The
fp32 side outputs (rstd, mean, lse, stats, per-row loss) are checked with T = fp32.  A reference that
is zero everywhere asks for exact zeros; pure identities are compared bitwise.  Every case is also run
with the fp32 evaluation in place of the kernel on the CPU (test_fp32_evaluation_within_tolerance_cpu):
no case relies on leniency.

AdamW's reference takes lr, betas, eps and weight decay rounded to fp32, the values the native entry
receives (0.999 is not a float: 1 - fp32(0.999) differs from 0.001 by 1.3e-5 of it); the bias
corrections are formed in double from the unrounded betas, as the host code does.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from kernel_checks import BF16, F16, F32, _WORST, _dt_id, assert_within, bits_equal

gpu = pytest.mark.gpu
F64 = torch.float64
DTYPES = [BF16, F16, F32]

# Largest err / tol measured on MI355X per group, bf16 / fp16 / fp32 (every run prints them with -s):
#   rmsnorm fwd     0.99 / 0.49 / 0.07   (y chunks8; fp32: generic1003 offset100)
#   layernorm fwd   0.99 / 0.49 / 0.24   (y pass8; fp32: chunks2 offset100)
#   rmsnorm bwd     1.00 / 0.50 / 0.21   (0.995: dx chunks5_generic; fp32: dw 300 x 300 cols 7)
#   layernorm bwd   1.00 / 0.50 / 0.15   (0.996: db generic1003; fp32: dw 300 x 300 cols 7)
#   swiglu          0.99 / 0.49 / 0.11   (grid-stride case; fp32: da n = 7)
#   cross entropy   0.98 / 0.54 / 0.10   (dlogits two_trips mean; fp16: dlogits rows300 mean, subnormal)
#   adamw           1.00 / 1.00 / 0.07   (0.996 / 0.997: exp_avg at |g| ~ 1e-4, for fp16 subnormal)
# As in test_decode_kernels.py a correctly rounded bf16 output reaches 1.0 of the rounding term alone
# and fp16 0.5 (1.0 below 6e-5, where fp16 is spaced absolutely); the fp32 figures are the share of
# 8 e32 + floor the kernels use.  No group needed more than the factor 8.  The whole file takes 9 s on
# MI355X (390 tests, the slowest GPU test 1 s: the first launch); the SwiGLU grid-stride cases take
# 0.11 / 0.14 / 0.06 s.


def VEC(dtype):
    return 4 if dtype == F32 else 8


def dev(gpu_run):
    return "cuda" if gpu_run else "cpu"


def off1(t):
    """A contiguous copy of ``t`` that starts one element into a larger buffer (not 16-byte aligned)."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and (t.device.type == "cpu" or t.numel() == 0 or v.data_ptr() % 16 != 0)
    return v


def check(out, r64, r32, T, group, what):
    assert out.dtype == T, (what, out.dtype, T)
    assert_within(out, r64, r32, T, group, what, rel_floor=True)


def as_kernel(r32, T):
    """The fp32 evaluation standing in for a kernel: its result rounded to the output dtype."""
    return None if r32 is None else r32.to(T)


# ------------------------------------------------------------------------------------------------
# references (dt = float64: the reference; dt = float32: the plain fp32 evaluation)
# ------------------------------------------------------------------------------------------------
def ref_rms_fwd(x, w, eps, dt=F64):
    x = x.to(dt)
    rstd = torch.rsqrt(x.pow(2).mean(-1) + eps)
    y = x * rstd[:, None]
    if w is not None:
        y = y * w.to(dt)
    return y, rstd


def ref_rms_bwd(dy, x, w, rstd, res, dt=F64):
    """(dx, dw) from the saved fp32 ``rstd`` (upcast exactly); ``res`` is added to dx."""
    dy, x, r = dy.to(dt), x.to(dt), rstd.to(dt)[:, None]
    xh = x * r
    gw = dy if w is None else dy * w.to(dt)
    dot = (gw * xh).mean(-1, keepdim=True)
    dx = r * (gw - xh * dot)
    if res is not None:
        dx = dx + res.to(dt)
    return dx, (None if w is None else (dy * xh).sum(0))


def ref_ln_fwd(x, w, b, eps, dt=F64):
    x = x.to(dt)
    mean = x.mean(-1)
    d = x - mean[:, None]
    rstd = torch.rsqrt((d * d).mean(-1) + eps)
    y = d * rstd[:, None]
    if w is not None:
        y = y * w.to(dt)
    if b is not None:
        y = y + b.to(dt)
    return y, mean, rstd


def ref_ln_bwd(dy, x, w, mean, rstd, res, dt=F64):
    """(dx, dw, db) from the saved fp32 ``mean`` / ``rstd`` (upcast exactly)."""
    dy, x, mu, r = dy.to(dt), x.to(dt), mean.to(dt)[:, None], rstd.to(dt)[:, None]
    xh = (x - mu) * r
    gw = dy if w is None else dy * w.to(dt)
    a1 = gw.mean(-1, keepdim=True)
    a2 = (gw * xh).mean(-1, keepdim=True)
    dx = r * (gw - a1 - xh * a2)
    if res is not None:
        dx = dx + res.to(dt)
    return dx, (dy * xh).sum(0), dy.sum(0)


def ref_swiglu_fwd(a, b, dt=F64):
    a, b = a.to(dt), b.to(dt)
    return a * torch.sigmoid(a) * b


def ref_swiglu_bwd(g, a, b, dt=F64):
    g, a, b = g.to(dt), a.to(dt), b.to(dt)
    s = torch.sigmoid(a)
    return g * b * (s * (1 + a * (1 - s))), g * a * s


def ref_ce(logits, target, weight, ignore_index, reduction, ls, g, dt=F64):
    """loss rows, lse, (reduced loss, count), dlogits for the upstream gradient ``g`` (per row for
    'none', a scalar otherwise).  'mean' divides by max(count, 1) without class weights (torch gives
    NaN when every row is ignored) and by the kept rows' target weights with them."""
    x = logits.to(dt)
    rows, V = x.shape
    kept = target != ignore_index
    t = torch.where(kept, target, torch.zeros_like(target))
    keep = kept.to(dt)
    w = torch.ones(V, dtype=dt, device=x.device) if weight is None else weight.to(dt)
    lse = torch.logsumexp(x, -1)
    wt = w[t] * keep
    xt = torch.where(kept, x.gather(1, t[:, None])[:, 0], torch.zeros_like(lse))  # x[0] of an ignored row may be -inf
    loss = wt * (lse - xt)
    if ls != 0.0:  # no -inf logits here: sum_c w_c (lse - x_c) would not be finite
        loss = (1 - ls) * loss + keep * (ls / V) * (w * (lse[:, None] - x)).sum(-1)
    count = wt.sum()
    if reduction == "mean":
        red = loss.sum() / (count.clamp(min=1) if weight is None else count)
    else:
        red = loss.sum()
    gr = g.to(dt)
    if reduction == "mean":
        gr = gr / (count.clamp(min=1) if weight is None else count)
    gr = (gr.expand(rows) * keep)[:, None]
    p = torch.exp(x - lse[:, None])
    onehot = torch.zeros_like(x).scatter_(1, t[:, None], 1.0)
    pc = (1 - ls) * wt + (ls / V) * w.sum() * keep
    dl = gr * (p * pc[:, None] - (1 - ls) * wt[:, None] * onehot - (ls / V) * w)
    return loss, lse, red, count, dl


def f32r(v):
    """A Python float rounded to fp32, as ctypes passes it to the native entry."""
    return torch.tensor(v, dtype=F32).item()


def ref_adamw(p, g, m, v, step, lr, b1, b2, eps, wd, dt=F64):
    bc1 = 1 - b1 ** step
    bc2_sqrt = math.sqrt(1 - b2 ** step)
    lr, b1, b2, eps, wd = (f32r(h) for h in (lr, b1, b2, eps, wd))
    p, g, m, v = p.to(dt), g.to(dt), m.to(dt), v.to(dt)
    p = p * (1 - lr * wd)
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    p = p - (lr / bc1) * m / (v.sqrt() / bc2_sqrt + eps)
    return p, m, v


# ------------------------------------------------------------------------------------------------
# the references against torch (CPU, fp64)
# ------------------------------------------------------------------------------------------------
def _close(a, b, tol=1e-11):
    torch.testing.assert_close(a, b, atol=tol, rtol=tol)


def test_ref_norms_match_torch_cpu():
    torch.manual_seed(0)
    rows, cols, eps = 5, 13, 1e-5
    x = torch.randn(rows, cols, dtype=F64, requires_grad=True)
    w = torch.randn(cols, dtype=F64, requires_grad=True)
    b = torch.randn(cols, dtype=F64, requires_grad=True)
    dy, res = torch.randn(rows, cols, dtype=F64), torch.randn(rows, cols, dtype=F64)
    for ww in (w, None):
        y, rstd = ref_rms_fwd(x, ww, eps)
        _close(y, F.rms_norm(x, (cols,), ww, eps))
        gx, *gw = torch.autograd.grad(F.rms_norm(x, (cols,), ww, eps), [x] + ([ww] if ww is not None else []), dy)
        dx, dw = ref_rms_bwd(dy, x.detach(), ww, rstd.detach(), res)
        _close(dx, gx + res)
        assert (dw is None) == (ww is None)
        if ww is not None:
            _close(dw, gw[0])
    for ww, bb in ((w, b), (w, None), (None, None)):
        y, mean, rstd = ref_ln_fwd(x, ww, bb, eps)
        exp = F.layer_norm(x, (cols,), ww, bb, eps)
        _close(y, exp)
        _close(mean, x.mean(-1))
        _close(rstd, torch.rsqrt(x.var(-1, unbiased=False) + eps))
        params = [t for t in (ww, bb) if t is not None]
        gx, *gp = torch.autograd.grad(exp, [x] + params, dy)
        dx, dw, db = ref_ln_bwd(dy, x.detach(), ww, mean.detach(), rstd.detach(), res)
        _close(dx, gx + res)
        if ww is not None:
            _close(dw, gp[0])
        if bb is not None:
            _close(db, gp[1])


def test_ref_swiglu_matches_torch_cpu():
    torch.manual_seed(0)
    a = (torch.randn(37, dtype=F64) * 3).requires_grad_(True)
    b = torch.randn(37, dtype=F64, requires_grad=True)
    g = torch.randn(37, dtype=F64)
    y = F.silu(a) * b
    _close(ref_swiglu_fwd(a, b), y)
    ga, gb = torch.autograd.grad(y, [a, b], g)
    da, db = ref_swiglu_bwd(g, a.detach(), b.detach())
    _close(da, ga)
    _close(db, gb)


def test_ref_ce_matches_torch_cpu():
    torch.manual_seed(0)
    rows, V = 7, 11
    x = (torch.randn(rows, V, dtype=F64) * 3).requires_grad_(True)
    target = torch.randint(0, V, (rows,))
    target[2] = -100
    target[0], target[1] = 0, V - 1
    w = torch.rand(V, dtype=F64) + 0.5
    for weight in (None, w):
        for reduction in ("none", "mean", "sum"):
            for ls in (0.0, 0.1):
                exp = F.cross_entropy(x, target, weight=weight, ignore_index=-100, reduction=reduction, label_smoothing=ls)
                g = torch.randn(rows, dtype=F64) if reduction == "none" else torch.tensor(1.7, dtype=F64)
                loss, lse, red, count, dl = ref_ce(x.detach(), target, weight, -100, reduction, ls, g)
                _close(loss if reduction == "none" else red, exp)
                _close(lse, torch.logsumexp(x.detach(), -1))
                _close(count, (target != -100).sum().double() if weight is None else w[target[target != -100]].sum())
                (gx,) = torch.autograd.grad(exp, x, g)
                _close(dl, gx)
    # -inf logits, no smoothing: finite wherever the target logit is finite, as in torch
    xi = x.detach().clone()
    xi[:, 6:] = float("-inf")
    xi[:, 0] = float("-inf")
    t2 = torch.randint(1, 6, (rows,))
    loss, lse, red, _, dl = ref_ce(xi, t2, None, -100, "mean", 0.0, torch.tensor(1.0, dtype=F64))
    xi.requires_grad_(True)
    exp = F.cross_entropy(xi, t2)
    assert torch.isfinite(loss).all() and torch.isfinite(dl).all()
    _close(red, exp)
    _close(dl, torch.autograd.grad(exp, xi)[0])
    # every row ignored under 'mean': torch gives NaN, the kernels document sum / max(count, 1) = 0
    t3 = torch.full((rows,), -100)
    assert torch.isnan(F.cross_entropy(x.detach(), t3))
    loss, _, red, count, dl = ref_ce(x.detach(), t3, None, -100, "mean", 0.0, torch.tensor(1.0, dtype=F64))
    assert red.item() == 0 and count.item() == 0 and not dl.any()


def test_ref_adamw_matches_torch_cpu():
    torch.manual_seed(0)
    # hyperparameters that are floats already, so that rounding them to fp32 changes nothing
    lr, b1, b2, eps = 2.0 ** -7, 0.875, 1 - 2.0 ** -9, 2.0 ** -27
    for wd in (0.0, 0.125):
        assert all(f32r(h) == h for h in (lr, b1, b2, eps, wd))
        for step in (1, 7, 1000):
            p0, g = torch.randn(50, dtype=F64), torch.randn(50, dtype=F64)
            m0, v0 = torch.randn(50, dtype=F64) * 0.3, torch.rand(50, dtype=F64)
            p = torch.nn.Parameter(p0.clone())
            p.grad = g.clone()
            opt = torch.optim.AdamW([p], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
            opt.state[p] = {"step": torch.tensor(float(step - 1)), "exp_avg": m0.clone(), "exp_avg_sq": v0.clone()}
            opt.step()
            rp, rm, rv = ref_adamw(p0, g, m0, v0, step, lr, b1, b2, eps, wd)
            _close(opt.state[p]["exp_avg"], rm)
            _close(opt.state[p]["exp_avg_sq"], rv)
            _close(p.detach(), rp)


# ------------------------------------------------------------------------------------------------
# A. RMSNorm / LayerNorm forward
# ------------------------------------------------------------------------------------------------
EPS = 1e-5


def _row_scale(rows):
    return 0.5 + 1.5 * ((torch.arange(rows) * 37) % 101).float() / 101


def _col_scale(cols):
    return 0.5 + 1.5 * ((torch.arange(cols) * 53) % 97).float() / 97


def norm_fwd_cols(dtype):
    """name -> cols; every dispatch branch of launch_fwd."""
    V, P = VEC(dtype), 256 * VEC(dtype)
    c = {f"chunks{C}": P * (C - 1) + V for C in (1, 2, 3, 5, 8)}
    c.update(pass1=P, pass8=8 * P, wave_plus_lane=65 * V, chunks9_generic=8 * P + V)
    c.update({f"generic{n}": n for n in (1, 7, 257, 1003)})
    c.update(misaligned_x=P + V, misaligned_w=P + V)
    return c


NORM_FWD_NAMES = list(norm_fwd_cols(BF16))


def _norm_fwd_inputs(name, dtype, device, kind="randn"):
    cols = norm_fwd_cols(dtype)[name]
    rows = 3 + cols % 5
    g = torch.Generator().manual_seed(cols * 8 + rows)
    x = torch.randn(rows, cols, generator=g) * _col_scale(cols)
    if kind == "offset100":
        x = 100 + torch.randn(rows, cols, generator=g)
    elif kind == "zero_row":
        x[1] = 0
    x = x.to(dtype).to(device)
    w = (1 + 0.5 * torch.randn(cols, generator=g)).to(dtype).to(device)
    b = torch.randn(cols, generator=g).to(dtype).to(device)
    if name == "misaligned_x":
        x = off1(x)
    if name == "misaligned_w":
        w, b = off1(w), off1(b)
    return x, w, b


def _run_rms_fwd(name, dtype, gpu_run, kind="randn"):
    x, w, _ = _norm_fwd_inputs(name, dtype, dev(gpu_run), kind)
    for ww in (w, None):
        r64, r32 = ref_rms_fwd(x, ww, EPS), ref_rms_fwd(x, ww, EPS, F32)
        if gpu_run:
            from lightning_thunder_amd.ops.rmsnorm import rms_norm_fwd

            y, rstd = rms_norm_fwd(x, ww, EPS)
        else:
            y, rstd = as_kernel(r32[0], dtype), r32[1]
        what = f"{name} cols={x.shape[1]} {kind} w={'yes' if ww is not None else 'none'}"
        check(y, r64[0], r32[0], dtype, "rmsnorm fwd", f"y {what}")
        check(rstd, r64[1], r32[1], F32, "rmsnorm fwd", f"rstd {what}")


def _run_ln_fwd(name, dtype, gpu_run, kind="randn"):
    x, w, b = _norm_fwd_inputs(name, dtype, dev(gpu_run), kind)
    for ww, bb in ((w, b), (w, None), (None, None)):
        r64, r32 = ref_ln_fwd(x, ww, bb, EPS), ref_ln_fwd(x, ww, bb, EPS, F32)
        if gpu_run:
            from lightning_thunder_amd.ops.rmsnorm import layer_norm_fwd

            y, mean, rstd = layer_norm_fwd(x, ww, bb, EPS)
        else:
            y, mean, rstd = as_kernel(r32[0], dtype), r32[1], r32[2]
        what = f"{name} cols={x.shape[1]} {kind} w={'yes' if ww is not None else 'none'} b={'yes' if bb is not None else 'none'}"
        check(y, r64[0], r32[0], dtype, "layernorm fwd", f"y {what}")
        check(mean, r64[1], r32[1], F32, "layernorm fwd", f"mean {what}")
        check(rstd, r64[2], r32[2], F32, "layernorm fwd", f"rstd {what}")


# (name, dtype, kind) beyond the plain sweep
NORM_FWD_EXTRA = [("chunks2", F32, "offset100"), ("chunks2", F16, "offset100"), ("generic1003", F32, "offset100"),
                  ("chunks2", BF16, "zero_row"), ("generic257", F32, "zero_row")]


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=_dt_id)
@pytest.mark.parametrize("name", NORM_FWD_NAMES)
def test_rms_norm_fwd(name, dtype):
    _run_rms_fwd(name, dtype, True)


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=_dt_id)
@pytest.mark.parametrize("name", NORM_FWD_NAMES)
def test_layer_norm_fwd(name, dtype):
    _run_ln_fwd(name, dtype, True)


@gpu
@pytest.mark.parametrize("name,dtype,kind", NORM_FWD_EXTRA, ids=lambda v: v if isinstance(v, str) else _dt_id(v))
def test_norm_fwd_offset_and_zero_rows(name, dtype, kind):
    # rows of 100 + randn: a variance formed as E[x^2] - E[x]^2 loses it to cancellation
    _run_ln_fwd(name, dtype, True, kind)
    _run_rms_fwd(name, dtype, True, kind)


# ------------------------------------------------------------------------------------------------
# B. RMSNorm / LayerNorm backward
# ------------------------------------------------------------------------------------------------
def norm_bwd_cols(dtype):
    """name -> cols; every dispatch branch of launch_bwd (kernel x column reduction)."""
    V, P = VEC(dtype), 256 * VEC(dtype)
    c = {"chunks1": V, "chunks2": P + V, "chunks4": 3 * P + V, "chunks5_generic": 4 * P + V,
         "generic7": 7, "generic1003": 1003, "cols1004": 1004,  # 16-bit: generic backward + v4 reduction
         "misaligned_dy": P + V, "misaligned_res": P + V}
    return c


NORM_BWD_NAMES = list(norm_bwd_cols(BF16))
ROWS_BLOCKS = [(7, 1), (7, 3), (5, 5)]  # 7 x 3: three rows per workgroup (a pair, then one), the last takes one


def _norm_bwd_inputs(cols, rows, dtype, device, name=""):
    g = torch.Generator().manual_seed(cols * 16 + rows)
    x = (torch.randn(rows, cols, generator=g) * _col_scale(cols) + 0.25).to(dtype).to(device)
    dy = (torch.randn(rows, cols, generator=g) * _row_scale(rows)[:, None]).to(dtype).to(device)
    w = (1 + 0.5 * torch.randn(cols, generator=g)).to(dtype).to(device)
    res = torch.randn(rows, cols, generator=g).to(dtype).to(device)
    if name == "misaligned_dy":
        dy = off1(dy)
    if name == "misaligned_res":
        res = off1(res)
    return x, dy, w, res


def _set_blocks(monkeypatch, blocks):
    if monkeypatch is not None:
        monkeypatch.setenv("LTA_RMS_BWD_BLOCKS", str(blocks))


def _run_rms_bwd(cols, rows, blocks, dtype, gpu_run, monkeypatch, name="", combos=((True, True), (True, False), (False, True))):
    x, dy, w, res = _norm_bwd_inputs(cols, rows, dtype, dev(gpu_run), name)
    rstd = ref_rms_fwd(x, None, EPS)[1].float()  # the fp64 value rounded once: the kernel is judged alone
    _set_blocks(monkeypatch, blocks)
    for has_w, has_res in combos:
        ww, rr = (w if has_w else None), (res if has_res else None)
        r64, r32 = ref_rms_bwd(dy, x, ww, rstd, rr), ref_rms_bwd(dy, x, ww, rstd, rr, F32)
        if gpu_run:
            from lightning_thunder_amd.ops.rmsnorm import rms_norm_bwd

            dx, dw = rms_norm_bwd(dy, x, ww, rstd, rr)
        else:
            dx, dw = as_kernel(r32[0], dtype), as_kernel(r32[1], dtype)
        what = f"{name} cols={cols} rows={rows} blocks={blocks} w={has_w} res={has_res}"
        check(dx, r64[0], r32[0], dtype, "rmsnorm bwd", f"dx {what}")
        assert (dw is None) == (not has_w)
        if has_w:
            check(dw, r64[1], r32[1], dtype, "rmsnorm bwd", f"dw {what}")


def _run_ln_bwd(cols, rows, blocks, dtype, gpu_run, monkeypatch, name="",
                combos=((True, True, True), (True, False, False), (False, False, True))):
    x, dy, w, res = _norm_bwd_inputs(cols, rows, dtype, dev(gpu_run), name)
    _, mean, rstd = ref_ln_fwd(x, None, None, EPS)
    mean, rstd = mean.float(), rstd.float()
    _set_blocks(monkeypatch, blocks)
    for has_w, has_b, has_res in combos:
        ww, rr = (w if has_w else None), (res if has_res else None)
        r64, r32 = ref_ln_bwd(dy, x, ww, mean, rstd, rr), ref_ln_bwd(dy, x, ww, mean, rstd, rr, F32)
        if gpu_run:
            from lightning_thunder_amd.ops.rmsnorm import layer_norm_bwd

            dx, dw, db = layer_norm_bwd(dy, x, ww, mean, rstd, has_b, rr)
        else:
            dx, dw, db = as_kernel(r32[0], dtype), (as_kernel(r32[1], dtype) if has_w else None), \
                (as_kernel(r32[2], dtype) if has_b else None)
        what = f"{name} cols={cols} rows={rows} blocks={blocks} w={has_w} b={has_b} res={has_res}"
        check(dx, r64[0], r32[0], dtype, "layernorm bwd", f"dx {what}")
        assert (dw is None) == (not has_w) and (db is None) == (not has_b)
        if has_w:
            check(dw, r64[1], r32[1], dtype, "layernorm bwd", f"dw {what}")
        if has_b:
            check(db, r64[2], r32[2], dtype, "layernorm bwd", f"db {what}")


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=_dt_id)
@pytest.mark.parametrize("name", NORM_BWD_NAMES)
def test_rms_norm_bwd(name, dtype, monkeypatch):
    for rows, blocks in ROWS_BLOCKS:
        _run_rms_bwd(norm_bwd_cols(dtype)[name], rows, blocks, dtype, True, monkeypatch, name)


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=_dt_id)
@pytest.mark.parametrize("name", NORM_BWD_NAMES)
def test_layer_norm_bwd(name, dtype, monkeypatch):
    for rows, blocks in ROWS_BLOCKS:
        _run_ln_bwd(norm_bwd_cols(dtype)[name], rows, blocks, dtype, True, monkeypatch, name)


# rows x workgroups at few columns: 300 x 300 runs the 8-way unrolled loop of column_reduce_v4_kernel (row
# groups 0..11 once) beside its tail loop; 700 x 512 gives two rows per workgroup and none to 350..511
MANY_BLOCKS = [(300, 300, 40), (700, 512, 40), (700, 512, 1003), (300, 300, 7)]


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=_dt_id)
@pytest.mark.parametrize("rows,blocks,cols", MANY_BLOCKS)
def test_rms_norm_bwd_many_workgroups(rows, blocks, cols, dtype, monkeypatch):
    _run_rms_bwd(cols, rows, blocks, dtype, True, monkeypatch, combos=((True, True),))


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=_dt_id)
@pytest.mark.parametrize("rows,blocks,cols", MANY_BLOCKS)
def test_layer_norm_bwd_many_workgroups(rows, blocks, cols, dtype, monkeypatch):
    _run_ln_bwd(cols, rows, blocks, dtype, True, monkeypatch, combos=((True, True, True),))


@gpu
@pytest.mark.parametrize("dtype", [BF16, F32], ids=_dt_id)
@pytest.mark.parametrize("cols", [40, 1003])
def test_norm_bwd_rowless_workgroups_write_zero_partials(cols, dtype):
    """700 rows on 512 workgroups through the native entries with a workspace full of a sentinel:
    a workgroup without rows that leaves its partial row unwritten puts the sentinel into dw / db."""
    import lightning_thunder_amd.ops.rmsnorm  # noqa: F401  (registers the signatures)
    from lightning_thunder_amd.ops._lib import dcode, ptr, require, stream_ptr

    lib = require()
    rows, blocks = 700, 512
    x, dy, w, res = _norm_bwd_inputs(cols, rows, dtype, "cuda")
    _, mean, rstd = ref_ln_fwd(x, None, None, EPS)
    mean, rstd = mean.float(), rstd.float()
    rstd_rms = ref_rms_fwd(x, None, EPS)[1].float()
    s = stream_ptr(x.device)

    dx, dw = torch.empty_like(x), torch.empty_like(w)
    ws = torch.full((blocks, cols), 1.0e30, device="cuda", dtype=F32)
    rc = lib.lta_rmsnorm_bwd_res(dcode(x), ptr(dy), ptr(x), ptr(w), ptr(rstd_rms), ptr(dx), ptr(dw), ptr(ws), rows, cols,
                                 blocks, ptr(res), s)
    assert rc == 0
    r64, r32 = ref_rms_bwd(dy, x, w, rstd_rms, res), ref_rms_bwd(dy, x, w, rstd_rms, res, F32)
    check(dx, r64[0], r32[0], dtype, "rmsnorm bwd", f"dx sentinel cols={cols}")
    check(dw, r64[1], r32[1], dtype, "rmsnorm bwd", f"dw sentinel cols={cols}")
    assert not (ws[350:] != 0).any(), "workgroups 350..511 have no rows: their partial rows must be zero"

    dx, dw, db = torch.empty_like(x), torch.empty_like(w), torch.empty_like(w)
    ws = torch.full((blocks, 2, cols), 1.0e30, device="cuda", dtype=F32)
    rc = lib.lta_layernorm_bwd_res(dcode(x), ptr(dy), ptr(x), ptr(w), ptr(mean), ptr(rstd), ptr(dx), ptr(dw), ptr(db),
                                   ptr(ws), rows, cols, blocks, ptr(res), s)
    assert rc == 0
    r64, r32 = ref_ln_bwd(dy, x, w, mean, rstd, res), ref_ln_bwd(dy, x, w, mean, rstd, res, F32)
    check(dx, r64[0], r32[0], dtype, "layernorm bwd", f"dx sentinel cols={cols}")
    check(dw, r64[1], r32[1], dtype, "layernorm bwd", f"dw sentinel cols={cols}")
    check(db, r64[2], r32[2], dtype, "layernorm bwd", f"db sentinel cols={cols}")
    assert not (ws == 1.0e30).any(), "a partial row was left unwritten"


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=_dt_id)
@pytest.mark.parametrize("cols", [16, 7])
def test_norms_empty_input(cols, dtype):
    from lightning_thunder_amd.ops.rmsnorm import layer_norm_bwd, layer_norm_fwd, rms_norm_bwd, rms_norm_fwd

    x = torch.empty(0, cols, device="cuda", dtype=dtype)
    w = torch.ones(cols, device="cuda", dtype=dtype)
    y, rstd = rms_norm_fwd(x, w, EPS)
    assert y.shape == (0, cols) and y.dtype == dtype and rstd.shape == (0,) and rstd.dtype == F32
    y, mean, rstd = layer_norm_fwd(x, w, w, EPS)
    assert y.shape == (0, cols) and mean.shape == (0,) and rstd.shape == (0,)
    dx, dw = rms_norm_bwd(x, x, w, rstd, x)
    assert dx.shape == (0, cols) and dw.dtype == dtype and dw.shape == (cols,) and not dw.any()
    dx, dw, db = layer_norm_bwd(x, x, w, mean, rstd, True, x)
    assert dx.shape == (0, cols) and dw.shape == db.shape == (cols,) and not dw.any() and not db.any()
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------
# C. SwiGLU
# ------------------------------------------------------------------------------------------------
def _swiglu_inputs(n, dtype, device, kind="randn"):
    g = torch.Generator().manual_seed(n % 100003 + 7)
    a = torch.randn(n, generator=g) * 3
    b = torch.randn(n, generator=g)
    gr = torch.randn(n, generator=g)
    if kind == "saturated":  # the gate and the gradient stay of order one
        vals = torch.tensor([0.0, -0.0, 1e-3, -1e-3, 20.0, -20.0, 87.0, -87.0, -100.0])
        a = vals.repeat(n // vals.numel() + 1)[:n]
    elif kind == "largest":  # largest finite 16-bit magnitudes; |b|, |g| = 1/2 keep a b and g a finite in T
        big = 65504.0 if dtype == F16 else torch.finfo(BF16).max
        a = big * (1 - 2 * (torch.arange(n) % 2).float())
        b = 0.5 * torch.sign(b)
        gr = 0.5 * torch.sign(gr)
    return tuple(t.to(dtype).to(device) for t in (a, b, gr))


def _run_swiglu(n, dtype, gpu_run, kind="randn", misalign=()):
    a, b, g = _swiglu_inputs(n, dtype, dev(gpu_run), kind)
    if "a" in misalign:
        a = off1(a)
    if "b" in misalign:
        b = off1(b)
    if "g" in misalign:
        g = off1(g)
    y64, y32 = ref_swiglu_fwd(a, b), ref_swiglu_fwd(a, b, F32)
    d64, d32 = ref_swiglu_bwd(g, a, b), ref_swiglu_bwd(g, a, b, F32)
    if gpu_run:
        from lightning_thunder_amd.ops.fused import swiglu_bwd, swiglu_fwd

        y = swiglu_fwd(a, b)
        da, db = swiglu_bwd(g, a, b)
    else:
        y, da, db = as_kernel(y32, dtype), as_kernel(d32[0], dtype), as_kernel(d32[1], dtype)
    what = f"n={n} {kind} misaligned={','.join(misalign) or 'no'}"
    check(y, y64, y32, dtype, "swiglu", f"y {what}")
    check(da, d64[0], d32[0], dtype, "swiglu", f"da {what}")
    check(db, d64[1], d32[1], dtype, "swiglu", f"db {what}")


SWIGLU_CASES = [(1, "randn", ()), (7, "randn", ()), (8, "randn", ()), (2055, "randn", ()),
                (2055, "saturated", ()), (2055, "largest", ()),
                (2055, "randn", ("a",)), (2055, "randn", ("b",)), (2055, "randn", ("g",)), (2048, "saturated", ("a", "b", "g"))]


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=_dt_id)
@pytest.mark.parametrize("n,kind,misalign", SWIGLU_CASES, ids=lambda v: "".join(v) if isinstance(v, tuple) else str(v))
def test_swiglu(n, kind, misalign, dtype):
    _run_swiglu(n, dtype, True, kind, misalign)


def swiglu_grid_stride_n(dtype):
    return 4096 * 256 * VEC(dtype) + VEC(dtype) + 3  # the grid is capped at 4096 workgroups: one vector more, and a tail


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=_dt_id)
def test_swiglu_grid_stride(dtype):
    import time

    t0 = time.perf_counter()
    _run_swiglu(swiglu_grid_stride_n(dtype), dtype, True)
    torch.cuda.synchronize()
    print(f"[swiglu {_dt_id(dtype)}] grid-stride case n={swiglu_grid_stride_n(dtype)} took {time.perf_counter() - t0:.2f} s")


# ------------------------------------------------------------------------------------------------
# D. cross entropy
# ------------------------------------------------------------------------------------------------
def ce_vocabs(dtype):
    return [8, 1000, 1003, 2 * 256 * VEC(dtype) + VEC(dtype)]


CE_V_IDS = ["V8", "V1000", "V1003_scalar", "two_trips"]


def _ce_inputs(V, dtype, device, rows=7, weight_dtype=None, misaligned=False, seed=0):
    """rows: 0 target 0, 1 target V-1, 2 target in the last (partial) vector, 3 ignored, 4 rising along
    the vocabulary (every trip of every thread rescales), 5 one logit more than 80 above the rest, 6.. random."""
    g = torch.Generator().manual_seed(V * 4 + rows + seed)
    x = torch.randn(rows, V, generator=g) * 2
    target = torch.randint(0, V, (rows,), generator=g)
    target[0] = 0
    if rows > 1:
        target[1] = V - 1
    if rows > 2:
        target[2] = max(V - 2, 0)
    if rows > 3:
        target[3] = -100
    if rows > 4:
        x[4] = torch.linspace(-8, 8, V) + 0.1 * torch.randn(V, generator=g)
    if rows > 5:
        x[5] = x[5].clamp(-3, 3)
        x[5, V // 3] = 90.0
    if rows > 8:
        target[rows // 2::7] = -100
    w = None if weight_dtype is None else (0.5 + torch.rand(V, generator=g)).to(weight_dtype).to(device)
    x = x.to(dtype).to(device)
    if misaligned:
        x = off1(x)
    return x, target.to(device), w


def _ce_g(reduction, rows, device):
    g = torch.Generator().manual_seed(rows)
    if reduction == "none":
        return (0.5 + torch.rand(rows, generator=g)).to(device)
    return torch.tensor(1.7).to(device)


def _run_ce(x, target, w, reduction, ls, dtype, gpu_run, what, check_finite_rows=None):
    rows, V = x.shape
    g = _ce_g(reduction, rows, x.device)
    loss64, lse64, red64, cnt64, dl64 = ref_ce(x, target, w, -100, reduction, ls, g)
    loss32, lse32, red32, cnt32, dl32 = ref_ce(x, target, w, -100, reduction, ls, g, F32)
    if gpu_run:
        from lightning_thunder_amd.ops.fused import cross_entropy_bwd, cross_entropy_fwd

        loss, lse, stats = cross_entropy_fwd(x, target, -100, reduction, ls, w)
        dl = cross_entropy_bwd(g, x, target, lse64.float(), torch.stack((red64, cnt64)).float(), -100, reduction, ls, w)
    else:
        loss = as_kernel(loss32 if reduction == "none" else red32, dtype)
        lse, stats, dl = lse32, torch.stack((red32, cnt32)), as_kernel(dl32, dtype)
    what = f"{what} V={V} rows={rows} {reduction} ls={ls} w={'none' if w is None else _dt_id(w.dtype)}"
    grp = "cross entropy"
    check(lse, lse64, lse32, F32, grp, f"lse {what}")
    if reduction == "none":
        check(loss, loss64, loss32, dtype, grp, f"loss {what}")
    else:
        check(loss, red64, red32, dtype, grp, f"loss {what}")
        check(stats[0], red64, red32, F32, grp, f"stats[0] {what}")
        check(stats[1], cnt64, cnt32, F32, grp, f"stats[1] {what}")
    check(dl, dl64, dl32, dtype, grp, f"dlogits {what}")
    ignored = target == -100
    if ignored.any():
        assert not dl[ignored].float().abs().any(), "the gradient of an ignored row is exactly zero"
        if reduction == "none":
            assert not loss[ignored].float().abs().any()


@gpu
@pytest.mark.parametrize("ls", [0.0, 0.1])
@pytest.mark.parametrize("reduction", ["none", "mean", "sum"])
@pytest.mark.parametrize("dtype", DTYPES, ids=_dt_id)
@pytest.mark.parametrize("vi", range(4), ids=CE_V_IDS)
def test_cross_entropy(vi, dtype, reduction, ls):
    x, t, _ = _ce_inputs(ce_vocabs(dtype)[vi], dtype, "cuda")
    _run_ce(x, t, None, reduction, ls, dtype, True, CE_V_IDS[vi])


@gpu
@pytest.mark.parametrize("ls", [0.0, 0.1])
@pytest.mark.parametrize("reduction", ["none", "mean", "sum"])
@pytest.mark.parametrize("wdtype", [BF16, F32], ids=_dt_id)
@pytest.mark.parametrize("dtype", [BF16, F32], ids=_dt_id)
@pytest.mark.parametrize("vi", [1, 2], ids=CE_V_IDS[1:3])
def test_cross_entropy_class_weights(vi, dtype, wdtype, reduction, ls):
    x, t, w = _ce_inputs(ce_vocabs(dtype)[vi], dtype, "cuda", weight_dtype=wdtype)
    _run_ce(x, t, w, reduction, ls, dtype, True, CE_V_IDS[vi])


@gpu
@pytest.mark.parametrize("reduction", ["none", "mean"])
@pytest.mark.parametrize("dtype", DTYPES, ids=_dt_id)
def test_cross_entropy_misaligned_and_many_rows(dtype, reduction):
    x, t, _ = _ce_inputs(ce_vocabs(dtype)[3], dtype, "cuda", misaligned=True)
    _run_ce(x, t, None, reduction, 0.1, dtype, True, "misaligned")
    x, t, _ = _ce_inputs(8, dtype, "cuda", rows=300)  # the reduction kernel's 256 threads loop twice
    _run_ce(x, t, None, reduction, 0.0, dtype, True, "rows300")


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=_dt_id)
def test_cross_entropy_all_rows_ignored(dtype):
    # torch returns NaN for 'mean' here; the kernels document sum / max(count, 1): loss 0, gradient exactly 0
    x, t, _ = _ce_inputs(1000, dtype, "cuda")
    t = torch.full_like(t, -100)
    for reduction in ("mean", "sum", "none"):
        _run_ce(x, t, None, reduction, 0.1, dtype, True, "all ignored")


def _ce_inf_inputs(V, dtype, device, pattern):
    """-inf logits (label_smoothing 0); every target logit is finite."""
    x, target, _ = _ce_inputs(V, dtype, device, rows=6)
    nv = VEC(dtype)
    ninf = float("-inf")
    if pattern == "masked_tail":  # padding of the vocabulary: the first logits of the later threads are all -inf
        keep = V // 5
        x[:, keep:] = ninf
        lo, hi = 0, keep
    elif pattern == "index0":
        x[:, 0] = ninf
        lo, hi = 1, V
    elif pattern == "block":  # the first 16-byte vector of threads 3..8
        x[:, 3 * nv:9 * nv] = ninf
        lo, hi = 9 * nv, V
    else:
        raise ValueError(pattern)
    g = torch.Generator().manual_seed(V)
    target = torch.randint(lo, hi, (x.shape[0],), generator=g).to(device)
    target[0], target[1], target[3] = lo, hi - 1, -100
    return x, target


CE_INF_PATTERNS = ["masked_tail", "index0", "block"]


def _run_ce_inf(vi, dtype, pattern, gpu_run):
    x, t = _ce_inf_inputs(ce_vocabs(dtype)[vi], dtype, dev(gpu_run), pattern)
    for reduction in ("none", "mean"):
        _run_ce(x, t, None, reduction, 0.0, dtype, gpu_run, f"-inf {pattern}")
    lse64, lse32 = torch.logsumexp(x.double(), -1), torch.logsumexp(x.float(), -1)
    l64, _, _, _, _ = ref_ce(x, t, None, -100, "none", 0.0, torch.ones(x.shape[0], device=x.device))
    l32, _, _, _, _ = ref_ce(x, t, None, -100, "none", 0.0, torch.ones(x.shape[0], device=x.device), F32)
    if gpu_run:
        from lightning_thunder_amd.ops.fused import ce_row_stats

        lse, lrows = ce_row_stats(x, t)
    else:
        lse, lrows = lse32, l32
    check(lse, lse64, lse32, F32, "cross entropy", f"ce_row_stats lse -inf {pattern}")
    check(lrows, l64, l32, F32, "cross entropy", f"ce_row_stats loss -inf {pattern}")


@gpu
@pytest.mark.parametrize("pattern", CE_INF_PATTERNS)
@pytest.mark.parametrize("dtype", DTYPES, ids=_dt_id)
@pytest.mark.parametrize("vi", [2, 3], ids=CE_V_IDS[2:])
def test_cross_entropy_neg_inf_logits(vi, dtype, pattern):
    _run_ce_inf(vi, dtype, pattern, True)


def _run_ce_row_stats(vi, dtype, gpu_run):
    x, t, _ = _ce_inputs(ce_vocabs(dtype)[vi], dtype, dev(gpu_run))
    ones = torch.ones(x.shape[0], device=x.device)
    l64, lse64, _, _, _ = ref_ce(x, t, None, -100, "none", 0.0, ones)
    l32, lse32, _, _, _ = ref_ce(x, t, None, -100, "none", 0.0, ones, F32)
    if gpu_run:
        from lightning_thunder_amd.ops.fused import ce_row_stats

        lse, lrows = ce_row_stats(x, t)
    else:
        lse, lrows = lse32, l32
    check(lse, lse64, lse32, F32, "cross entropy", f"ce_row_stats lse {CE_V_IDS[vi]}")
    check(lrows, l64, l32, F32, "cross entropy", f"ce_row_stats loss (fp32, before any cast) {CE_V_IDS[vi]}")
    assert lrows[3].item() == 0.0


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=_dt_id)
@pytest.mark.parametrize("vi", range(4), ids=CE_V_IDS)
def test_ce_row_stats(vi, dtype):
    _run_ce_row_stats(vi, dtype, True)


# ------------------------------------------------------------------------------------------------
# E. AdamW
# ------------------------------------------------------------------------------------------------
ADAMW_PAIRS = [(BF16, F32), (BF16, BF16), (F16, F16), (F16, F32), (F32, F32)]
# one launch: a scalar tail chunk (1, 33, + 5), one vector trip, a partial trip (2048 + 8), several chunks
ADAMW_SIZES = [1, 33, 2048, 16384, 16384 + 5, 16384 + 2048 + 8, 3 * 16384]
LR, B1, B2, ADAM_EPS = 1e-2, 0.9, 0.999, 1e-8


def _adamw_inputs(pdt, sdt, gscale, device, seed=0):
    """(p, g, m, v) per tensor; the first eighth of every tensor is untouched state with a zero gradient."""
    g_ = torch.Generator().manual_seed(seed)
    out = []
    for n in ADAMW_SIZES:
        p = 0.1 * torch.randn(n, generator=g_)
        g = gscale * torch.randn(n, generator=g_)
        m = 0.5 * gscale * torch.randn(n, generator=g_)
        v = 0.01 * gscale * gscale * (0.1 + torch.rand(n, generator=g_))
        z = (n + 7) // 8
        g[:z], m[:z], v[:z] = 0, 0, 0
        out.append((p.to(pdt).to(device), g.to(pdt).to(device), m.to(sdt).to(device), v.to(sdt).to(device)))
    return out


def _adamw_launch(tensors, pdt, sdt, step, wd, lean=False):
    """One multi-tensor launch on copies of ``tensors`` laid out as given; returns the updated (p, m, v)."""
    from lightning_thunder_amd.optim import AdamW

    opt = AdamW([torch.nn.Parameter(torch.zeros(1, device="cuda"))], lr=LR, betas=(B1, B2), eps=ADAM_EPS, weight_decay=wd)
    ps, gs = [], []
    for p, g, m, v in tensors:
        opt.state[p] = {"step": step, "exp_avg": m, "exp_avg_sq": v}
        ps.append(p)
        gs.append(g)
    opt._fused(ps, pdt, sdt, ps[0].device, step, LR, B1, B2, ADAM_EPS, wd, grads=gs, lean=lean)
    torch.cuda.synchronize()
    return [(p, opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"]) for p in ps]


def _clone(tensors, misalign=False):
    f = off1 if misalign else torch.clone
    return [tuple(f(t) for t in ts) for ts in tensors]


ADAMW_STEPS_WD_SCALE = [(step, wd, gs) for step in (1, 7, 1000) for wd in (0.0, 0.1) for gs in (1e-4, 1e3)]


def _run_adamw(pdt, sdt, gpu_run):
    for step, wd, gscale in ADAMW_STEPS_WD_SCALE:
        tensors = _adamw_inputs(pdt, sdt, gscale, dev(gpu_run), seed=step)
        refs64 = [ref_adamw(p, g, m, v, step, LR, B1, B2, ADAM_EPS, wd) for p, g, m, v in tensors]
        refs32 = [ref_adamw(p, g, m, v, step, LR, B1, B2, ADAM_EPS, wd, F32) for p, g, m, v in tensors]
        if gpu_run:
            outs = _adamw_launch(_clone(tensors), pdt, sdt, step, wd)
        else:
            outs = [(r[0].to(pdt), r[1].to(sdt), r[2].to(sdt)) for r in refs32]
        for n, o, r64, r32 in zip(ADAMW_SIZES, outs, refs64, refs32):
            what = f"n={n} step={step} wd={wd} |g|~{gscale:g} state={_dt_id(sdt)}"
            check(o[0], r64[0], r32[0], pdt, "adamw", f"p {what}")
            check(o[1], r64[1], r32[1], sdt, "adamw", f"exp_avg {what}")
            check(o[2], r64[2], r32[2], sdt, "adamw", f"exp_avg_sq {what}")
            z = (n + 7) // 8
            assert not o[1][:z].float().abs().any() and not o[2][:z].float().abs().any(), "untouched state stays zero"


def _pair_id(v):
    return _dt_id(v)


@gpu
@pytest.mark.parametrize("pdt,sdt", ADAMW_PAIRS, ids=_pair_id)
def test_adamw_single_steps(pdt, sdt):
    _run_adamw(pdt, sdt, True)


@gpu
@pytest.mark.parametrize("pdt,sdt", ADAMW_PAIRS, ids=_pair_id)
def test_adamw_bitwise_identities(pdt, sdt):
    """The comment of adamw_elem: the plain, non-temporal and lean instantiations, and the vector and
    the scalar path, round identically."""
    from lightning_thunder_amd.ops import require

    lib = require()
    step, wd = 7, 0.1
    tensors = _adamw_inputs(pdt, sdt, 1.0, "cuda", seed=3)

    def same(a, b, what):
        for n, x, y in zip(ADAMW_SIZES, a, b):
            for name, s, t in zip(("p", "exp_avg", "exp_avg_sq"), x, y):
                assert bits_equal(s, t), f"{what}: {name} of the tensor of {n} elements differs"

    old = lib.lta_adamw_set_nt(1)
    try:
        base = _adamw_launch(_clone(tensors), pdt, sdt, step, wd)
        assert not bits_equal(base[3][0], tensors[3][0]), "the launch must have updated the parameters"
        same(base, _adamw_launch(_clone(tensors, misalign=True), pdt, sdt, step, wd), "aligned (vector) against offset view (scalar)")
        same(base, _adamw_launch(_clone(tensors), pdt, sdt, step, wd, lean=True), "lean against plain")
        lib.lta_adamw_set_nt(0)
        same(base, _adamw_launch(_clone(tensors), pdt, sdt, step, wd), "non-temporal on against off")
    finally:
        lib.lta_adamw_set_nt(old)


# ------------------------------------------------------------------------------------------------
# every case above with the fp32 evaluation in place of the kernel (CPU)
# ------------------------------------------------------------------------------------------------
def test_fp32_evaluation_within_tolerance_cpu():
    """err / tol <= 1 for the plain fp32 evaluation of every case, rounded to the output type: every
    reference is finite on its inputs and no case leans on the tolerance."""
    for dtype in DTYPES:
        for name in NORM_FWD_NAMES:
            _run_rms_fwd(name, dtype, False)
            _run_ln_fwd(name, dtype, False)
        for name in NORM_BWD_NAMES:
            for rows, blocks in ROWS_BLOCKS:
                _run_rms_bwd(norm_bwd_cols(dtype)[name], rows, blocks, dtype, False, None, name)
                _run_ln_bwd(norm_bwd_cols(dtype)[name], rows, blocks, dtype, False, None, name)
        for rows, blocks, cols in MANY_BLOCKS:
            _run_rms_bwd(cols, rows, blocks, dtype, False, None, combos=((True, True),))
            _run_ln_bwd(cols, rows, blocks, dtype, False, None, combos=((True, True, True),))
        for n, kind, misalign in SWIGLU_CASES:
            _run_swiglu(n, dtype, False, kind, misalign)
        for vi in range(4):
            for reduction in ("none", "mean", "sum"):
                for ls in (0.0, 0.1):
                    x, t, _ = _ce_inputs(ce_vocabs(dtype)[vi], dtype, "cpu")
                    _run_ce(x, t, None, reduction, ls, dtype, False, CE_V_IDS[vi])
                    if vi in (1, 2) and dtype != F16:
                        for wdtype in (BF16, F32):
                            x, t, w = _ce_inputs(ce_vocabs(dtype)[vi], dtype, "cpu", weight_dtype=wdtype)
                            _run_ce(x, t, w, reduction, ls, dtype, False, CE_V_IDS[vi])
            _run_ce_row_stats(vi, dtype, False)
        x, t, _ = _ce_inputs(8, dtype, "cpu", rows=300)
        _run_ce(x, t, None, "mean", 0.0, dtype, False, "rows300")
        x, t, _ = _ce_inputs(1000, dtype, "cpu")
        _run_ce(x, torch.full_like(t, -100), None, "mean", 0.1, dtype, False, "all ignored")
        for vi in (2, 3):
            for pattern in CE_INF_PATTERNS:
                _run_ce_inf(vi, dtype, pattern, False)
    for name, dtype, kind in NORM_FWD_EXTRA:
        _run_ln_fwd(name, dtype, False, kind)
        _run_rms_fwd(name, dtype, False, kind)
    _run_swiglu(swiglu_grid_stride_n(BF16), BF16, False)
    for pdt, sdt in ADAMW_PAIRS:
        _run_adamw(pdt, sdt, False)
    assert max(_WORST.values()) <= 1.0
