"""The three decode-step kernels the other batteries only graze, against fp64 references written here:

* ``decode_attn`` (csrc/decode_attention.hip): all four (WSPLIT, split-K) launch shapes, pinned by a
  spy on the native entry so a change of the dispatch heuristic fails loudly;
* ``qkv_rope_fwd`` / ``qkv_rope_bwd`` / ``qkv_rope_cache_fwd`` (csrc/rope.hip): both kernels, more
  than one pass of the thread loop, the grid-stride loop, and the stores into a static KV cache;
* ``argmax_last`` (csrc/sampling.hip): odd vocabulary sizes that really reach the kernel (spy), ties,
  infinities and NaN.

Tolerance of every rounded output, per element:  ulp(T) * |ref64| + 8 * e32 + 1e-6.
``ulp`` is the spacing of T at 1 (2^-8 bf16, 2^-10 fp16, 2^-23 fp32): the single rounding of the
output.  ``e32`` is the largest error of a plain torch fp32 evaluation of the same reference formula on
the same inputs; the kernels accumulate in fp32, and the factor 8 covers their fast exp and their
summation order.  Pure moves (v heads, unrotated tail, cache rows, indices) are compared bitwise.

The references take the 16-bit inputs upcast exactly.  The random cos / sin tables have two different
halves on purpose: with a real RoPE table (both halves equal) a kernel that mixes them up is invisible.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from kernel_checks import ABS_FLOOR, BF16, F16, F32, ULP, _dt_id, assert_within, bits_equal

gpu = pytest.mark.gpu

# Largest err / tol measured on MI355X per group, bf16 / fp16 / fp32 (every run prints them with -s):
#   decode attention   0.99 / 0.49         (rows4/rising, rows4/leftpad)
#   RoPE fwd / bwd     1.00 / 0.50 / 0.07  (0.996: bwd hs128 rope32 cos=bf16)
#   RoPE into cache    0.99 / 0.49
# 2^-8 |x| is exactly the largest half-spacing of bf16 (reached just above a power of two), so a
# correctly rounded bf16 output sits at up to 1.0 of the first term alone; fp16 (spacing 2^-10 |x| at
# most, half of it the rounding) at up to 0.5.  No case needed more than the factor 8.


# ------------------------------------------------------------------------------------------------
# references
# ------------------------------------------------------------------------------------------------
def _attention_probs(q, k, v, mask, causal, scale, dtype):
    q, k, v = q.to(dtype), k.to(dtype), v.to(dtype)
    g = q.shape[1] // k.shape[1]
    k, v = k.repeat_interleave(g, dim=1), v.repeat_interleave(g, dim=1)
    T, S = q.shape[2], k.shape[2]
    s = torch.matmul(q, k.transpose(-1, -2)) * scale
    if causal:  # top-left aligned: query t sees keys 0..t
        keep = torch.ones(T, S, dtype=torch.bool, device=q.device).tril()
        s = s.masked_fill(~keep, float("-inf"))
    if mask is not None:
        s = s.masked_fill(~torch.broadcast_to(mask, s.shape), float("-inf"))
    return torch.softmax(s, dim=-1), s, v


def ref_attention(q, k, v, mask, causal, scale, dtype=torch.float64):
    """softmax(Q K^T * scale + mask) V; q [B, Hq, T, D], k / v [B, Hkv, S, D], bool mask (True = attend)
    broadcastable to [B, Hq, T, S].  A row with no key to attend to is NaN."""
    p, _, v = _attention_probs(q, k, v, mask, causal, scale, dtype)
    return torch.matmul(p, v)


def ref_qkv_rope(qkv, cos, sin, nh, ng, hs, rope_n, dtype=torch.float64):
    """qkv [B, T, (nh + 2 ng) hs] -> q [B, nh, T, hs], k, v [B, ng, T, hs]; rotate-half on the first
    ``rope_n`` dims of the q and k heads with cos / sin [T, rope_n]; v passes through."""
    B, T, _ = qkv.shape
    x = qkv.to(dtype).view(B, T, nh + 2 * ng, hs).transpose(1, 2)
    c, s = cos[:T].to(dtype), sin[:T].to(dtype)
    h = rope_n // 2

    def rot(u):
        r = u[..., :rope_n]
        turned = torch.cat((-r[..., h:], r[..., :h]), dim=-1)
        return torch.cat((r * c + turned * s, u[..., rope_n:]), dim=-1)

    return rot(x[:, :nh]), rot(x[:, nh:nh + ng]), x[:, nh + ng:]


def test_ref_attention_matches_sdpa_cpu():
    torch.manual_seed(0)
    B, Hq, Hkv, T, S, D = 2, 4, 2, 3, 11, 8
    q = torch.randn(B, Hq, T, D, dtype=torch.float64)
    k = torch.randn(B, Hkv, S, D, dtype=torch.float64)
    v = torch.randn(B, Hkv, S, D, dtype=torch.float64)
    kk, vv = k.repeat_interleave(Hq // Hkv, 1), v.repeat_interleave(Hq // Hkv, 1)
    mask = torch.rand(B, 1, T, S) > 0.4
    mask[..., 0] = True
    tril = torch.ones(T, S, dtype=torch.bool).tril()
    for m, causal, scale in ((None, False, D ** -0.5), (None, True, D ** -0.5), (mask, False, 0.3), (mask, True, 0.3)):
        ref = ref_attention(q, k, v, m, causal, scale)
        am = m if not causal else (tril if m is None else m & tril)
        exp = F.scaled_dot_product_attention(q, kk, vv, attn_mask=am, scale=scale)
        torch.testing.assert_close(ref, exp, atol=1e-12, rtol=1e-12)
        if m is None and causal:
            exp2 = F.scaled_dot_product_attention(q, kk, vv, is_causal=True, scale=scale)
            torch.testing.assert_close(ref, exp2, atol=1e-12, rtol=1e-12)
    # a row with nothing to attend to is NaN, every other row is not
    mask[1, 0, 2] = False
    ref = ref_attention(q, k, v, mask, False, 0.3)
    assert torch.isnan(ref[1, :, 2]).all() and torch.isnan(ref).sum().item() == Hq * D


def test_ref_qkv_rope_matches_litgpt_cpu():
    from lightning_thunder_amd.models.litgpt import qkv_split_rope

    torch.manual_seed(0)
    for nh, ng, hs, rope_n in ((4, 2, 16, 16), (3, 1, 32, 16)):
        B, T = 2, 5
        qkv = torch.randn(B, T, (nh + 2 * ng) * hs, dtype=torch.float64)
        cos, sin = torch.rand(T, rope_n, dtype=torch.float64) * 2 - 1, torch.rand(T, rope_n, dtype=torch.float64) * 2 - 1
        for a, b in zip(ref_qkv_rope(qkv, cos, sin, nh, ng, hs, rope_n), qkv_split_rope(qkv, cos, sin, nh, ng, hs, rope_n)):
            torch.testing.assert_close(a, b, atol=1e-14, rtol=1e-14)


# ------------------------------------------------------------------------------------------------
# A. decode attention
# ------------------------------------------------------------------------------------------------
@pytest.fixture
def attn_spy(monkeypatch):
    """Records every native decode-attention launch as (wsplit, nsplit, q ptr, k ptr, v ptr)."""
    import lightning_thunder_amd.ops.attention  # noqa: F401  (registers the signature on the real entry first)
    from lightning_thunder_amd.ops import require

    lib = require()
    real = lib.lta_decode_attn
    calls = []

    def spy(*a):
        calls.append({"wsplit": bool(a[19]), "nsplit": int(a[16]), "q": a[1], "k": a[2], "v": a[3]})
        return real(*a)

    monkeypatch.setattr(lib, "lta_decode_attn", spy)
    return calls


def _rising_inputs(B, Hq, Hkv, T, S, D, delta=0.5):
    """q scaled by 8 and k[j] = base + (j // 64) * delta * qhat: with scale D^-0.5 the score of every
    query row rises by 8 a delta (a in [0.75, 1.25]) from one 64-key block to the next."""
    qhat = F.normalize(torch.randn(B, Hkv, 1, D), dim=-1)
    a = 0.75 + 0.5 * torch.rand(B, Hq, T, 1)
    q = 8.0 * (math.sqrt(D) * a * qhat.repeat_interleave(Hq // Hkv, 1) + 0.5 * torch.randn(B, Hq, T, D))
    blk = (torch.arange(S) // 64).view(1, 1, S, 1).float()
    k = 0.02 * torch.randn(B, Hkv, S, D) + blk * delta * qhat
    return q, k


def _check_rising(q, k, v, scale):
    """The construction does what it says, on the exactly upcast inputs in fp64."""
    p, s, _ = _attention_probs(q, k, v, None, False, scale, torch.float64)
    assert torch.isfinite(s).all() and torch.isfinite(p).all()
    S = s.shape[-1]
    nblk = (S + 63) // 64
    pad = torch.full(s.shape[:-1] + (nblk * 64 - S,), float("-inf"), dtype=s.dtype, device=s.device)
    bmax = torch.cat((s, pad), -1).view(*s.shape[:-1], nblk, 64).max(-1).values
    assert (bmax[..., 1:] > bmax[..., :-1] + 0.5).all(), "the running maximum must rise with every block"
    assert p.max().item() < 1 - 1e-3, p.max().item()
    return bmax


VARIATIONS = ["plain", "views", "leftpad", "hole", "headoff", "tailoff", "causal_mask", "rising", "scale", "dead_row"]


def _attn_case(B, Hq, Hkv, T, S, D, dtype, var, seed=0, delta=0.5):
    """Inputs of one decode-attention case, built on the CPU (deterministic) in ``dtype``."""
    torch.manual_seed(seed)
    q = torch.randn(B, Hq, T, D)
    k = torch.randn(B, Hkv, S, D)
    v = torch.randn(B, Hkv, S, D)
    c = {"mask": None, "causal": False, "scale": D ** -0.5, "dead": None, "views": False}
    if var == "views":
        c["views"] = True
    elif var == "leftpad":  # [B, 1, T, S], another pad length per batch; batch 0 skips a whole 64-key block
        pad = 70 + (torch.arange(B) * 37) % 200
        c["mask"] = (torch.arange(S).view(1, 1, 1, S) >= pad.view(B, 1, 1, 1)).expand(B, 1, T, S).contiguous()
    elif var == "hole":  # [T, S]: two all-false 64-key blocks in the middle, ragged elsewhere
        m = torch.rand(T, S) > 0.2
        m[:, 64:192] = False
        m[:, 0] = True
        c["mask"] = m
    elif var == "headoff":  # [B, 1, 1, S]: nothing before S // 2 + 64, i.e. the whole first split is false
        m = torch.rand(B, 1, 1, S) > 0.2
        m[..., :S // 2 + 64] = False
        m[..., S - 2] = True
        c["mask"] = m
    elif var == "tailoff":  # [1, Hq, T, S]: nothing past S // 2, i.e. every later split is entirely false
        m = torch.rand(1, Hq, T, S) > 0.2
        m[..., S // 2:] = False
        m[..., 3] = True
        c["mask"] = m
    elif var == "causal_mask":
        m = torch.rand(B, 1, T, S) > 0.3
        m[..., 0] = True  # every causal row keeps key 0
        c["mask"], c["causal"] = m, True
    elif var == "rising":
        q, k = _rising_inputs(B, Hq, Hkv, T, S, D, delta)
    elif var == "scale":
        c["scale"] = 0.05
    elif var == "dead_row":
        m = torch.rand(B, Hq, T, S) > 0.2
        m[..., 1] = True
        dead = (B - 1, Hq // 2, T - 1)
        m[dead] = False
        c["mask"], c["dead"] = m, dead
    elif var != "plain":
        raise ValueError(var)
    c.update(q=q.to(dtype), k=k.to(dtype), v=v.to(dtype))
    return c


def _run_attn(c, dtype, expect, spy, what):
    from lightning_thunder_amd.ops.attention import decode_attn

    q, k, v = c["q"].cuda(), c["k"].cuda(), c["v"].cuda()
    mask = None if c["mask"] is None else c["mask"].cuda()
    if c["views"]:
        B, Hq, T, D = q.shape
        S = k.shape[2]
        # the slack rows hold values that would wreck the result if a key past S were read
        kbuf = torch.full((B, k.shape[1], S + 192, D), 60.0, device="cuda", dtype=dtype)
        vbuf = torch.full((B, k.shape[1], S + 192, D), -900.0, device="cuda", dtype=dtype)
        kbuf[:, :, :S], vbuf[:, :, :S] = k, v
        k, v = kbuf[:, :, :S], vbuf[:, :, :S]
        qbuf = q.transpose(1, 2).contiguous()  # [B, T, Hq, D]
        q = qbuf.transpose(1, 2)
        assert not k.is_contiguous() and not v.is_contiguous() and (T == 1 or not q.is_contiguous())
    if c.get("check_rising"):
        _check_rising(q, k, v, c["scale"])
    spy.clear()
    out = decode_attn(q, k, v, mask, c["causal"], c["scale"])
    assert len(spy) == 1, "decode_attn must launch the native kernel exactly once"
    call = spy[0]
    assert (call["wsplit"], call["nsplit"] > 1) == expect, \
        f"{what}: expected (wsplit, split) = {expect}, launched wsplit={call['wsplit']} nsplit={call['nsplit']}"
    if c["views"]:  # read in place: no copy was made for the strided views
        assert (call["q"], call["k"], call["v"]) == (q.data_ptr(), k.data_ptr(), v.data_ptr())
    assert out.dtype == dtype and out.shape == q.shape and out.is_contiguous()
    ref64 = ref_attention(q, k, v, mask, c["causal"], c["scale"])
    ref32 = ref_attention(q, k, v, mask, c["causal"], c["scale"], torch.float32)
    if c["dead"] is not None:
        D = q.shape[-1]
        dead = c["dead"]
        assert torch.isnan(ref64[dead]).all() and torch.isnan(ref64).sum().item() == D
        assert torch.isnan(out[dead]).all(), f"{what}: the fully masked row must be NaN"
        assert torch.isnan(out).sum().item() == D, f"{what}: NaN outside the fully masked row"
        out, ref64, ref32 = out.clone(), ref64.clone(), ref32.clone()
        out[dead], ref64[dead], ref32[dead] = 0, 0, 0
    assert_within(out, ref64, ref32, dtype, "decode attention", what)


# (B, Hq, Hkv, T, S, D) -> expected (WSPLIT kernel, split-K + combine)
PATH_SHAPES = {
    "rows4": ((4, 8, 2, 8, 300, 64), (False, False)),          # rows = 256: four rows per block, one split
    "rows4_split": ((43, 6, 3, 1, 520, 64), (False, True)),    # rows = 258: last block half empty, blocks span batches
    "wsplit": ((2, 8, 2, 2, 300, 128), (True, False)),         # rows = 32: one row per block, waves split the keys
    "wsplit_split": ((2, 8, 2, 2, 600, 128), (True, True)),    # ... and split-K + combine on top
}


@gpu
@pytest.mark.parametrize("dtype", [BF16, F16], ids=_dt_id)
@pytest.mark.parametrize("var", VARIATIONS)
@pytest.mark.parametrize("path", list(PATH_SHAPES))
def test_decode_attn_paths(path, var, dtype, attn_spy):
    shape, expect = PATH_SHAPES[path]
    c = _attn_case(*shape, dtype, var)
    c["check_rising"] = var == "rising"
    _run_attn(c, dtype, expect, attn_spy, f"{path}/{var}")


@gpu
@pytest.mark.parametrize("dtype", [BF16, F16], ids=_dt_id)
@pytest.mark.parametrize("var", ["plain", "views", "headoff", "tailoff", "rising"])
def test_decode_attn_batch8_llama_split(var, dtype, attn_spy):
    # batch-8 decode of a 32-head model: four rows per block, four splits of 256 keys plus the combine.
    # 'rising' with delta = 1.5: a score step of >= 1.5 * 5.5 per block, 12 blocks between the maxima of
    # the first and the last split, so they differ by more than ln(FLT_MAX) = 88.7 and a combine that
    # does not rescale by the maximum over all splits overflows.
    c = _attn_case(8, 32, 8, 1, 1024, 128, dtype, var, delta=1.5)
    c["check_rising"] = var == "rising"
    _run_attn(c, dtype, (False, True), attn_spy, f"batch8/{var}")


@gpu
@pytest.mark.parametrize("dtype", [BF16, F16], ids=_dt_id)
@pytest.mark.parametrize("S", [1, 63, 64, 65, 255, 256, 257, 511, 512, 513])
def test_decode_attn_wsplit_key_edges(S, dtype, attn_spy):
    # single-key softmax, the 64-key block edge and the S // 256 split threshold
    c = _attn_case(1, 8, 2, 1, S, 128, dtype, "plain", seed=S)
    _run_attn(c, dtype, (True, S >= 512), attn_spy, f"S={S}")
    if S > 64:
        c = _attn_case(1, 8, 2, 1, S, 128, dtype, "rising", seed=S)
        c["check_rising"] = True
        _run_attn(c, dtype, (True, S >= 512), attn_spy, f"S={S}/rising")


def test_rising_max_construction_cpu():
    """The 'rising' inputs on the CPU: finite fp64 scores, a block maximum that rises with every
    64-key block for every query row, and no probability within 1e-3 of one."""
    shapes = [(s, 0.5) for s, _ in PATH_SHAPES.values()] + [((1, 8, 2, 1, 65, 128), 0.5), ((1, 8, 2, 1, 513, 128), 0.5),
                                                            ((8, 32, 8, 1, 1024, 128), 1.5)]
    for shape, delta in shapes:
        for dtype in (BF16, F16):
            c = _attn_case(*shape, dtype, "rising", delta=delta)
            bmax = _check_rising(c["q"], c["k"], c["v"], c["scale"])
            assert bmax.shape[-1] == (shape[4] + 63) // 64


# ------------------------------------------------------------------------------------------------
# B. RoPE and RoPE into the cache
# ------------------------------------------------------------------------------------------------
def _rope_inputs(B, T, nh, ng, hs, rope_n, dtype, cos_dtype, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    qkv = torch.randn(B, T, (nh + 2 * ng) * hs, device="cuda", generator=g).to(dtype)
    cos = (torch.rand(T, rope_n, device="cuda", generator=g) * 2 - 1).to(cos_dtype)
    sin = (torch.rand(T, rope_n, device="cuda", generator=g) * 2 - 1).to(cos_dtype)
    return qkv, cos, sin, g


def _rope_fwd_bwd(B, T, nh, ng, hs, rope_n, dtype, cos_dtype, adjoint=True):
    from lightning_thunder_amd.ops.fused import qkv_rope_bwd, qkv_rope_fwd

    qkv, cos, sin, g = _rope_inputs(B, T, nh, ng, hs, rope_n, dtype, cos_dtype)
    what = f"nh{nh} ng{ng} hs{hs} rope{rope_n} cos={_dt_id(cos_dtype)}"
    out = qkv_rope_fwd(qkv, cos, sin, nh, ng, hs, rope_n)
    ref32 = ref_qkv_rope(qkv, cos, sin, nh, ng, hs, rope_n, torch.float32)
    x64 = qkv.double().requires_grad_(True)
    ref64 = ref_qkv_rope(x64, cos, sin, nh, ng, hs, rope_n)
    for name, o, r64, r32 in zip("qkv", out, ref64, ref32):
        assert o.dtype == dtype and o.is_contiguous()
        assert_within(o, r64.detach(), r32, dtype, "rope fwd/bwd", f"fwd {name} {what}")
    heads = qkv.view(B, T, nh + 2 * ng, hs).transpose(1, 2)
    assert bits_equal(out[2], heads[:, nh + ng:]), "v is a pure move"
    if rope_n < hs:
        assert bits_equal(out[0][..., rope_n:], heads[:, :nh, :, rope_n:]), "unrotated tail of q is a pure move"
        assert bits_equal(out[1][..., rope_n:], heads[:, nh:nh + ng, :, rope_n:]), "unrotated tail of k is a pure move"

    grads = [torch.randn(o.shape, device="cuda", generator=g).to(dtype) for o in out]
    dqkv = qkv_rope_bwd(*grads, cos, sin, nh, ng, hs, rope_n)
    assert dqkv.dtype == dtype and dqkv.shape == qkv.shape
    torch.autograd.backward(ref64, [t.double() for t in grads])
    x32 = qkv.float().requires_grad_(True)
    torch.autograd.backward(ref_qkv_rope(x32, cos, sin, nh, ng, hs, rope_n, torch.float32), [t.float() for t in grads])
    assert_within(dqkv, x64.grad, x32.grad, dtype, "rope fwd/bwd", f"bwd {what}")
    dheads = dqkv.view(B, T, nh + 2 * ng, hs).transpose(1, 2)
    assert bits_equal(dheads[:, nh + ng:], grads[2]), "dv is a pure move"
    if rope_n < hs:
        assert bits_equal(dheads[:, :nh, :, rope_n:], grads[0][..., rope_n:])
        assert bits_equal(dheads[:, nh:nh + ng, :, rope_n:], grads[1][..., rope_n:])

    if adjoint:
        # <bwd(g), x> = <g, fwd(x)> exactly; each kernel output carries one rounding of relative size
        # <= ulp / 2, so the two sums differ by at most ulp / 2 * (sum |bwd x| + sum |g fwd|) plus
        # the fp32 slack of the element tolerance on every term.
        x = qkv.double()
        lhs_terms = dqkv.double() * x
        rhs_terms = torch.cat([(gr.double() * o.double()).flatten() for gr, o in zip(grads, out)])
        lhs, rhs = lhs_terms.sum().item(), rhs_terms.sum().item()
        bound = 0.5 * ULP[dtype] * (lhs_terms.abs().sum().item() + rhs_terms.abs().sum().item()) \
            + ABS_FLOOR * (x.abs().sum().item() + sum(t.double().abs().sum().item() for t in grads))
        print(f"[rope adjoint {_dt_id(dtype)}] {what} |lhs-rhs|={abs(lhs - rhs):.3e} bound={bound:.3e}")
        assert abs(lhs - rhs) <= bound, (lhs, rhs, bound)


ROPE_SHAPES = [
    (32, 8, 128, 128),  # row kernel, 384 items: the 256-thread loop makes two passes
    (8, 4, 256, 256),   # row kernel, 16 pairs per head
    (6, 2, 96, 96),     # generic kernel (6 pairs: not a power of two)
    (4, 2, 80, 80),     # generic kernel
    (4, 2, 128, 32),    # partial rotation (generic kernel)
]


@gpu
@pytest.mark.parametrize("same_cos", [False, True], ids=["cos_fp32", "cos_same"])
@pytest.mark.parametrize("dtype", [BF16, F16], ids=_dt_id)
@pytest.mark.parametrize("nh,ng,hs,rope_n", ROPE_SHAPES)
def test_qkv_rope_fwd_bwd_fp64(nh, ng, hs, rope_n, dtype, same_cos):
    _rope_fwd_bwd(2, 5, nh, ng, hs, rope_n, dtype, dtype if same_cos else F32)


@gpu
@pytest.mark.parametrize("nh,ng,hs,rope_n", [(6, 2, 96, 96), (4, 2, 80, 80)])
def test_qkv_rope_fwd_bwd_fp64_fp32(nh, ng, hs, rope_n):
    _rope_fwd_bwd(2, 5, nh, ng, hs, rope_n, F32, F32)


@gpu
def test_qkv_rope_generic_grid_stride():
    # 2 * 2048 * 32 * 12 = 1.57 M work items > 4096 * 256: every thread of the capped grid loops
    _rope_fwd_bwd(2, 2048, 16, 8, 96, 96, BF16, F32, adjoint=False)


CACHE_S = 64
CACHE_POS = {
    "one": [37],
    "perm8": [5, 2, 9, 40, 0, 63, 17, 33],
    "ends": [CACHE_S - 1, 0, CACHE_S // 2],
}


def _pattern(shape, dtype, seed):
    """A deterministic non-zero fill (exact in bf16 and fp16), different for every element nearby."""
    n = math.prod(shape)
    return (((torch.arange(n, device="cuda") * 7 + seed) % 251).float() / 8 + 1).to(dtype).view(shape)


def _make_caches(layout, B, ng, S, hs, dtype):
    """(kc, vc, [underlying buffers]) pre-filled with a non-zero pattern."""
    if layout == "contiguous":
        kb, vb = _pattern((B, ng, S, hs), dtype, 1), _pattern((B, ng, S, hs), dtype, 2)
        return kb, vb, [kb, vb]
    if layout == "one_buffer":  # another base, equal strides
        buf = _pattern((B, 2, ng, S, hs), dtype, 3)
        return buf[:, 0], buf[:, 1], [buf]
    if layout == "slack_head":  # K is a [:, :ng] slice: another batch stride than V
        kb, vb = _pattern((B, ng + 1, S, hs), dtype, 4), _pattern((B, ng, S, hs), dtype, 5)
        return kb[:, :ng], vb, [kb, vb]
    if layout == "v_token_major":  # V stored [B, S, ng, hs]: another token and head stride than K
        kb, vb = _pattern((B, ng, S, hs), dtype, 6), _pattern((B, S, ng, hs), dtype, 7)
        return kb, vb.transpose(1, 2), [kb, vb]
    raise ValueError(layout)


@gpu
@pytest.mark.parametrize("layout", ["contiguous", "one_buffer", "slack_head", "v_token_major"])
@pytest.mark.parametrize("pos_kind", list(CACHE_POS))
@pytest.mark.parametrize("dtype", [BF16, F16], ids=_dt_id)
@pytest.mark.parametrize("hs", [64, 128, 96])
def test_qkv_rope_cache_fwd(hs, dtype, pos_kind, layout):
    from lightning_thunder_amd.ops.fused import qkv_rope_cache_fwd, qkv_rope_cache_supported, qkv_rope_fwd

    B, nh, ng, S = 2, 4, 2, CACHE_S
    pos = torch.tensor(CACHE_POS[pos_kind], device="cuda")
    T = pos.numel()
    qkv, cos_all, sin_all, _ = _rope_inputs(B, S, nh, ng, hs, hs, dtype, F32, seed=hs + T)
    qkv = qkv[:, :T].contiguous()
    cos, sin = cos_all[pos], sin_all[pos]  # gathered at the positions, as the models do
    kc, vc, bufs = _make_caches(layout, B, ng, S, hs, dtype)
    before = [b.clone() for b in bufs]
    assert qkv_rope_cache_supported(qkv, kc, vc, pos, ng, hs)
    q, kc2, vc2 = qkv_rope_cache_fwd(qkv, cos, sin, nh, ng, hs, hs, kc, vc, pos)
    for got, src in ((kc2, kc), (vc2, vc)):
        assert got.data_ptr() == src.data_ptr() and got.stride() == src.stride() and got.shape == src.shape
    q0, k0, v0 = qkv_rope_fwd(qkv, cos, sin, nh, ng, hs, hs)
    assert bits_equal(q, q0)
    assert bits_equal(kc[:, :, pos], k0), "K rows must land at pos[t]"
    assert bits_equal(vc[:, :, pos], v0), "V rows must land at pos[t]"
    r64 = ref_qkv_rope(qkv, cos, sin, nh, ng, hs, hs)
    r32 = ref_qkv_rope(qkv, cos, sin, nh, ng, hs, hs, torch.float32)
    what = f"hs{hs} {pos_kind} {layout}"
    assert_within(q, r64[0], r32[0], dtype, "rope into cache", f"q {what}")
    assert_within(kc[:, :, pos], r64[1], r32[1], dtype, "rope into cache", f"k {what}")
    assert bits_equal(vc[:, :, pos], r64[2].to(dtype)), "v is a pure move"
    # every byte outside the written rows is as before: other rows, the slack head, the other cache
    kc_e, vc_e, bufs_e = _make_caches(layout, B, ng, S, hs, dtype)
    kc_e[:, :, pos], vc_e[:, :, pos] = k0, v0
    assert len(bufs) == len(bufs_e) == len(before)
    for got, exp, old in zip(bufs, bufs_e, before):
        assert bits_equal(got, exp), "a store landed outside the rows at pos"
        assert not bits_equal(got, old)


@gpu
@pytest.mark.parametrize("hs", [64, 96])
def test_qkv_rope_cache_unsupported(hs):
    from lightning_thunder_amd.executors.hipex import _qkv_rope_cache_impl
    from lightning_thunder_amd.ops.fused import qkv_rope_cache_supported

    dtype, B, nh, ng, S = BF16, 2, 4, 2, CACHE_S
    pos = torch.tensor(CACHE_POS["perm8"], device="cuda")
    T = pos.numel()
    qkv, cos_all, sin_all, _ = _rope_inputs(B, S, nh, ng, hs, hs, dtype, F32, seed=11)
    qkv = qkv[:, :T].contiguous()
    cos, sin = cos_all[pos], sin_all[pos]
    fill_k, fill_v = _pattern((B, ng, S, hs), dtype, 1), _pattern((B, ng, S, hs), dtype, 2)
    n = fill_k.numel()

    def aligned():
        return fill_k.clone(), fill_v.clone()

    def offset4():  # views that start 8 bytes into a buffer: rows are not 16-byte aligned
        kb, vb = torch.empty(n + 4, device="cuda", dtype=dtype), torch.empty(n + 4, device="cuda", dtype=dtype)
        kc, vc = kb[4:].view(B, ng, S, hs), vb[4:].view(B, ng, S, hs)
        kc.copy_(fill_k)
        vc.copy_(fill_v)
        assert kc.data_ptr() % 16 == 8
        return kc, vc

    kc, vc = aligned()
    assert qkv_rope_cache_supported(qkv, kc, vc, pos, ng, hs)
    q_ok, k_ok, v_ok = _qkv_rope_cache_impl(qkv, cos, sin, nh, ng, hs, hs, kc, vc, pos)
    assert not bits_equal(k_ok, fill_k) and not bits_equal(v_ok, fill_v)

    assert not qkv_rope_cache_supported(qkv, *offset4(), pos, ng, hs)
    assert not qkv_rope_cache_supported(qkv, *aligned(), pos.int(), ng, hs)
    assert not qkv_rope_cache_supported(qkv, kc.to(F16), vc.to(F16), pos, ng, hs)
    assert not qkv_rope_cache_supported(qkv, kc, vc.float(), pos, ng, hs)
    big_k, big_v = fill_k.repeat(2, 1, 1, 1)[:B + 1], fill_v.repeat(2, 1, 1, 1)[:B + 1]
    assert not qkv_rope_cache_supported(qkv, big_k, big_v, pos, ng, hs)

    # the fallback of the executor gives what the fused launch gives
    for kc_u, vc_u, p in (offset4() + (pos,), aligned() + (pos.int(),)):
        q_u, k_u, v_u = _qkv_rope_cache_impl(qkv, cos, sin, nh, ng, hs, hs, kc_u, vc_u, p)
        assert k_u.data_ptr() == kc_u.data_ptr() and v_u.data_ptr() == vc_u.data_ptr()
        assert bits_equal(q_u, q_ok) and bits_equal(k_u, k_ok) and bits_equal(v_u, v_ok)


# ------------------------------------------------------------------------------------------------
# C. argmax
# ------------------------------------------------------------------------------------------------
@pytest.fixture
def argmax_spy(monkeypatch):
    import lightning_thunder_amd.ops.sampling  # noqa: F401  (registers the signature on the real entry first)
    from lightning_thunder_amd.ops import require

    lib = require()
    real = lib.lta_argmax_rows
    calls = []

    def spy(*a):
        calls.append(a)
        return real(*a)

    monkeypatch.setattr(lib, "lta_argmax_rows", spy)
    return calls


ARGMAX_THREADS = 1024  # one workgroup per row; thread c % 1024 owns 16-byte vector c


def _argmax_scenarios(V, nv):
    """(name, {index: value} to plant in one row, expected index) for a row of V values read as
    vectors of ``nv``.  Values beyond the random base (|x| <= 4) decide the result."""
    nvec = V // nv
    body, tail = nvec * nv, V - nvec * nv
    inf, nan = float("inf"), float("nan")
    sc = [("max_at_0", {0: 100.0}, 0), ("max_at_last", {V - 1: 100.0}, V - 1)]
    if nvec >= 1:
        sc.append(("max_in_last_full_vector", {body - nv + (1 if nv > 1 else 0): 100.0}, body - nv + (1 if nv > 1 else 0)))
    if tail:
        sc.append(("max_in_tail", {body: 100.0}, body))
    if nvec >= 1 and tail:
        sc.append(("tie_body_tail", {body - 1: 50.0, V - 1: 50.0}, body - 1))
    if nvec > ARGMAX_THREADS + 5:
        # vector 70 belongs to wave 1, vector 1024 + 5 to wave 0: the larger index sits in the wave
        # whose result the final scan starts from
        sc.append(("tie_two_waves", {70 * nv + 1: 50.0, (ARGMAX_THREADS + 5) * nv: 50.0}, 70 * nv + 1))
        # vectors 5 and 1024 + 5 are consecutive loads of thread 5
        sc.append(("tie_same_lane", {5 * nv + 2: 50.0, (ARGMAX_THREADS + 5) * nv + 2: 50.0}, 5 * nv + 2))
    if V >= 2:
        sc.append(("tie_neighbours", {V - 2: 50.0, V - 1: 50.0}, V - 2))
    if V >= 3:
        sc.append(("pos_inf", {V // 2: inf, V - 1: inf, 0: 100.0}, V // 2))
        sc.append(("one_nan", {V // 3: nan, 0: inf}, V // 3))  # NaN beats +inf, as in torch.argmax
        sc.append(("two_nans", {V // 3: nan, V - 1: nan, 0: inf}, V // 3))  # the first NaN wins
    else:
        sc.append(("pos_inf", {V - 1: inf}, V - 1))
        sc.append(("one_nan", {V - 1: nan}, V - 1))
    return sc


@gpu
@pytest.mark.parametrize("dtype", [BF16, F16, F32], ids=_dt_id)
@pytest.mark.parametrize("R", [1, 3])
@pytest.mark.parametrize("V", [1, 7, 8, 9, 32003, 65536 + 8, 128256 + 3])
def test_argmax_kernel_exact(V, R, dtype, argmax_spy):
    from lightning_thunder_amd.ops.sampling import argmax_last

    g = torch.Generator().manual_seed(V * 8 + R)
    ld = (V + 8) // 8 * 8  # row stride: a multiple of 8 elements, so an odd V still runs the kernel
    nv = 16 // torch.empty(0, dtype=dtype).element_size()

    def run(rows, what, expect=None):
        """rows [R, V] fp32 on the CPU -> kernel result on buf[:, :V]; exact against torch.argmax."""
        buf = torch.full((R, ld), 1000.0, dtype=dtype)  # the slack would win if it were read
        buf[:, :V] = rows.to(dtype)
        x = buf.cuda()[:, :V]
        assert x.stride(0) == ld and x.data_ptr() % 16 == 0
        n = len(argmax_spy)
        got = argmax_last(x)
        assert len(argmax_spy) == n + 1, f"{what}: the kernel was not launched"
        ref = torch.argmax(x.cpu().float(), dim=-1)
        assert got.dtype == torch.int64 and got.shape == (R,)
        assert torch.equal(got.cpu(), ref), f"{what}: {got.tolist()} != {ref.tolist()}"
        if expect is not None:
            r, idx = expect
            assert got[r].item() == idx, f"{what}: row {r} gave {got[r].item()}, planted {idx}"
        gk = argmax_last(x, keepdim=True)
        assert gk.shape == (R, 1) and torch.equal(gk[:, 0], got)

    base = torch.randn(R, V, generator=g).clamp_(-4, 4)
    run(base, "random")
    run(-base.abs() - 1, "negative only")
    for i, (name, plant, idx) in enumerate(_argmax_scenarios(V, nv)):
        rows = base.clone()
        r = i % R
        for j, val in plant.items():
            rows[r, j] = val
        run(rows, name, (r, idx))
    rows = base.clone()
    rows[R - 1] = float("-inf")
    run(rows, "all -inf", (R - 1, 0))


@gpu
@pytest.mark.parametrize("dtype", [BF16, F32], ids=_dt_id)
def test_argmax_falls_back_on_unaligned_rows(dtype, argmax_spy):
    from lightning_thunder_amd.ops.sampling import argmax_last

    torch.manual_seed(0)
    x = torch.randn(3, 32003, device="cuda").to(dtype)  # row stride 32003: rows are not 16-byte aligned
    x[1, 77] = x[1, 30000] = 50.0
    got = argmax_last(x)
    assert len(argmax_spy) == 0, "rows that are not 16-byte aligned must not reach the kernel"
    assert torch.equal(got.cpu(), torch.argmax(x.cpu().float(), dim=-1)) and got[1].item() == 77
