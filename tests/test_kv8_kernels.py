"""The two kernels of the e4m3 KV cache against references built from the exactly dequantised bytes:

* ``decode_attn_kv8`` (csrc/decode_attention.hip, K/V element type uint8): the four launch shapes and the
  variations of ``test_decode_kernels.py``, the WSPLIT key edges, and the unpack of every e4m3 byte at
  every position of a 16-byte load, bit for bit;
* ``qkv_rope_cache_fwd`` with uint8 caches (csrc/rope.hip): written rows bitwise equal to
  ``clamp -> to(float8_e4m3fn) -> view(uint8)`` of ``qkv_rope_fwd``'s k / v, every other byte untouched.

The references read ``bytes.view(float8_e4m3fn).double()``, so quantisation error is part of no tolerance:
``assert_within`` applies with its formula ulp(T) |ref| + 8 e32 + 1e-6, the arithmetic after the unpack
being the 16-bit kernel's.
"""
import pytest
import torch

from kernel_checks import BF16, F16, F32, _dt_id, assert_within, bits_equal
from test_decode_kernels import (CACHE_POS, CACHE_S, PATH_SHAPES, VARIATIONS, _attn_case, _check_rising, _rope_inputs,
                                 ref_attention)

gpu = pytest.mark.gpu
U8, F8 = torch.uint8, torch.float8_e4m3fn

# Largest err / tol measured on MI355X, bf16 / fp16 (every run prints them with -s):
#   decode attention over e4m3   0.99 / 0.49   (rows4/hole, wsplit_split/causal_mask)
# as for the 16-bit kernel: 2^-8 |x| is the largest half-spacing of bf16, so a correctly rounded output
# sits at up to 1.0 of the first term alone (fp16: 0.5).  The RoPE writes and the unpack are bitwise.


def e4m3_bytes(t):
    return t.float().clamp(-448.0, 448.0).to(F8).view(U8)


def dequantised(b8):
    return b8.view(F8).float()  # exact: every e4m3 value is an fp32 (and a bf16, and an fp16) value


@pytest.fixture
def attn8_spy(monkeypatch):
    """Records every native e4m3 decode-attention launch as (wsplit, nsplit, q ptr, k ptr, v ptr)."""
    import lightning_thunder_amd.ops.attention  # noqa: F401  (registers the signature on the real entry first)
    from lightning_thunder_amd.ops import require

    lib = require()
    real = lib.lta_decode_attn_kv8
    calls = []

    def spy(*a):
        calls.append({"wsplit": bool(a[19]), "nsplit": int(a[16]), "q": a[1], "k": a[2], "v": a[3]})
        return real(*a)

    def never(*a):
        raise AssertionError("an e4m3 cache must not reach the 16-bit entry")

    monkeypatch.setattr(lib, "lta_decode_attn_kv8", spy)
    monkeypatch.setattr(lib, "lta_decode_attn", never)
    return calls


def _case8(B, Hq, Hkv, T, S, D, dtype, var, seed=0, delta=0.5):
    """``test_decode_kernels._attn_case`` with K / V quantised on the CPU (randn -> clamp -> to(f8))."""
    c = _attn_case(B, Hq, Hkv, T, S, D, dtype, var, seed=seed, delta=delta)
    c["k8"], c["v8"] = e4m3_bytes(c.pop("k")), e4m3_bytes(c.pop("v"))
    return c


def _run_attn8(c, dtype, expect, spy, what):
    from lightning_thunder_amd.ops.attention import decode_attn_kv8

    q, k8, v8 = c["q"].cuda(), c["k8"].cuda(), c["v8"].cuda()
    mask = None if c["mask"] is None else c["mask"].cuda()
    if c["views"]:
        B, Hq, T, D = q.shape
        S = k8.shape[2]
        # the slack rows hold bytes that would wreck the result if a key past S were read: 60.0 and -448.0
        kbuf = torch.full((B, k8.shape[1], S + 192, D), 0x67, device="cuda", dtype=U8)
        vbuf = torch.full((B, k8.shape[1], S + 192, D), 0xFE, device="cuda", dtype=U8)
        assert dequantised(kbuf[0, 0, 0, :1]).item() == 60.0 and dequantised(vbuf[0, 0, 0, :1]).item() == -448.0
        kbuf[:, :, :S], vbuf[:, :, :S] = k8, v8
        k8, v8 = kbuf[:, :, :S], vbuf[:, :, :S]
        q = q.transpose(1, 2).contiguous().transpose(1, 2)
        assert not k8.is_contiguous() and not v8.is_contiguous() and (T == 1 or not q.is_contiguous())
    k, v = dequantised(k8), dequantised(v8)
    if c.get("check_rising"):
        _check_rising(q, k, v, c["scale"])
    spy.clear()
    out = decode_attn_kv8(q, k8, v8, mask, c["causal"], c["scale"])
    assert len(spy) == 1, "decode_attn_kv8 must launch the native kernel exactly once"
    call = spy[0]
    assert (call["wsplit"], call["nsplit"] > 1) == expect, \
        f"{what}: expected (wsplit, split) = {expect}, launched wsplit={call['wsplit']} nsplit={call['nsplit']}"
    if c["views"]:  # read in place: no copy was made for the strided views
        assert (call["q"], call["k"], call["v"]) == (q.data_ptr(), k8.data_ptr(), v8.data_ptr())
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
    assert_within(out, ref64, ref32, dtype, "decode attention kv8", what)
    return out


@gpu
@pytest.mark.parametrize("dtype", [BF16, F16], ids=_dt_id)
@pytest.mark.parametrize("var", VARIATIONS)
@pytest.mark.parametrize("path", list(PATH_SHAPES))
def test_decode_attn_kv8_paths(path, var, dtype, attn8_spy):
    shape, expect = PATH_SHAPES[path]
    c = _case8(*shape, dtype, var)
    c["check_rising"] = var == "rising"
    _run_attn8(c, dtype, expect, attn8_spy, f"{path}/{var}")


@gpu
@pytest.mark.parametrize("dtype", [BF16, F16], ids=_dt_id)
@pytest.mark.parametrize("S", [1, 63, 64, 65, 255, 256, 257, 511, 512, 513])
def test_decode_attn_kv8_wsplit_key_edges(S, dtype, attn8_spy):
    c = _case8(1, 8, 2, 1, S, 128, dtype, "plain", seed=S)
    _run_attn8(c, dtype, (True, S >= 512), attn8_spy, f"S={S}")


def test_kv8_rising_max_construction_cpu():
    """The 'rising' inputs keep their property after K is quantised to e4m3 (checked on the CPU)."""
    for shape, _ in PATH_SHAPES.values():
        for dtype in (BF16, F16):
            c = _case8(*shape, dtype, "rising")
            _check_rising(c["q"], dequantised(c["k8"]), dequantised(c["v8"]), c["scale"])


def test_kv8_launch_shape_is_the_16_bit_one_cpu():
    """One function of (rows, S) picks wsplit / nsplit / chunk for both cache types."""
    from lightning_thunder_amd.ops.attention import decode_launch_shape

    for (B, Hq, _, T, S, _), (wsplit, split) in PATH_SHAPES.values():
        w, n, chunk = decode_launch_shape(B * Hq * T, S)
        assert (w, n > 1) == (wsplit, split) and chunk % 64 == 0 and n * chunk >= S > (n - 1) * chunk


# ------------------------------------------------------------------------------------------------
# the unpack, bit for bit
# ------------------------------------------------------------------------------------------------
UNPACK_SHAPE = (16, 1, 1, 16, 256)  # B, Hq, Hkv, T, S: 256 query rows, one per key


def _every_byte(S, D):
    """[S, D] uint8 with every finite e4m3 byte at every position d (so at every d mod 16): key s holds
    (s + 17 d) mod 256 at d, the two NaN codes replaced by zero."""
    s, d = torch.arange(S).view(S, 1), torch.arange(D).view(1, D)
    b = ((s + 17 * d) % 256).to(U8)
    finite = (b & 0x7F) != 0x7F
    for pos in range(16):
        seen = set(b[:, pos][finite[:, pos]].tolist())
        assert seen == set(range(256)) - {0x7F, 0xFF}
    return torch.where(finite, b, torch.zeros_like(b))


@gpu
@pytest.mark.parametrize("dtype", [BF16, F16], ids=_dt_id)
@pytest.mark.parametrize("D", [64, 128])
def test_decode_attn_kv8_unpacks_every_byte_exactly(D, dtype, attn8_spy):
    """A one-hot mask per query row: p = 1, l = 1, so the output row is the selected V row itself, and every
    e4m3 value is exact in bf16 and fp16: bitwise equality, the sign of -0 (byte 0x80) included."""
    from lightning_thunder_amd.ops.attention import decode_attn_kv8

    B, Hq, Hkv, T, S = UNPACK_SHAPE
    g = torch.Generator().manual_seed(D)
    v8 = _every_byte(S, D).view(1, 1, S, D).expand(B, Hkv, S, D).contiguous()
    k8 = e4m3_bytes(torch.randn(B, Hkv, S, D, generator=g))
    q = torch.randn(B, Hq, T, D, generator=g).to(dtype)
    key = (torch.arange(B).view(B, 1) * T + torch.arange(T).view(1, T))  # [B, T]: every key once
    mask = torch.zeros(B, Hq, T, S, dtype=torch.bool)
    mask[torch.arange(B).view(B, 1), 0, torch.arange(T).view(1, T), key] = True
    assert (mask.sum(-1) == 1).all() and sorted(key.flatten().tolist()) == list(range(S))
    out = decode_attn_kv8(q.cuda(), k8.cuda(), v8.cuda(), mask.cuda())
    assert len(attn8_spy) == 1 and not attn8_spy[0]["wsplit"] and attn8_spy[0]["nsplit"] == 1
    expect = v8[0, 0][key].view(B, 1, T, D).view(F8).to(dtype)
    assert not torch.isnan(expect.float()).any()
    assert (expect.view(torch.int16) == -32768).any(), "the expected rows hold a -0"
    assert bits_equal(out.cpu(), expect), "the kernel's unpack of an e4m3 byte is not the value of that byte"


@gpu
@pytest.mark.parametrize("dtype", [BF16, F16], ids=_dt_id)
@pytest.mark.parametrize("D", [64, 128])
def test_decode_attn_kv8_small_and_subnormal_keys(D, dtype, attn8_spy):
    """K uniform over the finite codes of magnitude below 2: all subnormals and both zeros occur."""
    B, Hq, Hkv, T, S = UNPACK_SHAPE
    g = torch.Generator().manual_seed(100 + D)
    k8 = torch.randint(0, 0x40, (B, Hkv, S, D), generator=g).to(U8) | (torch.randint(0, 2, (B, Hkv, S, D), generator=g).to(U8) << 7)
    assert dequantised(k8).abs().max().item() < 2 and set(k8.flatten().tolist()) == set(range(0x40)) | set(range(0x80, 0xC0))
    c = {"q": (4 * torch.randn(B, Hq, T, D, generator=g)).to(dtype), "k8": k8,
         "v8": e4m3_bytes(torch.randn(B, Hkv, S, D, generator=g)), "mask": None, "causal": False, "scale": D ** -0.5,
         "dead": None, "views": False}
    _run_attn8(c, dtype, (False, False), attn8_spy, f"small keys D={D}")


@gpu
def test_decode_attn_kv8_copies_what_it_cannot_read_in_place(attn8_spy):
    """Rows that are not 16-byte aligned (a view 8 bytes into a buffer) are copied, as for the 16-bit kernel."""
    from lightning_thunder_amd.ops.attention import decode_attn_kv8

    c = _case8(2, 8, 2, 2, 300, 128, BF16, "plain")
    q, k8, v8 = c["q"].cuda(), c["k8"].cuda(), c["v8"].cuda()
    kb = torch.empty(k8.numel() + 8, device="cuda", dtype=U8)
    k_off = kb[8:].view(k8.shape)
    k_off.copy_(k8)
    assert k_off.data_ptr() % 16 == 8
    out = decode_attn_kv8(q, k_off, v8)
    assert len(attn8_spy) == 1 and attn8_spy[0]["k"] != k_off.data_ptr() and attn8_spy[0]["v"] == v8.data_ptr()
    attn8_spy.clear()
    assert bits_equal(out, decode_attn_kv8(q, k8, v8))
    with pytest.raises(ValueError):
        decode_attn_kv8(q, k8.view(F8).to(BF16), v8)


# ------------------------------------------------------------------------------------------------
# RoPE into an e4m3 cache
# ------------------------------------------------------------------------------------------------
ROPE_POS = dict(CACHE_POS, prefill=list(range(8)))


def _byte_pattern(shape, seed):
    n = 1
    for s in shape:
        n *= s
    return ((torch.arange(n, device="cuda") * 7 + seed) % 251 + 1).to(U8).view(shape)


def _make_caches8(layout, B, ng, S, hs):
    """(kc, vc, [underlying buffers]) uint8, pre-filled with a non-zero byte pattern."""
    if layout == "contiguous":
        kb, vb = _byte_pattern((B, ng, S, hs), 1), _byte_pattern((B, ng, S, hs), 2)
        return kb, vb, [kb, vb]
    if layout == "slack":  # 8 slack rows per head and a pitch 64 bytes longer than a row
        kb, vb = _byte_pattern((B, ng, S + 8, hs + 64), 3), _byte_pattern((B, ng + 1, S + 8, hs + 8), 4)
        return kb[:, :, :S, :hs], vb[:, :ng, :S, :hs], [kb, vb]
    raise ValueError(layout)


def _rope8_inputs(B, S, T, nh, ng, hs, dtype, cos_dtype, seed):
    qkv, cos_all, sin_all, g = _rope_inputs(B, S, nh, ng, hs, hs, dtype, cos_dtype, seed=seed)
    qkv = qkv[:, :T].float()
    # a third of the entries at +-1e3 (saturation), a third at 1e-3 (subnormals, underflow to +-0)
    kind = torch.randint(0, 3, qkv.shape, device="cuda", generator=g)
    qkv = torch.where(kind == 0, qkv * 1e3, torch.where(kind == 1, qkv * 1e-3, qkv))
    return qkv.to(dtype).contiguous(), cos_all, sin_all


@gpu
@pytest.mark.parametrize("layout", ["contiguous", "slack"])
@pytest.mark.parametrize("pos_kind", list(ROPE_POS))
@pytest.mark.parametrize("same_cos", [False, True], ids=["cos_fp32", "cos_same"])
@pytest.mark.parametrize("dtype", [BF16, F16], ids=_dt_id)
@pytest.mark.parametrize("nh,ng,hs", [(4, 2, 64), (8, 2, 128)])
def test_qkv_rope_cache_fwd_kv8(nh, ng, hs, dtype, same_cos, pos_kind, layout, monkeypatch):
    from lightning_thunder_amd.ops import require
    from lightning_thunder_amd.ops.fused import qkv_rope_cache_fwd, qkv_rope_cache_supported, qkv_rope_fwd

    B, S = 2, CACHE_S
    pos = torch.tensor(ROPE_POS[pos_kind], device="cuda")
    T = pos.numel()
    qkv, cos_all, sin_all = _rope8_inputs(B, S, T, nh, ng, hs, dtype, dtype if same_cos else F32, seed=hs + T)
    cos, sin = cos_all[pos], sin_all[pos]
    kc, vc, bufs = _make_caches8(layout, B, ng, S, hs)
    before = [b.clone() for b in bufs]
    assert qkv_rope_cache_supported(qkv, kc, vc, pos, ng, hs, hs)
    lib = require()
    real, calls = lib.lta_qkv_rope_cache_fwd_kv8, []
    monkeypatch.setattr(lib, "lta_qkv_rope_cache_fwd_kv8", lambda *a: calls.append(a) or real(*a))
    q, kc2, vc2 = qkv_rope_cache_fwd(qkv, cos, sin, nh, ng, hs, hs, kc, vc, pos)
    assert len(calls) == 1 and (calls[0][6], calls[0][7]) == (kc.data_ptr(), vc.data_ptr())
    for got, src in ((kc2, kc), (vc2, vc)):
        assert got.data_ptr() == src.data_ptr() and got.stride() == src.stride() and got.dtype == U8
    q0, k0, v0 = qkv_rope_fwd(qkv, cos, sin, nh, ng, hs, hs)
    k8, v8 = e4m3_bytes(k0), e4m3_bytes(v0)
    assert bits_equal(q, q0)
    assert torch.equal(kc[:, :, pos], k8), "K rows must land at pos[t] as the unfused program's bytes"
    assert torch.equal(vc[:, :, pos], v8), "V rows must land at pos[t] as the unfused program's bytes"
    # saturation to +-448, never a NaN code; in v (a pure move of the inputs) subnormals and both zeros occur
    k_codes, v_codes = set(k8.flatten().tolist()), set(v8.flatten().tolist())
    assert not (k_codes | v_codes) & {0x7F, 0xFF} and {0x7E, 0xFE} <= k_codes
    assert {0x7E, 0xFE, 0x00, 0x80} <= v_codes and v_codes & {0x01, 0x81}
    kc_e, vc_e, bufs_e = _make_caches8(layout, B, ng, S, hs)
    kc_e[:, :, pos], vc_e[:, :, pos] = k8, v8
    for got, exp, old in zip(bufs, bufs_e, before):
        assert torch.equal(got, exp), "a store landed outside the rows at pos"
        assert not torch.equal(got, old)


@gpu
def test_qkv_rope_cache_kv8_unsupported_head_size():
    """hs = 96 is no row-kernel shape: the wrapper reports unsupported and the executor's fallback writes
    the bytes of the unfused program."""
    from lightning_thunder_amd.executors.hipex import _qkv_rope_cache_impl
    from lightning_thunder_amd.ops.fused import qkv_rope_cache_supported, qkv_rope_fwd

    B, S, nh, ng, hs, dtype = 2, CACHE_S, 4, 2, 96, BF16
    pos = torch.tensor(CACHE_POS["perm8"], device="cuda")
    qkv, cos_all, sin_all = _rope8_inputs(B, S, pos.numel(), nh, ng, hs, dtype, F32, seed=5)
    cos, sin = cos_all[pos], sin_all[pos]
    kc, vc, bufs = _make_caches8("contiguous", B, ng, S, hs)
    assert not qkv_rope_cache_supported(qkv, kc, vc, pos, ng, hs, hs)
    ok = _make_caches8("contiguous", B, ng, S, 64)
    assert not qkv_rope_cache_supported(qkv[..., :8 * 64].contiguous(), ok[0], ok[1], pos, ng, 64, 32), "partial rotation"
    q, kc2, vc2 = _qkv_rope_cache_impl(qkv, cos, sin, nh, ng, hs, hs, kc, vc, pos)
    assert kc2.data_ptr() == kc.data_ptr() and vc2.data_ptr() == vc.data_ptr()
    q0, k0, v0 = qkv_rope_fwd(qkv, cos, sin, nh, ng, hs, hs)
    kc_e, vc_e, _ = _make_caches8("contiguous", B, ng, S, hs)
    kc_e[:, :, pos], vc_e[:, :, pos] = e4m3_bytes(k0), e4m3_bytes(v0)
    assert bits_equal(q, q0) and torch.equal(kc, kc_e) and torch.equal(vc, vc_e)
    with pytest.raises(ValueError):
        _qkv_rope_cache_impl(qkv, cos, sin, nh, ng, hs, hs, kc, vc.view(torch.int8).to(dtype), pos)
