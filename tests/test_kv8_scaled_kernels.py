"""The two kernels of the scaled e4m3 KV cache (``ops/kv8.py``: e4m3 bytes plus one power-of-two scale byte per
row) against the plain-torch definition:

* ``decode_attn_kv8s`` (csrc/decode_attention.hip, scaled mode): the four launch shapes and the variations of
  ``test_decode_kernels.py``, the WSPLIT key edges, strided views and the shift property.  Every case is held
  twice: to fp64 over the exactly dequantised cache with ``assert_within`` (quantisation is in no tolerance), and
  bit for bit to the 16-bit kernel over ``dequantise_rows`` of the same bytes;
* ``qkv_rope_cache_fwd`` with scale caches (csrc/rope.hip, scaled mode): bytes and scale bytes bitwise equal to
  ``quantise_rows(qkv_rope_fwd(...))``, every other byte of all four caches untouched.

Inputs of the attention cases: V rows are ``randn * 2^u`` with ``u`` drawn per (head, key) row from -12 .. 6, and
so are the K rows except in the 'rising' variation, whose K keeps its construction (its rows span 2^-6 .. 2^3
by themselves).  q is scaled by 2^-4 next to such K so that every score stays within 60 of its row maximum (no
probability is an fp32 subnormal, which the bit-for-bit claim excludes); ``test_kv8s_scores_stay_in_range_cpu``
checks that for every case on the CPU.
"""
import pytest
import torch

from kernel_checks import BF16, F16, F32, _dt_id, assert_within, bits_equal
from test_decode_kernels import CACHE_POS, CACHE_S, PATH_SHAPES, VARIATIONS, _attn_case, _check_rising, ref_attention

from lightning_thunder_amd.ops.kv8 import dequantise_rows, quantise_rows

gpu = pytest.mark.gpu
U8 = torch.uint8
EDGE_S = [1, 63, 64, 65, 255, 256, 257, 511, 512, 513]


def _case8s(B, Hq, Hkv, T, S, D, dtype, var, seed=0):
    """``test_decode_kernels._attn_case`` with row magnitudes spread over 2^-12 .. 2^6 and K / V quantised on the
    CPU with ``quantise_rows``: adds k8, ks, v8, vs (the 16-bit k / v are dropped)."""
    c = _attn_case(B, Hq, Hkv, T, S, D, dtype, var, seed=seed)
    g = torch.Generator().manual_seed(1000 + seed)
    uk = torch.randint(-12, 7, (B, Hkv, S, 1), generator=g)
    uv = torch.randint(-12, 7, (B, Hkv, S, 1), generator=g)
    k, v = c.pop("k").float(), c.pop("v").float() * torch.exp2(uv.float())
    if var != "rising":
        k = k * torch.exp2(uk.float())
        c["q"] = (c["q"].float() * 2.0 ** -4).to(dtype)
    c["k8"], c["ks"] = quantise_rows(k.to(dtype))
    c["v8"], c["vs"] = quantise_rows(v.to(dtype))
    return c


def _all_cases():
    for path, (shape, _) in PATH_SHAPES.items():
        for var in VARIATIONS:
            for dtype in (BF16, F16):
                yield f"{path}/{var}/{_dt_id(dtype)}", _case8s(*shape, dtype, var), var
    for S in EDGE_S:
        for dtype in (BF16, F16):
            yield f"S={S}/{_dt_id(dtype)}", _case8s(1, 8, 2, 1, S, 128, dtype, "plain", seed=S), "plain"


def test_kv8s_scores_stay_in_range_cpu():
    """Every attention case: scales differ within 64-key blocks, the scores a row attends to lie within 60 of
    the row's maximum (so exp(s - max) >= 8.7e-27 is a normal fp32 and so is its product with any 2^e), and the
    'rising' cases keep their property after quantisation."""
    for what, c, var in _all_cases():
        k = dequantise_rows(c["k8"], c["ks"], torch.float64)
        q = c["q"].double()
        g = q.shape[1] // k.shape[1]
        s = torch.matmul(q, k.repeat_interleave(g, 1).transpose(-1, -2)) * c["scale"]
        T, S = s.shape[-2:]
        keep = torch.ones(s.shape, dtype=torch.bool)
        if c["causal"]:
            keep &= torch.ones(T, S, dtype=torch.bool).tril()
        if c["mask"] is not None:
            keep &= torch.broadcast_to(c["mask"], s.shape)
        top = s.masked_fill(~keep, float("-inf")).max(-1, keepdim=True).values
        live = keep & torch.isfinite(top)
        spread = (top - s)[live].max().item()
        assert spread <= 60.0, (what, spread)
        if S >= 64:
            for sc in (c["vs"],) if var == "rising" else (c["ks"], c["vs"]):
                assert len(set(sc[0, 0, :64, 0].tolist())) > 3, f"{what}: one scale per block would hide a wrong lane"
        assert int(c["ks"].min()) >= 112 and int(c["ks"].max()) <= 134
        if var == "rising":
            _check_rising(c["q"], dequantise_rows(c["k8"], c["ks"], F32), dequantise_rows(c["v8"], c["vs"], F32), c["scale"])


@pytest.fixture
def attn8s_spy(monkeypatch):
    """Records every native scaled-e4m3 decode-attention launch; the unscaled e4m3 entry must not be used, and
    the 16-bit entry only where the test itself asks for the reference kernel."""
    import lightning_thunder_amd.ops.attention  # noqa: F401  (registers the signatures on the real entries first)
    from lightning_thunder_amd.ops import require

    lib = require()
    real = lib.lta_decode_attn_kv8s
    calls = []

    def spy(*a):
        calls.append({"wsplit": bool(a[21]), "nsplit": int(a[18]), "q": a[1], "k": a[2], "v": a[3], "ks": a[4], "vs": a[5]})
        return real(*a)

    def never(*a):
        raise AssertionError("a scaled e4m3 cache must not reach the unscaled entry")

    monkeypatch.setattr(lib, "lta_decode_attn_kv8s", spy)
    monkeypatch.setattr(lib, "lta_decode_attn_kv8", never)
    return calls


def _run_attn8s(c, dtype, expect, spy, what):
    from lightning_thunder_amd.ops.attention import decode_attn, decode_attn_kv8s

    q = c["q"].cuda()
    k8, ks, v8, vs = (c[n].cuda() for n in ("k8", "ks", "v8", "vs"))
    mask = None if c["mask"] is None else c["mask"].cuda()
    if c["views"]:
        B, Hq, T, D = q.shape
        Hkv, S = k8.shape[1], k8.shape[2]
        # slack rows: the bytes of 60.0 and -448.0 under the largest scale, 2^7
        kbuf = torch.full((B, Hkv, S + 192, D), 0x67, device="cuda", dtype=U8)
        vbuf = torch.full((B, Hkv, S + 192, D), 0xFE, device="cuda", dtype=U8)
        ksbuf = torch.full((B, Hkv, S + 192, 1), 134, device="cuda", dtype=U8)
        vsbuf = torch.full((B, Hkv, S + 192, 1), 134, device="cuda", dtype=U8)
        kbuf[:, :, :S], vbuf[:, :, :S], ksbuf[:, :, :S], vsbuf[:, :, :S] = k8, v8, ks, vs
        k8, v8, ks, vs = kbuf[:, :, :S], vbuf[:, :, :S], ksbuf[:, :, :S], vsbuf[:, :, :S]
        q = q.transpose(1, 2).contiguous().transpose(1, 2)
        assert not k8.is_contiguous() and not ks.is_contiguous() and (T == 1 or not q.is_contiguous())
    spy.clear()
    out = decode_attn_kv8s(q, k8, v8, ks, vs, mask, c["causal"], c["scale"])
    assert len(spy) == 1, "decode_attn_kv8s must launch the native kernel exactly once"
    call = spy[0]
    assert (call["wsplit"], call["nsplit"] > 1) == expect, \
        f"{what}: expected (wsplit, split) = {expect}, launched wsplit={call['wsplit']} nsplit={call['nsplit']}"
    if c["views"]:  # read in place: no copy was made for the strided views
        assert (call["q"], call["k"], call["v"], call["ks"], call["vs"]) == \
            (q.data_ptr(), k8.data_ptr(), v8.data_ptr(), ks.data_ptr(), vs.data_ptr())
    assert out.dtype == dtype and out.shape == q.shape and out.is_contiguous()
    # 1. fp64 over the exactly dequantised cache
    k, v = dequantise_rows(k8, ks, F32), dequantise_rows(v8, vs, F32)
    ref64 = ref_attention(q, k, v, mask, c["causal"], c["scale"])
    ref32 = ref_attention(q, k, v, mask, c["causal"], c["scale"], torch.float32)
    # 2. the 16-bit kernel over the dequantised cache (exact in bf16 and fp16), bit for bit
    kd, vd = dequantise_rows(k8, ks, dtype), dequantise_rows(v8, vs, dtype)
    assert torch.equal(kd.float(), k) and torch.equal(vd.float(), v), "dequantised values must be exact in T"
    plain = decode_attn(q, kd, vd, mask, c["causal"], c["scale"])
    assert len(spy) == 1
    if c["dead"] is not None:
        D = q.shape[-1]
        dead = c["dead"]
        assert torch.isnan(ref64[dead]).all() and torch.isnan(ref64).sum().item() == D
        assert torch.isnan(out[dead]).all(), f"{what}: the fully masked row must be NaN"
        assert torch.isnan(out).sum().item() == D, f"{what}: NaN outside the fully masked row"
        assert torch.isnan(plain[dead]).all()
        out, plain, ref64, ref32 = out.clone(), plain.clone(), ref64.clone(), ref32.clone()
        out[dead], plain[dead], ref64[dead], ref32[dead] = 0, 0, 0, 0
    assert_within(out, ref64, ref32, dtype, "decode attention kv8s", what)
    assert bits_equal(out, plain), \
        f"{what}: {(out != plain).sum().item()} elements differ from the 16-bit kernel over the dequantised cache"
    return out


@gpu
@pytest.mark.parametrize("dtype", [BF16, F16], ids=_dt_id)
@pytest.mark.parametrize("var", VARIATIONS)
@pytest.mark.parametrize("path", list(PATH_SHAPES))
def test_decode_attn_kv8s_paths(path, var, dtype, attn8s_spy):
    shape, expect = PATH_SHAPES[path]
    _run_attn8s(_case8s(*shape, dtype, var), dtype, expect, attn8s_spy, f"{path}/{var}")


@gpu
@pytest.mark.parametrize("dtype", [BF16, F16], ids=_dt_id)
@pytest.mark.parametrize("S", EDGE_S)
def test_decode_attn_kv8s_wsplit_key_edges(S, dtype, attn8s_spy):
    c = _case8s(1, 8, 2, 1, S, 128, dtype, "plain", seed=S)
    _run_attn8s(c, dtype, (True, S >= 512), attn8s_spy, f"S={S}")


@gpu
@pytest.mark.parametrize("dtype", [BF16, F16], ids=_dt_id)
@pytest.mark.parametrize("path", ["rows4", "wsplit_split"])
def test_decode_attn_kv8s_value_shift(path, dtype, attn8s_spy):
    """V quantised from ``v * 2^-10`` has the same bytes and scale bytes 10 lower, and the kernel's output is
    2^-10 times the output for v, bit for bit (V rows of 2^8 randn: both exponents strictly inside [-15, 7])."""
    from lightning_thunder_amd.ops.attention import decode_attn_kv8s

    shape, _ = PATH_SHAPES[path]
    c = _case8s(*shape, dtype, "plain", seed=7)
    torch.manual_seed(11)
    v = ((torch.randn(c["v8"].shape) * 2.0 ** 10).round() / 4).to(dtype)  # multiples of 1/4: the shift is exact in T
    assert torch.equal((v.float() * 2.0 ** -10).to(dtype).float(), v.float() * 2.0 ** -10)
    (v8, vs), (v8b, vsb) = quantise_rows(v), quantise_rows((v.float() * 2.0 ** -10).to(dtype))
    assert torch.equal(v8, v8b) and torch.equal(vs.int() - 10, vsb.int()) and 112 < int(vsb.min()) and int(vs.max()) < 134
    q, k8, ks = c["q"].cuda(), c["k8"].cuda(), c["ks"].cuda()
    a = decode_attn_kv8s(q, k8, v8.cuda(), ks, vs.cuda(), None, False, c["scale"])
    b = decode_attn_kv8s(q, k8, v8b.cuda(), ks, vsb.cuda(), None, False, c["scale"])
    assert len(attn8s_spy) == 2 and a.float().abs().max().item() > 1.0
    # exact wherever T holds 2^-10 a exactly, i.e. outside fp16's subnormals (below 2^-14 a second rounding to
    # fp16's absolute spacing 2^-24 comes in: within one such step there)
    want, normal = a.float() * 2.0 ** -10, b.float().abs() >= torch.finfo(dtype).smallest_normal
    assert normal.float().mean().item() > 0.99 and (dtype == F16 or normal.all())
    assert torch.equal(want[normal], b.float()[normal])
    assert ((want - b.float()).abs()[~normal] <= 2.0 ** -24).all()


@gpu
def test_decode_attn_kv8s_refuses_malformed_scales():
    from lightning_thunder_amd.ops.attention import decode_attn_kv8s, decode_attn_kv8s_supported

    c = _case8s(2, 8, 2, 2, 100, 64, BF16, "plain")
    q, k8, v8, ks, vs = (c[n].cuda() for n in ("q", "k8", "v8", "ks", "vs"))
    assert decode_attn_kv8s_supported(q, k8, v8, ks, vs)
    for bad_ks in (ks[:, :, :99], ks.float(), ks.expand(2, 2, 100, 2), ks.cpu(), None):
        assert not decode_attn_kv8s_supported(q, k8, v8, bad_ks, vs)
        with pytest.raises(ValueError):
            decode_attn_kv8s(q, k8, v8, bad_ks, vs)
    assert not decode_attn_kv8s_supported(q[..., :32], k8[..., :32], v8[..., :32], ks, vs)  # head dim 32
    assert not decode_attn_kv8s_supported(q.expand(2, 8, 2, 64).repeat(1, 1, 9, 1), k8, v8, ks, vs)  # T = 18


# ------------------------------------------------------------------------------------------------
# RoPE into a scaled e4m3 cache
# ------------------------------------------------------------------------------------------------
ROPE_POS = {1: CACHE_POS["one"], 5: CACHE_POS["perm8"][:5]}


def _outlier_qkv(B, T, nh, ng, hs, dtype, seed):
    """qkv [B, T, (nh + 2 ng) hs]: every k / v head row is randn times a per-row power of two and carries one
    element 2^6 larger than the rest, whose index walks over all ``hs`` positions from row to row (a reduce
    that misses a lane then picks the wrong exponent).  One v row is all zero, one holds 60000 (saturates)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, T, nh + 2 * ng, hs, generator=g)
    rows = B * T * 2 * ng
    assert rows >= hs, "the outlier must visit every position"
    kv = x[:, :, nh:].reshape(rows, hs)
    r = torch.arange(rows)
    kv *= torch.exp2(((r % 11) - 6).float()).view(rows, 1)
    idx = (r * 5 + 3) % hs  # 5 is coprime to every head size here: all positions within any hs consecutive rows
    assert set(idx.tolist()) == set(range(hs))
    kv[r, idx] *= 64.0
    x[:, :, nh:] = kv.view(B, T, 2 * ng, hs)
    x[0, 0, nh + ng] = 0.0
    x[B - 1, T - 1, nh + 2 * ng - 1, hs // 2] = 60000.0
    return x.view(B, T, (nh + 2 * ng) * hs).to(dtype).cuda()


def _sentinel_caches(B, ng, S, hs):
    """Views [B, ng, S, hs] / [B, ng, S, 1] inside larger sentinel-filled buffers (0x5A bytes, 0 scales)."""
    kb = torch.full((B, ng, S + 8, hs + 64), 0x5A, device="cuda", dtype=U8)
    vb = torch.full((B, ng + 1, S + 8, hs + 8), 0x5A, device="cuda", dtype=U8)
    ksb = torch.zeros((B, ng, S + 8, 3), device="cuda", dtype=U8)
    vsb = torch.zeros((B, ng + 1, S, 1), device="cuda", dtype=U8)
    views = (kb[:, :, :S, :hs], vb[:, :ng, :S, :hs], ksb[:, :, :S, :1], vsb[:, :ng])
    return views, (kb, vb, ksb, vsb)


def _rope_cos_sin(S, hs, cos_dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(S, hs, generator=g) * 2 - 1).to(cos_dtype).cuda(),
            (torch.rand(S, hs, generator=g) * 2 - 1).to(cos_dtype).cuda())


def _check_rope_s8(nh, ng, hs, Tn, dtype, cos_dtype, monkeypatch):
    from lightning_thunder_amd.ops import require
    from lightning_thunder_amd.ops.fused import qkv_rope_cache_fwd, qkv_rope_cache_scaled_supported, qkv_rope_fwd

    S = CACHE_S
    B = max(2, -(-hs // (Tn * 2 * ng)))
    pos = torch.tensor(ROPE_POS[Tn], device="cuda")
    qkv = _outlier_qkv(B, Tn, nh, ng, hs, dtype, seed=hs + Tn)
    cos_all, sin_all = _rope_cos_sin(S, hs, cos_dtype, seed=hs)
    cos, sin = cos_all[pos], sin_all[pos]
    (kc, vc, ksc, vsc), bufs = _sentinel_caches(B, ng, S, hs)
    assert qkv_rope_cache_scaled_supported(qkv, kc, vc, ksc, vsc, pos, ng, hs, hs)
    lib = require()
    real, calls = lib.lta_qkv_rope_cache_fwd_kv8s, []
    monkeypatch.setattr(lib, "lta_qkv_rope_cache_fwd_kv8s", lambda *a: calls.append(a) or real(*a))
    q, *got = qkv_rope_cache_fwd(qkv, cos, sin, nh, ng, hs, hs, kc, vc, pos, k_scale=ksc, v_scale=vsc)
    assert len(calls) == 1 and tuple(calls[0][6:10]) == tuple(t.data_ptr() for t in (kc, vc, ksc, vsc))
    for g_, src in zip(got, (kc, vc, ksc, vsc)):
        assert g_.data_ptr() == src.data_ptr() and g_.stride() == src.stride() and g_.dtype == U8
    q0, k0, v0 = qkv_rope_fwd(qkv, cos, sin, nh, ng, hs, hs)
    (k8, ks), (v8, vs) = quantise_rows(k0), quantise_rows(v0)
    assert bits_equal(q, q0)
    assert torch.equal(ksc[:, :, pos], ks), "K scale bytes must be quantise_rows' at pos[t]"
    assert torch.equal(vsc[:, :, pos], vs), "V scale bytes must be quantise_rows' at pos[t]"
    assert torch.equal(kc[:, :, pos], k8), "K bytes must be quantise_rows' at pos[t]"
    assert torch.equal(vc[:, :, pos], v8), "V bytes must be quantise_rows' at pos[t]"
    # the inputs did what they are for: several exponents, the zero row's clamp, the saturating row
    assert len(set(ks.flatten().tolist())) > 4 and len(set(vs.flatten().tolist())) > 4
    assert int(vs[0, 0, 0]) == 112 and not v8[0, 0, 0].any()
    assert int(vs[-1, -1, -1]) == 134 and int(v8[-1, -1, -1, hs // 2]) == 0x7E
    (kc_e, vc_e, ksc_e, vsc_e), bufs_e = _sentinel_caches(B, ng, S, hs)
    kc_e[:, :, pos], vc_e[:, :, pos], ksc_e[:, :, pos], vsc_e[:, :, pos] = k8, v8, ks, vs
    for name, got_b, exp_b in zip(("k", "v", "k_scale", "v_scale"), bufs, bufs_e):
        assert torch.equal(got_b, exp_b), f"a store landed outside the rows at pos in the {name} cache"


@gpu
@pytest.mark.parametrize("same_cos", [False, True], ids=["cos_fp32", "cos_same"])
@pytest.mark.parametrize("dtype", [BF16, F16], ids=_dt_id)
@pytest.mark.parametrize("Tn", [1, 5])
@pytest.mark.parametrize("nh,ng", [(4, 4), (8, 2)])
@pytest.mark.parametrize("hs", [16, 32, 64, 128])
def test_qkv_rope_cache_fwd_kv8s(hs, nh, ng, Tn, dtype, same_cos, monkeypatch):
    _check_rope_s8(nh, ng, hs, Tn, dtype, dtype if same_cos else F32, monkeypatch)


@gpu
@pytest.mark.parametrize("dtype", [BF16, F16], ids=_dt_id)
@pytest.mark.parametrize("Tn", [1, 5])
def test_qkv_rope_cache_fwd_kv8s_second_trip_in_half_a_wave(Tn, dtype, monkeypatch):
    """nh = ng = 12 at hs = 128: 36 heads x 8 lanes = 288 items, so the item loop's second trip runs in the
    first 32 lanes of wave 0 (v heads), the rest of the workgroup inactive."""
    _check_rope_s8(12, 12, 128, Tn, dtype, F32, monkeypatch)


@gpu
@pytest.mark.parametrize("case", ["partial_rotation", "hs48", "fp32"])
def test_qkv_rope_cache_s8_unsupported_shapes_take_the_composite(case, monkeypatch):
    """Outside the row kernel's shapes the operator writes what the model's program writes, without a native
    scaled launch."""
    from lightning_thunder_amd.executors.hipex import _qkv_rope_cache_s8_impl
    from lightning_thunder_amd.ops import require
    from lightning_thunder_amd.ops.fused import qkv_rope_cache_scaled_supported, qkv_rope_fwd

    nh, ng, hs, rope_n, dtype = {"partial_rotation": (4, 2, 64, 32, BF16), "hs48": (4, 2, 48, 48, BF16),
                                 "fp32": (4, 2, 64, 64, F32)}[case]
    B, S, T = 2, CACHE_S, 5
    pos = torch.tensor(ROPE_POS[T], device="cuda")
    g = torch.Generator().manual_seed(3)
    qkv = (torch.randn(B, T, (nh + 2 * ng) * hs, generator=g) * 8).to(dtype).cuda()
    cos_all, sin_all = _rope_cos_sin(S, rope_n, F32, seed=4)
    cos, sin = cos_all[pos], sin_all[pos]
    kc, vc = (torch.full((B, ng, S, hs), 0x5A, device="cuda", dtype=U8) for _ in range(2))
    ksc, vsc = (torch.zeros((B, ng, S, 1), device="cuda", dtype=U8) for _ in range(2))
    assert not qkv_rope_cache_scaled_supported(qkv, kc, vc, ksc, vsc, pos, ng, hs, rope_n)
    lib = require()
    monkeypatch.setattr(lib, "lta_qkv_rope_cache_fwd_kv8s",
                        lambda *a: pytest.fail("an unsupported shape reached the native scaled entry"))
    q, *got = _qkv_rope_cache_s8_impl(qkv, cos, sin, nh, ng, hs, rope_n, kc, vc, ksc, vsc, pos)
    assert [t.data_ptr() for t in got] == [t.data_ptr() for t in (kc, vc, ksc, vsc)]
    q0, k0, v0 = qkv_rope_fwd(qkv, cos, sin, nh, ng, hs, rope_n)
    (k8, ks), (v8, vs) = quantise_rows(k0), quantise_rows(v0)
    exp = [torch.full_like(kc, 0x5A), torch.full_like(vc, 0x5A), torch.zeros_like(ksc), torch.zeros_like(vsc)]
    for e, rows in zip(exp, (k8, v8, ks, vs)):
        e[:, :, pos] = rows
    assert torch.equal(q, q0) and all(torch.equal(a, b) for a, b in zip((kc, vc, ksc, vsc), exp))
