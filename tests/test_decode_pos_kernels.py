"""The kernels of a ragged batch, where every sequence sits at its own position:

* the position mode of the decode-attention kernels (csrc/decode_attention.hip; ``decode_attn_pos``,
  ``decode_attn_kv8_pos``, ``decode_attn_kv8s_pos``): row (b, hq, t) attends keys ``0 .. n-1`` with
  ``n = clamp(pos[b, t] + 1, 0, S)``, no mask tensor.  Every case against fp64 with ``assert_within``; all four
  launch shapes, pinned with ``decode_launch_shape`` and a spy on the native entry; K / V rows past a sequence's
  last position are NaN, so a finite result shows that nothing past ``pos`` is consumed;
* the per-row mode of the cache-writing RoPE kernels (csrc/rope.hip; ``qkv_rope_cache_rows_fwd``): bitwise
  ``qkv_rope_fwd`` (then ``e4m3_bytes`` / ``quantise_rows``) per sequence, every other cache byte untouched, and
  nothing written for a position outside the cache.

Tolerance of every rounded output, per element:  ulp(T) * |ref64| + 8 * e32 + 1e-6  (kernel_checks.py).
"""
import pytest
import torch

from kernel_checks import BF16, F16, F32, _dt_id, assert_guard_intact, assert_within, bits_equal, guarded, nan_padded
from test_decode_kernels import ref_attention

from lightning_thunder_amd.ops.kv8 import dequantise_rows, e4m3_bytes, e4m3_values, quantise_rows

gpu = pytest.mark.gpu
U8 = torch.uint8
FORMATS = ["16bit", "kv8", "kv8s"]
ENTRY = {"16bit": "lta_decode_attn_pos", "kv8": "lta_decode_attn_kv8_pos", "kv8s": "lta_decode_attn_kv8s_pos"}

# (B, Hq, Hkv, T, S) -> (wsplit, nsplit) that decode_launch_shape must give
LAUNCH_SHAPES = {
    "wsplit_t1": ((2, 4, 2, 1, 320), (True, 1)),
    "wsplit_t3": ((2, 4, 2, 3, 320), (True, 1)),
    "wsplit_split_t1": ((2, 4, 2, 1, 640), (True, 2)),
    "wsplit_split_t3": ((2, 4, 2, 3, 640), (True, 2)),
    "rows4": ((4, 32, 8, 2, 320), (False, 1)),
    "rows4_split": ((4, 32, 8, 2, 640), (False, 2)),
}


def _position_sets(B, T, S):
    """[B, T] position tensors that together hold: 0, the block edge 63 / 64, 5 (at two splits the second one is
    empty), a value inside the last split, and S - 1; different per sequence and per row."""
    want = [0, 63, 64, 5, S - 7, S - 1, 200, S // 2 + 3]
    n = B * T
    want = want[:max(6, min(n, len(want)))]
    sets = []
    for i in range(0, len(want), n):
        vals = (want[i:i + n] + want * (n // len(want) + 1))[:n]  # topped up from the front, round and round
        sets.append(torch.tensor(vals, dtype=torch.int64).view(B, T))
    assert {int(v) for s in sets for v in s.flatten()} >= {0, 63, 64, 5, S - 7, S - 1}
    return sets


def _kv_case(B, Hq, Hkv, T, S, D, dtype, fmt, seed=0):
    """q [B, Hq, T, D] and a cache in ``fmt``: (q, caches as the kernel takes them, the cache's exact values in
    fp32).  e4m3 values are those of the stored bytes, so quantisation is in no tolerance."""
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, Hq, T, D, generator=g).to(dtype)
    k = torch.randn(B, Hkv, S, D, generator=g).to(dtype)
    v = torch.randn(B, Hkv, S, D, generator=g).to(dtype)
    if fmt == "16bit":
        return q, (k, v), (k.float(), v.float())
    if fmt == "kv8":
        k8, v8 = e4m3_bytes(k), e4m3_bytes(v)
        return q, (k8, v8), (e4m3_values(k8, F32), e4m3_values(v8, F32))
    u = torch.randint(-6, 5, (2, B, Hkv, S, 1), generator=g).float()
    (k8, ks), (v8, vs) = quantise_rows((k.float() * torch.exp2(u[0])).to(dtype)), \
        quantise_rows((v.float() * torch.exp2(u[1])).to(dtype))
    q = (q.float() * 2.0 ** -4).to(dtype)  # scores stay within 60 of the row maximum (no subnormal probability)
    return q, (k8, v8, ks, vs), (dequantise_rows(k8, ks, F32), dequantise_rows(v8, vs, F32))


def _poisoned(caches, exact, pos, fmt):
    """The caches on the GPU inside larger buffers, every key row past its sequence's largest position poisoned:
    NaN in a 16-bit cache (which sits in a NaN-padded buffer), the NaN byte 0x7F in an e4m3 cache; the exact
    values get zeros there (the reference must not see them)."""
    S = caches[0].shape[2]
    last = pos.clamp(-1, S - 1).max(dim=1).values  # [B]
    dead = (torch.arange(S).view(1, 1, S, 1) > last.view(-1, 1, 1, 1))
    out = []
    for c in caches:
        c = c.clone()
        if c.dtype == U8:
            if c.shape[-1] > 1:  # bytes; the scale bytes of dead rows stay valid exponents
                c.masked_fill_(dead, 0x7F)
            buf = torch.full((*c.shape[:2], S + 16, c.shape[3] + (16 if c.shape[3] > 1 else 2)), 0x7F, dtype=U8,
                             device="cuda")
            view = buf[:, :, :S, :c.shape[3]]
            view.copy_(c)
            out.append(view)
        else:
            out.append(nan_padded(c.masked_fill(dead, float("nan")).cuda()))
    return out, [e.masked_fill(dead, 0.0).cuda() for e in exact]


def _launch(fmt, q, caches, pos, scale=None):
    from lightning_thunder_amd.ops import attention as A

    fn = {"16bit": A.decode_attn_pos, "kv8": A.decode_attn_kv8_pos, "kv8s": A.decode_attn_kv8s_pos}[fmt]
    return fn(q, *caches, pos, scale)


class _Calls(list):
    """The spy's record, with the real mask entries kept for tests that compare against them."""


@pytest.fixture
def pos_spy(monkeypatch):
    """Records (entry, wsplit, nsplit) of every native position launch; the mask entries must not run."""
    import lightning_thunder_amd.ops.attention  # noqa: F401
    from lightning_thunder_amd.ops import require

    lib = require()
    calls = _Calls()
    for fmt, name in ENTRY.items():
        real, off = getattr(lib, name), 2 if fmt == "kv8s" else 0

        def spy(*a, _real=real, _name=name, _off=off):
            calls.append((_name, bool(a[17 + _off]), int(a[15 + _off])))
            return _real(*a)

        monkeypatch.setattr(lib, name, spy)
    calls.mask_entries = {}
    for name in ("lta_decode_attn", "lta_decode_attn_kv8", "lta_decode_attn_kv8s"):
        calls.mask_entries[name] = getattr(lib, name)

        def never(*a, _name=name):
            raise AssertionError(f"a position launch must not go through {_name}")

        monkeypatch.setattr(lib, name, never)
    calls.monkeypatch, calls.lib = monkeypatch, lib
    return calls


def _mask_of(pos, S):
    return torch.arange(S, device=pos.device).view(1, 1, 1, S) <= pos[:, None, :, None]


@gpu
@pytest.mark.parametrize("dtype", [BF16, F16], ids=_dt_id)
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("shape", list(LAUNCH_SHAPES))
def test_decode_attn_pos_against_fp64(shape, fmt, D, dtype, pos_spy):
    from lightning_thunder_amd.ops.attention import decode_launch_shape

    (B, Hq, Hkv, T, S), (wsplit, nsplit) = LAUNCH_SHAPES[shape]
    assert decode_launch_shape(B * Hq * T, S)[:2] == (wsplit, nsplit)
    q, caches, exact = _kv_case(B, Hq, Hkv, T, S, D, dtype, fmt, seed=S + D)
    qg = nan_padded(q.cuda())
    for n, pos in enumerate(_position_sets(B, T, S)):
        cg, (k, v) = _poisoned(caches, exact, pos, fmt)
        posg = pos.cuda()
        pos_spy.clear()
        out = _launch(fmt, qg, cg, posg)
        assert list(pos_spy) == [(ENTRY[fmt], wsplit, nsplit)], pos_spy
        assert out.dtype == dtype and out.shape == q.shape and out.is_contiguous()
        mask = _mask_of(posg, S)
        ref64 = ref_attention(qg, k, v, mask, False, D ** -0.5)
        ref32 = ref_attention(qg, k, v, mask, False, D ** -0.5, F32)
        assert torch.isfinite(out).all(), f"{shape} set {n}: a key past a row's position was consumed"
        assert_within(out, ref64, ref32, dtype, f"decode attention pos {fmt}", f"{shape} D{D} set {n}")


@gpu
@pytest.mark.parametrize("dtype", [BF16, F16], ids=_dt_id)
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("shape", ["wsplit_t3", "wsplit_split_t3", "rows4", "rows4_split"])
def test_full_positions_equal_the_mask_kernel_bit_for_bit(shape, D, dtype, pos_spy):
    """pos = S - 1 for every row: the row's chunk is the host's chunk, and the result is ``decode_attn``'s under an
    all-true mask bit for bit."""
    from lightning_thunder_amd.ops.attention import decode_attn

    (B, Hq, Hkv, T, S), (wsplit, nsplit) = LAUNCH_SHAPES[shape]
    q, (k, v), _ = _kv_case(B, Hq, Hkv, T, S, D, dtype, "16bit", seed=1)
    q, k, v = q.cuda(), k.cuda(), v.cuda()
    pos = torch.full((B, T), S - 1, dtype=torch.int64, device="cuda")
    out = _launch("16bit", q, (k, v), pos)
    assert list(pos_spy) == [("lta_decode_attn_pos", wsplit, nsplit)]
    pos_spy.monkeypatch.setattr(pos_spy.lib, "lta_decode_attn", pos_spy.mask_entries["lta_decode_attn"])
    ref = decode_attn(q, k, v, torch.ones(B, 1, T, S, dtype=torch.bool, device="cuda"))
    assert bits_equal(out, ref), f"{(out != ref).sum().item()} elements differ from the mask kernel"


@gpu
@pytest.mark.parametrize("dtype", [BF16, F16], ids=_dt_id)
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("fmt", ["kv8", "kv8s"])
@pytest.mark.parametrize("shape", ["wsplit_t3", "wsplit_split_t3", "rows4", "rows4_split"])
def test_e4m3_position_kernels_equal_the_16_bit_one_bit_for_bit(shape, fmt, D, dtype, pos_spy):
    """Both e4m3 position kernels equal the 16-bit position kernel over the dequantised cache bit for bit.  The
    contract's exclusions: fp32 subnormal or overflowing partial sums (these inputs have none) and results that are
    zero, whose sign may differ (the e4m3 kernels start their sums from -0, so a stored -0 that is all a row sees
    stays -0; at position 0 a result element is the single V element itself).  Zero results must be zero in both
    and stay rare."""
    (B, Hq, Hkv, T, S), _ = LAUNCH_SHAPES[shape]
    q, caches, exact = _kv_case(B, Hq, Hkv, T, S, D, dtype, fmt, seed=2)
    q = q.cuda()
    caches = [c.cuda() for c in caches]
    kd, vd = (e.to(dtype).cuda() for e in exact)
    assert torch.equal(kd.float().cpu(), exact[0]) and torch.equal(vd.float().cpu(), exact[1])
    for n, pos in enumerate(_position_sets(B, T, S)):
        pos = pos.cuda()
        out = _launch(fmt, q, caches, pos)
        plain = _launch("16bit", q, (kd, vd), pos)
        zero = plain == 0
        assert zero.float().mean().item() < 1e-2 and (out[zero] == 0).all()
        out, plain = out.masked_fill(zero, 0), plain.masked_fill(zero, 0)
        assert bits_equal(out, plain), f"set {n}: {(out != plain).sum().item()} elements differ"
    assert {c[0] for c in pos_spy} == {ENTRY[fmt], ENTRY["16bit"]}


# operator (executors/hipex.py ``_decode_attn_<op>_impl``, ops/attention.py ``decode_attn_<op>_supported``) ->
# (cache format, whether it takes positions in place of a mask)
DECLINING = {"kv8": ("kv8", False), "kv8s": ("kv8s", False), "pos": ("16bit", True), "kv8_pos": ("kv8", True),
             "kv8s_pos": ("kv8s", True)}


@gpu
@pytest.mark.parametrize("op", list(DECLINING))
def test_decode_operators_decline_17_query_rows(op, pos_spy):
    """One query row more than the e4m3 and position kernels take: ``*_supported`` refuses, the operator launches
    none of those entries and runs the program as the model spells it, the 16-bit mask kernel (which takes any row
    count) over the dequantised cache under the caller's mask, or under ``position_mask`` for the position forms."""
    from lightning_thunder_amd.executors import hipex
    from lightning_thunder_amd.ops import attention as A
    from lightning_thunder_amd.ops.kv_rows import position_mask

    fmt, by_pos = DECLINING[op]
    B, Hq, Hkv, T, S, D, dtype = 1, 4, 2, A.DECODE_MAX_QUERIES + 1, 96, 64, BF16
    assert T == 17
    q, caches, exact = _kv_case(B, Hq, Hkv, T, S, D, dtype, fmt, seed=4)
    q = q.cuda()
    caches = [c.cuda() for c in caches]
    kd, vd = (e.to(dtype).cuda() for e in exact)
    assert torch.equal(kd.float().cpu(), exact[0]) and torch.equal(vd.float().cpu(), exact[1])
    impl, supported = getattr(hipex, f"_decode_attn_{op}_impl"), getattr(A, f"decode_attn_{op}_supported")
    # the fixture bars the three mask entries; the fallback is the 16-bit one, the format's own stays barred
    pos_spy.monkeypatch.setattr(pos_spy.lib, "lta_decode_attn", pos_spy.mask_entries["lta_decode_attn"])
    for n, pos in enumerate(_position_sets(B, T, S)):
        pos = pos.cuda()
        mask = position_mask(pos, S)
        if by_pos:
            assert not supported(q, *caches, pos)
            out = impl(q, *caches, pos, None)
        else:
            assert not supported(q, *caches)
            out = impl(q, *caches, mask, False, None)
        assert list(pos_spy) == [], f"a position entry ran: {list(pos_spy)}"
        ref = A.decode_attn(q, kd, vd, mask)
        assert out.shape == q.shape and bits_equal(out, ref), f"set {n}: {(out != ref).sum().item()} elements differ"


@gpu
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("shape", ["wsplit_split_t3", "rows4"])
def test_positions_outside_the_cache_are_clamped(shape, fmt, pos_spy):
    """pos >= S attends all S keys and nothing more (the cache is a view inside a poisoned buffer); pos = -1 gives
    the NaN row of a fully masked one."""
    (B, Hq, Hkv, T, S), _ = LAUNCH_SHAPES[shape]
    D, dtype = 64, BF16
    q, caches, exact = _kv_case(B, Hq, Hkv, T, S, D, dtype, fmt, seed=3)
    q = q.cuda()
    pos = torch.full((B, T), S - 1, dtype=torch.int64)
    pos[0, 0], pos[B - 1, T - 1] = S, S + 12345
    pos[0, T - 1] = -1
    pos[B - 1, 0] = -2 ** 40
    cg, _ = _poisoned(caches, exact, torch.full((B, T), S - 1), fmt)  # nothing poisoned inside, the slack is
    out = _launch(fmt, q, cg, pos.cuda())
    ref = _launch(fmt, q, cg, pos.clamp(-1, S - 1).cuda())
    dead = pos < 0
    assert dead.sum().item() == 2
    rows = dead[:, None, :, None].expand(B, Hq, T, D).cuda()
    assert torch.isnan(out[rows]).all(), "a row with no key to attend to is NaN"
    assert torch.isfinite(out[~rows]).all(), "a position past the cache must not read past it"
    assert bits_equal(out[~rows], ref[~rows])
    full = _launch(fmt, q, cg, torch.full((B, T), S - 1, dtype=torch.int64, device="cuda"))
    assert bits_equal(out[0, :, 0], full[0, :, 0]) and bits_equal(out[B - 1, :, T - 1], full[B - 1, :, T - 1])


@gpu
def test_decode_attn_pos_refuses_what_the_kernels_do_not_take():
    from lightning_thunder_amd.ops import attention as A

    q, (k, v), _ = _kv_case(2, 4, 2, 2, 64, 64, BF16, "16bit")
    q, k, v = q.cuda(), k.cuda(), v.cuda()
    pos = torch.tensor([[3, 4], [9, 10]], device="cuda")
    assert A.decode_attn_pos_supported(q, k, v, pos)
    for bad in (pos[0], pos.int(), pos[:, :1], pos.cpu(), None):
        assert not A.decode_attn_pos_supported(q, k, v, bad)
        with pytest.raises(ValueError):
            A.decode_attn_pos(q, k, v, bad)
    assert not A.decode_attn_pos_supported(q[..., :32], k[..., :32], v[..., :32], pos)  # head dim 32
    assert not A.decode_attn_pos_supported(q.float(), k.float(), v.float(), pos)
    q17 = q[:, :, :1].expand(2, 4, 17, 64)
    assert not A.decode_attn_pos_supported(q17, k, v, pos[:, :1].expand(2, 17))  # 17 query rows
    k8 = e4m3_bytes(k)
    assert A.decode_attn_kv8_pos_supported(q, k8, k8, pos) and not A.decode_attn_kv8_pos_supported(q, k8, k8, pos[0])
    assert not A.decode_attn_kv8s_pos_supported(q, k8, k8, None, None, pos)


# ------------------------------------------------------------------------------------------------
# RoPE into the cache at per-row positions
# ------------------------------------------------------------------------------------------------
ROPE_S = 16
ROPE_POS = {1: [[5], [0], [15]], 2: [[5, 6], [0, 9], [14, 15]]}
ROPE_ENTRY = {"16bit": "lta_qkv_rope_cache_fwd_rows", "kv8": "lta_qkv_rope_cache_fwd_kv8_rows",
              "kv8s": "lta_qkv_rope_cache_fwd_kv8s_rows"}


def _rope_caches(fmt, B, ng, S, hs, dtype):
    """(caches as views inside sentinel buffers, the buffers).  16-bit: SENTINEL words; e4m3: 0x5A bytes and zero
    scale bytes (``test_kv8_scaled_kernels._sentinel_caches``)."""
    if fmt == "16bit":
        (kb, kc), (vb, vc) = (guarded((B, ng, S, hs), "cuda", dtype=dtype) for _ in range(2))
        return (kc, vc), (kb, vb)
    kb = torch.full((B, ng, S + 8, hs + 64), 0x5A, device="cuda", dtype=U8)
    vb = torch.full((B, ng + 1, S + 8, hs + 8), 0x5A, device="cuda", dtype=U8)
    views, bufs = (kb[:, :, :S, :hs], vb[:, :ng, :S, :hs]), (kb, vb)
    if fmt == "kv8s":
        ksb = torch.zeros((B, ng, S + 8, 3), device="cuda", dtype=U8)
        vsb = torch.zeros((B, ng + 1, S, 1), device="cuda", dtype=U8)
        views, bufs = (*views, ksb[:, :, :S, :1], vsb[:, :ng]), (*bufs, ksb, vsb)
    return views, bufs


def _rope_rows_inputs(B, T, nh, ng, hs, dtype, cos_dtype, pos):
    """(qkv [B, T, (nh + 2 ng) hs], cos and sin [B, T, hs] gathered per token, pos int64 [B, T]) on the GPU."""
    S = ROPE_S
    g = torch.Generator().manual_seed(hs + T)
    qkv = (torch.randn(B, T, (nh + 2 * ng) * hs, generator=g) * 4).to(dtype).cuda()
    cos_tab = (torch.rand(S, hs, generator=g) * 2 - 1).to(cos_dtype).cuda()
    sin_tab = (torch.rand(S, hs, generator=g) * 2 - 1).to(cos_dtype).cuda()
    pos = torch.tensor(pos, dtype=torch.int64, device="cuda")
    rot = pos.clamp(0, S - 1)  # a token outside the cache still gets a rotation for its q row
    return qkv, cos_tab[rot], sin_tab[rot], pos


def _assert_rope_rows(fmt, qkv, cos, sin, pos, nh, ng, hs, q, bufs):
    """``q`` and the cache buffers ``bufs`` against the shared-position kernel per sequence, its rows stored as the
    format stores them at the positions inside the cache, the sentinel everywhere else.  Returns the rows written."""
    from lightning_thunder_amd.ops.fused import qkv_rope_fwd

    (B, T), S, dtype = pos.shape, ROPE_S, qkv.dtype
    exp_caches, exp_bufs = _rope_caches(fmt, B, ng, S, hs, dtype)
    written = 0
    for b in range(B):
        q0, k0, v0 = qkv_rope_fwd(qkv[b:b + 1], cos[b], sin[b], nh, ng, hs, hs)
        assert bits_equal(q[b:b + 1], q0), f"q of sequence {b}"
        rows = {"16bit": lambda: (k0, v0), "kv8": lambda: (e4m3_bytes(k0), e4m3_bytes(v0)),
                "kv8s": lambda: tuple(t for pair in zip(quantise_rows(k0), quantise_rows(v0)) for t in pair)}[fmt]()
        for t in range(T):
            p = int(pos[b, t])
            if 0 <= p < S:
                written += 1
                for e, r in zip(exp_caches, rows):
                    e[b, :, p] = r[0, :, t]
    assert written == int(((pos >= 0) & (pos < S)).sum())
    for name, got_b, exp_b in zip(("k", "v", "k_scale", "v_scale"), bufs, exp_bufs):
        assert torch.equal(got_b, exp_b), f"the {name} cache differs from the per-sequence rows (or a store strayed)"
    return written


def _check_rope_rows(fmt, B, T, nh, ng, hs, dtype, cos_dtype, pos, monkeypatch):
    from lightning_thunder_amd.ops import require
    from lightning_thunder_amd.ops.fused import qkv_rope_cache_rows_fwd, qkv_rope_cache_rows_supported

    S = ROPE_S
    qkv, cos, sin, pos = _rope_rows_inputs(B, T, nh, ng, hs, dtype, cos_dtype, pos)
    caches, bufs = _rope_caches(fmt, B, ng, S, hs, dtype)
    scales = dict(k_scale=caches[2], v_scale=caches[3]) if fmt == "kv8s" else {}
    assert qkv_rope_cache_rows_supported(qkv, cos, sin, caches[0], caches[1], pos, ng, hs, hs, **scales)
    lib = require()
    calls = []
    for name in ROPE_ENTRY.values():
        monkeypatch.setattr(lib, name, lambda *a, _r=getattr(lib, name), _n=name: calls.append(_n) or _r(*a))
    for name in ("lta_qkv_rope_cache_fwd", "lta_qkv_rope_cache_fwd_kv8", "lta_qkv_rope_cache_fwd_kv8s"):
        monkeypatch.setattr(lib, name, lambda *a, _n=name: pytest.fail(f"per-row positions reached {_n}"))
    q, *got = qkv_rope_cache_rows_fwd(qkv, cos, sin, nh, ng, hs, hs, caches[0], caches[1], pos, **scales)
    assert calls == [ROPE_ENTRY[fmt]]
    for g_, src in zip(got, caches):
        assert g_.data_ptr() == src.data_ptr() and g_.stride() == src.stride()
    written = _assert_rope_rows(fmt, qkv, cos, sin, pos, nh, ng, hs, q, bufs)
    if fmt == "16bit":
        for buf in bufs:
            assert_guard_intact(buf, (B, ng, S, hs), "rope rows")
    return written


@gpu
@pytest.mark.parametrize("dtype", [BF16, F16], ids=_dt_id)
@pytest.mark.parametrize("same_cos", [False, True], ids=["cos_fp32", "cos_same"])
@pytest.mark.parametrize("T", [1, 2])
@pytest.mark.parametrize("hs", [64, 128])
@pytest.mark.parametrize("fmt", FORMATS)
def test_qkv_rope_cache_rows(fmt, hs, T, same_cos, dtype, monkeypatch):
    n = _check_rope_rows(fmt, 3, T, 4, 2, hs, dtype, dtype if same_cos else F32, ROPE_POS[T], monkeypatch)
    assert n == 3 * T


@gpu
@pytest.mark.parametrize("fmt", ["kv8", "kv8s"])
def test_qkv_rope_cache_rows_operators_decline_hs96(fmt, monkeypatch):
    """hs = 96 is no row-kernel shape, so ``qkv_rope_cache_rows_supported`` refuses uint8 caches and the per-row
    operators write what the model's program writes (RoPE, quantise, one row write per buffer) without an e4m3
    rows launch.  One uint8 cache beside a 16-bit one is refused."""
    from lightning_thunder_amd.executors.hipex import _qkv_rope_cache_rows_impl, _qkv_rope_cache_rows_s8_impl
    from lightning_thunder_amd.ops import require
    from lightning_thunder_amd.ops.fused import qkv_rope_cache_rows_supported

    B, T, nh, ng, hs, dtype = 3, 2, 4, 2, 96, BF16
    qkv, cos, sin, pos = _rope_rows_inputs(B, T, nh, ng, hs, dtype, F32, ROPE_POS[T])
    caches, bufs = _rope_caches(fmt, B, ng, ROPE_S, hs, dtype)
    scales = dict(k_scale=caches[2], v_scale=caches[3]) if fmt == "kv8s" else {}
    assert not qkv_rope_cache_rows_supported(qkv, cos, sin, caches[0], caches[1], pos, ng, hs, hs, **scales)
    lib = require()
    for name in (ROPE_ENTRY["kv8"], ROPE_ENTRY["kv8s"]):
        monkeypatch.setattr(lib, name, lambda *a, _n=name: pytest.fail(f"an unsupported shape reached {_n}"))
    impl = _qkv_rope_cache_rows_s8_impl if fmt == "kv8s" else _qkv_rope_cache_rows_impl
    q, *got = impl(qkv, cos, sin, nh, ng, hs, hs, *caches, pos)
    assert [t.data_ptr() for t in got] == [t.data_ptr() for t in caches]
    assert _assert_rope_rows(fmt, qkv, cos, sin, pos, nh, ng, hs, q, bufs) == B * T
    if fmt == "kv8":
        with pytest.raises(ValueError):
            _qkv_rope_cache_rows_impl(qkv, cos, sin, nh, ng, hs, hs, caches[0], torch.zeros_like(caches[1], dtype=dtype),
                                      pos)


@gpu
@pytest.mark.parametrize("dtype", [BF16, F16], ids=_dt_id)
@pytest.mark.parametrize("T", [1, 2])
def test_qkv_rope_cache_rows_generic_kernel_hs96(T, dtype, monkeypatch):
    """hs = 96 (six chunk pairs, no power of two) takes the generic kernel; 16-bit caches only."""
    assert _check_rope_rows("16bit", 3, T, 4, 2, 96, dtype, F32, ROPE_POS[T], monkeypatch) == 3 * T


@gpu
@pytest.mark.parametrize("T", [1, 2])
def test_qkv_rope_cache_rows_generic_kernel_fp32(T):
    """fp32 activations and caches: the generic kernel's 4-element chunks."""
    from lightning_thunder_amd.ops.fused import qkv_rope_cache_rows_fwd, qkv_rope_fwd

    B, nh, ng, hs, S = 3, 4, 2, 96, ROPE_S
    g = torch.Generator().manual_seed(T)
    qkv = torch.randn(B, T, (nh + 2 * ng) * hs, generator=g).cuda()
    cos_tab, sin_tab = (torch.rand(S, hs, generator=g).cuda() * 2 - 1 for _ in range(2))
    pos = torch.tensor(ROPE_POS[T], device="cuda")
    kc, vc = (torch.full((B, ng, S, hs), 7.5, device="cuda") for _ in range(2))
    q, k_all, v_all = qkv_rope_cache_rows_fwd(qkv, cos_tab[pos], sin_tab[pos], nh, ng, hs, hs, kc, vc, pos)
    ek, ev = torch.full_like(kc, 7.5), torch.full_like(vc, 7.5)
    for b in range(B):
        q0, k0, v0 = qkv_rope_fwd(qkv[b:b + 1], cos_tab[pos[b]], sin_tab[pos[b]], nh, ng, hs, hs)
        assert torch.equal(q[b:b + 1], q0)
        ek[b, :, pos[b]], ev[b, :, pos[b]] = k0[0], v0[0]
    assert torch.equal(kc, ek) and torch.equal(vc, ev)


@gpu
@pytest.mark.parametrize("fmt,hs", [(f, 64) for f in FORMATS] + [("16bit", 96)])  # e4m3: the row kernel's sizes only
def test_qkv_rope_cache_rows_outside_the_cache_write_nothing(fmt, hs, monkeypatch):
    pos = [[-1, 3], [ROPE_S, ROPE_S + 1000], [7, -2 ** 40]]
    assert _check_rope_rows(fmt, 3, 2, 4, 2, hs, BF16, F32, pos, monkeypatch) == 2


@gpu
def test_qkv_rope_cache_rows_refuses_what_the_kernels_do_not_take():
    from lightning_thunder_amd.ops.fused import qkv_rope_cache_rows_fwd, qkv_rope_cache_rows_supported

    B, T, nh, ng, hs, S = 2, 2, 4, 2, 64, ROPE_S
    qkv = torch.randn(B, T, (nh + 2 * ng) * hs, device="cuda", dtype=BF16)
    cos = torch.rand(B, T, hs, device="cuda")
    kc, vc = (torch.zeros(B, ng, S, hs, device="cuda", dtype=BF16) for _ in range(2))
    pos = torch.tensor([[1, 2], [5, 6]], device="cuda")
    assert qkv_rope_cache_rows_supported(qkv, cos, cos, kc, vc, pos, ng, hs, hs)
    for bad_pos in (pos[0], pos.int(), pos[:, :1]):
        assert not qkv_rope_cache_rows_supported(qkv, cos, cos, kc, vc, bad_pos, ng, hs, hs)
        with pytest.raises(ValueError):
            qkv_rope_cache_rows_fwd(qkv, cos, cos, nh, ng, hs, hs, kc, vc, bad_pos)
    assert not qkv_rope_cache_rows_supported(qkv, cos[0], cos[0], kc, vc, pos, ng, hs, hs)  # shared [T, hs] tables
    k8 = torch.zeros(B, ng, S, 96, device="cuda", dtype=U8)
    qkv96 = torch.randn(B, T, (nh + 2 * ng) * 96, device="cuda", dtype=BF16)
    cos96 = torch.rand(B, T, 96, device="cuda")
    assert not qkv_rope_cache_rows_supported(qkv96, cos96, cos96, k8, k8, pos, ng, 96, 96)  # e4m3 at hs 96
