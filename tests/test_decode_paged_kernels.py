"""The kernels of a paged KV cache (ops/kv_pages.py):

* the paged mode of the decode-attention kernels (csrc/decode_attention.hip; ``decode_attn_paged``,
  ``decode_attn_kv8_paged``, ``decode_attn_kv8s_paged``): the position mode with key j of sequence b read at pool row
  ``table[b, j // page] * page + j % page``.  Every case against fp64 with ``assert_within`` and, bit for bit, against
  the position kernel over ``gather_pages`` of the same pools (the two differ in addresses only); all four launch
  shapes, pinned with ``decode_launch_shape`` and a spy on the native entries.  Every pool row no live key refers to
  is poisoned (NaN, or the NaN byte 0x7F) and the pools sit in guarded buffers, so a finite result shows that nothing
  else was read, and the unchanged buffers that nothing was written;
* the slot write of the cache-writing RoPE (csrc/rope.hip per-row entries; ``qkv_rope_cache_slots_fwd``): bitwise the
  per-row write per sequence, every other pool byte and the sink row untouched.

Tolerance of every rounded output, per element:  ulp(T) * |ref64| + 8 * e32 + 1e-6  (kernel_checks.py).
"""
import pytest
import torch

from kernel_checks import BF16, F16, F32, SENTINEL, _dt_id, assert_guard_intact, assert_within, bits_equal, guarded
from test_decode_kernels import ref_attention
from test_decode_pos_kernels import _kv_case, _rope_rows_inputs

from lightning_thunder_amd.ops.kv8 import e4m3_values
from lightning_thunder_amd.ops.kv_pages import gather_pages, page_slots, paged_mask

gpu = pytest.mark.gpu
U8, I64 = torch.uint8, torch.int64
FORMATS = ["16bit", "kv8", "kv8s"]
ENTRY = {"16bit": "lta_decode_attn_paged", "kv8": "lta_decode_attn_kv8_paged", "kv8s": "lta_decode_attn_kv8s_paged"}
POS_ENTRY = {f: e.replace("_paged", "_pos") for f, e in ENTRY.items()}
MASK_ENTRY = {f: e.replace("_paged", "") for f, e in ENTRY.items()}

# (B, Hq, Hkv, T, S) -> (wsplit, nsplit) that decode_launch_shape must give; S is a multiple of every page size
LAUNCH_SHAPES = {
    "wsplit_t1": ((2, 4, 2, 1, 384), (True, 1)),
    "wsplit_t3": ((2, 4, 2, 3, 384), (True, 1)),
    "wsplit_split_t1": ((2, 4, 2, 1, 640), (True, 2)),
    "wsplit_split_t3": ((2, 4, 2, 3, 640), (True, 2)),
    "rows4": ((4, 32, 8, 2, 384), (False, 1)),
    "rows4_split": ((4, 32, 8, 2, 640), (False, 2)),
}
PAGE_SIZES = [16, 64, 128]
SPARE_PAGES = 3  # pages no table refers to


def _position_sets(B, T, S, page):
    """[B, T] position tensors that together hold 0, page - 1, page, 63, 64, a value inside the last split and
    S - 1; different per sequence and per row."""
    want = [0, page - 1, page, 63, 64, S - 7, S - 1, 5, 200, S // 2 + 3]
    n = B * T
    sets = []
    for i in range(0, 8, n):
        vals = (want[i:i + n] + want * (n // len(want) + 1))[:n]  # topped up from the front, round and round
        sets.append(torch.tensor(vals, dtype=I64).view(B, T))
    assert {int(v) for s in sets for v in s.flatten()} >= {0, page - 1, page, 63, 64, S - 7, S - 1}
    return sets


def _table(B, S, page, seed=0):
    """A shuffled block table [B, S / page] over ``B * S / page + SPARE_PAGES`` pages, and that page count."""
    P = S // page
    num_pages = B * P + SPARE_PAGES
    g = torch.Generator().manual_seed(seed + page)
    table = torch.randperm(num_pages, generator=g)[:B * P].view(B, P).to(I64)
    assert not torch.equal(table.flatten(), torch.arange(B * P)), "the table is no identity"
    return table, num_pages


def _pools(caches, exact, pos, table, page, num_pages, fmt):
    """The logical ``caches`` [B, Hkv, S, d] laid out in pools [Hkv, R + 1, d] on the GPU through ``table``; a key row
    is live when ``paged_mask`` shows it to some query row of its sequence.  Every other pool row (dead keys, spare
    pages, pages of dropped table entries, the sink) is poisoned: NaN in a 16-bit pool, the NaN byte 0x7F in an e4m3
    pool (scale bytes stay valid exponents).  Returns (pools as views of guarded buffers, the buffers, the exact
    values with zeros at the dead keys)."""
    B, Hkv, S, _ = caches[0].shape
    R = num_pages * page
    live = paged_mask(pos, table, page, num_pages).any(dim=2)[:, 0]  # [B, S]
    views, bufs = [], []
    for c in caches:
        d = c.shape[3]
        bytes_ = c.dtype == U8
        pool = torch.full((Hkv, R + 1, d), 0x7F if bytes_ else float("nan"), dtype=c.dtype)
        if bytes_ and d == 1:
            pool.fill_(127)
        for b in range(B):
            for i in range(S // page):
                p = int(table[b, i])
                if not 0 <= p < num_pages:
                    continue
                rows = c[b, :, i * page:(i + 1) * page].clone()
                if not (bytes_ and d == 1):
                    rows[:, ~live[b, i * page:(i + 1) * page]] = 0x7F if bytes_ else float("nan")
                pool[:, p * page:(p + 1) * page] = rows
        if bytes_:
            buf = torch.full((Hkv, R + 1 + 8, d + 16 if d > 1 else 3), 0x7F, dtype=U8, device="cuda")
            view = buf[:, :R + 1, :d]
        else:
            buf, view = guarded((Hkv, R + 1, d), "cuda", dtype=c.dtype)
        view.copy_(pool)
        views.append(view)
        bufs.append(buf)
    dead = ~live[:, None, :, None]
    return views, bufs, [e.masked_fill(dead, 0.0).cuda() for e in exact]


def _launch(fmt, q, pools, pos, table, page, num_pages, scale=None):
    from lightning_thunder_amd.ops import attention as A

    fn = {"16bit": A.decode_attn_paged, "kv8": A.decode_attn_kv8_paged, "kv8s": A.decode_attn_kv8s_paged}[fmt]
    return fn(q, *pools, pos, table, page, num_pages, scale)


def _launch_pos(fmt, q, caches, pos, scale=None):
    from lightning_thunder_amd.ops import attention as A

    fn = {"16bit": A.decode_attn_pos, "kv8": A.decode_attn_kv8_pos, "kv8s": A.decode_attn_kv8s_pos}[fmt]
    return fn(q, *caches, pos, scale)


@pytest.fixture
def spy(monkeypatch):
    """Records (entry, wsplit, nsplit) of every native paged, position and mask launch of the decode kernels."""
    import lightning_thunder_amd.ops.attention  # noqa: F401
    from lightning_thunder_amd.ops import require

    lib = require()
    calls = []
    for fmt in FORMATS:
        off = 2 if fmt == "kv8s" else 0
        # argument positions of (nsplit, wsplit): the mask entries carry chunk before and causal after nsplit
        for name, ns, ws in ((ENTRY[fmt], 15, 17), (POS_ENTRY[fmt], 15, 17), (MASK_ENTRY[fmt], 16, 19)):
            def record(*a, _real=getattr(lib, name), _name=name, _ns=ns + off, _ws=ws + off):
                calls.append((_name, bool(a[_ws]), int(a[_ns])))
                return _real(*a)

            monkeypatch.setattr(lib, name, record)
    return calls


def _run_and_check(fmt, q, caches, exact, pos, table, page, num_pages, dtype, D, what, spy, shape=None):
    """One paged launch over poisoned, guarded pools: the launch shape, finite, within tolerance of fp64 under
    ``paged_mask``, nothing written.  Returns (out, the pools, pos / table on the GPU)."""
    pools, bufs, (k, v) = _pools(caches, exact, pos, table, page, num_pages, fmt)
    before = [b.clone() for b in bufs]
    posg, tabg = pos.cuda(), table.cuda()
    del spy[:]
    out = _launch(fmt, q, pools, posg, tabg, page, num_pages)
    if shape is not None:
        assert spy == [(ENTRY[fmt], *shape)], spy
    assert out.dtype == dtype and out.shape == q.shape and out.is_contiguous()
    mask = paged_mask(posg, tabg, page, num_pages)
    ref64 = ref_attention(q, k, v, mask, False, D ** -0.5)
    ref32 = ref_attention(q, k, v, mask, False, D ** -0.5, F32)
    assert torch.isfinite(out).all(), f"{what}: a pool row no live key refers to was consumed"
    assert_within(out, ref64, ref32, dtype, f"decode attention paged {fmt}", what)
    for buf, old, pool in zip(bufs, before, pools):
        assert torch.equal(buf, old), f"{what}: a pool buffer was written"
        if buf.dtype == torch.int16:
            assert_guard_intact(buf, pool.shape, what)
    return out, pools, posg, tabg


def _check_case(shape, fmt, page, D, dtype, spy):
    from lightning_thunder_amd.ops.attention import decode_launch_shape

    (B, Hq, Hkv, T, S), (wsplit, nsplit) = LAUNCH_SHAPES[shape]
    assert decode_launch_shape(B * Hq * T, S)[:2] == (wsplit, nsplit)
    q, caches, exact = _kv_case(B, Hq, Hkv, T, S, D, dtype, fmt, seed=S + D + page)
    q = q.cuda()
    table, num_pages = _table(B, S, page)
    for n, pos in enumerate(_position_sets(B, T, S, page)):
        what = f"{shape} D{D} page{page} set {n}"
        out, pools, posg, tabg = _run_and_check(fmt, q, caches, exact, pos, table, page, num_pages, dtype, D, what, spy,
                                                (wsplit, nsplit))
        # the same pools, gathered: the position kernel computes the same sums in the same order
        gathered = [gather_pages(p, tabg, page) for p in pools]
        assert all(g.shape[:3] == (B, Hkv, S) for g in gathered)
        ref = _launch_pos(fmt, q, gathered, posg)
        assert spy[-1] == (POS_ENTRY[fmt], wsplit, nsplit)
        assert bits_equal(out, ref), f"{what}: {(out != ref).sum().item()} elements differ from the position kernel"


@gpu
@pytest.mark.parametrize("D,dtype", [(64, BF16), (128, F16)], ids=["D64_bf16", "D128_fp16"])
@pytest.mark.parametrize("page", PAGE_SIZES)
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("shape", list(LAUNCH_SHAPES))
def test_decode_attn_paged_against_fp64_and_the_position_kernel(shape, fmt, page, D, dtype, spy):
    _check_case(shape, fmt, page, D, dtype, spy)


@gpu
@pytest.mark.parametrize("D,dtype", [(64, F16), (128, BF16)], ids=["D64_fp16", "D128_bf16"])
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("shape,page", [("wsplit_split_t3", 16), ("rows4", 64), ("rows4_split", 128)])
def test_decode_attn_paged_other_type_pairs(shape, page, fmt, D, dtype, spy):
    _check_case(shape, fmt, page, D, dtype, spy)


@gpu
@pytest.mark.parametrize("page", PAGE_SIZES)
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("shape", list(LAUNCH_SHAPES))
def test_table_holes_and_bad_entries_are_masked_keys(shape, fmt, page, spy):
    """A ``-1`` below a row's position and an entry ``>= num_pages`` (and one far outside): their keys are invalid
    like masked ones and nothing of them is read (those pages' rows are poisoned wherever they might point).  Against
    fp64 under ``paged_mask``; at one split bit for bit against the mask kernel over ``gather_pages`` under that mask
    (the unscaled e4m3 mask kernel rounds acc / l its own way, see csrc ``normalised``, so that format is held to
    the 16-bit mask kernel over the exact values, zero results aside as in ``test_decode_pos_kernels.py``)."""
    from lightning_thunder_amd.ops import attention as A

    (B, Hq, Hkv, T, S), (wsplit, nsplit) = LAUNCH_SHAPES[shape]
    D, dtype = 64, BF16
    q, caches, exact = _kv_case(B, Hq, Hkv, T, S, D, dtype, fmt, seed=7 + page)
    q = q.cuda()
    table, num_pages = _table(B, S, page, seed=1)
    P = S // page
    assert P >= 3
    table[0, 0] = -1  # a hole at the very start, below every position of the sequence
    table[0, P - 1] = -7
    table[B - 1, 1] = num_pages  # the first page past the pool
    table[B - 1, P - 1] = 2 ** 40
    pos = torch.full((B, T), S - 1, dtype=I64)
    pos[0, 0] = S - page - 3  # every sequence keeps a live page: 1 of sequence 0, 0 of the last one
    out, pools, posg, tabg = _run_and_check(fmt, q, caches, exact, pos, table, page, num_pages, dtype, D,
                                            f"{shape} page{page} holes", spy, (wsplit, nsplit))
    if nsplit != 1:
        return
    mask = paged_mask(posg, tabg, page, num_pages)
    gathered = [gather_pages(p, tabg, page) for p in pools]
    if fmt == "16bit":
        ref = A.decode_attn(q, *gathered, mask)
    elif fmt == "kv8s":
        ref = A.decode_attn_kv8s(q, *gathered, mask)
    else:
        ref = A.decode_attn(q, *(e4m3_values(g, dtype) for g in gathered), mask)
        zero = ref == 0
        assert zero.float().mean().item() < 1e-2 and (out[zero] == 0).all()
        out, ref = out.masked_fill(zero, 0), ref.masked_fill(zero, 0)
    assert bits_equal(out, ref), f"{(out != ref).sum().item()} elements differ from the mask kernel"


@gpu
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("shape", ["wsplit_split_t3", "rows4"])
def test_positions_outside_the_cache_are_clamped(shape, fmt, spy):
    """pos >= S attends all S keys and nothing more; pos = -1 gives the NaN row of a fully masked one; so does a
    sequence whose table row is all ``-1``."""
    (B, Hq, Hkv, T, S), _ = LAUNCH_SHAPES[shape]
    D, dtype, page = 64, BF16, 64
    q, caches, exact = _kv_case(B, Hq, Hkv, T, S, D, dtype, fmt, seed=3)
    q = q.cuda()
    table, num_pages = _table(B, S, page, seed=2)
    pos = torch.full((B, T), S - 1, dtype=I64)
    pos[0, 0], pos[B - 1, T - 1] = S, S + 12345
    pos[0, T - 1] = -1
    pos[B - 1, 0] = -2 ** 40
    pools, _, _ = _pools(caches, exact, pos.clamp(-1, S - 1), table, page, num_pages, fmt)
    tabg = table.cuda()
    out = _launch(fmt, q, pools, pos.cuda(), tabg, page, num_pages)
    ref = _launch(fmt, q, pools, pos.clamp(-1, S - 1).cuda(), tabg, page, num_pages)
    dead = pos < 0
    assert dead.sum().item() == 2
    rows = dead[:, None, :, None].expand(B, Hq, T, D).cuda()
    assert torch.isnan(out[rows]).all(), "a row with no key to attend to is NaN"
    assert torch.isfinite(out[~rows]).all(), "a position past the capacity must not read past the table"
    assert bits_equal(out[~rows], ref[~rows])
    tabg[1] = -1  # a released sequence
    out = _launch(fmt, q, pools, pos.clamp(0, S - 1).cuda(), tabg, page, num_pages)
    assert torch.isnan(out[1]).all() and torch.isfinite(out[0]).all()


@gpu
def test_paged_wrappers_refuse_what_the_kernels_do_not_take(spy):
    """17 query rows, head size 96 and page size 24 (and a few more) are declined by ``*_supported`` and raised by
    the wrappers; the operator runs 17 rows as the model spells them (gather, mask, the mask kernel)."""
    from lightning_thunder_amd.executors import hipex
    from lightning_thunder_amd.ops import attention as A

    B, Hq, Hkv, T, S, D, page = 2, 4, 2, 2, 96, 64, 16
    table, num_pages = _table(B, S, page)
    R = num_pages * page
    g = torch.Generator().manual_seed(5)
    q = torch.randn(B, Hq, T, D, generator=g).to(BF16).cuda()
    kp, vp = (torch.randn(Hkv, R + 1, D, generator=g).to(BF16).cuda() for _ in range(2))
    pos = torch.tensor([[3, 4], [40, 95]]).cuda()
    tab = table.cuda()
    k8, v8 = kp.view(torch.int16).to(U8), vp.view(torch.int16).to(U8)
    ks = torch.full((Hkv, R + 1, 1), 127, dtype=U8, device="cuda")
    assert A.decode_attn_paged_supported(q, kp, vp, pos, tab, page, num_pages)
    assert A.decode_attn_kv8_paged_supported(q, k8, v8, pos, tab, page, num_pages)
    assert A.decode_attn_kv8s_paged_supported(q, k8, v8, ks, ks, pos, tab, page, num_pages)
    q17 = q[:, :, :1].expand(B, Hq, 17, D).contiguous()
    pos17 = pos[:, :1].expand(B, 17).contiguous()
    q96, kp96 = torch.zeros(B, Hq, T, 96, dtype=BF16, device="cuda"), torch.zeros(Hkv, R + 1, 96, dtype=BF16, device="cuda")
    bad = [dict(q=q17, pos=pos17), dict(q=q96, k=kp96, v=kp96), dict(page=24), dict(page=8), dict(num_pages=num_pages + 1),
           dict(pos=pos.int()), dict(table=tab.int()), dict(table=tab[:1]), dict(pos=pos[0]), dict(table=tab.cpu()),
           dict(k=kp[:, 1:]), dict(q=q.float())]
    for change in bad:
        a = dict(q=q, k=kp, v=vp, pos=pos, table=tab, page=page, num_pages=num_pages)
        a.update(change)
        args = (a["q"], a["k"], a["v"], a["pos"], a["table"], a["page"], a["num_pages"])
        assert not A.decode_attn_paged_supported(*args), change
        with pytest.raises(ValueError):
            A.decode_attn_paged(*args)
        if set(change) & {"k", "v"}:
            continue
        a8 = (a["q"], k8, v8, a["pos"], a["table"], a["page"], a["num_pages"])
        a8s = (a["q"], k8, v8, ks, ks, a["pos"], a["table"], a["page"], a["num_pages"])
        assert not A.decode_attn_kv8_paged_supported(*a8) and not A.decode_attn_kv8s_paged_supported(*a8s), change
        with pytest.raises(ValueError):
            A.decode_attn_kv8_paged(*a8)
        with pytest.raises(ValueError):
            A.decode_attn_kv8s_paged(*a8s)
    assert not A.decode_attn_kv8s_paged_supported(q, k8, v8, ks[:, :-1], ks, pos, tab, page, num_pages)
    odd = torch.zeros(k8.numel() + 8, dtype=U8, device="cuda")[8:].view(k8.shape)  # 8 bytes off a 16-byte boundary
    assert odd.data_ptr() % 16 == 8 and not A.decode_attn_kv8_paged_supported(q, odd, odd, pos, tab, page, num_pages)
    assert spy == [], "a refused call launched something"
    out = hipex._decode_attn_paged_impl(q17, kp, vp, pos17, tab, page, num_pages, None)
    assert [c[0] for c in spy] == ["lta_decode_attn"]
    ref = A.decode_attn(q17, gather_pages(kp, tab, page), gather_pages(vp, tab, page),
                        paged_mask(pos17, tab, page, num_pages))
    assert bits_equal(out, ref)


# ------------------------------------------------------------------------------------------------
# RoPE into the pools at every token's slot
# ------------------------------------------------------------------------------------------------
ROPE_S, ROPE_PAGE = 32, 16  # two pages per sequence
ROPE_POS = {1: [[5], [16], [31]], 2: [[5, 6], [15, 16], [30, 31]]}


def _sentinel_pools(fmt, ng, rows, hs, dtype):
    """(pools as views inside sentinel buffers, the buffers): SENTINEL words around a 16-bit pool, 0x5A bytes around
    an e4m3 one, zero bytes around the scale pools."""
    if fmt == "16bit":
        (kb, kp), (vb, vp) = (guarded((ng, rows, hs), "cuda", dtype=dtype) for _ in range(2))
        return (kp, vp), (kb, vb)
    kb = torch.full((ng, rows + 8, hs + 64), 0x5A, device="cuda", dtype=U8)
    vb = torch.full((ng + 1, rows + 8, hs + 8), 0x5A, device="cuda", dtype=U8)
    views, bufs = (kb[:, :rows, :hs], vb[:ng, :rows, :hs]), (kb, vb)
    if fmt == "kv8s":
        ksb = torch.zeros((ng, rows + 8, 3), device="cuda", dtype=U8)
        vsb = torch.zeros((ng + 1, rows, 1), device="cuda", dtype=U8)
        views, bufs = (*views, ksb[:, :rows, :1], vsb[:ng]), (*bufs, ksb, vsb)
    return views, bufs


def _check_slot_write(fmt, T, hs, dtype, pos, table, num_pages, monkeypatch):
    """The slot write against the per-row write into a static cache [B, ng, S, hs]: pool row ``slots[b, t]`` holds
    that cache's row ``pos[b, t]`` bit for bit, everything else (other rows, the sink, the guards) is untouched.
    Returns the rows written."""
    from lightning_thunder_amd.ops import require
    from lightning_thunder_amd.ops.fused import (qkv_rope_cache_rows_fwd, qkv_rope_cache_slots_fwd,
                                                 qkv_rope_cache_slots_supported)

    B, nh, ng, S, page = len(pos), 4, 2, ROPE_S, ROPE_PAGE
    R = num_pages * page
    qkv, cos, sin, posg = _rope_rows_inputs(B, T, nh, ng, hs, dtype, F32, pos)
    # _rope_rows_inputs draws its rotation tables for 16 positions; a position's rotation does not matter here
    slots = page_slots(table.cuda(), posg, page, R)
    cdt = dtype if fmt == "16bit" else U8
    static = [torch.zeros(B, ng, S, hs, device="cuda", dtype=cdt) for _ in range(2)]
    if fmt == "kv8s":
        static += [torch.zeros(B, ng, S, 1, device="cuda", dtype=U8) for _ in range(2)]
    scales = lambda c: dict(k_scale=c[2], v_scale=c[3]) if fmt == "kv8s" else {}
    q0, *_ = qkv_rope_cache_rows_fwd(qkv, cos, sin, nh, ng, hs, hs, static[0], static[1], posg, **scales(static))
    pools, bufs = _sentinel_pools(fmt, ng, R + 1, hs, dtype)
    exp_pools, exp_bufs = _sentinel_pools(fmt, ng, R + 1, hs, dtype)
    assert qkv_rope_cache_slots_supported(qkv, cos, sin, pools[0], pools[1], slots, ng, hs, hs, **scales(pools))
    lib = require()
    calls = []
    for name in ("lta_qkv_rope_cache_fwd_rows", "lta_qkv_rope_cache_fwd_kv8_rows", "lta_qkv_rope_cache_fwd_kv8s_rows"):
        monkeypatch.setattr(lib, name, lambda *a, _r=getattr(lib, name), _n=name: calls.append(_n) or _r(*a))
    q, *got = qkv_rope_cache_slots_fwd(qkv, cos, sin, nh, ng, hs, hs, pools[0], pools[1], slots, **scales(pools))
    assert calls == [{"16bit": "lta_qkv_rope_cache_fwd_rows", "kv8": "lta_qkv_rope_cache_fwd_kv8_rows",
                      "kv8s": "lta_qkv_rope_cache_fwd_kv8s_rows"}[fmt]]
    assert bits_equal(q, q0)
    for g_, src in zip(got, pools):
        assert g_.data_ptr() == src.data_ptr() and g_.stride() == src.stride()
    written = 0
    for b in range(B):
        for t in range(T):
            s = int(slots[b, t])
            if s == R:
                continue
            written += 1
            for e, c in zip(exp_pools, static):
                e[:, s] = c[b, :, int(posg[b, t])]
    for name, got_b, exp_b in zip(("k", "v", "k_scale", "v_scale"), bufs, exp_bufs):
        assert torch.equal(got_b, exp_b), f"the {name} pool differs from the per-row write (or a store strayed)"
    if fmt == "16bit":
        for buf in bufs:
            assert_guard_intact(buf, (ng, R + 1, hs), "rope slots")
            assert (buf[:, R, :hs] == SENTINEL).all(), "the sink row is untouched by the kernel"
    return written


@gpu
@pytest.mark.parametrize("dtype", [BF16, F16], ids=_dt_id)
@pytest.mark.parametrize("T", [1, 2])
@pytest.mark.parametrize("hs", [64, 128])
@pytest.mark.parametrize("fmt", FORMATS)
def test_qkv_rope_cache_slots(fmt, hs, T, dtype, monkeypatch):
    table = torch.tensor([[4, 1], [0, 6], [5, 2]])  # shuffled, page 3 spare
    assert _check_slot_write(fmt, T, hs, dtype, ROPE_POS[T], table, 7, monkeypatch) == 3 * T


@gpu
@pytest.mark.parametrize("fmt", FORMATS)
def test_qkv_rope_cache_slots_without_a_page_write_nothing(fmt, monkeypatch):
    """Positions outside [0, S), a position on a page the sequence does not have, a table entry past the pool: their
    slot is the sink row R, and the kernel writes nothing for it."""
    pos = [[-1, 3], [ROPE_S, 20], [7, 17]]
    table = torch.tensor([[4, 1], [0, -1], [5, 7]])  # sequence 1 has one page; 7 is no page of a 7-page pool
    assert _check_slot_write(fmt, 2, 64, BF16, pos, table, 7, monkeypatch) == 2
