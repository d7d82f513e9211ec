"""The prefill attention kernel that reads a KV cache by positions (csrc/prefill_attention.hip; ``prefill_attn_pos``,
``prefill_attn_kv8_pos``, ``prefill_attn_kv8s_pos`` and the three ``*_paged`` forms): row (b, hq, t) attends keys
``0 .. n-1`` with ``n = clamp(pos[b, t] + 1, 0, S)``, on a paged cache those whose table entry is a page.

Contracts, per element:

* the 16-bit forms equal what they replace bit for bit: ``attn_fwd(q, k, v, causal=False, mask=position_mask(pos,
  S))[0]`` (the masked v1 forward), rows without a live key included (zeros); the paged form the same call over the
  logical cache under ``paged_mask``;
* every e4m3 form, static and paged, equals the 16-bit form over the dequantised cache bit for bit (the LDS tiles are
  the same, so are the MFMA operands);
* against fp64 under the equivalent mask with the forward-O tolerance of ``test_attention_kernels.check``:
  ``R_T(ref) + R_T(P) @ |V| + 8 e32 + 1e-6 max |ref|``; rows without a live key are exact zeros.

Every key row no live key refers to is poisoned (NaN, or the NaN byte 0x7F) and the caches and pools sit in larger
buffers, so a finite result shows that nothing else was read; the masked v1 reference therefore runs over the same
cache with zeros in place of the poison (a dead key contributes 0 * 0 there and nothing here).  Shapes are the
smallest that reach every branch: T = 17 (one partial wave), T = 129 (a second workgroup of one row), T = 160 over
S = 320 with chunk-style positions that cross the 64- and 128-key tile edges, a non-monotone set with dead and
clamped rows, and every row at ``S - 1``.  On a paged cache the capacity is S rounded up to the page size.
"""
import ctypes

import pytest
import torch

from kernel_checks import BF16, F16, F32, _dt_id, assert_guard_intact, assert_within, bits_equal, guarded
from test_attention_kernels import ref_attention
from test_decode_paged_kernels import _pools, _table
from test_decode_pos_kernels import _kv_case, _poisoned

from lightning_thunder_amd.ops.kv_pages import paged_mask
from lightning_thunder_amd.ops.kv_rows import position_mask

gpu = pytest.mark.gpu
U8, I64, F64 = torch.uint8, torch.int64, torch.float64
FORMATS = ["16bit", "kv8", "kv8s"]
POS_ENTRY = {"16bit": "lta_prefill_attn_pos", "kv8": "lta_prefill_attn_kv8_pos", "kv8s": "lta_prefill_attn_kv8s_pos"}
PAGED_ENTRY = {f: e.replace("_pos", "_paged") for f, e in POS_ENTRY.items()}
INVALID = 1  # hipErrorInvalidValue
GQA = (2, 4, 2)  # B, Hq, Hkv
TYPES = [(64, BF16), (64, F16), (128, BF16), (128, F16)]
_type_id = lambda p: f"D{p[0]}_{_dt_id(p[1])}"  # noqa: E731

# name -> (T, S)
CASES = {"t17": (17, 192), "t129": (129, 192), "chunk": (160, 320), "mixed": (160, 320), "last": (160, 320)}


def _positions(name, B, T, S):
    """int64 [B, T] positions of a case (see the module docstring)."""
    t = torch.arange(T)
    if name in ("t17", "t129", "chunk"):
        base = {"t17": (150, 37), "t129": (60, 3), "chunk": (150, 37)}[name]
        pos = torch.stack([base[b % 2] + t for b in range(B)])
        assert int(pos.max()) < S
        return pos.to(I64)
    if name == "last":
        return torch.full((B, T), S - 1, dtype=I64)
    g = torch.Generator().manual_seed(T + S)
    special = [0, 63, 64, 15, 16, 127, 128, S - 1, -1, S + 5]  # tile edges, the edges of every page size, dead, clamped
    rows = []
    for b in range(B):
        vals = torch.cat([torch.tensor(special), torch.randint(0, S, (T - len(special),), generator=g)])
        rows.append(vals[torch.randperm(T, generator=g)])
    pos = torch.stack(rows).to(I64)
    assert set(special) <= {int(x) for x in pos[0]} and (pos[0, 1:] < pos[0, :-1]).any()
    return pos


def _fns(fmt, paged=False):
    from lightning_thunder_amd.ops import attention as A

    return getattr(A, POS_ENTRY[fmt].replace("lta_", "").replace("_pos", "_paged" if paged else "_pos"))


@pytest.fixture
def spy(monkeypatch):
    """Records the name and the q pointer of every native prefill launch."""
    import lightning_thunder_amd.ops.attention  # noqa: F401
    from lightning_thunder_amd.ops import require

    lib = require()
    calls = []
    for name in (*POS_ENTRY.values(), *PAGED_ENTRY.values()):
        def record(*a, _real=getattr(lib, name), _name=name):
            calls.append((_name, a[1]))
            return _real(*a)

        monkeypatch.setattr(lib, name, record)
    return calls


def _check_fp64(out, q, kx, vx, mask, dtype, what):
    """``test_attention_kernels.check`` for the forward O of the masked v1 kernel, on this test's operands."""
    out, q, kx, vx, mask = (t.cpu() for t in (out, q, kx, vx, mask))
    do = torch.zeros_like(q)
    r64 = ref_attention(q, kx, vx, do, mask, dt=F64, model=dtype)
    r32 = ref_attention(q, kx, vx, do, mask, dt=F32)
    dead = ~mask.expand(q.shape[0], 1, q.shape[2], mask.shape[3]).any(-1)[:, 0]  # [B, T]
    assert not torch.isnan(out).any(), f"{what}: NaN in the kernel output"
    if dead.any():
        assert not r64["o"].transpose(1, 2)[dead].any()
        assert not out.transpose(1, 2)[dead].any(), f"{what}: a row without a live key must be exactly zero"
    assert_within(out, r64["o"], r32["o"], dtype, "prefill attention O", what, rel_floor=True, extra=r64["x_o"])
    return int(dead.sum())


def _masked_v1(q, k, v, mask):
    from lightning_thunder_amd.ops.attention import attn_fwd

    return attn_fwd(q, k, v, causal=False, mask=mask)[0]


def _run_static(name, fmt, D, dtype, heads, spy):
    B, Hq, Hkv = heads
    T, S = CASES[name]
    what = f"{name} {fmt} D{D} {_dt_id(dtype)}"
    q, caches, exact = _kv_case(B, Hq, Hkv, T, S, D, dtype, fmt, seed=T + S + D)
    q, pos = q.cuda(), _positions(name, B, T, S)
    poisoned, (kx, vx) = _poisoned(caches, exact, pos, fmt)
    posg = pos.cuda()
    del spy[:]
    out = _fns(fmt)(q, *poisoned, posg)
    assert [c[0] for c in spy] == [POS_ENTRY[fmt]], spy
    assert out.dtype == dtype and out.shape == q.shape and out.transpose(1, 2).is_contiguous(), "O is stored [B, T, Hq, D]"
    assert torch.isfinite(out).all(), f"{what}: a key past its sequence's last position was consumed"
    mask = position_mask(posg, S)
    n_dead = _check_fp64(out, q, kx, vx, mask, dtype, what)
    assert n_dead == int((pos < 0).sum()) and (n_dead > 0) == (name == "mixed")
    k16, v16 = kx.to(dtype), vx.to(dtype)  # the (dequantised) cache with zeros at the poisoned rows: exact in T
    assert torch.equal(k16.float(), kx) and torch.equal(v16.float(), vx)
    ref = _masked_v1(q, k16, v16, mask)
    assert bits_equal(out, ref), f"{what}: {(out != ref).sum().item()} elements differ from the masked v1 forward"
    if fmt != "16bit":
        ref16 = _fns("16bit")(q, k16, v16, posg)
        assert spy[-1][0] == POS_ENTRY["16bit"]
        assert bits_equal(out, ref16), f"{what}: {(out != ref16).sum().item()} elements differ from the 16-bit form"


@gpu
@pytest.mark.parametrize("D,dtype", TYPES, ids=[_type_id(p) for p in TYPES])
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("name", list(CASES))
def test_prefill_attn_pos_against_fp64_and_the_masked_forward(name, fmt, D, dtype, spy):
    _run_static(name, fmt, D, dtype, GQA, spy)


@gpu
@pytest.mark.parametrize("fmt", FORMATS)
def test_prefill_attn_pos_mha(fmt, spy):
    _run_static("t129", fmt, 64, BF16, (1, 2, 2), spy)


# ------------------------------------------------------------------------------------------------
# paged caches
# ------------------------------------------------------------------------------------------------
def _run_paged(name, fmt, page, D, dtype, spy, holes=False):
    B, Hq, Hkv = GQA
    T, S0 = CASES[name]
    S = -(-S0 // page) * page  # the table's capacity
    what = f"{name} {fmt} page{page} D{D} {_dt_id(dtype)}{' holes' if holes else ''}"
    q, caches, exact = _kv_case(B, Hq, Hkv, T, S, D, dtype, fmt, seed=T + S + D + page)
    q, pos = q.cuda(), _positions(name, B, T, S0)
    table, num_pages = _table(B, S, page)
    P = S // page
    if holes:
        assert P >= 3
        table[0, P // 2] = -1  # a dropped entry in the middle of sequence 0: later pages stay live
        table[B - 1, 0] = num_pages  # the first page past the pool: rows of the last sequence below `page` see no key
    pools, bufs, (kx, vx) = _pools(caches, exact, pos, table, page, num_pages, fmt)
    before = [b.clone() for b in bufs]
    posg, tabg = pos.cuda(), table.cuda()
    del spy[:]
    out = _fns(fmt, paged=True)(q, *pools, posg, tabg, page, num_pages)
    assert [c[0] for c in spy] == [PAGED_ENTRY[fmt]], spy
    assert out.dtype == dtype and out.shape == q.shape
    assert torch.isfinite(out).all(), f"{what}: a pool row no live key refers to was consumed"
    for buf, old, pool in zip(bufs, before, pools):
        assert torch.equal(buf, old), f"{what}: a pool buffer was written"
        if buf.dtype == torch.int16:
            assert_guard_intact(buf, pool.shape, what)
    mask = paged_mask(posg, tabg, page, num_pages)
    n_dead = _check_fp64(out, q, kx, vx, mask, dtype, what)
    if holes:
        assert n_dead >= int((pos[B - 1] < page).sum()), "a row of the last sequence below `page` has no live key"
        assert name != "mixed" or n_dead > int((pos < 0).sum())
        live_after = mask[0, 0, :, (P // 2 + 1) * page:].any()
        assert live_after, "keys behind the dropped page stay live"
    k16, v16 = kx.to(dtype), vx.to(dtype)  # gather_pages of the pools, zeros in place of the poison
    ref = _masked_v1(q, k16, v16, mask)
    assert bits_equal(out, ref), f"{what}: {(out != ref).sum().item()} elements differ from the masked v1 forward"
    if not holes:  # every key below a position is live: the position form over the gathered cache is the same sum
        ref16 = _fns("16bit")(q, k16, v16, posg)
        assert bits_equal(out, ref16), f"{what}: {(out != ref16).sum().item()} elements differ from the position form"


@gpu
@pytest.mark.parametrize("D,dtype", [(64, BF16), (128, F16)], ids=["D64_bf16", "D128_fp16"])
@pytest.mark.parametrize("page", [16, 64, 128])
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("name", list(CASES))
def test_prefill_attn_paged_against_fp64_and_the_masked_forward(name, fmt, page, D, dtype, spy):
    _run_paged(name, fmt, page, D, dtype, spy)


@gpu
@pytest.mark.parametrize("D,dtype", [(64, F16), (128, BF16)], ids=["D64_fp16", "D128_bf16"])
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("name,page", [("t17", 16), ("chunk", 64), ("mixed", 128)])
def test_prefill_attn_paged_other_type_pairs(name, page, fmt, D, dtype, spy):
    _run_paged(name, fmt, page, D, dtype, spy)


@gpu
@pytest.mark.parametrize("page", [16, 64, 128])
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("name", ["chunk", "mixed"])
def test_table_holes_and_bad_entries_are_dead_keys(name, fmt, page, spy):
    """A ``-1`` in the middle of a sequence and an entry equal to ``num_pages``: their keys are dead like masked ones
    and nothing of them is read (their pages' rows are poisoned), later pages stay live, and a row whose every key is
    dead yields zeros."""
    _run_paged(name, fmt, page, 64, BF16, spy, holes=True)


# ------------------------------------------------------------------------------------------------
# the native entries: guarded output, refusals, strided q
# ------------------------------------------------------------------------------------------------
def _native(fmt, q, caches, pos, o, pages=None, **over):
    """One call of the native entry with the wrapper's argument list, any of it replaced through ``over``."""
    from lightning_thunder_amd.ops import require
    from lightning_thunder_amd.ops._lib import dcode, ptr, stream_ptr

    lib = require()
    B, Hq, T, D = q.shape
    k, v, *scales = caches
    if pages is not None:
        table, page, num_pages = pages
        a = dict(Hkv=k.shape[0], S=table.shape[1] * page, lg_page=page.bit_length() - 1, num_pages=num_pages, table=ptr(table))
        cst = lambda c: (0, *c.stride()[:2])  # noqa: E731
        tab_st = tuple(table.stride())
    else:
        a = dict(Hkv=k.shape[1], S=k.shape[2])
        cst = lambda c: tuple(c.stride()[:3])  # noqa: E731
        tab_st = ()
    a.update(Hq=Hq, k=ptr(k), v=ptr(v), scales=[ptr(s) for s in scales], k_st=cst(k))
    a.update(over)
    st = (*q.stride()[:3], *a["k_st"], *cst(v), *pos.stride(), *(s for c in scales for s in cst(c)), *tab_st)
    st = (ctypes.c_int64 * len(st))(*st)
    ost = (ctypes.c_int64 * 3)(*o.stride()[:3])
    tail = (a["table"], a["lg_page"], a["num_pages"]) if pages is not None else ()
    entry = (PAGED_ENTRY if pages is not None else POS_ENTRY)[fmt]
    return getattr(lib, entry)(dcode(q), ptr(q), a["k"], a["v"], *a["scales"], ptr(pos), ptr(o), B, a["Hq"], a["Hkv"], T,
                               a["S"], D, ctypes.cast(st, ctypes.c_void_p), ctypes.cast(ost, ctypes.c_void_p),
                               float(D ** -0.5), *tail, stream_ptr(q.device))


def _guarded_out(B, Hq, T, D, dtype):
    buf, view = guarded((B, T, Hq, D), "cuda", dtype=dtype)
    return buf, view.transpose(1, 2)


@gpu
@pytest.mark.parametrize("paged", [False, True], ids=["static", "paged"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_output_is_written_inside_its_rows_only(fmt, paged):
    """The output in a sentinel-filled buffer with a longer pitch and more rows: T = 129 ends in a workgroup of one
    row, whose 127 other lanes must store nothing."""
    (B, Hq, Hkv), (T, S), D, dtype, page = GQA, CASES["t129"], 64, BF16, 64
    q, caches, exact = _kv_case(B, Hq, Hkv, T, S, D, dtype, fmt, seed=11)
    q, pos = q.cuda(), _positions("t129", B, T, S)
    buf, o = _guarded_out(B, Hq, T, D, dtype)
    if paged:
        table, num_pages = _table(B, S, page)
        pools, _, _ = _pools(caches, exact, pos, table, page, num_pages, fmt)
        tabg = table.cuda()
        assert _native(fmt, q, pools, pos.cuda(), o, pages=(tabg, page, num_pages)) == 0
        ref = _fns(fmt, True)(q, *pools, pos.cuda(), tabg, page, num_pages)
    else:
        poisoned, _ = _poisoned(caches, exact, pos, fmt)
        assert _native(fmt, q, poisoned, pos.cuda(), o) == 0
        ref = _fns(fmt)(q, *poisoned, pos.cuda())
    torch.cuda.synchronize()
    assert_guard_intact(buf, (B, T, Hq, D), f"{fmt} paged={paged}")
    assert bits_equal(o.contiguous(), ref.contiguous())


@gpu
def test_entries_refuse_and_leave_the_output_untouched(spy):
    """``Hq % Hkv != 0``, ``lg_page = 3``, ``S % page != 0``, null scales and a misaligned e4m3 row: the entry returns
    hipErrorInvalidValue and launches nothing (the sentinel-filled output stays as it is)."""
    (B, Hq, Hkv), (T, S), D, dtype, page = GQA, CASES["t17"], 64, BF16, 16
    pos = _positions("t17", B, T, S).cuda()
    table, num_pages = _table(B, S, page)
    tabg = table.cuda()
    buf, o = _guarded_out(B, Hq, T, D, dtype)
    clean = buf.clone()
    ops = {}
    for fmt in FORMATS:
        q, caches, exact = _kv_case(B, Hq, Hkv, T, S, D, dtype, fmt, seed=5)
        ops[fmt] = (q.cuda(), [c.cuda() for c in caches],
                    _pools(caches, exact, pos.cpu(), table, page, num_pages, fmt)[0])
    q, caches, pools = ops["16bit"]
    q8, caches8, pools8 = ops["kv8"]
    qs, caches_s, pools_s = ops["kv8s"]
    pages = (tabg, page, num_pages)
    k8 = caches8[0]
    off = torch.zeros(k8.numel() + 16, dtype=U8, device="cuda")[8:8 + k8.numel()].view(k8.shape)  # 8 bytes off
    assert off.data_ptr() % 16 == 8
    pitch = torch.zeros((*k8.shape[:3], D + 8), dtype=U8, device="cuda")[..., :D]  # rows 72 bytes apart
    refused = {
        "Hq % Hkv": lambda: _native("16bit", q, caches, pos, o, Hkv=3),
        "Hq % Hkv paged": lambda: _native("16bit", q, pools, pos, o, pages=pages, Hkv=3),
        "lg_page 3": lambda: _native("16bit", q, pools, pos, o, pages=pages, lg_page=3),
        "lg_page 25": lambda: _native("kv8", q8, pools8, pos, o, pages=pages, lg_page=25),
        "S % page": lambda: _native("16bit", q, pools, pos, o, pages=pages, S=S - 8),
        "S % page kv8s": lambda: _native("kv8s", qs, pools_s, pos, o, pages=pages, S=S + 4),
        "num_pages 0": lambda: _native("kv8", q8, pools8, pos, o, pages=pages, num_pages=0),
        "null table": lambda: _native("16bit", q, pools, pos, o, pages=pages, table=None),
        "null scales": lambda: _native("kv8s", qs, caches_s, pos, o, scales=[None, None]),
        "null v scale paged": lambda: _native("kv8s", qs, pools_s, pos, o, pages=pages, scales=[ptr_of(pools_s[2]), None]),
        "e4m3 row off 16 bytes": lambda: _native("kv8", q8, [off, caches8[1]], pos, o),
        "e4m3 row pitch": lambda: _native("kv8", q8, [pitch, caches8[1]], pos, o),
    }
    for what, call in refused.items():
        assert call() == INVALID, what
        torch.cuda.synchronize()
        assert torch.equal(buf, clean), f"{what}: a refused call wrote the output"
    assert _native("16bit", q, caches, pos, o) == 0, "the same operands without the fault are taken"
    torch.cuda.synchronize()
    assert not torch.equal(buf, clean)


def ptr_of(t):
    from lightning_thunder_amd.ops._lib import ptr

    return ptr(t)


@gpu
def test_wrappers_refuse_what_the_kernel_does_not_take(spy):
    from lightning_thunder_amd.ops import attention as A

    (B, Hq, Hkv), (T, S), D, page = GQA, CASES["t17"], 64, 16
    q, (k, v), _ = _kv_case(B, Hq, Hkv, T, S, D, BF16, "16bit")
    q, k, v = q.cuda(), k.cuda(), v.cuda()
    pos = _positions("t17", B, T, S).cuda()
    assert A.prefill_attn_pos_supported(q, k, v, pos)
    q96 = torch.zeros(B, Hq, T, 96, dtype=BF16, device="cuda")
    k96 = torch.zeros(B, Hkv, S, 96, dtype=BF16, device="cuda")
    for args in ((q, k, v, pos.int()), (q, k, v, pos[:, :5]), (q, k[:, :1].expand(B, 3, S, D), v, pos), (q96, k96, k96, pos),
                 (q.float(), k, v, pos), (q, k.half(), v.half(), pos)):
        assert not A.prefill_attn_pos_supported(*args)
        with pytest.raises(ValueError):
            A.prefill_attn_pos(*args)
    table, num_pages = _table(B, S, page)
    kp, vp = (torch.zeros(Hkv, num_pages * page + 1, D, dtype=BF16, device="cuda") for _ in range(2))
    assert A.prefill_attn_paged_supported(q, kp, vp, pos, table.cuda(), page, num_pages)
    for change in (dict(page=24), dict(page=8), dict(num_pages=num_pages + 1), dict(table=table), dict(table=table.cuda().int())):
        a = dict(page=page, num_pages=num_pages, table=table.cuda())
        a.update(change)
        args = (q, kp, vp, pos, a["table"], a["page"], a["num_pages"])
        assert not A.prefill_attn_paged_supported(*args), change
        with pytest.raises(ValueError):
            A.prefill_attn_paged(*args)
    assert spy == [], "a refused call launched something"


@gpu
@pytest.mark.parametrize("fmt", FORMATS)
def test_strided_q_is_read_in_place(fmt, spy):
    """q as the head split of a fused qkv projection ``[B, T, (Hq + 2 Hkv) D]``: the entry gets that buffer's pointer
    and strides, and the result is the dense q's bit for bit."""
    (B, Hq, Hkv), (T, S), D, dtype = GQA, CASES["t129"], 64, BF16
    q, caches, exact = _kv_case(B, Hq, Hkv, T, S, D, dtype, fmt, seed=3)
    pos = _positions("t129", B, T, S)
    poisoned, _ = _poisoned(caches, exact, pos, fmt)
    qkv = torch.randn(B, T, (Hq + 2 * Hkv) * D, device="cuda").to(dtype)
    view = qkv[..., :Hq * D].view(B, T, Hq, D).transpose(1, 2)
    view.copy_(q)
    assert not view.is_contiguous()
    out = _fns(fmt)(view, *poisoned, pos.cuda())
    assert spy[-1] == (POS_ENTRY[fmt], view.data_ptr()), "q was copied"
    ref = _fns(fmt)(q.cuda(), *poisoned, pos.cuda())
    assert bits_equal(out.contiguous(), ref.contiguous())


def test_positions_of_the_cases_cpu():
    """The position sets hold what the module docstring says (no GPU)."""
    B = GQA[0]
    for name, (T, S) in CASES.items():
        pos = _positions(name, B, T, S)
        assert pos.shape == (B, T) and pos.dtype == I64
    chunk = _positions("chunk", B, 160, 320)
    n = chunk + 1
    assert (n[0].min() <= 192 < n[0].max()) and (n[1].min() <= 64 < n[1].max()) and (n[1].max() > 128)
    assert not torch.equal(chunk[0], chunk[1])
    mixed = _positions("mixed", B, 160, 320)
    assert {0, 63, 64, 15, 16, 127, 128, 319, -1, 325} <= {int(x) for x in mixed[1]}
