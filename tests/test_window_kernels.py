"""The window mode of the KV-cache kernels (csrc/decode_attention.hip and csrc/prefill_attention.hip, the ``*_win``
entries; ``window=`` of the position and paged wrappers of ops/attention.py): row (b, hq, t) at position p attends
key j iff ``p - W < j <= p``, W keys with its own, the live range ``[lo, n)`` with ``lo = max(0, n - W)``.

Contracts, for the decode and the prefill kernel alike:

1. every element within ``assert_within`` of fp64 under ``window_mask`` / ``paged_window_mask``, with every key row
   outside ``[lo, n)`` of its sequence poisoned (NaN, or the NaN byte 0x7F), below the window as well as past the
   position (decode: outside every row's own range; prefill, which stages whole tiles: outside the span of its
   sequence's ranges), and the caches and pools inside guarded buffers that stay as they were;
2. where ``W >= n`` for every row the result is the entry's without a window, bit for bit;
3. both e4m3 forms equal the 16-bit window form over the dequantised cache bit for bit (a zero's sign excepted for
   the decode kernel, as in ``test_decode_pos_kernels.py``);
4. the paged form equals the static form over ``gather_pages`` bit for bit, and stays so when every table entry
   wholly below the smallest ``lo`` is ``-1`` or an id outside the pool: such an entry is never loaded;
5. ``window = 0`` is refused with hipErrorInvalidValue and nothing is written;
and for the 16-bit prefill forms bit equality with the masked v1 forward under the window mask.

End to end, the compiled bf16 ``mistral-like`` / ``gemma2-like`` models under a hipGraph decode step give the tokens
and cache buffers of the same program under ``LTA_KV_WINDOW_FUSION=0`` bit for bit.

Tolerance of every rounded output, per element:  ulp(T) * |ref64| + 8 * e32 + 1e-6  (kernel_checks.py); the prefill
kernel's is ``test_prefill_pos_kernels._check_fp64``'s.  Everything is built on the GPU once per case and reused."""
import pytest
import torch

import lightning_thunder_amd as thunder
from kernel_checks import BF16, F16, F32, _dt_id, assert_guard_intact, assert_within, bits_equal, guarded
from test_decode_kernels import ref_attention
from test_decode_pos_kernels import LAUNCH_SHAPES, _kv_case, _position_sets
from test_prefill_pos_kernels import _check_fp64, _masked_v1
from test_ragged_generate import FORMATS as CACHE_FORMATS, _model

from lightning_thunder_amd.models.litgpt import generate
from lightning_thunder_amd.ops.kv_pages import PageTable, gather_pages, paged_window_mask, write_slots
from lightning_thunder_amd.ops.kv_rows import window_mask

gpu = pytest.mark.gpu
U8, I64 = torch.uint8, torch.int64
FORMATS = ["16bit", "kv8", "kv8s"]
PAGE = 16
SPARE_PAGES = 3
TYPES = [(64, BF16), (64, F16), (128, BF16), (128, F16)]
_type_id = lambda p: f"D{p[0]}_{_dt_id(p[1])}"  # noqa: E731
INVALID = 1  # hipErrorInvalidValue


def _entry(kind, fmt, paged, win=True):
    name = {"16bit": f"lta_{kind}_attn", "kv8": f"lta_{kind}_attn_kv8", "kv8s": f"lta_{kind}_attn_kv8s"}[fmt]
    return name + ("_paged" if paged else "_pos") + ("_win" if win else "")


def _wrapper(kind, fmt, paged):
    from lightning_thunder_amd.ops import attention as A

    return getattr(A, _entry(kind, fmt, paged, win=False)[len("lta_"):])


@pytest.fixture
def spy(monkeypatch):
    """Records (entry, wsplit, nsplit) of every native decode launch by positions, and the name of every prefill one."""
    import lightning_thunder_amd.ops.attention  # noqa: F401
    from lightning_thunder_amd.ops import require

    lib = require()
    calls = []
    for fmt in FORMATS:
        off = 2 if fmt == "kv8s" else 0
        for paged in (False, True):
            for win in (False, True):
                name = _entry("decode", fmt, paged, win)

                def record(*a, _real=getattr(lib, name), _name=name, _off=off):
                    calls.append((_name, bool(a[17 + _off]), int(a[15 + _off])))
                    return _real(*a)

                monkeypatch.setattr(lib, name, record)
                name = _entry("prefill", fmt, paged, win)

                def record_prefill(*a, _real=getattr(lib, name), _name=name):
                    calls.append((_name,))
                    return _real(*a)

                monkeypatch.setattr(lib, name, record_prefill)
    return calls


# ------------------------------------------------------------------------------------------------
# operands on the GPU: poisoned caches in guarded buffers, static and paged
# ------------------------------------------------------------------------------------------------
def _table(B, S, seed=0):
    """A shuffled block table [B, S / 16] over ``B * S / 16 + SPARE_PAGES`` pages on the GPU, and that page count."""
    P = S // PAGE
    num_pages = B * P + SPARE_PAGES
    g = torch.Generator().manual_seed(seed + S)
    table = torch.randperm(num_pages, generator=g)[:B * P].view(B, P).to(I64)
    assert not torch.equal(table.flatten(), torch.arange(B * P)), "the table is no identity"
    return table.cuda(), num_pages


class _Operands:
    """q and a cache of one format on the GPU, as the static and the paged entries take it, with every key row that
    ``live`` [B, S] does not name poisoned: NaN in a 16-bit cache, the byte 0x7F in an e4m3 one (scale bytes stay
    valid exponents); every pool row without a key (spare pages, the sink) is poisoned too.  The caches are views of
    larger poisoned buffers, the 16-bit pools of sentinel-guarded ones."""

    def __init__(self, B, Hq, Hkv, T, S, D, dtype, fmt, seed, paged):
        q, caches, exact = _kv_case(B, Hq, Hkv, T, S, D, dtype, fmt, seed=seed)
        self.q, self.caches, self.exact = q.cuda(), [c.cuda() for c in caches], [e.cuda() for e in exact]
        self.fmt, self.dtype, self.S, self.paged = fmt, dtype, S, paged
        if paged:
            self.table, self.num_pages = _table(B, S, seed)
            j = torch.arange(S, device="cuda")
            self.slots = self.table[:, j // PAGE] * PAGE + j % PAGE  # [B, S]: every key's pool row

    @staticmethod
    def _poison_value(c):
        return 0x7F if c.dtype == U8 else float("nan")

    def poisoned(self, live):
        """(the caches or pools for the kernel, their buffers, the exact fp32 values with zeros at the dead keys)."""
        dead = ~live[:, None, :, None]
        views, bufs = [], []
        for c in self.caches:
            B, H, S, d = c.shape
            scales = c.dtype == U8 and d == 1
            logical = c if scales else c.masked_fill(dead, self._poison_value(c))
            if self.paged:
                R = self.num_pages * PAGE
                if c.dtype == U8:
                    buf = torch.full((H, R + 1 + 8, d + 16 if d > 1 else 3), 127 if scales else 0x7F, dtype=U8, device="cuda")
                    view = buf[:, :R + 1, :d]
                else:
                    buf, view = guarded((H, R + 1, d), "cuda", dtype=c.dtype)
                    view.fill_(float("nan"))
                write_slots(view, self.slots, logical)
            else:
                if c.dtype == U8:
                    buf = torch.full((B, H, S + 16, d + (16 if d > 1 else 2)), 0x7F, dtype=U8, device="cuda")
                else:
                    buf = torch.full((B, H, S + 8, d + 8), float("nan"), dtype=c.dtype, device="cuda")
                view = buf[:, :, :S, :d]
                view.copy_(logical)
            views.append(view)
            bufs.append(buf)
        return views, bufs, [e.masked_fill(dead, 0.0) for e in self.exact]

    def dequantised(self, exact):
        """The exact values in the activation dtype (exact: e4m3 values and their power-of-two multiples fit)."""
        kd, vd = (e.to(self.dtype) for e in exact)
        assert torch.equal(kd.float(), exact[0]) and torch.equal(vd.float(), exact[1])
        return kd, vd


def _words(buf):
    """A buffer as integers (a NaN-filled one compares equal to its copy)."""
    return buf.view(torch.int16) if buf.is_floating_point() else buf


def _launch(kind, fmt, ops, views, pos, window=None, table=None):
    fn = _wrapper(kind, fmt, ops.paged)
    if ops.paged:
        return fn(ops.q, *views, pos, ops.table if table is None else table, PAGE, ops.num_pages, None, window=window)
    return fn(ops.q, *views, pos, None, window=window)


def _static_16bit(kind, q, kd, vd, pos, window=None):
    return _wrapper(kind, "16bit", False)(q, kd, vd, pos, None, window=window)


def _holes(table, pos, S, window, num_pages):
    """``table`` with every entry wholly below the smallest ``lo`` of its sequence's rows that attend anything
    replaced: (by -1, by ids outside the pool, the number of entries replaced)."""
    n = (pos + 1).clamp(0, S)
    lo = (pos + 1 - window).clamp(min=0).minimum(n)
    lo = torch.where(n > 0, lo, torch.full_like(lo, S)).min(dim=1).values  # [B]
    below = torch.arange(table.shape[1], device=table.device)[None, :] < (lo // PAGE)[:, None]
    bad = torch.where(torch.arange(table.shape[1], device=table.device)[None, :] % 2 == 0, num_pages, 2 ** 40)
    return table.masked_fill(below, -1), torch.where(below, bad.expand_as(table), table), int(below.sum())


def _same_but_zero_signs(out, ref):
    zero = ref == 0
    assert zero.float().mean().item() < 1e-2 and (out[zero] == 0).all()
    return bits_equal(out.masked_fill(zero, 0), ref.masked_fill(zero, 0))


# ------------------------------------------------------------------------------------------------
# decode
# ------------------------------------------------------------------------------------------------
def _decode_windows(S):
    return [1, 5, 64, 65, 200, S, S + 9]


def test_decode_cases_put_lo_where_the_kernel_branches_cpu():
    """Windows and positions together put lo at 0, 63, 64, inside the last split and at n - 1 (no GPU)."""
    for (B, Hq, Hkv, T, S), (_, nsplit) in LAUNCH_SHAPES.values():
        los, full = set(), 0
        for W in _decode_windows(S):
            for pos in _position_sets(B, T, S):
                n = pos + 1
                lo = (n - W).clamp(min=0)
                los |= {(int(a), int(b)) for a, b in zip(lo.flatten(), n.flatten())}
                full += bool((W >= n).all())
        assert {lo for lo, _ in los} >= {0, 63, 64} and full >= 2
        assert any(lo == n - 1 for lo, n in los) and any(lo > S - 64 for lo, _ in los)
        assert any(lo % 64 and lo > 64 for lo, _ in los), "a window that starts inside a 64-key block"


@gpu
@pytest.mark.parametrize("paged", [False, True], ids=["static", "paged"])
@pytest.mark.parametrize("D,dtype", TYPES, ids=[_type_id(p) for p in TYPES])
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("shape", list(LAUNCH_SHAPES))
def test_decode_attn_window(shape, fmt, D, dtype, paged, spy):
    from lightning_thunder_amd.ops.attention import decode_launch_shape

    (B, Hq, Hkv, T, S), (wsplit, nsplit) = LAUNCH_SHAPES[shape]
    assert decode_launch_shape(B * Hq * T, S)[:2] == (wsplit, nsplit) and S % PAGE == 0
    ops = _Operands(B, Hq, Hkv, T, S, D, dtype, fmt, S + D, paged)
    sets = [p.cuda() for p in _position_sets(B, T, S)]
    sets.append((S - 1 - 3 * torch.arange(B * T, device="cuda")).view(B, T))  # every row deep: whole pages lie below
    no_window_runs = holes = 0
    for W in _decode_windows(S):
        for n_set, pos in enumerate(sets):
            what = f"{shape} {fmt} D{D} paged={paged} W{W} set {n_set}"
            mask = window_mask(pos, S, W)
            views, bufs, (k, v) = ops.poisoned(mask.any(dim=2)[:, 0])
            before = [b.clone() for b in bufs]
            del spy[:]
            out = _launch("decode", fmt, ops, views, pos, W)
            assert spy == [(_entry("decode", fmt, paged), wsplit, nsplit)], spy
            assert out.dtype == dtype and out.shape == ops.q.shape and out.is_contiguous()
            # 1. fp64 under the window mask; nothing outside [lo, n) was consumed, nothing was written
            assert torch.isfinite(out).all(), f"{what}: a key outside the window was consumed"
            ref64 = ref_attention(ops.q, k, v, mask, False, D ** -0.5)
            ref32 = ref_attention(ops.q, k, v, mask, False, D ** -0.5, F32)
            assert_within(out, ref64, ref32, dtype, f"decode attention window {fmt}", what)
            for buf, old, view in zip(bufs, before, views):
                assert torch.equal(_words(buf), _words(old)), f"{what}: a cache buffer was written"
                if buf.dtype == torch.int16:
                    assert_guard_intact(buf, view.shape, what)
            # 2. a window no row reaches the start of: the entry without a window
            if bool((W >= pos + 1).all()):
                plain = _launch("decode", fmt, ops, views, pos)
                assert spy[-1][0] == _entry("decode", fmt, paged, win=False)
                assert bits_equal(out, plain), f"{what}: {(out != plain).sum().item()} elements differ from no window"
                no_window_runs += 1
            # 3. / 4. the 16-bit static window form over the dequantised (gathered) cache
            kd, vd = ops.dequantised((k, v))
            ref16 = _static_16bit("decode", ops.q, kd, vd, pos, W)
            if fmt == "16bit":
                assert bits_equal(out, ref16), f"{what}: {(out != ref16).sum().item()} elements differ from the static form"
            else:
                assert _same_but_zero_signs(out, ref16), f"{what}: differs from the 16-bit form"
            if paged:
                gathered = [gather_pages(p, ops.table, PAGE) for p in views]
                static = _wrapper("decode", fmt, False)(ops.q, *gathered, pos, None, window=W)
                assert bits_equal(out, static), f"{what}: differs from the static form over gather_pages"
                minus, outside, n_holes = _holes(ops.table, pos, S, W, ops.num_pages)
                if n_holes:
                    holes += 1
                    for tab in (minus, outside):
                        again = _launch("decode", fmt, ops, views, pos, W, table=tab)
                        assert bits_equal(out, again), f"{what}: a table entry below the window was read"
    assert no_window_runs >= 2 and (holes >= 2 or not paged)


# ------------------------------------------------------------------------------------------------
# prefill
# ------------------------------------------------------------------------------------------------
PREFILL_HEADS, PREFILL_S = (2, 4, 2), 320
PREFILL_T = [17, 130, 200]
PREFILL_W = [1, 17, 64, 100, 129, PREFILL_S + 1]


def _prefill_positions(T):
    """Three int64 [B, T] sets: chunks at base 0 and 100, and a shuffled, non-monotone one; each with one row at -1
    (no key at all, in a tile whose other rows are live)."""
    B = PREFILL_HEADS[0]
    sets = []
    for c0 in (0, 100):
        pos = torch.arange(c0, c0 + T).expand(B, T).clone()
        pos[1] += 7
        sets.append(pos)
    g = torch.Generator().manual_seed(T)
    sets.append(torch.stack([torch.randperm(PREFILL_S - 20, generator=g)[:T] + 10 * b for b in range(B)]))
    for i, pos in enumerate(sets):
        pos[i % B, (5 * i + 3) % T] = -1
        assert int(pos.max()) < PREFILL_S
    assert (sets[2][0, 1:] < sets[2][0, :-1]).any()
    return [p.to(I64) for p in sets]


def _span(pos, S, W):
    """bool [B, S]: the keys from a sequence's lowest window start to its highest position.  The prefill kernel stages
    whole key tiles between its workgroup's lowest ``lo`` and highest ``n`` (a key in a gap between two rows' windows
    is staged and weighs 0 in every row, as a key past a row's position always has), so this is what may be read: every
    key below every window and past every position is poisoned."""
    n = (pos + 1).clamp(0, S)
    lo = (pos + 1 - W).clamp(min=0).minimum(n)
    first = torch.where(n > 0, lo, torch.full_like(lo, S)).min(dim=1).values
    j = torch.arange(S, device=pos.device)
    return (j >= first[:, None]) & (j < n.max(dim=1).values[:, None])


@gpu
@pytest.mark.parametrize("paged", [False, True], ids=["static", "paged"])
@pytest.mark.parametrize("D,dtype", TYPES, ids=[_type_id(p) for p in TYPES])
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("T", PREFILL_T)
def test_prefill_attn_window(T, fmt, D, dtype, paged, spy):
    (B, Hq, Hkv), S = PREFILL_HEADS, PREFILL_S
    ops = _Operands(B, Hq, Hkv, T, S, D, dtype, fmt, T + D, paged)
    no_window_runs = holes = skipped_tiles = 0
    for W in PREFILL_W:
        for n_set, pos in enumerate(_prefill_positions(T)):
            what = f"T{T} {fmt} D{D} paged={paged} W{W} set {n_set}"
            pos = pos.cuda()
            mask = window_mask(pos, S, W)
            views, bufs, (k, v) = ops.poisoned(_span(pos, S, W))
            before = [b.clone() for b in bufs]
            del spy[:]
            out = _launch("prefill", fmt, ops, views, pos, W)
            assert spy == [(_entry("prefill", fmt, paged),)], spy
            assert out.dtype == dtype and out.shape == ops.q.shape
            # 1. fp64 under the window mask; rows without a key are zeros
            assert torch.isfinite(out).all(), f"{what}: a key outside the window was consumed"
            assert _check_fp64(out, ops.q, k, v, mask, dtype, what) == 1
            for buf, old, view in zip(bufs, before, views):
                assert torch.equal(_words(buf), _words(old)), f"{what}: a cache buffer was written"
                if buf.dtype == torch.int16:
                    assert_guard_intact(buf, view.shape, what)
            # the masked v1 forward under the window mask, over zeros in place of the poison
            kd, vd = ops.dequantised((k, v))
            v1 = _masked_v1(ops.q, kd, vd, mask)
            assert bits_equal(out, v1), f"{what}: {(out != v1).sum().item()} elements differ from the masked v1 forward"
            # 2. no row reaches the start of its window
            if bool((W >= pos + 1).all()):
                plain = _launch("prefill", fmt, ops, views, pos)
                assert spy[-1] == (_entry("prefill", fmt, paged, win=False),)
                assert bits_equal(out, plain), f"{what}: {(out != plain).sum().item()} elements differ from no window"
                no_window_runs += 1
            # 3. / 4.
            ref16 = _static_16bit("prefill", ops.q, kd, vd, pos, W)
            assert bits_equal(out, ref16), f"{what}: {(out != ref16).sum().item()} elements differ from the 16-bit form"
            n = (pos + 1).clamp(0, S)
            skipped_tiles += int(((n - W).clamp(min=0)[n > 0].min() // 64) > 0)
            if paged:
                gathered = [gather_pages(p, ops.table, PAGE) for p in views]
                static = _wrapper("prefill", fmt, False)(ops.q, *gathered, pos, None, window=W)
                assert bits_equal(out, static), f"{what}: differs from the static form over gather_pages"
                minus, outside, n_holes = _holes(ops.table, pos, S, W, ops.num_pages)
                if n_holes:
                    holes += 1
                    for tab in (minus, outside):
                        again = _launch("prefill", fmt, ops, views, pos, W, table=tab)
                        assert bits_equal(out, again), f"{what}: a table entry below the window was read"
    assert no_window_runs >= 3 and (holes >= 1 or not paged)
    assert skipped_tiles >= 1, "some case starts its tile loop past tile 0"


# ------------------------------------------------------------------------------------------------
# refusals
# ------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("paged", [False, True], ids=["static", "paged"])
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("kind", ["decode", "prefill"])
def test_window_zero_is_refused_and_nothing_is_written(kind, fmt, paged, spy, monkeypatch):
    """The native ``*_win`` entry with window = 0 (the wrapper's own check taken out of the way) returns
    hipErrorInvalidValue and launches nothing: every buffer the wrapper allocated still holds its fill."""
    from lightning_thunder_amd.ops import attention as A

    B, Hq, Hkv, T, S, D = 2, 4, 2, (2 if kind == "decode" else 20), 640, 64
    ops = _Operands(B, Hq, Hkv, T, S, D, BF16, fmt, 9, paged)
    pos = torch.full((B, T), S - 1, dtype=I64, device="cuda")
    views, _, _ = ops.poisoned(torch.ones(B, S, dtype=torch.bool, device="cuda"))
    for bad in (0, -3, 2.0, True, "4"):
        with pytest.raises(ValueError, match="window"):
            _launch(kind, fmt, ops, views, pos, bad)
    assert spy == []
    made, empty = [], torch.empty

    def filled(*a, **kw):
        t = empty(*a, **kw)
        if t.is_cuda:
            made.append(t.view(torch.int16 if t.element_size() == 2 else torch.int32).fill_(0x5A3C))
        return t

    monkeypatch.setattr(A, "_window_arg", lambda fn, window: (window,))
    monkeypatch.setattr(torch, "empty", filled)
    with pytest.raises(RuntimeError, match=f"{_entry(kind, fmt, paged)} failed with HIP error code {INVALID}"):
        _launch(kind, fmt, ops, views, pos, 0)
    monkeypatch.setattr(torch, "empty", empty)
    torch.cuda.synchronize()
    assert len(made) == (3 if kind == "decode" else 1), "the output (and the decode kernel's two split buffers)"
    assert all(bool((t == 0x5A3C).all()) for t in made), "a refused launch wrote something"
    assert [c[0] for c in spy] == [_entry(kind, fmt, paged)]
    out = _launch(kind, fmt, ops, views, pos, 1)  # the same operands with a window of one key are taken
    assert torch.isfinite(out).all()


# ------------------------------------------------------------------------------------------------
# end to end: the compiled models, fused against LTA_KV_WINDOW_FUSION=0
# ------------------------------------------------------------------------------------------------
E2E_LENGTHS, E2E_NEW, E2E_CACHE = (40, 9), 60, 128
E2E_CASES = [("mistral-like", route, fmt, None) for route in ("ragged", "paged") for fmt in CACHE_FORMATS] + \
    [("mistral-like", "ragged", "16bit", 16), ("mistral-like", "paged", "e4m3_row", 16),
     ("gemma2-like", "ragged", "16bit", None), ("gemma2-like", "paged", "16bit", None),
     ("gemma2-like", "paged", "e4m3_row", 16)]
_WINDOW_OPS = ("kv_window_mask", "kv_paged_window_mask")


def _bf16_model(name):
    kw = dict(n_layer=2, n_embd=256, n_head=4, n_query_groups=2, head_size=64, intermediate_size=384)
    m32 = _model(name, device="cuda", dtype=torch.float32, **kw)
    return m32.to(torch.bfloat16)


def _prompt():
    g = torch.Generator().manual_seed(8)
    prompt = torch.randint(1, 300, (len(E2E_LENGTHS), max(E2E_LENGTHS)), generator=g)
    return prompt.cuda(), torch.tensor(E2E_LENGTHS, device="cuda")


def _compiled_generate(m, route, fmt, chunk, num_pages=None):
    """(tokens, every cache buffer at the end, the symbol names of every program compiled)."""
    from lightning_thunder_amd.transforms.hipgraph import HipGraphTransform

    kw = dict(page_size=PAGE, num_pages=num_pages) if route == "paged" else {}
    m.set_kv_cache(len(E2E_LENGTHS), E2E_CACHE, device=torch.device("cuda"), **kw, **CACHE_FORMATS[fmt])
    jm = thunder.jit(m, transforms=[HipGraphTransform()])
    names = []

    def fwd(idx, pos):
        misses = thunder.cache_misses(jm)
        out = jm(idx, pos)
        if thunder.cache_misses(jm) != misses:
            names.append([s.sym.name for b in thunder.last_traces(jm)[-1].bound_symbols
                          for s in (b.subsymbols if b.sym.name.startswith("HipGraph") else [b])])
        return out

    prompt, lengths = _prompt()
    out = generate(m, prompt, E2E_NEW, forward=fwd, prompt_lengths=lengths, pad_id=0, prefill_chunk=chunk)
    buffers = [b.clone() for block in m.transformer.h for b in block.attn.kv_cache.buffers()]
    return out, buffers, names


@gpu
@pytest.mark.parametrize("name,route,fmt,chunk", E2E_CASES, ids=["-".join(map(str, c)) for c in E2E_CASES])
def test_compiled_generate_equals_the_unfused_program(name, route, fmt, chunk, monkeypatch):
    """Positions run to 98, so the decode step's window starts past key 64.  The whole-prompt prefill of the paged
    route (40 rows at 2-D positions) reads through the prefill kernel, a chunked one through the decode kernel too (16
    and 8 rows); the ragged route's whole-prompt prefill runs at the shared 1-D positions on the masked flash kernel,
    as ever.  ``mistral-like`` on the paged route trims as it goes, the same way in both runs."""
    m = _bf16_model(name)
    out, buffers, names = _compiled_generate(m, route, fmt, chunk)
    flat = [n for program in names for n in program]
    assert len(names) >= 2 and not any(w in n for n in flat for w in _WINDOW_OPS), "the fused programs hold no window mask"
    layers = 2 if name == "mistral-like" else 1
    step = names[-1]  # the decode step: one window attention per windowed layer, the plain form for the others
    assert sum(n.startswith("hip_decode_attn") and n.endswith("_win") for n in step) == layers, step
    assert sum(n.startswith("hip_decode_attn") for n in step) == 2, step
    if route == "paged" and chunk is None:
        assert sum(n.startswith("hip_prefill_attn") and n.endswith("_win") for n in names[0]) == layers, names[0]
    if chunk is not None:
        assert all(sum(n.endswith("_win") for n in program) == layers for program in names), names
    monkeypatch.setenv("LTA_KV_WINDOW_FUSION", "0")
    ref, ref_buffers, ref_names = _compiled_generate(m, route, fmt, chunk)
    ref_flat = [n for program in ref_names for n in program]
    assert not any(n.endswith("_win") for n in ref_flat) and any(w in n for n in ref_flat for w in _WINDOW_OPS)
    assert torch.equal(out, ref), f"{(out != ref).sum().item()} tokens differ from the unfused program"
    assert len(buffers) == len(ref_buffers)
    for got, want in zip(buffers, ref_buffers):
        assert torch.equal(got, want), "a cache buffer differs from the unfused program's"


@gpu
@pytest.mark.parametrize("chunk", [None, 16])
def test_compiled_paged_generate_with_trimming_equals_a_pool_that_needs_none(chunk, monkeypatch):
    """mistral-like on a pool of B * 4 pages (64 rows per sequence for 99 positions) against the same run on a static
    cache's pool with ``PageTable.trim`` switched off: the same tokens."""
    m = _bf16_model("mistral-like")
    B = len(E2E_LENGTHS)
    out, _, _ = _compiled_generate(m, "paged", "16bit", chunk, num_pages=B * 4)
    assert 0 < m.kv_pages.peak_pages_in_use <= B * 3
    monkeypatch.setattr(PageTable, "trim", lambda self, first_live: None)
    ref, _, _ = _compiled_generate(m, "paged", "16bit", chunk)
    assert m.kv_pages.peak_pages_in_use == sum(-(-(n + E2E_NEW - 1) // PAGE) for n in E2E_LENGTHS)
    assert torch.equal(out, ref)
