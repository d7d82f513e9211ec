"""Sliding-window attention above the kernels (CPU, fp64): ``Config.sliding_window_size`` / ``sliding_window_indices``,
the mask definitions ``window_mask`` / ``paged_window_mask``, the window of context of ``GPT.forward``, the equivalence
of ``generate``'s routes under a window, ``PageTable.trim`` with the trimming ``generate`` does for a model whose every
layer is windowed, and the ``hipex`` rewrites of the two window masks into the ``*_win`` forms (hand-built traces, the
way ``test_hipex_pos_passes.py`` pins the position forms).

The convention everywhere: the token at position p sees key j iff ``p - W < j <= p``, that is W keys with its own."""
import math

import pytest
import torch

import test_hipex_paged_passes as paged_passes
import test_hipex_pos_passes as pos_passes
import test_hipex_prefill_passes as prefill_passes
from lightning_thunder_amd.executors import hipex
from lightning_thunder_amd.models.litgpt import Config, generate
from lightning_thunder_amd.ops.kv_pages import PageTable, kv_paged_window_mask, paged_mask, paged_window_mask
from lightning_thunder_amd.ops.kv_rows import kv_window_mask, position_mask, window_mask
from lightning_thunder_amd.torch.custom_op import custom_op_symbol, opdef_of
from test_hipex_passes import Program
from test_ragged_generate import FORMATS, _model, _prompts

W, PAGE = 24, 16
F64 = torch.float64


# ------------------------------------------------------------------------------------------------
# Config
# ------------------------------------------------------------------------------------------------
def test_config_fields_and_the_shipped_windows():
    c = Config.from_name("llama3-like")
    assert c.sliding_window_size is None and c.sliding_window_indices is None and c.uniform_window is None
    assert [c.layer_window(i) for i in range(c.n_layer)] == [None, None]
    m = Config.from_name("mistral-like")
    assert m.sliding_window_size == W and m.sliding_window_indices == [1, 1] and m.uniform_window == W
    g = Config.from_name("gemma2-like")
    assert g.sliding_window_indices == [1, 0] and g.uniform_window is None
    assert [g.layer_window(i) for i in range(2)] == [W, None]
    assert Config.from_name("Mistral-7B-v0.1").sliding_window_size == 4096
    assert Config.from_name("Mistral-7B-v0.1").sliding_window_indices == [1] * 32
    assert Config.from_name("Mistral-7B-v0.2").sliding_window_size is None
    assert Config.from_name("mistral-like", n_layer=3).sliding_window_indices == [1, 1, 1]
    assert Config.from_name("mistral-like", sliding_window_size=None).sliding_window_indices is None


@pytest.mark.parametrize("bad", [dict(sliding_window_size=0), dict(sliding_window_size=-4), dict(sliding_window_size=2.5),
                                 dict(sliding_window_size=True), dict(sliding_window_size=8, sliding_window_indices=[1]),
                                 dict(sliding_window_size=8, sliding_window_indices=[1, 0, 1])])
def test_config_refuses_a_bad_window(bad):
    with pytest.raises(ValueError, match="sliding_window"):
        Config.from_name("llama3-like", **bad)


# ------------------------------------------------------------------------------------------------
# the mask definitions
# ------------------------------------------------------------------------------------------------
MASK_S = 40
MASK_POS = torch.tensor([[-1, 0, 5], [MASK_S - 1, MASK_S + 3, 23], [24, 17, 39]])


@pytest.mark.parametrize("window", [1, 7, 40, 55])
def test_window_mask_against_a_triple_loop(window):
    S = MASK_S
    mk = window_mask(MASK_POS, S, window)
    assert mk.shape == (3, 1, 3, S) and mk.dtype == torch.bool
    for b in range(3):
        for t in range(3):
            p = int(MASK_POS[b, t])
            assert mk[b, 0, t].tolist() == [p - window < j <= p for j in range(S)], (b, t)
            if 0 <= p < S:
                assert int(mk[b, 0, t].sum()) == min(window, p + 1), "W keys, the token's own included"
    assert torch.equal(kv_window_mask(MASK_POS, S, window), mk)
    if window >= S:  # no window, for every position inside the cache
        inside = MASK_POS < S
        assert torch.equal(mk[:, 0][inside], position_mask(MASK_POS, S)[:, 0][inside])


@pytest.mark.parametrize("window", [1, 7, 40, 55])
def test_paged_window_mask_against_a_triple_loop(window):
    page, num_pages = 8, 11
    S = MASK_S
    table = torch.tensor([[3, -1, 0, 10, 7], [1, 2, 11, 4, 5], [6, 8, 9, -7, 2 ** 40]])
    mk = paged_window_mask(MASK_POS, table, page, num_pages, window)
    assert mk.shape == (3, 1, 3, S) and mk.dtype == torch.bool
    for b in range(3):
        for t in range(3):
            p = int(MASK_POS[b, t])
            want = [p - window < j <= p and 0 <= int(table[b, j // page]) < num_pages for j in range(S)]
            assert mk[b, 0, t].tolist() == want, (b, t)
    assert torch.equal(kv_paged_window_mask(MASK_POS, table, page, num_pages, window), mk)
    if window >= S:
        inside = MASK_POS < S
        assert torch.equal(mk[:, 0][inside], paged_mask(MASK_POS, table, page, num_pages)[:, 0][inside])


# ------------------------------------------------------------------------------------------------
# the window of context
# ------------------------------------------------------------------------------------------------
def _same_weights(name, like, **kw):
    m = _model(name, dtype=F64, **kw)
    m.load_state_dict(like.state_dict())
    return m


def test_window_of_context_of_the_cacheless_forward():
    """One layer under the identity rotation (cos = 1, sin = 0: no position enters but through the mask): the logits
    at position p of the windowed forward over 60 tokens are those of the model without a window run on the last 24
    tokens up to p alone.  (Through more layers the context grows by W - 1 per layer, so one layer it is.)"""
    T = 60
    m = _model("mistral-like", dtype=F64, n_layer=1)
    ref = _same_weights("llama3-like", m, n_layer=1)
    for mod in (m, ref):
        mod.set_rope_cache(T)
        mod.cos, mod.sin = torch.ones_like(mod.cos), torch.zeros_like(mod.sin)
    idx = torch.randint(1, 300, (2, T), generator=torch.Generator().manual_seed(5))
    logits = m(idx)
    plain = ref(idx)
    assert torch.equal(logits[:, :W], plain[:, :W]), "below W tokens the window hides nothing"
    assert not torch.allclose(logits[:, W:], plain[:, W:], rtol=1e-6, atol=1e-6), "past W tokens it does"
    for p in (W, W + 1, 37, T - 1):
        alone = ref(idx[:, p - W + 1:p + 1])[:, -1]
        torch.testing.assert_close(logits[:, p], alone, rtol=1e-10, atol=1e-10)


@pytest.mark.parametrize("name", ["mistral-like", "gemma2-like"])
def test_positions_below_the_window_equal_the_model_without_one(name):
    """Two layers with RoPE: every route's logits at positions < W are the no-window model's exactly (the same
    operations: a forward of at most W tokens builds no band mask), and past W they differ."""
    m = _model(name, dtype=F64)
    ref = _same_weights("llama3-like", m)
    idx = torch.randint(1, 300, (2, 60), generator=torch.Generator().manual_seed(6))
    for mod in (m, ref):
        mod.set_rope_cache(128)
    assert torch.equal(m(idx[:, :W]), ref(idx[:, :W]))
    full, plain = m(idx), ref(idx)
    assert torch.equal(full[:, :W], plain[:, :W]) or torch.allclose(full[:, :W], plain[:, :W], rtol=1e-12, atol=1e-12)
    assert not torch.allclose(full[:, W:], plain[:, W:], rtol=1e-6, atol=1e-6)
    # the cache routes compute the same logits as the cache-less forward
    for kw, pos in ((dict(), torch.arange(60)), (dict(), torch.arange(60).expand(2, 60).contiguous()),
                    (dict(page_size=PAGE), torch.arange(60).expand(2, 60).contiguous())):
        m.set_kv_cache(2, 112, **kw)
        if m.kv_pages is not None:
            m.kv_pages.reserve([60, 60])
        torch.testing.assert_close(m(idx, pos), full, rtol=1e-10, atol=1e-10)
    m.clear_kv_cache()


def test_a_cache_no_longer_than_the_window_runs_the_global_code():
    """Capacity <= W: no window mask is built on any route (the same ops as a model without a window)."""
    m = _model("mistral-like", dtype=F64)
    m.set_kv_cache(2, W)
    assert m.window_mask_cache is None
    m.set_kv_cache(2, W + 1)
    assert m.window_mask_cache is not None and m.window_mask_cache.shape == (1, 1, W + 1, W + 1)
    assert m.window_mask_cache[0, 0, W].tolist() == [False] + [True] * W
    m.set_kv_cache(2, 112, page_size=PAGE)
    assert m.window_mask_cache is None and m.mask_cache is None


# ------------------------------------------------------------------------------------------------
# generate: one answer on every route
# ------------------------------------------------------------------------------------------------
LENGTHS, NEW, CACHE = (40, 9), 70, 112


def _singles(m, rows, fmt):
    """Each prompt alone on the static 1-D route."""
    outs = []
    for r in rows:
        m.set_kv_cache(1, CACHE, **FORMATS[fmt])
        outs.append(generate(m, r[None], NEW)[0])
    return outs


@pytest.mark.parametrize("fmt", list(FORMATS))
@pytest.mark.parametrize("name", ["mistral-like", "gemma2-like"])
def test_generate_routes_agree_under_a_window(name, fmt):
    """Prompts of 40 and 9 tokens, 70 new tokens (positions up to 109, far past W = 24): the static 1-D route, the
    ragged 2-D route, chunked prefill at 1 / 16 / 64 columns and the paged cache give the same tokens, in every cache
    format against itself.  The window changes the answer: the model without one generates other tokens."""
    m = _model(name, dtype=F64)
    rows, padded, lengths = _prompts(LENGTHS, seed=3)
    singles = _singles(m, rows, fmt)
    if fmt == "16bit":
        plain = _same_weights("llama3-like", m)
        assert any(not torch.equal(a, b) for a, b in zip(singles, _singles(plain, rows, fmt))), \
            "the window must matter at these lengths"

    def check(out, what):
        for b, (n, s) in enumerate(zip(LENGTHS, singles)):
            assert torch.equal(out[b, :n + NEW], s), f"{what}: sequence {b} differs from its own static run"

    for kw, route in ((dict(), "ragged"), (dict(page_size=PAGE), "paged")):
        for chunk in (None, 1, 16, 64):
            m.set_kv_cache(len(LENGTHS), CACHE, **kw, **FORMATS[fmt])
            check(generate(m, padded, NEW, prompt_lengths=lengths, pad_id=0, prefill_chunk=chunk),
                  f"{route} chunk {chunk}")
    # the static route with a chunked prefill (equal lengths: no prompt_lengths)
    m.set_kv_cache(1, CACHE, **FORMATS[fmt])
    assert torch.equal(generate(m, rows[0][None], NEW, prefill_chunk=16)[0], singles[0])


# ------------------------------------------------------------------------------------------------
# trimming
# ------------------------------------------------------------------------------------------------
class _Watch:
    """``PageTable`` under watch: the most pages in use after any ``reserve``, and the ``trim`` calls."""

    def __init__(self, pages):
        self.pages, self.peak, self.trims = pages, 0, []
        reserve, trim = pages.reserve, pages.trim

        def watched_reserve(lengths):
            reserve(lengths)
            self.peak = max(self.peak, pages.pages_in_use)

        def watched_trim(first_live):
            self.trims.append(list(first_live))
            trim(first_live)

        pages.reserve, pages.trim = watched_reserve, watched_trim


def _trim_case(chunk):
    rows, padded, lengths = _prompts((100, 37) if chunk else LENGTHS, seed=3)
    new = 10 if chunk else NEW
    return rows, padded, lengths, new


@pytest.mark.parametrize("chunk", [None, 16], ids=["whole_prompt", "chunk16"])
def test_paged_generate_trims_and_fits_a_small_pool(chunk):
    """mistral-like (every layer windowed), page 16, a pool of B * 4 pages = 64 rows per sequence, fewer than the 110
    positions reached: generate finishes on the pages the window needs, with the static route's tokens, and never
    holds more than B * (ceil(W / 16) + 1) pages.  With prefill_chunk=16 a 100-token prompt goes through the same
    pool, its pages reserved chunk by chunk."""
    m = _model("mistral-like", dtype=F64)
    rows, padded, lengths, new = _trim_case(chunk)
    B = len(rows)
    singles = []
    for r in rows:
        m.set_kv_cache(1, CACHE)
        singles.append(generate(m, r[None], new)[0])
    m.set_kv_cache(B, CACHE, page_size=PAGE, num_pages=B * 4)
    assert m.kv_pages.rows == B * 64 and max(lengths) + new > 64
    watch = _Watch(m.kv_pages)
    out = generate(m, padded, new, prompt_lengths=lengths, pad_id=0, prefill_chunk=chunk)
    for b, (r, s) in enumerate(zip(rows, singles)):
        assert torch.equal(out[b, :len(r) + new], s), f"sequence {b} differs from its own static run"
    bound = B * (math.ceil(W / PAGE) + 1)
    print(f"peak pages in use {watch.peak} (bound {bound}), {len(watch.trims)} trims")
    assert 0 < watch.peak <= bound
    assert m.kv_pages.peak_pages_in_use == watch.peak
    assert watch.trims, "a model whose every layer is windowed trims"
    assert all(n >= 0 for t in watch.trims for n in t)
    # what is left: the pages of the last window, at the table indices they were given
    for b, n in enumerate(lengths.tolist()):
        last = n + new - 2  # the position of the last row that ran
        held = (m.kv_pages.table[b] >= 0).nonzero().flatten().tolist()
        assert held and held[0] == max(0, last - W + 1) // PAGE and held == list(range(held[0], held[-1] + 1))


def test_a_model_with_a_global_layer_never_trims():
    """gemma2-like on the same pool: its second layer attends everything, so no page can go and the pool runs out."""
    m = _model("gemma2-like", dtype=F64)
    rows, padded, lengths = _prompts(LENGTHS, seed=3)
    m.set_kv_cache(2, CACHE, page_size=PAGE, num_pages=2 * 4)
    watch = _Watch(m.kv_pages)
    with pytest.raises(RuntimeError, match="the pool is exhausted"):
        generate(m, padded, NEW, prompt_lengths=lengths, pad_id=0)
    assert watch.trims == []
    m.set_kv_cache(2, CACHE, page_size=PAGE)  # with the pool of a static cache it finishes, holding every page
    watch = _Watch(m.kv_pages)
    generate(m, padded, NEW, prompt_lengths=lengths, pad_id=0)
    assert watch.trims == [] and watch.peak == sum(math.ceil((n + NEW - 1) / PAGE) for n in LENGTHS)


# ------------------------------------------------------------------------------------------------
# PageTable.trim
# ------------------------------------------------------------------------------------------------
def _table(batch=2, max_pages=6, num_pages=9):
    pt = PageTable(batch, max_pages, PAGE, num_pages)
    pt.reserve([40, 20])  # pages 0 1 2 | 3 4
    assert pt.pages_of(0) == [0, 1, 2] and pt.pages_of(1) == [3, 4]
    return pt


def _consistent(pt):
    assert torch.equal(pt.table.cpu(), pt._host), "the device table equals the host table"
    held = [p for b in range(pt.batch_size) for p in pt.pages_of(b)]
    assert sorted(held) == sorted(set(held)) and not set(held) & set(pt._free), "no page is out twice"
    assert pt.pages_in_use == len(held) and len(held) + len(pt._free) == pt.num_pages
    assert sorted(int(p) for p in pt.table.flatten() if p >= 0) == sorted(held)


def test_trim_nothing_and_mid_page():
    pt = _table()
    addr = pt.table.data_ptr()
    pt.trim([0, 0])
    pt.trim([-5, 15])  # below the first page's end: the page stays
    assert pt.pages_of(0) == [0, 1, 2] and pt.pages_of(1) == [3, 4] and pt.pages_in_use == 5
    pt.trim([31, 16])  # position 31 is in page 1: only page 0 goes; 16 is the first position of page 1
    assert pt.pages_of(0) == [1, 2] and pt.pages_of(1) == [4] and pt.pages_in_use == 3
    assert pt.table.tolist() == [[-1, 1, 2, -1, -1, -1], [-1, 4, -1, -1, -1, -1]]
    assert pt.table.data_ptr() == addr, "updated in place"
    pt.trim([17, 3])  # never backwards
    assert pt.pages_of(0) == [1, 2] and pt.pages_of(1) == [4]
    _consistent(pt)
    with pytest.raises(ValueError):
        pt.trim([0])


def test_trim_all_then_reserve_and_release():
    pt = _table()
    pt.trim([10 ** 6, 32])
    assert pt.pages_of(0) == [] and pt.pages_of(1) == [] and pt.pages_in_use == 0
    assert (pt.table == -1).all()
    _consistent(pt)
    # a trimmed index is never filled again: the sequences go on at the indices past their old pages
    pt.reserve([60, 33])
    assert pt.table.tolist() == [[-1, -1, -1, 0, -1, -1], [-1, -1, 1, -1, -1, -1]]
    assert pt.pages_of(0) == [0] and pt.pages_of(1) == [1]
    pt.reserve([40, 20])  # shorter lengths take nothing away and give nothing back
    assert pt.pages_in_use == 2
    _consistent(pt)
    with pytest.raises(ValueError):
        pt.reserve([6 * PAGE + 1, 1])
    assert pt.pages_in_use == 2
    pt.release(0)
    assert pt.pages_of(0) == [] and pt.table[0].tolist() == [-1] * 6 and pt.pages_in_use == 1
    pt.reserve([17, 33])  # a released sequence starts from index 0 again
    assert pt.table[0].tolist() == [0, 2, -1, -1, -1, -1] and pt.pages_of(0) == [0, 2]
    _consistent(pt)
    pt.reset()
    assert pt.pages_in_use == 0 and (pt.table == -1).all() and pt.peak_pages_in_use == 0


def test_trimmed_pages_go_out_lowest_first():
    pt = _table(num_pages=6)
    pt.trim([32, 16])  # pages 0, 1 and 3 come back; 5 was never out
    assert sorted(pt._free) == [0, 1, 3, 5]
    pt.reserve([96, 48])  # sequence 0 takes three, then sequence 1 one
    assert pt.pages_of(0) == [2, 0, 1, 3] and pt.pages_of(1) == [4, 5]
    _consistent(pt)
    with pytest.raises(RuntimeError, match="the pool is exhausted"):
        pt.reserve([96, 49])
    _consistent(pt)
    assert pt.peak_pages_in_use == 6


def test_a_long_sequence_lives_on_a_window_of_pages():
    """200 positions through a table of 13 entries on a pool of 3 pages, one token at a time as generate does."""
    pt = PageTable(1, 13, PAGE, 3)
    for n in range(200):
        pt.trim([max(0, n - W + 1)])
        pt.reserve([n + 1])
        assert pt.pages_in_use <= 3
        first = max(0, n - W + 1) // PAGE
        assert (pt.table[0, :first] == -1).all() and (pt.table[0, first:n // PAGE + 1] >= 0).all()
    _consistent(pt)


# ------------------------------------------------------------------------------------------------
# hipex: the window masks into the *_win forms
# ------------------------------------------------------------------------------------------------
WINDOW_MASK = custom_op_symbol(opdef_of(kv_window_mask))
PAGED_WINDOW_MASK = custom_op_symbol(opdef_of(kv_paged_window_mask))
PASS_FORMATS = ["16bit", "e4m3", "e4m3_row"]


class _WithWindow:
    """A mask symbol that binds a trailing ``window``: the builders of the position / paged pass tests then spell the
    same programs over the window masks."""

    def __init__(self, sym, window):
        self.sym, self.window = sym, window

    def bind(self, *args, output, **kw):
        return self.sym.bind(*args, self.window, output=output, **kw)


def test_the_mask_symbols_are_the_ones_the_passes_match():
    assert WINDOW_MASK.id in hipex._KV_WINDOW_MASK_IDS and PAGED_WINDOW_MASK.id in hipex._KV_PAGED_WINDOW_MASK_IDS
    assert len(hipex._WINDOW_FORMS) == 12
    for op, win in hipex._WINDOW_FORMS.items():
        assert win.name == op.name + "_win" and getattr(hipex, win.name) is win


@pytest.mark.parametrize("fmt", PASS_FORMATS)
def test_decode_position_reads_take_the_window(fmt, monkeypatch):
    monkeypatch.setattr(pos_passes, "MASK", _WithWindow(WINDOW_MASK, 24))
    (lines, msg), names = pos_passes._read_program(fmt)
    op = {"16bit": "hip_decode_attn_pos_win", "e4m3": "hip_decode_attn_kv8_pos_win",
          "e4m3_row": "hip_decode_attn_kv8s_pos_win"}[fmt]
    assert lines == [f"o{n} = {op}(q{n}, {names[n]}, pos, 24, 0.125)" for n in range(2)], lines
    for case in ("mask_read_elsewhere", "mask_returned", "other_capacity", "causal"):
        (lines, _), _ = pos_passes._read_program(fmt, case)
        assert lines is None or (lines[0].startswith("mask = ") and "_win(" not in "".join(lines)), case


@pytest.mark.parametrize("fmt", PASS_FORMATS)
def test_decode_paged_reads_take_the_window(fmt, monkeypatch):
    monkeypatch.setattr(paged_passes, "MASK", _WithWindow(PAGED_WINDOW_MASK, 24))
    (lines, msg), names = paged_passes._read_program(fmt)
    op = paged_passes.PAGED_OP[fmt] + "_win"
    assert lines == [f"o{n} = {op}(q{n}, {names[n]}, pos, table, 16, 5, 24, 0.125)" for n in range(2)], lines
    (lines, _), names = paged_passes._read_program(fmt, "mask_returned")
    assert lines[0].startswith("mask = ") and "kv_paged_window_mask" in lines[0]
    assert lines[1:] == [f"o{n} = {op}(q{n}, {names[n]}, pos, table, 16, 5, 24, 0.125)" for n in range(2)]


@pytest.mark.parametrize("paged", [False, True], ids=["position_mask", "paged_mask"])
@pytest.mark.parametrize("fmt", PASS_FORMATS)
def test_prefill_reads_take_the_window(fmt, paged, monkeypatch):
    monkeypatch.setattr(prefill_passes, "POS_MASK", _WithWindow(WINDOW_MASK, 100))
    monkeypatch.setattr(prefill_passes, "PAGED_MASK", _WithWindow(PAGED_WINDOW_MASK, 100))
    (lines, msg), names = prefill_passes._program(fmt, paged)
    tail = "pos, table, 16, 20, 100, 0.125" if paged else "pos, 100, 0.125"
    op = f"{prefill_passes.OP[fmt]}_{'paged' if paged else 'pos'}_win"
    assert lines == [f"o{n} = {op}(q{n}, {names[n]}, {tail})" for n in range(2)], lines
    assert msg == prefill_passes._MSG
    for case in ("lse_read", "causal", "dropout", "d96"):  # the declined layer keeps the window mask
        (lines, _), names = prefill_passes._program(fmt, paged, case)
        assert "window_mask" in lines[0] and "\n".join(lines).count("_win(") == 1, case


@pytest.mark.parametrize("bad", [0, -1, 2.0, True])
def test_a_window_that_is_no_positive_int_is_left_alone(bad, monkeypatch):
    monkeypatch.setattr(pos_passes, "MASK", _WithWindow(WINDOW_MASK, bad))
    (lines, msg), _ = pos_passes._read_program("16bit")
    assert (lines, msg) == (None, None)


def _mixed_program(paged, prefill):
    """A step of a model with both kinds of layer: layer 0 under the window mask, layer 1 under the global one."""
    B, S, D = 3, 64, 64
    T = 40 if prefill else 1
    p = Program()
    pos, table = p.t("pos", B, T, dtype=torch.int64), p.t("table", B, 4, dtype=torch.int64)
    mask, wmask = p.ts("mask wmask", B, 1, T, S, dtype=torch.bool)
    if paged:
        p(paged_passes.MASK, pos, table, 16, 5, out=mask)
        p(PAGED_WINDOW_MASK, pos, table, 16, 5, 24, out=wmask)
    else:
        p(pos_passes.MASK, pos, S, out=mask)
        p(WINDOW_MASK, pos, S, 24, out=wmask)
    outs = []
    for layer, mk in enumerate((wmask, mask)):
        q, o = p.ts(f"q{layer} o{layer}", B, 8, T, D)
        if paged:
            kp, vp = p.ts(f"kp{layer} vp{layer}", 4, 16 * 5 + 1, D)
            k, v = p.ts(f"k{layer} v{layer}", B, 4, S, D)
            p(paged_passes.GATHER, kp, table, 16, out=k)
            p(paged_passes.GATHER, vp, table, 16, out=v)
        else:
            k, v = p.ts(f"kp{layer} vp{layer}", B, 4, S, D)
        if prefill:
            p(hipex.hip_attn_fwd_ex, q, k, v, mk, False, 0.125, 0.0, 0, 0,
              out=(o, p.t(f"lse{layer}", B, 8, T, dtype=torch.float32)))
        else:
            p(hipex.hip_decode_attn, q, k, v, mk, False, 0.125, out=o)
        outs.append(o)
    return p.run(*outs)


@pytest.mark.parametrize("prefill", [False, True], ids=["decode", "prefill"])
@pytest.mark.parametrize("paged", [False, True], ids=["static", "paged"])
def test_a_step_with_both_kinds_of_layer(paged, prefill, monkeypatch):
    kind = "prefill" if prefill else "decode"
    sel = "pos, table, 16, 5" if paged else "pos"
    form = "paged" if paged else "pos"
    lines, _ = _mixed_program(paged, prefill)
    assert lines == [f"o0 = hip_{kind}_attn_{form}_win(q0, kp0, vp0, {sel}, 24, 0.125)",
                     f"o1 = hip_{kind}_attn_{form}(q1, kp1, vp1, {sel}, 0.125)"], lines
    # the switch: the window layer keeps its mask and the masked kernel, the global layer is fused as ever
    monkeypatch.setenv("LTA_KV_WINDOW_FUSION", "0")
    lines, _ = _mixed_program(paged, prefill)
    text = "\n".join(lines)
    assert "_win(" not in text and f"o1 = hip_{kind}_attn_{form}(q1, kp1, vp1, {sel}, 0.125)" in lines
    assert sum("window_mask" in ln for ln in lines) == 1 and not any(ln.startswith("mask = ") for ln in lines)
    (o0,) = [ln for ln in lines if ln.startswith("o0")]
    assert ("hip_flash_attn_fwd_ex(q0, " if prefill else "hip_decode_attn(q0, ") in o0 and "wmask" in o0


@pytest.mark.parametrize("fmt", PASS_FORMATS)
def test_the_switch_keeps_window_masks_and_masked_kernels(fmt, monkeypatch):
    monkeypatch.setenv("LTA_KV_WINDOW_FUSION", "0")
    monkeypatch.setattr(pos_passes, "MASK", _WithWindow(WINDOW_MASK, 24))
    monkeypatch.setattr(paged_passes, "MASK", _WithWindow(PAGED_WINDOW_MASK, 24))
    monkeypatch.setattr(prefill_passes, "POS_MASK", _WithWindow(WINDOW_MASK, 24))
    monkeypatch.setattr(prefill_passes, "PAGED_MASK", _WithWindow(PAGED_WINDOW_MASK, 24))
    for lines in (pos_passes._read_program(fmt)[0][0], paged_passes._read_program(fmt)[0][0],
                  prefill_passes._program(fmt, False)[0][0], prefill_passes._program(fmt, True)[0][0]):
        if lines is None:
            continue  # nothing to rewrite at all
        text = "\n".join(lines)
        assert "_win(" not in text and "_pos(" not in text and "_paged(" not in text
        assert lines[0].startswith("mask = ") and "window_mask" in lines[0]


@pytest.mark.parametrize("fmt", PASS_FORMATS)
def test_programs_without_a_window_are_rewritten_as_before(fmt, monkeypatch):
    """The same final lines with the window switch either way: the programs of the earlier pass tests."""
    def all_lines():
        return [pos_passes._read_program(fmt)[0], paged_passes._read_program(fmt)[0],
                prefill_passes._program(fmt, False)[0], prefill_passes._program(fmt, True)[0]]

    on = all_lines()
    assert all("_win" not in ln and "window" not in ln for lines, _ in on for ln in lines)
    assert on[0][0] == [f"o{n} = {['hip_decode_attn_pos', 'hip_decode_attn_kv8_pos', 'hip_decode_attn_kv8s_pos'][PASS_FORMATS.index(fmt)]}"
                        f"(q{n}, {pos_passes._read_program(fmt)[1][n]}, pos, 0.125)" for n in range(2)]
    monkeypatch.setenv("LTA_KV_WINDOW_FUSION", "0")
    assert all_lines() == on


def test_benchmark_tools_take_sliding_window(capsys):
    """``--sliding-window N`` exists in both tools and is checked before anything touches a device."""
    from lightning_thunder_amd.benchmarks import generate as bg, inference as bi

    for mod in (bg, bi):
        with pytest.raises(SystemExit):
            mod.main(["--sliding-window", "0"])
        assert "--sliding-window must be >= 1" in capsys.readouterr().err
