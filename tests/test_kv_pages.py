"""The paged KV cache (``ops/kv_pages.py``): its definitions against per-element loops, the page allocator, and paged
``generate`` against the static ragged one, eager and compiled, for the three cache formats; then the compiled paged
decode step on the GPU."""
import pytest
import torch

import lightning_thunder_amd as thunder
from lightning_thunder_amd.models.litgpt import GPT, PagedKVCache, generate
from lightning_thunder_amd.ops.kv_pages import (PageTable, gather_pages, kv_page_slots, kv_paged_gather, kv_paged_mask,
                                                page_slots, paged_mask, write_slots)
from test_ragged_generate import CACHE, FORMATS, GPU_LENGTHS, LENGTHS, NEW, _gpu_models, _model, _prompts

PAGE = 16


# ------------------------------------------------------------------------------------------------
# the definitions
# ------------------------------------------------------------------------------------------------
def _table_case():
    """page 16, 3 table entries per sequence (S = 48), 5 pages (R = 80): an unallocated page, an entry past the pool."""
    table = torch.tensor([[3, 0, -1], [4, 5, 1], [-1, 2, -1]])
    pos = torch.tensor([[-1, 0, 15, 16, 17], [31, 32, 47, 48, 20], [0, 16, 31, 32, 100]])
    return table, pos, 16, 5


def test_page_slots_against_a_loop():
    table, pos, page, num_pages = _table_case()
    R, S = num_pages * page, table.shape[1] * page
    got = page_slots(table, pos, page, R)
    assert got.dtype == torch.int64 and got.shape == pos.shape
    for b in range(pos.shape[0]):
        for t in range(pos.shape[1]):
            p = int(pos[b, t])
            want = R
            if 0 <= p < S and 0 <= int(table[b, p // page]) < num_pages:
                want = int(table[b, p // page]) * page + p % page
            assert int(got[b, t]) == want, (b, t, p)
    assert got.tolist()[0] == [R, 48, 63, 0, 1] and got.tolist()[1][4] == R  # entry 5 is no page of a 5-page pool
    assert int(got[2, 0]) == R and int(got[2, 4]) == R  # an unallocated page; a position past S
    assert torch.equal(kv_page_slots(table, pos, page, R), got)


def test_gather_pages_and_paged_mask_against_a_loop():
    table, pos, page, num_pages = _table_case()
    R, S, H, D = num_pages * page, table.shape[1] * page, 2, 4
    pool = torch.arange(H * (R + 1) * D, dtype=torch.float32).view(H, R + 1, D)
    got = gather_pages(pool, table, page)
    assert got.shape == (3, H, S, D)
    mask = paged_mask(pos, table, page, num_pages)
    assert mask.shape == (3, 1, pos.shape[1], S) and mask.dtype == torch.bool
    for b in range(3):
        for j in range(S):
            pid = int(table[b, j // page])
            ok = 0 <= pid < num_pages
            for t in range(pos.shape[1]):
                assert bool(mask[b, 0, t, j]) == (j <= int(pos[b, t]) and ok), (b, t, j)
            if ok:
                assert torch.equal(got[b, :, j], pool[:, pid * page + j % page])
            elif pid < 0:
                assert torch.equal(got[b, :, j], pool[:, j % page]), "an entry < 0 reads page 0"
    assert not mask[:, :, 0].any() or not mask[0, 0, 0].any(), "position -1 sees nothing"
    assert not mask[0, 0, 0].any() and not mask[2].any(dim=-1)[0, 0]
    assert torch.equal(kv_paged_gather(pool, table, page), got)
    assert torch.equal(kv_paged_mask(pos, table, page, num_pages), mask)
    # without a page count only "no page" is hidden
    loose = paged_mask(pos, table, page)
    assert bool(loose[1, 0, 0, 16]) and not bool(mask[1, 0, 0, 16])


def test_write_slots_and_the_sink_row():
    table, pos, page, num_pages = _table_case()
    R, H, D = num_pages * page, 2, 4
    B, T = pos.shape
    slots = page_slots(table, pos, page, R)
    src = torch.arange(B * H * T * D, dtype=torch.float32).view(B, H, T, D) + 1
    pool = torch.zeros(H, R + 1, D)
    out = write_slots(pool, slots, src)
    assert out.data_ptr() == pool.data_ptr()
    exp = torch.zeros(H, R, D)
    for b in range(B):
        for t in range(T):
            if int(slots[b, t]) != R:
                exp[:, int(slots[b, t])] = src[b, :, t]
    assert torch.equal(pool[:, :R], exp), "every token with a page lands on its slot, nothing else is written"
    assert (slots == R).sum() > 1 and pool[:, R].ne(0).any(), "tokens without a page fall to the sink"


# ------------------------------------------------------------------------------------------------
# the allocator
# ------------------------------------------------------------------------------------------------
def test_page_table_allocates_lowest_first_and_never_moves_a_page():
    pt = PageTable(3, 4, 16, 8)
    ptr = pt.table.data_ptr()
    assert pt.table.dtype == torch.int64 and pt.table.shape == (3, 4) and (pt.table == -1).all()
    assert (pt.rows, pt.capacity, pt.pages_in_use) == (128, 64, 0)
    pt.reserve([16, 1, 17])
    assert pt.table.tolist() == [[0, -1, -1, -1], [1, -1, -1, -1], [2, 3, -1, -1]]
    pt.reserve([17, 1, 17])  # interleaved growth: sequence 0's second page comes after sequence 2's
    pt.reserve([17, 33, 10])  # sequence 2 keeps what it has
    assert pt.table.tolist() == [[0, 4, -1, -1], [1, 5, 6, -1], [2, 3, -1, -1]], "a non-identity table"
    assert pt.pages_in_use == 7
    held = [p for row in pt.table.tolist() for p in row if p >= 0]
    assert len(held) == len(set(held)), "no page is handed out twice"
    with pytest.raises(RuntimeError, match=r"2 more page\(s\) needed, 1 of 8 free"):
        pt.reserve([49, 33, 10])
    assert pt.pages_in_use == 7 and pt.table.tolist()[0] == [0, 4, -1, -1], "a refused reserve changes nothing"
    with pytest.raises(ValueError, match="holds 4 per sequence"):
        pt.reserve([65, 1, 1])
    with pytest.raises(ValueError):
        pt.reserve([1, 1])
    pt.release(1)
    assert pt.table.tolist()[1] == [-1] * 4 and pt.pages_in_use == 4 and pt.pages_of(1) == []
    pt.reserve([17, 0, 64])  # the freed pages go out again, lowest first
    assert pt.table.tolist() == [[0, 4, -1, -1], [-1, -1, -1, -1], [2, 3, 1, 5]]
    assert pt.pages_in_use == 6 and pt.table.data_ptr() == ptr, "the device table never moves"
    pt.reset()
    assert pt.pages_in_use == 0 and (pt.table == -1).all() and pt.table.data_ptr() == ptr
    for bad in (24, 8, 0, 16.0):
        with pytest.raises(ValueError):
            PageTable(1, 1, bad, 1)


def test_set_kv_cache_builds_pools_and_the_allocator():
    m = _model("llama3-like")
    c = m.config
    m.set_kv_cache(3, 40, page_size=16)
    assert m.max_seq_length == 48 and m.kv_pages.max_pages == 3 and m.kv_pages.num_pages == 9
    assert m.page_table is m.kv_pages.table
    for block in m.transformer.h:
        cache = block.attn.kv_cache
        assert isinstance(cache, PagedKVCache) and cache.k.shape == (c.n_query_groups, 9 * 16 + 1, c.head_size)
    m.set_kv_cache(3, 40, page_size=16, num_pages=4, dtype=torch.float8_e4m3fn, scale="row")
    cache = m.transformer.h[0].attn.kv_cache
    assert cache.k.dtype == torch.uint8 and cache.k.shape[1] == 65
    assert cache.k_scale.shape == (c.n_query_groups, 65, 1) and (cache.v_scale == 127).all()
    for bad in (24, 8):
        with pytest.raises(ValueError, match="power of two"):
            m.set_kv_cache(3, 40, page_size=bad)
    with pytest.raises(ValueError):
        m.set_kv_cache(3, 40, num_pages=4)
    with pytest.raises(TypeError, match="2-D input_pos"):
        m(torch.zeros(3, 2, dtype=torch.int64), torch.arange(2))
    m.set_kv_cache(3, 40)  # back to the static cache
    assert m.kv_pages is None and m.page_table is None and m.max_seq_length == 40
    assert m.transformer.h[0].attn.kv_cache.k.shape == (3, c.n_query_groups, 40, c.head_size)


# ------------------------------------------------------------------------------------------------
# generation: the paged cache against the static ragged one, token for token (fp64)
# ------------------------------------------------------------------------------------------------
def _pages_needed(lengths, new):
    """Pages of a run that feeds ``new - 1`` generated tokens back: positions 0 .. len + new - 2."""
    return sum(-(-(n + new - 1) // PAGE) for n in lengths)


@pytest.mark.parametrize("fmt", list(FORMATS))
@pytest.mark.parametrize("name", ["llama2-like", "llama3-like"])
def test_paged_generate_equals_the_static_ragged_generate(name, fmt):
    m = _model(name, dtype=torch.float64)
    rows, padded, lengths = _prompts()
    m.set_kv_cache(len(rows), CACHE, **FORMATS[fmt])
    ref = generate(m, padded, NEW, prompt_lengths=lengths, pad_id=0)
    need = _pages_needed(LENGTHS, NEW)
    assert need == 6 and max(LENGTHS) + NEW - 1 > PAGE, "generation crosses a page boundary"
    m.set_kv_cache(len(rows), CACHE, page_size=PAGE, num_pages=need, **FORMATS[fmt])
    out = generate(m, padded, NEW, prompt_lengths=lengths, pad_id=0)
    assert torch.equal(out, ref)
    pt = m.kv_pages
    assert pt.pages_in_use == need
    assert [len(pt.pages_of(b)) for b in range(4)] == [1, 2, 1, 2], "sequences 1 and 3 crossed into a second page"
    assert pt.pages_of(1) == [1, 4] and pt.pages_of(3) == [3, 5], "grown in step order: a non-identity table"
    # one page fewer: the pool runs out mid-generation
    m.set_kv_cache(len(rows), CACHE, page_size=PAGE, num_pages=need - 1, **FORMATS[fmt])
    with pytest.raises(RuntimeError, match="exhausted"):
        generate(m, padded, NEW, prompt_lengths=lengths, pad_id=0)


def test_paged_generate_without_lengths_takes_the_ragged_route():
    m = _model("llama3-like", dtype=torch.float64)
    _, padded, _ = _prompts()
    full = torch.where(padded == 0, torch.full_like(padded, 7), padded)  # every row a full prompt
    m.set_kv_cache(4, CACHE)
    ref = generate(m, full, NEW)
    m.set_kv_cache(4, CACHE, page_size=PAGE)
    out = generate(m, full, NEW)
    assert torch.equal(out, ref) and m.kv_pages.pages_in_use == 8
    with pytest.raises(ValueError, match="32 positions"):
        generate(m, full, CACHE - full.shape[1] + 1)


def test_paged_generate_eos_stops_a_sequences_pages():
    """``test_ragged_generate_eos_pads_finished_sequences_and_checks_the_cache`` on a paged cache: sequence 1 ends at
    its 4th new token, position 12, and never gets the second page its free run takes at position 16."""
    m = _model("llama3-like", dtype=torch.float64)
    rows, padded, lengths = _prompts()
    m.set_kv_cache(len(rows), CACHE)
    free = generate(m, padded, NEW, prompt_lengths=lengths, pad_id=0)
    b0, n0 = 1, LENGTHS[1]
    eos = int(free[b0, n0 + 3])
    new = [free[b, n:n + NEW].tolist() for b, n in enumerate(LENGTHS)]
    assert eos not in new[b0][:3]
    pad = next(t for t in range(319, 0, -1) if t != eos and all(t not in r for r in new))
    m.set_kv_cache(len(rows), CACHE)
    ref = generate(m, padded, NEW, prompt_lengths=lengths, pad_id=pad, eos_id=eos)
    m.set_kv_cache(len(rows), CACHE, page_size=PAGE)
    out = generate(m, padded, NEW, prompt_lengths=lengths, pad_id=pad, eos_id=eos)
    assert torch.equal(out, ref)
    ends = [new[b].index(eos) + 1 if eos in new[b] else NEW for b in range(4)]
    assert ends[b0] == 4 and max(ends) > 4
    pt = m.kv_pages
    assert len(pt.pages_of(b0)) == 1, "a finished sequence gets no further page"
    want = sum(-(-(n + min(e, NEW - 1)) // PAGE) for n, e in zip(LENGTHS, ends))
    assert pt.pages_in_use == want == _pages_needed(LENGTHS, NEW) - 1


@pytest.mark.parametrize("fmt", list(FORMATS))
def test_compiled_paged_generate_matches_eager_and_writes_slots_in_place(fmt):
    m = _model("llama3-like")
    rows, padded, lengths = _prompts()
    m.set_kv_cache(len(rows), CACHE, page_size=PAGE, **FORMATS[fmt])
    ref = generate(m, padded, NEW, prompt_lengths=lengths)
    m.set_kv_cache(len(rows), CACHE, page_size=PAGE, **FORMATS[fmt])
    jm = thunder.jit(m)
    out = generate(m, padded, NEW, prompt_lengths=lengths, forward=jm)
    assert torch.equal(ref, out)
    assert thunder.cache_misses(jm) == 2  # prefill + one paged decode program
    assert thunder.cache_hits(jm) == NEW - 2
    tr = str(thunder.last_traces(jm)[-1])
    buffers = 2 * (4 if fmt == "e4m3_row" else 2)  # per layer: k, v (and their scale pools)
    assert tr.count("index_copy_inplace(") == buffers, "one in-place slot write per pool"
    assert tr.count("kv_paged_gather(") == buffers
    assert "copy_(" not in tr and "torch.index_copy(" not in tr and ".index_copy(" not in tr
    assert tr.count("kv_page_slots(") == 1 and tr.count("kv_paged_mask(") == 1, "slots and mask once per step"


# ------------------------------------------------------------------------------------------------
# the compiled paged decode step on the GPU (the 2-layer head-size-64 model of test_ragged_generate.py)
# ------------------------------------------------------------------------------------------------
ROPE_SLOTS = {"16bit": "hip_qkv_rope_cache_slots", "e4m3": "hip_qkv_rope_cache_slots", "e4m3_row": "hip_qkv_rope_cache_slots_s8"}
ATTN_PAGED = {"16bit": "hip_decode_attn_paged", "e4m3": "hip_decode_attn_kv8_paged", "e4m3_row": "hip_decode_attn_kv8s_paged"}
NEW_OPS = set(ROPE_SLOTS.values()) | set(ATTN_PAGED.values())


def _teacher_forced_paged(model, fwd, seq, fmt, steps=15):
    """``test_ragged_generate._teacher_forced_ragged`` on a paged cache of page size 16: lengths 8, 3, 5 and 15 steps,
    so sequence 0 crosses into its second page at step 8, the others at steps 13 and 11."""
    B, Tmax = len(GPU_LENGTHS), max(GPU_LENGTHS)
    lengths = torch.tensor(GPU_LENGTHS, device="cuda")
    model.set_kv_cache(B, 64, device=torch.device("cuda"), page_size=PAGE, **FORMATS[fmt])
    held = list(GPU_LENGTHS)
    model.kv_pages.reserve(held)
    logits = fwd(seq[:, :Tmax], torch.arange(Tmax, device="cuda").expand(B, Tmax).contiguous())
    outs = [logits[torch.arange(B, device="cuda"), lengths - 1].float().clone()]
    pos = lengths.clone().view(B, 1)
    for i in range(steps):
        held = [n + 1 for n in held]
        model.kv_pages.reserve(held)
        tok = seq.gather(1, pos)
        outs.append(fwd(tok, pos)[:, -1].float().clone())  # graph replays return a static buffer: copy out
        pos.add_(1)
    assert model.kv_pages.pages_in_use == 6 and model.kv_pages.pages_of(0) == [0, 3]
    return torch.stack(outs)


@pytest.mark.gpu
@pytest.mark.parametrize("graphs", [False, True])
@pytest.mark.parametrize("fmt", list(FORMATS))
def test_paged_decode_logits_teacher_forced_gpu(fmt, graphs):
    """``test_ragged_decode_logits_teacher_forced_gpu`` on a paged cache: the compiled bf16 model's logits are within
    3 * base + 1e-3 of fp32 eager at every step (base: bf16 eager's own error; that test's bound, for its reason),
    two runs are bitwise equal, and the decode step's program holds per layer one slot-writing RoPE and one paged
    decode attention, no gather, no mask, no slot write and no cache write-back."""
    m32, mb = _gpu_models()
    seq = torch.randint(0, 300, (len(GPU_LENGTHS), 24), device="cuda")
    transforms = []
    if graphs:
        from lightning_thunder_amd.transforms.hipgraph import HipGraphTransform

        transforms.append(HipGraphTransform())
    ref = _teacher_forced_paged(m32, m32, seq, fmt)
    eager = _teacher_forced_paged(mb, mb, seq, fmt)
    jm = thunder.jit(mb, transforms=transforms)
    got = _teacher_forced_paged(mb, jm, seq, fmt)
    got2 = _teacher_forced_paged(mb, jm, seq, fmt)
    assert torch.equal(got, got2)
    for i in range(ref.shape[0]):
        base = ((eager[i] - ref[i]).norm() / ref[i].norm()).item()
        err = ((got[i] - ref[i]).norm() / ref[i].norm()).item()
        print(f"[paged teacher forced {fmt} graphs={graphs}] step {i} err={err:.3e} base={base:.3e}")
        assert err <= 3 * base + 1e-3, (i, err, base)
    if not graphs:
        trace = thunder.last_traces(jm)[-1]  # the decode step's program
        names = [b.sym.name for b in trace.bound_symbols]
        assert names.count(ROPE_SLOTS[fmt]) == 2 and names.count(ATTN_PAGED[fmt]) == 2, names
        assert "index_copy_inplace" not in names and "index_copy" not in names and "copy_" not in names
        assert not any("kv_paged_gather" in n or "kv_paged_mask" in n for n in names), "gathers and mask are gone"
        assert not any(n in ("hip_decode_attn", "hip_decode_attn_kv8", "hip_decode_attn_kv8s") for n in names)
        assert "copy_(" not in str(trace)


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", list(FORMATS))
def test_paged_decode_unfused_switch_gpu(fmt, monkeypatch):
    """LTA_KV_PAGED_FUSION=0: none of the new operators; the slot writes, the gathers and the mask stay, and the same
    bound holds."""
    monkeypatch.setenv("LTA_KV_PAGED_FUSION", "0")
    m32, mb = _gpu_models()
    seq = torch.randint(0, 300, (len(GPU_LENGTHS), 24), device="cuda")
    ref = _teacher_forced_paged(m32, m32, seq, fmt)
    eager = _teacher_forced_paged(mb, mb, seq, fmt)
    jm = thunder.jit(mb)
    got = _teacher_forced_paged(mb, jm, seq, fmt)
    for i in range(ref.shape[0]):
        base = ((eager[i] - ref[i]).norm() / ref[i].norm()).item()
        err = ((got[i] - ref[i]).norm() / ref[i].norm()).item()
        print(f"[paged teacher forced {fmt} unfused] step {i} err={err:.3e} base={base:.3e}")
        assert err <= 3 * base + 1e-3, (i, err, base)
    names = [b.sym.name for b in thunder.last_traces(jm)[-1].bound_symbols]
    buffers = 2 * (4 if fmt == "e4m3_row" else 2)
    assert not NEW_OPS & set(names), names
    assert names.count("index_copy_inplace") == buffers and "copy_" not in names
    assert sum("kv_paged_gather" in n for n in names) == buffers and any("kv_paged_mask" in n for n in names)
