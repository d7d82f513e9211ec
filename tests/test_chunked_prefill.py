"""Chunked prefill, ``generate(..., prefill_chunk=N)``: the prompt runs in slices of at most N columns at 2-D positions,
on the plain, ragged and paged routes, and returns the tokens of the whole-prompt prefill (CPU, fp64).  On the GPU the
compiled prefill by positions reads the cache through ``hip_prefill_attn_*`` (csrc/prefill_attention.hip) and gives
the logits and cache contents of the same program under ``LTA_KV_PREFILL_FUSION=0`` bit for bit."""
import pytest
import torch

import lightning_thunder_amd as thunder
from lightning_thunder_amd.models.litgpt import generate
from test_ragged_generate import FORMATS, _gpu_models, _model, _prompts

T, CACHE, NEW, PAGE = 21, 64, 6, 16
# len_b - 1 = 2, 11, 20, 7: at chunk 5 in the first, a middle and the last slice; at chunk 16 in the first and the last
LENGTHS = (3, 12, 21, 8)
CHUNKS = [1, 5, 16, T, T + 3]


def _full_prompt():
    _, padded, _ = _prompts(LENGTHS, seed=4)
    return torch.where(padded == 0, torch.full_like(padded, 7), padded)  # every row a full prompt


class _Counting:
    """``forward`` that records the shape and positions of every call."""

    def __init__(self, model):
        self.model, self.calls = model, []

    def __call__(self, idx, pos):
        self.calls.append((tuple(idx.shape), pos.clone()))
        return self.model(idx, pos)


def _check_chunk_calls(calls, chunk, B):
    """The prefill calls: slices of at most ``chunk`` columns at contiguous int64 [B, c1 - c0] positions arange(c0, c1)."""
    edges = list(range(0, T, chunk)) + [T]
    pre = calls[:len(edges) - 1]
    for (shape, pos), c0, c1 in zip(pre, edges, edges[1:]):
        assert shape == (B, c1 - c0) and pos.shape == (B, c1 - c0) and pos.dtype == torch.int64
        assert torch.equal(pos, torch.arange(c0, c1).expand(B, c1 - c0))
    assert all(shape == (B, 1) for shape, _ in calls[len(pre):]), "the decode loop is unchanged"
    assert len(calls) == len(pre) + NEW - 1


@pytest.mark.parametrize("chunk", CHUNKS)
def test_chunked_prefill_plain_route(chunk):
    m = _model("llama3-like", dtype=torch.float64)
    prompt = _full_prompt()
    m.set_kv_cache(len(LENGTHS), CACHE)
    ref = generate(m, prompt, NEW)
    m.set_kv_cache(len(LENGTHS), CACHE)
    fwd = _Counting(m)
    out = generate(m, prompt, NEW, forward=fwd, prefill_chunk=chunk)
    assert torch.equal(out, ref)
    _check_chunk_calls(fwd.calls, chunk, len(LENGTHS))


@pytest.mark.parametrize("chunk", CHUNKS)
def test_chunked_prefill_ragged_route(chunk):
    m = _model("llama3-like", dtype=torch.float64)
    _, padded, lengths = _prompts(LENGTHS, seed=4)
    assert padded.shape[1] == T
    m.set_kv_cache(len(LENGTHS), CACHE)
    ref = generate(m, padded, NEW, prompt_lengths=lengths, pad_id=0)
    m.set_kv_cache(len(LENGTHS), CACHE)
    fwd = _Counting(m)
    out = generate(m, padded, NEW, prompt_lengths=lengths, pad_id=0, forward=fwd, prefill_chunk=chunk)
    assert torch.equal(out, ref)
    _check_chunk_calls(fwd.calls, chunk, len(LENGTHS))


@pytest.mark.parametrize("fmt", list(FORMATS))
@pytest.mark.parametrize("chunk", CHUNKS)
def test_chunked_prefill_paged_route(chunk, fmt):
    m = _model("llama3-like", dtype=torch.float64)
    _, padded, lengths = _prompts(LENGTHS, seed=4)
    m.set_kv_cache(len(LENGTHS), CACHE, page_size=PAGE, **FORMATS[fmt])
    ref = generate(m, padded, NEW, prompt_lengths=lengths, pad_id=0)
    in_use, tables = m.kv_pages.pages_in_use, m.kv_pages.table.clone()
    m.set_kv_cache(len(LENGTHS), CACHE, page_size=PAGE, **FORMATS[fmt])
    fwd = _Counting(m)
    out = generate(m, padded, NEW, prompt_lengths=lengths, pad_id=0, forward=fwd, prefill_chunk=chunk)
    assert torch.equal(out, ref)
    assert m.kv_pages.pages_in_use == in_use and torch.equal(m.kv_pages.table, tables)
    _check_chunk_calls(fwd.calls, chunk, len(LENGTHS))


def test_chunked_prefill_keeps_one_row_of_logits_per_sequence():
    """The first token of row b comes from the chunk that holds column len_b - 1; no chunk's logits are kept."""
    from lightning_thunder_amd.models.litgpt import _chunked_prefill

    m = _model("llama3-like", dtype=torch.float64)
    _, padded, lengths = _prompts(LENGTHS, seed=4)
    m.set_kv_cache(len(LENGTHS), CACHE)
    whole = m(padded, torch.arange(T).expand(len(LENGTHS), T).contiguous())
    want = whole[torch.arange(len(LENGTHS)), lengths - 1]
    for chunk in (5, 16):
        m.set_kv_cache(len(LENGTHS), CACHE)
        last = _chunked_prefill(m, padded, chunk, lengths)
        assert last.shape == want.shape
        torch.testing.assert_close(last, want, rtol=1e-9, atol=1e-9)
    m.set_kv_cache(len(LENGTHS), CACHE)
    torch.testing.assert_close(_chunked_prefill(m, padded, 5), whole[:, -1], rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize("bad", [0, -3, 2.0, "4", True])
def test_prefill_chunk_must_be_a_positive_int(bad):
    m = _model("llama3-like")
    m.set_kv_cache(len(LENGTHS), CACHE)
    with pytest.raises(ValueError, match="prefill_chunk"):
        generate(m, _full_prompt(), NEW, prefill_chunk=bad)
    _, padded, lengths = _prompts(LENGTHS, seed=4)
    with pytest.raises(ValueError, match="prefill_chunk"):
        generate(m, padded, NEW, prompt_lengths=lengths, prefill_chunk=bad)


def test_benchmark_tools_take_prefill_chunk(capsys):
    """``--prefill-chunk N`` exists in both tools and is checked before anything touches a device."""
    from lightning_thunder_amd.benchmarks import generate as bg, inference as bi

    for mod in (bg, bi):
        with pytest.raises(SystemExit):
            mod.main(["--prefill-chunk", "0"])
        assert "--prefill-chunk must be >= 1" in capsys.readouterr().err


# ------------------------------------------------------------------------------------------------
# the compiled prefill by positions on the GPU (the 2-layer head-size-64 model of test_ragged_generate.py)
# ------------------------------------------------------------------------------------------------
GPU_B, GPU_T = 2, 40
PREFILL_OP = {(False, "16bit"): "hip_prefill_attn_pos", (False, "e4m3"): "hip_prefill_attn_kv8_pos",
              (False, "e4m3_row"): "hip_prefill_attn_kv8s_pos", (True, "16bit"): "hip_prefill_attn_paged",
              (True, "e4m3"): "hip_prefill_attn_kv8_paged", (True, "e4m3_row"): "hip_prefill_attn_kv8s_paged"}


def _compiled_prefill(mb, seq, fmt, paged):
    """One compiled forward of [B, 40] tokens at 2-D positions over a fresh cache: (logits, every cache buffer, the
    names of the final trace)."""
    kw = dict(page_size=PAGE) if paged else {}
    mb.set_kv_cache(GPU_B, CACHE, device=torch.device("cuda"), **kw, **FORMATS[fmt])
    if paged:
        mb.kv_pages.reserve([GPU_T] * GPU_B)
    jm = thunder.jit(mb)
    pos = torch.arange(GPU_T, device="cuda").expand(GPU_B, GPU_T).contiguous()
    logits = jm(seq, pos).clone()
    buffers = [b.clone() for block in mb.transformer.h for b in block.attn.kv_cache.buffers()]
    names = [b.sym.name for b in thunder.last_traces(jm)[-1].bound_symbols]
    return logits, buffers, names


@pytest.mark.gpu
@pytest.mark.parametrize("paged", [False, True], ids=["static", "paged"])
@pytest.mark.parametrize("fmt", list(FORMATS))
def test_compiled_prefill_by_positions_equals_the_unfused_program_gpu(fmt, paged, monkeypatch):
    _, mb = _gpu_models()
    seq = torch.randint(0, 300, (GPU_B, GPU_T), device="cuda")
    logits, buffers, names = _compiled_prefill(mb, seq, fmt, paged)
    assert names.count(PREFILL_OP[paged, fmt]) == 2, names
    gone = ("kv_paged_gather", "kv8_dequantise_rows", "kv_position_mask", "kv_paged_mask", "hip_flash_attn_fwd_ex")
    assert not any(g in n for n in names for g in gone), names
    monkeypatch.setenv("LTA_KV_PREFILL_FUSION", "0")
    ref_logits, ref_buffers, ref_names = _compiled_prefill(mb, seq, fmt, paged)
    assert not any("hip_prefill_attn" in n for n in ref_names) and ref_names.count("hip_flash_attn_fwd_ex") == 2
    assert any("kv_paged_mask" in n if paged else "kv_position_mask" in n for n in ref_names)
    assert torch.isfinite(logits).all()
    assert torch.equal(logits, ref_logits), f"{(logits != ref_logits).sum().item()} logits differ from the unfused program"
    assert len(buffers) == len(ref_buffers) == 2 * (4 if fmt == "e4m3_row" else 2)
    for got, want in zip(buffers, ref_buffers):
        assert torch.equal(got, want), "a cache buffer differs from the unfused program's"


@pytest.mark.gpu
def test_compiled_chunked_generate_equals_the_unfused_program_gpu(monkeypatch):
    """``generate(prefill_chunk=24)`` over a 40-token ragged prompt, compiled: chunks of 24 and 16 columns (the second
    at positions 24 .. 39 against the first one's keys), then the decode loop."""
    _, mb = _gpu_models()
    lengths = torch.tensor([40, 17, 29], device="cuda")
    seq = torch.randint(1, 300, (3, GPU_T), device="cuda")

    def run():
        mb.set_kv_cache(3, CACHE, device=torch.device("cuda"))
        jm = thunder.jit(mb)
        out = generate(mb, seq, 8, forward=jm, prompt_lengths=lengths, pad_id=0, prefill_chunk=24)
        return out, jm

    out, jm = run()
    assert out.shape == (3, GPU_T + 8)
    assert thunder.cache_misses(jm) == 3, "two prefill programs (24 and 16 columns) and the decode step"
    monkeypatch.setenv("LTA_KV_PREFILL_FUSION", "0")
    ref, _ = run()
    assert torch.equal(out, ref)
