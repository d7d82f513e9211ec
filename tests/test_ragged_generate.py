"""Ragged batches: per-sequence positions from ``generate(..., prompt_lengths=...)`` down to the KV-cache write
and the attention mask (``GPT.forward`` with an int64 ``[B, T]`` ``input_pos``)."""
import pytest
import torch

import lightning_thunder_amd as thunder
from lightning_thunder_amd.models.litgpt import GPT, generate, init_weights

LENGTHS = (3, 9, 1, 6)
CACHE, NEW = 32, 12
FORMATS = {"16bit": dict(), "e4m3": dict(dtype=torch.float8_e4m3fn),
           "e4m3_row": dict(dtype=torch.float8_e4m3fn, scale="row")}


def _model(name="llama3-like", device="cpu", dtype=torch.float32, **kw):
    """The settings of ``tests/test_generate.py::_model``."""
    torch.manual_seed(0)
    m = GPT.from_name(name, **kw).to(device=device, dtype=dtype)
    init_weights(m, std=0.2)
    m.requires_grad_(False)
    return m


def _prompts(lengths=LENGTHS, seed=1, device="cpu"):
    g = torch.Generator().manual_seed(seed)
    rows = [torch.randint(1, 300, (n,), generator=g) for n in lengths]
    padded = torch.zeros(len(lengths), max(lengths), dtype=torch.int64)
    for b, r in enumerate(rows):
        padded[b, :len(r)] = r
    return [r.to(device) for r in rows], padded.to(device), torch.tensor(lengths, device=device)


def _single_runs(m, rows, new, min_gap=None):
    """``generate`` of each prompt alone; with ``min_gap`` (a list) the smallest top-2 logit gap of every greedy
    choice of those runs is appended to it."""
    outs = []
    for r in rows:
        m.set_kv_cache(1, CACHE)
        fwd = m
        if min_gap is not None:
            def fwd(idx, pos, _m=m):
                logits = _m(idx, pos)
                top = logits[:, -1].topk(2, dim=-1).values
                min_gap.append((top[:, 0] - top[:, 1]).min().item())
                return logits
        outs.append(generate(m, r[None], new, forward=fwd)[0])
    return outs


@pytest.mark.parametrize("name", ["llama2-like", "llama3-like"])
def test_ragged_generate_equals_each_prompt_alone(name):
    m = _model(name, dtype=torch.float64)
    rows, padded, lengths = _prompts()
    gaps = []
    singles = _single_runs(m, rows, NEW, gaps)
    assert min(gaps) > 1e-6, f"a greedy choice of the reference run is a near tie ({min(gaps):.3e})"
    print(f"[{name}] smallest top-2 logit gap of the single runs: {min(gaps):.3e}")
    m.set_kv_cache(len(rows), CACHE)
    out = generate(m, padded, NEW, prompt_lengths=lengths, pad_id=0)
    assert out.shape == (len(rows), padded.shape[1] + NEW)
    for b, (r, s) in enumerate(zip(rows, singles)):
        n = len(r)
        assert torch.equal(out[b, :n + NEW], s), f"sequence {b} (length {n}) differs from its own run"
        assert not out[b, n + NEW:].any(), "pad_id after the new tokens"


@pytest.mark.parametrize("fmt", list(FORMATS))
@pytest.mark.parametrize("T", [1, 3])
def test_forward_with_batched_positions_matches_per_sequence_forwards(T, fmt):
    """Logits of one [B, T] forward at positions start_b .. start_b + T - 1 against B batch-1 forwards at 1-D
    positions, each over a cache prefilled with the same tokens, for every cache format against itself."""
    m = _model("llama3-like")
    B, pre = 3, (4, 1, 7)
    g = torch.Generator().manual_seed(2)
    toks = torch.randint(0, 300, (B, max(pre) + T), generator=g)
    ref = []
    for b in range(B):
        m.set_kv_cache(1, CACHE, **FORMATS[fmt])
        m(toks[b:b + 1, :pre[b]], torch.arange(pre[b]))
        ref.append(m(toks[b:b + 1, pre[b]:pre[b] + T], torch.arange(pre[b], pre[b] + T)))
    m.set_kv_cache(B, CACHE, **FORMATS[fmt])
    # the padded prefill of generate(): rows beyond a sequence's length hold other tokens' K/V for now
    m(toks[:, :max(pre)], torch.arange(max(pre)))
    pos = torch.tensor(pre)[:, None] + torch.arange(T)[None, :]
    step = torch.stack([toks[b, pre[b]:pre[b] + T] for b in range(B)])
    got = m(step, pos)
    torch.testing.assert_close(got, torch.cat(ref), atol=1e-4, rtol=1e-4)


def test_position_mask_and_row_write_definitions():
    from lightning_thunder_amd.ops.kv_rows import kv_position_mask, position_mask, write_rows

    pos = torch.tensor([[0, 5], [7, 2]])
    mk = position_mask(pos, 8)
    assert mk.shape == (2, 1, 2, 8) and mk.dtype == torch.bool
    for b in range(2):
        for t in range(2):
            assert mk[b, 0, t].tolist() == [j <= int(pos[b, t]) for j in range(8)]
    assert torch.equal(kv_position_mask(pos, 8), mk)
    cache = torch.zeros(2, 3, 8, 4)
    src = torch.arange(2 * 3 * 2 * 4, dtype=torch.float32).view(2, 3, 2, 4) + 1
    out = write_rows(cache, pos, src)
    assert out.data_ptr() == cache.data_ptr()
    exp = torch.zeros(2, 3, 8, 4)
    for b in range(2):
        for t in range(2):
            exp[b, :, pos[b, t]] = src[b, :, t]
    assert torch.equal(cache, exp)


def test_ragged_generate_eos_pads_finished_sequences_and_checks_the_cache():
    m = _model("llama3-like", dtype=torch.float64)
    rows, padded, lengths = _prompts()
    m.set_kv_cache(len(rows), CACHE)
    free = generate(m, padded, NEW, prompt_lengths=lengths, pad_id=0)
    # the 4th new token of sequence 1 as eos: nobody produces it earlier
    b0, n0 = 1, LENGTHS[1]
    eos = int(free[b0, n0 + 3])
    new = [free[b, n:n + NEW].tolist() for b, n in enumerate(LENGTHS)]
    assert eos not in new[b0][:3], "the chosen eos token must first appear at step 3 of sequence 1"
    pad = next(t for t in range(319, 0, -1) if t != eos and all(t not in r for r in new))  # a token nobody produces
    m.set_kv_cache(len(rows), CACHE)
    out = generate(m, padded, NEW, prompt_lengths=lengths, pad_id=pad, eos_id=eos)
    ends = []
    for b, n in enumerate(LENGTHS):
        end = new[b].index(eos) + 1 if eos in new[b] else NEW
        ends.append(end)
        assert out[b, :n].tolist() == padded[b, :n].tolist()
        assert out[b, n:n + end].tolist() == new[b][:end], f"sequence {b} must be unaffected up to its own end"
    steps = max(ends)  # the loop ends when all are done
    for b, n in enumerate(LENGTHS):
        assert (out[b, n + ends[b]:n + steps] == pad).all(), f"sequence {b} is pad_id after its eos"
        assert (out[b, n + steps:] == pad).all() and (out[b, n:n + ends[b]] != pad).all()
    assert ends[b0] == 4 and max(ends) > 4, "one sequence ends early while another keeps running"
    # overflow: the longest prompt plus the new tokens must fit the cache
    m.set_kv_cache(len(rows), CACHE)
    generate(m, padded, CACHE - max(LENGTHS), prompt_lengths=lengths)
    with pytest.raises(ValueError):
        generate(m, padded, CACHE - max(LENGTHS) + 1, prompt_lengths=lengths)
    with pytest.raises(ValueError):
        generate(m, padded, 2, prompt_lengths=torch.tensor([3, 10, 1, 6]))
    with pytest.raises(ValueError):
        generate(m, padded, 2, prompt_lengths=torch.tensor([3, 9, 0, 6]))


@pytest.mark.parametrize("fmt", list(FORMATS))
def test_compiled_ragged_generate_matches_eager_and_writes_rows_in_place(fmt):
    m = _model("llama3-like")
    rows, padded, lengths = _prompts()
    m.set_kv_cache(len(rows), CACHE, **FORMATS[fmt])
    ref = generate(m, padded, NEW, prompt_lengths=lengths)
    m.set_kv_cache(len(rows), CACHE, **FORMATS[fmt])
    jm = thunder.jit(m)
    out = generate(m, padded, NEW, prompt_lengths=lengths, forward=jm)
    assert torch.equal(ref, out)
    assert thunder.cache_misses(jm) == 2  # prefill + one ragged decode program
    assert thunder.cache_hits(jm) == NEW - 2
    tr = str(thunder.last_traces(jm)[-1])
    buffers = 2 * (4 if fmt == "e4m3_row" else 2)  # per layer: k, v (and their scale caches)
    assert tr.count("scatter_rows_inplace(") == buffers, "one in-place row write per cache buffer"
    assert "copy_(" not in tr and "torch.scatter(" not in tr  # no whole-cache write-back, no functional scatter
    assert "kv_position_mask" in tr


# ------------------------------------------------------------------------------------------------
# the compiled ragged decode step on the GPU (2-layer llama3-like at head size 64, the decode kernels' head dim)
# ------------------------------------------------------------------------------------------------
GPU_LENGTHS = (8, 3, 5)
ROPE_ROWS = {"16bit": "hip_qkv_rope_cache_rows", "e4m3": "hip_qkv_rope_cache_rows", "e4m3_row": "hip_qkv_rope_cache_rows_s8"}
ATTN_POS = {"16bit": "hip_decode_attn_pos", "e4m3": "hip_decode_attn_kv8_pos", "e4m3_row": "hip_decode_attn_kv8s_pos"}
NEW_OPS = set(ROPE_ROWS.values()) | set(ATTN_POS.values())


def _gpu_models():
    kw = dict(n_layer=2, n_embd=256, n_head=4, n_query_groups=2, head_size=64, intermediate_size=384)
    m32 = _model("llama3-like", device="cuda", dtype=torch.float32, **kw)
    mb = _model("llama3-like", device="cuda", dtype=torch.float32, **kw).to(torch.bfloat16)
    mb.load_state_dict({k: v.to(torch.bfloat16) for k, v in m32.state_dict().items()})
    return m32, mb


def _teacher_forced_ragged(model, fwd, seq, fmt, steps=15):
    """Padded prefill of [B, 8] at the shared positions, then ``steps`` decode steps of [B, 1] tokens at per-sequence
    positions starting at the lengths; sequence b is fed ``seq[b, len_b + i]`` at step i (the same tokens for every
    model).  Returns the logits of every sequence's own last prompt token and of every step, [1 + steps, B, V]."""
    B, Tmax = len(GPU_LENGTHS), max(GPU_LENGTHS)
    lengths = torch.tensor(GPU_LENGTHS, device="cuda")
    model.set_kv_cache(B, 64, device=torch.device("cuda"), **FORMATS[fmt])
    logits = fwd(seq[:, :Tmax], torch.arange(Tmax, device="cuda"))
    outs = [logits[torch.arange(B, device="cuda"), lengths - 1].float().clone()]
    pos = lengths.clone().view(B, 1)
    for i in range(steps):
        tok = seq.gather(1, pos)
        outs.append(fwd(tok, pos)[:, -1].float().clone())  # graph replays return a static buffer: copy out
        pos.add_(1)
    return torch.stack(outs)


@pytest.mark.gpu
@pytest.mark.parametrize("graphs", [False, True])
@pytest.mark.parametrize("fmt", list(FORMATS))
def test_ragged_decode_logits_teacher_forced_gpu(fmt, graphs):
    """``test_decode_logits_teacher_forced_gpu`` for a ragged batch: the compiled bf16 model's logits are within
    3 * base + 1e-3 of fp32 eager at every step (base: bf16 eager's own error; that test's bound, for its reason),
    replays are bitwise equal, and the decode step's program holds per layer one per-row cache-writing RoPE and one
    position-mode decode attention, no row write, no mask and no cache write-back."""
    m32, mb = _gpu_models()
    seq = torch.randint(0, 300, (len(GPU_LENGTHS), 24), device="cuda")
    transforms = []
    if graphs:
        from lightning_thunder_amd.transforms.hipgraph import HipGraphTransform

        transforms.append(HipGraphTransform())
    ref = _teacher_forced_ragged(m32, m32, seq, fmt)
    eager = _teacher_forced_ragged(mb, mb, seq, fmt)
    jm = thunder.jit(mb, transforms=transforms)
    got = _teacher_forced_ragged(mb, jm, seq, fmt)
    got2 = _teacher_forced_ragged(mb, jm, seq, fmt)
    assert torch.equal(got, got2)
    for i in range(ref.shape[0]):
        base = ((eager[i] - ref[i]).norm() / ref[i].norm()).item()
        err = ((got[i] - ref[i]).norm() / ref[i].norm()).item()
        print(f"[ragged teacher forced {fmt} graphs={graphs}] step {i} err={err:.3e} base={base:.3e}")
        assert err <= 3 * base + 1e-3, (i, err, base)
    if not graphs:
        trace = thunder.last_traces(jm)[-1]  # the decode step's program
        names = [b.sym.name for b in trace.bound_symbols]
        assert names.count(ROPE_ROWS[fmt]) == 2 and names.count(ATTN_POS[fmt]) == 2, names
        assert "scatter_rows_inplace" not in names and "scatter" not in names and "copy_" not in names
        assert not any("kv_position_mask" in n for n in names), "the mask has no reader left"
        assert not any(n in ("hip_decode_attn", "hip_decode_attn_kv8", "hip_decode_attn_kv8s") for n in names)
        assert "copy_(" not in str(trace)


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", list(FORMATS))
def test_ragged_decode_unfused_switch_gpu(fmt, monkeypatch):
    """LTA_KV_POS_FUSION=0: none of the new operators, the mask and the row writes stay, and the same bound holds."""
    monkeypatch.setenv("LTA_KV_POS_FUSION", "0")
    m32, mb = _gpu_models()
    seq = torch.randint(0, 300, (len(GPU_LENGTHS), 24), device="cuda")
    ref = _teacher_forced_ragged(m32, m32, seq, fmt)
    eager = _teacher_forced_ragged(mb, mb, seq, fmt)
    jm = thunder.jit(mb)
    got = _teacher_forced_ragged(mb, jm, seq, fmt)
    for i in range(ref.shape[0]):
        base = ((eager[i] - ref[i]).norm() / ref[i].norm()).item()
        err = ((got[i] - ref[i]).norm() / ref[i].norm()).item()
        print(f"[ragged teacher forced {fmt} unfused] step {i} err={err:.3e} base={base:.3e}")
        assert err <= 3 * base + 1e-3, (i, err, base)
    names = [b.sym.name for b in thunder.last_traces(jm)[-1].bound_symbols]
    assert not NEW_OPS & set(names), names
    assert names.count("scatter_rows_inplace") == 2 * (4 if fmt == "e4m3_row" else 2)
    assert any("kv_position_mask" in n for n in names) and "copy_" not in names


@pytest.mark.gpu
def test_ragged_generate_gpu_bf16():
    """``generate(..., prompt_lengths=...)`` through the compiled model with hipGraph replays: the prompt and the
    first new tokens agree with bf16 eager (later greedy tokens may flip on bf16 near-ties), replays are equal."""
    from lightning_thunder_amd.transforms.hipgraph import HipGraphTransform

    _, mb = _gpu_models()
    rows, padded, lengths = _prompts(GPU_LENGTHS, device="cuda")
    mb.set_kv_cache(len(rows), 64, device=torch.device("cuda"))
    ref = generate(mb, padded, 16, prompt_lengths=lengths)
    mb.set_kv_cache(len(rows), 64, device=torch.device("cuda"))
    jm = thunder.jit(mb, transforms=[HipGraphTransform()])
    out = generate(mb, padded, 16, prompt_lengths=lengths, forward=jm)
    out2 = generate(mb, padded, 16, prompt_lengths=lengths, forward=jm)
    torch.cuda.synchronize()
    for b, n in enumerate(GPU_LENGTHS):
        assert torch.equal(out[b, :n + 4], ref[b, :n + 4])
    assert torch.equal(out, out2)
