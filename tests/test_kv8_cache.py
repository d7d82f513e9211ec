"""The unscaled e4m3 KV cache (``set_kv_cache(dtype=torch.float8_e4m3fn)``): the model's semantics on the
CPU, the two hipex rewrites on hand-built traces, and the compiled decode path on the GPU.

The cache holds ``k.clamp(-448, 448).to(float8_e4m3fn).view(uint8)`` (the same for v) in uint8 buffers and
is read back as ``view(float8_e4m3fn).to(k.dtype)``, which is exact.  On the GPU the write runs in the RoPE
kernel (``hip_qkv_rope_cache`` with uint8 caches) and the decode attention reads the bytes itself
(``hip_decode_attn_kv8``); ``LTA_KV8_FUSION=0`` keeps the program as the model spells it.
"""
import pytest
import torch

import lightning_thunder_amd as thunder
from lightning_thunder_amd import torch as lt
from lightning_thunder_amd.executors import hipex
from lightning_thunder_amd.models.litgpt import GPT, generate, init_weights
from lightning_thunder_amd.transforms.inplace_index_copy import index_copy_inplace

from test_hipex_passes import Program, unchanged

BF16, F16, U8, I64 = torch.bfloat16, torch.float16, torch.uint8, torch.int64
F8, F8_E5M2 = torch.float8_e4m3fn, torch.float8_e5m2
gpu = pytest.mark.gpu


def _model(name="llama3-like", device="cpu", dtype=torch.float32, **kw):
    torch.manual_seed(0)
    m = GPT.from_name(name, **kw).to(device=device, dtype=dtype)
    init_weights(m, std=0.2)
    m.requires_grad_(False)
    return m


def _bytes(t):
    return t.clamp(-448.0, 448.0).to(F8).view(U8)


# ------------------------------------------------------------------------------------------------
# 1. model semantics (eager)
# ------------------------------------------------------------------------------------------------
def test_fp8_cache_holds_the_quantised_keys_and_values():
    m = _model()
    p = torch.randint(0, 300, (1, 8))
    seen = []
    m.set_kv_cache(1, 64)
    hook = m.transformer.h[0].attn.kv_cache.register_forward_pre_hook(lambda mod, args: seen.append(args))
    m(p, torch.arange(8))
    hook.remove()
    (_, k, v), = seen
    assert k.shape == v.shape == (1, 2, 8, 16)

    m.set_kv_cache(1, 64, dtype=F8)
    for block in m.transformer.h:
        c = block.attn.kv_cache
        assert c.k.dtype == c.v.dtype == U8 and c.k.shape == c.v.shape == (1, 2, 64, 16)
        assert not c.k.any() and not c.v.any()
    m(p, torch.arange(8))
    c = m.transformer.h[0].attn.kv_cache
    assert torch.equal(c.k[:, :, :8], _bytes(k)) and torch.equal(c.v[:, :, :8], _bytes(v))
    assert c.k[:, :, :8].any() and c.v[:, :, :8].any()
    assert not c.k[:, :, 8:].any() and not c.v[:, :, 8:].any()

    m.set_kv_cache(1, 64, dtype=F8)
    out = generate(m, p, 12)
    assert out.shape == (1, 20) and torch.equal(out[:, :8], p)


def test_fp8_cache_saturates_where_the_cast_alone_gives_nan():
    from lightning_thunder_amd.models.litgpt import KVCache

    c = KVCache((1, 1, 4, 16), (1, 1, 4, 16), dtype=F8)
    k = torch.full((1, 1, 1, 16), 1e3)
    k[..., 1::2] = -1e3
    v = torch.full((1, 1, 1, 16), 1e-3)
    assert torch.isnan(k.to(F8).float()).all()
    k_all, v_all = c(torch.tensor([2]), k, v)
    assert k_all.dtype == v_all.dtype == torch.float32
    assert torch.equal(k_all[0, 0, 2], k[0, 0, 0].clamp(-448, 448)) and not k_all[0, 0, [0, 1, 3]].any()
    assert set(c.k[0, 0, 2].tolist()) == {0x7E, 0xFE}
    assert torch.equal(v_all[0, 0, 2], v[0, 0, 0].to(F8).float())


@pytest.mark.parametrize("dtype", [F8_E5M2, torch.float8_e4m3fnuz])
def test_other_8bit_float_caches_are_refused(dtype):
    m = _model()
    with pytest.raises(ValueError, match="float8_e4m3fn"):
        m.set_kv_cache(1, 64, dtype=dtype)


def test_other_cache_dtypes_are_as_before():
    m = _model()
    m.set_kv_cache(1, 32, dtype=torch.float64)
    c = m.transformer.h[0].attn.kv_cache
    assert c.k.dtype == torch.float64
    k = torch.randn(1, 2, 1, 16)
    k_all, _ = c(torch.tensor([5]), k, k)
    assert k_all.dtype == torch.float64 and torch.equal(k_all[:, :, 5:6], k.double())


# ------------------------------------------------------------------------------------------------
# 2. the jitted program
# ------------------------------------------------------------------------------------------------
def test_fp8_cache_generate_matches_eager_and_reuses_programs():
    m = _model()
    p = torch.randint(0, 300, (1, 8))
    m.set_kv_cache(1, 64, dtype=F8)
    ref = generate(m, p, 12)
    m.set_kv_cache(1, 64, dtype=F8)
    jm = thunder.jit(m)
    out = generate(m, p, 12, forward=jm)
    assert torch.equal(ref, out)
    assert thunder.cache_misses(jm) == 2  # prefill + decode
    assert thunder.cache_hits(jm) == 10
    trace = thunder.last_traces(jm)[-1]
    tr = str(trace)
    assert "index_copy_inplace" in tr and "copy_(" not in tr
    writes = [b for b in trace.bound_symbols if b.sym.name == "index_copy_inplace"]
    assert len(writes) == 2 * len(m.transformer.h) and all(b.args[0].dtype == U8 and b.output.dtype == U8 for b in writes)


# ------------------------------------------------------------------------------------------------
# 3. the rewrites on hand-built traces
# ------------------------------------------------------------------------------------------------
_ROPE_CACHE = "q, kc2, vc2 = hip_qkv_rope_cache(qkv, cos, sin, 4, 4, 64, 64, kc, vc, pos)"
_KV = "hipex: 1 KV-cache write pair(s) fused into RoPE"
_READ = "hipex: 1 decode attention(s) read their e4m3 KV cache directly"


def _quantise(p, t, tag, lo=-448.0, hi=448.0, f8=F8, clamp=True):
    """``t -> clamp -> to(f8) -> view(uint8)``; returns the three values."""
    c, f, u = p.t(tag + "_c", 1, 4, 1, 64), p.t(tag + "_f", 1, 4, 1, 64, dtype=f8), p.t(tag + "_u", 1, 4, 1, 64, dtype=U8)
    if clamp:
        p(lt.clamp, t, lo, hi, out=c)
    p(lt.to, c if clamp else t, f8, out=f)
    p(lt.view, f, U8, out=u)
    return c, f, u


def _write_program(case=None):
    p = Program()
    pos, pos2 = p.ts("pos pos2", 1, dtype=I64)
    qkv, cos, sin = p.t("qkv", 1, 1, 3 * 4 * 64), p.t("cos", 1, 64), p.t("sin", 1, 64)
    q, k, v = p.ts("q k v", 1, 4, 1, 64)
    cache_dtype = BF16 if case == "bf16_cache" else U8
    kc, vc, kc2, vc2 = p.ts("kc vc kc2 vc2", 1, 4, 32, 64, dtype=cache_dtype)
    p(hipex.hip_qkv_rope, qkv, cos, sin, 4, 4, 64, 64, out=(q, k, v))
    kw = {"bounds": dict(lo=-440.0), "upper_bound": dict(hi=240.0), "no_clamp": dict(clamp=False), "e5m2": dict(f8=F8_E5M2)}
    links_k = _quantise(p, k, "k", **kw.get(case, {}))
    links_v = _quantise(p, v, "v")
    extra = []
    second = {"clamp_read_twice": 0, "cast_read_twice": 1, "bytes_read_twice": 2}.get(case)
    if second is not None:
        s = p.t("s", *links_k[second].shape, dtype=links_k[second].dtype)
        p(lt.neg, links_k[second], out=s)
        extra.append(s)
    if case == "v_bytes_returned":
        extra.append(links_v[2])
    if case == "late_q_read":
        extra.append(p(lt.neg, q, out=p.t("s", 1, 4, 1, 64)))
    if case is not None and case.startswith("late"):  # the positions are computed after the RoPE
        p(lt.silu, p.t("p0", 1, dtype=I64), out=pos)
    p(index_copy_inplace, kc, 2, pos, links_k[2], out=kc2)
    if case == "late_cache_read":  # between the two writes, which would both move to the later one
        extra.append(p(lt.neg, vc, out=p.t("s", 1, 4, 32, 64, dtype=U8)))
    p(index_copy_inplace, vc, 2, pos2 if case == "other_positions" else pos, links_v[2], out=vc2)
    return p.run(q, kc2, vc2, *extra)


def test_kv8_writes_fused_into_the_rope():
    assert _write_program() == ([_ROPE_CACHE], _KV)


def test_kv8_writes_fused_under_the_torch_executor_names():
    from lightning_thunder_amd.executors import torchex

    p = Program()
    pos = p.t("pos", 1, dtype=I64)
    qkv, cos, sin = p.t("qkv", 1, 1, 3 * 4 * 64), p.t("cos", 1, 64), p.t("sin", 1, 64)
    q, k, v = p.ts("q k v", 1, 4, 1, 64)
    kc, vc, kc2, vc2 = p.ts("kc vc kc2 vc2", 1, 4, 32, 64, dtype=U8)
    p(hipex.hip_qkv_rope, qkv, cos, sin, 4, 4, 64, 64, out=(q, k, v))
    us = []
    for t, tag in ((k, "k"), (v, "v")):
        c, f, u = p.t(tag + "_c", 1, 4, 1, 64), p.t(tag + "_f", 1, 4, 1, 64, dtype=F8), p.t(tag + "_u", 1, 4, 1, 64, dtype=U8)
        p(torchex.ex.opmap["torch_clamp"], t, -448.0, 448.0, out=c)
        p(torchex.ex.opmap["torch_to"], c, F8, out=f)
        p(torchex.ex.opmap["torch_view"], f, U8, out=u)
        us.append(u)
    p(index_copy_inplace, kc, 2, pos, us[0], out=kc2)
    p(index_copy_inplace, vc, 2, pos, us[1], out=vc2)
    assert p.run(q, kc2, vc2) == ([_ROPE_CACHE], _KV)


def test_kv8_writes_emitted_at_the_later_write():
    assert _write_program("late") == (["pos = silu(p0)", _ROPE_CACHE], _KV)


@pytest.mark.parametrize("case", ["bounds", "upper_bound", "no_clamp", "e5m2", "clamp_read_twice", "cast_read_twice",
                                  "bytes_read_twice", "v_bytes_returned", "other_positions", "bf16_cache",
                                  "late_q_read", "late_cache_read"])
def test_kv8_writes_refused(case):
    unchanged(_write_program(case))


def test_kv8_write_fusion_switch(monkeypatch):
    monkeypatch.setenv("LTA_KV8_FUSION", "0")
    unchanged(_write_program())


def _dequantise(p, cache, tag, f8=F8, dtype=BF16):
    f, d = p.t(tag + "f", 1, 4, 32, 64, dtype=f8), p.t(tag + "d", 1, 4, 32, 64, dtype=dtype)
    p(lt.view, cache, f8, out=f)
    p(lt.to, f, dtype, out=d)
    return f, d


def _read_program(case=None):
    p = Program()
    q, o = p.ts("q o", 1, 8, 1, 64)
    mask = p.t("mask", 1, 1, 1, 32, dtype=torch.bool)
    kc, vc = p.ts("kc vc", 1, 4, 32, 64, dtype=U8)
    extra = []
    _, kd = _dequantise(p, kc, "k", dtype=F16 if case == "dtype_mismatch" else BF16)
    if case == "mixed":
        vd = p.t("vd", 1, 4, 32, 64)  # a 16-bit value cache
        extra.append(vc)
    elif case == "e5m2":
        _, vd = _dequantise(p, vc, "v", f8=F8_E5M2)
    else:
        vf, vd = _dequantise(p, vc, "v")
    if case == "value_read_twice":
        s = p.t("s", 1, 4, 32, 64)
        p(lt.neg, vd, out=s)
        extra.append(s)
    if case == "view_read_twice":
        s = p.t("s", 1, 4, 32, 64, dtype=F8)
        p(lt.neg, vf, out=s)
        extra.append(s)
    p(hipex.hip_decode_attn, q, kd, vd, mask, False, 0.125, out=o)
    return p.run(o, *extra)


_ATTN8 = "o = hip_decode_attn_kv8(q, kc, vc, mask, False, 0.125)"


def test_kv8_read_fused_and_the_dequantise_dropped():
    assert _read_program() == ([_ATTN8], _READ)


def test_kv8_read_keeps_a_dequantised_value_that_is_read_elsewhere():
    assert _read_program("value_read_twice") == (
        ["vf = view(vc, torch.float8_e4m3fn)", "vd = to(vf, torch.bfloat16)", "s = neg(vd)", _ATTN8], _READ)


def test_kv8_read_keeps_a_view_that_is_read_elsewhere():
    assert _read_program("view_read_twice") == (["vf = view(vc, torch.float8_e4m3fn)", "s = neg(vf)", _ATTN8], _READ)


@pytest.mark.parametrize("case", ["mixed", "dtype_mismatch", "e5m2"])
def test_kv8_read_refused(case):
    unchanged(_read_program(case))


def test_kv8_read_fusion_switch(monkeypatch):
    monkeypatch.setenv("LTA_KV8_FUSION", "0")
    unchanged(_read_program())


def test_kv8_read_refused_after_an_inplace_write_of_the_cache():
    p = Program()
    q, o = p.ts("q o", 1, 8, 1, 64)
    mask = p.t("mask", 1, 1, 1, 32, dtype=torch.bool)
    pos = p.t("pos", 1, dtype=I64)
    row = p.t("row", 1, 4, 1, 64, dtype=U8)
    kc, vc, kc3 = p.ts("kc vc kc3", 1, 4, 32, 64, dtype=U8)
    _, kd = _dequantise(p, kc, "k")
    _, vd = _dequantise(p, vc, "v")
    p(index_copy_inplace, kc, 2, pos, row, out=kc3)  # the kernel would read the row the 16-bit copy predates
    p(hipex.hip_decode_attn, q, kd, vd, mask, False, 0.125, out=o)
    unchanged(p.run(o, kc3))


# ------------------------------------------------------------------------------------------------
# 4. the compiled decode path on the GPU (2-layer llama3-like at head size 64)
# ------------------------------------------------------------------------------------------------
def _gpu_models():
    kw = dict(n_layer=2, n_embd=256, n_head=4, n_query_groups=2, head_size=64, intermediate_size=384)
    m32 = _model("llama3-like", device="cuda", dtype=torch.float32, **kw)
    mb = _model("llama3-like", device="cuda", dtype=torch.float32, **kw).to(BF16)
    mb.load_state_dict({k: v.to(BF16) for k, v in m32.state_dict().items()})
    return m32, mb


def _teacher_forced(model, fwd, seq, steps):
    model.set_kv_cache(1, 64, device=torch.device("cuda"), dtype=F8)
    outs = [fwd(seq[:, :8], torch.arange(8, device="cuda"))[:, -1].float().clone()]
    for i in range(8, 8 + steps):
        outs.append(fwd(seq[:, i:i + 1], torch.tensor([i], device="cuda"))[:, -1].float().clone())
    caches = [(b.attn.kv_cache.k.clone(), b.attn.kv_cache.v.clone()) for b in model.transformer.h]
    return torch.stack(outs), caches


def _cache_shaped_casts(trace, cache_shape):
    """Casts / bitcasts that touch a whole cache (what the read fusion removes from a decode step)."""
    names = ("to", "torch_to", "convert_element_type", "view", "torch_view", "bitcast")
    out = []
    for b in trace.bound_symbols:
        subs = [b] + list(b.subsymbols or ()) if b.sym.is_fusion else [b]
        for s in subs:
            if s.sym.name in names and any(tuple(getattr(a, "shape", ())) == cache_shape for a in s.flat_proxy_args):
                out.append(s.sym.name)
    return out


@gpu
@pytest.mark.parametrize("graphs", [False, True])
def test_fp8_cache_decode_logits_teacher_forced_gpu(graphs):
    """``test_decode_logits_teacher_forced_gpu`` with the e4m3 cache in all three models: the compiled bf16
    model against bf16 eager and fp32 eager, err <= 3 base + 1e-3 at every step, replays bitwise equal; and
    the decode step's program holds one cache-writing RoPE and one e4m3 decode attention per layer."""
    m32, mb = _gpu_models()
    assert m32.config.head_size == 64 and m32.config.n_query_groups == 2
    seq = torch.randint(0, 300, (1, 24), device="cuda")
    transforms = []
    if graphs:
        from lightning_thunder_amd.transforms.hipgraph import HipGraphTransform

        transforms.append(HipGraphTransform())
    ref, _ = _teacher_forced(m32, m32, seq, 15)
    eager, _ = _teacher_forced(mb, mb, seq, 15)
    jm = thunder.jit(mb, transforms=transforms)
    got, _ = _teacher_forced(mb, jm, seq, 15)
    got2, _ = _teacher_forced(mb, jm, seq, 15)
    assert torch.equal(got, got2)
    for i in range(ref.shape[0]):
        base = ((eager[i] - ref[i]).norm() / ref[i].norm()).item()
        err = ((got[i] - ref[i]).norm() / ref[i].norm()).item()
        print(f"[kv8 teacher forced graphs={graphs}] step {i} err={err:.3e} base={base:.3e}")
        assert err <= 3 * base + 1e-3, (i, err, base)
    if not graphs:
        trace = thunder.last_traces(jm)[-1]  # the decode step's program
        names = [b.sym.name for b in trace.bound_symbols]
        assert names.count("hip_qkv_rope_cache") == 2 and names.count("hip_decode_attn_kv8") == 2, names
        assert "index_copy_inplace" not in names and "hip_decode_attn" not in names
        assert _cache_shaped_casts(trace, (1, 2, 64, 64)) == []
        for b in trace.bound_symbols:
            if b.sym.name == "hip_qkv_rope_cache":
                assert b.args[7].dtype == U8 and b.args[8].dtype == U8


@gpu
def test_fp8_cache_fused_decode_equals_the_unfused_program_gpu(monkeypatch):
    """The two rewrites change no bit: 8 teacher-forced decode steps of the fused program against the
    same program with ``LTA_KV8_FUSION=0`` (RoPE, clamp, cast, index_copy; dequantise, 16-bit decode
    attention), logits and cache bytes."""
    _, mb = _gpu_models()
    seq = torch.randint(0, 300, (1, 24), device="cuda")
    jm = thunder.jit(mb)
    fused, fused_caches = _teacher_forced(mb, jm, seq, 8)
    fused_names = [b.sym.name for b in thunder.last_traces(jm)[-1].bound_symbols]
    monkeypatch.setenv("LTA_KV8_FUSION", "0")
    jm0 = thunder.jit(mb)
    plain, plain_caches = _teacher_forced(mb, jm0, seq, 8)
    plain_names = [b.sym.name for b in thunder.last_traces(jm0)[-1].bound_symbols]
    assert fused_names.count("hip_decode_attn_kv8") == 2 and "hip_decode_attn_kv8" not in plain_names
    assert plain_names.count("hip_decode_attn") == 2 and plain_names.count("index_copy_inplace") == 4
    for (fk, fv), (pk, pv) in zip(fused_caches, plain_caches):
        assert torch.equal(fk, pk) and torch.equal(fv, pv), "the fused write must give the unfused program's bytes"
        assert fk[:, :, :16].any() and not fk[:, :, 16:].any()
    assert torch.equal(fused, plain), (fused - plain).abs().max().item()
