"""The scaled e4m3 KV cache (``set_kv_cache(dtype=torch.float8_e4m3fn, scale="row")``): the number format's
definition (``ops/kv8.py``) and the model's semantics on the CPU, the two hipex rewrites on hand-built traces,
and the compiled decode path on the GPU.

A row is stored as the e4m3 bytes of ``x * 2^-e`` plus the byte ``e + 127``, ``e`` the smallest exponent in
[-15, 7] with ``amax * 2^-e <= 448``.  On the GPU the write runs in the RoPE kernel (``hip_qkv_rope_cache_s8``)
and the decode attention applies the scales itself (``hip_decode_attn_kv8s``); ``LTA_KV8_FUSION=0`` keeps the
program as the model spells it, and the two agree bit for bit.
"""
import pytest
import torch

import lightning_thunder_amd as thunder
from lightning_thunder_amd import torch as lt
from lightning_thunder_amd.executors import hipex
from lightning_thunder_amd.models.litgpt import KVCache, generate
from lightning_thunder_amd.ops.kv8 import dequantise_rows, kv8_dequantise_rows, kv8_quantise_rows, quantise_rows
from lightning_thunder_amd.torch.custom_op import custom_op_symbol, opdef_of
from lightning_thunder_amd.transforms.inplace_index_copy import index_copy_inplace

from test_hipex_passes import Program, unchanged
from test_kv8_cache import _cache_shaped_casts, _gpu_models, _model, _quantise

BF16, F16, F32, U8, I64 = torch.bfloat16, torch.float16, torch.float32, torch.uint8, torch.int64
F8 = torch.float8_e4m3fn
gpu = pytest.mark.gpu
MAGNITUDES = [1e-6, 1e-5, 1e-4, 1e-3, 1e-2, 1e-1, 1.0, 1e1, 1e2, 1e3]


# ------------------------------------------------------------------------------------------------
# 1. the definition
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("m", MAGNITUDES)
def test_quantise_rows_definition(m, dtype):
    torch.manual_seed(0)
    x = (torch.randn(4, 3, 50, 64) * m).to(dtype)
    b, s = quantise_rows(x)
    assert b.dtype == s.dtype == U8 and b.shape == x.shape and s.shape == (4, 3, 50, 1)
    e = s.int() - 127
    assert int(e.min()) >= -15 and int(e.max()) <= 7
    exact = b.view(F8).double() * torch.exp2(e.double())
    for out in (dtype, F32):
        assert torch.equal(dequantise_rows(b, s, out).double(), exact), "dequantise_rows is exact"
    scaled = (x.double() * torch.exp2(-e.double())).abs().amax(-1, keepdim=True)
    assert (scaled[e < 7] <= 448).all(), "below the upper clamp no element saturates"
    assert (scaled[(e > -15) & (e < 7)] > 224).all(), "inside the range e is the smallest exponent that fits"
    if 1e-2 <= m <= 1e2:
        assert ((e > -15) & (e < 7)).all()
    # the error is the e4m3 rounding's (relative 2^-4 per element at worst, ~0.027 in L2 over a normal row)
    # wherever the row's values are e4m3 normals after scaling
    if m >= 1e-4:
        rel = ((exact - x.double()).norm() / x.double().norm()).item()
        assert rel < 0.04, rel


def test_quantise_rows_zero_and_saturating_rows():
    z = torch.zeros(2, 1, 3, 64, dtype=BF16)
    b, s = quantise_rows(z)
    assert (s == 112).all() and not b.any()
    for dtype in (BF16, F32):
        big = torch.full((1, 1, 2, 64), 1e5, dtype=dtype)
        big[..., 1::2] = -1e5
        b, s = quantise_rows(big)
        assert (s == 134).all() and set(b.flatten().tolist()) == {0x7E, 0xFE}
        assert torch.equal(dequantise_rows(b, s, F32), big.float().sign() * 57344.0)


@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("n", [-6, 3])
def test_quantise_rows_shift_invariance(n, dtype):
    """Rows whose exponent stays strictly inside the range: ``x * 2^n`` has the same bytes and a scale byte ``n``
    higher.  The inputs are multiples of 2^-6 of magnitude ~1, so ``x * 2^n`` is exact in T."""
    torch.manual_seed(1)
    x = ((torch.randn(8, 2, 5, 64) * 64).round() / 64).to(dtype)
    y = (x.float() * 2.0 ** n).to(dtype)
    assert torch.equal(y.float(), x.float() * 2.0 ** n)
    (bx, sx), (by, sy) = quantise_rows(x), quantise_rows(y)
    assert 112 < int(sx.min()) + min(n, 0) and int(sx.max()) + max(n, 0) < 134
    assert torch.equal(bx, by) and torch.equal(sx.int() + n, sy.int())


def test_custom_ops_are_the_definition():
    torch.manual_seed(2)
    x = torch.randn(2, 3, 4, 32).to(BF16)
    (b, s), (b0, s0) = kv8_quantise_rows(x), quantise_rows(x)
    assert torch.equal(b, b0) and torch.equal(s, s0)
    assert torch.equal(kv8_dequantise_rows(b, s, F16), dequantise_rows(b0, s0, F16))
    fake = kv8_quantise_rows(x.to("meta"))
    assert [(t.shape, t.dtype) for t in fake] == [(x.shape, U8), ((2, 3, 4, 1), U8)]
    assert kv8_dequantise_rows(*fake, BF16).shape == x.shape


# ------------------------------------------------------------------------------------------------
# 2. the model
# ------------------------------------------------------------------------------------------------
def test_scaled_cache_holds_the_quantised_keys_and_values():
    m = _model()
    p = torch.randint(0, 300, (1, 8))
    seen = []
    m.set_kv_cache(1, 64, dtype=F8, scale="row")
    for block in m.transformer.h:
        c = block.attn.kv_cache
        assert c.k.dtype == c.v.dtype == c.k_scale.dtype == c.v_scale.dtype == U8
        assert c.k.shape == c.v.shape == (1, 2, 64, 16) and c.k_scale.shape == c.v_scale.shape == (1, 2, 64, 1)
        assert not c.k.any() and not c.v.any() and (c.k_scale == 127).all() and (c.v_scale == 127).all()
        assert not set(c.state_dict()) & {"k", "v", "k_scale", "v_scale"}, "the four buffers are non-persistent"
    hook = m.transformer.h[0].attn.kv_cache.register_forward_pre_hook(lambda mod, args: seen.append(args))
    m(p, torch.arange(8))
    hook.remove()
    (_, k, v), = seen
    c = m.transformer.h[0].attn.kv_cache
    (k8, ks), (v8, vs) = quantise_rows(k), quantise_rows(v)
    assert torch.equal(c.k[:, :, :8], k8) and torch.equal(c.v[:, :, :8], v8)
    assert torch.equal(c.k_scale[:, :, :8], ks) and torch.equal(c.v_scale[:, :, :8], vs)
    assert c.k[:, :, :8].any() and (c.k_scale[:, :, :8] != 127).any()
    assert not c.k[:, :, 8:].any() and not c.v[:, :, 8:].any()
    assert (c.k_scale[:, :, 8:] == 127).all() and (c.v_scale[:, :, 8:] == 127).all()
    c.reset_parameters()
    assert not c.k.any() and not c.v.any() and (c.k_scale == 127).all() and (c.v_scale == 127).all()


@pytest.mark.parametrize("dtype", [BF16, torch.float32, None])
def test_scale_needs_the_e4m3_dtype(dtype):
    m = _model()
    with pytest.raises(ValueError, match="float8_e4m3fn"):
        m.set_kv_cache(1, 64, dtype=dtype, scale="row")
    with pytest.raises(ValueError, match="float8_e4m3fn"):
        KVCache((1, 2, 8, 16), (1, 2, 8, 16), dtype=dtype, scale="row")
    with pytest.raises(ValueError, match="scale"):
        KVCache((1, 2, 8, 16), (1, 2, 8, 16), dtype=F8, scale="tensor")


def test_scale_none_is_the_unscaled_cache():
    c = KVCache((1, 1, 4, 16), (1, 1, 4, 16), dtype=F8)
    assert sorted(n for n, _ in c.named_buffers()) == ["k", "v"] and c.scale is None
    torch.manual_seed(3)
    k = torch.randn(1, 1, 1, 16) * 300
    k_all, _ = c(torch.tensor([2]), k, k)
    assert torch.equal(c.k[0, 0, 2], k[0, 0, 0].clamp(-448, 448).to(F8).view(U8))
    assert torch.equal(k_all[0, 0, 2], k[0, 0, 0].clamp(-448, 448).to(F8).float())


def test_scaled_cache_keeps_small_values_the_unscaled_one_loses():
    """V rows of size 1e-3: attention over the scaled cache is within e4m3 rounding of attention over the fp32
    k / v; over the unscaled cache, whose small values fall into e4m3's subnormals, it is several times
    further off.  The two errors are compared with each other."""
    torch.manual_seed(4)
    B, G, S, D = 1, 2, 48, 64
    q, k, v = torch.randn(B, G, 4, D), torch.randn(B, G, S, D), torch.randn(B, G, S, D) * 1e-3
    pos = torch.arange(S)
    ref = torch.nn.functional.scaled_dot_product_attention(q, k, v)
    errs = {}
    for scale in (None, "row"):
        c = KVCache((B, G, S, D), (B, G, S, D), dtype=F8, scale=scale)
        k_all, v_all = c(pos, k, v)
        out = torch.nn.functional.scaled_dot_product_attention(q, k_all, v_all)
        errs[scale] = ((out - ref).norm() / ref.norm()).item()
    print(f"[kv8 scaled vs unscaled, V ~ 1e-3] rel err scaled {errs['row']:.3e} unscaled {errs[None]:.3e}")
    assert 4 * errs["row"] < errs[None], errs


def test_scaled_cache_generate_matches_eager_and_reuses_programs():
    m = _model()
    p = torch.randint(0, 300, (1, 8))
    m.set_kv_cache(1, 64, dtype=F8, scale="row")
    ref = generate(m, p, 12)
    m.set_kv_cache(1, 64, dtype=F8, scale="row")
    jm = thunder.jit(m)
    out = generate(m, p, 12, forward=jm)
    assert torch.equal(ref, out)
    assert thunder.cache_misses(jm) == 2  # prefill + decode
    assert thunder.cache_hits(jm) == 10
    trace = thunder.last_traces(jm)[-1]
    ids = [b.sym.id for b in trace.bound_symbols]
    n = len(m.transformer.h)
    assert sum(i in hipex._KV8_QUANTISE_IDS for i in ids) == 2 * n, "each quantise is one symbol"
    assert sum(i in hipex._KV8_DEQUANTISE_IDS for i in ids) == 2 * n, "each dequantise is one symbol"
    writes = [b for b in trace.bound_symbols if b.sym.name == "index_copy_inplace"]
    assert len(writes) == 4 * n and all(b.args[0].dtype == U8 for b in writes)


# ------------------------------------------------------------------------------------------------
# 3. the rewrites on hand-built traces
# ------------------------------------------------------------------------------------------------
QUANTISE, DEQUANTISE = custom_op_symbol(opdef_of(kv8_quantise_rows)), custom_op_symbol(opdef_of(kv8_dequantise_rows))
_ROPE_S8 = "q, kc2, vc2, ksc2, vsc2 = hip_qkv_rope_cache_s8(qkv, cos, sin, 4, 4, 64, 64, kc, vc, ksc, vsc, pos)"
_KV = "hipex: 1 KV-cache write pair(s) fused into RoPE"
_READ = "hipex: 1 decode attention(s) read their e4m3 KV cache directly"


def test_the_custom_op_symbols_are_the_ones_the_passes_match():
    assert QUANTISE.id in hipex._KV8_QUANTISE_IDS and DEQUANTISE.id in hipex._KV8_DEQUANTISE_IDS


def _write_program(case=None):
    p = Program()
    pos, pos2 = p.ts("pos pos2", 1, dtype=I64)
    qkv, cos, sin = p.t("qkv", 1, 1, 3 * 4 * 64), p.t("cos", 1, 64), p.t("sin", 1, 64)
    q, k, v = p.ts("q k v", 1, 4, 1, 64)
    kc, vc, kc2, vc2 = p.ts("kc vc kc2 vc2", 1, 4, 32, 64, dtype=U8)
    ksc, vsc, ksc2, vsc2 = p.ts("ksc vsc ksc2 vsc2", 1, 4, 32, 1, dtype=U8)
    k8, v8 = p.ts("k8 v8", 1, 4, 1, 64, dtype=U8)
    ks, vs = p.ts("ks vs", 1, 4, 1, 1, dtype=U8)
    p(hipex.hip_qkv_rope, qkv, cos, sin, 4, 4, 64, 64, out=(q, k, v))
    extra = []
    if case == "mixed_reverse":  # k through the unscaled cache's chain
        _, _, k8 = _quantise(p, k, "k")
    else:
        p(QUANTISE, k, out=(k8, ks))
    if case == "mixed":  # v through the unscaled cache's chain
        _, _, v8 = _quantise(p, v, "v")
    else:
        p(QUANTISE, v, out=(v8, vs))
    for name, t in (("bytes_read_twice", k8), ("scale_read_twice", vs)):
        if case == name:
            s = p.t("s", *t.shape, dtype=U8)
            p(lt.neg, t, out=s)
            extra.append(s)
    if case == "scale_returned":
        extra.append(ks)
    if case == "late_q_read":
        extra.append(p(lt.neg, q, out=p.t("s", 1, 4, 1, 64)))
    if case is not None and case.startswith("late"):  # the positions are computed after the RoPE
        p(lt.silu, p.t("p0", 1, dtype=I64), out=pos)
    p(index_copy_inplace, kc, 2, pos, k8, out=kc2)
    if case == "late_cache_read":  # between the first and the last write, which would all move to the last
        extra.append(p(lt.neg, vsc, out=p.t("s", 1, 4, 32, 1, dtype=U8)))
    p(index_copy_inplace, vc, 2, pos, v8, out=vc2)
    if case == "mixed_reverse":
        p(index_copy_inplace, vsc, 2, pos, vs, out=vsc2)
        return p.run(q, kc2, vc2, vsc2, *extra)
    p(index_copy_inplace, ksc, 2, pos2 if case == "scale_at_other_positions" else pos, ks, out=ksc2)
    if case != "mixed":
        p(index_copy_inplace, vsc, 3 if case == "other_dim" else 2, pos, vs, out=vsc2)
        return p.run(q, kc2, vc2, ksc2, vsc2, *extra)
    return p.run(q, kc2, vc2, ksc2, *extra)


def test_scaled_writes_fused_into_the_rope():
    assert _write_program() == ([_ROPE_S8], _KV)


def test_scaled_writes_emitted_at_the_last_write():
    assert _write_program("late") == (["pos = silu(p0)", _ROPE_S8], _KV)


@pytest.mark.parametrize("case", ["scale_at_other_positions", "bytes_read_twice", "scale_read_twice", "scale_returned",
                                  "mixed", "mixed_reverse", "other_dim", "late_q_read", "late_cache_read"])
def test_scaled_writes_refused(case):
    unchanged(_write_program(case))


def test_scaled_write_fusion_switch(monkeypatch):
    monkeypatch.setenv("LTA_KV8_FUSION", "0")
    unchanged(_write_program())


def _read_program(case=None):
    p = Program()
    q, o = p.ts("q o", 1, 8, 1, 64)
    mask = p.t("mask", 1, 1, 1, 32, dtype=torch.bool)
    pos = p.t("pos", 1, dtype=I64)
    kc, vc = p.ts("kc vc", 1, 4, 32, 64, dtype=U8)
    ksc, vsc, vsc3 = p.ts("ksc vsc vsc3", 1, 4, 32, 1, dtype=U8)
    kd = p.t("kd", 1, 4, 32, 64, dtype=F16 if case == "dtype_mismatch" else BF16)
    vd = p.t("vd", 1, 4, 32, 64)
    extra = []
    p(DEQUANTISE, kc, ksc, F16 if case == "dtype_mismatch" else BF16, out=kd)
    if case == "mixed":  # v through the unscaled cache's view / to
        vf = p.t("vf", 1, 4, 32, 64, dtype=F8)
        p(lt.view, vc, F8, out=vf)
        p(lt.to, vf, BF16, out=vd)
    else:
        p(DEQUANTISE, vc, vsc, BF16, out=vd)
    if case == "value_read_twice":
        s = p.t("s", 1, 4, 32, 64)
        p(lt.neg, vd, out=s)
        extra.append(s)
    if case == "scale_written_in_between":
        row = p.t("row", 1, 4, 1, 1, dtype=U8)
        p(index_copy_inplace, vsc, 2, pos, row, out=vsc3)  # the kernel would read a scale the 16-bit copy predates
        extra.append(vsc3)
    p(hipex.hip_decode_attn, q, kd, vd, mask, False, 0.125, out=o)
    return p.run(o, *extra)


_ATTN8S = "o = hip_decode_attn_kv8s(q, kc, vc, ksc, vsc, mask, False, 0.125)"


def test_scaled_read_fused_and_the_dequantise_dropped():
    assert _read_program() == ([_ATTN8S], _READ)


def test_scaled_read_keeps_a_dequantised_value_that_is_read_elsewhere():
    lines, msg = _read_program("value_read_twice")
    assert msg == _READ and lines[-1] == _ATTN8S and len(lines) == 3
    assert lines[0].startswith("vd = ") and "kv8_dequantise_rows(vc, vsc, torch.bfloat16)" in lines[0]
    assert lines[1] == "s = neg(vd)"


@pytest.mark.parametrize("case", ["mixed", "dtype_mismatch", "scale_written_in_between"])
def test_scaled_read_refused(case):
    unchanged(_read_program(case))


def test_scaled_read_fusion_switch(monkeypatch):
    monkeypatch.setenv("LTA_KV8_FUSION", "0")
    unchanged(_read_program())


# ------------------------------------------------------------------------------------------------
# 4. the compiled decode path on the GPU (2-layer llama3-like at head size 64, 2 groups, max_seq 64)
# ------------------------------------------------------------------------------------------------
def _teacher_forced(model, fwd, seq, steps):
    model.set_kv_cache(1, 64, device=torch.device("cuda"), dtype=F8, scale="row")
    outs = [fwd(seq[:, :8], torch.arange(8, device="cuda"))[:, -1].float().clone()]
    for i in range(8, 8 + steps):
        outs.append(fwd(seq[:, i:i + 1], torch.tensor([i], device="cuda"))[:, -1].float().clone())
    caches = [tuple(t.clone() for t in (c.k, c.v, c.k_scale, c.v_scale)) for c in (b.attn.kv_cache for b in model.transformer.h)]
    return torch.stack(outs), caches


@gpu
@pytest.mark.parametrize("graphs", [False, True])
def test_scaled_cache_decode_logits_teacher_forced_gpu(graphs):
    """``test_fp8_cache_decode_logits_teacher_forced_gpu`` with the scaled cache in all three models: the compiled
    bf16 model against bf16 eager and fp32 eager, err <= 3 base + 1e-3 at every step (that test's bound: the
    compiled program may differ from bf16 eager by bf16 rounding of other kernels, not by the cache, which all
    three quantise alike), replays bitwise equal; and the decode step's program holds one scaled cache-writing
    RoPE and one scaled decode attention per layer."""
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
        print(f"[kv8s teacher forced graphs={graphs}] step {i} err={err:.3e} base={base:.3e}")
        assert err <= 3 * base + 1e-3, (i, err, base)
    if not graphs:
        trace = thunder.last_traces(jm)[-1]  # the decode step's program
        names = [b.sym.name for b in trace.bound_symbols]
        assert names.count("hip_qkv_rope_cache_s8") == 2 and names.count("hip_decode_attn_kv8s") == 2, names
        assert "index_copy_inplace" not in names and "hip_decode_attn" not in names
        assert not any(b.sym.id in hipex._KV8_QUANTISE_IDS + hipex._KV8_DEQUANTISE_IDS for b in trace.bound_symbols)
        assert _cache_shaped_casts(trace, (1, 2, 64, 64)) == []
        for b in trace.bound_symbols:
            if b.sym.name == "hip_qkv_rope_cache_s8":
                assert all(b.args[i].dtype == U8 for i in (7, 8, 9, 10))


@gpu
def test_scaled_cache_fused_decode_equals_the_unfused_program_gpu(monkeypatch):
    """The two rewrites change no bit: 8 teacher-forced decode steps of the fused program against the same
    program with ``LTA_KV8_FUSION=0`` (RoPE, quantise op, four index_copy; dequantise op, 16-bit decode
    attention): logits, all four cache buffers, and the rows never written."""
    _, mb = _gpu_models()
    seq = torch.randint(0, 300, (1, 24), device="cuda")
    jm = thunder.jit(mb)
    fused, fused_caches = _teacher_forced(mb, jm, seq, 8)
    fused_names = [b.sym.name for b in thunder.last_traces(jm)[-1].bound_symbols]
    monkeypatch.setenv("LTA_KV8_FUSION", "0")
    jm0 = thunder.jit(mb)
    plain, plain_caches = _teacher_forced(mb, jm0, seq, 8)
    plain_names = [b.sym.name for b in thunder.last_traces(jm0)[-1].bound_symbols]
    assert fused_names.count("hip_decode_attn_kv8s") == 2 and fused_names.count("hip_qkv_rope_cache_s8") == 2
    assert "hip_decode_attn_kv8s" not in plain_names and "hip_qkv_rope_cache_s8" not in plain_names
    assert plain_names.count("hip_decode_attn") == 2 and plain_names.count("index_copy_inplace") == 8
    for f4, p4 in zip(fused_caches, plain_caches):
        for name, f, p_ in zip(("k", "v", "k_scale", "v_scale"), f4, p4):
            assert torch.equal(f, p_), f"the fused write must give the unfused program's {name} bytes"
        fk, _, fks, fvs = f4
        assert fk[:, :, :16].any() and not fk[:, :, 16:].any()
        assert (fks[:, :, :16] != 127).any() and (fks[:, :, 16:] == 127).all() and (fvs[:, :, 16:] == 127).all()
    assert torch.equal(fused, plain), (fused - plain).abs().max().item()
