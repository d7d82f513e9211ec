"""MXFP4 decode GEMV with the RMSNorm prologue, the gated (SwiGLU) pair, the bias / activation /
residual epilogue and grouped projections: kernel, op layer, executor pass and compiled decode."""
import functools

import pytest
import torch

MODES = ["plain_residual", "bias_silu_residual", "norm", "gated", "norm_gated", "norm_residual"]
# (N, K): 3 blocks per row (most lanes idle, N no multiple of the columns per workgroup); 65 blocks
# (a second loop trip with one live lane); the common case; the wide 8-columns-per-wave instantiation
SHAPES = [(130, 96), (512, 2080), (1536, 2048), (8192, 128)]
EPS = 1e-5


@functools.lru_cache(maxsize=None)
def _operands(N, K, device="cuda", dtype=torch.bfloat16):
    """One set of operands per shape, shared (and left unchanged) by every case of that shape."""
    from lightning_thunder_amd.ops import mxfp4

    gen = torch.Generator(device="cpu").manual_seed(N * 7919 + K)

    def randn(*shape):
        return torch.randn(*shape, generator=gen)

    o = dict(x=(randn(8, K) * 3).to(device, dtype), g=(torch.rand(K, generator=gen) + 0.5).to(device, dtype),
             bias=randn(N).to(device, dtype), res=randn(8, N).to(device, dtype))
    quant = mxfp4.quantize if device == "cuda" else mxfp4.quantize_reference
    o["q"], o["s"] = quant((randn(N, K) * 0.02).to(device, dtype))
    o["gq"], o["gs"] = quant((randn(N, K) * 0.02).to(device, dtype))
    return o


def _mode_kwargs(o, mode, M):
    kw = {}
    if "bias" in mode:
        kw["bias"] = o["bias"]
    if "residual" in mode:
        kw["residual"] = o["res"][:M]
    if "silu" in mode or "gated" in mode:
        kw["act"] = "silu"
    if "gated" in mode:
        kw["gate_q"], kw["gate_s"] = o["gq"], o["gs"]
    return kw


# ---- kernel against the reference ----------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("M", [1, 3, 8])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("N,K", SHAPES)
def test_gemv_fused_matches_reference(N, K, mode, M):
    from lightning_thunder_amd.ops import mxfp4
    from lightning_thunder_amd.ops.rmsnorm import rms_norm_fwd

    o = _operands(N, K)
    x = o["x"][:M]
    kw = _mode_kwargs(o, mode, M)
    norm = "norm" in mode
    assert mxfp4.gemv_fused_supported(x, o["q"], o["s"], norm_weight=o["g"] if norm else None, **kw)
    out = mxfp4.gemv_fused(x, o["q"], o["s"], norm=norm, norm_weight=o["g"] if norm else None, eps=EPS, **kw)
    xn = rms_norm_fwd(x, o["g"], EPS)[0] if norm else x
    ref = mxfp4.gemv_fused_reference(xn, o["q"], o["s"], **kw)
    assert out.shape == (M, N) and out.dtype == torch.bfloat16
    torch.testing.assert_close(out.float(), ref.float(), atol=3e-2, rtol=2e-2)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["plain_residual", "norm_residual", "norm_gated"])
@pytest.mark.parametrize("N,K", SHAPES)
def test_gemv_fused_strided_rows(N, K, mode):
    """x and the residual as non-contiguous row slices (ldx != K, ldr != N)."""
    from lightning_thunder_amd.ops import mxfp4
    from lightning_thunder_amd.ops.rmsnorm import rms_norm_fwd

    o = _operands(N, K)
    M = 3
    xw = torch.zeros(M, K + 64, device="cuda", dtype=torch.bfloat16)
    xw[:, :K] = o["x"][:M]
    x = xw[:, :K]
    rw = torch.zeros(M, N + 24, device="cuda", dtype=torch.bfloat16)
    rw[:, 8:8 + N] = o["res"][:M]
    kw = _mode_kwargs(o, mode, M)
    if "residual" in kw:
        kw["residual"] = rw[:, 8:8 + N]
        assert kw["residual"].stride(0) != N
    assert x.stride(0) != K
    norm = "norm" in mode
    g = o["g"] if norm else None
    assert mxfp4.gemv_fused_supported(x, o["q"], o["s"], norm_weight=g, **kw)
    out = mxfp4.gemv_fused(x, o["q"], o["s"], norm=norm, norm_weight=g, eps=EPS, **kw)
    # the same kernel on contiguous copies accumulates in the same order
    kc = dict(kw)
    if "residual" in kc:
        kc["residual"] = kc["residual"].contiguous()
    assert torch.equal(out, mxfp4.gemv_fused(x.contiguous(), o["q"], o["s"], norm=norm, norm_weight=g, eps=EPS, **kc))
    xn = rms_norm_fwd(x.contiguous(), g, EPS)[0] if norm else x
    ref = mxfp4.gemv_fused_reference(xn, o["q"], o["s"], **kw)
    torch.testing.assert_close(out.float(), ref.float(), atol=3e-2, rtol=2e-2)


@pytest.mark.gpu
@pytest.mark.parametrize("M", [1, 3, 8])
@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("ns", [(256, 64, 64), (130, 96), (8192, 256, 256)])
def test_gemv_group_equals_separate_launches(ns, norm, packed, M):
    """Same kernel, same accumulation order: each grouped output equals gemv_fused of that projection."""
    from lightning_thunder_amd.ops import mxfp4

    K = 256
    o = _operands(max(ns), K)
    x = o["x"][:M]
    g = o["g"] if norm else None
    # segments of different length cut from the shape's two weights
    src = [(o["q"], o["s"]), (o["gq"], o["gs"]), (o["q"].flip(0).contiguous(), o["s"].flip(0).contiguous())]
    weights = [(q[:n].contiguous(), s[:n].contiguous()) for (q, s), n in zip(src, ns)]
    outs = mxfp4.gemv_group(x, weights, norm=norm, norm_weight=g, eps=EPS, packed=packed)
    if packed:
        assert outs.shape == (M, sum(ns))
        outs = outs.split(list(ns), dim=1)
    assert len(outs) == len(ns)
    for out, (q, s) in zip(outs, weights):
        assert torch.equal(out, mxfp4.gemv_fused(x, q, s, norm=norm, norm_weight=g, eps=EPS))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["bias_silu_residual", "norm_gated"])
def test_gemv_fused_is_deterministic(mode):
    from lightning_thunder_amd.ops import mxfp4

    o = _operands(1536, 2048)
    kw = _mode_kwargs(o, mode, 3)
    norm = "norm" in mode
    run = lambda: mxfp4.gemv_fused(o["x"][:3], o["q"], o["s"], norm=norm, norm_weight=o["g"] if norm else None,
                                   eps=EPS, **kw)
    assert torch.equal(run(), run())
    ws = [(o["q"], o["s"]), (o["gq"], o["gs"])]
    a = mxfp4.gemv_group(o["x"][:3], ws, norm=True, norm_weight=o["g"], eps=EPS, packed=True)
    assert torch.equal(a, mxfp4.gemv_group(o["x"][:3], ws, norm=True, norm_weight=o["g"], eps=EPS, packed=True))


@pytest.mark.gpu
def test_unsupported_operands_take_the_reference():
    """9 rows, K = 48 and a misaligned x are refused by the kernel's entry point; the operator then
    computes the reference math.  (No MXFP4 weight has K = 48 - a block is 32 wide - so that case has
    no product to compare: the support check and the entry point's -2 are what is asserted.)"""
    from lightning_thunder_amd.ops import mxfp4
    from lightning_thunder_amd.ops._lib import require, stream_ptr
    from lightning_thunder_amd.executors import hipex

    N, K = 130, 96
    o = _operands(N, K)
    x9 = torch.cat([o["x"], o["x"][:1]])
    assert x9.shape[0] == 9 and not mxfp4.gemv_fused_supported(x9, o["q"], o["s"])
    xm = torch.zeros(3, K + 8, device="cuda", dtype=torch.bfloat16)[:, 4:4 + K]
    xm.copy_(o["x"][:3])
    assert xm.data_ptr() % 16 == 8 and not mxfp4.gemv_fused_supported(xm, o["q"], o["s"])
    for x in (x9, xm):
        with pytest.raises(ValueError):
            mxfp4.gemv_fused(x, o["q"], o["s"])
        kw = dict(bias=o["bias"], act="silu", norm=True, norm_weight=o["g"], eps=EPS)
        got = hipex._mxfp4_decode_linear_impl(x, o["q"], o["s"], **kw)
        assert torch.equal(got, mxfp4.gemv_fused_reference(x, o["q"], o["s"], **kw))
        outs = hipex._mxfp4_decode_group_impl(x, ((o["q"], o["s"]), (o["gq"], o["gs"])), True, o["g"], EPS, True)
        assert torch.equal(outs[:, :N], mxfp4.gemv_fused_reference(x, o["q"], o["s"], norm=True, norm_weight=o["g"],
                                                                   eps=EPS))

    x48 = torch.zeros(1, 48, device="cuda", dtype=torch.bfloat16)
    q48 = torch.zeros(N, 24, device="cuda", dtype=torch.uint8)
    s48 = torch.zeros(N, 1, device="cuda", dtype=torch.uint8)
    assert not mxfp4.gemv_fused_supported(x48, q48, s48)
    y = torch.full((1, N), 7.0, device="cuda", dtype=torch.bfloat16)
    lib = require()
    for M, Kk, xp, ldx in ((9, K, x9, K), (1, 48, x48, 48), (3, K, xm, K + 8)):
        rc = lib.lta_gemv_mxfp4_fused(xp.data_ptr(), o["q"].data_ptr(), o["s"].data_ptr(), None, None, None, 0, EPS,
                                      None, None, y.data_ptr(), M, N, Kk, ldx, N, 0, 0, stream_ptr(y.device))
        assert rc == -2
    torch.cuda.synchronize()
    assert (y == 7).all()  # nothing was launched


# ---- compiled decode ---------------------------------------------------------------------------------
def _litgpt():
    from lightning_thunder_amd.models.litgpt import GPT, init_weights

    torch.manual_seed(0)
    m = GPT.from_name("llama3-like", n_layer=2, n_embd=256, n_head=4, head_size=64, intermediate_size=512).to(
        device="cuda", dtype=torch.bfloat16)
    init_weights(m, std=0.05)
    m.requires_grad_(False)
    m.set_kv_cache(1, 64)
    return m


def _decode_inputs():
    gen = torch.Generator().manual_seed(1)
    idx = torch.randint(0, 300, (1, 8), generator=gen).cuda()
    toks = [torch.randint(0, 300, (1, 1), generator=gen).cuda() for _ in range(3)]
    return idx, torch.arange(8, device="cuda"), toks


@pytest.mark.gpu
def test_mxfp4_decode_fusion_in_litgpt_decode():
    import lightning_thunder_amd as thunder
    from lightning_thunder_amd.transforms.mxfp4_inference import MXFP4InferenceTransform

    idx, pos, toks = _decode_inputs()
    p1 = torch.tensor([8], device="cuda")
    m = _litgpt()
    jm = thunder.jit(m, transforms=[MXFP4InferenceTransform(skip=())])
    jm(idx, pos)
    out = jm(toks[0], p1)
    trace = str(thunder.last_traces(jm)[-1])
    assert "hip_mxfp4_decode_linear" in trace, trace
    assert "hip_rms_norm_fwd" not in trace and "hip_swiglu(" not in trace, trace
    assert "custom_op_lta_mxfp4_linear" not in trace, trace
    assert "'silu'" in trace and "True, t_transformer_ln_f_weight" in trace, trace  # gated pair; LM head's norm
    # the residual adds between blocks ride in the projections' epilogues
    assert not any("add(" in line and "[1, 1, 256]" in line for line in trace.splitlines()), trace
    # the same transformed module run eagerly takes the unfused custom-op path
    m.set_kv_cache(1, 64, device="cuda", dtype=torch.bfloat16)
    m(idx, pos)
    ref = m(toks[0], p1)
    torch.testing.assert_close(out.float(), ref.float(), atol=5e-2, rtol=5e-2)


@pytest.mark.gpu
def test_mxfp4_decode_fusion_switch_off(monkeypatch):
    import lightning_thunder_amd as thunder
    from lightning_thunder_amd.transforms.mxfp4_inference import MXFP4InferenceTransform

    monkeypatch.setenv("LTA_MXFP4_DECODE_FUSION", "0")
    idx, pos, toks = _decode_inputs()
    jm = thunder.jit(_litgpt(), transforms=[MXFP4InferenceTransform(skip=())])
    jm(idx, pos)
    jm(toks[0], torch.tensor([8], device="cuda"))
    trace = str(thunder.last_traces(jm)[-1])
    assert "custom_op_lta_mxfp4_linear" in trace and "hip_mxfp4_decode_linear" not in trace, trace


@pytest.mark.gpu
def test_mxfp4_decode_fusion_under_hipgraph():
    """The rewritten decode step captures (no host sync, no allocation but torch.empty) and replays
    to the same logits as the uncaptured fused program over three consecutive positions."""
    import lightning_thunder_amd as thunder
    from lightning_thunder_amd.transforms.hipgraph import HipGraphTransform
    from lightning_thunder_amd.transforms.mxfp4_inference import MXFP4InferenceTransform

    idx, pos, toks = _decode_inputs()
    plain = thunder.jit(_litgpt(), transforms=[MXFP4InferenceTransform(skip=())])
    graphed = thunder.jit(_litgpt(), transforms=[MXFP4InferenceTransform(skip=()), HipGraphTransform()])
    plain(idx, pos)
    graphed(idx, pos)
    for i, tok in enumerate(toks):
        p = torch.tensor([8 + i], device="cuda")
        a, b = plain(tok, p), graphed(tok, p)
        assert torch.equal(a, b), i
    assert "hip_mxfp4_decode_linear" in str(thunder.last_traces(plain)[-1])


@pytest.mark.gpu
def test_mxfp4_decode_fusion_in_hf_llama_decode(monkeypatch):
    tf = pytest.importorskip("transformers")
    import lightning_thunder_amd as thunder
    from lightning_thunder_amd.core.recipe import Plugin
    from lightning_thunder_amd.transforms.mxfp4_inference import MXFP4InferenceTransform

    class MXFP4(Plugin):
        def setup_transforms(self):
            return [MXFP4InferenceTransform(skip=())]

        def setup_executors(self):  # the recipe lists its executors: add the one that runs custom ops
            from lightning_thunder_amd.executors.custom_opex import custom_op_ex

            return [custom_op_ex]

    cfg = tf.LlamaConfig(vocab_size=512, hidden_size=256, intermediate_size=512, num_hidden_layers=2,
                         num_attention_heads=4, num_key_value_heads=2, max_position_embeddings=256)
    torch.manual_seed(0)
    with torch.device("cuda"):
        m = tf.LlamaForCausalLM(cfg).to(torch.bfloat16).eval()
    m.requires_grad_(False)
    x = torch.randint(1, 512, (1, 8), device="cuda")
    kw = dict(do_sample=False, max_new_tokens=6, min_new_tokens=6, cache_implementation="static", pad_token_id=0,
              disable_compile=True)
    tm = thunder.compile(m, recipe="hf-transformers", plugins=[MXFP4()])
    out = tm.generate(x, **kw)
    trace = str(thunder.last_traces(tm)[-1])
    assert "hip_mxfp4_decode_linear_group" in trace, trace
    assert any("hip_mxfp4_decode_linear(" in line and "'silu'" in line for line in trace.splitlines()), trace
    # the module is quantized now: compiled again with the pass off it runs the custom op per linear
    monkeypatch.setenv("LTA_MXFP4_DECODE_FUSION", "0")
    tm_off = thunder.compile(m, recipe="hf-transformers", plugins=[MXFP4()])
    ref = tm_off.generate(x, **kw)
    trace_off = str(thunder.last_traces(tm_off)[-1])
    assert "custom_op_lta_mxfp4_linear" in trace_off and "hip_mxfp4_decode_linear" not in trace_off, trace_off
    assert (out == ref).float().mean() > 0.8  # greedy tokens of a random model: bf16 rounding may flip a late one


# ---- CPU: the reference is the unfused composition; the pass leaves CPU programs alone ---------
@pytest.mark.parametrize("M", [1, 3, 8])
@pytest.mark.parametrize("mode", MODES)
def test_reference_equals_unfused_composition_cpu(mode, M):
    from lightning_thunder_amd.ops import mxfp4

    N, K = 130, 96
    o = _operands(N, K, "cpu", torch.float32)
    x = o["x"][:M]
    kw = _mode_kwargs(o, mode, M)
    norm = "norm" in mode
    out = mxfp4.gemv_fused_reference(x, o["q"], o["s"], norm=norm, norm_weight=o["g"] if norm else None, eps=EPS, **kw)
    h = x
    if norm:
        h = x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + EPS) * o["g"]
    y = h @ mxfp4.dequantize(o["q"], o["s"]).T
    if "bias" in kw:
        y = y + kw["bias"]
    if "gate_q" in kw:
        y = torch.nn.functional.silu(y) * (h @ mxfp4.dequantize(o["gq"], o["gs"]).T)
    elif kw.get("act") == "silu":
        y = torch.nn.functional.silu(y)
    if "residual" in kw:
        y = y + kw["residual"]
    assert out.dtype == torch.float32 and out.shape == (M, N)
    torch.testing.assert_close(out, y, atol=1e-5, rtol=0)
    assert not mxfp4.gemv_fused_supported(x, o["q"], o["s"])


def test_pass_leaves_cpu_programs_alone():
    import lightning_thunder_amd as thunder
    from lightning_thunder_amd.executors import hipex
    from lightning_thunder_amd.transforms.mxfp4_inference import MXFP4InferenceTransform

    assert hipex.hip_mxfp4_decode_linear is not None and hipex.hip_mxfp4_decode_linear_group is not None
    torch.manual_seed(4)
    m = torch.nn.Sequential(torch.nn.Linear(256, 512), torch.nn.SiLU(), torch.nn.Linear(512, 256))
    m.requires_grad_(False)
    jm = thunder.jit(m, transforms=[MXFP4InferenceTransform()])
    jm(torch.randn(4, 256))
    trace = str(thunder.last_traces(jm)[-1])
    assert "custom_op_lta_mxfp4_linear" in trace and "hip_mxfp4_decode_linear" not in trace, trace
