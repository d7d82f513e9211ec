"""Weight-only e4m3 decode GEMV (csrc/gemv_fp8.hip): kernel against fp64, bounds, groups, refusals, the
compiled decode step under FP8InferenceTransform(activations="bf16"), and the CPU specification."""
import functools

import pytest
import torch
import torch.nn.functional as F

from kernel_checks import BF16, ULP, assert_guard_intact, assert_within, guarded, nan_padded

# the six of test_mxfp4_decode_fusion.py, and the norm without a weight (the kernel's null-g branch)
MODES = ["plain_residual", "bias_silu_residual", "norm", "gated", "norm_gated", "norm_residual", "norm_unweighted"]
# (N, K) against the kernel's tiling.  A wave step is 1024 K-elements; the 4 waves stand 1 / 2 / 4 deep along K for
# K <= 1024 / <= 2048 / above.  A wave owns 4 rows at M > 4; at M = 3, 4 it owns 8; at M <= 2 it owns 16 when the
# launch streams >= 8192 rows, 4 when 8 would make fewer than 256 workgroups, else 8 (with two K-steps per request).
#  (130, 96): K below one wave step (6 live lanes), 4 waves along N, N no multiple of the columns per workgroup;
#  (72, 4112): one 16-byte piece past the 4096-wide workgroup step: a second trip with one live lane in one wave;
#  (1536, 2048): the ordinary case, two waves along K;  (8192, 128): the 16-row instantiation;
#  (2056, 4112): 8 rows at M <= 2 with the two-step request group, its second half one live lane; an N tail;
#  (8200, 4112): 16 rows with 4 waves along K, as the 7B projections run it, an N tail of 8 rows (the row clamp).
SHAPES = [(130, 96), (72, 4112), (1536, 2048), (8192, 128), (2056, 4112), (8200, 4112)]
EPS = 1e-5
SPECIAL = [0x7E, 0xFE, 0x00, 0x80] + list(range(0x01, 0x08)) + list(range(0x81, 0x88))  # +-448, +-0, subnormals


@functools.lru_cache(maxsize=None)
def _operands(N, K, device="cuda", dtype=BF16):
    """One set of operands per shape, shared (and left unchanged) by every case of that shape."""
    from lightning_thunder_amd.transforms.fp8_inference import quantize_weight_e4m3

    gen = torch.Generator(device="cpu").manual_seed(N * 7919 + K)
    randn = lambda *shape: torch.randn(*shape, generator=gen)
    o = dict(x=(randn(8, K) * 3).to(device, dtype), g=(torch.rand(K, generator=gen) + 0.5).to(device, dtype),
             bias=randn(N).to(device, dtype), res=randn(8, N).to(device, dtype))
    for name in ("q", "gq"):
        q, s = quantize_weight_e4m3(randn(N, K) * 0.02)
        q[:, :len(SPECIAL)] = torch.tensor(SPECIAL, dtype=torch.uint8)
        assert not ((q & 0x7F) == 0x7F).any()  # e4m3_bytes makes no NaN of finite input
        o[name], o[name + "_s"] = q.to(device), s.to(device)
    return o


def _mode_kwargs(o, mode, M):
    kw = dict(norm="norm" in mode, norm_weight=o["g"] if "norm" in mode and "unweighted" not in mode else None, eps=EPS)
    if "bias" in mode:
        kw["bias"] = o["bias"]
    if "residual" in mode:
        kw["residual"] = o["res"][:M]
    if "silu" in mode or "gated" in mode:
        kw["act"] = "silu"
    if "gated" in mode:
        kw["gate_q"], kw["gate_scale"] = o["gq"], o["gq_s"]
    return kw


def _formula(x, q, scale, prec, bias=None, residual=None, act=None, gate_q=None, gate_scale=None, norm=False,
             norm_weight=None, eps=EPS):
    """gemv_fused_reference's formula in ``prec`` without the final rounding, and the effect on it of a one-ulp
    flip of each bf16-rounded intermediate (the normalised activations, the two gated products)."""
    deq = lambda b, s: b.view(torch.float8_e4m3fn).to(prec) / s.to(prec)
    xf, w = x.to(prec), deq(q, scale)
    if norm:
        xf = xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)
        xf = (xf if norm_weight is None else xf * norm_weight.to(prec)).to(BF16).to(prec)
    ulp = ULP[BF16]
    v = xf @ w.T
    dv = ulp * (xf.abs() @ w.abs().T) if norm else torch.zeros_like(v)
    if gate_q is None:
        if bias is not None:
            v = v + bias.to(prec)
        sig = torch.sigmoid(v)
        slope = (sig * (1 + v * (1 - sig))).abs() if act == "silu" else 1.0
        v = F.silu(v) if act == "silu" else v
        return (v if residual is None else v + residual.to(prec)), dv * slope
    wg = deq(gate_q, gate_scale)
    a, b = v.to(BF16).to(prec), (xf @ wg.T).to(BF16).to(prec)
    db = ulp * b.abs() + (ulp * (xf.abs() @ wg.abs().T) if norm else 0)
    sig = torch.sigmoid(a)
    slope = (sig * (1 + a * (1 - sig))).abs()
    return F.silu(a) * b, (ulp * a.abs() + dv) * slope * b.abs() + F.silu(a).abs() * db


def _check_against_fp64_and_in_bounds(N, K):
    """Every mode at M = 1, 3, 8 against fp64.  At M = 3 also: the result inside a guarded buffer, x inside a NaN-filled
    one with a longer row stride, the residual with a row stride other than N: nothing outside is written or consumed,
    and the output is the contiguous call's bit for bit (the same kernel in the same order)."""
    from lightning_thunder_amd.ops import fp8_gemv as g8

    o = _operands(N, K)
    for mode in MODES:
        for M in (1, 3, 8):
            x, kw = o["x"][:M], _mode_kwargs(o, mode, M)
            out = g8.gemv_fused(x, o["q"], o["q_s"], **kw)
            assert out.shape == (M, N) and out.dtype == BF16
            ref64, extra = _formula(x, o["q"], o["q_s"], torch.float64, **kw)
            ref32, _ = _formula(x, o["q"], o["q_s"], torch.float32, **kw)
            assert_within(out, ref64, ref32, BF16, "gemv_e4m3", f"{mode} N={N} K={K} M={M}", extra=extra)
            if M != 3:
                continue
            xp = nan_padded(x)
            if "residual" in kw:
                kw["residual"] = nan_padded(kw["residual"])
                assert kw["residual"].stride(0) != N
            assert xp.stride(0) != K
            buf, y = guarded((M, N), "cuda")
            g8.gemv_fused(xp, o["q"], o["q_s"], out=y, **kw)
            assert_guard_intact(buf, (M, N), f"{mode} N={N} K={K}")
            assert torch.equal(y, out), (mode, N, K)


def _check_group_equals_separate_launches():
    """Two and three segments of unequal N (one with 16 rows per wave, 4 waves along K and an N tail), packed and not,
    norm on and off: each output is gemv_fused's bit for bit."""
    from lightning_thunder_amd.ops import fp8_gemv as g8

    o = _operands(8192, 128)
    cases = [(o, ns) for ns in [(256, 64, 64), (130, 96), (8192, 256, 256)]] + [(_operands(8200, 4112), (8200, 130))]
    for o, ns in cases:
        src = [(o["q"], o["q_s"]), (o["gq"], o["gq_s"]), (o["q"].flip(0).contiguous(), o["q_s"] * 2)]
        weights = [(q[:n].contiguous(), s) for (q, s), n in zip(src, ns)]
        for norm in (False, True):
            g = o["g"] if norm else None
            for M in (1, 3, 8):
                x = o["x"][:M]
                # one segment alone may take the 8-row tiling where the group takes 16: a row's sums do not depend on it
                want = [g8.gemv_fused(x, q, s, norm=norm, norm_weight=g, eps=EPS) for q, s in weights]
                for packed in (False, True):
                    outs = g8.gemv_group(x, weights, norm=norm, norm_weight=g, eps=EPS, packed=packed)
                    if packed:
                        assert outs.shape == (M, sum(ns))
                        outs = outs.split(list(ns), dim=1)
                    assert len(outs) == len(ns)
                    assert all(torch.equal(a, b) for a, b in zip(outs, want)), (ns, norm, M, packed)


def _check_unsupported_operands_take_the_reference():
    """9 rows, a misaligned x and K = 24: refused by the support check, gemv_fused and the C entry (-2, nothing
    launched); the operator then computes exactly the reference."""
    from lightning_thunder_amd.executors import hipex
    from lightning_thunder_amd.ops import fp8_gemv as g8
    from lightning_thunder_amd.ops._lib import require, stream_ptr

    N, K = 130, 96
    o = _operands(N, K)
    q, s = o["q"], o["q_s"]
    x9 = torch.cat([o["x"], o["x"][:1]])
    xm = torch.zeros(3, K + 8, device="cuda", dtype=BF16)[:, 4:4 + K]
    xm.copy_(o["x"][:3])
    assert xm.data_ptr() % 16 == 8
    x24, q24 = o["x"][:1, :24].contiguous(), q[:, :24].contiguous()
    y = torch.full((9, N), 7.0, device="cuda", dtype=BF16)
    for x, qq in ((x9, q), (xm, q), (x24, q24)):
        assert not g8.gemv_fused_supported(x, qq, s)
        with pytest.raises(ValueError):
            g8.gemv_fused(x, qq, s)
        rc = require().lta_gemv_e4m3_fused(x.data_ptr(), qq.data_ptr(), s.data_ptr(), None, None, None, 0, EPS, None,
                                           None, y.data_ptr(), x.shape[0], N, x.shape[1], x.stride(0), N, 0, 0,
                                           stream_ptr(y.device))
        assert rc == -2
        kw = dict(bias=o["bias"], act="silu", norm=True, norm_weight=o["g"][:x.shape[1]].clone(), eps=EPS)
        got = hipex._fp8_decode_linear_impl(x, qq, s, **kw)
        assert torch.equal(got, g8.gemv_fused_reference(x, qq, s, **kw))
    torch.cuda.synchronize()
    assert (y == 7).all()  # nothing was launched


def _litgpt():
    from lightning_thunder_amd.models.litgpt import GPT, init_weights

    torch.manual_seed(0)
    m = GPT.from_name("llama3-like", n_layer=2, n_embd=256, n_head=4, head_size=64, intermediate_size=512).to(
        device="cuda", dtype=BF16)
    init_weights(m, std=0.05)
    m.requires_grad_(False)
    m.set_kv_cache(1, 64)
    return m


def _check_decode_fusion_in_litgpt_decode(monkeypatch):
    import lightning_thunder_amd as thunder
    from lightning_thunder_amd.transforms.fp8_inference import FP8InferenceTransform
    from lightning_thunder_amd.transforms.hipgraph import HipGraphTransform

    gen = torch.Generator().manual_seed(1)
    idx, pos = torch.randint(0, 300, (1, 8), generator=gen).cuda(), torch.arange(8, device="cuda")
    toks = [torch.randint(0, 300, (1, 1), generator=gen).cuda() for _ in range(3)]

    def run(transforms):
        jm = thunder.jit(_litgpt(), transforms=transforms)
        jm(idx, pos)
        # clones: a captured program returns the same static buffer from every replay
        outs = [jm(tok, torch.tensor([8 + i], device="cuda")).clone() for i, tok in enumerate(toks)]
        return outs, str(thunder.last_traces(jm)[-1])

    fused, trace = run([FP8InferenceTransform(skip=(), activations="bf16")])
    assert "hip_fp8_decode_linear" in trace and "'silu'" in trace, trace
    assert all(s not in trace for s in ("custom_op_lta_fp8_linear_inference", "hip_swiglu(", "hip_rms_norm_fwd")), trace
    # captured: three consecutive positions replay to the uncaptured fused program's logits
    graphed, _ = run([FP8InferenceTransform(skip=(), activations="bf16"), HipGraphTransform()])
    assert all(torch.equal(a, b) for a, b in zip(fused, graphed))
    # the default W8A8 program is no candidate
    _, trace8 = run([FP8InferenceTransform(skip=())])
    assert "hip_fp8_decode_linear" not in trace8 and "custom_op_lta_fp8_linear_inference" in trace8, trace8
    monkeypatch.setenv("LTA_FP8_DECODE_FUSION", "0")
    unfused, trace_off = run([FP8InferenceTransform(skip=(), activations="bf16")])
    assert "custom_op_lta_fp8_linear_inference" in trace_off and "hip_fp8_decode_linear" not in trace_off, trace_off
    torch.testing.assert_close(fused[0].float(), unfused[0].float(), atol=5e-2, rtol=5e-2)


@pytest.mark.gpu
def test_fp8_decode_gemv_gpu(monkeypatch):
    """One test id for the GPU checks of this file (each a function above; the shapes share their operands)."""
    for N, K in SHAPES:
        _check_against_fp64_and_in_bounds(N, K)
    _check_group_equals_separate_launches()
    _check_unsupported_operands_take_the_reference()
    _check_decode_fusion_in_litgpt_decode(monkeypatch)


# ---- CPU: the reference is the unfused composition; the option; CPU programs keep the custom op ----------------
@pytest.mark.parametrize("mode", MODES)
def test_reference_equals_unfused_composition_cpu(mode):
    from lightning_thunder_amd.ops import fp8_gemv as g8
    from lightning_thunder_amd.transforms.fp8_inference import dequantize_e4m3

    N, K, M = 130, 96, 3
    o = _operands(N, K, "cpu", torch.float32)
    x, kw = o["x"][:M], _mode_kwargs(o, mode, M)
    out = g8.gemv_fused_reference(x, o["q"], o["q_s"], **kw)
    h = x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + EPS) * (1 if kw["norm_weight"] is None else o["g"]) \
        if kw["norm"] else x
    y = h @ dequantize_e4m3(o["q"], o["q_s"], torch.float32).T
    if "bias" in kw:
        y = y + kw["bias"]
    if "gate_q" in kw:
        y = F.silu(y) * (h @ dequantize_e4m3(o["gq"], o["gq_s"], torch.float32).T)
    elif kw.get("act") == "silu":
        y = F.silu(y)
    if "residual" in kw:
        y = y + kw["residual"]
    assert out.dtype == torch.float32 and out.shape == (M, N)
    torch.testing.assert_close(out, y, atol=1e-5, rtol=0)
    assert not g8.gemv_fused_supported(x, o["q"], o["q_s"])


def test_bf16_activations_option_cpu():
    import lightning_thunder_amd as thunder
    from lightning_thunder_amd.transforms.fp8_inference import FP8InferenceTransform, dequantize_e4m3

    with pytest.raises(ValueError):
        FP8InferenceTransform(activations="nope")
    torch.manual_seed(4)
    m = torch.nn.Linear(256, 512)
    m.requires_grad_(False)
    jm = thunder.jit(m, transforms=[FP8InferenceTransform(activations="bf16")])
    x = torch.randn(4, 256)
    out = jm(x)
    trace = str(thunder.last_traces(jm)[-1])
    assert "fp8_linear_inference" in trace and "hip_fp8_decode_linear" not in trace, trace
    torch.testing.assert_close(out, F.linear(x, dequantize_e4m3(m.fp8_weight, m.fp8_scale, torch.float32), m.bias))
