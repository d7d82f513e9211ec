"""MXFP4 kernel micro-benchmark: GEMM TF/s (random data), decode GEMV weight bandwidth, and the
fused decode GEMV launches against the unfused chains they replace.

``python scripts/mxfp4_bench.py [OUT.json] [--only gemm|gemv|decode_fusion] [--rows 1,8]``"""
import json
import sys

import torch

from lightning_thunder_amd.ops import mxfp4, fp8


def graph_time(fn, iters=50):
    """Kernel time without the Python launch overhead: `iters` calls captured in one graph."""
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(iters):
            fn()
    g.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def timeit(fn, iters=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3  # us


argv = sys.argv  # options are taken out in place: what is left is [script, OUT.json]
only = None
if "--only" in argv:
    only = argv[argv.index("--only") + 1]
    del argv[argv.index("--only"):argv.index("--only") + 2]
rows = (1, 8)
if "--rows" in argv:
    rows = tuple(int(v) for v in argv[argv.index("--rows") + 1].split(","))
    del argv[argv.index("--rows"):argv.index("--rows") + 2]
res = {"gemm": {}, "gemv": {}, "decode_fusion": {}}
for M, N, K in [(4096, 4096, 4096), (4096, 11008, 4096), (8192, 8192, 8192)] if only in (None, "gemm") else []:
    a = torch.randn(M, K, device="cuda", dtype=torch.bfloat16)
    b = torch.randn(N, K, device="cuda", dtype=torch.bfloat16)
    qa, sa = mxfp4.quantize(a)
    qb, sb = mxfp4.quantize(b)
    us = timeit(lambda: mxfp4.gemm_nt(qa, sa, qb, sb))
    q8a, s8a, _, _ = fp8.mx_quantize(a)
    q8b, s8b, _, _ = fp8.mx_quantize(b)
    us8 = timeit(lambda: fp8.gemm_nt_mx(q8a, s8a, q8b, s8b))
    usb = timeit(lambda: a @ b.T)
    f = 2 * M * N * K
    res["gemm"][f"{M}x{N}x{K}"] = {"mxfp4_us": round(us, 1), "mxfp4_tflops": round(f / us / 1e6),
                                   "mxfp8_tflops": round(f / us8 / 1e6), "bf16_hipblaslt_tflops": round(f / usb / 1e6)}
    print(M, N, K, res["gemm"][f"{M}x{N}x{K}"], flush=True)
for M, N, K in [(1, 2048, 2048), (1, 8192, 2048), (1, 2048, 8192), (1, 128256, 2048),
                (4, 8192, 2048)] if only in (None, "gemv") else []:
    w = torch.randn(N, K, device="cuda", dtype=torch.bfloat16) * 0.02
    x = torch.randn(M, K, device="cuda", dtype=torch.bfloat16)
    q, s = mxfp4.quantize(w)
    us = graph_time(lambda: mxfp4.gemv(x, q, s))
    usb = graph_time(lambda: x @ w.T)
    nbytes = q.numel() + s.numel()
    res["gemv"][f"{M}x{N}x{K}"] = {"mxfp4_us": round(us, 1), "weight_GBps": round(nbytes / us / 1e3),
                                   "bf16_torch_us": round(usb, 1),
                                   "bf16_GBps": round(w.numel() * 2 / usb / 1e3)}
    print(M, N, K, res["gemv"][f"{M}x{N}x{K}"], flush=True)


def decode_fusion(H=4096, I=11008):
    """The four decode sites of a Llama-2-7B layer (hidden H, MLP I): the launches a 4-bit layer ran
    before the fusion against the one fused launch, both captured in a graph.  Every call of a
    captured loop streams another copy of the weights (more copies than the 256 MB MALL holds), as
    a decode step that walks 32 layers does."""
    from lightning_thunder_amd.ops.fused import swiglu_fwd
    from lightning_thunder_amd.ops.rmsnorm import rms_norm_fwd

    def weights(N, K, total_rows):
        copies = max(2, -(-(640 << 20) // (total_rows * K // 2)))
        w = torch.randn(N, K, device="cuda", dtype=torch.bfloat16) * 0.02
        q, s = mxfp4.quantize(w)
        return [(q.clone(), s.clone()) for _ in range(copies)]

    class Rot:  # the next weight copy on every call
        def __init__(self, *lists):
            self.lists, self.i = lists, 0

        def __call__(self):
            self.i += 1
            return [l[self.i % len(l)] for l in self.lists]

    out = res["decode_fusion"]
    for M in rows:
        x = torch.randn(M, H, device="cuda", dtype=torch.bfloat16)
        xi = torch.randn(M, I, device="cuda", dtype=torch.bfloat16)
        r = torch.randn(M, H, device="cuda", dtype=torch.bfloat16)
        g = torch.rand(H, device="cuda", dtype=torch.bfloat16) + 0.5
        sites = {}
        wq, wk, wv = (weights(H, H, 3 * H) for _ in range(3))
        rot = Rot(wq, wk, wv)

        def qkv_unfused():
            xn = rms_norm_fwd(x, g, 1e-5)[0]
            return [mxfp4.gemv(xn, q, s) for q, s in rot()]

        sites["norm+qkv"] = (qkv_unfused, lambda: mxfp4.gemv_group(x, rot(), norm=True, norm_weight=g, eps=1e-5))
        wqkv = weights(3 * H, H, 3 * H)
        rot1 = Rot(wqkv)
        sites["norm+qkv(one weight)"] = (lambda: mxfp4.gemv(rms_norm_fwd(x, g, 1e-5)[0], *rot1()[0]),
                                         lambda: mxfp4.gemv_fused(x, *rot1()[0], norm=True, norm_weight=g, eps=1e-5))
        wo = weights(H, H, H)
        rot2 = Rot(wo)
        sites["o-proj+residual"] = (lambda: mxfp4.gemv(x, *rot2()[0]) + r,
                                    lambda: mxfp4.gemv_fused(x, *rot2()[0], residual=r))
        w1, w3 = weights(I, H, 2 * I), weights(I, H, 2 * I)
        rot3 = Rot(w1, w3)

        def gate_unfused():
            xn = rms_norm_fwd(x, g, 1e-5)[0]
            (q1, s1), (q3, s3) = rot3()
            return swiglu_fwd(mxfp4.gemv(xn, q1, s1), mxfp4.gemv(xn, q3, s3))

        def gate_fused():
            (q1, s1), (q3, s3) = rot3()
            return mxfp4.gemv_fused(x, q1, s1, act="silu", gate_q=q3, gate_s=s3, norm=True, norm_weight=g, eps=1e-5)

        sites["norm+gated pair"] = (gate_unfused, gate_fused)
        sites["qkv (no norm)"] = (lambda: [mxfp4.gemv(x, q, s) for q, s in rot()], lambda: mxfp4.gemv_group(x, rot()))

        def gate_only_unfused():
            (q1, s1), (q3, s3) = rot3()
            return swiglu_fwd(mxfp4.gemv(x, q1, s1), mxfp4.gemv(x, q3, s3))

        def gate_only_fused():
            (q1, s1), (q3, s3) = rot3()
            return mxfp4.gemv_fused(x, q1, s1, act="silu", gate_q=q3, gate_s=s3)

        sites["gated pair (no norm)"] = (gate_only_unfused, gate_only_fused)
        wd = weights(H, I, H)
        rot4 = Rot(wd)
        sites["down-proj+residual"] = (lambda: mxfp4.gemv(xi, *rot4()[0]) + r,
                                       lambda: mxfp4.gemv_fused(xi, *rot4()[0], residual=r))
        for name, (unfused, fused) in sites.items():
            # alternate the two, keep each one's median of 5
            tu, tf = [], []
            for _ in range(5):
                tu.append(graph_time(unfused))
                tf.append(graph_time(fused))
            out[f"M={M} {name}"] = {"unfused_us": round(sorted(tu)[2], 2), "fused_us": round(sorted(tf)[2], 2),
                                    "unfused_runs": [round(v, 2) for v in tu], "fused_runs": [round(v, 2) for v in tf]}
            print(f"M={M} {name}", out[f"M={M} {name}"], flush=True)


if only in (None, "decode_fusion"):
    decode_fusion()
json.dump(res, open(sys.argv[1] if len(sys.argv) > 1 else "gpurun_out/mxfp4_bench.json", "w"), indent=1)
