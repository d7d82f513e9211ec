"""e4m3 weight-only decode GEMV (csrc/gemv_fp8.hip) against the bf16 GEMV and the padded W8A8 path, and the
norm-prologue A/B behind hipex's _FP8_NORM_MAX_ROWS.

Device time per launch inside hipGraph replays (20 calls per graph, each on the next copy of the weight: more
copies than the MALL holds), median of 21, the versions alternating in one process; the bf16 GEMV is timed
twice per round and the difference of its two medians is the spread of a repeated identical run.

``python scripts/gemv_fp8_bench.py [--out profiles/gemv_fp8.txt] [--fusion-out profiles/fp8_decode_fusion.txt]``"""
import argparse
import statistics

import torch

from lightning_thunder_amd.ops import fp8_gemv as g8
from lightning_thunder_amd.ops.gemm import gemv_nt
from lightning_thunder_amd.ops.rmsnorm import rms_norm_fwd
from lightning_thunder_amd.transforms.fp8_inference import fp8_linear_inference, quantize_weight_e4m3

CALLS, ROUNDS = 20, 21
SHAPES = [("Llama-2-7B qkv", 12288, 4096, False), ("Llama-2-7B o-proj", 4096, 4096, False),
          ("Llama-2-7B gated", 11008, 4096, True), ("Llama-2-7B down", 4096, 11008, False),
          ("Llama-3.2-1B qkv", 3072, 2048, False), ("Llama-3.2-1B o-proj", 2048, 2048, False),
          ("Llama-3.2-1B gated", 8192, 2048, True), ("Llama-3.2-1B down", 2048, 8192, False)]


def graph_us(fn):
    """One graph of CALLS calls, device time per call (us) of its second replay."""
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(CALLS):
            fn()
    g.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / CALLS * 1e3


def medians(versions):
    """{name: fn} -> {name: median us}, every round running each version once, in order."""
    graphs = {k: [] for k in versions}
    for _ in range(ROUNDS):
        for k, fn in versions.items():
            graphs[k].append(graph_us(fn))
    return {k: statistics.median(v) for k, v in graphs.items()}


class Rot:
    """The next of ``copies`` clones of some tensors on every call."""

    def __init__(self, tensors, nbytes):
        n = max(2, -(-(640 << 20) // nbytes))
        self.items, self.i = [[t.clone() for t in tensors] for _ in range(n)], 0

    def __call__(self):
        self.i += 1
        return self.items[self.i % len(self.items)]


def operands(N, K, gated):
    ws = [torch.randn(N, K, device="cuda", dtype=torch.bfloat16) * 0.02 for _ in range(2 if gated else 1)]
    qs = [quantize_weight_e4m3(w) for w in ws]
    scales = [s for _, s in qs]
    return Rot(ws, N * K * 2 * len(ws)), Rot([q for q, _ in qs], N * K * len(ws)), scales


def kernel_table(out):
    lines = ["shape                 N      K     M   e4m3_us  bf16_us  bf16_again_us  w8a8_us   e4m3_GB/s  bf16_GB/s"]
    for name, N, K, gated in SHAPES:
        rot16, rot8, sc = operands(N, K, gated)
        for M in (1, 8):
            x = torch.randn(M, K, device="cuda", dtype=torch.bfloat16)
            if gated:
                e4 = lambda: (lambda q: g8.gemv_fused(x, q[0], sc[0], act="silu", gate_q=q[1], gate_scale=sc[1]))(rot8())
                bf = lambda: (lambda w: gemv_nt(x, w[0], act="silu", gate_weight=w[1]))(rot16())
                w8 = lambda: (lambda q: torch.nn.functional.silu(fp8_linear_inference(x, q[0], sc[0]))
                              * fp8_linear_inference(x, q[1], sc[1]))(rot8())
            else:
                e4 = lambda: g8.gemv_fused(x, rot8()[0], sc[0])
                bf = lambda: gemv_nt(x, rot16()[0])
                w8 = lambda: fp8_linear_inference(x, rot8()[0], sc[0])
            t = medians({"e4m3": e4, "bf16": bf, "bf16_again": bf, "w8a8": w8})
            nb = N * K * (2 if gated else 1)
            lines.append(f"{name:<20} {N:>6} {K:>6} {M:>3} {t['e4m3']:>9.2f} {t['bf16']:>8.2f} {t['bf16_again']:>14.2f} "
                         f"{t['w8a8']:>8.2f} {nb / t['e4m3'] / 1e3:>11.0f} {2 * nb / t['bf16'] / 1e3:>10.0f}")
            print(lines[-1], flush=True)
    open(out, "w").write(__doc__.split("``python")[0] + "\n" + "\n".join(lines) + "\n")


def fusion_table(out):
    """Folded norm prologue against rms_norm_fwd + the launch, Llama-2-7B qkv (one 12288 x 4096 weight, as LitGPT's
    fused qkv linear holds it; gemv_fused, not the three-way group) and gated pair."""
    H, I, eps = 4096, 11008, 1e-5
    g = torch.rand(H, device="cuda", dtype=torch.bfloat16) + 0.5
    _, rq, sq = operands(3 * H, H, False)
    _, rg, sg = operands(I, H, True)
    lines = ["site        M   norm+launch_us  folded_us  folded_again_us"]
    for M in (1, 2, 8):
        x = torch.randn(M, H, device="cuda", dtype=torch.bfloat16)
        sites = {
            "qkv": (lambda: g8.gemv_fused(rms_norm_fwd(x, g, eps)[0], rq()[0], sq[0]),
                    lambda: g8.gemv_fused(x, rq()[0], sq[0], norm=True, norm_weight=g, eps=eps)),
            "gated": (lambda: (lambda q: g8.gemv_fused(rms_norm_fwd(x, g, eps)[0], q[0], sg[0], act="silu", gate_q=q[1],
                                                        gate_scale=sg[1]))(rg()),
                      lambda: (lambda q: g8.gemv_fused(x, q[0], sg[0], act="silu", gate_q=q[1], gate_scale=sg[1],
                                                        norm=True, norm_weight=g, eps=eps))(rg())),
        }
        for name, (unfused, folded) in sites.items():
            t = medians({"unfused": unfused, "folded": folded, "folded_again": folded})
            lines.append(f"{name:<10} {M:>2} {t['unfused']:>16.2f} {t['folded']:>10.2f} {t['folded_again']:>16.2f}")
            print(lines[-1], flush=True)
    open(out, "w").write(fusion_table.__doc__ + "\nMedian of 21 graphs of 20 launches each, device us per launch; the two "
                         "folded columns are the same launch timed twice per round (run-to-run spread).\n\n"
                         + "\n".join(lines) + "\n")


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("--out", default="profiles/gemv_fp8.txt")
    p.add_argument("--fusion-out", default="profiles/fp8_decode_fusion.txt")
    p.add_argument("--only", choices=("kernel", "fusion"), default=None)
    a = p.parse_args()
    if a.only in (None, "fusion"):
        fusion_table(a.fusion_out)
    if a.only in (None, "kernel"):
        kernel_table(a.out)
