"""The scaled e4m3 KV cache (one power-of-two scale byte per row) against the bf16 cache and the unscaled e4m3
cache: the decode attention kernel, the cache-writing RoPE launch, and ``benchmarks/inference.py`` with
``--kv-cache-dtype fp8-row``.

    python scripts/decode_attn_kv8s_bench.py [--out profiles/decode_attn_kv8_scaled.txt] [--skip-models | --skip-kernels] [--note TEXT]

Measured as ``scripts/decode_attn_kv8_bench.py`` measures (its helpers are used): per shape one decode step's
attention (T = 1, the model's all-true mask row) over the three caches of the same logical content, each
version's launches captured into a hipGraph of ``--batch`` back-to-back calls (device time, no host gaps), the
replays of the versions alternating after warm-up, a point the median of ``--batches`` replays / batch.
"spread" is max - min of the bf16 kernel over its replays in the same run: the margin of the condition

    scaled kernel <= bf16 kernel + spread

at every shape (a cache that costs time against 16 bits cannot be turned on).  The ratio to the unscaled
kernel is what the two scale-byte loads and two multiplies per key cost; it is reported, not bounded.
The RoPE launch is timed the same way for the three cache types at Llama-2-7B, batch 1.

``--note`` is appended to the output verbatim (the outcome of comparing the existing kernels' instruction
streams with the parent commit's, which decides whether the parent's kernels need measuring at all).
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch

from decode_attn_kv8_bench import MODELS, fmt, measure

BF16, U8, F8 = torch.bfloat16, torch.uint8, torch.float8_e4m3fn


def part_one(args, lines):
    from lightning_thunder_amd.ops.attention import decode_attn, decode_attn_kv8, decode_attn_kv8s
    from lightning_thunder_amd.ops.fused import qkv_rope_cache_fwd
    from lightning_thunder_amd.ops.kv8 import dequantise_rows, quantise_rows

    lines.append(f"decode attention, T = 1, us per launch: median (min..max) of {args.batches} graph replays of {args.batch} "
                 "launches, versions alternating; spread = max - min of 'bf16'")
    lines.append(f"{'model':<13} {'B':>2} {'S':>5} | {'bf16 us':>24} | {'e4m3 us':>24} | {'scaled e4m3 us':>24} | {'spread':>6} | "
                 "scaled <= bf16+spread | scaled/bf16 | scaled/e4m3 | bits == bf16 kernel over dequantised")
    failed = []
    torch.manual_seed(0)
    for model, (Hq, Hkv, D) in MODELS.items():
        for B in (1, 8):
            for S in (2048, 8192):
                x = torch.randn(B, Hkv, S, D, device="cuda")
                y = torch.randn(B, Hkv, S, D, device="cuda")
                k8, v8 = (t.clamp(-448, 448).to(F8).view(U8) for t in (x, y))
                k, v = k8.view(F8).to(BF16), v8.view(F8).to(BF16)
                (k8s, ks), (v8s, vs) = quantise_rows(x.to(BF16)), quantise_rows(y.to(BF16))
                q = torch.randn(B, Hq, 1, D, device="cuda").to(BF16)
                mask = torch.ones(1, 1, 1, S, dtype=torch.bool, device="cuda")
                versions = {"bf16": lambda: decode_attn(q, k, v, mask), "e4m3": lambda: decode_attn_kv8(q, k8, v8, mask),
                            "scaled": lambda: decode_attn_kv8s(q, k8s, v8s, ks, vs, mask)}
                same = torch.equal(versions["scaled"](), decode_attn(q, dequantise_rows(k8s, ks, BF16),
                                                                     dequantise_rows(v8s, vs, BF16), mask))
                t = measure(versions, args.batch, args.batches)
                spread = max(t["bf16"]) - min(t["bf16"])
                m16, m8, ms = (statistics.median(t[n]) for n in ("bf16", "e4m3", "scaled"))
                ok = ms <= m16 + spread
                lines.append(f"{model:<13} {B:>2} {S:>5} | {fmt(t['bf16']):>24} | {fmt(t['e4m3']):>24} | {fmt(t['scaled']):>24} | "
                             f"{spread:>6.2f} | {'yes' if ok else 'NO':>21} | {ms / m16:>11.3f} | {ms / m8:>11.3f} | "
                             f"{'yes' if same else 'NO'}")
                print(lines[-1], flush=True)
                if not ok:
                    failed.append(f"{model} B={B} S={S}")
    lines.append("shapes that miss the condition: " + ("; ".join(failed) if failed else "none"))
    lines.append("")
    lines.append("cache-writing RoPE launch (qkv split + RoPE + K/V rows into the cache), Llama-2-7B, batch 1, T = 1, "
                 "position 2047 of 2048, us per launch")
    Hq, Hkv, D = MODELS["Llama-2-7B"]
    qkv = torch.randn(1, 1, (Hq + 2 * Hkv) * D, device="cuda").to(BF16)
    cos, sin = torch.rand(1, D, device="cuda"), torch.rand(1, D, device="cuda")
    pos = torch.tensor([2047], device="cuda")
    c16 = [torch.zeros(1, Hkv, 2048, D, device="cuda", dtype=BF16) for _ in range(2)]
    c8 = [torch.zeros(1, Hkv, 2048, D, device="cuda", dtype=U8) for _ in range(2)]
    c8s = [torch.zeros(1, Hkv, 2048, D, device="cuda", dtype=U8) for _ in range(2)]
    sc = [torch.full((1, Hkv, 2048, 1), 127, device="cuda", dtype=U8) for _ in range(2)]
    t = measure({"bf16": lambda: qkv_rope_cache_fwd(qkv, cos, sin, Hq, Hkv, D, D, *c16, pos),
                 "e4m3": lambda: qkv_rope_cache_fwd(qkv, cos, sin, Hq, Hkv, D, D, *c8, pos),
                 "scaled": lambda: qkv_rope_cache_fwd(qkv, cos, sin, Hq, Hkv, D, D, *c8s, pos, k_scale=sc[0], v_scale=sc[1])},
                args.batch, args.batches)
    k8, ks = quantise_rows(c16[0][:, :, 2047])
    assert torch.equal(c8s[0][:, :, 2047], k8) and torch.equal(sc[0][:, :, 2047], ks)
    lines.append(f"{'bf16 cache':>24} | {'e4m3 cache':>24} | {'scaled e4m3 cache':>24}")
    lines.append(f"{fmt(t['bf16']):>24} | {fmt(t['e4m3']):>24} | {fmt(t['scaled']):>24}")
    print(lines[-1], flush=True)


def part_two(args, lines):
    import gc
    import json
    import subprocess

    gc.collect()
    torch.cuda.empty_cache()
    lines.append("")
    lines.append(f"benchmarks/inference.py, hipgraph mode, one fresh process per row, {args.input_length} in / "
                 f"{args.output_length} out, {args.iterations} iterations after {args.warmup} warm-up: TBOT ms mean / median / "
                 "p90, TTFT ms median, GiB of the KV cache buffers (scale buffers included)")
    lines.append(f"{'model':<14} {'B':>2} {'kv cache':>8} | {'TBOT mean':>9} {'median':>7} {'p90':>7} | {'TTFT ms':>8} | {'cache GiB':>9}")
    for model, B in (("Llama-2-7b-hf", 1), ("Llama-3.2-1B", 8)):
        for kv in args.kv:
            cmd = [sys.executable, "-m", "lightning_thunder_amd.benchmarks.inference", "--model", model, "--batch-size", str(B),
                   "--input-length", str(args.input_length), "--output-length", str(args.output_length),
                   "--num-iterations", str(args.iterations), "--warmup-iterations", str(args.warmup), "--modes", "hipgraph",
                   "--kv-cache-dtype", kv]
            p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
            if p.returncode != 0:
                sys.exit(f"{' '.join(cmd)} failed ({p.returncode}):\n{p.stderr[-4000:]}")
            r = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
            tb = r["tbot_ms"]
            lines.append(f"{model:<14} {B:>2} {kv:>8} | {tb['mean']:>9.3f} {tb['median']:>7.3f} {tb['p90']:>7.3f} | "
                         f"{r['ttft_ms']['median']:>8.2f} | {r['kv_cache_gib']:>9.3f}")
            print(lines[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_attn_kv8_scaled.txt"))
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--batches", type=int, default=21)
    ap.add_argument("--skip-models", action="store_true", help="part one only")
    ap.add_argument("--skip-kernels", action="store_true", help="part two only")
    ap.add_argument("--kv", nargs="+", default=["model", "fp8", "fp8-row"], help="the cache types of part two")
    ap.add_argument("--input-length", type=int, default=2048)
    ap.add_argument("--output-length", type=int, default=64)
    ap.add_argument("--iterations", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--note", default=None, help="text appended to the output (instruction-stream comparison)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("decode_attn_kv8s_bench needs the GPU: a CPU timing says nothing about it")
    lines = [f"scaled e4m3 KV cache vs bf16 and unscaled e4m3, {torch.cuda.get_device_name(0)}", ""]

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines + (["", args.note] if args.note else [])) + "\n")

    if not args.skip_kernels:
        part_one(args, lines)
        save()
    if not args.skip_models:
        part_two(args, lines)
        save()
    print("\n".join(lines))


if __name__ == "__main__":
    main()
