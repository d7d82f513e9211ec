"""The position mode of the decode attention kernels against the mask kernels over the equivalent mask, and
``benchmarks/inference.py`` for a ragged batch against the same batch padded to equal length.

    python scripts/decode_attn_pos_bench.py [--out profiles/decode_attn_pos.txt] [--jsonl profiles/inference_ragged.jsonl]
                                            [--skip-models]

Part one: per shape and cache format (bf16, unscaled e4m3, e4m3 with row scales) one decode step's attention
(T = 1) over a cache of capacity S = 8192 whose sequences are live up to

    full     every sequence at position S - 1,
    2048     every sequence at position 2047,
    ragged   batch 8 only: positions 255, 1389, 2523, ... 8191 (evenly spaced lengths 256 .. 8192),

once by the position kernel (``decode_attn*_pos``, positions [B, 1]) and once by the mask kernel (``decode_attn*``)
with the mask the model would build, ``arange(S) <= pos`` as bool [B, 1, 1, S].  Each version's launches are captured
into a hipGraph of ``--batch`` back-to-back calls (device time, no host gaps); the replays of the two versions
alternate, after warm-up, and a point is the median of ``--batches`` replays / batch.  "spread" is max - min of the
mask kernel over its replays in the same run.  The condition, at full length only:

    position kernel <= mask kernel + spread

At the shorter live lengths the ratio position / mask is reported as measured.

Part two runs ``benchmarks.inference`` (hipgraph mode, Llama-3.2-1B, batch 8) in a fresh process per row: the ragged
batch (``--prompt-lengths``) and the same batch padded to its longest length, for the three cache formats; the JSON
lines go to ``--jsonl``.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from scripts.decode_attn_kv8_bench import fmt, measure

BF16 = torch.bfloat16
MODELS = {"Llama-2-7B": (32, 32, 128), "Llama-3.2-1B": (32, 8, 64)}  # Hq, Hkv, D
S = 8192
RAGGED_PROMPTS = "128,256,384,512,768,1024,1536,2048"


def live_sets(B):
    sets = {"full": [S - 1] * B, "2048": [2047] * B}
    if B == 8:
        sets["ragged"] = [256 + round(i * (S - 256) / 7) - 1 for i in range(8)]
    return sets


def part_one(args, lines):
    from lightning_thunder_amd.ops import attention as A
    from lightning_thunder_amd.ops.kv8 import dequantise_rows, e4m3_bytes, e4m3_values, quantise_rows

    lines.append(f"decode attention, T = 1, capacity S = {S}, us per launch: median (min..max) of {args.batches} graph replays "
                 f"of {args.batch} launches, versions alternating; spread = max - min of the mask kernel")
    lines.append(f"{'model':<13} {'B':>2} {'cache':>8} {'live':>6} | {'mask kernel us':>24} | {'position kernel us':>24} | "
                 f"{'spread':>6} | {'pos/mask':>8} | pos <= mask+spread | max|pos-mask|")
    failed = []
    torch.manual_seed(0)
    for model, (Hq, Hkv, D) in MODELS.items():
        for B in (1, 8):
            k = torch.randn(B, Hkv, S, D, device="cuda").to(BF16)
            v = torch.randn(B, Hkv, S, D, device="cuda").to(BF16)
            q = torch.randn(B, Hq, 1, D, device="cuda").to(BF16)
            k8, v8 = e4m3_bytes(k), e4m3_bytes(v)
            (ks8, ks), (vs8, vs) = quantise_rows(k), quantise_rows(v)
            caches = {"bf16": ((k, v), A.decode_attn, A.decode_attn_pos),
                      "fp8": ((k8, v8), A.decode_attn_kv8, A.decode_attn_kv8_pos),
                      "fp8-row": ((ks8, vs8, ks, vs), A.decode_attn_kv8s, A.decode_attn_kv8s_pos)}
            for cache, (ops, by_mask, by_pos) in caches.items():
                for live, positions in live_sets(B).items():
                    pos = torch.tensor(positions, device="cuda").view(B, 1)
                    mask = (torch.arange(S, device="cuda").view(1, 1, 1, S) <= pos.view(B, 1, 1, 1))
                    versions = {"mask": lambda: by_mask(q, *ops, mask), "pos": lambda: by_pos(q, *ops, pos)}
                    diff = (versions["mask"]().float() - versions["pos"]().float()).abs().max().item()
                    t = measure(versions, args.batch, args.batches)
                    spread = max(t["mask"]) - min(t["mask"])
                    mm, mp = statistics.median(t["mask"]), statistics.median(t["pos"])
                    ok = mp <= mm + spread
                    verdict = ("yes" if ok else "NO") if live == "full" else "n/a"
                    lines.append(f"{model:<13} {B:>2} {cache:>8} {live:>6} | {fmt(t['mask']):>24} | {fmt(t['pos']):>24} | "
                                 f"{spread:>6.2f} | {mp / mm:>8.3f} | {verdict:>18} | {diff:.1e}")
                    print(lines[-1], flush=True)
                    if live == "full" and not ok:
                        failed.append(f"{model} B={B} {cache}")
            del caches, k, v, k8, v8, ks8, vs8
    lines.append("full-length shapes that miss the condition: " + ("; ".join(failed) if failed else "none"))


def part_two(args, lines):
    import gc

    gc.collect()
    torch.cuda.empty_cache()
    longest = max(int(x) for x in RAGGED_PROMPTS.split(","))
    lines.append("")
    lines.append(f"benchmarks/inference.py, Llama-3.2-1B, batch 8, hipgraph mode, one fresh process per row, {args.output_length} "
                 f"out, {args.iterations} iterations after {args.warmup} warm-up: TBOT ms; ragged = --prompt-lengths "
                 f"{RAGGED_PROMPTS}, padded = --input-length {longest}")
    lines.append(f"{'kv cache':>8} {'batch':>7} | {'TBOT mean':>9} {'median':>7} {'p90':>7} | {'TTFT ms':>8}")
    rows = []
    for kv in ("model", "fp8", "fp8-row"):
        for batch, extra in (("ragged", ["--prompt-lengths", RAGGED_PROMPTS]), ("padded", ["--input-length", str(longest)])):
            cmd = [sys.executable, "-m", "lightning_thunder_amd.benchmarks.inference", "--model", "Llama-3.2-1B",
                   "--batch-size", "8", "--output-length", str(args.output_length), "--num-iterations", str(args.iterations),
                   "--warmup-iterations", str(args.warmup), "--modes", "hipgraph", "--kv-cache-dtype", kv, *extra]
            p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
            if p.returncode != 0:
                sys.exit(f"{' '.join(cmd)} failed ({p.returncode}):\n{p.stderr[-4000:]}")
            r = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
            r["batch"] = batch
            rows.append(r)
            tb = r["tbot_ms"]
            lines.append(f"{kv:>8} {batch:>7} | {tb['mean']:>9.3f} {tb['median']:>7.3f} {tb['p90']:>7.3f} | "
                         f"{r['ttft_ms']['median']:>8.2f}")
            print(lines[-1], flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(args.jsonl)), exist_ok=True)
            with open(args.jsonl, "w") as f:
                f.write("".join(json.dumps(x) + "\n" for x in rows))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_attn_pos.txt"))
    ap.add_argument("--jsonl", default=os.path.join(ROOT, "profiles", "inference_ragged.jsonl"))
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--batches", type=int, default=21)
    ap.add_argument("--skip-models", action="store_true", help="part one only")
    ap.add_argument("--output-length", type=int, default=64)
    ap.add_argument("--iterations", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("decode_attn_pos_bench needs the GPU: a CPU timing says nothing about it")
    lines = [f"decode attention from per-sequence positions vs from the mask, {torch.cuda.get_device_name(0)}", ""]

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")

    part_one(args, lines)
    save()
    if not args.skip_models:
        part_two(args, lines)
        save()
    print("\n".join(lines))


if __name__ == "__main__":
    main()
