"""The paged mode of the decode attention kernels against the position kernels over the equivalent contiguous cache,
and ``benchmarks/inference.py`` for a ragged batch on a paged cache against the same batch on the static one.

    python scripts/decode_attn_paged_bench.py [--out profiles/decode_attn_paged.txt] [--jsonl profiles/inference_paged.jsonl]
                                              [--skip-models | --only-models]

Part one: per shape and cache format (bf16, unscaled e4m3, e4m3 with row scales) one decode step's attention
(T = 1) over a cache of capacity S = 8192 whose sequences are live up to

    full     every sequence at position S - 1,
    2048     every sequence at position 2047,
    ragged   batch 8 only: positions 255, 1389, 2523, ... 8191 (evenly spaced lengths 256 .. 8192),

once by the position kernel (``decode_attn*_pos``) over the contiguous cache ``[B, Hkv, S, D]`` and once by the paged
kernel (``decode_attn*_paged``) over pools that hold the same rows, for page sizes 16, 64 and 256 and two block tables:
the identity (sequence b's pages in order, one after the other) and a random permutation of all pages.  The two
kernels compute the same sums in the same order, so their results must be equal bit for bit; that is checked for
every cell before it is timed.  Each version's launches are captured into a hipGraph of ``--batch`` back-to-back calls
(device time, no host gaps); the replays of the two versions alternate, after warm-up, and a point is the median of
``--batches`` replays / batch.  "spread" is max - min of the position kernel over its replays in the same cell.  No
ratio is fixed in advance: paged / position is reported per cell, and a cell is marked when the paged median lies
outside the position kernel's median +- spread.

Part two runs ``benchmarks.inference`` (hipgraph mode, Llama-3.2-1B, batch 8, ``--prompt-lengths`` 128 .. 2048) in a
fresh process per row: the static cache and a paged cache of page size 64 with exactly the pages the run needs, for
the three cache formats; the JSON lines go to ``--jsonl``.
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
from scripts.decode_attn_pos_bench import MODELS, RAGGED_PROMPTS, S, live_sets

BF16 = torch.bfloat16
PAGE_SIZES = (16, 64, 256)
MODEL_PAGE = 64


def pools_of(caches, table, page):
    """Pools ``[Hkv, R + 1, d]`` that hold the rows of the contiguous ``caches`` ``[B, Hkv, S, d]`` at the slots the
    table gives them (every page of every sequence is allocated: R = B * S)."""
    from lightning_thunder_amd.ops.kv_pages import page_slots

    B, Hkv, S_, _ = caches[0].shape
    R = B * S_
    every = torch.arange(S_, device=table.device).expand(B, S_)
    slots = page_slots(table, every, page, R).reshape(-1)
    out = []
    for c in caches:
        pool = torch.zeros(Hkv, R + 1, c.shape[3], device=c.device, dtype=c.dtype)
        pool.index_copy_(1, slots, c.permute(1, 0, 2, 3).reshape(Hkv, R, c.shape[3]))
        out.append(pool)
    return out


def part_one(args, lines):
    from lightning_thunder_amd.ops import attention as A
    from lightning_thunder_amd.ops.kv8 import e4m3_bytes, quantise_rows

    lines.append(f"decode attention, T = 1, capacity S = {S}, us per launch: median (min..max) of {args.batches} graph replays "
                 f"of {args.batch} launches, versions alternating; spread = max - min of the position kernel in the cell")
    lines.append(f"{'model':<13} {'B':>2} {'cache':>8} {'live':>6} {'page':>4} {'table':>8} | {'position kernel us':>24} | "
                 f"{'paged kernel us':>24} | {'spread':>6} | {'paged/pos':>9} | outside pos +- spread | bits equal")
    outside = []
    torch.manual_seed(0)
    for model, (Hq, Hkv, D) in MODELS.items():
        for B in (1, 8):
            k = torch.randn(B, Hkv, S, D, device="cuda").to(BF16)
            v = torch.randn(B, Hkv, S, D, device="cuda").to(BF16)
            q = torch.randn(B, Hq, 1, D, device="cuda").to(BF16)
            k8, v8 = e4m3_bytes(k), e4m3_bytes(v)
            (ks8, ks), (vs8, vs) = quantise_rows(k), quantise_rows(v)
            caches = {"bf16": ((k, v), A.decode_attn_pos, A.decode_attn_paged),
                      "fp8": ((k8, v8), A.decode_attn_kv8_pos, A.decode_attn_kv8_paged),
                      "fp8-row": ((ks8, vs8, ks, vs), A.decode_attn_kv8s_pos, A.decode_attn_kv8s_paged)}
            for cache, (ops, by_pos, by_page) in caches.items():
                for page in PAGE_SIZES:
                    P = S // page
                    tables = {"identity": torch.arange(B * P, device="cuda").view(B, P),
                              "shuffled": torch.randperm(B * P, device="cuda").view(B, P)}
                    for tname, table in tables.items():
                        pools = pools_of(ops, table, page)
                        for live, positions in live_sets(B).items():
                            pos = torch.tensor(positions, device="cuda").view(B, 1)
                            versions = {"pos": lambda: by_pos(q, *ops, pos),
                                        "paged": lambda: by_page(q, *pools, pos, table, page, B * P)}
                            same = torch.equal(versions["pos"]().view(torch.int16), versions["paged"]().view(torch.int16))
                            t = measure(versions, args.batch, args.batches)
                            spread = max(t["pos"]) - min(t["pos"])
                            mp, mg = statistics.median(t["pos"]), statistics.median(t["paged"])
                            out = abs(mg - mp) > spread
                            lines.append(f"{model:<13} {B:>2} {cache:>8} {live:>6} {page:>4} {tname:>8} | {fmt(t['pos']):>24} | "
                                         f"{fmt(t['paged']):>24} | {spread:>6.2f} | {mg / mp:>9.3f} | "
                                         f"{('slower' if mg > mp else 'faster') if out else 'no':>21} | {'yes' if same else 'NO'}")
                            print(lines[-1], flush=True)
                            if out:
                                outside.append((mg / mp, f"{model} B={B} {cache} {live} page {page} {tname}"))
                            if not same:
                                sys.exit("the paged kernel's result differs from the position kernel's: " + lines[-1])
                        del pools
            del caches, k, v, k8, v8, ks8, vs8
    lines.append(f"cells outside the position kernel's spread: {len(outside)}")
    for ratio, cell in sorted(outside, reverse=True):
        lines.append(f"  {ratio:.3f}  {cell}")


def part_two(args, lines):
    import gc

    gc.collect()
    torch.cuda.empty_cache()
    lengths = [int(x) for x in RAGGED_PROMPTS.split(",")]
    pages = sum(-(-(n + args.output_length - 1) // MODEL_PAGE) for n in lengths)
    lines.append("")
    lines.append(f"benchmarks/inference.py, Llama-3.2-1B, batch 8, hipgraph mode, one fresh process per row, {args.output_length} "
                 f"out, {args.iterations} iterations after {args.warmup} warm-up, --prompt-lengths {RAGGED_PROMPTS}: static "
                 f"cache vs --kv-page-size {MODEL_PAGE} --kv-num-pages {pages} (what the run needs)")
    lines.append(f"{'kv cache':>8} {'layout':>7} | {'TBOT mean':>9} {'median':>7} {'p90':>7} | {'TTFT ms':>8} | {'KV GiB':>7} | "
                 f"pages in use")
    rows = []
    for kv in ("model", "fp8", "fp8-row"):
        for layout, extra in (("static", []), ("paged", ["--kv-page-size", str(MODEL_PAGE), "--kv-num-pages", str(pages)])):
            cmd = [sys.executable, "-m", "lightning_thunder_amd.benchmarks.inference", "--model", "Llama-3.2-1B",
                   "--batch-size", "8", "--output-length", str(args.output_length), "--num-iterations", str(args.iterations),
                   "--warmup-iterations", str(args.warmup), "--modes", "hipgraph", "--kv-cache-dtype", kv,
                   "--prompt-lengths", RAGGED_PROMPTS, *extra]
            p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
            if p.returncode != 0:
                sys.exit(f"{' '.join(cmd)} failed ({p.returncode}):\n{p.stderr[-4000:]}")
            r = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
            r["layout"] = layout
            rows.append(r)
            tb = r["tbot_ms"]
            lines.append(f"{kv:>8} {layout:>7} | {tb['mean']:>9.3f} {tb['median']:>7.3f} {tb['p90']:>7.3f} | "
                         f"{r['ttft_ms']['median']:>8.2f} | {r['kv_cache_gib']:>7.3f} | {r.get('kv_pages_in_use')}")
            print(lines[-1], flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(args.jsonl)), exist_ok=True)
            with open(args.jsonl, "w") as f:
                f.write("".join(json.dumps(x) + "\n" for x in rows))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_attn_paged.txt"))
    ap.add_argument("--jsonl", default=os.path.join(ROOT, "profiles", "inference_paged.jsonl"))
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--batches", type=int, default=21)
    ap.add_argument("--skip-models", action="store_true", help="part one only")
    ap.add_argument("--only-models", action="store_true", help="part two only")
    ap.add_argument("--output-length", type=int, default=64)
    ap.add_argument("--iterations", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("decode_attn_paged_bench needs the GPU: a CPU timing says nothing about it")
    lines = [f"decode attention over a paged KV cache vs over the contiguous one, {torch.cuda.get_device_name(0)}", ""]

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")

    if not args.only_models:
        part_one(args, lines)
        save()
    if not args.skip_models:
        part_two(args, lines)
        save()
    print("\n".join(lines))


if __name__ == "__main__":
    main()
