"""The prefill attention kernel that reads the KV cache by positions (csrc/prefill_attention.hip) against the chain it
replaces, timed as a chain, and ``benchmarks/inference.py`` with the rewrite on and off.

    python scripts/prefill_attn_bench.py [--out profiles/prefill_attn_pos.txt] [--skip-models | --only-models]

Part one, per cell: one layer's prefill attention of T = 2048 query rows at positions ``arange(T)`` against a cache of
capacity S, once as the program the model spells,

    (gather_pages per pool)  ->  (e4m3_values / dequantise_rows)  ->  attn_fwd(..., mask=position_mask / paged_mask)

whose ``attn_fwd`` builds the fp32 mask image (``prepare_mask``) and launches the masked v1 forward over all of S, and
once as the one ``prefill_attn_*`` launch.  The two must be equal bit for bit; that is checked for every cell before it
is timed.  Cells: Llama-3.2-1B (32 / 8 heads, D 64) and Llama-2-7B (32 / 32, D 128), batch 1 and 8, S in {2176, 8192},
the three cache formats, the static cache and a paged one (pages 16 and 64, shuffled table).  Each version's calls are
captured into a hipGraph of ``--batch`` back-to-back calls (device time, no host gaps); the replays of the two versions
alternate, after warm-up, and a point is the median of ``--batches`` replays / batch.  "spread" is max - min of the
chain's replays.  Acceptance: the new launch takes no longer than the chain's median plus its spread; a cell that
misses is listed.

Two rows per (model, batch) for information only: the unmasked causal kernel over ``k[:, :, :T]`` (what a prefill
without a cache runs: v1 through ``lta_attn_fwd_set_impl(0)`` and the default, v4 at D 128), the floor of a position
kernel of v1's structure; and one chunked case, T = 512 at base 1536.

Part two runs ``benchmarks.inference`` (hipgraph mode, Llama-3.2-1B, batch 8, a 2048-token prompt, 64 new tokens,
``--kv-page-size 16``) in a fresh process per row: ``LTA_KV_PREFILL_FUSION=0`` / the default / ``=0`` again per cache
format (the switch leaves the prefill as the chain above; no decode code differs), and one ``--prefill-chunk 512`` row.
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
from scripts.decode_attn_paged_bench import pools_of

BF16 = torch.bfloat16
MODELS = {"Llama-3.2-1B": (32, 8, 64), "Llama-2-7B": (32, 32, 128)}
T = 2048
CAPACITIES = (2176, 8192)
PAGE_SIZES = (16, 64)


def _chain(fmt_, q, ops, mask, table=None, page=None):
    """The unfused program of one layer: gathers, dequantise, mask image + masked v1 forward."""
    from lightning_thunder_amd.ops.attention import attn_fwd
    from lightning_thunder_amd.ops.kv8 import dequantise_rows, e4m3_values
    from lightning_thunder_amd.ops.kv_pages import gather_pages

    def run():
        c = ops if table is None else [gather_pages(p, table, page) for p in ops]
        if fmt_ == "fp8":
            k, v = e4m3_values(c[0], q.dtype), e4m3_values(c[1], q.dtype)
        elif fmt_ == "fp8-row":
            k, v = dequantise_rows(c[0], c[2], q.dtype), dequantise_rows(c[1], c[3], q.dtype)
        else:
            k, v = c
        return attn_fwd(q, k, v, causal=False, mask=mask())[0]

    return run


def part_one(args, lines):
    from lightning_thunder_amd.ops import attention as A
    from lightning_thunder_amd.ops import require
    from lightning_thunder_amd.ops.kv8 import e4m3_bytes, quantise_rows
    from lightning_thunder_amd.ops.kv_pages import paged_mask
    from lightning_thunder_amd.ops.kv_rows import position_mask

    lines.append(f"prefill attention, T = {T} rows at positions arange(T), us per call: median (min..max) of {args.batches} "
                 f"graph replays of {args.batch} calls, versions alternating; spread = max - min of the chain")
    lines.append(f"{'model':<13} {'B':>2} {'S':>5} {'cache':>8} {'layout':>9} | {'replaced chain us':>28} | "
                 f"{'prefill_attn us':>28} | {'spread':>8} | {'new/chain':>9} | new <= chain + spread | bits equal")
    missed = []
    new_fns = {"bf16": (A.prefill_attn_pos, A.prefill_attn_paged), "fp8": (A.prefill_attn_kv8_pos, A.prefill_attn_kv8_paged),
               "fp8-row": (A.prefill_attn_kv8s_pos, A.prefill_attn_kv8s_paged)}
    torch.manual_seed(0)
    for model, (Hq, Hkv, D) in MODELS.items():
        for B in (1, 8):
            q = torch.randn(B, Hq, T, D, device="cuda").to(BF16)
            pos = torch.arange(T, device="cuda").expand(B, T).contiguous()
            for S in CAPACITIES:
                k = torch.randn(B, Hkv, S, D, device="cuda").to(BF16)
                v = torch.randn(B, Hkv, S, D, device="cuda").to(BF16)
                (ks8, ks), (vs8, vs) = quantise_rows(k), quantise_rows(v)
                caches = {"bf16": (k, v), "fp8": (e4m3_bytes(k), e4m3_bytes(v)), "fp8-row": (ks8, vs8, ks, vs)}
                for cache, ops in caches.items():
                    by_pos, by_page = new_fns[cache]
                    layouts = {"static": None}
                    for page in PAGE_SIZES:
                        layouts[f"page {page}"] = page
                    for layout, page in layouts.items():
                        if page is None:
                            versions = {"chain": _chain(cache, q, ops, lambda: position_mask(pos, S)),
                                        "new": lambda: by_pos(q, *ops, pos)}
                        else:
                            P = S // page
                            table = torch.randperm(B * P, device="cuda").view(B, P)
                            pools = pools_of(ops, table, page)
                            versions = {"chain": _chain(cache, q, pools, lambda: paged_mask(pos, table, page, B * P), table, page),
                                        "new": lambda: by_page(q, *pools, pos, table, page, B * P)}
                        same = torch.equal(versions["chain"]().contiguous().view(torch.int16),
                                           versions["new"]().contiguous().view(torch.int16))
                        t = measure(versions, args.batch, args.batches)
                        spread = max(t["chain"]) - min(t["chain"])
                        mc, mn = statistics.median(t["chain"]), statistics.median(t["new"])
                        ok = mn <= mc + spread
                        lines.append(f"{model:<13} {B:>2} {S:>5} {cache:>8} {layout:>9} | {fmt(t['chain']):>28} | "
                                     f"{fmt(t['new']):>28} | {spread:>8.2f} | {mn / mc:>9.3f} | {'yes' if ok else 'NO':>21} | "
                                     f"{'yes' if same else 'NO'}")
                        print(lines[-1], flush=True)
                        if not ok:
                            missed.append(lines[-1])
                        if not same:
                            sys.exit("the prefill kernel's result differs from the chain's: " + lines[-1])
                        if page is not None:
                            del pools, table
                del caches, k, v, ks8, vs8, ks, vs
            # for information: the unmasked causal kernel over the T live keys, and one chunk of 512 rows at base 1536
            k = torch.randn(B, Hkv, T, D, device="cuda").to(BF16)
            v = torch.randn(B, Hkv, T, D, device="cuda").to(BF16)
            lib = require()
            causal = lambda: A.attn_fwd(q, k, v, causal=True)[0]  # noqa: E731
            old = lib.lta_attn_fwd_set_impl(0)
            t1 = measure({"v1": causal}, args.batch, args.batches)["v1"]
            lib.lta_attn_fwd_set_impl(old)
            td = measure({"default": causal}, args.batch, args.batches)["default"]
            tn = measure({"new": lambda: A.prefill_attn_pos(q, k, v, pos)}, args.batch, args.batches)["new"]
            qc, pc = q[:, :, :512].contiguous(), (pos[:, :512] + 1536).contiguous()
            tc = measure({"chunk": lambda: A.prefill_attn_pos(qc, k, v, pc)}, args.batch, args.batches)["chunk"]
            lines.append(f"{model:<13} {B:>2} {T:>5} {'bf16':>8} {'info':>9} | causal v1 {fmt(t1)} | causal default {fmt(td)} | "
                         f"prefill_attn_pos over S = T {fmt(tn)} | chunk T = 512 at base 1536 {fmt(tc)}")
            print(lines[-1], flush=True)
            del k, v, q
    lines.append(f"cells where the new launch is slower than the chain's median + spread: {len(missed)}")
    lines.extend("  " + m for m in missed)


def part_two(args, lines):
    import gc

    gc.collect()
    torch.cuda.empty_cache()
    lines.append("")
    lines.append(f"benchmarks/inference.py, Llama-3.2-1B, batch 8, 2048 in, {args.output_length} out, hipgraph mode, --kv-page-size 16, "
                 f"one fresh process per row, {args.iterations} iterations after {args.warmup} warm-up")
    lines.append(f"{'kv cache':>8} {'prefill':>22} | {'TTFT median ms':>14} | {'TBOT mean':>9} {'median':>7} {'p90':>7} | peak GiB")
    runs = [(kv, label, env, []) for kv in ("model", "fp8", "fp8-row")
            for label, env in (("chain (fusion off)", "0"), ("prefill_attn", "1"), ("chain (fusion off)", "0"))]
    runs.append(("model", "prefill_attn, chunk 512", "1", ["--prefill-chunk", "512"]))
    for kv, label, env, extra in runs:
        cmd = [sys.executable, "-m", "lightning_thunder_amd.benchmarks.inference", "--model", "Llama-3.2-1B",
               "--batch-size", "8", "--input-length", "2048", "--output-length", str(args.output_length),
               "--num-iterations", str(args.iterations), "--warmup-iterations", str(args.warmup), "--modes", "hipgraph",
               "--kv-cache-dtype", kv, "--kv-page-size", "16", *extra]
        p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600,
                           env={**os.environ, "LTA_KV_PREFILL_FUSION": env})
        if p.returncode != 0:
            sys.exit(f"{' '.join(cmd)} failed ({p.returncode}):\n{p.stderr[-4000:]}")
        r = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
        tb = r["tbot_ms"]
        lines.append(f"{kv:>8} {label:>22} | {r['ttft_ms']['median']:>14.2f} | {tb['mean']:>9.3f} {tb['median']:>7.3f} "
                     f"{tb['p90']:>7.3f} | {r['max_memory_allocated_gib']}")
        print(lines[-1], flush=True)
        args.save()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prefill_attn_pos.txt"))
    ap.add_argument("--batch", type=int, default=3)
    ap.add_argument("--batches", type=int, default=21)
    ap.add_argument("--skip-models", action="store_true", help="part one only")
    ap.add_argument("--only-models", action="store_true", help="part two only (appended to --out)")
    ap.add_argument("--output-length", type=int, default=64)
    ap.add_argument("--iterations", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("prefill_attn_bench needs the GPU: a CPU timing says nothing about it")
    lines = [f"prefill attention by positions vs the chain it replaces, {torch.cuda.get_device_name(0)}", ""]
    if args.only_models and os.path.exists(args.out):
        with open(args.out) as f:
            lines = f.read().splitlines()

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")

    args.save = save
    if not args.only_models:
        part_one(args, lines)
        save()
    if not args.skip_models:
        part_two(args, lines)
        save()


if __name__ == "__main__":
    main()
