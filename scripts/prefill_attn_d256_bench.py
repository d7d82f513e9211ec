"""The head-dim-256 prefill kernel (csrc/prefill_attention_d256.hip) against the chain it replaces, timed as a chain.

    python scripts/prefill_attn_d256_bench.py [--out profiles/prefill_attn_d256.txt] [--models Gemma-2b] [--batches-of 1]

The method is ``scripts/prefill_attn_bench.py``'s part one: per cell one layer's prefill attention of T = 2048 query
rows at positions ``arange(T)`` against a cache of capacity S, once as the program the model spells without the kernel,

    (gather_pages per pool)  ->  (e4m3_values / dequantise_rows)  ->  attn_fwd(..., mask=position_mask / paged_mask)

(the fp32 mask image plus the masked v1 forward in its 32-key-tile D = 256 build over all of S), once as the one
``prefill_attn_*`` launch.  Cells: Gemma-2b (8 heads on 1 KV head) and Gemma-7b (16 on 16), batch 1 and 8, S in {2176,
8192}, the three cache formats, the static cache and a paged one (pages 16 and 64, shuffled table); and one windowed
chunk per (model, batch, format, static / page 16): 512 rows at base S - 512 of S = 8192 under W = 4096, against the
same chain under ``window_mask`` / ``paged_window_mask``.  Each version is captured into a hipGraph of ``--batch``
back-to-back calls (device time, no host gaps); the replays of the two versions alternate after warm-up, and a point
is the median of ``--batches`` replays / batch.  "spread" is max - min of the chain's replays.  Acceptance: the new
launch takes no longer than the chain's median plus its spread; a cell that misses is listed, not tuned away.

The kernel defers the rescale of O, so it does not give the chain's bits: the column ``max |new - chain|`` is there to
show that both compute the same thing (a cell beyond 2^-6 max |chain| stops the run).

One row per (model, batch) for information: the bf16 static form at S = T against the causal ring kernel of
csrc/attention_fwd_d256.hip at the same shape (``attn_fwd(causal=True)``), the ceiling of this structure; the gap is the
price of staging through registers."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from scripts.decode_attn_kv8_bench import fmt, measure
from scripts.decode_attn_paged_bench import pools_of
from scripts.prefill_attn_bench import _chain

BF16 = torch.bfloat16
MODELS = {"Gemma-2b": (8, 1, 256), "Gemma-7b": (16, 16, 256)}
T = 2048
CAPACITIES = (2176, 8192)
PAGE_SIZES = (16, 64)
CHUNK, WINDOW = 512, 4096


def _cell(lines, missed, args, head, versions):
    """Checks, times and reports one cell: ``versions`` = {"chain": fn, "new": fn}."""
    ref, out = versions["chain"]().float(), versions["new"]().float()
    diff, scale = (ref - out).abs().max().item(), ref.abs().max().item()
    t = measure(versions, args.batch, args.batches)
    spread = max(t["chain"]) - min(t["chain"])
    mc, mn = statistics.median(t["chain"]), statistics.median(t["new"])
    ok = mn <= mc + spread
    lines.append(f"{head} | {fmt(t['chain']):>30} | {fmt(t['new']):>28} | {spread:>8.2f} | {mn / mc:>9.3f} | "
                 f"{'yes' if ok else 'NO':>21} | {diff:.2e}")
    print(lines[-1], flush=True)
    args.save()
    if not ok:
        missed.append(lines[-1])
    if not diff <= scale / 64:
        sys.exit("the prefill kernel's result is not the chain's: " + lines[-1])


def run(args, lines):
    from lightning_thunder_amd.ops import attention as A
    from lightning_thunder_amd.ops.kv8 import e4m3_bytes, quantise_rows
    from lightning_thunder_amd.ops.kv_pages import paged_mask, paged_window_mask
    from lightning_thunder_amd.ops.kv_rows import position_mask, window_mask

    lines.append(f"prefill attention at head dim 256, T = {T} rows at positions arange(T) (window rows: {CHUNK} rows at base "
                 f"S - {CHUNK}, W = {WINDOW}), us per call: median (min..max) of {args.batches} graph replays of {args.batch} "
                 f"calls, versions alternating; spread = max - min of the chain")
    lines.append(f"{'model':<9} {'B':>2} {'S':>5} {'cache':>8} {'layout':>9} {'rows':>6} | {'replaced chain us':>30} | "
                 f"{'prefill_attn us':>28} | {'spread':>8} | {'new/chain':>9} | new <= chain + spread | max |new - chain|")
    missed = []
    new_fns = {"bf16": (A.prefill_attn_pos, A.prefill_attn_paged), "fp8": (A.prefill_attn_kv8_pos, A.prefill_attn_kv8_paged),
               "fp8-row": (A.prefill_attn_kv8s_pos, A.prefill_attn_kv8s_paged)}
    torch.manual_seed(0)
    for model in args.models:
        Hq, Hkv, D = MODELS[model]
        for B in args.batches_of:
            q = torch.randn(B, Hq, T, D, device="cuda").to(BF16)
            pos = torch.arange(T, device="cuda").expand(B, T).contiguous()
            for S in CAPACITIES:
                k = torch.randn(B, Hkv, S, D, device="cuda").to(BF16)
                v = torch.randn(B, Hkv, S, D, device="cuda").to(BF16)
                (ks8, ks), (vs8, vs) = quantise_rows(k), quantise_rows(v)
                caches = {"bf16": (k, v), "fp8": (e4m3_bytes(k), e4m3_bytes(v)), "fp8-row": (ks8, vs8, ks, vs)}
                qc, pc = q[:, :, :CHUNK].contiguous(), (pos[:, :CHUNK] + (S - CHUNK)).contiguous()
                for cache, ops in caches.items():
                    by_pos, by_page = new_fns[cache]
                    for page in (None, *PAGE_SIZES):
                        layout = "static" if page is None else f"page {page}"
                        head = f"{model:<9} {B:>2} {S:>5} {cache:>8} {layout:>9}"
                        windowed = S > WINDOW and page in (None, 16)
                        if page is None:
                            _cell(lines, missed, args, f"{head} {T:>6}",
                                  {"chain": _chain(cache, q, ops, lambda: position_mask(pos, S)),
                                   "new": lambda: by_pos(q, *ops, pos)})
                            if windowed:
                                _cell(lines, missed, args, f"{head} {'win':>6}",
                                      {"chain": _chain(cache, qc, ops, lambda: window_mask(pc, S, WINDOW)),
                                       "new": lambda: by_pos(qc, *ops, pc, window=WINDOW)})
                            continue
                        P = S // page
                        table = torch.randperm(B * P, device="cuda").view(B, P)
                        pools = pools_of(ops, table, page)
                        _cell(lines, missed, args, f"{head} {T:>6}",
                              {"chain": _chain(cache, q, pools, lambda: paged_mask(pos, table, page, B * P), table, page),
                               "new": lambda: by_page(q, *pools, pos, table, page, B * P)})
                        if windowed:
                            _cell(lines, missed, args, f"{head} {'win':>6}",
                                  {"chain": _chain(cache, qc, pools, lambda: paged_window_mask(pc, table, page, B * P, WINDOW),
                                                   table, page),
                                   "new": lambda: by_page(qc, *pools, pc, table, page, B * P, window=WINDOW)})
                        del pools, table
                del caches, k, v, ks8, vs8, ks, vs
            # for information: the causal ring kernel over S = T, the ceiling of this structure
            k = torch.randn(B, Hkv, T, D, device="cuda").to(BF16)
            v = torch.randn(B, Hkv, T, D, device="cuda").to(BF16)
            t = measure({"ring": lambda: A.attn_fwd(q, k, v, causal=True)[0], "new": lambda: A.prefill_attn_pos(q, k, v, pos)},
                        args.batch, args.batches)
            lines.append(f"{model:<9} {B:>2} {T:>5} {'bf16':>8} {'info':>9} | causal ring kernel {fmt(t['ring'])} | "
                         f"prefill_attn_pos over S = T {fmt(t['new'])} | new/ring "
                         f"{statistics.median(t['new']) / statistics.median(t['ring']):.3f}")
            print(lines[-1], flush=True)
            args.save()
            del k, v, q
    lines.append(f"cells where the new launch is slower than the chain's median + spread: {len(missed)}")
    lines.extend("  " + m for m in missed)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prefill_attn_d256.txt"))
    ap.add_argument("--batch", type=int, default=3)
    ap.add_argument("--batches", type=int, default=21)
    ap.add_argument("--models", nargs="+", default=list(MODELS), choices=list(MODELS))
    ap.add_argument("--batches-of", nargs="+", type=int, default=[1, 8], help="the batch sizes of the cells")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("prefill_attn_d256_bench needs the GPU: a CPU timing says nothing about it")
    lines = [f"prefill attention at head dim 256 vs the chain it replaces, {torch.cuda.get_device_name(0)}", ""]

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")

    args.save = save
    run(args, lines)
    save()


if __name__ == "__main__":
    main()
