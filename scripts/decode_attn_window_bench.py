"""The window mode of the decode and prefill attention kernels against their position mode, and
``benchmarks/inference.py`` with and without ``--sliding-window`` on a paged cache.

    python scripts/decode_attn_window_bench.py [--out profiles/decode_attn_window.txt] [--jsonl profiles/inference_window.jsonl]
                                               [--skip-models | --only-models] [--skip-prefill]

Part one: per head shape, batch, cache format (bf16, unscaled e4m3, e4m3 with row scales) and layout (static, paged
with pages of 16 and 64 rows behind a shuffled block table) one decode step's attention (T = 1) over a cache of
capacity S = 32768 under a window of W = 4096 keys, four launches on the same buffers and the same grid:

    win        the window kernel, every sequence at position S - 1 (reads keys S - W .. S - 1),
    pos@W-1    the position kernel, every sequence at position W - 1 (reads keys 0 .. W - 1: as many),
    pos@S-1    the position kernel, every sequence at position S - 1 (reads all S keys),
    win>=n     the window kernel at position S - 1 under a window of S keys (reads all S keys).

(a) win against pos@W-1: the same number of keys, so win should be no slower than that kernel's median plus its own
spread; (b) pos@S-1 / win is what the window buys at this context; (c) win>=n against pos@S-1 is what the extra
instantiation costs.  Each version's launches are captured into a hipGraph of ``--batch`` back-to-back calls (device
time, no host gaps); the replays of the versions alternate, after warm-up, and a point is the median of ``--batches``
replays / batch; "spread" is max - min of a version over its replays in the cell.  No ratio is fixed in advance: every
cell is reported, and (a) and (c) are marked where they miss.

Part two: one prefill chunk of 512 rows at positions 16384 .. 16895 over the same capacity, W = 4096: the window
kernel against the position kernel for the same chunk and against what it replaces under LTA_KV_WINDOW_FUSION=0, the
window mask built and the masked flash forward run over it (16-bit static cache, where that chain needs no gather or
dequantise pass).

Part three runs ``benchmarks.inference`` (hipgraph mode, Llama-3.2-1B, batch 8, page size 16, a 4096-token prompt in
chunks of 512, 64 new tokens) in a fresh process per row, with ``--sliding-window 1024`` and without; the JSON lines go
to ``--jsonl``.
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
from scripts.decode_attn_pos_bench import MODELS

BF16 = torch.bfloat16
S, W = 32768, 4096
LAYOUTS = (("static", None), ("page 16", 16), ("page 64", 64))


def _med(t):
    return statistics.median(t)


def _spread(t):
    return max(t) - min(t)


def part_one(args, lines):
    from lightning_thunder_amd.ops import attention as A
    from lightning_thunder_amd.ops.kv8 import e4m3_bytes, quantise_rows

    lines.append(f"decode attention, T = 1, capacity S = {S}, window W = {W}, us per launch: median (min..max) of {args.batches} "
                 f"graph replays of {args.batch} launches, versions alternating")
    lines.append(f"{'model':<13} {'B':>2} {'cache':>8} {'layout':>8} | {'win us':>24} | {'pos@W-1 us':>24} | {'pos@S-1 us':>24} | "
                 f"{'win>=n us':>24} | (a) win/pos@W-1 within its spread | (b) pos@S-1/win | (c) win>=n/pos@S-1 within spread")
    missed = []
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
            last = torch.full((B, 1), S - 1, dtype=torch.int64, device="cuda")
            short = torch.full((B, 1), W - 1, dtype=torch.int64, device="cuda")
            for cache, (ops, by_pos, by_page) in caches.items():
                for layout, page in LAYOUTS:
                    if page is None:
                        def run(pos, window=None, _f=by_pos, _ops=ops):
                            return _f(q, *_ops, pos, window=window)
                    else:
                        P = S // page
                        table = torch.randperm(B * P, device="cuda").view(B, P)
                        pools = pools_of(ops, table, page)

                        def run(pos, window=None, _f=by_page, _pools=pools, _t=table, _p=page, _n=B * P):
                            return _f(q, *_pools, pos, _t, _p, _n, window=window)
                    versions = {"win": lambda: run(last, W), "pos_w": lambda: run(short), "pos_s": lambda: run(last),
                                "win_all": lambda: run(last, S)}
                    if not torch.equal(versions["win_all"]().view(torch.int16), versions["pos_s"]().view(torch.int16)):
                        sys.exit(f"{model} B={B} {cache} {layout}: a window of S keys differs from the position kernel")
                    t = measure(versions, args.batch, args.batches)
                    a_ok = _med(t["win"]) <= _med(t["pos_w"]) + _spread(t["pos_w"])
                    c_ok = abs(_med(t["win_all"]) - _med(t["pos_s"])) <= _spread(t["pos_s"])
                    lines.append(f"{model:<13} {B:>2} {cache:>8} {layout:>8} | {fmt(t['win']):>24} | {fmt(t['pos_w']):>24} | "
                                 f"{fmt(t['pos_s']):>24} | {fmt(t['win_all']):>24} | "
                                 f"{_med(t['win']) / _med(t['pos_w']):>6.3f} {'yes' if a_ok else 'NO':>3} | "
                                 f"{_med(t['pos_s']) / _med(t['win']):>6.2f}x | "
                                 f"{_med(t['win_all']) / _med(t['pos_s']):>6.3f} {'yes' if c_ok else 'NO':>3}")
                    print(lines[-1], flush=True)
                    for ok, what in ((a_ok, "(a)"), (c_ok, "(c)")):
                        if not ok:
                            missed.append(f"{what} {model} B={B} {cache} {layout}")
                    if page is not None:
                        del pools
            del caches, k, v, k8, v8, ks8, vs8
    lines.append(f"cells that miss (a) or (c): {len(missed)}")
    lines.extend("  " + m for m in missed)


def part_prefill(args, lines):
    from lightning_thunder_amd.ops import attention as A
    from lightning_thunder_amd.ops.kv_rows import window_mask

    T, base = 512, 16384
    lines.append("")
    lines.append(f"prefill attention, one chunk of {T} rows at positions {base} .. {base + T - 1}, capacity S = {S}, W = {W}, bf16 "
                 f"static cache, us per launch (as above)")
    lines.append(f"{'model':<13} {'B':>2} | {'window kernel us':>26} | {'position kernel us':>26} | {'mask + masked flash us':>26} | "
                 f"pos/win | chain/win")
    torch.manual_seed(0)
    for model, (Hq, Hkv, D) in MODELS.items():
        for B in (1, 8):
            k = torch.randn(B, Hkv, S, D, device="cuda").to(BF16)
            v = torch.randn(B, Hkv, S, D, device="cuda").to(BF16)
            q = torch.randn(B, Hq, T, D, device="cuda").to(BF16)
            pos = torch.arange(base, base + T, device="cuda").expand(B, T).contiguous()
            versions = {"win": lambda: A.prefill_attn_pos(q, k, v, pos, window=W),
                        "pos": lambda: A.prefill_attn_pos(q, k, v, pos),
                        "chain": lambda: A.attn_fwd(q, k, v, causal=False, mask=window_mask(pos, S, W))[0]}
            if not torch.equal(versions["win"]().view(torch.int16), versions["chain"]().view(torch.int16)):
                sys.exit(f"{model} B={B}: the window kernel differs from the masked flash forward")
            t = measure(versions, max(1, args.batch // 10), args.batches)
            lines.append(f"{model:<13} {B:>2} | {fmt(t['win']):>26} | {fmt(t['pos']):>26} | {fmt(t['chain']):>26} | "
                         f"{_med(t['pos']) / _med(t['win']):>6.2f}x | {_med(t['chain']) / _med(t['win']):>8.2f}x")
            print(lines[-1], flush=True)
            del k, v, q


def part_models(args, lines):
    import gc

    gc.collect()
    torch.cuda.empty_cache()
    lines.append("")
    lines.append(f"benchmarks/inference.py, Llama-3.2-1B, batch 8, hipgraph mode, one fresh process per row, --kv-page-size 16, "
                 f"--input-length 4096 --prefill-chunk 512, {args.output_length} out, {args.iterations} iterations after "
                 f"{args.warmup} warm-up")
    lines.append(f"{'window':>6} | {'TTFT ms':>8} | {'TBOT mean':>9} {'median':>7} {'p90':>7} | {'KV GiB':>7} | peak pages in use")
    rows = []
    for window in (None, 1024):
        extra = [] if window is None else ["--sliding-window", str(window)]
        cmd = [sys.executable, "-m", "lightning_thunder_amd.benchmarks.inference", "--model", "Llama-3.2-1B",
               "--batch-size", "8", "--input-length", "4096", "--prefill-chunk", "512", "--output-length", str(args.output_length),
               "--num-iterations", str(args.iterations), "--warmup-iterations", str(args.warmup), "--modes", "hipgraph",
               "--kv-page-size", "16", *extra]
        p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
        if p.returncode != 0:
            sys.exit(f"{' '.join(cmd)} failed ({p.returncode}):\n{p.stderr[-4000:]}")
        r = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
        rows.append(r)
        tb = r["tbot_ms"]
        lines.append(f"{str(window):>6} | {r['ttft_ms']['median']:>8.2f} | {tb['mean']:>9.3f} {tb['median']:>7.3f} {tb['p90']:>7.3f} | "
                     f"{r['kv_cache_gib']:>7.3f} | {r.get('kv_pages_peak')} of {r.get('kv_num_pages')}")
        print(lines[-1], flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.jsonl)), exist_ok=True)
        with open(args.jsonl, "w") as f:
            f.write("".join(json.dumps(x) + "\n" for x in rows))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_attn_window.txt"))
    ap.add_argument("--jsonl", default=os.path.join(ROOT, "profiles", "inference_window.jsonl"))
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--batches", type=int, default=21)
    ap.add_argument("--skip-models", action="store_true", help="the kernels only")
    ap.add_argument("--only-models", action="store_true", help="part three only")
    ap.add_argument("--skip-prefill", action="store_true")
    ap.add_argument("--output-length", type=int, default=64)
    ap.add_argument("--iterations", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("decode_attn_window_bench needs the GPU: a CPU timing says nothing about it")
    lines = [f"attention under a sliding window vs by positions alone, {torch.cuda.get_device_name(0)}", ""]

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")

    if not args.only_models:
        part_one(args, lines)
        save()
        if not args.skip_prefill:
            part_prefill(args, lines)
            save()
    if not args.skip_models:
        part_models(args, lines)
        save()
    print("\n".join(lines))


if __name__ == "__main__":
    main()
