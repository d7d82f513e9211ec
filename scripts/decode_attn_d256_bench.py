"""The decode attention kernel at head dim 256 (csrc/decode_attention_wide.h) against the chain that ran for the same
call before it existed: the mask operation, the page gathers and the dequantise pass where the format has them, and
ATen's scaled_dot_product_attention over the result.

    python scripts/decode_attn_d256_bench.py [--out profiles/decode_attn_d256.txt] [--batch 20] [--batches 21]

Gemma-2b (8 query heads on 1 KV head) and Gemma-7b (16 on 16), T = 1, batch 1 / 8, capacity S 2048 / 8192 with every
sequence at position S - 1 (full) and S / 4 - 1 (quarter), three cache formats (bf16, unscaled e4m3, e4m3 with row
scales), static and paged (pages of 16 rows behind a shuffled block table), and one window row (S 32768, W 4096).
Each side's launches are captured into a hipGraph of ``--batch`` back-to-back calls (device time, no host gaps); the
replays of the two sides alternate after warm-up and a point is the median of ``--batches`` replays / batch.  K/V GB/s
counts the live keys' K and V bytes once per KV head.  No ratio is fixed in advance: every cell is reported, and a
cell whose kernel median is not below the chain's is listed under "Known gaps".
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import torch.nn.functional as F

from scripts.decode_attn_kv8_bench import fmt, measure
from scripts.decode_attn_paged_bench import pools_of

BF16 = torch.bfloat16
D, PAGE = 256, 16
MODELS = {"Gemma-2b": (8, 1), "Gemma-7b": (16, 16)}


def cells(model, B, S, live, window=None):
    """(cache, layout, the kernel call, the chain call, K/V bytes read) for every format and layout of one shape."""
    from lightning_thunder_amd.ops import attention as A
    from lightning_thunder_amd.ops.kv8 import dequantise_rows, e4m3_bytes, e4m3_values, quantise_rows
    from lightning_thunder_amd.ops.kv_pages import gather_pages, paged_mask
    from lightning_thunder_amd.ops.kv_rows import position_mask, window_mask

    Hq, Hkv = MODELS[model]
    k = torch.randn(B, Hkv, S, D, device="cuda").to(BF16)
    v = torch.randn(B, Hkv, S, D, device="cuda").to(BF16)
    q = torch.randn(B, Hq, 1, D, device="cuda").to(BF16)
    pos = torch.full((B, 1), live - 1, dtype=torch.int64, device="cuda")
    (ks8, ks), (vs8, vs) = quantise_rows(k), quantise_rows(v)
    formats = {"bf16": ((k, v), A.decode_attn_pos, A.decode_attn_paged, lambda c: c, 2),
               "fp8": ((e4m3_bytes(k), e4m3_bytes(v)), A.decode_attn_kv8_pos, A.decode_attn_kv8_paged,
                       lambda c: (e4m3_values(c[0], BF16), e4m3_values(c[1], BF16)), 1),
               "fp8-row": ((ks8, vs8, ks, vs), A.decode_attn_kv8s_pos, A.decode_attn_kv8s_paged,
                           lambda c: (dequantise_rows(c[0], c[2], BF16), dequantise_rows(c[1], c[3], BF16)), 1)}
    sdpa = lambda kk, vv, mask: F.scaled_dot_product_attention(q, kk, vv, attn_mask=mask, enable_gqa=True)  # noqa: E731
    kv_bytes = 2 * B * Hkv * min(live, window or live) * D
    for cache, (ops, by_pos, by_page, values, size) in formats.items():
        def static_mask():
            return position_mask(pos, S) if window is None else window_mask(pos, S, window)

        yield (cache, "static", lambda _f=by_pos, _o=ops: _f(q, *_o, pos, window=window),
               lambda _o=ops, _v=values: sdpa(*_v(_o), static_mask()), kv_bytes * size)
        if window is not None:
            continue
        P = S // PAGE
        table = torch.randperm(B * P, device="cuda").view(B, P)
        pools = pools_of(ops, table, PAGE)

        def chain(_p=pools, _t=table, _v=values):
            return sdpa(*_v([gather_pages(p, _t, PAGE) for p in _p]), paged_mask(pos, _t, PAGE, B * P))

        yield (cache, "page 16", lambda _f=by_page, _p=pools, _t=table: _f(q, *_p, pos, _t, PAGE, B * P), chain,
               kv_bytes * size)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_attn_d256.txt"))
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--batches", type=int, default=21)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("decode_attn_d256_bench needs the GPU: a CPU timing says nothing about it")
    lines = [f"decode attention at head dim 256 vs the chain it replaces, {torch.cuda.get_device_name(0)}", "",
             f"T = 1, us per launch: median (min..max) of {args.batches} graph replays of {args.batch} launches, sides alternating",
             f"{'model':<9} {'B':>2} {'S':>6} {'live':>6} {'cache':>8} {'layout':>8} | {'kernel us':>24} | {'chain us':>24} | "
             f"chain/kernel | K/V GB/s"]
    gaps = []
    torch.manual_seed(0)
    shapes = [(m, B, S, live, None) for m in MODELS for B in (1, 8) for S in (2048, 8192) for live in (S, S // 4)]
    shapes.append(("Gemma-2b", 8, 32768, 32768, 4096))
    for model, B, S, live, window in shapes:
        for cache, layout, kernel, chain, kv_bytes in cells(model, B, S, live, window):
            err = (kernel().float() - chain().float()).abs().max().item()
            if not err < 0.1:
                sys.exit(f"{model} B={B} S={S} {cache} {layout}: the kernel differs from the chain by {err}")
            t = measure({"kernel": kernel, "chain": chain}, args.batch, args.batches)
            mk, mc = statistics.median(t["kernel"]), statistics.median(t["chain"])
            what = f"{model:<9} {B:>2} {S:>6} {('W' + str(window)) if window else live:>6} {cache:>8} {layout:>8}"
            lines.append(f"{what} | {fmt(t['kernel']):>24} | {fmt(t['chain']):>24} | {mc / mk:>11.2f}x | {kv_bytes / mk / 1e3:>8.0f}")
            print(lines[-1], flush=True)
            if not mk < mc:
                gaps.append(f"  {what}: kernel {mk:.2f} us, chain {mc:.2f} us")
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")
    lines += ["", f"Known gaps (kernel median not below the chain's): {len(gaps)}", *gaps]
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[-1 - len(gaps):]))


if __name__ == "__main__":
    main()
