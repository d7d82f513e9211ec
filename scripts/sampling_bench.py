"""Decode-step sampling: one ``sample_last`` call (csrc/sampling.hip, one launch) against the eager op
sequence ``models/litgpt.generate`` ran before it (divide, topk, where, fp32 softmax, multinomial).  The
sequence is copied here as the baseline; it had no top-p, so those points add the usual eager nucleus
filter (sort, softmax, cumsum, scatter) to it.

    python scripts/sampling_bench.py [--out profiles/sampling_bench.txt]

Per point: R rows of V bf16 logits (randn * 2: with these nothing is far enough below the maximum to skip
its draw, the kernel's slowest case).  Time per call = HIP-event time over a batch of back-to-back calls /
batch size, so launch gaps count where the host is the limit, as they do between graph replays in
``generate``; the two versions alternate batch by batch, after warm-up, and the medians are compared.
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from lightning_thunder_amd.ops.sampling import sample_last


def eager_sample(last, temperature, top_k, top_p):
    last = last / temperature
    if top_k is not None:
        v, _ = torch.topk(last, min(top_k, last.size(-1)))
        last = torch.where(last < v[:, [-1]], torch.full_like(last, -float("inf")), last)
    if top_p is not None:  # not in generate before: the common eager formulation
        s, idx = torch.sort(last.float(), dim=-1, descending=True)
        pr = torch.softmax(s, -1)
        drop = pr.cumsum(-1) - pr >= top_p
        last = last.masked_fill(torch.zeros_like(drop).scatter_(-1, idx, drop), -float("inf"))
    return torch.multinomial(torch.softmax(last.float(), -1), 1)


def batch_us(fn, batch):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(batch):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / batch * 1000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "sampling_bench.txt"))
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--batches", type=int, default=21)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("sampling_bench needs the GPU: a CPU timing says nothing about it")
    lines = [f"sample_last (one launch) vs the eager sampling chain, bf16 logits randn*2, temperature 0.8, "
             f"{torch.cuda.get_device_name(0)}",
             f"us per call: median of {args.batches} batches of {args.batch} back-to-back calls (HIP events), "
             "versions alternating; ratio = eager / kernel",
             f"{'R':>3} {'V':>7} {'filter':<22} {'kernel us':>10} {'eager us':>10} {'ratio':>6}   kernel min..max / eager min..max"]
    slower = []
    torch.manual_seed(0)
    for R in (1, 8):
        for V in (32000, 128256):
            x = (torch.randn(R, V, device="cuda") * 2).to(torch.bfloat16)
            for k, p in ((None, None), (50, None), (None, 0.9), (50, 0.9)):
                fk = lambda: sample_last(x, 0.8, k, p, keepdim=True)  # noqa: E731
                fe = lambda: eager_sample(x, 0.8, k, p)  # noqa: E731
                for _ in range(args.batch):
                    fk()
                    fe()
                torch.cuda.synchronize()
                tk, te = [], []
                for _ in range(args.batches):
                    tk.append(batch_us(fk, args.batch))
                    te.append(batch_us(fe, args.batch))
                mk, me = statistics.median(tk), statistics.median(te)
                name = "none" if k is None and p is None else " ".join(
                    f"{n}={v}" for n, v in (("top_k", k), ("top_p", p)) if v is not None)
                lines.append(f"{R:>3} {V:>7} {name:<22} {mk:>10.1f} {me:>10.1f} {me / mk:>6.2f}   "
                             f"{min(tk):.1f}..{max(tk):.1f} / {min(te):.1f}..{max(te):.1f}")
                print(lines[-1], flush=True)
                if mk > me:
                    slower.append(f"R={R} V={V} {name}")
    lines.append("points where the kernel is slower than the eager chain: " + ("; ".join(slower) if slower else "none"))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
