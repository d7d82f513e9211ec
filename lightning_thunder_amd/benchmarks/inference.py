"""Prefill / decode inference benchmark (parity: reference ``thunder/benchmarks/benchmark_inference.py``:
throughput and latency of the prefill and decode phases — TTFT, TBOT, tokens/s — with batch size,
input/output lengths, warmup and iteration counts).

The reference drives an HF ``AutoModelForCausalLM`` with a ``HybridChunkedCache``; here the model
is the LitGPT-architecture model of this package (``--model``, random-init bf16 weights, no
checkpoints offline) with its static KV cache, so every mode runs the same model code:

* ``eager``    — PyTorch eager (ROCm);
* ``thunder``  — ``jit(model)``: prefill and decode are two cached programs on the HIP executors;
* ``hipgraph`` — ``jit`` + ``HipGraphTransform``: the decode step replays as a hipGraph.

Per iteration: one prefill of ``--input-length`` tokens for ``--batch-size`` sequences (TTFT =
its latency, including the first sampled token), then ``--output-length - 1`` decode steps
(TBOT = mean latency of one decode step).  Every phase is bracketed by device synchronisation.
``--prompt-lengths a,b,c,...`` (one per sequence) makes the batch ragged: the prompt is right-padded to the longest
length (which replaces ``--input-length``), the first token of sequence b comes from its own last prompt position,
and every decode step runs at per-sequence positions (an int64 ``[B, 1]`` tensor advanced in place).
Prints one JSON line per mode with mean / median / p90 over ``--num-iterations`` iterations
after ``--warmup-iterations`` untimed ones.
"""
from __future__ import annotations

import argparse
import json
import statistics
import time

import torch

from . import KV_CACHE_FORMATS


def _percentile(xs, q):
    s = sorted(xs)
    return s[min(len(s) - 1, int(round(q * (len(s) - 1))))]


def _build(args, device):
    from ..models.litgpt import GPT, Config, init_weights

    kw = {} if args.n_layer is None else {"n_layer": args.n_layer}
    if args.sliding_window is not None:  # every layer attends its last N keys, whatever the config says
        kw.update(sliding_window_size=args.sliding_window, sliding_window_indices=None)
    cfg = Config.from_name(args.model, **kw)
    with torch.device("meta"):
        model = GPT(cfg)
    model = model.to_empty(device=device).to(torch.bfloat16)
    torch.manual_seed(0)
    init_weights(model)
    model.requires_grad_(False)
    model.eval()
    model.set_kv_cache(args.batch_size, args.input_length + args.output_length + 8, device=device,
                       page_size=args.kv_page_size, num_pages=args.kv_num_pages, **KV_CACHE_FORMATS[args.kv_cache_dtype])
    return model, cfg


def _forward_for(mode, model):
    import lightning_thunder_amd as thunder

    if mode == "eager":
        return model
    if mode == "thunder":
        return thunder.jit(model)
    if mode == "hipgraph":
        from ..transforms.hipgraph import HipGraphTransform

        return thunder.jit(model, transforms=[HipGraphTransform()])
    raise ValueError(f"unknown mode {mode!r}")


def run(mode: str, args) -> dict:
    from ..models.litgpt import _chunked_prefill
    from ..ops.sampling import argmax_last

    device = torch.device("cuda", 0)
    torch.empty(1, device=device)  # the allocator exists from the first allocation on
    torch.cuda.reset_peak_memory_stats(device)
    model, cfg = _build(args, device)
    fwd = _forward_for(mode, model)
    gen = torch.Generator(device).manual_seed(1)
    prompt = torch.randint(0, cfg.vocab_size, (args.batch_size, args.input_length), device=device, generator=gen)
    prefill_pos = torch.arange(args.input_length, device=device)
    pages = model.kv_pages  # a paged cache (--kv-page-size) takes one position per token: the ragged route
    ragged = args.prompt_lengths is not None or pages is not None
    host_lengths = args.prompt_lengths or [args.input_length] * args.batch_size
    # every layer under one window: a paged cache gives up the pages below it, as generate() does
    trim = cfg.uniform_window if pages is not None else None
    if pages is not None:
        prefill_pos = prefill_pos.expand(args.batch_size, -1).contiguous()
    if ragged:
        lengths = torch.tensor(host_lengths, dtype=torch.int64, device=device)
        last = lengths - 1
        rows = torch.arange(args.batch_size, device=device)
        pos = torch.empty((args.batch_size, 1), dtype=torch.int64, device=device)
    else:
        pos = torch.empty(1, dtype=torch.int64, device=device)

    def iteration():
        if pages is not None:
            pages.reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        move_pages = None
        if pages is not None:
            held = list(host_lengths)
            if trim is None or args.prefill_chunk is None:
                pages.reserve(held)
            else:  # pages chunk by chunk, those below the chunk's windows handed back first
                def move_pages(c0, c1):
                    pages.trim([max(0, min(c0, n) - trim + 1) for n in held])
                    pages.reserve([min(c1, n) for n in held])
        if args.prefill_chunk is not None:  # slices of the prompt at 2-D positions, as generate(prefill_chunk=...) runs them
            tok = argmax_last(_chunked_prefill(fwd, prompt, args.prefill_chunk, lengths if ragged else None,
                                               move_pages), keepdim=True)
        else:
            logits = fwd(prompt, prefill_pos)
            tok = argmax_last(logits[rows, last] if ragged else logits[:, -1], keepdim=True)
        torch.cuda.synchronize()
        ttft = time.perf_counter() - t0
        if ragged:
            pos.copy_(lengths.view(-1, 1))
        else:
            pos.fill_(args.input_length)
        steps = []
        for _ in range(args.output_length - 1):
            t1 = time.perf_counter()
            if pages is not None:  # room for this step's token, from host-side counters
                if trim is not None:
                    pages.trim([max(0, n - trim + 1) for n in held])
                held = [n + 1 for n in held]
                pages.reserve(held)
            logits = fwd(tok, pos)
            tok = argmax_last(logits[:, -1], keepdim=True)
            pos.add_(1)
            torch.cuda.synchronize()
            steps.append(time.perf_counter() - t1)
        return ttft, steps

    t0 = time.perf_counter()
    iteration()
    first = time.perf_counter() - t0
    for _ in range(args.warmup_iterations):
        iteration()
    ttfts, tbots, totals = [], [], []
    for _ in range(args.num_iterations):
        ttft, steps = iteration()
        ttfts.append(ttft)
        tbots.extend(steps)
        totals.append(ttft + sum(steps))
    B, n_out = args.batch_size, args.output_length
    decode_s = sum(tbots)
    return {
        "metric": f"{args.model} prefill/decode inference (batch {B}, {args.input_length} in, {n_out} out)",
        "mode": mode,
        "ttft_ms": {"mean": round(1e3 * statistics.mean(ttfts), 3), "median": round(1e3 * statistics.median(ttfts), 3),
                    "p90": round(1e3 * _percentile(ttfts, 0.9), 3)},
        "tbot_ms": ({"mean": round(1e3 * statistics.mean(tbots), 3), "median": round(1e3 * statistics.median(tbots), 3),
                     "p90": round(1e3 * _percentile(tbots, 0.9), 3)} if tbots else None),
        "prefill_tokens_per_s": round(B * args.input_length / statistics.mean(ttfts), 1),
        "decode_tokens_per_s": round(B * len(tbots) / decode_s, 1) if tbots else None,
        "total_tokens_per_s": round(B * n_out * len(totals) / sum(totals), 1),
        "latency_ms_per_request": round(1e3 * statistics.mean(totals), 2),
        "first_call_s": round(first, 2),
        "batch_size": B, "input_length": args.input_length, "output_length": n_out,
        "prompt_lengths": args.prompt_lengths, "prefill_chunk": args.prefill_chunk,
        "dtype": "bf16", "kv_cache_dtype": args.kv_cache_dtype,
        "kv_cache_gib": round(sum(c.numel() * c.element_size() for b in model.transformer.h
                                  for c in b.attn.kv_cache.buffers()) / 2 ** 30, 3),  # scale buffers included
        "kv_page_size": args.kv_page_size, "kv_num_pages": None if pages is None else pages.num_pages,
        "kv_pages_in_use": None if pages is None else pages.pages_in_use,
        "kv_pages_peak": None if pages is None else pages.peak_pages_in_use,  # of the last iteration
        "sliding_window": cfg.sliding_window_size,
        "memory_allocated_gib": round(torch.cuda.memory_allocated(device) / 2 ** 30, 3),  # held after the last step
        "max_memory_allocated_gib": round(torch.cuda.max_memory_allocated(device) / 2 ** 30, 3),
        "data": "synthetic prompt, random-init weights", "n_gpus": 1,
    }


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    p.add_argument("--model", default="Llama-3.2-1B")
    p.add_argument("--batch-size", type=int, default=1)
    p.add_argument("--input-length", type=int, default=2048)
    p.add_argument("--output-length", type=int, default=128)
    p.add_argument("--num-iterations", type=int, default=5)
    p.add_argument("--warmup-iterations", type=int, default=2)
    p.add_argument("--modes", default="eager,thunder,hipgraph")
    p.add_argument("--n-layer", type=int, default=None, help="debug only")
    p.add_argument("--kv-cache-dtype", choices=sorted(KV_CACHE_FORMATS), default="model",
                   help="'fp8' keeps the static KV cache as unscaled e4m3 (half the bytes), 'fp8-row' as e4m3 "
                        "with one power-of-two scale byte per (token, kv head) row")
    p.add_argument("--prompt-lengths", default=None,
                   help="a,b,c,...: one prompt length per sequence (a ragged batch, right-padded to the longest); "
                        "--batch-size must match")
    p.add_argument("--kv-page-size", type=int, default=None,
                   help="a power of two >= 16: a paged KV cache (pools of pages and a block table) instead of the "
                        "static one")
    p.add_argument("--kv-num-pages", type=int, default=None,
                   help="pages per pool of a paged cache (default: what the static cache would hold)")
    p.add_argument("--prefill-chunk", type=int, default=None,
                   help="run the prompt in slices of at most this many columns at 2-D positions (chunked prefill)")
    p.add_argument("--sliding-window", type=int, default=None,
                   help="a sliding window of this many keys on every layer (overrides the model's config); with a paged "
                        "cache the pages below the window go back to the pool")
    args = p.parse_args(argv)
    if args.sliding_window is not None and args.sliding_window < 1:
        p.error("--sliding-window must be >= 1")
    if args.kv_num_pages is not None and args.kv_page_size is None:
        p.error("--kv-num-pages needs --kv-page-size")
    if args.prefill_chunk is not None and args.prefill_chunk < 1:
        p.error("--prefill-chunk must be >= 1")
    if args.output_length < 1:
        p.error("--output-length must be >= 1")
    if args.prompt_lengths is not None:
        try:
            args.prompt_lengths = [int(x) for x in args.prompt_lengths.split(",")]
        except ValueError:
            p.error("--prompt-lengths takes comma-separated integers")
        if len(args.prompt_lengths) != args.batch_size or min(args.prompt_lengths) < 1:
            p.error("--prompt-lengths needs one positive length per sequence of --batch-size")
        args.input_length = max(args.prompt_lengths)
    for mode in args.modes.split(","):
        print(json.dumps(run(mode, args)), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
