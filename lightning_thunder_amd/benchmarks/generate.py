"""Generation latency benchmark (parity: reference ``examples/quickstart/hf_llm.py``; README
``README.md:308-317``: HF Llama-3.2-1B, 100 new tokens, static cache — eager 1,493 ms,
Thunder + CUDAGraphs 542 ms on 1x H100).

Same task on MI355X with the LitGPT-architecture Llama-3.2-1B (random-init weights, synthetic
prompt; no checkpoints offline): greedy decoding of ``--new-tokens`` tokens after a
``--prompt-len`` token prompt with a static KV cache, bf16 (``--temperature`` > 0 with ``--top-k`` /
``--top-p`` / ``--seed``: sampled decoding through ``ops.sampling.sample_last``, LitGPT modes only).  Modes:

* ``eager``    — PyTorch eager (ROCm), same model code;
* ``thunder``  — ``jit(model)``: prefill and decode are two cached programs (hipex/hipfuse kernels,
  in-place KV-cache updates);
* ``hipgraph`` — ``jit(model, transforms=[HipGraphTransform()])``: the decode step replays as
  hipGraphs (the "reduce-overhead" configuration);
* ``hf_eager`` / ``hf_thunder`` / ``hf_hipgraph`` — the reference's exact setup: a
  ``transformers.LlamaForCausalLM`` (Llama-3.2-1B architecture, random init) driven by HF
  ``model.generate(cache_implementation="static")``, eager or through
  ``compile(recipe="hf-transformers"[, plugins="reduce-overhead"])``.

``--prompt-lengths a,b,c,...`` with a matching ``--batch-size`` (LitGPT modes only) generates for a ragged batch:
the prompt is right-padded to the longest length and decoding runs at per-sequence positions
(``generate(..., prompt_lengths=...)``).

Prints one JSON line per mode: mean latency (ms) of ``--iters`` full generations after
``--warmup`` untimed ones.
"""
from __future__ import annotations

import argparse
import json
import sys
import time

import torch

from . import KV_CACHE_FORMATS


def _build(model_name: str, max_seq: int, device, n_layer=None, kv_cache_dtype: str = "model", batch_size: int = 1,
           page_size=None, num_pages=None, sliding_window=None):
    from ..models.litgpt import GPT, Config, init_weights

    kw = {} if n_layer is None else {"n_layer": n_layer}
    if sliding_window is not None:  # every layer attends its last N keys, whatever the config says
        kw.update(sliding_window_size=sliding_window, sliding_window_indices=None)
    cfg = Config.from_name(model_name, **kw)
    with torch.device("meta"):
        model = GPT(cfg)
    model = model.to_empty(device=device).to(torch.bfloat16)
    torch.manual_seed(0)
    init_weights(model)
    model.requires_grad_(False)
    model.eval()
    model.set_kv_cache(batch_size, max_seq, device=device, page_size=page_size, num_pages=num_pages,
                       **KV_CACHE_FORMATS[kv_cache_dtype])
    return model, cfg


def _build_hf(device, n_layer=None):
    """Hugging Face ``LlamaForCausalLM`` with the Llama-3.2-1B architecture (random init)."""
    import transformers as tf

    cfg = tf.LlamaConfig(vocab_size=128256, hidden_size=2048, intermediate_size=8192,
                         num_hidden_layers=n_layer or 16, num_attention_heads=32, num_key_value_heads=8,
                         max_position_embeddings=131072, rope_theta=500000.0, rms_norm_eps=1e-5,
                         tie_word_embeddings=True,
                         rope_scaling={"rope_type": "llama3", "factor": 32.0, "low_freq_factor": 1.0,
                                       "high_freq_factor": 4.0, "original_max_position_embeddings": 8192})
    torch.manual_seed(0)  # the same random weights in every mode: generated tokens are comparable
    with torch.device(device):
        model = tf.LlamaForCausalLM(cfg).to(torch.bfloat16)
    model.requires_grad_(False)
    model.eval()
    return model, cfg


def run(mode: str, args) -> dict:
    import lightning_thunder_amd as thunder
    from ..models.litgpt import generate

    device = torch.device("cuda", 0)
    sampling = args.temperature > 0 and not mode.startswith("hf_")  # the HF modes stay greedy
    if mode.startswith("hf_"):
        # the reference's benchmark: HF transformers model.generate with a static cache
        model, cfg = _build_hf(device, args.n_layer)
        if mode == "hf_eager":
            gm = model
        else:
            gm = thunder.compile(model, recipe="hf-transformers",
                                 plugins="reduce-overhead" if mode == "hf_hipgraph" else None)
        prompt = torch.randint(1, cfg.vocab_size, (1, args.prompt_len), device=device,
                               generator=torch.Generator(device).manual_seed(1))
        kw = dict(max_new_tokens=args.new_tokens, min_new_tokens=args.new_tokens, do_sample=False,
                  cache_implementation="static", pad_token_id=0, disable_compile=True)

        def once():
            return gm.generate(prompt, **kw)
    else:
        model, cfg = _build(args.model, args.prompt_len + args.new_tokens + 8, device, args.n_layer, args.kv_cache_dtype,
                            args.batch_size, args.kv_page_size, args.kv_num_pages, args.sliding_window)
        prompt = torch.randint(0, cfg.vocab_size, (args.batch_size, args.prompt_len), device=device)
        lengths = None
        if args.prompt_lengths is not None:
            lengths = torch.tensor(args.prompt_lengths, dtype=torch.int64, device=device)
        if mode == "eager":
            fwd = model
        elif mode == "thunder":
            fwd = thunder.jit(model)
        else:
            from ..transforms.hipgraph import HipGraphTransform

            transforms = [HipGraphTransform()]
            if mode == "hipgraph_mxfp4":
                # 4-bit weights (OCP MXFP4, every linear incl. the LM head), bf16 activations
                from ..transforms.mxfp4_inference import MXFP4InferenceTransform

                transforms.insert(0, MXFP4InferenceTransform(skip=()))
            fwd = thunder.jit(model, transforms=transforms)

        def once():
            if sampling:  # every timed generation draws the same tokens
                torch.manual_seed(args.seed)
            return generate(model, prompt, args.new_tokens, forward=fwd, temperature=args.temperature,
                            top_k=args.top_k, top_p=args.top_p, prompt_lengths=lengths,
                            prefill_chunk=args.prefill_chunk)

    t0 = time.perf_counter()
    out = once()
    torch.cuda.synchronize()
    first = time.perf_counter() - t0
    for _ in range(args.warmup):
        once()
    torch.cuda.synchronize()
    times = []
    for _ in range(args.iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = once()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    ms = 1000 * sum(times) / len(times)
    res = {
        "metric": f"{args.model} {'sampled' if sampling else 'greedy'} generate latency ({args.new_tokens} new tokens, static KV cache)",
        "model_impl": "transformers.LlamaForCausalLM" if mode.startswith("hf_") else "lightning_thunder_amd litgpt GPT",
        "mode": mode, "value": round(ms, 2), "unit": "ms", "higher_is_better": False,
        "ms_per_token": round(ms / args.new_tokens, 3), "first_call_s": round(first, 2),
        "prompt_len": args.prompt_len, "new_tokens": args.new_tokens, "batch_size": args.batch_size,
        "prompt_lengths": args.prompt_lengths, "prefill_chunk": None if mode.startswith("hf_") else args.prefill_chunk,
        "kv_cache_dtype": "model" if mode.startswith("hf_") else args.kv_cache_dtype,
        "dtype": "mxfp4 weights, bf16 activations" if mode.endswith("mxfp4") else "bf16",
        "data": "synthetic prompt, random-init weights", "n_gpus": 1,
        "reference_ms": {"thunder+cudagraphs (1xH100)": 542, "eager (1xH100)": 1493},
    }
    if not mode.startswith("hf_"):
        caches = [b.attn.kv_cache for b in model.transformer.h]
        res["kv_cache_gib"] = round(sum(t.numel() * t.element_size() for c in caches for t in c.buffers()) / 2 ** 30, 3)
        pages = model.kv_pages
        res.update(kv_page_size=args.kv_page_size, kv_num_pages=None if pages is None else pages.num_pages,
                   kv_pages_in_use=None if pages is None else pages.pages_in_use,
                   kv_pages_peak=None if pages is None else pages.peak_pages_in_use,  # of the last generation
                   sliding_window=cfg.sliding_window_size)
    if sampling:
        res.update(temperature=args.temperature, top_k=args.top_k, top_p=args.top_p, seed=args.seed)
    first_new = args.prompt_lengths[0] if args.prompt_lengths and not mode.startswith("hf_") else out.shape[1] - args.new_tokens
    res["tokens"] = out[0, first_new:first_new + args.new_tokens].tolist()
    return res


def _prefix_match(a, b) -> int:
    n = 0
    for x, y in zip(a, b):
        if x != y:
            break
        n += 1
    return n


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--model", default="Llama-3.2-1B")
    p.add_argument("--prompt-len", type=int, default=16)
    p.add_argument("--new-tokens", type=int, default=100)
    p.add_argument("--iters", type=int, default=3)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--modes", default="eager,thunder,hipgraph")
    p.add_argument("--n-layer", type=int, default=None, help="debug only")
    p.add_argument("--temperature", type=float, default=0.0, help="> 0: sample (LitGPT modes only) instead of greedy")
    p.add_argument("--top-k", type=int, default=None)
    p.add_argument("--top-p", type=float, default=None)
    p.add_argument("--kv-cache-dtype", choices=sorted(KV_CACHE_FORMATS), default="model",
                   help="LitGPT modes: 'fp8' keeps the static KV cache as unscaled e4m3 (half the bytes), "
                        "'fp8-row' as e4m3 with one power-of-two scale byte per (token, kv head) row")
    p.add_argument("--seed", type=int, default=0, help="torch.manual_seed before every sampled generation")
    p.add_argument("--batch-size", type=int, default=1, help="LitGPT modes: sequences per generation")
    p.add_argument("--prompt-lengths", default=None,
                   help="LitGPT modes: a,b,c,... one prompt length per sequence (a ragged batch, right-padded to the "
                        "longest, which replaces --prompt-len); --batch-size must match")
    p.add_argument("--kv-page-size", type=int, default=None,
                   help="LitGPT modes: a power of two >= 16: a paged KV cache (pools of pages and a block table) "
                        "instead of the static one")
    p.add_argument("--kv-num-pages", type=int, default=None,
                   help="pages per pool of a paged cache (default: what the static cache would hold)")
    p.add_argument("--prefill-chunk", type=int, default=None,
                   help="LitGPT modes: run the prompt in slices of at most this many columns at 2-D positions "
                        "(generate(prefill_chunk=...))")
    p.add_argument("--sliding-window", type=int, default=None,
                   help="LitGPT modes: a sliding window of this many keys on every layer (overrides the model's config); "
                        "with a paged cache generate() hands the pages below the window back to the pool")
    args = p.parse_args(argv)
    if args.sliding_window is not None and args.sliding_window < 1:
        p.error("--sliding-window must be >= 1")
    if args.kv_num_pages is not None and args.kv_page_size is None:
        p.error("--kv-num-pages needs --kv-page-size")
    if args.prefill_chunk is not None and args.prefill_chunk < 1:
        p.error("--prefill-chunk must be >= 1")
    if args.kv_page_size is not None and any(m.startswith("hf_") for m in args.modes.split(",")):
        p.error("--kv-page-size is for the LitGPT modes")
    if args.prompt_lengths is not None:
        try:
            args.prompt_lengths = [int(x) for x in args.prompt_lengths.split(",")]
        except ValueError:
            p.error("--prompt-lengths takes comma-separated integers")
        if len(args.prompt_lengths) != args.batch_size or min(args.prompt_lengths) < 1:
            p.error("--prompt-lengths needs one positive length per sequence of --batch-size")
        if any(m.startswith("hf_") for m in args.modes.split(",")):
            p.error("--prompt-lengths is for the LitGPT modes")
        args.prompt_len = max(args.prompt_lengths)
    elif args.batch_size != 1 and any(m.startswith("hf_") for m in args.modes.split(",")):
        p.error("--batch-size is for the LitGPT modes")
    results = []
    ref = {}  # model family -> tokens of its eager mode
    for mode in args.modes.split(","):
        r = run(mode, args)
        fam = "hf" if mode.startswith("hf_") else "litgpt"
        if mode in ("eager", "hf_eager"):
            ref[fam] = r["tokens"]
        if fam in ref and "temperature" not in r:  # sampled runs draw from different streams: no such check
            # greedy decoding of a random-init model: logits are nearly flat, so one bf16 rounding
            # difference flips an argmax and the continuation diverges; the leading tokens that agree
            # with eager are the numerics check
            r["prefix_match_vs_eager"] = _prefix_match(r["tokens"], ref[fam])
        r["tokens"] = r["tokens"][:8]
        results.append(r)
        print(json.dumps(r), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
