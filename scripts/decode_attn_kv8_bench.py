"""The e4m3 KV cache against the bf16 one: the decode attention kernel, the cache-writing RoPE launch, and
``benchmarks/inference.py`` with and without ``--kv-cache-dtype fp8``.

    python scripts/decode_attn_kv8_bench.py [--parent-lib PATH] [--out profiles/decode_attn_kv8.txt] [--skip-models]

Part one: per shape one decode step's attention (T = 1, the model's all-true mask row) over a bf16 cache and
over an e4m3 cache of the same logical content, and with ``--parent-lib`` (the native library built from the
parent commit) the bf16 kernel of that build, to show what the K/V element-type template parameter cost the
16-bit instantiations.  Each version's launches are captured into a hipGraph of ``--batch`` back-to-back calls
(device time, no host gaps); the replays of the versions alternate, after warm-up, and a point is the median
of ``--batches`` replays / batch.  "spread" is max - min of the parent's bf16 kernel (of this build's when no
parent library is given) over its replays in the same run: the margin of the two conditions

    fp8 kernel <= parent bf16 kernel + spread        bf16 kernel <= parent bf16 kernel + spread

GB/s = the K and V bytes of the cache over the time (the stream the kernel exists for; q, o and the split-K
workspace are not counted).  The RoPE launch is timed the same way for both cache types.

Part two runs ``benchmarks.inference`` (hipgraph mode) in a fresh process per model and cache type, one after
the other, and reports TBOT, the bytes of the cache buffers and the allocator's held and peak bytes.
"""
import argparse
import ctypes
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

BF16, U8, F8 = torch.bfloat16, torch.uint8, torch.float8_e4m3fn
MODELS = {"Llama-2-7B": (32, 32, 128), "Llama-3.2-1B": (32, 8, 64)}  # Hq, Hkv, D


def parent_decode_attn(path):
    """``decode_attn`` of another build of the native library (the same wrapper code, its entry)."""
    from lightning_thunder_amd.ops import attention as A

    lib = ctypes.CDLL(os.path.abspath(path))
    lib.lta_decode_attn.argtypes = A.require().lta_decode_attn.argtypes
    lib.lta_decode_attn.restype = ctypes.c_int

    def run(q, k, v, mask):
        B, Hq, T, D = q.shape
        Hkv, S = k.shape[1], k.shape[2]
        mask = torch.broadcast_to(mask, (B, Hq, T, S))
        rows = B * Hq * T
        wsplit, nsplit, chunk = A.decode_launch_shape(rows, S)
        o = torch.empty((B, Hq, T, D), device=q.device, dtype=q.dtype)
        ws_acc = ws_ml = None
        if nsplit > 1:
            ws_acc = torch.empty((nsplit, rows, D), device=q.device, dtype=torch.float32)
            ws_ml = torch.empty((nsplit, rows, 2), device=q.device, dtype=torch.float32)
        st = (ctypes.c_int64 * 13)(*q.stride()[:3], *k.stride()[:3], *v.stride()[:3], *mask.stride())
        rc = lib.lta_decode_attn(A.dcode(q), A.ptr(q), A.ptr(k), A.ptr(v), mask.data_ptr(), A.ptr(o), A.ptr(ws_acc),
                                 A.ptr(ws_ml), B, Hq, Hkv, T, S, D, ctypes.cast(st, ctypes.c_void_p), chunk, nsplit, 0,
                                 1.0 / math.sqrt(D), int(wsplit), A.stream_ptr(q.device))
        A.check(rc, "parent lta_decode_attn")
        return o

    return run


def graphed(fn, batch):
    """A hipGraph of ``batch`` back-to-back calls of ``fn``; returns replay() -> us per call (device events)."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(batch):
            fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def replay():
        s.record()
        g.replay()
        e.record()
        e.synchronize()
        return s.elapsed_time(e) / batch * 1000

    return replay


def measure(versions, batch, batches):
    """{name: fn} -> {name: [us per call] per replay}, the versions alternating replay by replay, the order
    rotating from round to round (what a version finds in the caches depends on which one ran before it)."""
    replays = {n: graphed(f, batch) for n, f in versions.items()}
    for r in replays.values():
        for _ in range(3):
            r()
    out = {n: [] for n in versions}
    names = list(replays)
    for i in range(batches):
        for n in names[i % len(names):] + names[:i % len(names)]:
            out[n].append(replays[n]())
    return out


def fmt(ts):
    return f"{statistics.median(ts):8.2f} ({min(ts):.2f}..{max(ts):.2f})"


def part_one(args, lines):
    from lightning_thunder_amd.ops.attention import decode_attn, decode_attn_kv8
    from lightning_thunder_amd.ops.fused import qkv_rope_cache_fwd

    parent = parent_decode_attn(args.parent_lib) if args.parent_lib else None
    base = "parent bf16" if parent else "bf16"
    lines.append(f"decode attention, T = 1, us per launch: median (min..max) of {args.batches} graph replays of {args.batch} "
                 f"launches, versions alternating; spread = max - min of '{base}'")
    lines.append(f"{'model':<13} {'B':>2} {'S':>5} | {'bf16 us':>22} {'GB/s':>6} | {'fp8 us':>22} {'GB/s':>6} | "
                 f"{'parent bf16 us':>22} | {'spread':>6} | fp8 <= parent+spread | bf16 <= parent+spread | max|fp8-bf16|")
    failed = []
    torch.manual_seed(0)
    for model, (Hq, Hkv, D) in MODELS.items():
        for B in (1, 8):
            for S in (2048, 8192):
                k8 = (torch.randn(B, Hkv, S, D, device="cuda")).clamp(-448, 448).to(F8).view(U8)
                v8 = (torch.randn(B, Hkv, S, D, device="cuda")).clamp(-448, 448).to(F8).view(U8)
                k, v = k8.view(F8).to(BF16), v8.view(F8).to(BF16)  # the same logical cache
                q = torch.randn(B, Hq, 1, D, device="cuda").to(BF16)
                mask = torch.ones(1, 1, 1, S, dtype=torch.bool, device="cuda")
                versions = {"bf16": lambda: decode_attn(q, k, v, mask), "fp8": lambda: decode_attn_kv8(q, k8, v8, mask)}
                if parent:
                    versions["parent bf16"] = lambda: parent(q, k, v, mask)
                o16, o8 = versions["bf16"](), versions["fp8"]()
                diff = (o16.float() - o8.float()).abs().max().item()
                if parent:
                    assert torch.equal(o16, versions["parent bf16"]()), "the bf16 kernel no longer computes the parent's bits"
                t = measure(versions, args.batch, args.batches)
                ref = t[base]
                spread = max(ref) - min(ref)
                m16, m8, mp = (statistics.median(t[n]) for n in ("bf16", "fp8", base))
                ok8, ok16 = m8 <= mp + spread, m16 <= mp + spread
                gb16, gb8 = 2 * k.numel() * 2 / m16 / 1e3, 2 * k8.numel() / m8 / 1e3
                lines.append(f"{model:<13} {B:>2} {S:>5} | {fmt(t['bf16']):>22} {gb16:>6.0f} | {fmt(t['fp8']):>22} {gb8:>6.0f} | "
                             f"{(fmt(t['parent bf16']) if parent else 'not measured'):>22} | {spread:>6.2f} | "
                             f"{'yes' if ok8 else 'NO':>20} | {('yes' if ok16 else 'NO') if parent else 'n/a':>21} | {diff:.1e}")
                print(lines[-1], flush=True)
                if not ok8:
                    failed.append(f"fp8 {model} B={B} S={S}")
                if parent and not ok16:
                    failed.append(f"bf16 {model} B={B} S={S}")
    lines.append("shapes that miss their condition: " + ("; ".join(failed) if failed else "none"))
    lines.append("")
    lines.append("cache-writing RoPE launch (qkv split + RoPE + K/V rows into the cache), T = 1, position 2047 of 2048, us per launch")
    lines.append(f"{'model':<13} {'B':>2} | {'bf16 cache':>22} | {'e4m3 cache':>22}")
    for model, (Hq, Hkv, D) in MODELS.items():
        for B in (1, 8):
            qkv = torch.randn(B, 1, (Hq + 2 * Hkv) * D, device="cuda").to(BF16)
            cos, sin = torch.rand(1, D, device="cuda"), torch.rand(1, D, device="cuda")
            pos = torch.tensor([2047], device="cuda")
            c16 = [torch.zeros(B, Hkv, 2048, D, device="cuda", dtype=BF16) for _ in range(2)]
            c8 = [torch.zeros(B, Hkv, 2048, D, device="cuda", dtype=U8) for _ in range(2)]
            t = measure({"bf16": lambda: qkv_rope_cache_fwd(qkv, cos, sin, Hq, Hkv, D, D, *c16, pos),
                         "fp8": lambda: qkv_rope_cache_fwd(qkv, cos, sin, Hq, Hkv, D, D, *c8, pos)}, args.batch, args.batches)
            assert torch.equal(c8[0][:, :, 2047], c16[0][:, :, 2047].clamp(-448, 448).to(F8).view(U8))
            lines.append(f"{model:<13} {B:>2} | {fmt(t['bf16']):>22} | {fmt(t['fp8']):>22}")
            print(lines[-1], flush=True)


def part_two(args, lines):
    import gc
    import json
    import subprocess

    gc.collect()
    torch.cuda.empty_cache()  # the children below get the device to themselves but for this process' context
    lines.append("")
    lines.append(f"benchmarks/inference.py, hipgraph mode, one fresh process per row, {args.input_length} in / "
                 f"{args.output_length} out, {args.iterations} iterations after {args.warmup} warm-up: TBOT ms mean / median / "
                 "p90; GiB of the KV cache buffers, of torch.cuda.memory_allocated after the last step, and of the process' "
                 "torch.cuda.max_memory_allocated (the 7B peak is the model's construction, before any cache exists)")
    lines.append(f"{'model':<14} {'B':>2} {'kv cache':>8} | {'TBOT mean':>9} {'median':>7} {'p90':>7} | {'TTFT ms':>8} | "
                 f"{'cache GiB':>9} {'held GiB':>8} {'peak GiB':>8}")
    for model, B in (("Llama-2-7b-hf", 1), ("Llama-3.2-1B", 8)):
        for kv in ("model", "fp8"):
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
                         f"{r['ttft_ms']['median']:>8.2f} | {r['kv_cache_gib']:>9.3f} {r['memory_allocated_gib']:>8.3f} "
                         f"{r['max_memory_allocated_gib']:>8.3f}")
            print(lines[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_attn_kv8.txt"))
    ap.add_argument("--parent-lib", default=None, help="the native library built from the parent commit")
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--batches", type=int, default=21)
    ap.add_argument("--skip-models", action="store_true", help="part one only")
    ap.add_argument("--input-length", type=int, default=2048)
    ap.add_argument("--output-length", type=int, default=64)
    ap.add_argument("--iterations", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("decode_attn_kv8_bench needs the GPU: a CPU timing says nothing about it")
    lines = [f"e4m3 KV cache vs bf16 KV cache, {torch.cuda.get_device_name(0)}", ""]

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
