"""Runtime-sized (symbolic) hipfuse regions against their static-shape twins and against the per-op ATen chain
a ``cache="symbolic values"`` program ran before symbolic regions existed.

Cases: bias + GELU(tanh) at [8, 1024, 4096] bf16 (pointwise mode) and a row softmax (over a biased input, the
bias parameter pins the reduced extent) at [8192, 1024] bf16 (row mode).  Per case:

  (i)   the static-shape region's kernel,
  (ii)  the symbolic region's kernel,
  (iii) the same program under symbolic values on the torch executor alone (one ATen launch per op),

each as device time per call from batches of back-to-back calls rotating over input copies totalling >= 1 GB
(no Infinity Cache hits), median of 7 batches; and the host time of one ``HipFusion.__call__`` of a static and of
a symbolic region (small tensors, wall clock over 2000 calls, the queue drained afterwards).

    python scripts/hipfuse_symbolic_bench.py [--out FILE]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import lightning_thunder_amd as thunder
from lightning_thunder_amd.executors import hipfuse
from lightning_thunder_amd.executors import hipfuse_codegen as cg


class BiasGelu(torch.nn.Module):
    def __init__(self, C):
        super().__init__()
        self.b = torch.nn.Parameter(torch.randn(C, device="cuda", dtype=torch.bfloat16))

    def forward(self, x):
        return torch.nn.functional.gelu(x + self.b, approximate="tanh")


class BiasSoftmax(torch.nn.Module):
    def __init__(self, C):
        super().__init__()
        self.b = torch.nn.Parameter(torch.randn(C, device="cuda", dtype=torch.bfloat16))

    def forward(self, x):
        return torch.softmax(x + self.b, -1)


def per_call_us(fn, copies, reps=7):
    fn(copies[0])
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for c in copies:
            fn(c)
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3 / len(copies))
    ts.sort()
    return ts[len(ts) // 2]


def region(jm):
    (fb,) = hipfuse.fusions(thunder.last_traces(jm)[-1])
    return fb._call_ctx[fb.sym.name]


def kernel_call(hf, m):
    """One launch of region ``hf``'s kernel for the input it is called with (the output is reused)."""
    state = {}

    def run(x):
        tensors = [m.b if len(p.shape) == 1 else x for p in (hf.inputs[i] for i in hf.tensor_pos)]
        if "ks" not in state:
            state["out"] = torch.empty_like(x)
            if hf.symbolic:
                key, ext, words, D = cg.sym_call(hf.plan, [(t.shape, t.stride(), True) for t in tensors])
                fns, ks = hf._variant(tensors, (), key)
                state.update(tail=ext + words, grid=(cg.sym_grid(ks.sym_mode, D, hf.plan.red), 1, 1))
            else:
                fns, ks = hf._variant(tensors)
                state.update(tail=None, grid=None)
            state.update(ks=ks, fns=fns)
        hipfuse.launch(state["ks"], state["fns"], tensors, [state["out"]], [], tail=state["tail"], grid=state["grid"])

    return run, state


def host_us(hf, args, n=2000):
    for _ in range(50):
        hf(*args)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        hf(*args)
    dt = time.perf_counter() - t0
    torch.cuda.synchronize()
    return dt / n * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the table to this file")
    args = ap.parse_args()
    lines = ["hipfuse symbolic regions, MI355X, bf16; device us per call (median of 7 batches over rotating copies)", ""]
    host = []
    for name, mod, shape in (("bias+gelu(tanh) [8,1024,4096]", BiasGelu(4096), (8, 1024, 4096)),
                             ("row softmax(x+b) [8192,1024]", BiasSoftmax(1024), (8192, 1024))):
        x = torch.randn(*shape, device="cuda", dtype=torch.bfloat16)
        nbytes = 2 * x.numel() * 2
        copies = [x.clone() for _ in range(max(2, min(64, -(-int(1e9) // (nbytes // 2)))))]
        jit_static = thunder.jit(mod, executors=["hipfuse", "torch"])
        jit_sym = thunder.jit(mod, executors=["hipfuse", "torch"], cache="symbolic values")
        jit_aten = thunder.jit(mod, executors=["torch"], cache="symbolic values")
        with torch.no_grad():
            ref = jit_static(x)
            assert torch.equal(jit_sym(x), ref), "symbolic region differs from the static one"
            jit_aten(x)
            hs, hy = region(jit_static), region(jit_sym)
            assert hy.symbolic and not hs.symbolic
            run_s, st_s = kernel_call(hs, mod)
            run_y, st_y = kernel_call(hy, mod)
            t_static = per_call_us(run_s, copies)
            t_sym = per_call_us(run_y, copies)
            t_aten = per_call_us(jit_aten, copies)
            small = torch.randn(*((2, 8, shape[-1]) if len(shape) == 3 else (16, shape[-1])), device="cuda", dtype=torch.bfloat16)
            jit_static(small), jit_sym(small)
            hs2, hy2 = region(jit_static), region(jit_sym)
            order = lambda hf: [mod.b if len(p.shape) == 1 else small for p in hf.inputs]
            host.append((name, host_us(hs2, order(hs2)), host_us(hy2, order(hy2))))
        lines += [name,
                  f"  (i)   static region    {t_static:9.2f} us  {nbytes / t_static / 1e6:6.2f} TB/s  {st_s['ks'].mode} vec={st_s['ks'].vec}",
                  f"  (ii)  symbolic region  {t_sym:9.2f} us  {nbytes / t_sym / 1e6:6.2f} TB/s  {st_y['ks'].mode} vec={st_y['ks'].vec}"
                  f"  ({(t_sym / t_static - 1) * 100:+.1f} % vs (i))",
                  f"  (iii) per-op ATen      {t_aten:9.2f} us  ((ii) is {t_aten / t_sym:.2f}x faster)", ""]
        del copies
    lines.append("host us per HipFusion.__call__ (small tensors, 2000 calls)")
    for name, a, b in host:
        lines.append(f"  {name:32s} static {a:6.2f}   symbolic {b:6.2f}")
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
