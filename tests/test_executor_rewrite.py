"""The rewrite helper the hipex post-claim passes are written on (executors/rewrite.py)."""
import torch

from lightning_thunder_amd import torch as lt
from lightning_thunder_amd.core import prims
from lightning_thunder_amd.core.proxies import TensorProxy
from lightning_thunder_amd.core.trace import TraceCtx, tracectx
from lightning_thunder_amd.executors import hipex
from lightning_thunder_amd.executors.rewrite import Rewrite, operands


def _program():
    trace = TraceCtx()
    with tracectx(trace):
        x, w, r, y, z = (TensorProxy(name=n, shape=s, device="cuda", dtype=torch.bfloat16)
                         for n, s in (("x", (1, 256)), ("w", (512, 256)), ("r", (1, 512)), ("y", (1, 512)), ("z", (1, 512))))
    trace.bound_symbols += [hipex.hip_decode_linear.bind(x, w, residual=r, output=y), lt.mul.bind(y, y, output=z),
                            prims.python_return.bind(z, y, output=None)]
    return trace, (x, w, r, y, z)


def test_operands_by_parameter_name():
    trace, (x, w, r, y, z) = _program()
    b = trace.bound_symbols[0]
    assert operands(b) == dict(x=x, w=w, bias=None, residual=r, act=None, gate_weight=None, norm=False, norm_weight=None,
                               eps=1e-5)
    assert operands(b, ("x", "q", "s")) == dict(x=x, q=w, s=None)


def test_lookups_and_finish():
    trace, (x, w, r, y, z) = _program()
    rw = Rewrite(trace, hipex.ex)
    assert rw.producer(y) == 0 and rw.producer(x) is None and rw.producer(None, -1) == -1
    assert rw.consumers(y) == [1, 1, 2] and rw.uses(y) == 3 and rw.uses(z) == 1  # the return reads, too
    assert rw.finish("nothing") is trace
    rw.replace(1, hipex.hip_swiglu.bind(y, y, output=z))
    rw.drop(0)
    assert rw.touched(0) and rw.touched(1) and rw.dropped(0) and not rw.dropped(1) and not rw.touched(2)
    new = rw.finish("hipex: test")
    assert [b.sym.name for b in new.bound_symbols] == ["hip_swiglu", "python_return"]
    assert new.bound_symbols[0]._call_ctx and new.scopes == [new.bound_symbols]
    assert str(new.get_provenance().pss) == "hipex: test" and len(trace.bound_symbols) == 3
