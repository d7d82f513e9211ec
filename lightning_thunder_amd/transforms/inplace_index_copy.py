"""In-place ``index_copy`` for static caches (parity: reference ``thunder/recipes/hf_transformers.py``
``InplaceIndexCopyTransform`` :26-97).

Functionalization turns ``cache.index_copy_(dim, pos, new)`` into a functional
``t = index_copy(cache, dim, pos, new)`` plus a write-back ``copy_(t, cache)`` at the end of the
program.  For a KV cache that copies the *whole* cache twice per layer per token.  When the cache
is not read between the update and the write-back (other than through ``t``) and nothing is
differentiated through it, the pair is replaced by one in-place ``index_copy_`` whose output
aliases the cache: O(tokens) instead of O(cache) HBM traffic per step.

The batched write of a ragged batch is treated the same way: ``cache.scatter_(2, pos[:, None, :, None]
.expand_as(src), src)`` (``pos`` int64 ``[B, T]``, one cache row per token) arrives as ``t = scatter(cache, 2,
idx, src)`` plus the write-back and becomes one ``scatter_rows_inplace(cache, pos, src)``.
"""
from __future__ import annotations

import torch

from ..core import prims
from ..core.prims import PrimIDs, OpTags
from ..core.proxies import TensorProxy
from ..core.symbol import Symbol, register_symbol
from ..core.trace import TraceCtx, from_trace, TraceProvenance
from ..core.transform_common import Transform


def _meta(buf, dim, index, src):
    return TensorProxy(like=buf)


index_copy_inplace = Symbol("index_copy_inplace", _meta, id="lta.index_copy_inplace", is_prim=True,
                            tags=(OpTags.DONT_DCE, OpTags.IN_PLACE))
index_copy_inplace.written_args = (0,)
register_symbol(index_copy_inplace)


def _rows_meta(buf, pos, src):
    return TensorProxy(like=buf)


# buf[b, :, pos[b, t], :] = src[b, :, t, :] in place (ops/kv_rows.py write_rows)
scatter_rows_inplace = Symbol("scatter_rows_inplace", _rows_meta, id="lta.scatter_rows_inplace", is_prim=True,
                              tags=(OpTags.DONT_DCE, OpTags.IN_PLACE))
scatter_rows_inplace.written_args = (0,)
register_symbol(scatter_rows_inplace)


def _impl(buf, dim, index, src):
    return buf.index_copy_(dim, index, src)


def _rows_impl(buf, pos, src):
    from ..ops.kv_rows import write_rows

    return write_rows(buf, pos, src)


def _register():
    from ..executors import torchex

    op = torchex.ex.register_operator("index_copy_inplace", like=index_copy_inplace, fn=_impl)
    torchex.ex.register_implementation(index_copy_inplace, op)
    op = torchex.ex.register_operator("scatter_rows_inplace", like=scatter_rows_inplace, fn=_rows_impl)
    torchex.ex.register_implementation(scatter_rows_inplace, op)


_register()

_INDEX_COPY_IDS = {"auto.torch.TensorBase.index_copy", "auto.torch.index_copy", "torch.index_copy"}


def _is_index_copy(b) -> bool:
    return b.sym.id in _INDEX_COPY_IDS or b.sym.name in ("index_copy",)


_SCATTER_IDS = {"torch.scatter", "auto.torch.TensorBase.scatter", "auto.torch.scatter"}
_ROW_KEY = (slice(None), None, slice(None), None)


def _row_positions(bsyms, producers, b):
    """``(buf, pos, src)`` when ``b`` is ``scatter(buf, 2, pos[:, None, :, None].expand_as(src), src)`` with
    ``pos`` int64 ``[B, T]``, ``buf`` ``[B, H, S, D]`` and ``src`` ``[B, H, T, D]``, else None."""
    if b.sym.id not in _SCATTER_IDS and b.sym.name != "scatter":
        return None
    args = list(b.args) + [b.kwargs[k] for k in ("dim", "index", "src") if k in b.kwargs]
    if len(args) != 4 or b.kwargs.get("value") is not None or b.kwargs.get("reduce") is not None:
        return None
    buf, dim, idx, src = args
    if not all(isinstance(t, TensorProxy) for t in (buf, idx, src)) or buf.ndim != 4 or dim not in (2, -2):
        return None
    if tuple(idx.shape) != tuple(src.shape) or src.ndim != 4 or src.dtype != buf.dtype:
        return None
    if tuple(src.shape[:2]) != tuple(buf.shape[:2]) or src.shape[3] != buf.shape[3]:
        return None
    e = producers.get(idx.name)
    if e is None or bsyms[e].sym.name not in ("expand_as", "expand") or not isinstance(bsyms[e].args[0], TensorProxy):
        return None
    col = bsyms[e].args[0]
    g = producers.get(col.name)
    if g is None or bsyms[g].sym.id != "torch.Tensor.__getitem__" or len(bsyms[g].args) != 2:
        return None
    pos, key = bsyms[g].args
    if not isinstance(pos, TensorProxy) or not isinstance(key, tuple) or tuple(key) != _ROW_KEY:
        return None
    if pos.dtype != torch.int64 or tuple(pos.shape) != (src.shape[0], src.shape[2]):
        return None
    return buf, pos, src


def inplace_index_copy(trace: TraceCtx) -> TraceCtx:
    """Rewrites ``t = index_copy(buf, ...)`` + ``copy_(t, buf)`` into ``t = index_copy_inplace(buf, ...)``, and
    ``t = scatter(buf, 2, <pos per row>, src)`` + ``copy_(t, buf)`` into ``t = scatter_rows_inplace(buf, pos, src)``."""
    bsyms = list(trace.bound_symbols)
    producers: dict[str, int] = {}
    for i, b in enumerate(bsyms):
        for o in b.flat_proxy_outs:
            producers.setdefault(o.name, i)
    arg_names = {a.name for a in trace.args if isinstance(a, TensorProxy)}
    consumers: dict[str, list[int]] = {}
    for i, b in enumerate(bsyms):
        for a in b.flat_proxy_args:
            consumers.setdefault(a.name, []).append(i)
    drop: set[int] = set()
    replace: dict[int, object] = {}
    for i, b in enumerate(bsyms):
        rows = _row_positions(bsyms, producers, b)
        if rows is not None:
            buf, pos, src = rows
        elif not _is_index_copy(b) or len(b.args) < 4 and not b.kwargs:
            continue
        else:
            args = list(b.args) + [b.kwargs.get(k) for k in ("dim", "index", "source") if k in b.kwargs]
            if len(args) != 4:
                continue
            buf, dim, index, src = args
        out = b.output
        if not (isinstance(buf, TensorProxy) and isinstance(out, TensorProxy) and buf.name in arg_names):
            continue
        if buf.requires_grad:
            continue
        # the write-back of the functional result into the buffer
        wb = [j for j in consumers.get(out.name, []) if bsyms[j].sym.id == PrimIDs.COPY_
              and bsyms[j].args[0] is not None and bsyms[j].args[0].name == out.name
              and isinstance(bsyms[j].args[1], TensorProxy) and bsyms[j].args[1].name == buf.name]
        if len(wb) != 1:
            continue
        j = wb[0]
        # no other reader of the old buffer value after the update
        others = [k for k in consumers.get(buf.name, []) if k > i and k != j]
        if others:
            continue
        if rows is not None:
            replace[i] = scatter_rows_inplace.bind(buf, pos, src, output=out)
        else:
            replace[i] = index_copy_inplace.bind(buf, dim, index, src, output=out)
        drop.add(j)
        # any consumer of the copy_ output is re-pointed at the in-place result
        cj = bsyms[j].output
        if isinstance(cj, TensorProxy) and consumers.get(cj.name):
            drop.discard(j)
            replace.pop(i)
    if not replace:
        return trace
    # the index tensors of the batched writes (expand_as, then pos[:, None, :, None]) when nothing reads them now
    for i in sorted(replace, reverse=True):
        if replace[i].sym is not scatter_rows_inplace:
            continue
        t = bsyms[i].args[2] if len(bsyms[i].args) > 2 else bsyms[i].kwargs["index"]
        for _ in range(2):
            j = producers[t.name]
            if any(k not in drop and k not in replace for k in consumers.get(t.name, [])):
                break
            drop.add(j)
            t = bsyms[j].args[0]
    new = from_trace(trace)
    new.bound_symbols = [replace.get(i, b) for i, b in enumerate(bsyms) if i not in drop]
    new.set_provenance(TraceProvenance(f"In-place index_copy ({len(replace)} cache updates)"))
    return new


class InplaceIndexCopyTransform(Transform):
    """``transform_traces_pre_prologue`` hook running :func:`inplace_index_copy` (use for programs
    that are not differentiated; ``jit`` already applies the pass to every no-grad program)."""

    def transform_traces_pre_prologue(self, prologue_trace, computation_trace, epilogue_trace, **kwargs):
        return prologue_trace, inplace_index_copy(computation_trace), epilogue_trace
