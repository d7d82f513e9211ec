"""The bookkeeping every peephole rewrite of a claimed trace needs: who produces a value, who reads it,
which positions are dropped or replaced, and the rebuilt trace at the end."""
from __future__ import annotations

import inspect
from functools import lru_cache

from ..core.trace import TraceProvenance, from_trace


@lru_cache(maxsize=None)
def _parameters(meta):
    return tuple((p.name, None if p.default is p.empty else p.default) for p in inspect.signature(meta).parameters.values())


def operands(bsym, names=None) -> dict:
    """The operands of ``bsym`` by parameter name, from its args and kwargs; parameters it does not pass
    take their default (None without one).  ``names`` spells the positional order of an operator whose
    meta does not (a traced custom op); otherwise it is read off the operator's meta function."""
    params = tuple((n, None) for n in names) if names is not None else _parameters(bsym.sym.meta)
    d = dict(params)
    d.update(zip((n for n, _ in params), bsym.args))
    d.update((k, v) for k, v in bsym.kwargs.items() if k in d)
    return d


class Rewrite:
    """One pass over ``trace``: look positions up, mark them with ``drop`` / ``replace``, then ``finish``."""

    def __init__(self, trace, executor):
        self.trace = trace
        self.executor = executor
        self.bsyms = list(trace.bound_symbols)
        self._producer: dict[str, int] = {}
        self._consumers: dict[str, list[int]] = {}
        for i, b in enumerate(self.bsyms):
            for a in b.flat_proxy_args:
                self._consumers.setdefault(a.name, []).append(i)
            for o in b.flat_proxy_outs:
                self._producer[o.name] = i
        self._dropped: set[int] = set()
        self._replaced: dict[int, object] = {}

    def producer(self, t, default=None):
        """The position that produces ``t`` (``default`` for a program input or a non-proxy)."""
        return self._producer.get(getattr(t, "name", None), default)

    def consumers(self, t) -> list[int]:
        """The positions that read ``t``, once per read; the return symbol is a reader like any other."""
        return self._consumers.get(t.name, [])

    def uses(self, t) -> int:
        return len(self.consumers(t))

    def touched(self, i) -> bool:
        return i in self._dropped or i in self._replaced

    def dropped(self, i) -> bool:
        return i in self._dropped

    def drop(self, *positions) -> None:
        self._dropped.update(positions)

    def replace(self, i, bsym) -> None:
        self._replaced[i] = self.executor.bind_call_ctx(bsym)

    @property
    def replaced(self) -> int:
        return len(self._replaced)

    def finish(self, message: str):
        """The trace itself if nothing was marked, else the rebuilt one with ``message`` as its provenance."""
        if not self._dropped and not self._replaced:
            return self.trace
        new = from_trace(self.trace)
        new.bound_symbols = [self._replaced.get(i, b) for i, b in enumerate(self.bsyms) if i not in self._dropped]
        new.scopes = [new.bound_symbols]
        new.set_provenance(TraceProvenance(message))
        return new
