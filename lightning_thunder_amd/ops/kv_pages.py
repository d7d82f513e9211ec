"""The paged KV cache in plain torch: a pool of fixed-size pages per layer and one block table per model.

A static cache holds ``B x max_seq`` rows per layer whatever the sequences hold; a paged one holds the pages
the sequences have been given.  The functions here are the definition the kernels follow
(``csrc/decode_attention.hip`` paged mode reads through the table, ``csrc/rope.hip`` per-row mode writes at
``page_slots``).

**Pool.**  Every K and V buffer is ``[n_query_groups, R + 1, head_size]`` with ``R = num_pages * page_size``:
physical page ``p`` is rows ``p * page_size .. (p + 1) * page_size - 1`` of every head.  Row ``R`` is a sink: a
token without a page is written there by the torch path (the kernels write nothing for it) and nothing ever
reads it.  The scaled e4m3 format (``ops/kv8.py``) adds scale pools ``[n_query_groups, R + 1, 1]``, uint8,
initialised to 127.

**Block table.**  int64 ``[B, max_pages]`` on the device, shared by all layers: ``table[b, i]`` is the physical
page that holds positions ``i * page_size .. (i + 1) * page_size - 1`` of sequence b, ``-1`` for "no page".  The
logical capacity is ``S = max_pages * page_size``; ``page_size`` is a power of two, at least 16.

``page_slots``, ``gather_pages`` and ``paged_mask`` are also ``torch.library`` custom ops (``lta::kv_page_slots``,
``lta::kv_paged_gather``, ``lta::kv_paged_mask``), so a traced program holds each as one symbol that the HIP
executor can drop once the kernels take the table themselves.
"""
from __future__ import annotations

import heapq
from typing import Optional, Sequence

import torch

MIN_PAGE_SIZE = 16


def check_page_size(page_size: int) -> int:
    """``page_size`` as an int when it is a power of two >= 16, else ``ValueError``."""
    if isinstance(page_size, bool) or not isinstance(page_size, int) or page_size < MIN_PAGE_SIZE \
            or page_size & (page_size - 1):
        raise ValueError(f"KV cache: page_size must be a power of two >= {MIN_PAGE_SIZE}, got {page_size!r}")
    return page_size


def page_slots(table: torch.Tensor, pos: torch.Tensor, page_size: int, R: int) -> torch.Tensor:
    """int64 ``[B, T]``: the physical pool row of token (b, t) at position ``pos[b, t]``,
    ``table[b, pos // page_size] * page_size + pos % page_size``; ``R`` (the sink row) when ``pos`` is outside
    ``[0, S)`` or the table entry is outside ``[0, R // page_size)``."""
    S = table.shape[1] * page_size
    num_pages = R // page_size
    inside = (pos >= 0) & (pos < S)
    p = pos.clamp(0, S - 1)
    pid = table.gather(1, torch.div(p, page_size, rounding_mode="floor"))
    ok = inside & (pid >= 0) & (pid < num_pages)
    return torch.where(ok, pid * page_size + p % page_size, torch.full_like(p, R))


def gather_pages(pool: torch.Tensor, table: torch.Tensor, page_size: int) -> torch.Tensor:
    """``[B, H, S, D]``: the logical cache of every sequence out of ``pool`` ``[H, R + 1, D]``.  A table entry
    outside ``[0, num_pages)`` reads page 0 (the last page when too large); ``paged_mask`` hides its keys."""
    B, P = table.shape
    H, rows, D = pool.shape
    num_pages = (rows - 1) // page_size
    pid = table.clamp(0, max(num_pages - 1, 0))
    r = (pid[:, :, None] * page_size + torch.arange(page_size, device=table.device)).reshape(-1)
    return pool.index_select(1, r).view(H, B, P * page_size, D).transpose(0, 1)


def paged_mask(pos: torch.Tensor, table: torch.Tensor, page_size: int, num_pages: Optional[int] = None) -> torch.Tensor:
    """bool ``[B, 1, T, S]``: ``mask[b, 0, t, j] = j <= pos[b, t] and 0 <= table[b, j // page_size] < num_pages``
    (without ``num_pages`` only the lower bound is checked)."""
    live = table >= 0
    if num_pages is not None:
        live = live & (table < num_pages)
    live = live.repeat_interleave(page_size, dim=1)  # [B, S]
    j = torch.arange(live.shape[1], device=pos.device)
    return (j <= pos[:, None, :, None]) & live[:, None, None, :]


def paged_window_mask(pos: torch.Tensor, table: torch.Tensor, page_size: int, num_pages: Optional[int],
                      window: int) -> torch.Tensor:
    """bool ``[B, 1, T, S]``: ``paged_mask`` under a sliding window, and-ed with ``j > pos[b, t] - window`` (``window``
    keys, the token's own included: the Mistral / HF convention).  A page wholly below every row's window may hold
    any table entry: its keys are hidden either way, which is what lets ``PageTable.trim`` take it back."""
    j = torch.arange(table.shape[1] * page_size, device=pos.device)
    return paged_mask(pos, table, page_size, num_pages) & (j > pos[:, None, :, None] - window)


def write_slots(pool: torch.Tensor, slots: torch.Tensor, src: torch.Tensor) -> torch.Tensor:
    """``pool[:, slots[b, t], :] = src[b, :, t, :]`` in place (pool ``[H, R + 1, D]``, src ``[B, H, T, D]``, slots
    int64 ``[B, T]``): the ``[H, B * T, D]`` relayout, then one ``index_copy_`` along the rows.  Returns ``pool``."""
    B, H, T, D = src.shape
    return pool.index_copy_(1, slots.reshape(-1), src.permute(1, 0, 2, 3).reshape(H, B * T, D))


@torch.library.custom_op("lta::kv_page_slots", mutates_args=())
def kv_page_slots(table: torch.Tensor, pos: torch.Tensor, page_size: int, R: int) -> torch.Tensor:
    return page_slots(table, pos, page_size, R)


@kv_page_slots.register_fake
def _kv_page_slots_fake(table, pos, page_size, R):
    return pos.new_empty(pos.shape, dtype=torch.int64)


@torch.library.custom_op("lta::kv_paged_gather", mutates_args=())
def kv_paged_gather(pool: torch.Tensor, table: torch.Tensor, page_size: int) -> torch.Tensor:
    return gather_pages(pool, table, page_size)


@kv_paged_gather.register_fake
def _kv_paged_gather_fake(pool, table, page_size):
    B, P = table.shape
    return pool.new_empty((B, pool.shape[0], P * page_size, pool.shape[2]))


@torch.library.custom_op("lta::kv_paged_mask", mutates_args=())
def kv_paged_mask(pos: torch.Tensor, table: torch.Tensor, page_size: int, num_pages: int) -> torch.Tensor:
    return paged_mask(pos, table, page_size, num_pages)


@kv_paged_mask.register_fake
def _kv_paged_mask_fake(pos, table, page_size, num_pages):
    B, T = pos.shape
    return pos.new_empty((B, 1, T, table.shape[1] * page_size), dtype=torch.bool)


@torch.library.custom_op("lta::kv_paged_window_mask", mutates_args=())
def kv_paged_window_mask(pos: torch.Tensor, table: torch.Tensor, page_size: int, num_pages: int,
                         window: int) -> torch.Tensor:
    return paged_window_mask(pos, table, page_size, num_pages, window)


@kv_paged_window_mask.register_fake
def _kv_paged_window_mask_fake(pos, table, page_size, num_pages, window):
    B, T = pos.shape
    return pos.new_empty((B, 1, T, table.shape[1] * page_size), dtype=torch.bool)


class PageTable:
    """The host-side allocator of a paged cache; it owns the device block table ``table`` (int64
    ``[batch_size, max_pages]``, ``-1`` = no page).

    The allocator works from host-side lengths only and synchronises nothing.  The device table is updated in
    place, at a fixed address, so a captured decode step keeps replaying while sequences grow.

    Under a sliding window a sequence gives its lowest pages back (``trim``): it then holds the table indices
    ``first .. end - 1``, the entries below ``first`` are ``-1`` again and stay so until ``release``."""

    def __init__(self, batch_size: int, max_pages: int, page_size: int, num_pages: int, device=None):
        self.page_size = check_page_size(page_size)
        if batch_size < 1 or max_pages < 1 or num_pages < 1:
            raise ValueError(f"PageTable: batch_size, max_pages and num_pages must be positive, got {batch_size}, "
                             f"{max_pages}, {num_pages}")
        self.batch_size, self.max_pages, self.num_pages = batch_size, max_pages, num_pages
        self.table = torch.full((batch_size, max_pages), -1, dtype=torch.int64, device=device)
        self._host = torch.full((batch_size, max_pages), -1, dtype=torch.int64)
        self._held = [0] * batch_size  # every sequence's table index past its last page
        self._first = [0] * batch_size  # and that of its first page: the indices below it were trimmed
        self.peak_pages_in_use = 0  # the most pages out at once since the last reset()
        self._free = list(range(num_pages))  # a heap: the lowest free page goes out first

    @property
    def rows(self) -> int:
        """``R``: the pool rows that pages cover (the sink row follows them)."""
        return self.num_pages * self.page_size

    @property
    def capacity(self) -> int:
        """``S``: the positions a sequence can hold."""
        return self.max_pages * self.page_size

    @property
    def pages_in_use(self) -> int:
        return self.num_pages - len(self._free)

    def pages_of(self, b: int) -> list[int]:
        return self._host[b, self._first[b]:self._held[b]].tolist()

    def reserve(self, lengths: Sequence[int]) -> None:
        """Gives every sequence pages up to table index ``ceil(lengths[b] / page_size)``, lowest free page first.  A
        page a sequence already has never moves, a sequence keeps pages beyond its length, and a table index that
        ``trim`` emptied gets no page again.  ``ValueError`` for a length beyond
        ``max_pages`` pages, ``RuntimeError`` when the pool has too few free pages; neither changes anything."""
        lengths = [int(n) for n in (lengths.tolist() if isinstance(lengths, torch.Tensor) else lengths)]
        if len(lengths) != self.batch_size:
            raise ValueError(f"PageTable.reserve: {len(lengths)} lengths for a batch of {self.batch_size}")
        want = [max(-(-n // self.page_size), held) for n, held in zip(lengths, self._held)]
        if max(want) > self.max_pages:
            raise ValueError(f"PageTable.reserve: a length of {max(lengths)} needs {max(want)} pages, the table "
                             f"holds {self.max_pages} per sequence ({self.capacity} positions)")
        needed = sum(want) - sum(self._held)
        if needed > len(self._free):
            raise RuntimeError(f"PageTable.reserve: the pool is exhausted: {needed} more page(s) needed, "
                               f"{len(self._free)} of {self.num_pages} free")
        if not needed:
            return
        for b, n in enumerate(want):
            for i in range(self._held[b], n):
                self._host[b, i] = heapq.heappop(self._free)
            self._held[b] = n
        self.peak_pages_in_use = max(self.peak_pages_in_use, self.pages_in_use)
        self.table.copy_(self._host)

    def trim(self, first_live: Sequence[int]) -> None:
        """The pages of sequence b that lie wholly below position ``first_live[b]`` go back to the free list and their
        table entries become ``-1``: what a sliding window leaves behind.  A page that holds ``first_live[b]`` stays.
        Host-side only, no synchronisation; the device table is updated in place when anything changed."""
        first_live = [int(n) for n in (first_live.tolist() if isinstance(first_live, torch.Tensor) else first_live)]
        if len(first_live) != self.batch_size:
            raise ValueError(f"PageTable.trim: {len(first_live)} positions for a batch of {self.batch_size}")
        changed = False
        for b, n in enumerate(first_live):
            upto = min(max(n, 0) // self.page_size, self._held[b])
            for i in range(self._first[b], upto):
                heapq.heappush(self._free, int(self._host[b, i]))
                self._host[b, i] = -1
                changed = True
            self._first[b] = max(self._first[b], upto)
        if changed:
            self.table.copy_(self._host)

    def release(self, b: int) -> None:
        """The pages of sequence ``b`` go back to the free list; its table row becomes ``-1``."""
        for p in self.pages_of(b):
            heapq.heappush(self._free, p)
        self._held[b] = self._first[b] = 0
        self._host[b] = -1
        self.table.copy_(self._host)

    def reset(self) -> None:
        for b in range(self.batch_size):
            if self._held[b]:
                self.release(b)
        self.peak_pages_in_use = 0
