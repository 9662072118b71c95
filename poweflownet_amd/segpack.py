"""Segment packing of mixed-size graph batches: the host-side planner (pure Python / numpy, no GPU, no kernels).

Every fast route of the library is chosen by one number, `seg_nodes`: "no edge of the batch crosses a multiple of seg_nodes"
(pfn_graph_segments).  The kernels behind it form their row blocks from whole segments and never ask that a segment BE one graph,
so a segment may hold several whole graphs followed by isolated padding rows: a padding row receives no message, sends none, and
-- its loss gradient being zero -- contributes exact zeros to every weight gradient.  `plan` lays a ragged batch out that way:

  S      = max(sizes)                                   rows per segment
  bins   = first-fit-decreasing of the graphs into bins of S rows, stable order by (-size, batch position)
  start  = first padded row of every graph: the graphs of a bin are contiguous in the order they were placed, padding rows last

It returns None -- "do not pack, behave as before" -- for a uniform batch, for fewer than two graphs, and when the padded layout
would hold more than (1 + max_padding) * N rows: padded rows cost GEMM and walk work in proportion, so the cap is a condition, not
a measurement.  Which kernels a given (S, n_pad) then gets is decided by the library's own fit predicates, as for a uniform batch.
"""
from __future__ import annotations

from functools import lru_cache
from typing import Optional, Sequence

import numpy as np


class SegPlan:
    """Layout of one ragged batch in equal segments.  `sizes`, `ptr` (G + 1, exclusive offsets of the caller's rows), `start` (G)
    and `fill` (n_seg: rows of each segment that belong to a graph) are int32 numpy arrays."""

    def __init__(self, sizes: np.ndarray, start: np.ndarray, fill: np.ndarray, S: int):
        self.sizes, self.start, self.fill, self.S = sizes, start, fill, int(S)
        self.n_graphs, self.n_seg = int(sizes.shape[0]), int(fill.shape[0])
        self.n, self.n_pad = int(sizes.sum()), self.n_seg * self.S
        self.ptr = np.zeros(self.n_graphs + 1, dtype=np.int32)
        np.cumsum(sizes, out=self.ptr[1:])

    @property
    def padding(self) -> float:
        """Share of padding rows relative to the real ones: n_pad / N - 1."""
        return self.n_pad / self.n - 1.0

    def host_row_of(self) -> np.ndarray:
        """The padded row of every real row, from the plan alone (what the device pack writes as `row_of`)."""
        g = np.repeat(np.arange(self.n_graphs), self.sizes)
        return (self.start[g] + np.arange(self.n) - self.ptr[:-1][g]).astype(np.int32)

    def meta(self) -> np.ndarray:
        """ptr | start | fill as ONE int32 array: the only per-batch host -> device traffic of a pack, O(G)."""
        return np.concatenate([self.ptr, self.start, self.fill]).astype(np.int32)

    def __repr__(self):
        return (f"SegPlan(graphs={self.n_graphs}, N={self.n}, S={self.S}, n_seg={self.n_seg}, n_pad={self.n_pad}, "
                f"padding={100.0 * self.padding:.1f}%)")


def _first_fit_decreasing(values, counts, S: int):
    """First-fit-decreasing of a size list given as its distinct sizes in DECREASING order and their counts: (start of every graph
    in that sorted order, fill per bin).  Graphs of one size are placed as a group: successive equal items of a first-fit go to the
    bins in index order, each open bin taking as many as still fit, the rest to new bins -- one numpy pass over the bins per
    distinct size picks the bins with room, the new bins are laid out in one go, and no step is taken per graph."""
    total = int(sum(counts))
    start = np.empty(total, dtype=np.int64)
    fill = np.zeros(total, dtype=np.int64)           # (a graph opens one bin at most)
    nb = pos = 0
    for s, count in zip(values, counts):
        if s == 0:                                   # empty graphs take no rows: they sit at row 0 of the layout
            start[pos:pos + count] = 0
            pos += count
            continue
        left = count
        for b in np.flatnonzero(fill[:nb] <= S - s).tolist():
            f = int(fill[b])
            k = min((S - f) // s, left)
            start[pos:pos + k] = range(b * S + f, b * S + f + k * s, s)
            fill[b] = f + k * s
            pos += k
            left -= k
            if left == 0:
                break
        if left > 0:                                 # new bins, S // s graphs each, the last one what is left
            per = S // s
            new = -(-left // per)
            j = np.arange(left)
            start[pos:pos + left] = (nb + j // per) * S + (j % per) * s
            fill[nb:nb + new] = per * s
            fill[nb + new - 1] = (left - per * (new - 1)) * s
            nb += new
            pos += left
    return start, fill[:nb].copy()


@lru_cache(maxsize=256)
def _layout_of_sorted(values: tuple, counts: tuple):
    """The layout depends on the ORDER of a batch only through the stable sort: it is computed for the sorted list -- keyed by
    how many graphs of each size there are, so a loader that draws from a few grid cases meets the same few keys again and again
    -- and handed to the batch positions through the sort permutation (`plan`)."""
    start, fill = _first_fit_decreasing(values, counts, values[0])
    return start.astype(np.int32), fill.astype(np.int32)


def plan(sizes: Sequence[int], max_padding: float = 0.25) -> Optional[SegPlan]:
    """The segment layout of a batch of graphs with `sizes` nodes each, or None: do not pack (see the module docstring).
    Deterministic."""
    arr = np.asarray(sizes, dtype=np.int64)
    if arr.ndim != 1 or arr.shape[0] < 2:
        return None
    lo, S = int(arr.min()), int(arr.max())
    if lo < 0 or lo == S:
        return None
    order = np.argsort(-arr, kind="stable")
    values, counts = np.unique(-arr, return_counts=True)            # ascending in -size = decreasing in size
    start_sorted, fill = _layout_of_sorted(tuple((-values).tolist()), tuple(counts.tolist()))
    n, n_pad = int(arr.sum()), int(fill.shape[0]) * S
    if n_pad > (1.0 + max_padding) * n or n_pad >= 2 ** 31:
        return None
    start = np.empty(arr.shape[0], dtype=np.int32)
    start[order] = start_sorted
    return SegPlan(arr.astype(np.int32), start, fill, S)
