"""Shared helpers of the non-finite propagation tests (tests/test_nonfinite_host.py, tests/test_gpu_nonfinite.py).

The contract under test: a NaN or Inf in an input reaches every output row of its receptive field, and ONLY those, as it does in
the reference (torch.relu / threshold_backward: a unit is off iff its pre-activation compares <= 0, NaN is on).  Ring graphs make
the receptive field a known interval of rows, so the expected row sets are written down, not computed.
"""
import functools

import torch

from poweflownet_amd.data import Batch
from poweflownet_amd.synth import make_graph
from tests.util import record

VALUES = {"nan": float("nan"), "+inf": float("inf"), "-inf": float("-inf")}


@functools.lru_cache(maxsize=4)
def ring_batch(seg, B, seed=0):
    """B graphs, each a ring i -> (i + 1) % seg stored once (every node has degree 2 after undirecting), bus types, masks and
    statistics as in synth.make_graph, collated like the loader.  Cached and SHARED: never written (poison() copies)."""
    i = torch.arange(seg, dtype=torch.long)
    ring = torch.stack([i, (i + 1) % seg])
    return Batch.from_data_list([make_graph(seg, seg, seed=seed * 1_000_003 + b, edge_index=ring) for b in range(B)])


def poison(data, where, row, value, col=None):
    """A copy of `data` with ONE entry replaced: x[row, 1] (where == "x") or edge_attr[row, 0] (where == "edge_attr")."""
    assert where in ("x", "edge_attr"), where
    d = data.clone()
    t = getattr(d, where)
    t[row, (1 if where == "x" else 0) if col is None else col] = value
    return d


def nonfinite_rows(t):
    """The sorted indices of the rows (dim 0) of `t` that hold a NaN or an Inf."""
    t = t.detach().cpu()
    bad = ~torch.isfinite(t.reshape(t.shape[0], -1)).all(dim=1)
    return torch.nonzero(bad).flatten().tolist()


def _finite_err(got, want, both):
    if not bool(both.any()):
        return 0.0, 0.0
    g, w = got[both].double(), want[both].double()
    return (g - w).abs().max().item(), w.abs().max().item()


def assert_same_nonfinite(got, want, what, rtol):
    """The non-finite entry sets of `got` and `want` are EQUAL (NaN against Inf is not distinguished: finite or not), and on the
    rest |got - want| <= rtol * max |finite want|."""
    got, want = got.detach().cpu(), want.detach().cpu()
    assert got.shape == want.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(want.shape)}"
    bg, bw = ~torch.isfinite(got), ~torch.isfinite(want)
    dropped, extra = int((bw & ~bg).sum()), int((bg & ~bw).sum())
    err, scale = _finite_err(got, want, ~bg & ~bw)
    record(f"{what}: {int(bw.sum())} non-finite entries expected, {dropped} dropped, {extra} extra", err, scale, rtol)
    assert dropped == 0 and extra == 0, \
        (f"{what}: {dropped} non-finite entries of the reference are finite here (rows {nonfinite_rows(bw & ~bg)[:8]}), "
         f"{extra} finite ones are not (rows {nonfinite_rows(bg & ~bw)[:8]})")
    assert err <= rtol * scale + 1e-30, f"{what}: finite entries: max err {err:.3e} vs scale {scale:.3e}, bound {rtol:g}"


def assert_covers_nonfinite(got, want, what, rtol):
    """For parameter gradients (sums over all rows: where the reference is non-finite, so is `got`; an entry the reference keeps
    finite may be either only where a 0 * NaN decides -- not claimed).  Entries finite in both are close: rtol * max |finite want|."""
    got, want = got.detach().cpu(), want.detach().cpu()
    assert got.shape == want.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(want.shape)}"
    bg, bw = ~torch.isfinite(got), ~torch.isfinite(want)
    dropped = int((bw & ~bg).sum())
    err, scale = _finite_err(got, want, ~bg & ~bw)
    record(f"{what}: {int(bw.sum())} non-finite entries expected, {dropped} dropped, {int((bg & ~bw).sum())} extra", err, scale, rtol)
    assert dropped == 0, f"{what}: {dropped} of {int(bw.sum())} non-finite entries of the reference are finite here"
    assert err <= rtol * scale + 1e-30, f"{what}: finite entries: max err {err:.3e} vs scale {scale:.3e}, bound {rtol:g}"
