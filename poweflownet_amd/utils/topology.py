"""Per-sample topology perturbation on the device: `perturb_topology` is ONE `pfn_topology_perturb` launch (csrc/topology.hip), one
workgroup per sample.  It stands where the reference calls `perturb_topology` (utils/data_utils.py:12-59, dataset_generator.py
-r / -a): remove random lines, start over while a bus is left unsupplied, add lines between random bus pairs as copies of random
existing lines.  The drawing rule is fixed in include/pfn_hip.h -- Philox words counted by the global sample number -- so a sample's
draw depends on (seed, sample) alone.  `unsupplied_buses` is the reference's connectivity check for given line lists.  No CPU path."""
from dataclasses import dataclass

import torch

from .. import _lib as L

STATUS = {-1: "no connected draw in max_attempts", -4: "a line names a bus outside the grid"}
MAX_ATTEMPTS = 1024


@dataclass
class PerturbedTopology:
    """`edge_index` [S, 2, e_out] int64 (kept base lines in base order, then the added lines; -1 rows where the sample failed),
    `source` [S, e_out] int32 (the base line an output line is, or copies its parameters from), `status` [S] int32 (>= 1: attempts
    used; < 0: `STATUS`) -- all on the device, nothing read back."""
    edge_index: torch.Tensor
    source: torch.Tensor
    status: torch.Tensor


def _grid(edge_index, n_bus, root, who, per_sample_ok):
    if isinstance(n_bus, bool) or not isinstance(n_bus, int) or n_bus < 1:
        raise ValueError(f"{who}: n_bus must be a positive int; got {n_bus!r}")
    if isinstance(root, bool) or not isinstance(root, int) or not 0 <= root < n_bus:
        raise ValueError(f"{who}: root must be a bus in [0, {n_bus}); got {root!r}")
    dims = (2, 3) if per_sample_ok else (2,)
    if not isinstance(edge_index, torch.Tensor) or edge_index.dtype != torch.int64 or edge_index.dim() not in dims or edge_index.shape[-2] != 2:
        want = "(2, e) or (S, 2, e)" if per_sample_ok else "(2, e)"
        got = f"{edge_index.dtype} {tuple(edge_index.shape)}" if isinstance(edge_index, torch.Tensor) else type(edge_index).__name__
        raise RuntimeError(f"{who}: edge_index must be an int64 tensor {want}; got {got}")


def perturb_topology(edge_index, n_bus, *, num_samples, remove=0, add=0, seed=0, first_sample=0, root=0, max_attempts=20) -> PerturbedTopology:
    """Draw `num_samples` perturbed line lists of the base grid `edge_index` [2, e] (int64 local bus ids, on the device) with
    `n_bus` buses: `remove` random lines leave, redrawn up to `max_attempts` times until every bus is reachable from `root`; then
    `add` lines between random distinct bus pairs arrive, each a copy of a random base line (`source` says which).  Every sample has
    e_out = e - remove + add lines.  Sample s of the call is global sample `first_sample + s`; its draw depends on (`seed`, that
    number) only, so a set drawn in batches with a running `first_sample` equals the set drawn at once.

    ValueError for a count or option that cannot be drawn, RuntimeError for a tensor of the wrong kind or place.  Nothing is read
    back: look at `status` (or not) where it suits the caller."""
    who = "perturb_topology"
    for name, v, lo in (("num_samples", num_samples, 0), ("remove", remove, 0), ("add", add, 0), ("first_sample", first_sample, 0)):
        if isinstance(v, bool) or not isinstance(v, int) or v < lo:
            raise ValueError(f"{who}: {name} must be an int >= {lo}; got {v!r}")
    if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 1 << 64:
        raise ValueError(f"{who}: seed must be an int in [0, 2^64); got {seed!r}")
    if isinstance(max_attempts, bool) or not isinstance(max_attempts, int) or not 1 <= max_attempts <= MAX_ATTEMPTS:
        raise ValueError(f"{who}: max_attempts must be an int in [1, {MAX_ATTEMPTS}]; got {max_attempts!r}")
    if first_sample + num_samples > 1 << 32:
        raise ValueError(f"{who}: sample numbers {first_sample} + [0, {num_samples}) do not fit the 32-bit counter word")
    _grid(edge_index, n_bus, root, who, per_sample_ok=False)
    e = int(edge_index.shape[1])
    if remove > e:
        raise ValueError(f"{who}: cannot remove {remove} of {e} lines")
    if e - remove < n_bus - 1:
        raise ValueError(f"{who}: {e} lines less {remove} cannot connect {n_bus} buses")
    if add > 0 and n_bus < 2:
        raise ValueError(f"{who}: cannot add {add} lines to a grid of {n_bus} bus")
    dev = L.require_device(edge_index, what=f"{who} input")
    edge_index = edge_index.contiguous()
    e_out = e - remove + add
    out = torch.empty(num_samples, 2, e_out, dtype=torch.int64, device=dev)
    source = torch.empty(num_samples, e_out, dtype=torch.int32, device=dev)
    status = torch.empty(num_samples, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        L.check(L.load().pfn_topology_perturb(edge_index.data_ptr(), e, n_bus, num_samples, first_sample, remove, add, seed, root,
                                              max_attempts, out.data_ptr(), source.data_ptr(), status.data_ptr(), L.stream_ptr()),
                "pfn_topology_perturb")
    return PerturbedTopology(edge_index=out, source=source, status=status)


def unsupplied_buses(edge_index, n_bus, root=0) -> torch.Tensor:
    """int32 [S]: the number of buses not reachable from `root` over each sample's lines -- `edge_index` int64 [S, 2, e] on the
    device, or [2, e] (S = 1) -- or -4 where a line of that sample names a bus outside [0, n_bus).  0 is the reference's
    "no unsupplied bus".  Nothing is read back."""
    who = "unsupplied_buses"
    _grid(edge_index, n_bus, root, who, per_sample_ok=True)
    dev = L.require_device(edge_index, what=f"{who} input")
    edge_index = edge_index.contiguous()
    per_sample = edge_index.dim() == 3
    S, e = (int(edge_index.shape[0]) if per_sample else 1), int(edge_index.shape[-1])
    count = torch.empty(S, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        L.check(L.load().pfn_topology_unsupplied(edge_index.data_ptr(), int(per_sample), e, S, n_bus, root, count.data_ptr(), L.stream_ptr()),
                "pfn_topology_unsupplied")
    return count
