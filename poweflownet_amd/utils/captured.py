"""The capture rules `GraphedTrainStep` (utils/training.py), `GraphedEvalStep` (utils/evaluation.py) and `dp.GraphedStep` share:
what is raised around a hipGraph capture and put back after it, how the warm-up runs, what a captured launch keeps alive and how
a batch gets into the captured inputs.  Each rule is here once, with its reason.  Torch only: nothing here loads the HIP library
(`GraphCSR` is imported where it is needed), so the rules are tested without a device (tests/test_captured_host.py)."""
import contextlib
import gc

import torch
import torch.nn as nn


def topology_owners(model, *modules):
    """Everything that keeps an adjacency per `edge_index`: the model, then the sub-modules of `modules` that walk the grid
    themselves (PowerImbalance, also inside MixedMSEPoweImbalance), in `modules()` order, each once; a loss that is no nn.Module
    owns none."""
    owners = [model] if hasattr(model, "dynamic_topology") else []
    for m in modules:
        for o in (m.modules() if isinstance(m, nn.Module) else ()):
            if hasattr(o, "dynamic_topology") and not any(o is seen for seen in owners):
                owners.append(o)
    return owners


@contextlib.contextmanager
def capture_state(owners, model, dynamic: bool, segment_build: bool):
    """The state a captured body runs in, for the warm-up and the capture ONLY (and for every replay of dp.GraphedStep's "eager"
    form, which calls the captured closure itself); whatever was there before comes back, also when the capture raises.

    `dynamic`: `dynamic_topology` on the model AND on every loss module that keeps an adjacency of its own (PowerImbalance: with
    its cache the replayed loss kept walking the capture-time topology) -- the captured launches rebuild the adjacency
    from the captured edge_index buffer on the device, checks included; forwards outside the graph (the other loop, the short last
    batch) keep the validated, cached build.  `segment_build`: `model.segment_build`, for a body whose gather built the adjacency
    itself (`BatchSource.topo`) -- should the model ever decline that adjacency, its own in-graph build of the collated list is the
    segmented one too."""
    prev = [(o, o.dynamic_topology) for o in owners] if dynamic else []
    prev_seg = getattr(model, "segment_build", False)
    try:
        for o, _ in prev:
            o.dynamic_topology = True
        if segment_build:
            model.segment_build = True
        yield
    finally:
        for o, was in prev:
            o.dynamic_topology = was
        if segment_build:
            model.segment_build = prev_seg


def run_on(side, body, passes: int = 1):
    """`body()` on the stream `side`, ordered after what the current stream holds and before what it gets next."""
    cur = torch.cuda.current_stream()
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        for _ in range(passes):
            out = body()
    cur.wait_stream(side)
    return out


def warm_up(side, body, passes: int = 2):
    """The passes torch asks for before a capture, off the capture stream: they fill the allocator and the adjacency caches."""
    run_on(side, body, passes)


@contextlib.contextmanager
def no_gc():
    """No cyclic collection inside a capture window.  The backward pass of a captured step runs on autograd's thread and allocates
    Python objects there, so an automatic collection can begin in the middle of the capture, on a thread that is not the capturing
    one; what its finalizers do (freeing device tensors, destroying events or graphs) are runtime calls a capture in progress does
    not permit, and an error raised inside a destructor ends the process (seen once: an abort from a collection that had started at
    the first allocation of MaskEmbdMultiMPN's captured backward).  The collector is held back until the attempt is over; nothing
    is lost, the next pass collects the same objects.  A collector that was off stays off."""
    was_on = gc.isenabled()
    gc.disable()
    try:
        yield
    finally:
        if was_on:
            gc.enable()


def held_adjacencies(owners, *extra):
    """The `GraphCSR`s a captured launch reads: the adjacencies the owners built during the warm-up, whose only other owner is a
    one-entry cache -- a batch with another edge_index (training and evaluation take turns, a short last batch) would evict and
    free them -- and `extra` (the one a captured gather builds into).  Kept for as long as the graph is."""
    return [o._graphs._graph for o in owners if getattr(o, "_graphs", None) is not None] + [g for g in extra if g is not None]


def copy_batch(static, data, with_edge_index: bool) -> None:
    """A collated batch into the captured inputs; the edge list too when the adjacency is rebuilt inside the graph."""
    for k in ("x", "y", "pred_mask", "edge_attr") + (("edge_index",) if with_edge_index else ()):
        getattr(static, k).copy_(getattr(data, k))


def topologies_gatherable(model, owners, dataset) -> bool:
    """Can a captured body pull a batch AND its adjacency from `dataset` (`BatchSource.topo`)?  The model takes a segment hint and
    an adopted adjacency, it is the only owner of one (a loss module that walks the grid itself keeps a build of its own and passes
    no hint: the dynamic path), and the dataset holds a dense edge block per case (`can_gather_topologies()`)."""
    return bool(hasattr(model, "segment_build") and hasattr(getattr(model, "_graphs", None), "adopt") and owners == [model]
                and hasattr(dataset, "can_gather_topologies") and dataset.can_gather_topologies())


class BatchSource:
    """Where a captured body pulls its batch from, INSIDE the graph: a device-resident dataset and the captured buffer that names
    the samples -- per batch the host copies into `buffer` and launches the graph, no collate, no per-field copies.
      indexed  `buffer` = the sample indices (device int64); the five row gathers (`gather_into`)
      topo     the same for a split with one line set per sample: the ONE call that gathers the rows, collates the samples' edge
               lists and builds their adjacency into `topo_graph`, one workgroup per graph (`gather_topologies_into`)
      slots    `buffer` = the slot table [n_slots, 2] int32 of a mixed batch's bucket (`gather_slots_into`)"""
    __slots__ = ("kind", "dataset", "buffer", "topo_graph")

    def __init__(self, kind, dataset, buffer, topo_graph=None):
        self.kind, self.dataset, self.buffer, self.topo_graph = kind, dataset, buffer, topo_graph

    @classmethod
    def indexed(cls, dataset, idx):
        return cls("indexed", dataset, idx.clone())

    @classmethod
    def topo(cls, dataset, idx, device):
        from ..networks.MPN import GraphCSR
        B = int(idx.numel())
        n_of, e_of, _ = dataset.case_sizes()
        return cls("topo", dataset, idx.clone(), GraphCSR.for_block(B * n_of[0], B * e_of[0], n_of[0], e_of[0], device))

    @classmethod
    def slots(cls, dataset, n_slots, device):
        return cls("slots", dataset, torch.zeros(n_slots, 2, dtype=torch.int32, device=device))

    def pull(self, data, model) -> None:
        if self.kind == "slots":
            self.dataset.gather_slots_into(data, self.buffer)
        elif self.kind == "topo":
            # the gather wrote data.edge_index AND its adjacency in one call: the model's next cache lookup takes it as built
            self.dataset.gather_topologies_into(data, self.buffer, self.topo_graph)
            model._graphs.adopt(data.edge_index, self.topo_graph)
        else:
            self.dataset.gather_into(data, self.buffer)
