"""The capture rules of poweflownet_amd/utils/captured.py on fake objects: no device, no HIP library."""
import gc
from types import SimpleNamespace

import pytest
import torch
import torch.nn as nn

from poweflownet_amd.utils.captured import BatchSource, capture_state, copy_batch, no_gc, topology_owners


class _Owner(nn.Module):
    def __init__(self, dynamic=False):
        super().__init__()
        self.dynamic_topology = dynamic


class _Plain(nn.Module):                       # a module without an adjacency of its own
    pass


class _Boom(Exception):
    pass


# ------------------------------------------------------------------------------------------- capture_state
def _state_fixture():
    owners = [_Owner(True), _Owner(False)]
    model = SimpleNamespace(segment_build=True)
    return owners, model


@pytest.mark.parametrize("raises", [False, True])
def test_capture_state_raises_the_flags_and_restores_the_previous_values(raises):
    owners, model = _state_fixture()
    seen = {}
    try:
        with capture_state(owners, model, dynamic=True, segment_build=True):
            seen["dyn"] = [o.dynamic_topology for o in owners]
            seen["seg"] = model.segment_build
            if raises:
                raise _Boom()
    except _Boom:
        assert raises
    assert seen == {"dyn": [True, True], "seg": True}
    assert [o.dynamic_topology for o in owners] == [True, False]       # their own previous values, not False
    assert model.segment_build is True


@pytest.mark.parametrize("raises", [False, True])
def test_capture_state_restores_a_segment_build_that_was_off(raises):
    owners, model = [_Owner(False)], SimpleNamespace(segment_build=False)
    try:
        with capture_state(owners, model, dynamic=True, segment_build=True):
            assert model.segment_build is True and owners[0].dynamic_topology is True
            if raises:
                raise _Boom()
    except _Boom:
        pass
    assert model.segment_build is False and owners[0].dynamic_topology is False


def test_capture_state_without_dynamic_touches_nothing():
    class Watched:
        """Counts every write of `dynamic_topology`."""
        def __init__(self, value):
            object.__setattr__(self, "writes", 0)
            object.__setattr__(self, "dynamic_topology", value)

        def __setattr__(self, name, value):
            object.__setattr__(self, "writes", self.writes + 1)
            object.__setattr__(self, name, value)

    owners, model = [Watched(True), Watched(False)], Watched(False)
    object.__setattr__(model, "segment_build", True)
    with capture_state(owners, model, dynamic=False, segment_build=False):
        assert [o.dynamic_topology for o in owners] == [True, False] and model.segment_build is True
    assert [o.writes for o in owners] == [0, 0] and model.writes == 0
    assert [o.dynamic_topology for o in owners] == [True, False] and model.segment_build is True


# ----------------------------------------------------------------------------------------- topology_owners
def test_topology_owners_model_first_then_loss_submodules_in_modules_order():
    model = _Owner()
    a, b = _Owner(), _Owner()
    loss = nn.Sequential(_Plain(), a, nn.Sequential(b))
    assert [id(o) for o in topology_owners(model, loss)] == [id(model), id(a), id(b)]
    top = _Owner()                                                     # the loss itself owns one: modules() starts with it
    top.inner = a
    assert [id(o) for o in topology_owners(model, top)] == [id(model), id(top), id(a)]


def test_topology_owners_lists_a_module_reachable_twice_once():
    model, shared = _Owner(), _Owner()
    loss = nn.Sequential(shared, nn.Sequential(shared))
    report = nn.Sequential(shared)
    owners = topology_owners(model, loss, report, shared)
    assert [id(o) for o in owners] == [id(model), id(shared)]


def test_topology_owners_leaves_out_a_model_without_the_attribute():
    model, a = _Plain(), _Owner()
    assert [id(o) for o in topology_owners(model, a)] == [id(a)]
    assert topology_owners(model, None, lambda out, y: out) == []      # a loss that is no nn.Module owns nothing


# ---------------------------------------------------------------------------------------- BatchSource.pull
class _Recorder:
    def __init__(self):
        self.calls = []

    def gather_into(self, data, buffer):
        self.calls.append(("gather_into", data, buffer))

    def gather_topologies_into(self, data, buffer, graph):
        self.calls.append(("gather_topologies_into", data, buffer, graph))

    def gather_slots_into(self, data, buffer):
        self.calls.append(("gather_slots_into", data, buffer))


def _fake_model(ds):
    def adopt(edge_index, graph):
        ds.calls.append(("adopt", edge_index, graph))
    return SimpleNamespace(_graphs=SimpleNamespace(adopt=adopt))


def test_batch_source_pull_indexed_and_slots_make_their_one_call():
    data = SimpleNamespace(edge_index=object())
    for kind, call in (("indexed", "gather_into"), ("slots", "gather_slots_into")):
        ds, buffer = _Recorder(), object()
        BatchSource(kind, ds, buffer).pull(data, _fake_model(ds))
        assert ds.calls == [(call, data, buffer)]


def test_batch_source_pull_topo_gathers_then_adopts():
    ds, buffer, graph = _Recorder(), object(), object()
    data = SimpleNamespace(edge_index=object())
    source = BatchSource("topo", ds, buffer, graph)
    source.pull(data, _fake_model(ds))
    assert ds.calls == [("gather_topologies_into", data, buffer, graph), ("adopt", data.edge_index, graph)]


def test_batch_source_constructors_own_their_buffers():
    ds, idx = _Recorder(), torch.tensor([3, 1, 2])
    source = BatchSource.indexed(ds, idx)
    assert (source.kind, source.dataset, source.topo_graph) == ("indexed", ds, None)
    assert torch.equal(source.buffer, idx) and source.buffer.data_ptr() != idx.data_ptr()
    source = BatchSource.slots(ds, 5, "cpu")
    assert source.kind == "slots" and source.topo_graph is None
    assert source.buffer.shape == (5, 2) and source.buffer.dtype == torch.int32 and not source.buffer.any()


# ---------------------------------------------------------------------------------------------- copy_batch
@pytest.mark.parametrize("with_edge_index", [False, True])
def test_copy_batch_copies_the_edge_list_only_when_asked(with_edge_index):
    def batch(fill):
        return SimpleNamespace(x=torch.full((3, 4), fill), y=torch.full((3, 4), fill + 1), pred_mask=torch.full((3, 4), fill + 2),
                               edge_attr=torch.full((2, 2), fill + 3), edge_index=torch.full((2, 2), int(fill) + 4),
                               bus_type=torch.full((3,), fill + 5))
    static, data = batch(0.0), batch(10.0)
    held = {k: getattr(static, k) for k in vars(static)}
    copy_batch(static, data, with_edge_index)
    assert all(getattr(static, k) is t for k, t in held.items())       # copied INTO the captured tensors, none replaced
    for k in ("x", "y", "pred_mask", "edge_attr"):
        assert torch.equal(getattr(static, k), getattr(data, k))
    assert torch.equal(static.edge_index, data.edge_index) == with_edge_index
    assert torch.equal(static.bus_type, torch.full((3,), 5.0))         # no other field


# --------------------------------------------------------------------------------------------------- no_gc
@pytest.mark.parametrize("raises", [False, True])
@pytest.mark.parametrize("was_on", [True, False])
def test_no_gc_reenables_the_collector_only_if_it_was_on(was_on, raises):
    before = gc.isenabled()
    try:
        gc.enable() if was_on else gc.disable()
        try:
            with no_gc():
                assert not gc.isenabled()
                if raises:
                    raise _Boom()
        except _Boom:
            assert raises
        assert gc.isenabled() == was_on
    finally:
        gc.enable() if before else gc.disable()
