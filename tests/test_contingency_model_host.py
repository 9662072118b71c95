"""The network's N-1 screen without a GPU: the yardstick of the batch builder (tests/contingency_model_ref.py) gives the bits of
`PowerFlowData` itself -- `_Block`, its normalisation and its collate, fed the reduced grids as raw files --, `contingency_screen_model`
refuses what it must on the host before anything touches the device, and the C ABI carries the three symbols and refuses bad sizes
before anything is launched.  (Wrong dtypes and shapes of DEVICE tensors are refused by `_check`, which asks for the device first:
tests/test_gpu_contingency_model.py.)"""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from poweflownet_amd import _lib as L
from poweflownet_amd.datasets import PowerFlowData
from poweflownet_amd.synth import make_physical_inputs
from poweflownet_amd.utils.contingency import ModelContingencyResult, contingency_screen_model
from tests import contingency_model_ref as R


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _raw_files(root, bt, spec, ei, rx):
    """every (scenario, outage) of the grid as a sample of a raw dataset: node [T, n, 6], edge [T, e - 1, 4] (float64 files)"""
    S, n, e = spec.shape[0], spec.shape[1], ei.shape[1]
    node, edge = np.zeros((S * e, n, 6)), np.zeros((S * e, e - 1, 4))
    for t in range(S * e):
        s, k = divmod(t, e)
        idx = R.kept_lines(k, e).numpy()
        node[t, :, 0], node[t, :, 1], node[t, :, 2:] = np.arange(n), bt.numpy(), spec[s].numpy()
        edge[t, :, :2], edge[t, :, 2:] = ei[:, idx].numpy().T, rx[s, idx].numpy()
    os.makedirs(os.path.join(root, "raw"))
    np.save(os.path.join(root, "raw", "case5_edge_features.npy"), edge)
    np.save(os.path.join(root, "raw", "case5_node_features.npy"), node)


@pytest.mark.parametrize("normalise", [True, False])
def test_the_yardstick_gives_the_bits_of_the_dataset_and_its_collate(tmp_path, normalise):
    n, e, S = 5, 6, 2
    ei, bt, rx, spec = make_physical_inputs(n, e, S, seed=1)
    spec = spec.clone()
    spec[0, 1, 0] = -0.37                                                   # (a masked entry that is not zero: multiplied by 0, not skipped)
    _raw_files(str(tmp_path), bt, spec, ei, rx)
    ds = PowerFlowData(root=str(tmp_path), case="5", split=[1.0, 0.0, 0.0], task="train", normalize=normalise)
    assert len(ds) == S * e and not ds._blocks[0].static_topology
    stats = dict(zip(("xymean", "xystd", "edgemean", "edgestd"), ds.get_data_means_stds())) if normalise else {}
    for items in (R.chunk_items(0, S * e, S, e), R.chunk_items(4, 5, S, e), R.chunk_items(9, 7, S, e)):     # whole, straddling, padded tail
        want = ds.collate_indices(items)
        got = R.batch_ref(bt, spec, ei, rx, items, **stats)
        for name in ("x", "edge_attr"):
            assert getattr(want, name).dtype == torch.float32 and torch.equal(_bits(getattr(want, name)), _bits(got[name])), name
        for name in ("bus_type", "edge_index", "batch", "ptr"):
            assert torch.equal(getattr(want, name), got[name]), name
        assert got["pred_mask"].dtype == torch.float32 and torch.equal(want.pred_mask.float(), got["pred_mask"])
    assert R.chunk_items(9, 7, S, e) == [9, 10, 11, 11, 11, 11, 11] and R.kept_lines(2, 6).tolist() == [0, 1, 3, 4, 5]
    # the masked entry went through the multiplication: x there is (-0.37 * 0 - mean) / (std + 1e-7)
    x = R.batch_ref(bt, spec, ei, rx, [0], **stats)["x"]
    want = torch.tensor(-0.37) * 0.0
    if normalise:
        want = (want - stats["xymean"][0, 0]) / (stats["xystd"][0, 0] + 0.0000001)
    assert torch.equal(_bits(x[1, 0]), _bits(want.float()))


class _Stub(nn.Module):
    def forward(self, data):
        return torch.zeros(data.x.shape[0], 4)


def test_what_the_entry_refuses_on_the_host():
    ei, bt, rx, spec = make_physical_inputs(5, 6, 2, seed=1)
    ok = (bt, spec, ei, rx)
    with pytest.raises(ValueError, match="nn.Module"):
        contingency_screen_model(lambda b: None, *ok)
    with pytest.raises(ValueError, match="nn.Module"):
        contingency_screen_model(None, *ok)
    for chunk in (0, -3, 2.5, True, 2 ** 24):
        with pytest.raises(ValueError, match="chunk"):
            contingency_screen_model(_Stub(), *ok, chunk=chunk)
    for name in ("keep_table", "keep_predictions", "graphed"):
        with pytest.raises(ValueError, match=name):
            contingency_screen_model(_Stub(), *ok, **{name: 1})
    with pytest.raises(ValueError, match="one line"):                       # e == 1 leaves no line
        contingency_screen_model(_Stub(), bt, spec, ei[:, :1], rx[:, :1])
    for name, count in (("xymean", 4), ("xystd", 4), ("edgemean", 2), ("edgestd", 2)):
        with pytest.raises(ValueError, match=name):
            contingency_screen_model(_Stub(), *ok, **{name: torch.ones(count + 1)})
    with pytest.raises(RuntimeError, match="no CPU fallback"):              # everything else is asked of DEVICE tensors
        contingency_screen_model(_Stub(), *ok, xymean=torch.zeros(1, 4), xystd=torch.ones(1, 4))


def test_the_result_ranks_like_the_dc_screen_and_says_whose_figure_it_carries():
    nan, inf = float("nan"), float("inf")
    sev = torch.tensor([[0.5, inf, 2.0, nan, 2.0]])
    z = torch.zeros(1, 5, dtype=torch.int32)
    res = ModelContingencyResult(severity=sev, worst_line=z, overloads=z, islands=z[0])
    assert res.ranking(5)[0].tolist() == [[3, 1, 2, 4, 0]] and res.loading is None and res.predictions is None and res.captures == 0
    assert "dc_severity" in ModelContingencyResult.__doc__ and "network" in ModelContingencyResult.__doc__


def test_abi_surface_and_refusals():
    names = ("pfn_contingency_model_lds_max_bus", "pfn_contingency_model_batch", "pfn_contingency_model_loadings")
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pfn_hip.h")).read()
    lib = L.load()
    for name in names:
        assert name in L.SYMBOLS and name + "(" in header and hasattr(lib, name)
    assert lib.pfn_abi_version() == 8
    assert lib.pfn_contingency_model_lds_max_bus() == lib.pfn_branch_flows_lds_max_bus() == 10176
    p = C.c_void_p(256)                                                      # (never followed: every call below is refused first)

    def batch(S=2, n=14, e=20, chunk=8, x=p):
        return lib.pfn_contingency_model_batch(p, p, p, p, S, n, e, p, chunk, None, None, None, None, x, p, p, p, p, p, None)

    def loadings(S=2, n=14, e=20, chunk=8, route=0, out=p):
        return lib.pfn_contingency_model_loadings(out, p, p, p, p, None, 0, p, S, n, e, p, chunk, None, None, route, p, p, p, None, None, None)
    for call in (batch, loadings):
        assert call(e=1) == -1 and b"bad sizes" in lib.pfn_last_error()     # one line: nothing stays
        assert call(chunk=0) == -1 and b"bad sizes" in lib.pfn_last_error()
        assert call(n=1) == -1 and b"bad sizes" in lib.pfn_last_error()
        assert call(S=0) == 0
    assert batch(x=None) == -1 and b"null" in lib.pfn_last_error()
    assert batch(x=C.c_void_p(264)) == -1 and b"aligned" in lib.pfn_last_error()
    assert loadings(out=None) == -1 and b"null" in lib.pfn_last_error()
    assert loadings(route=3) == -1 and b"route" in lib.pfn_last_error()
    assert loadings(n=10177, e=12000, chunk=2, route=1) == -1 and b"bytes of LDS" in lib.pfn_last_error()
