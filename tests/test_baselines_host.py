"""CPU-side checks of the GCN / MLP baselines: the GCNConv semantics pinned by closed forms (PyG is not installed, so the float64
restatement in tests/baselines_ref.py is itself held to hand-computed values), the state_dict contracts, the C ABI additions, and
the Laplacian of the Tikhonov baseline."""
import math
import os
import re

import numpy as np
import pytest
import torch

from poweflownet_amd import _lib as L
from poweflownet_amd.networks.GCN import GCN, GCNConv
from poweflownet_amd.networks.MLP import MLP
from poweflownet_amd.synth import make_batch, make_topology
from poweflownet_amd.utils.baselines import graph_laplacian, tikhonov_regularizer
from tests.baselines_ref import GCN64, MLP64, gcn_conv64, gcn_degrees, laplacian64, tikhonov64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GCN_SYMBOLS = ("pfn_gcn_conv_workspace_bytes", "pfn_gcn_conv_forward", "pfn_gcn_conv_backward")


def test_gcn_conv_closed_form_on_a_directed_path():
    """Path 0 -> 1 -> 2 stored one direction, W = I, no bias: d = (1, 2, 2), so out_0 = x_0, out_1 = x_0 / sqrt(2) + x_1 / 2,
    out_2 = x_1 / 2 + x_2 / 2."""
    x = torch.tensor([[1.0, -2.0, 0.5], [3.0, 0.25, -1.0], [-0.75, 4.0, 2.0]], dtype=torch.float64)
    ei = torch.tensor([[0, 1], [1, 2]])
    out = gcn_conv64(x, ei, torch.eye(3, dtype=torch.float64))
    want = torch.stack([x[0], x[0] / math.sqrt(2.0) + x[1] / 2, x[1] / 2 + x[2] / 2])
    assert torch.allclose(out, want, rtol=0, atol=1e-15)


def test_gcn_conv_self_loops_parallel_lines_and_isolated_nodes():
    """A stored self loop is replaced by the one unit loop, a doubled line counts twice, an isolated node keeps H_i + b."""
    # 0 -> 1 twice, 1 -> 1 stored, 2 -> 0, node 3 isolated, node 4 a source only
    ei = torch.tensor([[0, 0, 1, 2, 4], [1, 1, 1, 0, 2]])
    assert gcn_degrees(ei, 5).tolist() == [2, 3, 2, 1, 1]
    g = torch.Generator().manual_seed(5)
    x = torch.randn(5, 3, generator=g, dtype=torch.float64)
    w = torch.randn(2, 3, generator=g, dtype=torch.float64)
    b = torch.randn(2, generator=g, dtype=torch.float64)
    h = x @ w.t()
    out = gcn_conv64(x, ei, w, b)
    d = torch.tensor([2.0, 3.0, 2.0, 1.0, 1.0], dtype=torch.float64)
    dis = d.rsqrt()
    want = torch.stack([
        dis[0] * (dis[2] * h[2] + dis[0] * h[0]),
        dis[1] * (2 * dis[0] * h[0] + dis[1] * h[1]),
        dis[2] * (dis[4] * h[4] + dis[2] * h[2]),
        h[3],
        h[4],
    ]) + b
    assert torch.allclose(out, want, rtol=0, atol=1e-14)


def test_state_dict_keys_and_strict_loading():
    m = GCN(4, 4, 129)
    want = sorted([f"conv{i}.lin.weight" for i in (1, 2, 3)] + [f"conv{i}.bias" for i in (1, 2, 3)])
    assert sorted(m.state_dict().keys()) == want
    assert tuple(m.conv1.lin.weight.shape) == (129, 4) and tuple(m.conv3.lin.weight.shape) == (4, 129)
    assert float(m.conv2.bias.detach().abs().max()) == 0.0                               # zeros; glorot bound for the weight
    assert float(m.conv2.lin.weight.detach().abs().max()) <= math.sqrt(6.0 / 258.0)
    ref = GCN64(4, 4, 129)
    assert sorted(ref.state_dict().keys()) == want
    m.load_state_dict({k: v.float() for k, v in ref.state_dict().items()}, strict=True)
    assert GCN(8, 4, 16, with_mask=True).with_mask and not m.with_mask
    mlp = MLP(56, 56, 128, 3, 0.2)
    want = sorted([f"layers.{i}.weight" for i in range(4)] + [f"layers.{i}.bias" for i in range(4)])
    assert sorted(mlp.state_dict().keys()) == want
    ref = MLP64(56, 56, 128, 3)
    assert sorted(ref.state_dict().keys()) == want
    mlp.load_state_dict({k: v.float() for k, v in ref.state_dict().items()}, strict=True)
    assert tuple(GCNConv(5, 3, bias=False).state_dict().keys()) == ("lin.weight",)


def test_baselines_have_no_cpu_path():
    d = make_batch("14", 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        GCN(4, 4, 8)(d)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        GCN(8, 4, 8, with_mask=True)(d)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        MLP(56, 56, 16, 3, 0.2)(d)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        GCNConv(4, 4)(d.x, d.edge_index)


def test_gcn_symbols_are_declared_bound_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pfn_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(pfn_[a-z0-9_]+)\s*\(", text))
    lib = L.load()
    for name in GCN_SYMBOLS:
        assert name in L.SYMBOLS, name
        assert name in declared, name
        assert hasattr(lib, name), name
    assert lib.pfn_abi_version() == 8                                            # additive
    ws = lib.pfn_gcn_conv_workspace_bytes(1652, 2604, 129, 129)
    assert ws >= 1652 * 132 + 3 * 1652 * 132 * 4                                  # gate bytes + three row buffers
    assert lib.pfn_gcn_conv_forward(None, 5, 4, 4, 4, None, 4, None, None, 0, None, 4, None, 0, None) == -1
    assert b"null" in lib.pfn_last_error()


def test_graph_laplacian_matches_a_numpy_construction():
    ei = make_topology(14, 20, 0)
    lap = graph_laplacian(ei, 14)
    a = np.zeros((14, 14))
    for s, d in ei.t().tolist():
        a[s, d] += 1
        a[d, s] += 1
    want = np.diag(a.sum(1)) - a
    assert lap.dtype == torch.float64 and np.array_equal(lap.numpy(), want)
    assert np.array_equal(lap.numpy(), lap.numpy().T) and np.array_equal(laplacian64(ei, 14).numpy(), want)
    # a stored self edge cancels in D - A
    assert torch.equal(graph_laplacian(torch.tensor([[0, 1], [0, 2]]), 3), laplacian64(torch.tensor([[1], [2]]), 3))
    y = torch.randn(14, 4, generator=torch.Generator().manual_seed(0), dtype=torch.float64)
    z, z64 = tikhonov_regularizer(1.25, lap, y), tikhonov64(1.25, lap, y)
    assert float((z - z64).abs().max()) <= 1e-10 * float(z64.abs().max())
