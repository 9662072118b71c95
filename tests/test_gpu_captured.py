"""`GraphedTrainStep` and `GraphedEvalStep` leave the model and the optimizer as they found them (utils/captured.py: the flags are
raised for the warm-up and the capture only), for each of the three uniform batch sources: a device-resident set gathered inside
the graph, a list-backed loader (a new edge_index per batch: the dynamic form) and a set with one line set per sample whose
adjacency is built inside the graph.  Case 14, 22 samples, batches of 8, 8 and 6."""
import math

import numpy as np
import pytest
import torch

from poweflownet_amd.data import DataLoader
from poweflownet_amd.datasets import PowerFlowData
from poweflownet_amd.loss import MSELoss
from poweflownet_amd.networks.MPN import MaskEmbdMultiMPN
from poweflownet_amd.optim import FlatAdamW
from poweflownet_amd.synth import make_topology
from poweflownet_amd.utils.custom_loss_functions import Masked_L2_loss
from poweflownet_amd.utils.evaluation import GraphedEvalStep, evaluate_epoch
from poweflownet_amd.utils.training import GraphedTrainStep, train_epoch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _case14(root, per_sample_topology):
    """44 raw samples (the training half of the split: 22), with one line set for all of them or one per sample."""
    rng = np.random.default_rng(5)
    S, n, e = 44, 14, 20
    node = np.zeros((S, n, 6))
    node[:, :, 0] = np.arange(n)
    node[:, :, 1] = np.where(np.arange(n) == 0, 0, np.where(np.arange(n) % 3 == 0, 1, 2))
    node[:, :, 2:] = rng.normal(size=(S, n, 4))
    edge = np.zeros((S, e, 4))
    for s in range(S):
        edge[s, :, :2] = make_topology(n, e, seed=100 + s if per_sample_topology else 100).numpy().T
    edge[:, :, 2:] = np.abs(rng.normal(size=(S, e, 2))) * 0.1 + 0.01
    (root / "raw").mkdir()
    np.save(root / "raw" / "case14_edge_features.npy", edge)
    np.save(root / "raw" / "case14_node_features.npy", node)
    ds = PowerFlowData(root=str(root), case="14", split=[.5, .25, .25], task="train", device=DEV)
    assert len(ds) == 22
    return ds


@pytest.mark.parametrize("source", ["indexed", "list", "topo"])
def test_a_graphed_train_and_eval_epoch_leave_the_model_as_they_found_it(tmp_path, source):
    ds = _case14(tmp_path, per_sample_topology=source == "topo")
    assert ds.can_gather() == (source != "topo") and ds.can_gather_topologies() == (source == "topo")
    over = [ds[i] for i in range(len(ds))] if source == "list" else ds    # Batch.from_data_list: a new edge_index per batch
    torch.manual_seed(7)
    model = MaskEmbdMultiMPN(4, 2, 4, 32, 3, 2, 0.0).to(DEV)
    opt = FlatAdamW(model, lr=1e-3)
    loss_fn, eval_loss = MSELoss(), Masked_L2_loss(regularize=False)
    gt = GraphedTrainStep(model, loss_fn, opt, per_sample_topology=source == "topo")
    ge = GraphedEvalStep(model, eval_loss)
    model.train()
    was_training = model.training
    assert model.dynamic_topology is False and model.segment_build is False and model._mse_attach is None

    train_loss = train_epoch(model, DataLoader(over, batch_size=8, shuffle=False), loss_fn, opt, DEV, graph=gt)
    eval_value = evaluate_epoch(model, DataLoader(over, batch_size=8, shuffle=False), eval_loss, DEV, graph=ge)

    assert math.isfinite(train_loss) and math.isfinite(eval_value)
    # the epochs went the way this case is about
    assert not gt.any_disabled() and not ge.disabled and ge.eager_batches == 0
    assert ge.captures == (3 if source == "list" else 2)           # per batch size; the list's first one once more, dynamic
    if source == "indexed":
        assert sorted(gt._children) == [6, 8] and not gt._topo_children and not gt.dynamic
        assert all(ch.graph is not None and not ch.dynamic for ch in gt._children.values())
        assert all(ch.graph is not None and not ch.dynamic for ch in ge._children.values())
    elif source == "list":
        assert gt.dynamic and gt.graph is not None and not gt._children and not gt._topo_children
        assert all(ch.graph is not None and ch.dynamic for ch in ge._children.values())
    else:
        assert sorted(gt._topo_children) == [6, 8] and not gt._children
        assert all(ch.graph is not None and ch.dynamic for ch in gt._topo_children.values())
        assert all(ch.graph is not None and ch.dynamic for ch in ge._children.values())
    # ... and left nothing behind
    assert model.dynamic_topology is False
    assert model.segment_build is False
    assert getattr(opt, "guard", None) is None
    assert model.training is was_training
    assert model._mse_attach is None
