"""What the CPU oracle (the reference dataflow: torch.relu, threshold_backward) does with ONE non-finite input entry, written down
literally.  tests/test_gpu_nonfinite.py holds the HIP path to the same behaviour; this module pins the yardstick itself, so a change
of the oracle (or of torch) that drops a NaN fails here first, without a GPU.

MaskEmbdMultiMPN(4, 2, 4, 9, 2, 1): EdgeAggregation (radius 1), TAGConv K = 1 (radius 1), EdgeAggregation (radius 1) on rings of 40
nodes, so an entry of x reaches the rows within 3 of its own and the gradient of x the rows within 6 of those that feed the loss."""
import pytest
import torch

from oracle import ref_cpu
from tests.nonfinite import VALUES, nonfinite_rows, poison, ring_batch

SEG, B = 40, 3
CASES = {"x": (list(range(47, 54)), list(range(44, 57))),              # x[50, 1]: out radius 3 = 1 + K + 1, grad x radius 6
         "edge_attr": (list(range(48, 54)), list(range(45, 57)))}      # edge_attr[50, 0]: the edge 50 -> 51 of graph 1


def _oracle():
    torch.manual_seed(0)
    return ref_cpu.MaskEmbdMultiMPN(4, 2, 4, 9, 2, 1, 0.0)


def test_relu_and_its_backward_keep_nan_and_inf():
    """torch.relu(nan, -0, inf, -inf) = (nan, -0, inf, 0); threshold_backward passes the gradient wherever !(result <= 0)."""
    z = torch.tensor([float("nan"), -0.0, float("inf"), float("-inf"), 2.0, -2.0], requires_grad=True)
    r = torch.relu(z)
    assert torch.isnan(r[0]) and r[1] == 0 and r[2] == float("inf") and r[3] == 0 and r[4] == 2 and r[5] == 0
    r.backward(torch.arange(1.0, 7.0))
    assert z.grad.tolist() == [1.0, 0.0, 3.0, 0.0, 5.0, 0.0]
    rec = []
    ref_cpu.gated_relu(z.detach(), None, rec)
    assert rec[0].tolist() == [True, False, True, False, True, False]      # the recorded gate is the backward's: NaN is ON
    g = ref_cpu.gated_relu(z.detach(), rec[0])
    assert torch.isnan(g[0]) and g[2] == float("inf") and g[4] == 2          # the gated form keeps NaN / Inf where the gate is 1
    assert g[1] == 0 and g[3] == 0 and g[5] == 0                             # ... and an off unit is 0 even at -Inf


@pytest.mark.parametrize("mode", ["eval", "train"])
@pytest.mark.parametrize("value", list(VALUES))
@pytest.mark.parametrize("where", ["x", "edge_attr"])
def test_oracle_spreads_one_nonfinite_entry_over_its_receptive_field(where, value, mode):
    ref = _oracle()
    ref.train(mode == "train")                                   # (p = 0: the two modes compute the same)
    data = poison(ring_batch(SEG, B, 0), where, 50, VALUES[value])
    data.x.requires_grad_(True)
    out = ref(data)
    loss = torch.nn.MSELoss()(out, data.y)
    loss.backward()
    out_rows, gx_rows = CASES[where]
    assert nonfinite_rows(out) == out_rows
    assert nonfinite_rows(data.x.grad) == gx_rows
    assert not torch.isfinite(loss)
    for t in (out, data.x.grad):                                  # graphs 0 and 2 stay finite
        assert torch.isfinite(t[:SEG]).all() and torch.isfinite(t[2 * SEG:]).all()
    for name, p in ref.named_parameters():
        bad = int((~torch.isfinite(p.grad)).sum())
        if name == "mask_embd.0.weight":                          # hidden units that are off on the poisoned rows stay finite
            assert bad == 24 and p.grad.numel() == 36, (name, bad)
        elif name == "mask_embd.0.bias":
            assert bad == 6 and p.grad.numel() == 9, (name, bad)
        elif (where, value) == ("edge_attr", "+inf") and name.startswith("layers.0.edge_aggr.0."):
            # hidden unit 5 of layer 0 has a negative weight on edge_attr[:, 0]: +Inf switches it OFF on the poisoned edge (a -Inf
            # pre-activation), and with this seed it is off on every other edge that a non-finite gradient reaches, so its row of
            # the weight gradient stays finite except the edge_attr[:, 0] column (0 * Inf = NaN), and so does its bias gradient
            fin = torch.isfinite(p.grad)
            assert bad == p.grad.numel() - (9 if name.endswith("weight") else 1), (name, bad)
            assert bool(fin[5].sum() == (9 if name.endswith("weight") else 1)) and (name.endswith("bias") or not bool(fin[5, 8])), (name, fin)
        else:
            assert bad == p.grad.numel(), (name, bad, p.grad.numel())


def test_clean_batch_stays_finite():
    ref = _oracle()
    data = ring_batch(SEG, B, 0)
    out = ref(data)
    torch.nn.MSELoss()(out, data.y).backward()
    assert torch.isfinite(out).all() and all(torch.isfinite(p.grad).all() for p in ref.parameters())
