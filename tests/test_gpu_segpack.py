"""Mixed-size batches on the segment fast paths (MI355X): the three segpack kernels bit for bit against their numpy restatement
(tests/test_segpack_host.py), and the model on a packed batch against the CPU oracle, against its own unpacked route, and through
the training loop."""
import os

import numpy as np
import pytest
import torch

from oracle import ref_cpu
from poweflownet_amd import _lib as L
from poweflownet_amd import segpack
from poweflownet_amd.networks.MPN import MaskEmbdMultiMPN, PackedSegments, _SegPackFn
from poweflownet_amd.synth import make_batch
from tests.test_segpack_host import (COMPOSITIONS, _mixed_root, ball_like_sizes, make_ragged_batch, np_gather_rows, np_pack,
                                     np_scatter_rows)
from tests.util import (RTOL, _assert_grads_on_hip_gates, _check_full_size, _exported_masks, _fp64_truth, _run, assert_close)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

SEG_CLASSES = ("ea_seg_fwd", "ea_seg_bwd", "front_seg_fwd+pack", "seg_lin_hops_fwd", "seg_lin_hops_bwd")
PACK_CLASSES = ("segpack_rows", "segpack_edges", "segpack_gather", "segpack_scatter")
MIXED = [118] * 40 + [14] * 88
TINY = [14, 7, 7, 5, 5, 1, 1, 14, 7, 5, 1, 1]          # 68 rows in 5 segments of 14: 2.9 % padding


def _models(h=129, layers=4, K=3, p=0.0, seed=1234, train=False):
    torch.manual_seed(seed)
    ref = ref_cpu.MaskEmbdMultiMPN(4, 2, 4, h, layers, K, p)
    m = MaskEmbdMultiMPN(4, 2, 4, h, layers, K, p)
    m.load_state_dict(ref.state_dict())
    m.segment_packing = True                                  # (off by default)
    return m.to(DEV).train(train), ref.train(train)


# ----------------------------------------------------------------------------------------------------- kernels
KERNEL_CASES = {
    **{k: (v[0], {}) for k, v in COMPOSITIONS.items()},
    "ball-like 512": (ball_like_sizes(), {}),
    "1-node, edgeless and isolated": ([5, 1, 9, 3, 9, 1, 2], {"edgeless": (3,), "isolated": (2, 6)}),
}


@pytest.mark.parametrize("mask_dtype", [torch.int64, torch.float32])
@pytest.mark.parametrize("name", sorted(KERNEL_CASES))
def test_kernels_are_bit_exact_against_the_numpy_restatement(name, mask_dtype):
    sizes, kw = KERNEL_CASES[name]
    b = make_ragged_batch(sizes, seed=2, **kw)
    plan = segpack.plan(sizes, max_padding=1.0)
    mask = b.pred_mask.to(mask_dtype)
    if mask_dtype == torch.float32:
        mask = mask * 0.75                                   # (a float mask is moved as it is, not re-derived)
    want = np_pack(plan, b.x.numpy(), mask.numpy(), b.edge_index.numpy())
    pk = PackedSegments(plan, torch.device(DEV))
    x_pad, mask_pad, ei_pad = _SegPackFn.apply(pk, b.x.to(DEV), mask.to(DEV), b.edge_index.to(DEV))
    got = (x_pad, mask_pad, ei_pad, pk.row_of, pk.src_of)
    for g, w, what in zip(got, want, ("x_pad", "mask_pad", "edge_index_pad", "row_of", "src_of")):
        assert g.cpu().numpy().dtype == w.dtype and np.array_equal(g.cpu().numpy(), w), (name, what)
    rng = np.random.default_rng(0)
    for f in (4, 3, 132):                                    # 16-byte rows, a width that is not a multiple of four, wide rows
        u = rng.standard_normal((plan.n_pad, f)).astype(np.float32)
        v = rng.standard_normal((plan.n, f)).astype(np.float32)
        assert np.array_equal(pk.gather(torch.from_numpy(u).to(DEV)).cpu().numpy(), np_gather_rows(u, want[3])), (name, f)
        assert np.array_equal(pk.scatter(torch.from_numpy(v).to(DEV)).cpu().numpy(), np_scatter_rows(v, want[3], plan.n_pad)), (name, f)


def test_an_edge_id_out_of_range_is_marked_not_followed():
    b = make_ragged_batch([5, 9, 3])
    ei = b.edge_index.clone()
    ei[0, 1], ei[1, 2] = 17, -4                              # N = 17
    plan = segpack.plan(b._graph_sizes, max_padding=1.0)
    pk = PackedSegments(plan, torch.device(DEV))
    _, _, ei_pad = _SegPackFn.apply(pk, b.x.to(DEV), b.pred_mask.to(DEV), ei.to(DEV))
    assert np.array_equal(ei_pad.cpu().numpy(), np_pack(plan, b.x.numpy(), b.pred_mask.numpy(), ei.numpy())[2])
    assert ei_pad[0, 1].item() == -1 and ei_pad[1, 2].item() == -1


# ------------------------------------------------------------------------------------------------- whole model
def test_mixed_batch_full_size_vs_oracle():
    """Standard configuration, 40 x 118 + 88 x 14 buses: forward against the fp32 and fp64 oracle, the elementwise record, every
    parameter gradient against the fp64 oracle on the exported gates (node gates come back in the caller's row order)."""
    m, ref = _models()
    data = make_ragged_batch(MIXED, seed=0)
    _check_full_size(m, ref, data, "mixed 40x118+88x14")
    assert m.last_segment_plan is not None and (m.last_segment_plan.S, m.last_segment_plan.n_pad) == (118, 51 * 118)


def test_tiny_mixed_batch_with_single_node_graphs_vs_oracle():
    m, ref = _models(h=12, layers=3, K=2, seed=5)
    data = make_ragged_batch(TINY, seed=1)
    _check_full_size(m, ref, data, "tiny mixed {1,5,7,14}")
    assert (m.last_segment_plan.S, m.last_segment_plan.n_pad) == (14, 70)


def test_packed_batch_takes_the_graph_resident_route():
    """A training step on a ragged batch lists the graph-resident kernel classes and the pack / unpack classes; with
    segment_packing off it lists none of them, and computes the same."""
    from poweflownet_amd.loss import MSELoss
    m, _ = _models(p=0.2, train=True)
    d = make_ragged_batch(MIXED, seed=3).to(DEV)
    packed = _run(m, d, MSELoss(), attach=False, x_grad=True)
    for k in SEG_CLASSES + PACK_CLASSES:
        assert packed["launches"].get(k, 0) >= 1, (k, packed["launches"])
    assert packed["launches"]["segpack_rows"] == 1 and packed["launches"]["segpack_edges"] == 1
    m.eval()                                                  # (dropout is keyed by the row: compare the two layouts without it)
    packed = _run(m, d, MSELoss(), attach=False, x_grad=True)
    m.segment_packing = False
    plain = _run(m, d, MSELoss(), attach=False, x_grad=True)
    assert m.last_segment_plan is None
    for k in SEG_CLASSES + PACK_CLASSES:
        assert k not in plain["launches"], (k, plain["launches"])
    assert_close(packed["out"], plain["out"], RTOL, "packed vs unpacked: out")
    assert_close(packed["g"], plain["g"], RTOL, "packed vs unpacked: flat gradient")
    assert_close(packed["gx"], plain["gx"], RTOL, "packed vs unpacked: grad_x")


def _input_grads(m, d, packing):
    """(grad_x, grad_edge_attr, exported gates) of one MSELoss step on `d` with segment packing on or off."""
    from tests.util import _cpu_gates
    m.segment_packing = packing
    m.zero_grad(set_to_none=True)
    x, ea = d.x.clone().requires_grad_(True), d.edge_attr.clone().requires_grad_(True)
    dd = d.clone()
    dd.x, dd.edge_attr = x, ea
    out = m(dd)
    assert (m.last_segment_plan is not None) == packing
    torch.nn.MSELoss()(out, d.y).backward()
    return x.grad.clone(), ea.grad.clone(), _cpu_gates(m)


def test_input_and_edge_attribute_gradients_match_the_unpacked_route():
    """grad_x and grad_edge_attr of the packed route against the unpacked route at RTOL, standard configuration.

    Two fp32 arithmetic orders of this network agree on a gradient only while they take the same ReLU decisions: one
    pre-activation within the forward rounding error of zero flips its gate in one of them and moves the input gradients of the
    rows around it by far more than 1e-5 of the largest entry (tests/util._assert_grads_on_hip_gates; the CPU oracle alone, fp32
    against fp64, 40 x 118 + 88 x 14, seed 3: one flipped gate of ~10^7, grad_x off by 3.8e-5).  The number of decisions grows
    with the batch, so the routes are compared on a batch of the size the existing route-against-route test uses
    (test_fused_front_and_back_equal_generic_gemm_path: 708 rows) -- 6 x 118 + 12 x 14 = 876 rows -- and the test first asserts
    that the two routes DID take the same decisions, so that a flip is reported as what it is.  At 40 x 118 + 88 x 14, seed 4,
    this comparison measured 1.69e-3 of the largest entry (2.0e-7 against 1.2e-4) for grad_x on an MI355X; that size is held
    against the fp64 oracle on each route's own decisions instead (next test)."""
    from tests.util import _gate_differences
    m, _ = _models()
    d = make_ragged_batch([118] * 6 + [14] * 12, seed=4).to(DEV)
    gx_p, gea_p, gates_p = _input_grads(m, d, True)
    gx_u, gea_u, gates_u = _input_grads(m, d, False)
    flips = _gate_differences(gates_p, gates_u)
    assert sum(flips.values()) == 0, f"the two routes took different ReLU decisions, the gradients are not comparable: {flips}"
    assert_close(gx_p, gx_u, RTOL, "grad_x: packed vs unpacked")
    assert_close(gea_p, gea_u, RTOL, "grad_edge_attr: packed vs unpacked")


def test_input_and_edge_attribute_gradients_at_full_size_vs_fp64_oracle():
    """40 x 118 + 88 x 14: grad_x and grad_edge_attr of either route against the float64 oracle held to THAT route's ReLU
    decisions, at north_star's 1e-5 -- the yardstick the parameter gradients are held to (_assert_grads_on_hip_gates)."""
    import copy
    from tests.util import _to64
    m, ref = _models()
    data = make_ragged_batch(MIXED, seed=4)
    d = data.to(DEV)
    torch.set_num_threads(min(32, os.cpu_count() or 8))
    for packing in (True, False):
        gx, gea, gates = _input_grads(m, d, packing)
        ref64 = copy.deepcopy(ref).double()
        ref64.zero_grad(set_to_none=True)
        ref64.gates = gates
        d64 = _to64(data)
        d64.x, d64.edge_attr = d64.x.clone().requires_grad_(True), d64.edge_attr.clone().requires_grad_(True)
        torch.nn.MSELoss()(ref64(d64), d64.y).backward()
        assert_close(gx, d64.x.grad.float(), RTOL, f"grad_x vs fp64 oracle on the HIP gates, packing {packing}")
        assert_close(gea, d64.edge_attr.grad.float(), RTOL, f"grad_edge_attr vs fp64 oracle on the HIP gates, packing {packing}")


def test_train_mode_matches_oracle_fed_the_exported_masks():
    """Dropout is keyed by the PADDED row: the exported keep masks (pfn_dropout_mask over n_pad rows) are moved into the caller's
    row order through row_of and fed to the oracle; then as tests/test_gpu_parity.py does for uniform batches."""
    m, ref = _models(p=0.2, seed=99, train=True)
    m.seed_dropout(31337)
    data = make_ragged_batch(MIXED, seed=3)
    dd = data.to(DEV)
    out = m(dd)
    torch.nn.MSELoss()(out, dd.y).backward()
    pk = m.last_segment_plan
    ref.dropout_masks = [pk.gather(k).cpu() for k in _exported_masks(m, pk.n_pad)]
    torch.set_num_threads(min(32, os.cpu_count() or 8))
    out_ref = ref(data)
    out64, _ = _fp64_truth(ref, data)
    assert_close(out, out_ref, RTOL, "mixed train-mode out")
    assert_close(out, out64.float(), RTOL, "mixed train-mode out vs fp64")
    _assert_grads_on_hip_gates(m, ref, data, "mixed train mode", out)


def test_attach_is_transparent_on_a_packed_forward():
    from poweflownet_amd.loss import MSELoss
    m, _ = _models(p=0.2, train=True)
    d = make_ragged_batch(MIXED, seed=6).to(DEV)
    loss_fn = MSELoss()
    plain = _run(m, d, loss_fn, attach=False, x_grad=True)
    fused = _run(m, d, loss_fn, attach=True, x_grad=True)
    assert m._mse_attach is None
    assert "ea_seg_bwd+out+mse" not in fused["launches"] and fused["launches"] == plain["launches"]
    for k in ("out", "loss", "g", "gx"):
        assert torch.equal(fused[k], plain[k]), k


def test_equal_counts_of_two_sizes_stay_finite_batch_after_batch():
    """32 x 118 + 32 x 14 divides evenly into "66-node graphs": the hint N // n_graphs is rejected by the first, validated build
    and taken on trust by every later build of the same shape, which then poisons the output.  A batch that carries its size list
    never gets that hint, packed or not."""
    m, ref = _models()
    sizes = [118] * 32 + [14] * 32
    for packing in (True, False):
        m.segment_packing = packing
        for rep in range(3):
            data = make_ragged_batch(sizes, seed=10 + rep)
            with torch.no_grad():
                out = m(data.to(DEV))
                want = ref(data)
            assert torch.isfinite(out).all(), (packing, rep)
            assert_close(out, want, RTOL, f"equal counts, packing {packing}, batch {rep}")
    assert m._graphs.device_rebuilds >= 2


def test_batches_with_ptr_but_no_size_list_stay_finite_batch_after_batch():
    """What a real PyG loader hands over: `ptr`, no host-side size list.  14 + 6 + 14 + 6 = 40 rows in 4 graphs divides into
    "10-node graphs"; the first, validated build rejects that hint, and the cache remembers it (_GraphCache._rejected): every later
    tensor of the shape -- built unverified, the checks left on the device -- gets no hint instead of the rejected one on trust
    (which poisoned every output).  Three fresh batches (new tensors, new samples), then a UNIFORM batch of the very same shape
    (4 x 10 nodes, the same 58 stored edges), which would have honoured the hint and now merely runs on the generic kernels.
    (`dynamic_topology=True` has no validated build to learn from and is left as it is: there the hint is the caller's promise.)"""
    from poweflownet_amd.data import Batch
    from poweflownet_amd.synth import make_graph, make_topology
    m, ref = _models(h=33, layers=3, K=2, seed=7)
    sizes = [14, 6, 14, 6]
    shape = None
    for rep in range(3):
        data = make_ragged_batch(sizes, seed=20 + rep)
        del data.__dict__["_graph_sizes"]
        assert data.ptr.tolist() == [0, 14, 20, 34, 40]
        shape = tuple(data.edge_index.shape)
        with torch.no_grad():
            out = m(data.to(DEV))
            want = ref(data)
        assert m._graphs._graph.seg_nodes == 0, rep
        assert torch.isfinite(out).all(), rep
        assert_close(out, want, RTOL, f"ptr without a size list, batch {rep}")
    assert m._graphs.device_rebuilds >= 2
    edges = [15, 14, 15, 14]
    uniform = Batch.from_data_list([make_graph(10, e, seed=90 + g, edge_index=make_topology(10, e, g)) for g, e in enumerate(edges)])
    del uniform.__dict__["_graph_sizes"]
    assert tuple(uniform.edge_index.shape) == shape and uniform.x.shape[0] == 40
    with torch.no_grad():
        out = m(uniform.to(DEV))
        want = ref(uniform)
    assert m._graphs.device_rebuilds >= 3 and m._graphs._graph.seg_nodes == 0
    assert torch.isfinite(out).all()
    assert_close(out, want, RTOL, "a uniform batch of the shape whose hint was rejected")


def test_a_size_list_that_lies_raises_on_the_validated_build():
    m, _ = _models(h=12, layers=2, K=2)
    d = make_ragged_batch([14, 5, 14, 5]).to(DEV)
    d._graph_sizes = (5, 14, 14, 5)              # graph 0's edges now join the "graphs" 0 and 1, which the plan puts in two segments
    with pytest.raises(RuntimeError, match="size list"):
        m(d)
    d._graph_sizes = (14, 5, 14, 6)
    with pytest.raises(RuntimeError, match="adds up"):
        m(d)


def test_uniform_batches_and_batches_without_a_size_list_run_none_of_it():
    m, _ = _models()
    uniform = make_batch("14", 8).to(DEV)
    ragged = make_ragged_batch([118, 14, 14, 14]).to(DEV)      # 47.5 % padding: the cap rejects it
    bare = make_ragged_batch(MIXED).to(DEV)
    del bare.__dict__["_graph_sizes"]
    for d in (uniform, ragged, bare):
        L.profile_report(reset=True)
        L.profile_enable(True)
        with torch.no_grad():
            m(d)
        torch.cuda.synchronize()
        L.profile_enable(False)
        rep = L.profile_report(reset=True)
        assert m.last_segment_plan is None and not any(k.startswith("segpack") for k in rep), sorted(rep)


def test_train_epoch_over_a_mixed_device_resident_dataset(tmp_path):
    from poweflownet_amd.data import DataLoader
    from poweflownet_amd.datasets import PowerFlowData
    from poweflownet_amd.loss import MSELoss
    from poweflownet_amd.optim import FlatAdamW
    from poweflownet_amd.utils.training import train_epoch
    ds = PowerFlowData(root=_mixed_root(tmp_path, samples=48), case="mixed", split=[.5, .25, .25], task="train", device=DEV)
    assert len(ds) == 48 and ds.device.type == "cuda"
    torch.manual_seed(2)
    m = MaskEmbdMultiMPN(4, 2, 4, 16, 3, 2, 0.1).to(DEV)
    m.segment_packing = True
    opt = FlatAdamW(m, lr=1e-3)
    loader = DataLoader(ds, batch_size=12, shuffle=True, generator=torch.Generator().manual_seed(1))
    packed = 0
    orig = m._forward_packed

    def counting(*a, **k):
        nonlocal packed
        packed += 1
        return orig(*a, **k)
    m._forward_packed = counting
    losses = [train_epoch(m, loader, MSELoss(), opt, DEV) for _ in range(2)]
    assert all(np.isfinite(l) and l > 0 for l in losses), losses
    assert packed >= 1
