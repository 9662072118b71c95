"""Host-side checks of the k-hop locality analysis (poweflownet_amd/utils/explanation.py): the center-sampling sequence of the
reference's explain_epoch and the instance planning (saturation dedupe, chunking, offsets).  No GPU needed."""
import numpy as np
import pytest

from poweflownet_amd.utils.explanation import InstancePlan, instance_offsets, sample_centers, saturation_radius


def _reference_draws(num_nodes, num_batches):
    """The np.random calls of the reference's explain_epoch (utils/explanation.py:66-85), restated."""
    num_node_sample = 350
    if num_nodes > 1000:
        np.random.choice(num_node_sample, 350, replace=False).tolist()
    else:
        np.arange(num_nodes).tolist()
    out = []
    for _ in range(num_batches):
        if num_nodes > 1000:
            out.append(np.random.choice(num_nodes, 350, replace=False).tolist())
        else:
            out.append(np.arange(num_nodes).tolist())
    return out


@pytest.mark.parametrize("num_nodes", [118, 1200, 6470])
@pytest.mark.parametrize("seed", [0, 1, 1234])
def test_center_sampling_follows_the_reference_sequence(num_nodes, seed):
    np.random.seed(seed)
    want = _reference_draws(num_nodes, 5)
    after_ref = np.random.random()
    np.random.seed(seed)
    got = sample_centers(num_nodes, 5)
    assert got == want
    assert np.random.random() == after_ref                     # the generator is left where the reference leaves it
    if num_nodes > 1000:
        assert all(len(set(c)) == 350 and max(c) < num_nodes for c in got)
        assert got[0] != got[1]                                # a fresh draw per batch
    else:
        assert got[0] == list(range(num_nodes))


def _synthetic_histograms(rng, centers, rmax):
    """Cumulative ball sizes that grow until a per-center saturation radius, then stay flat."""
    sat = rng.integers(0, rmax + 1, size=centers)
    nc = np.zeros((centers, rmax + 1), dtype=np.int64)
    ec = np.zeros_like(nc)
    for c in range(centers):
        grow = rng.integers(1, 9, size=rmax + 1)
        grow[0] = 1
        grow[sat[c] + 1:] = 0
        nc[c] = np.cumsum(grow)
        ec[c] = np.cumsum(np.where(np.arange(rmax + 1) == 0, 0, 2 * grow + rng.integers(0, 3, size=rmax + 1) * (grow > 0)))
    return nc, ec, sat


@pytest.mark.parametrize("seed", [0, 3, 11])
@pytest.mark.parametrize("samples", [1, 3])
def test_instance_plan_dedupes_saturated_radii_and_chunks_under_budget(seed, samples):
    rng = np.random.default_rng(seed)
    nc, ec, sat = _synthetic_histograms(rng, 37, 12)
    assert (saturation_radius(nc) == sat).all()
    radii = [0, 1, 2, 5, 7, 12, 3]
    budget = 40
    p = InstancePlan(nc, ec, radii, samples, budget)
    # every (center, radius, sample) answered by the instance (center, min(radius, saturation), sample)
    for c in range(37):
        for j, r in enumerate(radii):
            for s in range(samples):
                i = p.index[c, j, s]
                assert (p.inst_row[i], p.inst_radius[i], p.inst_sample[i]) == (c, min(r, sat[c]), s)
                assert p.node_size[i] == nc[c, min(r, sat[c])] and p.edge_size[i] == ec[c, min(r, sat[c])]
            assert p.node_count[c, j] == nc[c, r]              # saturated sizes equal the true ball sizes
    keys = set(zip(p.inst_row.tolist(), p.inst_radius.tolist(), p.inst_sample.tolist()))
    assert len(keys) == p.num_instances                        # each instance once
    want = sum(len({min(r, sat[c]) for r in radii}) for c in range(37)) * samples
    assert p.num_instances == want
    # chunks: contiguous cover of [0, I); each within the budget unless it is a single instance; greedy (the next instance
    # would not have fit)
    assert p.chunks[0][0] == 0 and p.chunks[-1][1] == p.num_instances
    for (a, b), (a2, _) in zip(p.chunks, p.chunks[1:]):
        assert b == a2
    for k, (a, b) in enumerate(p.chunks):
        size = int(p.node_size[a:b].sum())
        assert size <= budget or b - a == 1
        if k + 1 < len(p.chunks):
            assert size + int(p.node_size[b]) > budget


def test_instance_offsets_are_exclusive_prefix_sums():
    sizes = [3, 0, 5, 1]
    assert instance_offsets(sizes).tolist() == [0, 3, 3, 8, 9]
    assert instance_offsets([]).tolist() == [0]
    assert instance_offsets(np.array([2], dtype=np.int32)).dtype == np.int64


def test_instance_plan_rejects_bad_radii():
    nc = np.array([[1, 2, 2]])
    with pytest.raises(ValueError):
        InstancePlan(nc, nc, [3], 1, 10)
    with pytest.raises(ValueError):
        InstancePlan(nc, nc, [-1], 1, 10)
    with pytest.raises(ValueError):
        InstancePlan(nc, nc, [0], 1, 0)
