"""The topology perturbation without a GPU: the yardstick itself (tests/topology_ref.py -- Philox known answers, the structure and
the uniformity of its draws, the give-up path) and the refusals of the Python wrapper and the C entry points that need no device.
tests/test_gpu_topology.py holds csrc/topology.hip to this yardstick bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

from poweflownet_amd import _lib as L
from poweflownet_amd.synth import make_topology
from poweflownet_amd.utils.topology import PerturbedTopology, perturb_topology, unsupplied_buses
from tests import topology_ref as T


# ------------------------------------------------------------------------------------------------- Philox
KNOWN = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
         ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
         ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1")]


def _project_round_function(c, k0, k1):
    """csrc/pfn_internal.hpp philox4x32_10, statement by statement: one 64-bit product per multiplier, the key bumped per round."""
    c = [int(x) for x in c]
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        hi0, lo0, hi1, lo1 = p0 >> 32, p0 & 0xFFFFFFFF, p1 >> 32, p1 & 0xFFFFFFFF
        c = [hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c


@pytest.mark.parametrize("counter, key, want", KNOWN)
def test_philox_known_answers(counter, key, want):
    assert " ".join(f"{int(w):08x}" for w in T.philox4x32_10(*counter, *key)) == want
    assert " ".join(f"{w:08x}" for w in _project_round_function(counter, *key)) == want


def test_philox_is_elementwise():
    """The yardstick draws a whole line list per call: element j of an array call is the scalar call of counter j."""
    w = T.philox4x32_10(np.arange(50, dtype=np.uint64), 3, 2 ** 32 - 1, 1, 7, 9)
    for j in (0, 17, 49):
        assert [int(x[j]) for x in w] == [int(x) for x in T.philox4x32_10(j, 3, 2 ** 32 - 1, 1, 7, 9)]


# ------------------------------------------------------------------------------------------------- structure
def _components(n, lines):
    parent = list(range(n))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i
    for f, t in lines:
        parent[find(int(f))] = find(int(t))
    return len({find(i) for i in range(n)})


@pytest.mark.parametrize("seed", [7, 2024])
def test_structure_of_a_draw(seed):
    n, e, r, a, S = 14, 20, 2, 1, 256
    base = make_topology(n, e).numpy()
    out, source, status = T.perturb(base, n, S, r, a, seed)
    print(f"seed {seed}: {int((status < 0).sum())} failures, at most {status.max()} attempts, mean {status.mean():.2f}")
    assert out.shape == (S, 2, 19) and source.shape == (S, 19) and out.dtype == np.int64 and source.dtype == np.int32
    assert (status >= 1).all() and status.max() <= 20
    kept = source[:, :e - r]
    assert (np.diff(kept, axis=1) > 0).all()                                  # base order, no line twice: exactly r are absent
    assert all(len(set(range(e)) - set(row)) == r for row in kept)
    assert (out[:, :, :e - r] == base[:, kept].transpose(1, 0, 2)).all()
    added = out[:, :, e - r:]
    assert (added >= 0).all() and (added < n).all() and (added[:, 0] != added[:, 1]).all()
    assert (source[:, e - r:] >= 0).all() and (source[:, e - r:] < e).all()
    for s in range(S):                                                        # connected BEFORE the added line, as the rule accepts it
        assert _components(n, out[s, :, :e - r].T) == 1


def test_removed_line_is_uniform_over_the_lines_that_may_leave():
    n, e, S = 14, 20, 4000
    base = make_topology(n, e).numpy()
    bridges = [j for j in range(e) if _components(n, np.delete(base, j, axis=1).T) > 1]
    assert bridges == [1, 3, 5]
    _, source, status = T.perturb(base, n, S, 1, 0, seed=7)
    assert (status >= 1).all()
    removed = np.array([(set(range(e)) - set(row)).pop() for row in source])
    counts = np.bincount(removed, minlength=e)
    assert counts[bridges].sum() == 0
    others = np.delete(counts, bridges)
    chi2 = float(((others - S / 17) ** 2 / (S / 17)).sum())
    print(f"chi-square of the 17 counts: {chi2:.1f}")
    assert chi2 < 39.25                                                       # the 99.9 % point of 16 degrees of freedom


def test_give_up_path():
    n, e = 8, 10
    base = make_topology(n, e).numpy()
    out, source, status = T.perturb(base, n, 256, 3, 0, seed=7)
    failed = status == -1
    print(f"{int(failed.sum())} of 256 without a connected draw")
    assert 0 < failed.sum() < 256 and ((status >= 1) | failed).all() and status.max() <= 20
    assert (out[failed] == -1).all() and (source[failed] == -1).all()
    assert (out[~failed] >= 0).all() and all(_components(n, x.T) == 1 for x in out[~failed])
    # one attempt only: more samples fail, and those that pass used one
    _, _, once = T.perturb(base, n, 256, 3, 0, seed=7, max_attempts=1)
    assert ((once == 1) == (status == 1)).all() and (once[status != 1] == -1).all()


def test_yardstick_counts_and_bad_ids():
    ring = np.stack([np.arange(6), (np.arange(6) + 1) % 6])
    assert T.unsupplied(ring, 6) == 0 and T.unsupplied(ring[:, :3], 6, root=1) == 2
    assert T.unsupplied(np.array([[1], [2]]), 4, root=0) == 3                 # an isolated root
    assert T.unsupplied(np.array([[0], [4]]), 4) == -4
    out, source, status = T.perturb(np.array([[0, 1, 2], [1, 2, 3]]), 3, 4, 0, 0, 1)
    assert (status == -4).all() and (out == -1).all() and (source == -1).all()
    out, source, status = T.perturb(ring, 6, 3, 0, 0, 1)
    assert (status == 1).all() and (out == ring).all() and (source == np.arange(6)).all()


# ------------------------------------------------------------------------------------------------- refusals
def test_python_wrapper_refusals():
    base = make_topology(14, 20)
    ok = dict(num_samples=4, remove=1, add=1)
    for bad, match in ((dict(remove=-1), "remove"), (dict(add=-2), "add"), (dict(remove=21), "21 of 20"), (dict(remove=8), "cannot connect"),
                       (dict(root=14), "root"), (dict(root=-1), "root"), (dict(max_attempts=0), "max_attempts"),
                       (dict(max_attempts=1025), "1025"), (dict(num_samples=-1), "num_samples"), (dict(seed=-1), "seed"),
                       (dict(seed=1 << 64), "seed"), (dict(first_sample=-1), "first_sample"), (dict(first_sample=(1 << 32) - 3), "32-bit"),
                       (dict(remove=1.0), "remove")):
        with pytest.raises(ValueError, match=match):
            perturb_topology(base, 14, **{**ok, **bad})
    with pytest.raises(ValueError, match="n_bus"):
        perturb_topology(base, 0, **ok)
    with pytest.raises(ValueError, match="cannot add"):
        perturb_topology(torch.zeros(2, 0, dtype=torch.int64), 1, num_samples=1, add=1)
    with pytest.raises(RuntimeError, match=r"int64 tensor \(2, e\).*int32"):
        perturb_topology(base.int(), 14, **ok)
    with pytest.raises(RuntimeError, match=r"\(4, 2, 20\)"):                   # a per-sample list is not a base grid
        perturb_topology(base.expand(4, 2, 20), 14, **ok)
    with pytest.raises(RuntimeError, match=r"\(20, 2\)"):
        perturb_topology(base.T, 14, **ok)
    with pytest.raises(RuntimeError, match="no CPU fallback"):                 # everything else is in order: there is no CPU path
        perturb_topology(base, 14, **ok)
    with pytest.raises(ValueError, match="root"):
        unsupplied_buses(base, 14, root=14)
    with pytest.raises(RuntimeError, match=r"\(2, e\) or \(S, 2, e\).*float32"):
        unsupplied_buses(base.float(), 14)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        unsupplied_buses(base.expand(3, 2, 20), 14)
    assert set(PerturbedTopology.__dataclass_fields__) == {"edge_index", "source", "status"}


def test_library_refusals_launch_nothing():
    """PFN_EINVAL before any device call, so these answer without a GPU; the pointers are host buffers nothing dereferences."""
    lib = L.load()
    buf = (C.c_int64 * 64)()
    p = C.addressof(buf)

    def perturb(e=20, n=14, S=4, first=0, r=1, a=1, seed=0, root=0, attempts=20):
        return lib.pfn_topology_perturb(p, e, n, S, first, r, a, seed, root, attempts, p, p, p, None)
    for kw, text in ((dict(r=-1), b"remove -1"), (dict(a=-1), b"add -1"), (dict(r=21), b"remove 21"), (dict(r=8), b"cannot connect"),
                     (dict(e=0, n=1, r=0, a=1), b"cannot be added"), (dict(root=14), b"root 14"), (dict(root=-1), b"root -1"),
                     (dict(attempts=0), b"max_attempts 0"), (dict(attempts=1025), b"max_attempts 1025"),
                     (dict(first=-1), b"32-bit"), (dict(first=(1 << 32) - 3), b"32-bit"),
                     (dict(e=40000, n=6470), b"bytes of LDS")):
        assert perturb(**kw) == -1 and text in lib.pfn_last_error(), (kw, lib.pfn_last_error())
    assert lib.pfn_topology_unsupplied(p, 0, 20, 4, 14, 14, p, None) == -1 and b"root 14" in lib.pfn_last_error()
    assert lib.pfn_topology_unsupplied(p, 0, 60000, 4, 6470, 0, p, None) == -1 and b"bytes of LDS" in lib.pfn_last_error()
    # no samples: nothing to do, nothing launched
    assert perturb(S=0) == 0 and lib.pfn_topology_unsupplied(p, 1, 20, 0, 14, 0, p, None) == 0


# ------------------------------------------------------------------------------------------------- generator, host side
def test_generator_flags_and_per_sample_raw_files(tmp_path, capsys):
    import dataset_generator
    with pytest.raises(SystemExit) as ex:                                     # refused while parsing, before a device is asked for
        dataset_generator.main(["--case", "14", "--samples", "4", "--root", str(tmp_path), "-r", "-1"])
    assert ex.value.code == 2 and "at least 0" in capsys.readouterr().err
    base = make_topology(14, 20).numpy()
    out, source, status = T.perturb(base, 14, 3, 1, 1, seed=0)
    rng = np.random.default_rng(0)
    rx, tables = rng.uniform(0.01, 0.1, (3, 20, 2)), rng.normal(size=(3, 14, 4))
    bus_type = np.where(np.arange(14) == 0, 0, 2)
    paths = dataset_generator.write_raw(str(tmp_path), "14perturbed1r1a", bus_type, out, rx, tables)
    assert [p.split("/")[-1] for p in paths] == ["case14perturbed1r1a_node_features.npy", "case14perturbed1r1a_edge_features.npy"]
    node, edge = np.load(paths[0]), np.load(paths[1])
    assert node.shape == (3, 14, 6) and edge.shape == (3, 20, 4)
    assert (edge[:, :, :2].transpose(0, 2, 1) == out).all() and (edge[:, :, 2:] == rx).all() and (node[:, :, 2:] == tables).all()
    paths = dataset_generator.write_raw(str(tmp_path), "14", bus_type, base, rx, tables)      # one list for all samples, as before
    assert (np.load(paths[1])[:, :, :2] == base.T).all()
