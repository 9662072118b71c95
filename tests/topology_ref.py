"""The float-free numpy yardstick of the topology perturbation (include/pfn_hip.h "topology perturbation" states the rule): Philox4x32-10
from the paper (Salmon et al., SC'11), the removal / addition draws word for word, reachability by plain propagation.  It imports
nothing of the library; tests hold csrc/topology.hip to it bit for bit."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
LO = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Four uint32 output words (arrays broadcast together) of counter (c0, c1, c2, c3) under key (k0, k1)."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & LO for c in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2                 # 32 x 32 -> 64 bits: exact in uint64
        hi0, lo0, hi1, lo1 = p0 >> S32, p0 & LO, p1 >> S32, p1 & LO
        c0, c1, c2, c3 = hi1 ^ c1 ^ np.uint64(k0), lo1, hi0 ^ c3 ^ np.uint64(k1), lo0
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return tuple(c.astype(np.uint32) for c in (c0, c1, c2, c3))


def unsupplied(edge_index, n_bus, root=0, keep=None):
    """Buses not reachable from `root` over the lines of one [2, e] list (those with keep[j] where given); -4 for an id outside [0, n)."""
    ei = np.asarray(edge_index, dtype=np.int64)
    if ((ei < 0) | (ei >= n_bus)).any():
        return -4
    f, t = (ei[0], ei[1]) if keep is None else (ei[0][keep], ei[1][keep])
    reached = np.zeros(n_bus, dtype=bool)
    reached[root] = True
    while True:
        rf, rt = reached[f], reached[t]
        grow = rf != rt
        if not grow.any():
            return int(n_bus - reached.sum())
        reached[f[grow]] = True
        reached[t[grow]] = True


def unsupplied_batch(edge_index, n_bus, root=0):
    ei = np.asarray(edge_index, dtype=np.int64)
    return np.array([unsupplied(x, n_bus, root) for x in (ei if ei.ndim == 3 else ei[None])], dtype=np.int32)


def perturb(edge_index, n_bus, num_samples, remove=0, add=0, seed=0, first_sample=0, root=0, max_attempts=20):
    """(edge_index_out [S, 2, e_out] int64, source [S, e_out] int32, status [S] int32) by the rule of include/pfn_hip.h."""
    ei = np.asarray(edge_index, dtype=np.int64)
    e, n, r, a = ei.shape[1], int(n_bus), int(remove), int(add)
    assert 0 <= r <= e and a >= 0 and e - r >= n - 1 and (a == 0 or n >= 2) and 0 <= root < n and 1 <= max_attempts <= 1024
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    e_out = e - r + a
    out = np.full((num_samples, 2, e_out), -1, dtype=np.int64)
    source = np.full((num_samples, e_out), -1, dtype=np.int32)
    status = np.full(num_samples, -1, dtype=np.int32)
    if ((ei < 0) | (ei >= n)).any():
        status[:] = -4
        return out, source, status
    lines = np.arange(e, dtype=np.uint64)
    for s in range(num_samples):
        sample = first_sample + s
        for attempt in range(max_attempts):
            key = philox4x32_10(lines, attempt, sample, 0, k0, k1)[0]
            packed = (key.astype(np.uint64) << S32) | lines
            keep = np.ones(e, dtype=bool)
            keep[np.argsort(packed, kind="stable")[:r]] = False
            if unsupplied(ei, n, root, keep) == 0:
                status[s] = attempt + 1
                break
        else:
            continue
        kept = np.flatnonzero(keep)
        out[s, :, :e - r] = ei[:, kept]
        source[s, :e - r] = kept
        if a:
            w = philox4x32_10(np.arange(a, dtype=np.uint64), 0, sample, 1, k0, k1)
            w0, w1, w2 = (x.astype(np.int64) for x in w[:3])
            frm = w0 % n
            out[s, 0, e - r:] = frm
            out[s, 1, e - r:] = (frm + 1 + w1 % (n - 1)) % n
            source[s, e - r:] = w2 % e
    return out, source, status
