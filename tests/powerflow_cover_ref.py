"""A plain restatement of the cover route's two host rules (poweflownet_amd/utils/powerflow.py cover_list, csrc/powerflow_cover.hip),
with dictionaries and loops where the product sorts arrays: the cover list of a chunk of per-sample line lists, and the slot rule
that places a sample's lines in it.  A line's key is its unordered bus pair."""
from collections import Counter, defaultdict

import numpy as np


def key(a, b):
    return (min(int(a), int(b)), max(int(a), int(b)))


def cover(samples, base=None):
    """int64 [2, e_cover]: `base` [2, e0] as it stands, then, ascending by key and oriented (min, max), as many further copies of
    every pair as the sample that holds it most often needs beyond the base's count."""
    base = np.zeros((2, 0), dtype=np.int64) if base is None else np.asarray(base, dtype=np.int64)
    have = Counter(key(a, b) for a, b in base.T)
    need = Counter()
    for s in samples:
        for q, c in Counter(key(a, b) for a, b in np.asarray(s).T).items():
            need[q] = max(need[q], c)
    extra = [q for q in sorted(need) for _ in range(need[q] - have[q])]
    return np.concatenate([base, np.array(extra, dtype=np.int64).reshape(-1, 2).T], axis=1)


def slots(sample, cover_list, n):
    """[e]: the cover line of every line of `sample` [2, e] -- its k-th line with a key takes the k-th cover line with that key --
    or -1: no such cover line, a bus outside [0, n), one bus twice."""
    places = defaultdict(list)
    for c, (a, b) in enumerate(np.asarray(cover_list).T):
        places[key(a, b)].append(c)
    taken, out = Counter(), []
    for a, b in np.asarray(sample).T:
        if not (0 <= a < n and 0 <= b < n) or a == b:
            out.append(-1)
            continue
        q = key(a, b)
        out.append(places[q][taken[q]] if taken[q] < len(places.get(q, ())) else -1)
        taken[q] += 1
    return np.array(out, dtype=np.int64)


def cover_map(samples, rx, cover_list, n, fill=np.nan):
    """(line_mask uint8 [S, e_cover], rx_cover float64 [S, e_cover, 2] with `fill` where the mask is 0, unplaced int32 [S])"""
    S, ec = len(samples), np.asarray(cover_list).shape[1]
    mask, out, unplaced = np.zeros((S, ec), dtype=np.uint8), np.full((S, ec, 2), fill, dtype=np.float64), np.zeros(S, dtype=np.int32)
    for s in range(S):
        where = slots(samples[s], cover_list, n)
        mask[s, where[where >= 0]] = 1
        out[s, where[where >= 0]] = np.asarray(rx[s])[where >= 0]
        unplaced[s] = int((where < 0).sum())
    return mask, out, unplaced
