"""update_memory_surp_base (memory_2.py:364-536) restated in plain NumPy for the tests.

Row by row, in order, over every cache row: create a missing group; otherwise the surprise min(1 - cos) against the tokens
of the existing groups at the (2r+1)^3 - 1 surrounding positions (+inf with none, NaN when any token is zero), compared in
double with the threshold; a surprising token is appended or overwrites the slot of the first NaN / first minimum of
1 - cos, then the group is rewritten with one token per component of sim > boring_threshold, in the order of each
component's smallest index.  Cosines are taken in f64 (the margins recorded below say how far the data keeps them from
every decision); a merged token is torch.mean of f32 rows (sequential f32 sum, then / n), a merged distance the f64 mean.
"""
from itertools import product

import numpy as np

PATHS = ("create", "reject", "nan_reject", "append", "replace", "replace_nan", "merge")


def name_key(p):
    return "grid_%d_%d_%d" % tuple(int(v) for v in p)


def store_from_arrays(pos, cnt, feats, dists):
    """{(r, c, h): [features list (f32 rows), distances list (float), merged flags]} from name-ordered arrays."""
    st, t = {}, 0
    for p, c in zip(np.asarray(pos).reshape(-1, 3), np.asarray(cnt).reshape(-1)):
        c = int(c)
        st[tuple(int(v) for v in p)] = [[np.asarray(feats[t + k], np.float32).copy() for k in range(c)],
                                        [float(dists[t + k]) for k in range(c)], [False] * c]
        t += c
    return st


def store_to_arrays(st, D):
    keys = sorted((k for k in st if st[k][0]), key=name_key)
    pos = np.array(keys, np.int32).reshape(-1, 3)
    cnt = np.array([len(st[k][0]) for k in keys], np.int32)
    feats = np.stack([f for k in keys for f in st[k][0]]) if keys else np.zeros((0, D), np.float32)
    dists = np.array([d for k in keys for d in st[k][1]], np.float64)
    merged = np.array([m for k in keys for m in st[k][2]], bool)
    return pos, cnt, feats.astype(np.float32), dists, merged


def _unit(rows):
    rows = np.asarray(rows, np.float64)
    n = np.linalg.norm(rows, axis=-1, keepdims=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(n > 0, rows / np.where(n > 0, n, 1), np.nan)


def replay(st, cache_pos, cache_feat, cache_dis, radius=1, surprise_threshold=0.5, boring_threshold=0.95, cache_size=10):
    """Run the policy over the cache rows on the store `st` (modified in place).  Returns (path counts, margins):
    margins['surprise'] / ['boring'] are the smallest distances of a compared value to its threshold, ['argmin'] the smallest
    gap between the two smallest 1 - cos of a replacement without NaN."""
    offs = [o for o in product(range(-radius, radius + 1), repeat=3) if o != (0, 0, 0)]
    counts = dict.fromkeys(PATHS, 0)
    margins = {"surprise": np.inf, "boring": np.inf, "argmin": np.inf}
    bt = float(np.float32(boring_threshold))       # memory_2.py:408: an f32 matrix against the threshold
    for i in range(len(cache_pos)):
        p = tuple(int(v) for v in cache_pos[i])
        x = np.asarray(cache_feat[i], np.float32)
        d = float(cache_dis[i])
        g = st.get(p)
        if g is None or not g[0]:
            st[p] = [[x.copy()], [d], [False]]
            counts["create"] += 1
            continue
        nb = []
        for o in offs:
            q = st.get((p[0] + o[0], p[1] + o[1], p[2] + o[2]))
            if q is not None:
                nb.extend(q[0])
        if not nb:
            s = np.inf
        else:
            cos = _unit(np.stack(nb)) @ _unit(x)
            s = np.nan if np.isnan(cos).any() else float(np.min(1.0 - cos))
        if np.isfinite(s):
            margins["surprise"] = min(margins["surprise"], abs(s - surprise_threshold))
        if not s > surprise_threshold:
            counts["nan_reject" if np.isnan(s) else "reject"] += 1
            continue
        feats, dists, merged = g
        if len(feats) < cache_size:
            feats.append(x.copy()); dists.append(d); merged.append(False)
            counts["append"] += 1
        else:
            cd = 1.0 - _unit(np.stack(feats)) @ _unit(x)
            nan = np.isnan(cd)
            if nan.any():
                k = int(np.argmax(nan))
                counts["replace_nan"] += 1
            else:
                k = int(np.argmin(cd))
                if len(cd) > 1:      # cache_size 1: nothing to choose between
                    srt = np.sort(cd)
                    margins["argmin"] = min(margins["argmin"], float(srt[1] - srt[0]))
            counts["replace"] += 1
            feats[k], dists[k], merged[k] = x.copy(), d, False
        n = len(feats)
        if n < 2:
            continue
        u = _unit(np.stack(feats))
        sim = u @ u.T
        iu = np.triu_indices(n, 1)
        fin = sim[iu][~np.isnan(sim[iu])]
        if fin.size:
            margins["boring"] = min(margins["boring"], float(np.min(np.abs(fin - bt))))
        with np.errstate(invalid="ignore"):
            adj = sim > bt
        comp = [-1] * n
        for a in range(n):
            if comp[a] >= 0:
                continue
            comp[a], stack = a, [a]
            while stack:
                b = stack.pop()
                for c in np.nonzero(adj[b])[0]:
                    if comp[c] < 0:
                        comp[c] = a
                        stack.append(c)
        nf, nd, nm = [], [], []
        for a in range(n):
            if comp[a] != a:
                continue
            mem = [b for b in range(n) if comp[b] == a]
            if len(mem) == 1:
                nf.append(feats[a]); nd.append(dists[a]); nm.append(merged[a])
            else:
                acc = feats[mem[0]].copy()
                for b in mem[1:]:
                    acc = acc + feats[b]
                nf.append(acc / np.float32(len(mem)))
                nd.append(float(np.sum(np.array([dists[b] for b in mem], np.float64))) / len(mem))
                nm.append(True)
                counts["merge"] += 1
        g[0], g[1], g[2] = nf, nd, nm
    return counts, margins
