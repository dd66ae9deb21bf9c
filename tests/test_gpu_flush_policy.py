"""bsc_set_flush_policy: the flush bsc_ingest runs when a passing point meets a full cache (memory_2.py:880-881) under the
surprise policy, against the replay (tests/surprise_replay.py) over the list of passing rows."""
import math
import random

import numpy as np
import pytest

import flush_policy_cases as FC
import surprise_replay as R
from test_gpu_surprise import _dist_replay, assert_store_matches

pytestmark = pytest.mark.gpu

DIMS = (8, 520)              # 520: not a multiple of 64 lanes x 4
_rows, _exp = {}, {}


def _engine(D, iter_size, mode="exact", **kw):
    import bsc_nav_amd as B
    return B.VoxelEngine(FC.H, FC.W, FC.GS, FC.CELL, FC.FLOOR, FC.TOP, FC.G, D, mode=mode, iter_size=iter_size,
                         cache_size=FC.CS, max_points=FC.F * FC.H * FC.W, **kw)


def _ingest(eng, D, f0=0, f1=FC.F, keep=None):
    """Frames f0 .. f1 - 1 in one call; keep: only the first `keep` sampled pixels of the last frame."""
    import torch
    import bsc_nav_amd as B
    depth, rgb, tokens, poses, idx, off = FC.frames(D)
    chain = B.PoseChain()
    Ts = np.stack([chain.pc_transform(p) for p in poses])
    o = (off[f0:f1 + 1] - off[f0]).copy()
    if keep is not None:
        o[-1] = o[-2] + keep
    sl = slice(int(off[f0]), int(off[f0] + o[-1]))
    eng.ingest(torch.from_numpy(depth[f0:f1]).cuda(), torch.from_numpy(rgb[f0:f1]).cuda(), torch.from_numpy(tokens[f0:f1]).cuda(),
               Ts[f0:f1], sample_idx=torch.from_numpy(idx[sl]).cuda(), offsets=o)


def rows(D):
    """Engine A: a cache that never fills; its export is the list of passing rows in order (feat, pos, dis), and the number
    of rows after each pair of frames.  Also the cut of the last frame's samples after which exactly 4 (P // 4) rows have
    passed: with a cache of P // 4 - 1 rows the last passing point of that call is the one that meets the full cache."""
    if D not in _rows:
        eng = _engine(D, 1 << 14)
        cum = []
        for f0 in range(0, FC.F, 2):
            _ingest(eng, D, f0, f0 + 2)
            cum.append(eng.counters()["iter_id"])
        assert eng.counters()["flushes"] == 0
        cache = eng.export_cache()
        P = cum[-1]
        target, lo, hi = 4 * (P // 4), 0, FC.PER_FRAME
        while lo < hi:                           # the passing count grows by at most one per sampled pixel
            mid = (lo + hi) // 2
            eng.reset()
            _ingest(eng, D, keep=mid)
            lo, hi = (lo, mid) if eng.counters()["iter_id"] >= target else (mid + 1, hi)
        eng.reset()
        _ingest(eng, D, keep=lo)
        assert eng.counters()["iter_id"] == target
        _rows[D] = cache, cum, lo
        eng.close()
    return _rows[D]


def sizes(D):
    P = len(rows(D)[0][1])
    return {"cross": P // 4 - 2, "exact": P // 4 - 1}


def expected(D, radius, kind):
    key = (D, radius, kind)
    if key not in _exp:
        n = sizes(D)[kind]
        feat, pos, dis = rows(D)[0]
        P = 4 * (len(pos) // 4) if kind == "exact" else len(pos)
        st = {}
        m, rem, counts, margins = FC.replay_stream(st, (feat[:P], pos[:P], dis[:P]), n, radius)
        _exp[key] = n, m, rem, counts, margins, R.store_to_arrays(st, D)
    return _exp[key]


@pytest.mark.parametrize("kind", ["cross", "exact"])
@pytest.mark.parametrize("radius", [0, 1])
@pytest.mark.parametrize("D", DIMS)
def test_automatic_surprise_flush_matches_replay(D, radius, kind):
    n, m, rem, counts, margins, store = expected(D, radius, kind)
    (feat, pos, dis), _, keep = rows(D)
    P = 4 * (len(pos) // 4) if kind == "exact" else len(pos)
    feat, pos, dis = feat[:P], pos[:P], dis[:P]
    assert m >= 3 and (rem == 0) == (kind == "exact")
    assert min(margins.values()) >= 1e-4, margins
    eng = _engine(D, n)
    eng.set_flush_policy("surprise", radius, FC.STHR, FC.BTHR)
    _ingest(eng, D, keep=keep if kind == "exact" else None)
    c = eng.counters()
    assert c["flushes"] == m and c["iter_id"] == rem
    cf, cp, cd = eng.export_cache()
    assert np.array_equal(cf, feat[P - rem:]) and np.array_equal(cp, pos[P - rem:]) and np.array_equal(cd, dis[P - rem:])
    assert_store_matches(eng.export_store(), *store, f"D{D} r{radius} {kind}")
    u = eng.store_usage()
    assert u["live_rows"] == int(store[1].sum()) and u["live_rows"] <= u["pool_rows"] <= u["capacity"]
    eng.close()


def test_every_replay_path_is_taken():
    tot = dict.fromkeys(R.PATHS, 0)
    for D in DIMS:
        for radius in (0, 1):
            for kind in ("cross", "exact"):
                counts = expected(D, radius, kind)[3]
                tot = {p: tot[p] + counts[p] for p in tot}
    for p in ("create", "append", "replace", "reject", "merge"):
        assert tot[p] > 0, tot


def test_policy_round_trip():
    """dist -> surprise -> dist across three ingest calls on one engine; the middle call has no draw callback."""
    D = 8
    (feat, pos, dis), cum, _ = rows(D)
    n = sizes(D)["cross"] // 2
    eng = _engine(D, n)
    policy = ["dist", "surprise", "dist"]
    for j, f0 in enumerate(range(0, FC.F, 2)):
        eng.set_flush_policy(policy[j], 1, FC.STHR, FC.BTHR)
        random.seed(40 + j)
        _ingest(eng, D, f0, f0 + 2)
    st, k, worst = {}, 0, np.inf
    for j in range(3):
        random.seed(40 + j)
        while k * (n + 1) + n < cum[j]:          # flush k is triggered by row k (n + 1) + n, inside call j
            a = k * (n + 1)
            if policy[j] == "dist":
                _dist_replay(st, pos[a:a + n], feat[a:a + n], dis[a:a + n], FC.CS)
            else:
                _, g = R.replay(st, pos[a:a + n], feat[a:a + n], dis[a:a + n], 1, FC.STHR, FC.BTHR, FC.CS)
                worst = min(worst, min(g.values()))
            k += 1
    assert k >= 3 and worst >= 1e-4
    per_call = [sum(1 for i in range(k) if (cum[j - 1] if j else 0) <= i * (n + 1) + n < cum[j]) for j in range(3)]
    assert all(per_call), f"a call without a flush: {per_call}"
    assert eng.counters()["flushes"] == k
    assert_store_matches(eng.export_store(), *R.store_to_arrays(st, D), "dist-surprise-dist")
    cf, cp, cd = eng.export_cache()
    assert np.array_equal(cp, pos[k * (n + 1):]) and np.array_equal(cf, feat[k * (n + 1):])
    eng.close()


def test_errors_keep_the_previous_policy():
    import bsc_nav_amd as B
    D = 8
    dense = _engine(D, 100, mode="mean")
    with pytest.raises(B._lib.BscError, match="status -4"):
        dense.set_flush_policy("surprise")
    with pytest.raises(B._lib.BscError, match="status -4"):
        dense.set_flush_policy("dist")
    dense.close()
    n, m, rem, _, _, store = expected(D, 0, "cross")
    eng = _engine(D, n)
    eng.set_flush_policy("surprise", 0, FC.STHR, FC.BTHR)
    for args in [(-1, 0.5, 0.95), (4, 0.5, 0.95), (1, math.nan, 0.95), (1, 0.5, math.nan)]:
        with pytest.raises(B._lib.BscError, match="status -1"):
            eng.set_flush_policy("surprise", *args)
    with pytest.raises(B._lib.BscError, match="status -1"):
        B._lib.check(eng.lib.bsc_set_flush_policy(eng.h, 2, 1, 0.5, 0.95))        # unknown policy
    with pytest.raises(ValueError):
        eng.set_flush_policy("random")
    eng.reset()                                                                      # configuration: reset keeps it
    assert eng._flush_policy == "surprise"
    _ingest(eng, D)
    assert eng.counters()["flushes"] == m
    assert_store_matches(eng.export_store(), *store, "after refused calls and a reset")
    eng.close()
    # the LDS bound of bsc_flush_surprise: cache_size 17 at 1024-D holds radius 1, not radius 3
    big = B.VoxelEngine(FC.H, FC.W, 32, FC.CELL, -0.4, 0.4, FC.G, 1024, mode="exact", iter_size=64, cache_size=17)
    with pytest.raises(B._lib.BscError, match="status -1"):
        big.set_flush_policy("surprise", 3, 0.5, 0.95)
    big.set_flush_policy("surprise", 1, 0.5, 0.95)
    big.close()


def test_dropin_attribute(tmp_path):
    """VoxelTokenMemory.flush_policy = "surprise" through ingest_frames == the engine-level run; surprise_threshold changed
    between two calls takes effect in the second."""
    import torch
    import bsc_nav_amd as B
    from bsc_nav_amd.geometry import sample_indices
    D, rate = 8, 6
    depth, rgb, tokens, poses, _, _ = FC.frames(D)
    n = 300
    args = B.MemoryArgs(width=FC.W, height=FC.H, grid_size=FC.GS, cell_size=FC.CELL, floor_height=FC.FLOOR, map_height=FC.TOP,
                        depth_sample_rate=rate, query_width=FC.G * 14, query_height=FC.G * 14, memory_path=str(tmp_path),
                        scene_name="scene", token_dim=D, iter_size=n, cache_size=FC.CS)
    assert B.VoxelTokenMemory(args, need_diffusion=False).flush_policy == "dist"
    args.flush_policy = "surprise"
    mem = B.VoxelTokenMemory(args, need_diffusion=False, alpha_source="device", max_frames_per_call=3)
    assert mem.flush_policy == "surprise"
    eng = B.VoxelEngine(FC.H, FC.W, FC.GS, FC.CELL, FC.FLOOR, FC.TOP, FC.G, D, mode="exact", iter_size=n, cache_size=FC.CS,
                        max_points=3 * FC.H * FC.W, min_h=mem.minh, max_h=mem.maxh)
    pose_chain = lambda: B.PoseChain(args.base_forward_axis, args.base_left_axis, args.base_up_axis, args.base2cam_rot,
                                     args.sensor_height)
    chain = pose_chain()
    dev = lambda a: torch.from_numpy(a).cuda()
    flushes = []
    for call, (f0, sthr) in enumerate([(0, 0.5), (3, math.inf)]):
        mem.surprise_threshold = sthr
        np.random.seed(70 + call)
        mem.ingest_frames(dev(rgb[f0:f0 + 3]), dev(depth[f0:f0 + 3]), poses[f0:f0 + 3], tokens=dev(tokens[f0:f0 + 3]))
        np.random.seed(70 + call)
        idxs = [sample_indices(FC.H * FC.W, rate) for _ in range(3)]
        off = np.concatenate([[0], np.cumsum([len(i) for i in idxs])]).astype(np.int64)
        Ts = np.stack([chain.pc_transform(p) for p in poses[f0:f0 + 3]])
        eng.set_flush_policy("surprise", 1, sthr, 0.95)
        eng.ingest(dev(depth[f0:f0 + 3]), dev(rgb[f0:f0 + 3]), dev(tokens[f0:f0 + 3]), Ts, dev(np.concatenate(idxs)), off)
        flushes.append(eng.counters()["flushes"])
        assert mem.engine.counters()["flushes"] == flushes[-1]
        a, b = mem.engine.export_store(), eng.export_store()
        assert all(np.array_equal(x, y) for x, y in zip(a, b)), f"call {call}"
    assert flushes[0] >= 1 and flushes[1] > flushes[0]
    # +inf only creates groups: a second call under 0.5 would have stored more tokens
    ref = B.VoxelEngine(FC.H, FC.W, FC.GS, FC.CELL, FC.FLOOR, FC.TOP, FC.G, D, mode="exact", iter_size=n, cache_size=FC.CS,
                        max_points=3 * FC.H * FC.W, min_h=mem.minh, max_h=mem.maxh)
    chain2 = pose_chain()
    ref.set_flush_policy("surprise", 1, 0.5, 0.95)
    for call, f0 in enumerate((0, 3)):
        np.random.seed(70 + call)
        idxs = [sample_indices(FC.H * FC.W, rate) for _ in range(3)]
        off = np.concatenate([[0], np.cumsum([len(i) for i in idxs])]).astype(np.int64)
        Ts = np.stack([chain2.pc_transform(p) for p in poses[f0:f0 + 3]])
        ref.ingest(dev(depth[f0:f0 + 3]), dev(rgb[f0:f0 + 3]), dev(tokens[f0:f0 + 3]), Ts, dev(np.concatenate(idxs)), off)
    assert ref.counters()["store_tokens"] > eng.counters()["store_tokens"]
    for e in (eng, ref, mem.engine):
        e.close()
