"""bsc_score_map / VoxelEngine.score_map / VoxelTokenMemory.voxel_score_map: for every query the best score per top-down cell
(r, c) and the height of the voxel that has it — the field that bsc_localize_regions ranks from and keeps only K of.  Its scores
must be the ranking's own, bit for bit: both calls share the scan (localize.hip region_scan)."""
import random

import numpy as np
import pytest

import golden_util as gu

pytestmark = pytest.mark.gpu
KFULL = 4096                       # the largest K of bsc_localize_regions: a complete ranking of the maps below
NEG_INF = np.float32(-np.inf)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device (no CPU fallback exists)")
    return torch


# ---- helpers -----------------------------------------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _cells_from_ranking(pos, sim, gs):
    """The rule of the map applied to a complete ranking (pos (n,3), sim (n,)): per (r, c) the largest similarity and, among
    the entries that have it, the smallest h; cells outside the ranking -inf / -1."""
    score, height = np.full((gs, gs), NEG_INF, np.float32), np.full((gs, gs), -1, np.int32)
    pos, sim = np.asarray(pos, np.int64).reshape(-1, 3), np.asarray(sim, np.float32).reshape(-1)
    if len(pos):
        cell = pos[:, 0] * gs + pos[:, 1]
        order = np.lexsort((pos[:, 2], -sim.astype(np.float64), cell))        # cell, then best similarity, then lowest h
        first = order[np.r_[True, cell[order][1:] != cell[order][:-1]]]
        score.reshape(-1)[cell[first]] = sim[first]
        height.reshape(-1)[cell[first]] = pos[first, 2]
    return score, height


def _assert_map_is_ranking(score, height, pos, sim, cnt, gs, what):
    """score / height (Q,gs,gs) device tensors against the complete rankings of localize_regions (pos, sim, cnt)."""
    score, height = score.cpu().numpy(), height.cpu().numpy()
    assert score.dtype == np.float32 and height.dtype == np.int32 and score.shape == height.shape == (len(cnt), gs, gs)
    for i in range(len(cnt)):
        n = int(cnt[i])
        assert n < KFULL, "the ranking is not complete"
        rs, rh = _cells_from_ranking(pos[i, :n], sim[i, :n], gs)
        assert np.array_equal(_bits(score[i]), _bits(rs)), (what, i, "score bits")
        assert np.array_equal(height[i], rh), (what, i, "height")


def _ragged_store(V, D, gs, seed):
    """NumPy alone: V distinct voxels in gs^3, 1..10 tokens each, rows grouped by voxel."""
    rng = np.random.RandomState(seed)
    codes = rng.permutation(gs ** 3)[:V]
    keys = np.stack([codes // (gs * gs), (codes // gs) % gs, codes % gs], 1).astype(np.int32)
    cnt = rng.randint(1, 11, size=V).astype(np.int32)
    rows = rng.standard_normal((int(cnt.sum()), D)).astype(np.float32)
    return rng, keys, cnt, rows


def _engine(torch, mode, keys, cnt, rows, gs, D):
    """The map built by import: an exact store with its ragged rows, or a dense `mean` map holding each voxel's first row."""
    import bsc_nav_amd as B
    V = len(keys)
    if mode == "exact":
        eng = B.VoxelEngine(48, 64, gs, 0.1, -3.2, 3.2, 16, D, mode="exact", iter_size=256, voxel_capacity=V + 8,
                            token_capacity=len(rows) + 4096, max_points=4096)
        eng.import_rgb(keys, np.zeros((V, 3), np.uint8), np.ones(V, np.float32))
        eng.import_store(keys, cnt, rows, np.zeros(len(rows), np.float32))
        return eng, cnt, rows
    first = np.r_[0, np.cumsum(cnt)[:-1]]
    eng = B.VoxelEngine(48, 64, gs, 0.1, -3.2, 3.2, 16, D, mode=mode, voxel_capacity=V + 8, max_points=4096)
    eng.dense_replace(torch.from_numpy(keys).cuda(), torch.from_numpy(rows[first]).cuda(),
                      torch.ones(V, dtype=torch.int32, device="cuda"))
    return eng, np.ones(V, np.int32), np.ascontiguousarray(rows[first])


def _mixed_regions(rng, Q, gs, keys, open_kind=True, start=0):
    """Regions per query, cycling through: none (or, when a batch must not hold an open query, a sphere around everything), a
    small sphere, a floor band, sphere plus band, a region that sees nothing."""
    radius, curr, floor = [], [], []
    for i in range(Q):
        kind = (i + start) % 5
        c = keys[rng.randint(len(keys))].tolist()
        if kind == 0:
            r, f = (None, None) if open_kind else (4.0 * gs, None)
        elif kind == 1:
            r, f = 5.5, None
        elif kind == 2:
            r, f = None, (gs // 4, gs // 2)
        elif kind == 3:
            r, f = 9.0, (gs // 3, gs // 3 + 4)
        else:
            r, f, c = 1.0, None, [-50, -50, -50]
        radius.append(r); curr.append(c); floor.append(f)
    return radius, curr, floor


SMALL = dict(V=3000, D=64, gs=32, seed=21)


@pytest.fixture(scope="module")
def small_maps(torch_cuda):
    """V = 3000 voxels in 32^3: about three voxels share every column.  One exact and one dense map for the whole module."""
    rng, keys, cnt, rows = _ragged_store(**SMALL)
    out = {"keys": keys}
    for mode in ("exact", "mean"):
        out[mode] = _engine(torch_cuda, mode, keys, cnt, rows, SMALL["gs"], SMALL["D"])[0]
    yield out
    for mode in ("exact", "mean"):
        out[mode].close()


# ---- 1. bit-exact against the complete ranking --------------------------------------------------------------------------
@pytest.mark.parametrize("knob", [None, "never", "always"])
@pytest.mark.parametrize("Q", [1, 8, 70, 300])
@pytest.mark.parametrize("mode", ["exact", "mean"])
def test_map_equals_the_complete_ranking_bit_for_bit(torch_cuda, small_maps, monkeypatch, mode, Q, knob):
    """Q = 1 / 8 on the vector ALUs, 70 on the f32 MFMA plus a piece launch, 300 on the piece scan.  Batch A holds queries
    without any region (no visibility pass), batch B none (pass, mask, and under `always` the gathered rows), batch C only
    regions that see nothing.  Each map against a localize_regions call made under the same BSC_REGION_PRUNE."""
    torch = torch_cuda
    eng, keys, gs, D = small_maps[mode], small_maps["keys"], SMALL["gs"], SMALL["D"]
    if knob is None:
        monkeypatch.delenv("BSC_REGION_PRUNE", raising=False)
    else:
        monkeypatch.setenv("BSC_REGION_PRUNE", knob)
    rng = np.random.RandomState(1000 + Q)
    q = torch.from_numpy(rng.standard_normal((Q, D)).astype(np.float32)).cuda()
    for batch, (open_kind, start) in (("A", (True, 0)), ("B", (False, 1 if Q == 1 else 0)), ("C", (True, 4))):
        radius, curr, floor = _mixed_regions(rng, Q, gs, keys, open_kind, start)
        if batch == "C":
            radius, curr, floor = [1.0] * Q, [[-50, -50, -50]] * Q, [None] * Q
        pos, sim, cnt = eng.localize_regions(q, K=KFULL, radius=radius, curr=curr, floor=floor)
        score, height = eng.score_map(q, radius=radius, curr=curr, floor=floor)
        assert score.is_cuda and height.is_cuda
        if batch == "C":
            assert not cnt.any()
        else:
            assert cnt.max() > gs * gs // 2 or Q == 1
        _assert_map_is_ranking(score, height, pos, sim, cnt, gs, (mode, Q, knob, batch))
    # no region argument at all: the NULL pointer, against the ranking without regions
    pos, sim, cnt = eng.localize_regions(q[:min(Q, 8)], K=KFULL)
    score, height = eng.score_map(q[:min(Q, 8)])
    assert cnt.min() == len(keys)
    _assert_map_is_ranking(score, height, pos, sim, cnt, gs, (mode, Q, knob, "NULL"))


# ---- 2. against an independent fp64 scan --------------------------------------------------------------------------------
MEDIUM = dict(V=1 << 14, D=64, gs=64, seed=33)
GAP = 4e-6


def _fp64_columns(keys, cnt, rows, q, radius, curr, floor, gs):
    """NumPy alone, float64: per query the column maximum of the voxels' best cosines, the h of the voxel that has it and the
    gap to the column's second-best voxel (inf with one voxel) -> (score (Q,gs,gs), height, gap), empty cells -inf / -1 / inf."""
    r64, q64 = rows.astype(np.float64), q.astype(np.float64)
    rn = r64 / np.maximum(np.linalg.norm(r64, axis=1, keepdims=True), 1e-8)
    qn = q64 / np.maximum(np.linalg.norm(q64, axis=1, keepdims=True), 1e-8)
    sims = qn @ rn.T
    best = np.maximum.reduceat(sims, np.r_[0, np.cumsum(cnt)[:-1]], axis=1)                 # (Q,V)
    k64 = keys.astype(np.int64)
    cell = k64[:, 0] * gs + k64[:, 1]
    Q = len(q)
    score, height = np.full((Q, gs * gs), -np.inf), np.full((Q, gs * gs), -1, np.int64)
    gap = np.full((Q, gs * gs), np.inf)
    for i in range(Q):
        seen = np.ones(len(keys), bool)
        if radius[i] is not None:
            seen &= ((k64 - np.asarray(curr[i], np.int64)) ** 2).sum(1).astype(np.float64) <= float(radius[i]) ** 2
        if floor[i] is not None:
            seen &= (k64[:, 2] >= floor[i][0]) & (k64[:, 2] <= floor[i][1])
        idx = np.nonzero(seen)[0]
        if not len(idx):
            continue
        order = idx[np.lexsort((-best[i, idx], cell[idx]))]                                  # cell, then best first
        c = cell[order]
        head = np.r_[True, c[1:] != c[:-1]]
        first = order[head]
        score[i, cell[first]], height[i, cell[first]] = best[i, first], k64[first, 2]
        second = np.nonzero(~head & np.r_[False, head[:-1]])[0]                              # the entry right behind a head
        gap[i, c[second]] = best[i, order[second - 1]] - best[i, order[second]]
    shape = (Q, gs, gs)
    return score.reshape(shape), height.reshape(shape), gap.reshape(shape)


@pytest.mark.parametrize("mode", ["exact", "mean"])
def test_map_matches_an_independent_fp64_scan(torch_cuda, mode):
    """Scores within 2e-6 (the bar of the localize tests) where finite, the same empty cells, and the height wherever the fp64
    gap between the column's best two voxels exceeds 4e-6 — which the builder first confirms, on the CPU, to leave out at most
    1 % of the non-empty cells."""
    torch = torch_cuda
    V, D, gs = MEDIUM["V"], MEDIUM["D"], MEDIUM["gs"]
    rng, keys, cnt, rows = _ragged_store(**MEDIUM)
    Q = 8
    q = rng.standard_normal((Q, D)).astype(np.float32)
    radius = [None, 14.0, None, 20.0, 1.0, None, 30.0, 8.5]
    curr = [[0, 0, 0], [30, 31, 32], [0, 0, 0], [20, 40, 30], [-50, -50, -50], [0, 0, 0], [32, 32, 32], [50, 12, 40]]
    floor = [None, None, (16, 40), (25, 35), None, (0, 63), None, None]
    if mode != "exact":
        first = np.r_[0, np.cumsum(cnt)[:-1]]
        cnt_ref, rows_ref = np.ones(V, np.int32), rows[first]
    else:
        cnt_ref, rows_ref = cnt, rows
    ref_s, ref_h, gap = _fp64_columns(keys, cnt_ref, rows_ref, q, radius, curr, floor, gs)
    filled = np.isfinite(ref_s)
    clear = filled & (gap > GAP)
    skipped = int(filled.sum() - clear.sum())
    print(f"{mode}: {int(filled.sum())} non-empty cells, {skipped} with a best-two gap <= {GAP}")
    assert filled[0].sum() > gs * gs // 2 and not filled[4].any() and 0 < filled[1].sum() < filled[0].sum()
    assert skipped <= 0.01 * filled.sum(), "the seed leaves too many columns undecided"      # before any GPU work
    eng = _engine(torch, mode, keys, cnt, rows, gs, D)[0]
    score, height = eng.score_map(torch.from_numpy(q).cuda(), radius=radius, curr=curr, floor=floor)
    score, height = score.cpu().numpy(), height.cpu().numpy()
    eng.close()
    assert np.array_equal(np.isfinite(score), filled), "pattern of empty cells"
    assert np.all(score[~filled] == NEG_INF) and np.all(height[~filled] == -1)
    err = np.abs(score[filled].astype(np.float64) - ref_s[filled])
    print(f"{mode}: largest score error {err.max():.3e}")
    assert err.max() <= 2e-6
    assert np.array_equal(height[clear], ref_h[clear])


# ---- 3. planted exact ties ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["exact", "mean"])
def test_equal_scores_give_the_smallest_height(torch_cuda, mode):
    torch = torch_cuda
    D, gs = 64, 32
    rng = np.random.RandomState(8)
    t = rng.standard_normal(D).astype(np.float32)
    # ids 0, 1, 2: one column at h = 9, 2, 5 in that order; id 3: another column; then voxels that do not interfere
    keys = np.array([[5, 7, 9], [5, 7, 2], [5, 7, 5], [10, 3, 4], [5, 7, 1], [5, 7, 30], [10, 3, 0], [20, 20, 20]], np.int32)
    rows = np.stack([t, t, t, t] + [rng.standard_normal(D).astype(np.float32) for _ in range(4)])
    eng = _engine(torch, mode, keys, np.ones(len(keys), np.int32), rows, gs, D)[0]
    score, height = eng.score_map(torch.from_numpy(t).cuda())
    score, height = score.cpu().numpy()[0], height.cpu().numpy()[0]
    pos, sim, cnt = eng.localize_regions(torch.from_numpy(t).cuda().reshape(1, -1), K=16)
    eng.close()
    assert height[5, 7] == 2 and height[10, 3] == 4 and height[20, 20] == 20
    assert _bits(score[5, 7]) == _bits(score[10, 3]) == _bits(sim[0, 0]) and abs(float(score[5, 7]) - 1.0) < 2e-6
    assert np.isfinite(score).sum() == 3 and (height >= 0).sum() == 3


# ---- 4. the grid_0_0_0 group --------------------------------------------------------------------------------------------
def _golden_engine(torch, z):
    """The HIP engine driven like obs2voxeltoken drives the reference, frame by frame, on an ingest fixture."""
    import bsc_nav_amd as B
    from oracle import oracle as orc
    cfg, rgb, depth, poses, tokens = gu.ingest_inputs(z)
    N = cfg["H"] * cfg["W"]
    P_max = sum(len(range(0, N, cfg["s"])) for _ in range(cfg["F"]))
    eng = B.VoxelEngine(cfg["H"], cfg["W"], cfg["gs"], cfg["cs"], cfg["floor_height"], cfg["map_height"], cfg["g"], cfg["D"],
                        mode="exact", iter_size=cfg.get("iter_size", 50000), max_points=max(P_max, N))
    oc = orc.make_config(cfg["H"], cfg["W"], cfg["gs"], cfg["cs"], cfg["floor_height"], cfg["map_height"], cfg["g"], cfg["D"])
    chain = B.PoseChain()
    np.random.seed(cfg["seed"])
    random.seed(cfg["seed"])
    d_depth, d_rgb, d_tok = torch.from_numpy(depth).cuda(), torch.from_numpy(rgb).cuda(), torch.from_numpy(tokens).cuda()
    for f in range(cfg["F"]):
        T = chain.pc_transform(poses[f])
        idx = B.sample_indices(N, cfg["s"])
        g = orc.geometry(oc, depth[f], idx, T)
        alpha = np.array([np.exp(-r / (2 * 0.6)) for r in g["r2"]], dtype=np.float64)          # memory_2.py:873-875
        eng.ingest(d_depth[f:f + 1], d_rgb[f:f + 1], d_tok[f:f + 1], T[None], torch.from_numpy(idx).cuda(),
                   np.array([0, len(idx)]), torch.from_numpy(alpha).cuda())
    return cfg, eng


def test_zero_group_counts_at_cell_0_0(torch_cuda):
    """The flush of this fixture leaves the grid_0_0_0 group of zero rows behind; bsc_localize reports it at (0, 0, 0), and so
    does the map.  The fixture holds more voxels than the largest K, so the complete ranking is that of a sphere around
    (0, 0, 0) which holds the whole column (0, 0): the map of that sphere follows from it cell by cell, and so does cell (0, 0)
    of the map without any region."""
    torch = torch_cuda
    z = gu.load("g3_flush_small_cache")
    cfg, eng = _golden_engine(torch, z)
    eng.flush()
    gs = cfg["gs"]
    specs = list(gu.query_specs(z))
    q = torch.from_numpy(np.stack([s["pooled"].reshape(-1) for s in specs[:2]])).cuda()
    R = float(eng.export_rgb()[0][:, 2].max()) + 1.0
    pos, sim, cnt = eng.localize(q, K=KFULL, radius=R, curr=[0, 0, 0])
    score, height = eng.score_map(q, radius=R, curr=[0, 0, 0])
    s_all, h_all = eng.score_map(q)
    for i in range(len(q)):
        zero = np.nonzero((pos[i, :cnt[i]] == 0).all(1))[0]
        assert len(zero) == 1, "the fixture no longer holds the grid_0_0_0 group"
        rs, rh = _cells_from_ranking(pos[i, :cnt[i]], sim[i, :cnt[i]], gs)
        assert np.isfinite(rs[0, 0]) and rs[0, 0] >= sim[i, zero[0]]
        for sm, hm in ((score, height), (s_all, h_all)):
            assert _bits(sm[i, 0, 0].cpu().numpy()) == _bits(rs[0, 0]) and int(hm[i, 0, 0]) == rh[0, 0]
    _assert_map_is_ranking(score, height, pos, sim, cnt, gs, "g3_flush_small_cache")
    eng.close()


# ---- 5. chunking --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["exact", "mean"])
def test_one_query_per_chunk_equals_one_chunk(torch_cuda, small_maps, monkeypatch, mode):
    torch = torch_cuda
    eng, keys, gs, D = small_maps[mode], small_maps["keys"], SMALL["gs"], SMALL["D"]
    rng = np.random.RandomState(77)
    q = torch.from_numpy(rng.standard_normal((5, D)).astype(np.float32)).cuda()
    radius, curr, floor = _mixed_regions(rng, 5, gs, keys)
    monkeypatch.delenv("BSC_SCORE_MAP_CHUNK_MB", raising=False)
    s0, h0 = eng.score_map(q, radius=radius, curr=curr, floor=floor)
    one_query_mb = gs * gs * 8 / 2 ** 20                           # the packed keys of one query
    monkeypatch.setenv("BSC_SCORE_MAP_CHUNK_MB", repr(one_query_mb * 1.5))
    s1, h1 = eng.score_map(q, radius=radius, curr=curr, floor=floor)
    monkeypatch.setenv("BSC_SCORE_MAP_CHUNK_MB", repr(one_query_mb * 2.5))       # chunks of 2, 2, 1
    s2, h2 = eng.score_map(q, radius=radius, curr=curr, floor=floor)
    assert np.isfinite(s0.cpu().numpy()).any(axis=(1, 2)).tolist() == [True, True, True, True, False]
    for s, h in ((s1, h1), (s2, h2)):
        assert np.array_equal(_bits(s.cpu().numpy()), _bits(s0.cpu().numpy())) and torch.equal(h, h0)


# ---- 6. resident results ------------------------------------------------------------------------------------------------
def test_resident_localize_results_survive_a_map_call(torch_cuda, small_maps):
    torch = torch_cuda
    eng, keys, gs, D = small_maps["exact"], small_maps["keys"], SMALL["gs"], SMALL["D"]
    rng = np.random.RandomState(5)
    q = torch.from_numpy(rng.standard_normal((4, D)).astype(np.float32)).cuda()
    radius, curr = [None, 9.0, 12.0, 7.0], [[0, 0, 0], [10, 10, 10], [20, 15, 17], [5, 25, 15]]
    p, s, n = eng.localize_regions(q, K=100, radius=radius, curr=curr)
    before = eng.cluster_centers_batch(eps=4.0, min_samples=3)
    q2 = torch.from_numpy(rng.standard_normal((7, D)).astype(np.float32)).cuda()
    eng.score_map(q2, radius=6.0, curr=[16, 16, 16])
    eng.score_map(q2)
    after = eng.cluster_centers_batch(eps=4.0, min_samples=3)
    host = eng.cluster_centers_batch([p[i, :n[i]] for i in range(4)], [s[i, :n[i]] for i in range(4)], eps=4.0, min_samples=3)
    assert any(len(c[0]) for c in before)
    for b, a, h in zip(before, after, host):
        assert np.array_equal(b[0], a[0]) and np.array_equal(b[1], a[1]) and b[2] == a[2]
        assert np.array_equal(a[0], h[0]) and np.array_equal(a[1], h[1]) and a[2] == h[2]


# ---- 7. refusals --------------------------------------------------------------------------------------------------------
def test_invalid_arguments_are_refused_and_nothing_is_written(torch_cuda, small_maps):
    torch = torch_cuda
    from bsc_nav_amd.engine import _dp, _hp, region_array
    eng, gs, D = small_maps["mean"], SMALL["gs"], SMALL["D"]
    q = torch.randn((1025, D), device="cuda")
    score = torch.full((4, gs, gs), 123.25, dtype=torch.float32, device="cuda")
    height = torch.full((4, gs, gs), 77, dtype=torch.int32, device="cuda")
    good = region_array(4, radius=[5.0, None, 8.0, 3.0], curr=[10, 10, 10])
    nan = good.copy(); nan["radius"][2] = np.nan
    res = good.copy(); res["reserved"][3] = 1
    call = eng.lib.bsc_score_map
    INVALID = -1
    assert call(eng.h, _dp(q), 4, _hp(good), None, _dp(height)) == INVALID
    assert call(None, _dp(q), 4, _hp(good), _dp(score), _dp(height)) == INVALID
    assert call(eng.h, None, 4, _hp(good), _dp(score), _dp(height)) == INVALID
    assert call(eng.h, _dp(q), 0, _hp(good), _dp(score), _dp(height)) == INVALID
    assert call(eng.h, _dp(q), 1025, None, _dp(score), _dp(height)) == INVALID
    assert call(eng.h, _dp(q), 4, _hp(nan), _dp(score), _dp(height)) == INVALID
    assert call(eng.h, _dp(q), 4, _hp(res), _dp(score), _dp(height)) == INVALID
    torch.cuda.synchronize()
    assert bool((score == 123.25).all()) and bool((height == 77).all())
    assert call(eng.h, _dp(q), 4, _hp(good), _dp(score), None) == 0               # heights are optional
    torch.cuda.synchronize()
    assert bool((height == 77).all()) and not bool((score == 123.25).any())
    s2, h2 = eng.score_map(q[:4], radius=[5.0, None, 8.0, 3.0], curr=[10, 10, 10])
    assert np.array_equal(_bits(s2.cpu().numpy()), _bits(score.cpu().numpy()))
    assert eng.score_map(q[:4], heights=False)[1] is None


# ---- 8. empty memory ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["exact", "mean", "max"])
def test_empty_memory_gives_an_empty_map(torch_cuda, mode):
    torch = torch_cuda
    import bsc_nav_amd as B
    gs, D = 48, 32
    eng = B.VoxelEngine(48, 64, gs, 0.1, -3.2, 3.2, 16, D, mode=mode, iter_size=256, max_points=4096)
    q = torch.randn((3, D), device="cuda")
    for kw in ({}, dict(radius=5.0, curr=[1, 2, 3]), dict(floor=(0, 10))):
        score, height = eng.score_map(q, **kw)
        assert score.shape == (3, gs, gs) and bool((score == float("-inf")).all()) and bool((height == -1).all())
    eng.close()


# ---- 9. the drop-in class -----------------------------------------------------------------------------------------------
class _FakeDino:
    def __init__(self, tokens):
        self.tokens, self.frame = tokens, 0

    def forward_features(self, x):
        import torch
        t = torch.from_numpy(self.tokens[self.frame]).cuda()
        return {"x_norm_patchtokens": t.reshape(1, -1, t.shape[-1])}


def test_voxel_score_map_follows_voxel_localized_batch(torch_cuda, tmp_path):
    torch = torch_cuda
    import bsc_nav_amd as B
    z = gu.load("g2_mini_s7_yaw")
    cfg, rgb, depth, poses, tokens = gu.ingest_inputs(z)
    args = B.MemoryArgs(width=cfg["W"], height=cfg["H"], grid_size=cfg["gs"], cell_size=cfg["cs"],
                        floor_height=cfg["floor_height"], map_height=cfg["map_height"], depth_sample_rate=cfg["s"],
                        query_width=cfg["g"] * 14, query_height=cfg["g"] * 14, memory_path=str(tmp_path), scene_name="scene",
                        token_dim=cfg["D"], iter_size=cfg.get("iter_size", 50000))
    dino = _FakeDino(tokens)
    mem = B.VoxelTokenMemory(args, preload_dino=dino, need_diffusion=False, alpha_source="host")
    np.random.seed(cfg["seed"])
    random.seed(cfg["seed"])
    for f in range(cfg["F"]):
        dino.frame = f
        mem.obs2voxeltoken({"rgb": rgb[f], "depth": depth[f]}, poses[f])
    mem.update_memory_dist_base()
    gs = cfg["gs"]
    prompts = [torch.from_numpy(s["pooled"].reshape(-1)).cuda() for s in gu.query_specs(z)]
    prompts = (prompts + [prompts[0] + prompts[-1]])[:3]
    assert len(prompts) == 3
    vox = np.asarray(mem.grid_rgb_pos)
    assert len(vox) < KFULL
    centre = vox[len(vox) // 2].tolist()

    def check(out, score, height, what):
        assert score.is_cuda and tuple(score.shape) == (len(out), gs, gs) and score.dtype == torch.float32
        assert height.is_cuda and height.dtype == torch.int32
        for i, (top1, tpos, tsim) in enumerate(out):
            rs, rh = _cells_from_ranking(tpos, tsim.astype(np.float32), gs)
            assert np.array_equal(_bits(score[i].cpu().numpy()), _bits(rs)), (what, i)
            assert np.array_equal(height[i].cpu().numpy(), rh), (what, i)

    radii, currs = [np.inf, 9.0, 14.0], [centre, centre, vox[3].tolist()]
    check(mem.voxel_localized_batch(prompts, K=KFULL, region_radius=radii, curr_grid=currs),
          *mem.voxel_score_map(prompts, region_radius=radii, curr_grid=currs), "regions")
    check(mem.voxel_localized_batch(torch.stack(prompts), K=KFULL), *mem.voxel_score_map(torch.stack(prompts)), "open")
    # the loaded single floor applies exactly when voxel_localized_batch applies it; a list overrides it per query
    lo = int(np.median(vox[:, 2]))
    mem.args.load_single_floor = True
    mem.floor_min_height, mem.floor_max_height = lo, lo + 2
    score, height = mem.voxel_score_map(prompts)
    check(mem.voxel_localized_batch(prompts, K=KFULL), score, height, "single floor")
    h = height.cpu().numpy()
    assert (h >= 0).any() and np.all((h[h >= 0] >= lo) & (h[h >= 0] <= lo + 2))
    floors = [None, (lo, lo + 2), None]
    score, height = mem.voxel_score_map(prompts, floors=floors)
    check(mem.voxel_localized_batch(prompts, K=KFULL, floors=floors), score, height, "floors override")
    h = height.cpu().numpy()
    assert np.any((h[0] >= 0) & ((h[0] < lo) | (h[0] > lo + 2)))
    mem.args.load_single_floor = False
