"""bsc_cluster_centers_batch / VoxelEngine.cluster_centers_batch / VoxelTokenMemory.working_memory_retrieval_batch: the
cluster centres of every query of a localize batch in one call (working_memory_retrival, BSCAgent.py:587-664, and the
three-radius loop, :1078-1098).  The checkers are the committed oracle (pinned to the reference's own outputs in
g5_cluster_centers) and the single-query entry point bsc_cluster_centers — never the batch path itself."""
import ctypes as C
import random

import numpy as np
import pytest

import golden_util as gu
from test_gpu_localize_regions import _FakeDino, _medium_map

pytestmark = pytest.mark.gpu
BSC_E_INVALID = -1
GOLDEN_CASES = ["c1", "c2", "c3", "c4", "c5", "c6", "c7"]
BIT_ROW_MAX = 256            # CL_BITN of cluster.hip: up to here the adjacency is kept as bit rows, above it is recomputed


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device (no CPU fallback exists)")
    return torch


# ---- helpers -----------------------------------------------------------------------------------------------------------
def _tiny_engine():
    import bsc_nav_amd as B
    return B.VoxelEngine(48, 64, 64, 0.1, -3.2, 3.2, 16, 16, mode="mean", voxel_capacity=64, max_points=4096)


def _hp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _raw(eng, Q, K, counts, pos, sim, eps, min_samples, handle="ctx", rows=None, drop=None):
    """bsc_cluster_centers_batch through ctypes with sentinel-filled outputs -> (status, centers, labels, sizes, n_clusters).
    rows: rows of the output arrays (default Q); drop: name of an output passed as NULL."""
    rows = Q if rows is None else rows
    out = dict(centers=np.full((rows, max(K, 1), 3), 7.5, np.float64), labels=np.full((rows, max(K, 1)), 77, np.int32),
               sizes=np.full((rows, max(K, 1)), 77, np.int32), ncl=np.full(rows, 77, np.int32))
    ptr = {k: (None if k == drop else _hp(v)) for k, v in out.items()}
    st = eng.lib.bsc_cluster_centers_batch(eng.h if handle == "ctx" else None, Q, K, _hp(counts), _hp(pos), _hp(sim), float(eps),
                                           int(min_samples), ptr["centers"], ptr["labels"], ptr["sizes"], ptr["ncl"])
    return st, out["centers"], out["labels"], out["sizes"], out["ncl"]


def _untouched(res):
    _, centers, labels, sizes, ncl = res
    return bool(np.all(centers == 7.5) and np.all(labels == 77) and np.all(sizes == 77) and np.all(ncl == 77))


def _assert_rows(res, cnt):
    """The padding the header promises: labels -1 from n_i on, centre / size rows zero from n_clusters_i on."""
    st, centers, labels, sizes, ncl = res
    assert st == 0
    for i, n in enumerate(cnt):
        assert 0 <= ncl[i] <= n
        assert np.all(labels[i, n:] == -1) and np.all(labels[i, :n] >= -1) and np.all(labels[i, :n] < max(ncl[i], 1))
        assert not centers[i, ncl[i]:].any() and not sizes[i, ncl[i]:].any()


def _same(a, b):
    """(centers, labels, sizes) bit for bit."""
    return (a[0].shape == b[0].shape and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
            and list(a[2]) == list(b[2]))


def _assert_oracle(got, pos, sim, eps, min_samples):
    """Bar of test_cluster_centers_match_reference: labels and sizes exact, centres 1e-12 relative (f64 sums, same order)."""
    from oracle import oracle as orc
    c, l, s = orc.cluster_centers(np.ascontiguousarray(pos, np.int32), np.asarray(sim, np.float32).astype(np.float64),
                                  eps=eps, min_samples=min_samples)
    assert np.array_equal(got[1], l) and list(got[2]) == [int(v) for v in s]
    assert got[0].shape == np.asarray(c).shape and got[0].dtype == np.float64
    np.testing.assert_allclose(got[0], c, rtol=1e-12, atol=0)


# ---- 1. the reference's own answers, seven cases in one call ------------------------------------------------------------
def test_goldens_as_one_batch(torch_cuda):
    from bsc_nav_amd.engine import pad_cluster_batch
    z = gu.load("g5_cluster_centers")
    eng = _tiny_engine()
    pos = [z[f"{c}_pos"] for c in GOLDEN_CASES]
    sim = [z[f"{c}_sim"] for c in GOLDEN_CASES]
    assert len({len(p) for p in pos}) > 1, "the golden cases are expected to differ in length"
    out = eng.cluster_centers_batch(pos, sim)
    assert len(out) == len(GOLDEN_CASES)
    for c, (centers, labels, sizes) in zip(GOLDEN_CASES, out):
        assert np.array_equal(labels, z[f"{c}_labels"]) and labels.dtype == np.int64
        assert sizes == [int(v) for v in z[f"{c}_sizes"]]
        assert centers.shape == z[f"{c}_centers"].shape and centers.dtype == np.float64
        np.testing.assert_allclose(centers, z[f"{c}_centers"], rtol=1e-12, atol=0)
    P, S, cnt = pad_cluster_batch(pos, sim)
    res = _raw(eng, len(cnt), P.shape[1], cnt, P, S, 10.0, 5)
    _assert_rows(res, cnt)
    for i, c in enumerate(GOLDEN_CASES):
        assert res[4][i] == len(z[f"{c}_sizes"]) and np.array_equal(res[2][i, :cnt[i]], z[f"{c}_labels"])
    eng.close()


# ---- 2. batch == loop over the single call, bit for bit -----------------------------------------------------------------
SIZES = [0, 1, 4, 5, 37, 100, BIT_ROW_MAX, BIT_ROW_MAX + 1, 1024]
Q_SYN, Q_SAME, Q_NOISE, Q_TIE = 64, 5 + 9, 5 + 18, 5 + 27          # special queries, all of n = 100 (index % 9 == 5)


def _synthetic_clouds(seed):
    """Q_SYN clouds in a 256^3 grid: 1-5 Gaussian blobs (sigma 1.5 .. 5) holding ~80 % of the points, the rest uniform noise;
    sizes cycle through SIZES.  Three special queries of 100 points: all points identical, uniform noise only, and two far
    blobs of 50 points that all carry the similarity 0.5 (their mean similarities tie exactly: stable order)."""
    rs = np.random.RandomState(seed)
    pos, sim = [], []
    for i in range(Q_SYN):
        n = SIZES[i % len(SIZES)]
        nb = rs.randint(1, 6)
        centres = rs.randint(30, 226, size=(nb, 3))
        sigma = rs.uniform(1.5, 5.0, size=nb)
        which = rs.randint(0, nb, size=n)
        p = np.rint(centres[which] + rs.standard_normal((n, 3)) * sigma[which, None])
        noise = rs.rand(n) < 0.2
        p[noise] = rs.randint(0, 256, size=(int(noise.sum()), 3))
        s = rs.uniform(0.1, 0.9, size=n).astype(np.float32)
        if i == Q_SAME:
            p[:] = [17, 200, 93]
        elif i == Q_NOISE:
            p = rs.randint(0, 256, size=(n, 3)).astype(np.float64)
        elif i == Q_TIE:
            p[:50] = np.rint([40, 40, 40] + rs.standard_normal((50, 3)) * 1.2)
            p[50:] = np.rint([200, 200, 200] + rs.standard_normal((50, 3)) * 1.2)
            order = rs.permutation(n)
            p, s = p[order], np.full(n, 0.5, np.float32)
        pos.append(np.clip(p, 0, 255).astype(np.int32).reshape(n, 3))
        sim.append(s)
    assert len(pos[Q_SAME]) == len(pos[Q_NOISE]) == len(pos[Q_TIE]) == 100
    return pos, sim


@pytest.mark.parametrize("min_samples", [1, 5])
@pytest.mark.parametrize("eps", [3.0, 10.0])
def test_batch_equals_loop_of_single_calls(torch_cuda, eps, min_samples):
    from bsc_nav_amd.engine import pad_cluster_batch
    eng = _tiny_engine()
    pos, sim = _synthetic_clouds(1234)
    out = eng.cluster_centers_batch(pos, sim, eps=eps, min_samples=min_samples)
    assert len(out) == Q_SYN
    seen_sizes, multi, noisy = set(), 0, 0
    for i in range(Q_SYN):
        n = len(pos[i])
        seen_sizes.add(n)
        assert len(out[i][1]) == n
        if n == 0:
            assert out[i][0].shape == (0, 3) and out[i][2] == []
            continue
        one = eng.cluster_centers(pos[i], sim[i], eps=eps, min_samples=min_samples)
        assert _same(out[i], one), f"query {i} (n = {n}): the batch differs from bsc_cluster_centers"
        _assert_oracle(out[i], pos[i], sim[i], eps, min_samples)
        multi += len(out[i][2]) >= 2
        noisy += len(out[i][2]) >= 2 and bool(np.any(out[i][1] < 0))
    assert seen_sizes == set(SIZES)
    assert multi >= 20, "the clouds are meant to give several clusters"
    assert out[Q_SAME][2] == [100] and np.all(out[Q_SAME][1] == 0)
    if min_samples == 1:                                           # every point is a core point: no noise anywhere
        assert noisy == 0 and len(out[Q_NOISE][2]) == 100
    else:
        assert noisy >= 20 and len(out[Q_NOISE][2]) == 0 and np.all(out[Q_NOISE][1] == -1)
    # two clusters with the same mean similarity (every point carries 0.5): the one seeded first, label 0, stays first
    c, l, s = out[Q_TIE]
    assert s == [50, 50] and set(l.tolist()) == {0, 1} and l[0] == 0
    assert np.linalg.norm(c[0] - pos[Q_TIE][0]) < 6 < 200 < np.linalg.norm(c[1] - pos[Q_TIE][0])
    P, S, cnt = pad_cluster_batch(pos, sim)
    _assert_rows(_raw(eng, Q_SYN, P.shape[1], cnt, P, S, eps, min_samples), cnt)
    eng.close()


# ---- 3. the resident results of localize_regions ------------------------------------------------------------------------
def _mixed_regions(kk, Q, gs, seed):
    """Region kinds cycling per query: none, radius 30 around a voxel, a floor band, no voxel at all, fewer than K voxels."""
    rs = np.random.RandomState(seed)
    occupied = set(map(tuple, kk.tolist()))
    while True:
        empty_c = rs.randint(0, gs, size=3)
        if tuple(empty_c.tolist()) not in occupied:
            break
    radius, curr, floor, kind = [], [], [], []
    for i in range(Q):
        k = i % 5
        v = kk[rs.randint(len(kk))].tolist()
        radius.append([None, 30.0, None, 0.0, 3.0][k])
        curr.append(empty_c.tolist() if k == 3 else v)
        floor.append((20, 24) if k == 2 else None)
        kind.append(k)
    return radius, curr, floor, kind


def _check_resident(eng, p, s, n, K, eps, min_samples):
    """resident batch == host-form batch of the returned top-K == the single resident call per query -> n_clusters per query."""
    res = eng.cluster_centers_batch(eps=eps, min_samples=min_samples)
    host = eng.cluster_centers_batch(p, s, counts=n, eps=eps, min_samples=min_samples)
    assert len(res) == len(host) == len(n)
    for i in range(len(n)):
        assert len(res[i][1]) == n[i]
        assert _same(res[i], host[i]), f"query {i}: resident and host form differ"
    res2 = eng.cluster_centers_batch(eps=eps, min_samples=min_samples)     # the host-form call left the resident results alone
    for i in range(len(n)):
        assert _same(res[i], res2[i])
        if n[i] >= 1:
            one = eng.cluster_centers(K=int(n[i]), query_index=i, eps=eps, min_samples=min_samples)
            assert _same(res[i], one), f"query {i}: the batch differs from bsc_cluster_centers(query_index)"
        else:
            assert res[i][0].shape == (0, 3) and res[i][2] == []
    return [len(r[2]) for r in res]


@pytest.mark.parametrize("mode", ["exact", "mean"])
def test_resident_results_of_localize_regions(torch_cuda, mode):
    torch = torch_cuda
    eng, keys, kk, rows, seg, gen = _medium_map(torch, mode)
    K, gs = 100, 64
    formed = 0
    for Q in (1, 8, 256):
        q = torch.randn((Q, rows.shape[1]), device="cuda", generator=gen)
        if Q == 1:                                                 # one query: every region kind in a call of its own
            batches = [([r], [c], [f], [k]) for r, c, f, k in zip(*_mixed_regions(kk, 5, gs, 40))]
        else:
            batches = [_mixed_regions(kk, Q, gs, 40 + Q)]
        kinds_seen = set()
        for radius, curr, floor, kind in batches:
            p, s, n = eng.localize_regions(q, K=K, radius=radius, curr=curr, floor=floor)
            for i, k in enumerate(kind):
                kinds_seen.add(k)
                assert (n[i] == 0) if k == 3 else (1 <= n[i] < K) if k == 4 else (n[i] == K), (Q, i, k, n[i])
            _check_resident(eng, p, s, n, K, 10.0, 5)
            formed += sum(c >= 1 for c in _check_resident(eng, p, s, n, K, 20.0, 3))
            if Q == 8:                                             # a shorter K and counts of the caller's own
                short = eng.cluster_centers_batch(K=40, eps=20.0, min_samples=3)
                mine = np.minimum(n, 40) // 2
                half = eng.cluster_centers_batch(K=40, counts=mine, eps=20.0, min_samples=3)
                for i in range(Q):
                    m = min(int(n[i]), 40)
                    assert len(short[i][1]) == m and len(half[i][1]) == mine[i]
                    if m >= 1:
                        assert _same(short[i], eng.cluster_centers(p[i, :m], s[i, :m], eps=20.0, min_samples=3))
                    if mine[i] >= 1:
                        assert _same(half[i], eng.cluster_centers(p[i, :mine[i]], s[i, :mine[i]], eps=20.0, min_samples=3))
        assert kinds_seen == {0, 1, 2, 3, 4}
    assert formed >= 1, "eps = 20 / min_samples = 3 is meant to form clusters: the comparison must not be about empty results only"
    eng.close()


# ---- 4. the drop-in class -----------------------------------------------------------------------------------------------
def _golden_memory(torch, tmp_path, name="g2_mini_s1"):
    import bsc_nav_amd as B
    z = gu.load(name)
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
    return z, mem


def test_working_memory_retrieval_batch(torch_cuda, tmp_path):
    torch = torch_cuda
    z, mem = _golden_memory(torch, tmp_path)
    specs = list(gu.query_specs(z))
    prompts = [torch.from_numpy(s["pooled"].reshape(-1)).cuda() for s in specs]
    assert len(prompts) >= 2
    vox = np.asarray(mem.grid_rgb_pos)
    centre = vox[len(vox) // 2].tolist()
    far = (vox.max(0) + 50).tolist()
    K, eps, ms = 100, 4.0, 3
    radii = [np.inf if i % 3 == 0 else 6.0 + 3 * i for i in range(len(prompts))] + [1.0]
    currs = [centre if i % 2 else vox[(7 * i) % len(vox)].tolist() for i in range(len(prompts))] + [far]
    batch_prompts = prompts + [prompts[0]]                         # the last one looks into an empty region
    out = mem.working_memory_retrieval_batch(batch_prompts, K=K, region_radius=radii, curr_grid=currs, eps=eps, min_samples=ms)
    loc = mem.voxel_localized_batch(batch_prompts, K=K, region_radius=radii, curr_grid=currs)
    assert len(out) == len(loc) == len(batch_prompts)
    n_clustered = 0
    for i, (centers, tpos, tsim, labels, sizes) in enumerate(out):
        assert tpos.dtype == np.int64 and tsim.dtype == np.float64 and centers.dtype == np.float64 and centers.shape[1:] == (3,)
        assert np.array_equal(tpos, loc[i][1]) and np.array_equal(tsim, loc[i][2])
        if len(tpos) == 0:
            assert i == len(prompts) and centers.shape == (0, 3) and len(labels) == 0 and sizes == []
            continue
        assert _same((centers, labels, sizes), mem.weighted_cluster_centers(loc[i][1], loc[i][2], eps=eps, min_samples=ms))
        n_clustered += len(sizes) >= 1
    assert len(out[-1][1]) == 0 and n_clustered >= 1
    # weighted_cluster_centers_batch: the lists voxel_localized_batch returned, empty one included
    twin = mem.weighted_cluster_centers_batch([l[1] for l in loc], [l[2] for l in loc], eps=eps, min_samples=ms)
    for i in range(len(out)):
        assert _same(twin[i], (out[i][0], out[i][3], out[i][4]))
    # the adaptive-region loop (BSCAgent.py:1078-1098) as one call == three single retrievals
    three = mem.working_memory_retrieval_batch([prompts[0]] * 3, K=K, region_radius=(30, 40, 50), curr_grid=centre, eps=eps,
                                               min_samples=ms)
    near = mem.working_memory_retrieval_batch([prompts[0]] * 3, K=K, region_radius=(30, 40, 50), curr_grid=centre, eps=eps,
                                              min_samples=ms, nearest_first=True)
    for j, r in enumerate((30, 40, 50)):
        _, tpos, tsim = mem.voxel_localized(prompts[0], K=K, region_radius=r, curr_grid=centre)
        single = mem.weighted_cluster_centers(tpos, tsim, eps=eps, min_samples=ms)
        assert np.array_equal(three[j][1], tpos) and np.array_equal(three[j][2], tsim)
        assert _same((three[j][0], three[j][3], three[j][4]), single)
        # nearest_first: BSCAgent.py:1086-1090 with a stable sort; top-K and labels stay as they are
        order = np.argsort(np.linalg.norm(single[0] - np.array(centre), axis=1), kind="stable")
        assert np.array_equal(near[j][0], single[0][order]) and near[j][4] == [single[2][k] for k in order]
        assert np.array_equal(near[j][1], tpos) and np.array_equal(near[j][3], single[1])
        d = np.linalg.norm(near[j][0] - np.array(centre), axis=1)
        assert np.all(np.diff(d) >= 0)
    assert any(len(t[4]) >= 2 for t in three), "the ordering check needs a prompt with several clusters"
    with pytest.raises(ValueError):
        mem.working_memory_retrieval_batch(prompts[:1], K=K, nearest_first=True)
    mem.engine.close()


# ---- 5. refusals --------------------------------------------------------------------------------------------------------
def test_invalid_arguments_are_refused_and_change_nothing(torch_cuda):
    torch = torch_cuda
    eng, keys, kk, rows, seg, gen = _medium_map(torch, "mean")
    lib = eng.lib
    fresh = _tiny_engine()                                         # has not localized yet: nothing resident
    res = _raw(fresh, 1, 10, None, None, None, 10.0, 5)
    assert res[0] == BSC_E_INVALID and lib.bsc_last_error() and _untouched(res)
    fresh.close()
    Q, K = 4, 10
    q = torch.randn((Q, rows.shape[1]), device="cuda", generator=gen)
    p, s, n = eng.localize_regions(q, K=K, radius=[None, 30.0, 2.0, None], curr=kk[5].tolist())
    assert n[0] == K and 1 <= n[2] < K
    good = _raw(eng, Q, K, None, None, None, 20.0, 3)
    assert good[0] == 0
    _assert_rows(good, n)
    nan = float("nan")
    cnt_ok = np.array(n, np.int32)
    cases = {
        "NULL context": dict(handle=None),
        "NULL centers": dict(drop="centers"), "NULL labels": dict(drop="labels"), "NULL sizes": dict(drop="sizes"),
        "NULL n_clusters": dict(drop="ncl"),
        "n_queries 0": dict(Q=0), "n_queries 1025": dict(Q=1025, pos=np.zeros((1025, K, 3), np.int32), sim=np.zeros((1025, K), np.float32)),
        "K 0": dict(K=0), "K 1025": dict(K=1025, pos=np.zeros((Q, 1025, 3), np.int32), sim=np.zeros((Q, 1025), np.float32)),
        "min_samples 0": dict(min_samples=0), "NaN eps": dict(eps=nan),
        "NaN eps, host form": dict(eps=nan, pos=p, sim=s),
        "host count above K": dict(pos=p, sim=s, counts=np.array([K, K + 1, 0, 1], np.int32)),
        "host count negative": dict(pos=p, sim=s, counts=np.array([K, -1, 0, 1], np.int32)),
        "resident count above the query's results": dict(counts=np.array([n[0], n[1], n[2] + 1, n[3]], np.int32)),
        "resident count negative": dict(counts=np.array([n[0], -1, 0, 0], np.int32)),
        "pos without sim": dict(pos=p), "sim without pos": dict(sim=s),
        "resident, other query count": dict(Q=3), "resident, more queries": dict(Q=5),
        "resident, K above the call's": dict(K=K + 1),
    }
    for name, kw in cases.items():
        a = dict(Q=Q, K=K, counts=None, pos=None, sim=None, eps=20.0, min_samples=3, handle="ctx", drop=None)
        a.update(kw)
        res = _raw(eng, a["Q"], a["K"], a["counts"], a["pos"], a["sim"], a["eps"], a["min_samples"], handle=a["handle"],
                   rows=max(a["Q"], 1), drop=a["drop"])
        assert res[0] == BSC_E_INVALID, name
        assert len(lib.bsc_last_error()) > 0, name
        assert _untouched(res), name
        again = _raw(eng, Q, K, None, None, None, 20.0, 3)         # the resident results were not disturbed
        assert again[0] == 0 and all(np.array_equal(x, y) for x, y in zip(good[1:], again[1:])), name
    ok = _raw(eng, Q, K, cnt_ok, None, None, 20.0, 3)              # counts equal to what the queries found: the default
    assert ok[0] == 0 and all(np.array_equal(x, y) for x, y in zip(good[1:], ok[1:]))
    with pytest.raises(RuntimeError):
        eng.cluster_centers_batch(K=K + 1)
    with pytest.raises(ValueError):
        eng.cluster_centers_batch(p, None)
    eng.close()


# ---- 6. two contexts ----------------------------------------------------------------------------------------------------
def test_two_contexts_keep_their_own_results(torch_cuda):
    torch = torch_cuda
    ea, _, kka, rows_a, _, gen_a = _medium_map(torch, "mean", seed=3)
    eb, _, kkb, rows_b, _, gen_b = _medium_map(torch, "exact", seed=4)
    qa = torch.randn((8, rows_a.shape[1]), device="cuda", generator=gen_a)
    qb = torch.randn((5, rows_b.shape[1]), device="cuda", generator=gen_b)
    pa, sa, na = ea.localize_regions(qa, K=100, radius=25.0, curr=kka[7].tolist())
    pb, sb, nb = eb.localize_regions(qb, K=60, radius=[None, 20.0, 3.0, 25.0, None], curr=kkb[9].tolist())
    assert not np.array_equal(pa[0, :60], pb[0])
    ra1 = ea.cluster_centers_batch(eps=20.0, min_samples=3)
    rb1 = eb.cluster_centers_batch(eps=20.0, min_samples=3)
    ra2 = ea.cluster_centers_batch(eps=20.0, min_samples=3)
    rb2 = eb.cluster_centers_batch(eps=20.0, min_samples=3)
    assert len(ra1) == 8 and len(rb1) == 5
    for i in range(8):
        assert _same(ra1[i], ra2[i]) and _same(ra1[i], ea.cluster_centers(pa[i, :na[i]], sa[i, :na[i]], eps=20.0, min_samples=3))
    for i in range(5):
        assert _same(rb1[i], rb2[i]) and _same(rb1[i], eb.cluster_centers(pb[i, :nb[i]], sb[i, :nb[i]], eps=20.0, min_samples=3))
    assert any(len(r[2]) >= 1 for r in ra1) and any(len(r[2]) >= 1 for r in rb1)
    ea.close()
    eb.close()
