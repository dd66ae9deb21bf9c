"""bsc_topdown_slices / bsc_topdown_rebuild (VoxelEngine.topdown_slices / rebuild_topdown, VoxelTokenMemory.topdown_maps /
rgb_2d_map / rebuild_topdown_map): top-down maps of height bands from the stored voxels.  Everything here is integer work, so
colour, height and count must be exact.  The expected result is the rule restated in NumPy below (_rule); the golden maps are
the reference's own TrajectoryDrawer._get_rgb_2d_map (BSCAgent.py:203-234)."""
import ctypes as C

import numpy as np
import pytest

import golden_util as gu

pytestmark = pytest.mark.gpu
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device (no CPU fallback exists)")
    return torch


# ---- the rule, in NumPy -------------------------------------------------------------------------------------------------
def _rule(pos, rgb, gs, nh, bands):
    """pos (V,3) distinct stored positions, rgb (V,3); bands a list of (lo, hi) / None -> rgb (S,gs,gs,3) u8, height (S,gs,gs)
    i32, count (S,gs,gs) i32: per band and column the colour and h of the highest voxel with lo <= h <= hi (0 / -1: none) and
    the number of such voxels.  None or lo > hi: every height; bands are clipped to [0, nh)."""
    S = len(bands)
    out_rgb = np.zeros((S, gs * gs, 3), np.uint8)
    out_h = np.full((S, gs * gs), -1, np.int32)
    out_n = np.zeros((S, gs * gs), np.int32)
    pos, rgb = np.asarray(pos, np.int64).reshape(-1, 3), np.asarray(rgb, np.uint8).reshape(-1, 3)
    order = np.argsort(pos[:, 2], kind="stable")                # ascending h: of a column's writes below, the highest lands last
    cell, h, col = (pos[:, 0] * gs + pos[:, 1])[order], pos[order, 2], rgb[order]
    for s, b in enumerate(bands):
        lo, hi = (0, nh - 1) if (b is None or b[0] > b[1]) else (max(b[0], 0), min(b[1], nh - 1))
        sel = (h >= lo) & (h <= hi)
        out_n[s] = np.bincount(cell[sel], minlength=gs * gs)
        out_h[s][cell[sel]] = h[sel]
        out_rgb[s][cell[sel]] = col[sel]
    return out_rgb.reshape(S, gs, gs, 3), out_h.reshape(S, gs, gs), out_n.reshape(S, gs, gs)


def _assert_slices(got, want, what, heights=True, counts=True):
    rgb, h, n = want
    assert str(got["rgb"].dtype) == "torch.uint8" and got["rgb"].is_cuda and tuple(got["rgb"].shape) == rgb.shape, what
    assert np.array_equal(got["rgb"].cpu().numpy(), rgb), (what, "colour")
    for k, on in (("height", heights), ("count", counts)):
        assert not on or (str(got[k].dtype) == "torch.int32" and tuple(got[k].shape) == h.shape), (what, k)
    if heights:
        assert np.array_equal(got["height"].cpu().numpy(), h), (what, "height")
    else:
        assert got["height"] is None
    if counts:
        assert np.array_equal(got["count"].cpu().numpy(), n), (what, "count")
    else:
        assert got["count"] is None


# ---- 1. the reference's own maps ------------------------------------------------------------------------------------------
def test_golden_rgb_2d_maps_of_the_reference(torch_cuda, tmp_path):
    import bsc_nav_amd as B
    z = gu.load("g10_topdown_slice")
    pos, rgb, cuts, maps = z["pos"], z["rgb"], z["cuts"].tolist(), z["maps_bgr"]
    gs, nh, minh, cs = int(z["gs"]), int(z["nh"]), int(z["minh"]), float(z["cs"])
    assert len(cuts) == len(maps) == 7 and maps.shape == (7, gs, gs, 3)
    bands = [(I32_MIN, int(c)) for c in cuts]
    want = _rule(pos, rgb, gs, nh, bands)
    assert np.array_equal(want[0][..., ::-1], maps), "the NumPy rule of this file is not the reference's method"
    eng = B.VoxelEngine(48, 64, gs, cs, 0.0, 0.0, 16, 16, mode="mean", voxel_capacity=len(pos) + 8, max_points=4096,
                        min_h=minh, max_h=minh + nh)
    eng.import_rgb(pos, rgb, np.ones(len(pos), np.float32))
    got = eng.topdown_slices(bands)                              # the seven cuts in one call
    assert np.array_equal(got["rgb"].cpu().numpy()[..., ::-1], maps)
    _assert_slices(got, want, "golden")
    eng.close()
    # the drop-in class: floor_height / map_height that give the recorded minh and nh (memory_2.py:122-123 truncates)
    args = B.MemoryArgs(width=64, height=48, grid_size=gs, cell_size=cs, floor_height=-0.75, map_height=1.75,
                        query_width=224, query_height=224, memory_path=str(tmp_path), scene_name="scene", token_dim=16)
    mem = B.VoxelTokenMemory(args, preload_dino=None, need_diffusion=False, feature_mode="mean")
    assert mem.minh == minh and mem.cs == cs and mem.gs == gs and mem.maxh - mem.minh == nh
    mem.engine.import_rgb(pos, rgb, np.ones(len(pos), np.float32))
    mem._touch()
    for height, m in zip(z["heights"].tolist(), maps):
        out = mem.rgb_2d_map(height)
        assert isinstance(out, np.ndarray) and out.dtype == np.uint8 and out.flags["C_CONTIGUOUS"]
        assert np.array_equal(out, m), height
    # topdown_maps / rebuild_topdown_map: the open band by default, the selected floor under load_single_floor
    full = _rule(pos, rgb, gs, nh, [None])
    _assert_slices(mem.topdown_maps(), full, "topdown_maps()")
    assert not mem.cv_map.any() and not np.isfinite(mem.max_height).any()       # an imported memory has no map ...
    mem.rebuild_topdown_map()
    assert np.array_equal(mem.cv_map, full[0][0])                                # ... until it is rebuilt; the cache was dropped
    assert np.array_equal(mem.max_height, np.where(full[1][0] >= 0, full[1][0].astype(np.float64), -np.inf))
    mem.args.load_single_floor, mem.floor_min_height, mem.floor_max_height = True, 3, 9
    floor = _rule(pos, rgb, gs, nh, [(3, 9)])
    _assert_slices(mem.topdown_maps(), floor, "topdown_maps() of the floor")
    _assert_slices(mem.topdown_maps([None, (3, 9)]), _rule(pos, rgb, gs, nh, [None, (3, 9)]), "topdown_maps(bands)")
    mem.rebuild_topdown_map()
    assert np.array_equal(mem.cv_map, floor[0][0])
    mem.rebuild_topdown_map((0, 0))
    assert np.array_equal(mem.cv_map, _rule(pos, rgb, gs, nh, [(0, 0)])[0][0])
    mem.engine.close()


# ---- 2. generated maps -----------------------------------------------------------------------------------------------------
def _voxels(rng, gs, nh, V):
    """V distinct voxels in a random id order, no colour black.  When V leaves room for them: three columns with every height
    occupied and three with exactly one voxel; the rest anywhere outside those six columns."""
    V = min(V, gs * gs * nh * 3 // 4)                            # (gs 16, nh 5 holds 1280 cells: 5000 voxels become 960)
    cols = rng.permutation(gs * gs)
    pos = []
    if V >= 3 * nh + 3 + 8:
        for c in cols[:3]:
            pos += [(c // gs, c % gs, h) for h in range(nh)]
        pos += [(c // gs, c % gs, int(rng.randint(nh))) for c in cols[3:6]]
    rest = cols[6:]
    codes = rng.permutation(len(rest) * nh)[:V - len(pos)]
    pos += [(rest[k // nh] // gs, rest[k // nh] % gs, k % nh) for k in codes]
    pos = np.array(pos, np.int32).reshape(-1, 3)[rng.permutation(V)] if V else np.zeros((0, 3), np.int32)
    assert len(pos) == V == len(np.unique(pos, axis=0) if V else pos)
    return pos, rng.randint(1, 256, size=(V, 3)).astype(np.uint8)


def _bands(rng, nh, S):
    """The cases every map is cut by, then random bands up to S.  The mask of the kernels holds 64 heights per word, so the
    bands end at 63, start at 64 and straddle 63/64 and 127/128 (clipped where nh is smaller)."""
    fixed = [None, (5, 2),                                       # open, as None and as lo > hi
             (0, 0), (nh - 1, nh - 1), (63, 63), (64, 64), (nh // 2, nh // 2),       # lo == hi
             (0, 63), (10, 63), (64, 100), (64, 127), (60, 70), (63, 64), (120, 130), (127, 128), (128, nh - 1), (1, nh - 2),
             (-3, 2), (nh - 2, nh + 50), (-10, -1), (nh, nh + 3), (I32_MIN, 3), (0, I32_MAX), (I32_MIN, I32_MAX), (I32_MIN, -1)]
    if S <= 7:
        pick = [fixed[0], fixed[1]] + [fixed[i] for i in rng.permutation(np.arange(2, len(fixed)))[:5]]
        return pick[:S]
    out = list(fixed)
    while len(out) < S:
        a, b = sorted(int(v) for v in rng.randint(-4, nh + 4, size=2))
        out.append((a, b))
    return out[:S]


def _load(torch, eng, mode, pos, rgb):
    if mode == "exact":
        eng.import_rgb(pos, rgb, np.ones(len(pos), np.float32))
    else:
        V, D = len(pos), eng.cfg.token_dim
        eng.dense_replace(torch.from_numpy(pos).cuda(), torch.ones((V, D), dtype=torch.float32, device="cuda"),
                          torch.ones(V, dtype=torch.int32, device="cuda"), torch.from_numpy(rgb).cuda(),
                          torch.ones(V, dtype=torch.float32, device="cuda"))


def _make_engine(mode, gs, nh, vcap):
    import bsc_nav_amd as B
    kw = dict(iter_size=256, token_capacity=4096) if mode == "exact" else {}
    return B.VoxelEngine(48, 64, gs, 0.1, 0.0, 0.0, 16, 16, mode=mode, voxel_capacity=vcap, max_points=4096, min_h=-2, max_h=nh - 2,
                         **kw)


@pytest.mark.parametrize("mode", ["exact", "mean"])
@pytest.mark.parametrize("nh", [5, 64, 65, 200])
@pytest.mark.parametrize("gs", [16, 64])
def test_generated_maps(torch_cuda, gs, nh, mode):
    """One context per (gs, nh, mode); the map is replaced for every voxel count: none, one, around the 256 threads of a
    workgroup, several workgroups."""
    rng = np.random.RandomState(1000 * gs + nh)
    eng = _make_engine(mode, gs, nh, 5008)
    assert eng.nh == nh
    for V in (0, 1, 255, 256, 257, 5000):
        pos, rgb = _voxels(rng, gs, nh, V)
        _load(torch_cuda, eng, mode, pos, rgb)
        what = (gs, nh, mode, V)
        _assert_slices(eng.topdown_slices(), _rule(pos, rgb, gs, nh, [None]), what + ("NULL",))          # S = 1, NULL bands
        b7 = _bands(rng, nh, 7)
        want7 = _rule(pos, rgb, gs, nh, b7)
        _assert_slices(eng.topdown_slices(b7), want7, what + (7,))
        _assert_slices(eng.topdown_slices(b7, heights=False), want7, what + ("no heights",), heights=False)
        _assert_slices(eng.topdown_slices(b7, counts=False), want7, what + ("no counts",), counts=False)
        _assert_slices(eng.topdown_slices(b7, heights=False, counts=False), want7, what + ("colours",), False, False)
        if V in (1, 257, 5000):
            b256 = _bands(rng, nh, 256)
            _assert_slices(eng.topdown_slices(b256), _rule(pos, rgb, gs, nh, b256), what + (256,))
            one = b256[2 + V % 23]
            _assert_slices(eng.topdown_slices([one]), _rule(pos, rgb, gs, nh, [one]), what + (one,))     # S = 1 with a band
    eng.close()


# ---- 3. rows past max_id are never read -------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["exact", "mean"])
def test_stale_rows_are_not_seen(torch_cuda, mode):
    gs, nh = 32, 70
    rng = np.random.RandomState(3)
    eng = _make_engine(mode, gs, nh, 5008)
    pos, rgb = _voxels(rng, gs, nh, 5300)
    _load(torch_cuda, eng, mode, pos[:5000], rgb[:5000])
    assert int(eng.topdown_slices()["count"].sum()) == 5000
    if mode == "exact":
        eng.reset()
        z = eng.topdown_slices()                                 # an empty memory: zeros, -1, 0
        assert not z["rgb"].any() and bool((z["height"] == -1).all()) and not z["count"].any()
    _load(torch_cuda, eng, mode, pos[5000:], rgb[5000:])          # (dense_replace leaves the old rows 300 .. 4999 in place)
    bands = [None, (0, 63), (64, 69), (30, 40)]
    _assert_slices(eng.topdown_slices(bands), _rule(pos[5000:], rgb[5000:], gs, nh, bands), "300 after 5000")
    eng.close()


# ---- 4. after an ingest -------------------------------------------------------------------------------------------------------
def _ingest(torch, eng, cfg, rgb, depth, poses, tokens, chain, frames):
    import bsc_nav_amd as B
    N = cfg["H"] * cfg["W"]
    for f in frames:
        T = chain.pc_transform(poses[f])
        idx = B.sample_indices(N, cfg["s"])
        eng.ingest(torch.from_numpy(depth[f:f + 1]).cuda(), torch.from_numpy(rgb[f:f + 1]).cuda(),
                   torch.from_numpy(tokens[f:f + 1]).cuda(), T[None], torch.from_numpy(idx).cuda(), np.array([0, len(idx)]))


def _ingest_engine(cfg, **kw):
    import bsc_nav_amd as B
    return B.VoxelEngine(cfg["H"], cfg["W"], cfg["gs"], cfg["cs"], cfg["floor_height"], cfg["map_height"], cfg["g"], cfg["D"],
                         mode="exact", iter_size=cfg.get("iter_size", 50000), max_points=cfg["H"] * cfg["W"], **kw)


def test_open_band_after_an_ingest_is_the_resident_map(torch_cuda):
    """The highest point of a column lies in its highest voxel: the open band's height is max_height; colours and counts are
    those of export_rgb's rows."""
    import bsc_nav_amd as B
    cfg, rgb, depth, poses, tokens = gu.ingest_inputs(gu.load("g2_mini_s1"))
    np.random.seed(cfg["seed"])
    eng = _ingest_engine(cfg)
    _ingest(torch_cuda, eng, cfg, rgb, depth, poses, tokens, B.PoseChain(), range(cfg["F"]))
    got = eng.topdown_slices()
    mh, _ = eng.export_heightmap()
    assert np.isfinite(mh).any()
    assert np.array_equal(got["height"][0].cpu().numpy(), np.where(np.isfinite(mh), mh, -1).astype(np.int32))
    vpos, vrgb, _ = eng.export_rgb()
    assert len(vpos) > 0
    _assert_slices(got, _rule(vpos, vrgb, cfg["gs"], eng.nh, [None]), "after ingest")
    lo, hi = int(vpos[:, 2].min()) + 1, int(vpos[:, 2].max()) - 1
    _assert_slices(eng.topdown_slices([(lo, hi), (I32_MIN, lo)]), _rule(vpos, vrgb, cfg["gs"], eng.nh, [(lo, hi), (I32_MIN, lo)]),
                   "bands after ingest")
    eng.close()


# ---- 5. rebuild --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("band", [None, (20, 66), (64, 64), (200, 300)])
def test_rebuild_makes_the_slice_the_resident_map(torch_cuda, band):
    gs, nh = 64, 70
    rng = np.random.RandomState(5)
    eng = _make_engine("mean", gs, nh, 5008)
    pos, rgb = _voxels(rng, gs, nh, 5000)
    _load(torch_cuda, eng, "mean", pos, rgb)
    srgb, sh, _ = (a[0] for a in _rule(pos, rgb, gs, nh, [band]))
    assert not eng.export_heightmap()[1].any()                   # nothing before the rebuild
    eng.rebuild_topdown(band)
    mh, cv = eng.export_heightmap()
    assert np.array_equal(cv, srgb)
    assert np.array_equal(mh, np.where(sh >= 0, sh.astype(np.float64), -np.inf))
    mask = eng.frontier_mask()
    assert np.array_equal((mask & 1).astype(bool), srgb.sum(-1, dtype=np.int64) != 0)
    a = eng.frontier_clusters(None, 2, 3)
    eng.import_cv_map(srgb)
    assert np.array_equal(eng.frontier_mask(), mask)
    b = eng.frontier_clusters(None, 2, 3)
    assert a["n"] == b["n"] and a["best"] == b["best"] and (a["n"] > 0 or band not in (None, (20, 66)))
    for k in ("first", "sizes", "centers", "gains", "labels"):
        assert np.array_equal(a[k], b[k]), k
    _assert_slices(eng.topdown_slices([band]), _rule(pos, rgb, gs, nh, [band]), "slices after the rebuild")    # the voxels are as they were
    eng.close()


def test_ingest_continues_from_a_rebuilt_map(torch_cuda):
    """Engine B ingests all frames but the last; engine A is given B's voxels and rebuilds its map from them; the last frame
    then leaves the same max_height in both (memory_2.py:901-903: height >= max_height)."""
    import bsc_nav_amd as B
    cfg, rgb, depth, poses, tokens = gu.ingest_inputs(gu.load("g2_mini_s1"))
    F = cfg["F"]
    assert F >= 2
    np.random.seed(cfg["seed"])
    chain = B.PoseChain()
    eb = _ingest_engine(cfg)
    _ingest(torch_cuda, eb, cfg, rgb, depth, poses, tokens, chain, range(F - 1))
    ea = _ingest_engine(cfg)
    ea.import_rgb(*eb.export_rgb())
    assert not np.isfinite(ea.export_heightmap()[0]).any()
    ea.rebuild_topdown()
    assert np.array_equal(ea.export_heightmap()[0], eb.export_heightmap()[0])
    T = chain.pc_transform(poses[F - 1])
    idx = torch_cuda.from_numpy(B.sample_indices(cfg["H"] * cfg["W"], cfg["s"])).cuda()
    for e in (ea, eb):
        e.ingest(torch_cuda.from_numpy(depth[F - 1:F]).cuda(), torch_cuda.from_numpy(rgb[F - 1:F]).cuda(),
                 torch_cuda.from_numpy(tokens[F - 1:F]).cuda(), T[None], idx, np.array([0, idx.numel()]))
    mha, mhb = ea.export_heightmap()[0], eb.export_heightmap()[0]
    assert np.array_equal(mha, mhb) and np.isfinite(mhb).any()
    ea.close(); eb.close()


def test_slices_leave_the_resident_localize_results_alone(torch_cuda):
    import bsc_nav_amd as B
    torch = torch_cuda
    gs, D, V = 32, 64, 3000
    rng = np.random.RandomState(8)
    codes = rng.permutation(gs ** 3)[:V]
    keys = np.stack([codes // (gs * gs), (codes // gs) % gs, codes % gs], 1).astype(np.int32)
    rows = rng.standard_normal((V, D)).astype(np.float32)
    col = rng.randint(1, 256, size=(V, 3)).astype(np.uint8)
    eng = B.VoxelEngine(48, 64, gs, 0.1, -1.6, 1.6, 16, D, mode="exact", iter_size=256, voxel_capacity=V + 8,
                        token_capacity=V + 4096, max_points=4096)
    eng.import_rgb(keys, col, np.ones(V, np.float32))
    eng.import_store(keys, np.ones(V, np.int32), rows, np.zeros(V, np.float32))
    q = torch.from_numpy(rows[:3] + 0.05 * rng.standard_normal((3, D)).astype(np.float32)).cuda()
    p1, s1, c1 = eng.localize(q, K=200)
    before = [eng.cluster_centers(K=200, query_index=i, eps=6.0, min_samples=3) for i in range(3)]
    _assert_slices(eng.topdown_slices([None, (3, 20)]), _rule(keys, col, gs, eng.nh, [None, (3, 20)]), "between localize calls")
    after = [eng.cluster_centers(K=200, query_index=i, eps=6.0, min_samples=3) for i in range(3)]
    for (ca, la, sa), (cb, lb, sb) in zip(before, after):
        assert np.array_equal(ca, cb) and np.array_equal(la, lb) and sa == sb
    p2, s2, c2 = eng.localize(q, K=200)
    assert np.array_equal(p1, p2) and np.array_equal(s1, s2) and np.array_equal(c1, c2)
    eng.close()


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(torch_cuda):
    from bsc_nav_amd import _lib
    from bsc_nav_amd.engine import BAND_DTYPE, _dp, _hp
    torch = torch_cuda
    gs, nh = 16, 65
    rng = np.random.RandomState(6)
    eng = _make_engine("mean", gs, nh, 1024)
    pos, col = _voxels(rng, gs, nh, 600)
    _load(torch, eng, "mean", pos, col)
    eng.rebuild_topdown((0, 63))
    mh0, cv0 = eng.export_heightmap()
    S = 257
    rgb = torch.full((S, gs, gs, 3), 0xA5, dtype=torch.uint8, device="cuda")
    hgt = torch.full((S, gs, gs), -77, dtype=torch.int32, device="cuda")
    cnt = torch.full((S, gs, gs), -78, dtype=torch.int32, device="cuda")
    bands = np.zeros(S, BAND_DTYPE)
    bands["hi"] = nh
    for n, outs in ((0, (rgb, hgt, cnt)), (257, (rgb, hgt, cnt)), (-1, (rgb, hgt, cnt)), (4, (None, None, None))):
        with pytest.raises(RuntimeError) as e:
            _lib.check(eng.lib.bsc_topdown_slices(eng.h, n, _hp(bands), *[_dp(t) for t in outs]))
        assert "bsc_topdown_slices" in str(e.value)
    with pytest.raises(RuntimeError):
        _lib.check(eng.lib.bsc_topdown_slices(None, 1, _hp(bands), _dp(rgb), _dp(hgt), _dp(cnt)))
    with pytest.raises(RuntimeError):
        _lib.check(eng.lib.bsc_topdown_rebuild(None, 0, 5))
    with pytest.raises(RuntimeError):
        eng.topdown_slices([])
    with pytest.raises(RuntimeError):
        eng.topdown_slices([(0, 1)] * 257)
    torch.cuda.synchronize()
    assert bool((rgb == 0xA5).all()) and bool((hgt == -77).all()) and bool((cnt == -78).all())
    mh1, cv1 = eng.export_heightmap()
    assert np.array_equal(mh0, mh1) and np.array_equal(cv0, cv1) and cv0.any()
    # ... and the calls that are not refused still work: the last one given only a count
    got = torch.full((2, gs, gs), -78, dtype=torch.int32, device="cuda")
    _lib.check(eng.lib.bsc_topdown_slices(eng.h, 2, _hp(bands), None, None, _dp(got)))
    assert np.array_equal(got.cpu().numpy(), _rule(pos, col, gs, nh, [(0, nh), (0, nh)])[2])
    eng.close()
