"""bsc_render_views (VoxelEngine.render_views, VoxelTokenMemory.render_view / visible_voxels): per pixel of a camera pose the first
stored voxel its ray meets, the depth where the ray enters it and its colour.  The expected result is render_scenes.slab_reference:
a NumPy slab intersection of every ray with every voxel's cell box in f64, with the ingest's truncation-cell intervals.  A pixel is
ambiguous (tol 1e-9) when the winner's interval is shorter than tol or within tol of t_min / t_max, or another voxel enters within tol
of the winner; at most 0.5 % of a view's pixels may be (asserted); on every other pixel voxel and rgb must be equal and the depth
within 1e-6 max(1, t) — f32 rounding is 6e-8 relative and the two f64 evaluations differ by far less."""
import copy

import numpy as np
import pytest

import render_scenes as rs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device (no CPU fallback exists)")
    return torch


def _engine(grid, vcap, mode="mean"):
    import bsc_nav_amd as B
    kw = dict(iter_size=256, token_capacity=4096) if mode == "exact" else {}
    return B.VoxelEngine(48, 64, grid["gs"], grid["cs"], 0.0, 0.0, 16, 16, mode=mode, voxel_capacity=vcap, max_points=4096,
                         min_h=grid["min_h"], max_h=grid["min_h"] + grid["nh"], **kw)


def _load(eng, pos, rgb):
    eng.import_rgb(pos, rgb, np.ones(len(pos), np.float32))    # ids are the rows' indices


def _np(got):
    return {k: (None if v is None else v.cpu().numpy()) for k, v in got.items()}


def _assert_view(got, v, ref, rgb, what):
    """view v of the call's outputs (NumPy) against the reference of that camera"""
    P = len(ref["idx"])
    sure = ~ref["ambiguous"]
    n_amb = int(ref["ambiguous"].sum())
    idx, t = ref["idx"], ref["t"]
    err = np.zeros(P)
    if got["depth"] is not None:
        err = np.abs(got["depth"][v].reshape(-1).astype(np.float64) - t) / np.maximum(1.0, t)
    print(what, "pixels", P, "ambiguous", n_amb, "hits", int((idx >= 0).sum()), "max depth error / max(1, t)", float(err[sure].max()))
    assert n_amb <= rs.AMBIGUOUS_CAP * P, (what, n_amb)
    if got["voxel"] is not None:
        assert got["voxel"].dtype == np.int32
        assert np.array_equal(got["voxel"][v].reshape(-1)[sure], idx[sure]), (what, "voxel")
    if got["rgb"] is not None:
        assert got["rgb"].dtype == np.uint8
        want = np.where(idx[:, None] >= 0, np.asarray(rgb)[np.maximum(idx, 0)], 0).astype(np.uint8)
        assert np.array_equal(got["rgb"][v].reshape(-1, 3)[sure], want[sure]), (what, "rgb")
    if got["depth"] is not None:
        assert got["depth"].dtype == np.float32
        assert np.all(err[sure] <= 1e-6), (what, "depth", float(err[sure].max()))


def _reference(grid, pos, T, H, W, kinv=None, band=None, t_range=None):
    t_min, t_max = t_range or (grid["t_min"], grid["t_max"])
    return rs.slab_reference(grid["gs"], grid["nh"], grid["min_h"], grid["cs"], pos, T, rs.kinv_fov(H, W) if kinv is None else kinv,
                             H, W, t_min, t_max, band)


@pytest.fixture(scope="module")
def case1():
    """the generated scene and the reference of its six cameras, computed once"""
    pos, rgb = rs.case1_voxels()
    cams = rs.case1_cameras()
    return pos, rgb, cams, [_reference(rs.CASE1, pos, T, H, W) for _, T, H, W in cams]


# ---- 1. generated scene ----------------------------------------------------------------------------------------------------
def test_generated_scene_six_cameras(torch_cuda, case1):
    pos, rgb, cams, refs = case1
    g = rs.CASE1
    eng = _engine(g, len(pos) + 8)
    _load(eng, pos, rgb)
    singles = []
    for (name, T, H, W), ref in zip(cams, refs):
        got = _np(eng.render_views(T, size=(H, W), kinv=rs.kinv_fov(H, W), t_range=(g["t_min"], g["t_max"])))
        assert got["voxel"].shape == (1, H, W) and got["depth"].shape == (1, H, W) and got["rgb"].shape == (1, H, W, 3)
        _assert_view(got, 0, ref, rgb, name)
        singles.append(got)
    # all six in one call equal six single calls bit for bit (one size per call: the two sizes are batched separately)
    for size in {(H, W) for _, _, H, W in cams}:
        members = [i for i, c in enumerate(cams) if (c[2], c[3]) == size]
        got = _np(eng.render_views(np.stack([cams[i][1] for i in members]), size=size, kinv=rs.kinv_fov(*size),
                                   t_range=(g["t_min"], g["t_max"])))
        for v, i in enumerate(members):
            for k in ("voxel", "depth", "rgb"):
                assert np.array_equal(got[k][v].view(np.uint8), singles[i][k][0].view(np.uint8)), (cams[i][0], k)
    # ... and all six at one size in one call equal their six single calls at that size
    Ts = np.stack([c[1] for c in cams])
    six = _np(eng.render_views(Ts, size=(24, 32), kinv=rs.kinv_fov(24, 32), t_range=(g["t_min"], g["t_max"])))
    for v in range(6):
        one = _np(eng.render_views(Ts[v], size=(24, 32), kinv=rs.kinv_fov(24, 32), t_range=(g["t_min"], g["t_max"])))
        for k in ("voxel", "depth", "rgb"):
            assert np.array_equal(six[k][v].view(np.uint8), one[k][0].view(np.uint8)), (cams[v][0], k, "six in one call")
    eng.close()


# ---- 2. bricks ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["faces", "one_per_brick", "full_brick"])
def test_bricks(torch_cuda, scene):
    g = rs.CASE2
    pos = rs.case2_scenes()[scene]
    rgb = rs.colours(len(pos))
    eng = _engine(g, len(pos) + 8)
    _load(eng, pos, rgb)
    seen = 0
    for name, T, H, W in rs.case2_cameras():
        ref = _reference(g, pos, T, H, W)
        got = _np(eng.render_views(T, size=(H, W), kinv=rs.kinv_fov(H, W), t_range=(g["t_min"], g["t_max"])))
        _assert_view(got, 0, ref, rgb, (scene, name))
        seen += int((ref["idx"] >= 0).sum())
    assert seen > 20, "the cameras of this scene see next to nothing"
    eng.close()


# ---- 3. the ingest's inverse ---------------------------------------------------------------------------------------------------
def test_render_inverts_the_ingest(torch_cuda):
    """One every-pixel frame is ingested next to the map origin (the double-width cells) and rendered from the same pose with the
    context's own K^-1: every pixel whose point went into the grid sees a voxel no farther than its own depth, and its own voxel
    where the reference says that one comes first."""
    import bsc_nav_amd as B
    torch = torch_cuda
    H, W, gs, cs, min_h, max_h = 48, 64, 64, 0.1, -8, 24
    grid = dict(gs=gs, nh=max_h - min_h, min_h=min_h, cs=cs)
    eng = B.VoxelEngine(H, W, gs, cs, 0.0, 0.0, 16, 16, mode="mean", max_points=H * W, min_h=min_h, max_h=max_h)
    rng = np.random.RandomState(3)
    yy, xx = np.mgrid[0:H, 0:W]
    depth = (1.2 + 0.5 * np.sin(xx / 9.0) + 0.4 * np.cos(yy / 7.0) + 0.05 * rng.rand(H, W)).astype(np.float32)
    colour = rng.randint(1, 256, size=(1, H, W, 3)).astype(np.uint8)
    T = rs._pose((0.03, -0.04, 0.02), rs._euler(-75.0, 12.0, 40.0))
    d_depth = torch.from_numpy(depth[None]).cuda()
    eng.ingest(d_depth, torch.from_numpy(colour).cuda(), torch.rand((1, 16, 16, 16), dtype=torch.float32, device="cuda"), T[None])
    geo = eng.geometry(d_depth, T)
    in_grid = (geo["flags"] & 3) == 3
    assert in_grid.sum() > H * W // 2 and np.all((geo["flags"][in_grid] & 4) == 4)
    own = geo["vox"].astype(np.int64) - np.array([0, 0, min_h])
    occ = eng.export_occupied()
    own_id = occ[own[in_grid, 0], own[in_grid, 1], own[in_grid, 2]]
    assert np.all(own_id >= 0)
    assert np.abs(geo["vox"][in_grid, :2] - gs // 2).min() == 0 and (geo["vox"][in_grid, 2] == 0).any(), "no point in a double-width cell"
    got = _np(eng.render_views(T, t_range=(eng.cfg.min_depth, eng.cfg.max_depth)))
    voxel, rdepth = got["voxel"][0].reshape(-1), got["depth"][0].reshape(-1).astype(np.float64)
    z = depth.reshape(-1).astype(np.float64)
    assert np.all(voxel[in_grid] >= 0), "a pixel whose point was ingested sees no voxel"
    print("largest depth / z among the ingested pixels", float((rdepth[in_grid] / z[in_grid]).max()))
    assert np.all(rdepth[in_grid] <= z[in_grid] * (1 + 1e-6))
    vpos, vrgb, _ = eng.export_rgb()
    ref = rs.slab_reference(gs, grid["nh"], min_h, cs, vpos, T, np.array(eng.cfg.Kinv).reshape(3, 3), H, W, eng.cfg.min_depth,
                            eng.cfg.max_depth)
    first = in_grid & ~ref["ambiguous"]
    first[in_grid] &= ref["idx"][in_grid] == own_id
    assert first.sum() > 100
    assert np.array_equal(voxel[first], occ[own[first, 0], own[first, 1], own[first, 2]])
    _assert_view(got, 0, ref, vrgb, "after the ingest")
    eng.close()


# ---- 4. band and range --------------------------------------------------------------------------------------------------------
def _walls():
    """wall A (row 10, heights 4 .. 7) in front of wall B (row 6, every height), seen from next to the origin along +x"""
    a = [(10, c, h) for c in range(4, 28) for h in range(4, 8)]
    b = [(6, c, h) for c in range(2, 30) for h in range(12)]
    T = rs._pose((0.1, 0.13, 0.1), rs._look((1.0, 0.02, 0.03)))
    return np.array(a, np.int32), np.array(b, np.int32), T


def test_band_and_range(torch_cuda):
    g = rs.CASE1
    a, b, T = _walls()
    pos = np.concatenate([a, b])
    rgb = rs.colours(len(pos))
    H, W = 24, 32
    kw = dict(size=(H, W), kinv=rs.kinv_fov(H, W))
    eng = _engine(g, len(pos) + 8)
    _load(eng, pos, rgb)
    full = _np(eng.render_views(T, t_range=(0.1, 10.0), **kw))
    _assert_view(full, 0, _reference(g, pos, T, H, W), rgb, "both walls")
    shows_a = (full["voxel"][0] >= 0) & (full["voxel"][0] < len(a))
    assert shows_a.sum() > 50
    # a band makes the voxels outside it transparent: wall A lies in heights 4 .. 7
    for band in [(8, 11), (0, 3), (8, 100), (-7, 3)]:
        got = _np(eng.render_views(T, band=band, t_range=(0.1, 10.0), **kw))
        _assert_view(got, 0, _reference(g, pos, T, H, W, band=band), rgb, ("band", band))
        assert not ((got["voxel"][0] >= 0) & (got["voxel"][0] < len(a))).any(), "wall A shows through a band that excludes it"
        assert (got["voxel"][0][shows_a] >= len(a)).any(), "nothing of wall B behind wall A"
    banded = _np(eng.render_views(T, band=(8, 11), t_range=(0.1, 10.0), **kw))
    for band in [(5, 2), None]:                                 # lo > hi as given, and None: every height
        got = _np(eng.render_views(T, band=band, t_range=(0.1, 10.0), **kw))
        assert all(np.array_equal(got[k], full[k]) for k in full), band
    got = _np(eng.render_views(T, band=(12, 40), t_range=(0.1, 10.0), **kw))     # entirely outside: empty
    assert (got["voxel"] == -1).all() and not got["depth"].any() and not got["rgb"].any()
    # t_max in front of the wall gives none (wall A starts at x = 1.5, the camera stands at x = 0.1)
    got = _np(eng.render_views(T, t_range=(0.1, 1.0), **kw))
    assert (got["voxel"] == -1).all() and not got["depth"].any() and not got["rgb"].any()
    got = _np(eng.render_views(T, t_range=(0.1, 1.6), **kw))
    _assert_view(got, 0, _reference(g, pos, T, H, W, t_range=(0.1, 1.6)), rgb, "t_max inside wall A")
    assert (got["voxel"] >= 0).any() and (got["voxel"] < len(a)).all()
    # the same scene without wall A's heights: only the voxels of heights 8 .. 11 imported, no band
    keep = (pos[:, 2] >= 8) & (pos[:, 2] <= 11)
    _load(eng, pos[keep], rgb[keep])
    plain = _np(eng.render_views(T, t_range=(0.1, 10.0), **kw))
    assert np.array_equal(plain["depth"], banded["depth"]) and np.array_equal(plain["rgb"], banded["rgb"])
    assert np.array_equal(plain["voxel"] >= 0, banded["voxel"] >= 0)
    # the camera inside an occupied voxel: that voxel at t_min, in every pixel
    cell = np.array([[16 - 0, 16 - 0, 0 + 4]], np.int32)        # the double-width cells around the origin (min_h -4)
    _load(eng, np.concatenate([cell, b]), rgb[:1 + len(b)])
    got = _np(eng.render_views(T, t_range=(0.1, 10.0), **kw))
    assert (got["voxel"] == 0).all() and (got["depth"] == np.float32(0.1)).all() and (got["rgb"] == rgb[0]).all()
    eng.close()


# ---- 5. state ------------------------------------------------------------------------------------------------------------------
def test_empty_memory_reset_and_optional_outputs(torch_cuda, case1):
    pos, rgb, cams, refs = case1
    g = rs.CASE1
    name, T, H, W = cams[0]
    kw = dict(size=(H, W), kinv=rs.kinv_fov(H, W), t_range=(g["t_min"], g["t_max"]))
    eng = _engine(g, len(pos) + 8, mode="exact")
    got = _np(eng.render_views(T, **kw))                         # an empty memory
    assert (got["voxel"] == -1).all() and not got["depth"].any() and not got["rgb"].any()
    _load(eng, pos, rgb)
    _assert_view(_np(eng.render_views(T, **kw)), 0, refs[0], rgb, "exact mode")
    eng.reset()
    got = _np(eng.render_views(T, **kw))
    assert (got["voxel"] == -1).all() and not got["depth"].any() and not got["rgb"].any()
    few = slice(1200, 1500)                                     # a smaller import: no voxel of the old scene appears
    _load(eng, pos[few], rgb[few])
    got = _np(eng.render_views(T, **kw))
    _assert_view(got, 0, _reference(g, pos[few], T, H, W), rgb[few], "300 after 1500")
    assert got["voxel"].max() < 300
    # each output may be left out
    whole = _np(eng.render_views(T, **kw))
    for want in (("voxel",), ("depth",), ("rgb",), ("voxel", "rgb"), ("depth", "rgb")):
        part = _np(eng.render_views(T, want=want, **kw))
        for k in ("voxel", "depth", "rgb"):
            assert (part[k] is None) == (k not in want), (want, k)
            assert part[k] is None or np.array_equal(part[k], whole[k]), (want, k)
    eng.close()


def test_exact_and_mean_mode_give_identical_images(torch_cuda, case1):
    pos, rgb, cams, refs = case1
    g = rs.CASE1
    images = []
    for mode in ("exact", "mean"):
        eng = _engine(g, len(pos) + 8, mode=mode)
        _load(eng, pos, rgb)
        name, T, H, W = cams[2]
        images.append(_np(eng.render_views(T, size=(H, W), kinv=rs.kinv_fov(H, W), t_range=(g["t_min"], g["t_max"]))))
        _assert_view(images[-1], 0, refs[2], rgb, mode)
        eng.close()
    for k in ("voxel", "depth", "rgb"):
        assert np.array_equal(images[0][k], images[1][k]), k


def test_refusals_write_nothing(torch_cuda, case1):
    from bsc_nav_amd import _lib
    from bsc_nav_amd.engine import _dp, _hp, band_array
    torch = torch_cuda
    pos, rgb, cams, refs = case1
    g = rs.CASE1
    eng = _engine(g, len(pos) + 8)
    _load(eng, pos, rgb)
    H, W = 24, 32
    vox = torch.full((2, H, W), -77, dtype=torch.int32, device="cuda")
    dep = torch.full((2, H, W), -7.5, dtype=torch.float32, device="cuda")
    col = torch.full((2, H, W, 3), 0xA5, dtype=torch.uint8, device="cuda")
    T = np.ascontiguousarray(np.stack([cams[0][1], cams[2][1]]).reshape(2, 16))
    K = np.ascontiguousarray(rs.kinv_fov(H, W).reshape(9))

    def call(h=eng.h, V=2, T=T, K=K, H=H, W=W, t_min=0.1, t_max=10.0, outs=(vox, dep, col)):
        return eng.lib.bsc_render_views(h, V, _hp(T), _hp(K), H, W, t_min, t_max, None, *[_dp(t) for t in outs])

    def bad(a, i, v):
        a = a.copy()
        a.reshape(-1)[i] = v
        return a

    nan, inf = float("nan"), float("inf")
    refused = [dict(h=None), dict(T=None), dict(V=0), dict(V=1025), dict(V=-1), dict(H=0), dict(H=4097), dict(W=0), dict(W=4097),
               dict(T=bad(T, 5, nan)), dict(T=bad(T, 16 + 3, inf)), dict(T=bad(T, 31, -inf)), dict(K=bad(K, 0, nan)), dict(K=bad(K, 2, inf)),
               dict(K=bad(K, 8, 2.0)), dict(K=bad(K, 6, 1e-3)), dict(K=bad(K, 7, -1.0)),
               dict(t_min=-0.1), dict(t_min=10.0), dict(t_min=11.0), dict(t_min=nan), dict(t_max=nan), dict(t_max=inf),
               dict(t_min=inf, t_max=inf), dict(outs=(None, None, None))]
    for kw in refused:
        assert call(**kw) == -1, kw                             # BSC_E_INVALID
        with pytest.raises(RuntimeError) as e:
            _lib.check(call(**kw))
        assert "bsc_render_views" in str(e.value), kw
    odd = _engine(dict(g, gs=31), 64)                            # an odd grid: row 0 would be a second irregular cell
    assert call(h=odd.h) == -1
    with pytest.raises(RuntimeError) as e:
        odd.render_views(cams[0][1], size=(H, W))
    assert "odd" in str(e.value)
    odd.close()
    with pytest.raises(RuntimeError):
        eng.render_views(T, size=(H, W), want=())
    with pytest.raises(ValueError):
        eng.render_views(T, size=(H, W), want=("voxel", "score"))
    torch.cuda.synchronize()
    assert bool((vox == -77).all()) and bool((dep == -7.5).all()) and bool((col == 0xA5).all())
    # ... and a call that is not refused still works, with t_min = 0 and a band given
    assert call(t_min=0.0) == 0
    band = band_array([(0, 100)])
    assert eng.lib.bsc_render_views(eng.h, 1, _hp(T), _hp(K), H, W, 0.1, 10.0, _hp(band), _dp(vox), None, None) == 0
    _assert_view(dict(voxel=vox.cpu().numpy(), depth=None, rgb=None), 0, refs[0], rgb, "after the refusals")
    eng.close()


# ---- 6. the class ---------------------------------------------------------------------------------------------------------------
def test_memory_render_view_and_visible_voxels(torch_cuda, tmp_path):
    import bsc_nav_amd as B
    g = rs.CASE1
    pos, rgb = rs.case1_voxels()
    args = B.MemoryArgs(width=64, height=48, grid_size=g["gs"], cell_size=g["cs"], floor_height=-1.0, map_height=2.0,
                        query_width=224, query_height=224, memory_path=str(tmp_path), scene_name="scene", token_dim=16)
    mem = B.VoxelTokenMemory(args, preload_dino=None, need_diffusion=False, feature_mode="mean", voxel_capacity=len(pos) + 8)
    assert mem.minh == g["min_h"] and mem.maxh - mem.minh == g["nh"] and mem.gs == g["gs"]
    mem.engine.import_rgb(pos, rgb, np.ones(len(pos), np.float32))
    mem._touch()
    first = np.array([0.2, 1.5, -0.1, 0.0, 0.0, 0.0, 1.0])
    pose = np.array([0.55, 1.5, 0.35, 0.0, 0.38268343236508978, 0.0, 0.92387953251128674])
    with pytest.raises(RuntimeError):                           # before the first frame there is no map frame
        mem.render_view(pose)
    with pytest.raises(RuntimeError):
        mem.visible_voxels(pose)
    assert mem.chain.inv_init_base_tf is None
    mem.chain.pc_transform(first)                               # what the first obs2voxeltoken does to the chain
    tf, anchor = mem.chain.tf.copy(), mem.chain.inv_init_base_tf.copy()
    T = copy.deepcopy(mem.chain).pc_transform(pose)
    view = mem.render_view(pose)
    assert np.array_equal(mem.chain.tf, tf) and np.array_equal(mem.chain.inv_init_base_tf, anchor)
    want = _np(mem.engine.render_views(T))
    assert set(view) == {"voxel", "depth", "rgb"} and all(isinstance(v, np.ndarray) for v in view.values())
    assert view["voxel"].shape == (48, 64) and view["depth"].shape == (48, 64) and view["rgb"].shape == (48, 64, 3)
    for k in view:
        assert np.array_equal(view[k], want[k][0]), k
    ref = rs.slab_reference(g["gs"], g["nh"], g["min_h"], g["cs"], pos, T, np.array(mem.engine.cfg.Kinv).reshape(3, 3), 48, 64,
                            mem.min_depth, mem.max_depth)
    _assert_view(want, 0, ref, rgb, "render_view")
    assert (view["voxel"] >= 0).sum() > 200
    # size / fov / max_range
    small = mem.render_view(pose, size=(24, 32), fov=70, max_range=2.5)
    want = _np(mem.engine.render_views(T, size=(24, 32), kinv=np.linalg.inv(B.cam_mat_fov(24, 32, 70)), t_range=(mem.min_depth, 2.5)))
    for k in small:
        assert small[k].shape[:2] == (24, 32) and np.array_equal(small[k], want[k][0]), k
    # visible_voxels: ascending ids, counts sum to the hit pixels
    vpos, counts = mem.visible_voxels(pose)
    ids, n = np.unique(view["voxel"][view["voxel"] >= 0], return_counts=True)
    assert vpos.dtype == np.int64 and counts.dtype == np.int64 and vpos.shape == (len(ids), 3)
    assert np.array_equal(vpos, pos[ids].astype(np.int64)) and np.array_equal(counts, n)
    assert counts.sum() == (view["voxel"] >= 0).sum()
    vpos2, counts2 = mem.visible_voxels(pose, size=(24, 32), fov=70, max_range=2.5)
    assert counts2.sum() == (small["voxel"] >= 0).sum()
    assert np.array_equal(mem.chain.tf, tf) and np.array_equal(mem.chain.inv_init_base_tf, anchor)
    # the floor band by default under load_single_floor
    mem.args.load_single_floor, mem.floor_min_height, mem.floor_max_height = True, 3, 7
    floor = mem.render_view(pose)
    want = _np(mem.engine.render_views(T, band=(3, 7)))
    for k in floor:
        assert np.array_equal(floor[k], want[k][0]), k
    shown = pos[floor["voxel"][floor["voxel"] >= 0]]
    assert len(shown) and shown[:, 2].min() >= 3 and shown[:, 2].max() <= 7
    assert not np.array_equal(floor["voxel"], view["voxel"])
    every = mem.render_view(pose, band=(0, g["nh"] - 1))        # a band given overrides the floor
    assert np.array_equal(every["voxel"], view["voxel"])
    fpos, fcounts = mem.visible_voxels(pose)
    assert fcounts.sum() == (floor["voxel"] >= 0).sum() and fpos[:, 2].min() >= 3 and fpos[:, 2].max() <= 7
    mem.engine.close()
