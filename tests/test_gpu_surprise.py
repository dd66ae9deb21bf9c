"""bsc_flush_surprise / VoxelTokenMemory.update_memory_surp_base (memory_2.py:364-536) on the GPU against the reference's
own results (g9_* fixtures) and against the test-side replay at the reference's shape."""
import math
import random

import numpy as np
import pytest

import golden_util as gu
import surprise_replay as R

pytestmark = pytest.mark.gpu


def assert_store_matches(got, pos, cnt, feat, dis, merged, tag=""):
    gpos, gcnt, gfeat, gdis = got
    assert np.array_equal(gpos, pos) and np.array_equal(gcnt, cnt), f"{tag}: voxels / counts differ"
    un = ~merged
    assert np.array_equal(gfeat[un], feat[un]), f"{tag}: un-merged tokens not bit-exact"
    assert np.array_equal(gdis[un].astype(np.float64), dis[un]), f"{tag}: un-merged distances not bit-exact"
    if merged.any():
        a, b = gfeat[merged].astype(np.float64), feat[merged].astype(np.float64)
        rel = np.linalg.norm(a - b, axis=1) / np.linalg.norm(b, axis=1)
        assert rel.max() <= 1e-6, f"{tag}: merged tokens off by {rel.max()}"
        ref32 = dis[merged].astype(np.float32)
        assert np.all(np.abs(gdis[merged] - ref32) <= np.spacing(np.abs(ref32))), f"{tag}: merged distances"


def _direct_engine(z):
    import bsc_nav_amd as B
    eng = B.VoxelEngine(48, 64, int(z["gs"]), float(z["cell"]), float(z["floor_height"]), float(z["map_height"]), 16,
                        int(z["D"]), mode="exact", iter_size=int(z["iter_size"]), cache_size=int(z["cache_size"]),
                        voxel_capacity=int(z["voxel_capacity"]) if "voxel_capacity" in z else None)
    vp = z["vox_pos"]
    eng.import_rgb(vp, np.zeros((len(vp), 3), np.uint8), np.zeros(len(vp), np.float32))
    eng.import_store(z["prior_pos"], z["prior_cnt"], z["prior_feat"], z["prior_dis"])
    eng.import_cache(z["cache_pos"], z["cache_feat"], z["cache_dis"])
    return eng


@pytest.mark.parametrize("name", ["g9_surprise_direct_c10", "g9_surprise_direct_c4"])
@pytest.mark.parametrize("radius", [1, 2])
def test_direct_fixture(name, radius):
    z = gu.load(name)
    eng = _direct_engine(z)
    c0 = eng.counters()
    assert c0["iter_id"] == int(z["iter_size"])
    eng.flush_surprise(radius, float(z["sthr"]), float(z["bthr"]))
    p = f"r{radius}_"
    got = eng.export_store()
    assert_store_matches(got, z[p + "pos"], z[p + "cnt"], z[p + "feat"], z[p + "dis"], z[p + "merged"], f"{name} r{radius}")
    c = eng.counters()
    assert c["iter_id"] == 0 and c["flushes"] == c0["flushes"] + 1
    assert c["store_voxels"] == len(z[p + "cnt"]) and c["store_tokens"] == int(z[p + "cnt"].sum())
    f, _, _ = eng.export_cache()
    assert len(f) == 0
    eng.close()


def _memory(z, tmp):
    import bsc_nav_amd as B
    from test_gpu_memory_api import FakeDino
    g = int(z["g"])
    args = B.MemoryArgs(width=int(z["W"]), height=int(z["H"]), grid_size=int(z["gs"]), cell_size=float(z["cell"]),
                        floor_height=float(z["floor_height"]), map_height=float(z["map_height"]),
                        depth_sample_rate=int(z["s"]), query_width=g * 14, query_height=g * 14, memory_path=str(tmp),
                        scene_name="scene", token_dim=int(z["D"]), iter_size=int(z["iter_size"]))
    dino = FakeDino(z["tokens"])
    return B.VoxelTokenMemory(args, preload_dino=dino, need_diffusion=False, alpha_source="host"), dino, args


def test_dropin_end_to_end(tmp_path):
    import synth
    z = gu.load("g9_surprise_e2e")
    seed, F = int(z["seed"]), int(z["F"])
    rgb, depth, poses = synth.make_frames(seed, F, int(z["H"]), int(z["W"]), str(z["kind"]))
    mem, dino, args = _memory(z, tmp_path)
    assert (mem.neighbor_radius, mem.boring_threshold, mem.surprise_threshold) == (1, 0.95, 0.5)
    np.random.seed(seed)
    random.seed(seed)
    for f in range(F):
        dino.frame = f
        mem.obs2voxeltoken({"rgb": rgb[f], "depth": depth[f]}, poses[f])
    assert mem.iter_id == int(z["iter_id"]) and mem.max_id == int(z["max_id"])
    pos0, cnt0, _, _ = mem.engine.export_store()
    assert np.array_equal(pos0, z["prior_pos"]) and np.array_equal(cnt0, z["prior_cnt"])
    mem.update_memory_surp_base()
    got = mem.engine.export_store()
    assert_store_matches(got, z["r1_pos"], z["r1_cnt"], z["r1_feat"], z["r1_dis"], z["r1_merged"], "e2e")
    assert mem.iter_id == 0
    # the shrunken store survives save_memory -> load_memory
    mem.initial_memory()
    mem.save_memory(original_pos=np.zeros(3, np.float32))
    mem2, _, args2 = _memory(z, tmp_path)
    args2.load_memory_path = mem.memory_save_path
    mem2.load_memory()
    got2 = mem2.engine.export_store()
    assert all(np.array_equal(a, b) for a, b in zip(got, got2))


def test_attributes_read_at_call_time(tmp_path):
    """radius / thresholds come from the attributes when the method runs: radius 2 on the drop-in == the r2 fixture."""
    z = gu.load("g9_surprise_direct_c10")
    eng = _direct_engine(z)
    import bsc_nav_amd as B
    mem = object.__new__(B.VoxelTokenMemory)
    mem.engine, mem.quiet = eng, True
    mem.neighbor_radius, mem.boring_threshold, mem.surprise_threshold = 2, float(z["bthr"]), float(z["sthr"])
    mem._touch = lambda: None
    B.VoxelTokenMemory.update_memory_surp_base(mem)
    assert_store_matches(eng.export_store(), z["r2_pos"], z["r2_cnt"], z["r2_feat"], z["r2_dis"], z["r2_merged"], "attrs")
    eng.close()


def test_errors_leave_state_unchanged():
    import bsc_nav_amd as B
    z = gu.load("g9_surprise_direct_c4")
    eng = _direct_engine(z)
    before = eng.export_store(), eng.export_cache(), eng.counters()
    for args in [(-1, 0.5, 0.95), (4, 0.5, 0.95), (1, math.nan, 0.95), (1, 0.5, math.nan)]:
        with pytest.raises(B._lib.BscError, match="status -1"):
            eng.flush_surprise(*args)
    bad = np.array([[15, 15, 7]], np.int32)      # no voxel there
    with pytest.raises(B._lib.BscError, match="status -1"):
        eng.import_cache(bad, np.ones((1, int(z["D"])), np.float32), np.ones(1, np.float32))
    after = eng.export_store(), eng.export_cache(), eng.counters()
    for x, y in zip(before[:2], after[:2]):
        assert all(np.array_equal(a, b) for a, b in zip(x, y))
    assert before[2] == after[2]
    eng.close()
    dense = B.VoxelEngine(48, 64, 16, 0.1, -0.4, 0.4, 16, 16, mode="mean")
    with pytest.raises(B._lib.BscError, match="status -4"):
        dense.flush_surprise()
    with pytest.raises(B._lib.BscError, match="status -4"):
        dense.import_cache(np.zeros((1, 3), np.int32), np.zeros((1, 16), np.float32), np.zeros(1, np.float32))
    dense.close()


def _dist_replay(st, pos, feat, dis, cs):
    """update_memory_dist_base (memory_2.py:326-358) on the replay's store, with Python's global RNG."""
    for i in range(len(pos)):
        p = tuple(int(v) for v in pos[i])
        g = st.get(p)
        if g is None or not g[0]:
            st[p] = [[np.asarray(feat[i], np.float32).copy()], [float(dis[i])], [False]]
        elif len(g[0]) < cs:
            g[0].append(np.asarray(feat[i], np.float32).copy()); g[1].append(float(dis[i])); g[2].append(False)
        else:
            k = random.choice(range(len(g[1])))
            g[0][k], g[1][k], g[2][k] = np.asarray(feat[i], np.float32).copy(), float(dis[i]), False


def test_dist_surprise_dist_sequence():
    z = gu.load("g9_surprise_direct_c10")
    cs, D = int(z["cache_size"]), int(z["D"])
    eng = _direct_engine(z)
    st = R.store_from_arrays(z["prior_pos"], z["prior_cnt"], z["prior_feat"], z["prior_dis"])
    rs = np.random.RandomState(5)
    n = int(z["iter_size"])
    # dist: the fixture's cache with shuffled block rows; surprise: the fixture's cache; dist again: the first one
    perm = rs.permutation(n)
    c1 = (z["cache_pos"][perm], z["cache_feat"][perm], z["cache_dis"][perm])
    eng.import_cache(*c1)
    random.seed(11)
    eng.flush()
    random.seed(11)
    _dist_replay(st, c1[0], c1[1], c1[2], cs)
    eng.import_cache(z["cache_pos"], z["cache_feat"], z["cache_dis"])
    eng.flush_surprise(1, float(z["sthr"]), float(z["bthr"]))
    counts, margins = R.replay(st, z["cache_pos"], z["cache_feat"], z["cache_dis"], 1, float(z["sthr"]), float(z["bthr"]), cs)
    assert min(margins.values()) > 1e-4, margins
    eng.import_cache(*c1)
    random.seed(12)
    eng.flush()
    random.seed(12)
    _dist_replay(st, c1[0], c1[1], c1[2], cs)
    pos, cnt, feat, dis, merged = R.store_to_arrays(st, D)
    assert_store_matches(eng.export_store(), pos, cnt, feat, dis, merged, "dist-surprise-dist")
    assert eng.counters()["flushes"] == 3
    eng.close()


def test_reference_shape_640x480_768():
    """640x480 frames, 768-D structured tokens, exact mode, iter_size 50 000: after an automatic mid-ingest flush, a cache of
    >= 40 000 rows is flushed by surprise and compared with the replay from the exported state."""
    import torch
    import bsc_nav_amd as B
    import synth
    H, W, g, D, gs = 480, 640, 14, 768, 512
    eng = B.VoxelEngine(H, W, gs, 0.05, -3.2, 3.2, g, D, mode="exact", iter_size=50000, max_points=H * W)
    rs = np.random.RandomState(3)
    q, _ = np.linalg.qr(rs.standard_normal((D, 24)))
    dirs = q.T.astype(np.float32)
    chain = B.PoseChain()
    random.seed(3)
    f, flushed = 0, False
    while True:
        rgb, depth, poses = synth.make_frames(100 + f, 1, H, W, "room", start_yaw_steps=f)
        k = (f + (np.arange(g)[:, None] // 3) * 5 + np.arange(g)[None, :] // 3) % 24
        tok = dirs[k] * rs.uniform(0.5, 2.0, (g, g, 1)).astype(np.float32)
        tok = (tok + 0.003 * rs.standard_normal((g, g, D))).astype(np.float32)[None]
        T = np.stack([chain.pc_transform(p) for p in poses])
        idx = torch.from_numpy(np.sort(rs.choice(H * W, 4000, replace=False)).astype(np.int32)).cuda()
        eng.ingest(torch.from_numpy(depth).cuda(), torch.from_numpy(rgb).cuda(), torch.from_numpy(tok).cuda(), T,
                   sample_idx=idx, offsets=[0, 4000])
        c = eng.counters()
        flushed = flushed or c["flushes"] > 0
        f += 1
        if flushed and c["iter_id"] >= 40000:
            break
        assert f < 400, "the cache never reached 40 000 rows after a flush"
    assert c["store_tokens"] > 0
    cache = eng.export_cache()
    prior = eng.export_store()
    rgbstate = eng.export_rgb()
    eng.flush_surprise()
    got = eng.export_store()
    st = R.store_from_arrays(*prior)
    ext = (np.concatenate([cache[1], np.zeros((50000 - len(cache[1]), 3), np.int32)]),
           np.concatenate([cache[0], np.zeros((50000 - len(cache[0]), D), np.float32)]),
           np.concatenate([cache[2], np.zeros(50000 - len(cache[2]), np.float32)]))
    counts, margins = R.replay(st, ext[0], ext[1], ext[2], 1, 0.5, 0.95, 10)
    assert min(margins.values()) >= 1e-4, f"data too close to a threshold: {margins}"
    pos, cnt, feat, dis, merged = R.store_to_arrays(st, D)
    assert_store_matches(got, pos, cnt, feat, dis, merged, "640x480x768")
    c2 = eng.counters()
    assert c2["iter_id"] == 0 and c2["flushes"] == c["flushes"] + 1 and c2["store_tokens"] == len(feat)
    # localize over the flushed engine == over a fresh engine that imported the exported store
    fresh = B.VoxelEngine(H, W, gs, 0.05, -3.2, 3.2, g, D, mode="exact", iter_size=50000, max_points=H * W)
    fresh.import_rgb(*rgbstate)
    fresh.import_store(*got)
    qv = torch.from_numpy((dirs[:3] + 0.01 * rs.standard_normal((3, D))).astype(np.float32)).cuda()
    a, b = eng.localize(qv, K=20), fresh.localize(qv, K=20)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    print(f"surprise flush at 640x480x768: {counts}")
    fresh.close()
    eng.close()
