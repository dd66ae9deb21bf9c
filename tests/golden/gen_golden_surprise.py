#!/usr/bin/env python3
"""Golden vectors of VoxelTokenMemory.update_memory_surp_base (memory_2.py:364-536), from the reference's own method.

Runs ONLY where the reference checkout can be imported (see gen_golden.py); only data is written:

  g9_surprise_direct_c10.npz / _c4.npz   a prior store made by update_memory_dist_base under a fixed random.seed, then a
                                          cache of dense neighbourhoods + a zero tail, flushed at radius 1 and at radius 2
  g9_surprise_e2e.npz                     synthetic frames through obs2voxeltoken, then update_memory_surp_base

Tokens are a few orthonormal directions plus small noise, so that every cosine sits far from both thresholds.  The
test-side replay (tests/surprise_replay.py) is run on the same inputs: it must equal the reference, its recorded margins
must exceed 1e-4, and (direct fixtures) every path of the policy must have fired.

Usage:  python tests/golden/gen_golden_surprise.py [--ref /root/reference]
"""
import argparse
import contextlib
import io
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import gen_golden as G  # noqa: E402
import synth  # noqa: E402
import surprise_replay as R  # noqa: E402

STHR, BTHR = 0.5, 0.95
MARGIN = 1e-4


def directions(rs, n, D):
    q, _ = np.linalg.qr(rs.standard_normal((D, n)))
    return q.T.astype(np.float32)


def token(rs, dirs, k, sigma=0.02):
    D = dirs.shape[1]
    return (dirs[k] * rs.uniform(0.5, 2.0) + sigma * rs.standard_normal(D)).astype(np.float32)


def run_ref(M, feat, pos, dis, fn):
    B = M.iter_size
    M.grid_feat = np.zeros((B, M.token_dim), np.float32)
    M.grid_feat_pos = np.zeros((B, 3), np.int32)
    M.grid_feat_dis = np.zeros(B, np.float32)
    M.grid_feat[:len(feat)], M.grid_feat_pos[:len(pos)], M.grid_feat_dis[:len(dis)] = feat, pos, dis
    with contextlib.redirect_stdout(io.StringIO()):
        fn()


def compare(ref, rep, tag):
    rpos, rcnt, rfeat, rdis = ref
    pos, cnt, feat, dis, merged = rep
    assert np.array_equal(rpos, pos) and np.array_equal(rcnt, cnt), f"{tag}: store layout differs from the reference"
    un = ~merged
    assert np.array_equal(rfeat[un], feat[un]) and np.array_equal(np.asarray(rdis, np.float64)[un], dis[un]), tag
    if merged.any():
        a, b = feat[merged].astype(np.float64), rfeat[merged].astype(np.float64)
        rel = np.linalg.norm(a - b, axis=1) / np.linalg.norm(b, axis=1)
        assert rel.max() <= 1e-6, f"{tag}: merged tokens {rel.max()}"
        d32, r32 = dis[merged].astype(np.float32), np.asarray(rdis[merged]).astype(np.float32)
        assert np.all(np.abs(d32 - r32) <= np.spacing(np.abs(r32))), f"{tag}: merged distances"


def direct(ref_utils, ref_mem, name, cs, seed, out_dir):
    rs = np.random.RandomState(seed)
    D, gs, nd = 48, 16, 20
    cfg = dict(gs=gs, cs=0.1, floor_height=-0.4, map_height=0.4, H=48, W=64, g=16, D=D, s=1, iter_size=400)
    nh = 8
    dirs = directions(rs, nd, D)
    # a dense block of voxels (a fifth without a prior group), an isolated voxel A (full group with a zero token), a zero-token voxel Z inside the block
    block = [(r, c, h) for r in range(3, 9) for c in range(3, 9) for h in range(1, 5) if rs.rand() < 0.55]
    A, Z = (13, 13, 6), block[len(block) // 2]
    vox = sorted(set(block) | {A})
    # prior cache (update_memory_dist_base): a few tokens per block voxel from a small per-voxel direction set
    pf, pp, pd = [], [], []
    own = {v: rs.choice(8, 3, replace=False) for v in block}
    for v in block:
        if rs.rand() < 0.2:      # no prior group: the surprise flush creates it
            continue
        for _ in range(rs.randint(1, 5)):
            pf.append(token(rs, dirs, rs.choice(own[v]))); pp.append(v); pd.append(rs.uniform(0.5, 5))
    for k in range(cs - 1):
        pf.append(token(rs, dirs, 8 + k % 12)); pp.append(A); pd.append(rs.uniform(0.5, 5))
    pf.append(np.zeros(D, np.float32)); pp.append(A); pd.append(1.0)
    pf.append(np.zeros(D, np.float32)); pp.append(Z); pd.append(2.0)
    perm = rs.permutation(len(pf))
    pf, pp, pd = np.array(pf)[perm], np.array(pp, np.int32)[perm], np.array(pd, np.float32)[perm]
    cfg["iter_size"] = len(pf) + 40          # + zero rows: grid_0_0_0 exists before the surprise flush
    # the cache: runs at block voxels (directions old and new), novel directions at A, a zero tail
    cf, cp, cd = [], [], []
    while len(cf) < 330:
        v = block[rs.randint(len(block))]
        for _ in range(rs.choice([1, 1, 2, 3])):
            k = rs.choice(own[v]) if rs.rand() < 0.3 else rs.randint(nd)
            cf.append(token(rs, dirs, k)); cp.append(v); cd.append(rs.uniform(0.5, 5))
    for k in list(range(nd)) * 2:
        cf.append(token(rs, dirs, k)); cp.append(A); cd.append(rs.uniform(0.5, 5))
        if rs.rand() < 0.3:
            cf.append(token(rs, dirs, k)); cp.append(A); cd.append(rs.uniform(0.5, 5))
    n_real = len(cf)
    cache_rows = n_real + 150
    out = dict(D=np.array(D), gs=np.array(gs), nh=np.array(nh), cell=np.array(cfg["cs"]),
               floor_height=np.array(cfg["floor_height"]), map_height=np.array(cfg["map_height"]), cache_size=np.array(cs),
               sthr=np.array(STHR), bthr=np.array(BTHR), vox_pos=np.array(vox, np.int32), iter_size=np.array(cache_rows))
    cache_f = np.zeros((cache_rows, D), np.float32)
    cache_p = np.zeros((cache_rows, 3), np.int32)
    cache_d = np.zeros(cache_rows, np.float32)
    cache_f[:n_real], cache_p[:n_real], cache_d[:n_real] = np.array(cf), np.array(cp, np.int32), np.array(cd, np.float32)
    out.update(cache_feat=cache_f, cache_pos=cache_p, cache_dis=cache_d)
    totals = dict.fromkeys(R.PATHS, 0)
    for radius in (1, 2):
        path = f"mem://{name}_r{radius}"
        G._File._stores.pop(path, None)
        M = G.make_ref_memory(ref_utils, ref_mem, cfg, np.zeros((1, 1, 1, D), np.float32), path)
        M.cache_size = cs
        random.seed(seed)
        run_ref(M, pf, pp, pd, M.update_memory_dist_base)
        prior = G.dump_store(path)
        M.iter_size = cache_rows
        M.neighbor_radius, M.boring_threshold, M.surprise_threshold = radius, BTHR, STHR
        run_ref(M, cache_f, cache_p, cache_d, M.update_memory_surp_base)
        ref = G.dump_store(path)
        st = R.store_from_arrays(*prior)
        counts, margins = R.replay(st, cache_p, cache_f, cache_d, radius, STHR, BTHR, cs)
        rep = R.store_to_arrays(st, D)
        compare(ref, rep, f"{name} r{radius}")
        assert min(margins.values()) > MARGIN, (name, radius, margins)
        for k in R.PATHS:
            totals[k] += counts[k]
        if radius == 1:
            out.update(prior_pos=prior[0], prior_cnt=prior[1], prior_feat=prior[2], prior_dis=prior[3].astype(np.float32))
        out.update({f"r{radius}_pos": rep[0], f"r{radius}_cnt": rep[1], f"r{radius}_feat": rep[2], f"r{radius}_dis": rep[3],
                    f"r{radius}_merged": rep[4], f"r{radius}_counts": np.array([counts[k] for k in R.PATHS]),
                    f"r{radius}_margins": np.array([margins["surprise"], margins["boring"], margins["argmin"]])})
        print(f"{name} r{radius}: {counts} margins {margins}")
    assert all(totals[k] > 0 for k in R.PATHS), (name, totals)
    out["paths"] = np.array(R.PATHS)
    p = os.path.join(out_dir, f"{name}.npz")
    np.savez_compressed(p, **out)
    print(f"{name}: {os.path.getsize(p) / 1e3:.0f} kB")


def e2e(ref_utils, ref_mem, name, seed, out_dir):
    cfg = dict(gs=128, cs=0.1, floor_height=-2.0, map_height=4.4, seed=seed, F=6, H=240, W=320, kind="room", g=14, D=32, s=100,
               iter_size=4000)
    rs = np.random.RandomState(seed)
    dirs = directions(rs, 12, cfg["D"])
    F, g, D = cfg["F"], cfg["g"], cfg["D"]
    rgb, depth, poses = synth.make_frames(seed, F, cfg["H"], cfg["W"], cfg["kind"])
    # the direction follows the patch (4 x 4 patches share one): neighbouring voxels mostly agree
    tokens = np.stack([token(rs, dirs, (f + (py // 4) * 4 + px // 4) % 12)
                       for f in range(F) for py in range(g) for px in range(g)]).reshape(F, g, g, D)
    path = f"mem://{name}"
    G._File._stores.pop(path, None)
    M = G.make_ref_memory(ref_utils, ref_mem, cfg, tokens, path)
    np.random.seed(seed)
    random.seed(seed)
    with contextlib.redirect_stdout(io.StringIO()):
        for f in range(F):
            M._frame = f
            M.obs2voxeltoken({"rgb": rgb[f], "depth": depth[f]}, poses[f])
    assert M.iter_id > 0 and M.iter_id < M.iter_size
    prior = G.dump_store(path)
    out = dict(seed=np.array(seed), F=np.array(F), H=np.array(cfg["H"]), W=np.array(cfg["W"]), g=np.array(g), D=np.array(D),
               gs=np.array(cfg["gs"]), cell=np.array(cfg["cs"]), floor_height=np.array(cfg["floor_height"]),
               map_height=np.array(cfg["map_height"]), s=np.array(cfg["s"]), iter_size=np.array(cfg["iter_size"]),
               kind=np.array(cfg["kind"]), tokens=tokens, iter_id=np.array(M.iter_id), max_id=np.array(M.max_id),
               cache_size=np.array(M.cache_size), sthr=np.array(STHR), bthr=np.array(BTHR),
               prior_pos=prior[0], prior_cnt=prior[1])
    cache = (M.grid_feat.copy(), M.grid_feat_pos.copy(), M.grid_feat_dis.copy())
    M.neighbor_radius, M.boring_threshold, M.surprise_threshold = 1, BTHR, STHR
    with contextlib.redirect_stdout(io.StringIO()):
        M.update_memory_surp_base()
    ref = G.dump_store(path)
    st = R.store_from_arrays(*prior)
    counts, margins = R.replay(st, cache[1], cache[0], cache[2], 1, STHR, BTHR, int(M.cache_size))
    rep = R.store_to_arrays(st, D)
    compare(ref, rep, name)
    assert min(margins.values()) > MARGIN, (name, margins)
    assert counts["create"] > 0 and counts["append"] > 0 and counts["reject"] > 0, counts
    out.update(r1_pos=rep[0], r1_cnt=rep[1], r1_feat=rep[2], r1_dis=rep[3], r1_merged=rep[4],
               r1_counts=np.array([counts[k] for k in R.PATHS]),
               r1_margins=np.array([margins["surprise"], margins["boring"], margins["argmin"]]), paths=np.array(R.PATHS))
    print(f"{name}: iter_id={M.iter_id} {counts} margins {margins}")
    p = os.path.join(out_dir, f"{name}.npz")
    np.savez_compressed(p, **out)
    print(f"{name}: {os.path.getsize(p) / 1e3:.0f} kB")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--out", default=HERE)
    a = ap.parse_args()
    ref_utils, ref_mem = G.import_reference(a.ref)
    direct(ref_utils, ref_mem, "g9_surprise_direct_c10", 10, 91, a.out)
    direct(ref_utils, ref_mem, "g9_surprise_direct_c4", 4, 94, a.out)
    e2e(ref_utils, ref_mem, "g9_surprise_e2e", 95, a.out)


if __name__ == "__main__":
    main()
