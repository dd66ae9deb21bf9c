#!/usr/bin/env python3
"""Time one bsc_flush_surprise at the reference's shape: 640x480 frames, 768-D tokens (ViT-B/16), exact mode, a full
50 000-row cache.  Frames (4 000 sampled pixels each, structured tokens) are ingested until the next frame could trigger the
automatic flush; the state is exported once and re-imported before each timed flush.  Prints the flush time in ms and the
schedule (tasks = runs of consecutive rows at one voxel, levels of the dependency recurrence, computed here on the host).

    timeout -k 10 600 python scripts/surprise_flush_time.py [--reps 3]
"""
import argparse
import os
import random
import sys
import time
from itertools import product

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests", "golden")]
import bsc_nav_amd as B  # noqa: E402
import synth  # noqa: E402


def schedule(pos, occ, radius=1):
    """tasks and levels of the recurrence the library's planner computes (k_surp_levels)."""
    key = [tuple(p) for p in pos]
    offs = list(product(range(-radius, radius + 1), repeat=3))
    last, n_tasks, n_lev = {}, 0, 0
    prev = None
    for k in key:
        if k == prev:
            continue
        prev = k
        n_tasks += 1
        L = 1 + max(last.get((k[0] + a, k[1] + b, k[2] + c), 0) for a, b, c in offs)
        last[k] = L
        n_lev = max(n_lev, L)
    return n_tasks, n_lev


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    H, W, g, D, gs, N, P = 480, 640, 14, 768, 512, 50000, 4000
    mk = lambda: B.VoxelEngine(H, W, gs, 0.05, -3.2, 3.2, g, D, mode="exact", iter_size=N, max_points=P)
    eng = mk()
    rs = np.random.RandomState(3)
    q, _ = np.linalg.qr(rs.standard_normal((D, 24)))
    dirs = q.T.astype(np.float32)
    chain = B.PoseChain()
    random.seed(3)
    f, last = 0, 0
    while True:
        rgb, depth, poses = synth.make_frames(100 + f, 1, H, W, "room", start_yaw_steps=f)
        k = (f + (np.arange(g)[:, None] // 3) * 5 + np.arange(g)[None, :] // 3) % 24
        tok = (dirs[k] * rs.uniform(0.5, 2.0, (g, g, 1)) + 0.003 * rs.standard_normal((g, g, D))).astype(np.float32)[None]
        T = np.stack([chain.pc_transform(p) for p in poses])
        idx = torch.from_numpy(np.sort(rs.choice(H * W, P, replace=False)).astype(np.int32)).cuda()
        eng.ingest(torch.from_numpy(depth).cuda(), torch.from_numpy(rgb).cuda(), torch.from_numpy(tok).cuda(), T,
                   sample_idx=idx, offsets=[0, P])
        c = eng.counters()
        f += 1
        step = c["iter_id"] - last
        last = c["iter_id"]
        if c["flushes"] == 0 and c["iter_id"] + 2 * max(step, 1) > N:
            break
    cache, store, rgbs = eng.export_cache(), eng.export_store(), eng.export_rgb()
    n_tasks, n_lev = schedule(np.concatenate([cache[1], np.zeros((N - len(cache[1]), 3), np.int32)]), None)
    times = []
    for r in range(a.reps):
        e2 = mk()
        e2.import_rgb(*rgbs)
        e2.import_store(*store)
        e2.import_cache(cache[1], cache[0], cache[2])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e2.flush_surprise()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
        after = e2.counters()
        e2.close()
    eng.close()
    print(f"frames={f} cache_rows={len(cache[1])} voxels={len(rgbs[0])} store_before={len(store[2])} "
          f"store_after={after['store_tokens']} tasks={n_tasks} levels={n_lev}")
    print(f"flush_surprise ms: {' '.join(f'{t:.2f}' for t in times)} (median {np.median(times):.2f})")


if __name__ == "__main__":
    main()
