#!/usr/bin/env python3
"""Build a memory under the surprise policy from the first frame on, at the shape of scripts/surprise_flush_time.py: 640x480
frames, 768-D structured tokens, exact mode, a 50 000-row cache, 4 000 sampled pixels per frame.  Every flush is the automatic
one inside ingest (bsc_set_flush_policy).  Prints one JSON line: flushes, ms per automatic flush (the ingest calls that
flushed, minus the median of those that did not; the compactions that ran behind those flushes included, and once more with
their time taken out), pool_rows / live_rows at the end, the automatic compactions of the build (how many, rows moved, ms;
bsc_compact_stats), localize ms for 1 and 256 queries, and last one explicit compaction of what the build left (rows moved,
rows freed, ms — under auto it usually finds nothing to do).  Run once per setting, each under its own time limit:

    BSC_STORE_COMPACT=auto  timeout -k 10 900 python scripts/surprise_build_time.py [--frames 150]
    BSC_STORE_COMPACT=never timeout -k 10 900 python scripts/surprise_build_time.py [--frames 150]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests", "golden")]
import bsc_nav_amd as B  # noqa: E402
import synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=150)
    a = ap.parse_args()
    H, W, g, D, gs, N, P = 480, 640, 14, 768, 512, 50000, 4000
    eng = B.VoxelEngine(H, W, gs, 0.05, -3.2, 3.2, g, D, mode="exact", iter_size=N, max_points=P)
    eng.set_flush_policy("surprise", 1, 0.5, 0.95)
    rs = np.random.RandomState(3)
    q, _ = np.linalg.qr(rs.standard_normal((D, 24)))
    dirs = q.T.astype(np.float32)
    chain = B.PoseChain()
    with_flush, without, flushes = [], [], 0
    for f in range(a.frames):
        rgb, depth, poses = synth.make_frames(100 + f, 1, H, W, "room", start_yaw_steps=f)
        k = (f + (np.arange(g)[:, None] // 3) * 5 + np.arange(g)[None, :] // 3) % 24
        tok = (dirs[k] * rs.uniform(0.5, 2.0, (g, g, 1)) + 0.003 * rs.standard_normal((g, g, D))).astype(np.float32)[None]
        T = np.stack([chain.pc_transform(p) for p in poses])
        idx = torch.from_numpy(np.sort(rs.choice(H * W, P, replace=False)).astype(np.int32)).cuda()
        args = (torch.from_numpy(depth).cuda(), torch.from_numpy(rgb).cuda(), torch.from_numpy(tok).cuda(), T)
        eng.sync()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.ingest(*args, sample_idx=idx, offsets=[0, P])
        eng.sync()
        ms = (time.perf_counter() - t0) * 1e3
        n = eng.counters()["flushes"]
        (with_flush if n > flushes else without).append(ms)
        flushes = n
    usage = eng.store_usage()
    auto = eng.compact_stats()
    loc = {}
    for nq in (1, 256):
        qv = torch.from_numpy((dirs[np.arange(nq) % 24] + 0.01 * rs.standard_normal((nq, D))).astype(np.float32)).cuda()
        eng.localize(qv, K=100)                     # name ranks, scales, scratch
        ts = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng.localize(qv, K=100)
            ts.append((time.perf_counter() - t0) * 1e3)
        loc[nq] = float(np.median(ts))
    t0 = time.perf_counter()
    before, after = eng.compact_store()
    compact_ms = (time.perf_counter() - t0) * 1e3
    final_moved = eng.compact_stats()["rows_moved"] - auto["rows_moved"]
    base = float(np.median(without)) if without else 0.0
    flush_ms = float(np.sum(with_flush) - base * len(with_flush)) if with_flush else None
    print(json.dumps(dict(
        compact=os.environ.get("BSC_STORE_COMPACT", "auto"), frames=a.frames, flushes=flushes,
        ms_per_auto_flush=flush_ms / flushes if flushes else None,
        ms_per_auto_flush_without_compaction=(flush_ms - auto["ms"]) / flushes if flushes else None, ingest_ms_without_flush=base,
        pool_rows=usage["pool_rows"], live_rows=usage["live_rows"], capacity=usage["capacity"],
        auto_compactions=auto["compactions"], auto_compact_rows_moved=auto["rows_moved"], auto_compact_ms=auto["ms"],
        final_compact_ms=compact_ms, final_compact_rows_moved=final_moved, final_compact_rows_freed=before - after,
        localize_ms_q1=loc[1], localize_ms_q256=loc[256])))
    eng.close()


if __name__ == "__main__":
    main()
