"""Inputs and expectations shared by tests/test_gpu_flush_policy.py: mini frames of tests/golden/synth.py with tokens handed in
(directions of surprise_cases.Tokens, so that no decision of the surprise policy sits near a threshold), and what a memory whose
automatic flush follows a policy must hold after ingest calls — computed from the list of passing rows and the replay.

NumPy only.  The automatic flush (memory_2.py:880-886): rows fill the cache in order; with a cache of n rows the passing point
number k (n + 1) + n of the stream finds it full, triggers flush k over the rows [k (n + 1), k (n + 1) + n) and loses its own
token; the next row is cache row 0."""
import numpy as np

import surprise_cases as SC
import surprise_replay as R
import synth

H, W, G, GS, CELL, FLOOR, TOP = 48, 64, 16, 128, 0.1, -2.0, 4.4      # the geometry of the smoke run
F, PER_FRAME, ND, CS = 6, 500, 6, 3
STHR, BTHR = 0.5, 0.95


def frames(D, seed=21):
    """depth (F,H,W) f32, rgb (F,H,W,4) u8, tokens (F,G,G,D) f32, poses (F,7), sample indices (F*PER_FRAME,) i32, offsets.
    The direction of a patch follows its 4 x 4 block and the frame, so a voxel seen again meets another direction."""
    rs = np.random.RandomState(seed)
    rgb, depth, poses = synth.make_frames(seed, F, H, W, "room")
    tok = SC.Tokens(rs, ND, D)
    k = (np.arange(F)[:, None, None] + (np.arange(G)[None, :, None] // 4) * 2 + np.arange(G)[None, None, :] // 4) % ND
    tokens = tok.many(k.reshape(-1)).reshape(F, G, G, D)
    rs_idx = np.random.RandomState(seed + 1)                 # its own stream: the same pixels for every token_dim
    idx = np.concatenate([np.sort(rs_idx.choice(H * W, PER_FRAME, replace=False)) for _ in range(F)]).astype(np.int32)
    off = (np.arange(F + 1) * PER_FRAME).astype(np.int64)
    return depth, rgb, tokens, poses, idx, off


def chunks(P, n):
    """(number of automatic flushes, rows left in the cache) after P passing rows through a cache of n rows."""
    m = P // (n + 1)
    return m, P - m * (n + 1)


def replay_stream(st, rows, n, radius, sthr=STHR, bthr=BTHR, cs=CS):
    """The surprise policy as the automatic flush over the passing rows (feat, pos, dis) on the store st (in place), the cache
    being empty at the first row.  -> (flushes, rows left, path counts, margins)."""
    feat, pos, dis = rows
    counts = dict.fromkeys(R.PATHS, 0)
    margins = {"surprise": np.inf, "boring": np.inf, "argmin": np.inf}
    m, rem = chunks(len(pos), n)
    for k in range(m):
        a = k * (n + 1)
        c, g = R.replay(st, pos[a:a + n], feat[a:a + n], dis[a:a + n], radius, sthr, bthr, cs)
        counts = {p: counts[p] + c[p] for p in counts}
        margins = {p: min(margins[p], g[p]) for p in margins}
    return m, rem, counts, margins
