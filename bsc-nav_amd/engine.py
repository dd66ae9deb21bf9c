"""VoxelEngine — thin Python handle on one libbscnav context (one GPU).

All arithmetic of the path runs in the HIP library; this class only marshals torch device tensors
(raw data_ptr) and NumPy host buffers across the C-ABI of include/bscnav.h.
"""
import ctypes as C
import random

import numpy as np
import torch

from . import _lib
from .geometry import cam_mat_fov, cam_mat_patch


def _hp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _dp(t):
    return None if t is None else C.c_void_p(t.data_ptr())


REGION_DTYPE = np.dtype([("radius", np.float64), ("curr", np.int32, (3,)), ("floor_lo", np.int32), ("floor_hi", np.int32),
                         ("reserved", np.int32)])          # struct bsc_region
assert REGION_DTYPE.itemsize == C.sizeof(_lib.BscRegion) == 32


def region_array(Q, radius=None, curr=None, floor=None):
    """The (Q,) bsc_region array of VoxelEngine.localize_regions from its arguments (needs no context):
    radius  None (no sphere for anyone), one number for all, or a sequence of Q numbers / Nones (None and inf: no sphere);
    curr    (3,) for all or (Q,3); may be None only when no query has a sphere;
    floor   None (no band for anyone), one (lo, hi) pair for all, or a sequence of Q pairs / Nones.
    A sequence of the wrong length raises ValueError."""
    Q = int(Q)
    out = np.zeros(Q, REGION_DTYPE)
    if radius is None or np.isscalar(radius):
        radius = [radius] * Q
    radius = list(radius)
    if len(radius) != Q:
        raise ValueError(f"radius: {len(radius)} entries for {Q} queries")
    out["radius"] = [-1.0 if (r is None or r == np.inf) else float(r) for r in radius]
    if curr is None:
        if np.any(~(out["radius"] < 0)):
            raise ValueError("a sphere (radius) needs curr")
    else:
        c = np.asarray(curr)
        if c.shape == (3,):
            c = np.broadcast_to(c, (Q, 3))
        if c.shape != (Q, 3):
            raise ValueError(f"curr: shape {c.shape}, expected (3,) or ({Q}, 3)")
        out["curr"] = c.astype(np.int32)
    if floor is None:
        floor = [None] * Q
    elif len(floor) == 2 and all(np.isscalar(v) for v in floor):
        floor = [floor] * Q
    floor = list(floor)
    if len(floor) != Q:
        raise ValueError(f"floor: {len(floor)} entries for {Q} queries")
    for i, f in enumerate(floor):
        if f is not None and len(f) != 2:
            raise ValueError(f"floor[{i}]: expected (lo, hi) or None")
        out["floor_lo"][i], out["floor_hi"][i] = (0, -1) if f is None else (int(f[0]), int(f[1]))
    return out


def score_map_regions(Q, radius=None, curr=None, floor=None):
    """The regions argument of VoxelEngine.score_map (needs no context): None — a NULL pointer, no region for any query — when
    radius, curr and floor are all None, otherwise region_array's (Q,) array."""
    if radius is None and curr is None and floor is None:
        return None
    return region_array(Q, radius, curr, floor)


BAND_DTYPE = np.dtype([("lo", np.int32), ("hi", np.int32)])          # struct bsc_band
assert BAND_DTYPE.itemsize == C.sizeof(_lib.BscBand) == 8
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


def band_array(bands=None):
    """The (S,) bsc_band array of VoxelEngine.topdown_slices from its argument (needs no context): None — a NULL pointer, one
    open band — or a sequence of (lo, hi) pairs / Nones, None being an open band (lo > hi: every height).  One (lo, hi) pair of
    numbers is one band.  Bounds beyond int32 are clamped to it; an entry that is no pair raises ValueError (an empty sequence gives
    an empty array, which the library refuses like more than 256 bands)."""
    if bands is None:
        return None
    bands = list(bands)
    if len(bands) == 2 and all(np.isscalar(v) for v in bands):
        bands = [tuple(bands)]
    out = np.zeros(len(bands), BAND_DTYPE)
    for i, b in enumerate(bands):
        if b is not None and len(b) != 2:
            raise ValueError(f"bands[{i}]: expected (lo, hi) or None")
        lo, hi = (0, -1) if b is None else (int(b[0]), int(b[1]))
        out["lo"][i], out["hi"][i] = min(max(lo, INT32_MIN), INT32_MAX), min(max(hi, INT32_MIN), INT32_MAX)
    return out


def pad_cluster_batch(pos, sim, counts=None):
    """The (pos (Q,K,3) int32, sim (Q,K) float32, counts (Q,) int32) arrays of VoxelEngine.cluster_centers_batch from its
    arguments (needs no context).  pos / sim are either arrays of those shapes, with counts (None: K points each, otherwise
    0 .. K), or sequences of Q per-query arrays (n_i,3) / (n_i,) of different lengths, which are padded to the longest
    (at least 1) with position 0 and similarity 0; counts must then be None.  Lengths that do not agree raise ValueError."""
    ragged = not (isinstance(pos, np.ndarray) and pos.ndim == 3)
    if ragged:
        if counts is not None:
            raise ValueError("counts: per-query arrays carry their own lengths")
        pos = [np.asarray(p, np.int32).reshape(-1, 3) for p in pos]
        sim = [np.asarray(s, np.float32).reshape(-1) for s in sim]
        if len(pos) != len(sim):
            raise ValueError(f"{len(pos)} position arrays for {len(sim)} similarity arrays")
        if len(pos) == 0:
            raise ValueError("no query")
        for i, (p, s) in enumerate(zip(pos, sim)):
            if len(p) != len(s):
                raise ValueError(f"query {i}: {len(p)} positions for {len(s)} similarities")
        cnt = np.array([len(p) for p in pos], np.int32)
        Q, K = len(pos), max(1, int(cnt.max()))
        P, S = np.zeros((Q, K, 3), np.int32), np.zeros((Q, K), np.float32)
        for i in range(Q):
            P[i, :cnt[i]] = pos[i]
            S[i, :cnt[i]] = sim[i]
        return P, S, cnt
    P = np.ascontiguousarray(pos, np.int32)
    S = np.ascontiguousarray(sim, np.float32)
    if P.shape[2] != 3 or S.shape != P.shape[:2]:
        raise ValueError(f"pos {P.shape} / sim {S.shape}: expected (Q,K,3) / (Q,K)")
    Q, K = S.shape
    if Q < 1 or K < 1:
        raise ValueError(f"pos {P.shape}: no query or no point")
    cnt = np.full(Q, K, np.int32) if counts is None else np.ascontiguousarray(counts, np.int32).reshape(-1)
    if len(cnt) != Q:
        raise ValueError(f"counts: {len(cnt)} entries for {Q} queries")
    if np.any(cnt < 0) or np.any(cnt > K):
        raise ValueError(f"counts outside 0..{K}")
    return P, S, cnt


class VoxelEngine:
    def __init__(self, height, width, grid_size, cell_size, floor_height, map_height, patch_grid, token_dim,
                 mode="exact", iter_size=50000, cache_size=10, voxel_capacity=None, token_capacity=None,
                 max_points=None, device=0, fov=90, min_depth=0.1, max_depth=10, min_h=None, max_h=None):
        if not torch.cuda.is_available():
            raise RuntimeError("bsc_nav_amd needs a ROCm GPU (MI355X / gfx950); there is no CPU path")
        self.lib = _lib.load()
        c = _lib.BscConfig()
        c.height, c.width, c.grid_size = int(height), int(width), int(grid_size)
        c.max_h = int(map_height / cell_size) if max_h is None else int(max_h)      # memory_2.py:122
        c.min_h = int(floor_height / cell_size) if min_h is None else int(min_h)    # memory_2.py:123
        c.patch_grid, c.token_dim = int(patch_grid), int(token_dim)
        c.iter_size, c.cache_size, c.mode = int(iter_size), int(cache_size), _lib.MODES[mode]
        c.voxel_capacity = int(voxel_capacity or int(grid_size) * int(grid_size))   # memory_2.py:715
        c.max_points = int(max_points or height * width)
        c.token_capacity = int(token_capacity or (c.voxel_capacity * 2 + iter_size)) if mode == "exact" else 0
        c.cell_size, c.min_depth, c.max_depth = float(cell_size), float(min_depth), float(max_depth)
        K = cam_mat_fov(height, width, fov)
        c.K[:] = K.flatten()
        c.Kinv[:] = np.linalg.inv(K).flatten()              # utils.py:164
        c.Kpatch[:] = cam_mat_patch(patch_grid, patch_grid).flatten()
        self.cfg = c
        self.mode = mode
        self.device = torch.device("cuda", device)
        self.nh = c.max_h - c.min_h
        torch.cuda.set_device(self.device)
        # The library launches on the stream that is current NOW; calls made later under another torch stream are
        # ordered against it in _enter() (see there).
        self.stream = torch.cuda.current_stream(self.device)
        h = C.c_void_p()
        _lib.check(self.lib.bsc_create(C.byref(c), device, C.c_void_p(self.stream.cuda_stream), C.byref(h)))
        self.h = h
        self.log_capacity = 0
        self._last_localize = None      # (Q, K, counts) of the last localize call: its results stay on the GPU for clustering
        self._draw = _lib.DRAW_FN(self._draw_cb)
        self._no_draw = _lib.DRAW_FN()    # NULL: what ingest hands over under the surprise policy, which never draws
        self._flush_policy = "dist"

    # memory_2.py:352 — Python's global RNG, one draw per row that meets a full voxel
    def _draw_cb(self, user, n, out):
        k = self.cfg.cache_size
        if n < 64:
            for i in range(n):
                out[i] = random.choice(range(k))
            return
        # many draws (saturated voxels): the same stream, advanced by the library's restatement of random.choice
        version, internal, gauss = random.getstate()
        key = np.array(internal[:624], dtype=np.uint32)
        pos = C.c_int32(internal[624])
        _lib.check(self.lib.bsc_host_choice_draws(key.ctypes.data_as(C.c_void_p), C.byref(pos), k, n,
                                                  C.cast(out, C.c_void_p)))
        random.setstate((version, tuple(key.tolist()) + (pos.value,), gauss))

    def _enter(self, *tensors):
        """Order the library stream after the caller's current stream and pin the inputs to it: when the caller works
        under a different torch stream than the one the engine was created on, the kernels must not start before
        the producers of `tensors` have finished, and the caching allocator must not hand their blocks out again
        while the library is still reading them."""
        cur = torch.cuda.current_stream(self.device)
        if cur != self.stream:
            self.stream.wait_stream(cur)
            for t in tensors:
                if t is not None:
                    t.record_stream(self.stream)

    def _leave(self):
        """Results written by the library (device outputs) become visible to the caller's current stream."""
        cur = torch.cuda.current_stream(self.device)
        if cur != self.stream:
            cur.wait_stream(self.stream)

    def close(self):
        if getattr(self, "h", None):
            self.lib.bsc_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self):
        _lib.check(self.lib.bsc_reset(self.h))

    def stream_wait_chain(self, stream):
        """`stream` (torch.cuda.Stream) waits on the GPU for the rgb chain kernels launched so far."""
        _lib.check(self.lib.bsc_stream_wait_chain(self.h, C.c_void_p(stream.cuda_stream)))

    def sync(self):
        """Everything ingest() has started or deferred (the rgb chain of the last call is launched lazily) is complete."""
        _lib.check(self.lib.bsc_sync(self.h))

    def ingest(self, depth, rgb, tokens, transforms, sample_idx=None, offsets=None, alpha=None):
        """depth (F,H,W) f32, rgb (F,H,W,C) u8, tokens (F,g,g,D) f32 or bf16 (widened exactly): contiguous CUDA
        tensors.  transforms (F,4,4) float64 NumPy.  sample_idx int32 CUDA + offsets (F+1) int64 NumPy, or None."""
        F = depth.shape[0] if depth.dim() == 3 else 1
        assert depth.is_cuda and rgb.is_cuda and tokens.is_cuda
        assert depth.dtype == torch.float32 and rgb.dtype == torch.uint8 and tokens.dtype in (torch.float32, torch.bfloat16)
        assert depth.is_contiguous() and rgb.is_contiguous() and tokens.is_contiguous()
        T = np.ascontiguousarray(np.asarray(transforms, dtype=np.float64).reshape(F, 16))
        off = None if offsets is None else np.ascontiguousarray(offsets, dtype=np.int64)
        if sample_idx is not None:
            assert sample_idx.is_cuda and sample_idx.dtype == torch.int32 and off is not None and len(off) == F + 1
        if alpha is not None:
            assert alpha.is_cuda and alpha.dtype == torch.float64
        self._enter(depth, rgb, tokens, sample_idx, alpha)
        _lib.check(self.lib.bsc_ingest_typed(self.h, F, _dp(depth), _dp(rgb), rgb.shape[-1], _dp(tokens),
                                             1 if tokens.dtype == torch.bfloat16 else 0, _hp(T), _dp(sample_idx),
                                             _hp(off), _dp(alpha),
                                             self._draw if self._flush_policy == "dist" else self._no_draw, None))

    def flush(self):
        _lib.check(self.lib.bsc_flush(self.h, self._draw, None))

    def flush_surprise(self, radius=1, surprise_threshold=0.5, boring_threshold=0.95):
        """update_memory_surp_base (memory_2.py:364-536) over every cache row; exact mode only."""
        _lib.check(self.lib.bsc_flush_surprise(self.h, int(radius), float(surprise_threshold), float(boring_threshold)))

    def set_flush_policy(self, policy="dist", radius=1, surprise_threshold=0.5, boring_threshold=0.95):
        """The flush ingest() runs when a passing point meets a full cache (memory_2.py:880-881): "dist"
        (update_memory_dist_base, the default) or "surprise" (update_memory_surp_base with these three parameters, no draws).
        Exact mode only; kept across reset(); a refused call leaves the previous policy in place."""
        if policy not in _lib.FLUSH_POLICIES:
            raise ValueError(f"flush policy {policy!r}: expected one of {sorted(_lib.FLUSH_POLICIES)}")
        _lib.check(self.lib.bsc_set_flush_policy(self.h, _lib.FLUSH_POLICIES[policy], int(radius), float(surprise_threshold),
                                                 float(boring_threshold)))
        self._flush_policy = policy

    def store_usage(self):
        """dict(pool_rows, live_rows, capacity): token-pool rows in use, rows some voxel's group still refers to, rows
        allocated (exact mode).  pool_rows > live_rows after merges of the surprise policy, until the store is compacted."""
        out = np.zeros(3, np.int64)
        _lib.check(self.lib.bsc_store_usage(self.h, _hp(out)))
        return dict(pool_rows=int(out[0]), live_rows=int(out[1]), capacity=int(out[2]))

    def compact_store(self):
        """Move the live token rows to the front of the pool (bsc_compact_store) -> (pool rows before, after)."""
        before, after = C.c_int64(), C.c_int64()
        _lib.check(self.lib.bsc_compact_store(self.h, C.byref(before), C.byref(after)))
        return before.value, after.value

    def compact_stats(self):
        """dict(compactions, rows_moved, ms): compactions since the engine was created that moved rows — explicit and automatic
        ones —, the rows they moved and the host time they took."""
        out = np.zeros(3, np.int64)
        _lib.check(self.lib.bsc_compact_stats(self.h, _hp(out)))
        return dict(compactions=int(out[0]), rows_moved=int(out[1]), ms=out[2] / 1e3)

    def counters(self):
        out = np.zeros(10, np.int64)
        _lib.check(self.lib.bsc_counters(self.h, _hp(out)))
        keys = ["max_id", "iter_id", "store_voxels", "store_tokens", "flushes", "points_passed", "points_seen",
                "voxel_rmw", "pairs", "pairs_last_call"]
        return {k: int(v) for k, v in zip(keys, out)}

    def geometry(self, depth, transform, sample_idx=None):
        P = depth.numel() if sample_idx is None else sample_idx.numel()
        o = dict(flags=np.zeros(P, np.uint8), pc=np.zeros((P, 3)), pg=np.zeros((P, 3)), vox=np.zeros((P, 3), np.int32),
                 pix=np.zeros((P, 2), np.int32), pat=np.zeros((P, 2), np.int32), r2=np.zeros(P), alpha=np.zeros(P))
        T = np.ascontiguousarray(np.asarray(transform, np.float64).reshape(16))
        _lib.check(self.lib.bsc_geometry(self.h, _dp(depth), _hp(T), _dp(sample_idx), P, _hp(o["flags"]), _hp(o["pc"]),
                                         _hp(o["pg"]), _hp(o["vox"]), _hp(o["pix"]), _hp(o["pat"]), _hp(o["r2"]),
                                         _hp(o["alpha"])))
        return o

    def sort_pairs_u32(self, keys, vals, begin_bit=0, end_bit=32):
        """The library's stable radix sort of (u32 key, u32 value) pairs on the key bits [begin_bit, end_bit): int32 CUDA tensors
        (bit patterns) in, sorted copies out."""
        ko, vo = torch.empty_like(keys), torch.empty_like(vals)
        _lib.check(self.lib.bsc_sort_pairs_u32(self.h, _dp(keys), _dp(vals), keys.numel(), begin_bit, end_bit, _dp(ko), _dp(vo)))
        return ko, vo

    # ---- exports / imports -------------------------------------------------------------------
    def export_rgb(self):
        n = self.counters()["max_id"]
        pos, rgb, w = np.zeros((n, 3), np.int32), np.zeros((n, 3), np.uint8), np.zeros(n, np.float32)
        _lib.check(self.lib.bsc_export_rgb(self.h, _hp(pos), _hp(rgb), _hp(w)))
        return pos, rgb, w

    def export_occupied(self):
        occ = np.zeros((self.cfg.grid_size, self.cfg.grid_size, self.nh), np.int32)
        _lib.check(self.lib.bsc_export_occupied(self.h, _hp(occ)))
        return occ

    def export_heightmap(self):
        gs = self.cfg.grid_size
        mh, cv = np.zeros((gs, gs), np.float64), np.zeros((gs, gs, 3), np.uint8)
        _lib.check(self.lib.bsc_export_heightmap(self.h, _hp(mh), _hp(cv)))
        return mh, cv

    def export_cache(self):
        n = self.counters()["iter_id"]
        f, p, d = np.zeros((n, self.cfg.token_dim), np.float32), np.zeros((n, 3), np.int32), np.zeros(n, np.float32)
        _lib.check(self.lib.bsc_export_cache(self.h, _hp(f), _hp(p), _hp(d)))
        return f, p, d

    def export_store(self):
        c = self.counters()
        V, T = c["store_voxels"], c["store_tokens"]
        pos, cnt = np.zeros((V, 3), np.int32), np.zeros(V, np.int32)
        feats, dists = np.zeros((T, self.cfg.token_dim), np.float32), np.zeros(T, np.float32)
        _lib.check(self.lib.bsc_export_store(self.h, _hp(pos), _hp(cnt), _hp(feats), _hp(dists)))
        return pos, cnt, feats, dists

    def export_dense(self):
        n = self.counters()["max_id"]
        acc, cnt = np.zeros((n, self.cfg.token_dim), np.float32), np.zeros(n, np.int32)
        _lib.check(self.lib.bsc_export_dense(self.h, _hp(acc), _hp(cnt)))
        return acc, cnt

    def import_rgb(self, pos, rgb, weight):
        pos = np.ascontiguousarray(pos, np.int32)
        rgb = np.ascontiguousarray(rgb, np.uint8)
        weight = np.ascontiguousarray(weight, np.float32)
        _lib.check(self.lib.bsc_import_rgb(self.h, len(pos), _hp(pos), _hp(rgb), _hp(weight)))

    def import_store(self, pos, cnt, feats, dists):
        pos = np.ascontiguousarray(pos, np.int32)
        cnt = np.ascontiguousarray(cnt, np.int32)
        feats = np.ascontiguousarray(feats, np.float32)
        dists = np.ascontiguousarray(dists, np.float32)
        _lib.check(self.lib.bsc_import_store(self.h, len(pos), len(feats), _hp(pos), _hp(cnt), _hp(feats), _hp(dists)))

    def import_cache(self, pos, feat, dis):
        """Counterpart of export_cache: rows 0 .. n-1 of the token cache (every cell must hold a voxel, [0,0,0] excepted)."""
        pos = np.ascontiguousarray(pos, np.int32).reshape(-1, 3)
        feat = np.ascontiguousarray(feat, np.float32).reshape(len(pos), self.cfg.token_dim)
        dis = np.ascontiguousarray(dis, np.float32).reshape(len(pos))
        _lib.check(self.lib.bsc_import_cache(self.h, len(pos), _hp(pos), _hp(feat), _hp(dis)))

    def import_dense(self, acc, cnt):
        acc = np.ascontiguousarray(acc, np.float32)
        cnt = np.ascontiguousarray(cnt, np.int32)
        _lib.check(self.lib.bsc_import_dense(self.h, len(cnt), _hp(acc), _hp(cnt)))

    # ---- query ------------------------------------------------------------------------------------
    def pool_query(self, tokens):
        """tokens (B,T,D) f32 CUDA -> (D) f32 CUDA   (memory_2.py:591-608)"""
        assert tokens.is_cuda and tokens.dtype == torch.float32 and tokens.is_contiguous()
        B, T, D = tokens.shape
        out = torch.empty(D, dtype=torch.float32, device=tokens.device)
        self._enter(tokens, out)
        _lib.check(self.lib.bsc_pool_query(self.h, _dp(tokens), B, T, D, _dp(out)))
        self._leave()
        return out

    def localize(self, q, K=100, radius=None, curr=None, floor=None):
        """q (Q,D) or (D) f32 CUDA -> (pos (Q,n,3) int32, sim (Q,n) f32, counts)."""
        q = q.reshape(-1, self.cfg.token_dim).contiguous()
        assert q.is_cuda and q.dtype == torch.float32
        Q = q.shape[0]
        pos, sim, cnt = np.zeros((Q, K, 3), np.int32), np.zeros((Q, K), np.float32), np.zeros(Q, np.int32)
        curr_a = None if curr is None else np.ascontiguousarray(curr, np.int32)
        lo, hi = (0, -1) if floor is None else (int(floor[0]), int(floor[1]))
        self._enter(q)
        _lib.check(self.lib.bsc_localize(self.h, _dp(q), Q, K, -1.0 if radius is None else float(radius), _hp(curr_a),
                                         lo, hi, _hp(pos), _hp(sim), _hp(cnt)))
        self._last_localize = (Q, K, cnt.copy())
        return pos, sim, cnt

    def localize_regions(self, q, K=100, radius=None, curr=None, floor=None):
        """localize with a sphere and a floor band per query, in one call (bsc_localize_regions): q (Q,D) f32 CUDA;
        radius a sequence of Q floats / Nones or one value for all; curr (Q,3) or (3,); floor a sequence of (lo, hi) / None
        or one (lo, hi) for all -> the triple of localize.  Only the rows some query can see are scanned when they are few."""
        q = q.reshape(-1, self.cfg.token_dim).contiguous()
        assert q.is_cuda and q.dtype == torch.float32
        Q = q.shape[0]
        regions = region_array(Q, radius, curr, floor)
        pos, sim, cnt = np.zeros((Q, K, 3), np.int32), np.zeros((Q, K), np.float32), np.zeros(Q, np.int32)
        self._enter(q)
        _lib.check(self.lib.bsc_localize_regions(self.h, _dp(q), Q, K, _hp(regions), _hp(pos), _hp(sim), _hp(cnt)))
        self._last_localize = (Q, K, cnt.copy())
        return pos, sim, cnt

    def score_map(self, q, radius=None, curr=None, floor=None, heights=True):
        """The best score per top-down cell for every query (bsc_score_map): q (Q,D) or (D) f32 CUDA; radius / curr / floor
        as in localize_regions (all three None: no region for any query)
        -> (score (Q,gs,gs) f32 CUDA, height (Q,gs,gs) i32 CUDA or None when heights is False).
        score[i,r,c] is the largest score among the voxels of column (r,c) that localize_regions would rank for query i, with
        the bits it has there (-inf: none); height[i,r,c] the stored h of the voxel that has it, the smallest h among equals
        (-1: none).  The resident results of the last localize call are untouched."""
        q = q.reshape(-1, self.cfg.token_dim).contiguous()
        assert q.is_cuda and q.dtype == torch.float32
        Q, gs = q.shape[0], self.cfg.grid_size
        regions = score_map_regions(Q, radius, curr, floor)
        score = torch.empty((Q, gs, gs), dtype=torch.float32, device=q.device)
        height = torch.empty((Q, gs, gs), dtype=torch.int32, device=q.device) if heights else None
        self._enter(q, score, height)
        _lib.check(self.lib.bsc_score_map(self.h, _dp(q), Q, _hp(regions), _dp(score), _dp(height)))
        self._leave()
        return score, height

    def topdown_slices(self, bands=None, heights=True, counts=True):
        """Top-down maps of height bands from the stored voxels (bsc_topdown_slices): bands a list of (lo, hi) — stored heights
        lo <= h <= hi, None or lo > hi: every height — or None for one open band
        -> dict(rgb (S,gs,gs,3) u8, height (S,gs,gs) i32, count (S,gs,gs) i32) of CUDA tensors; height / count are None when
        heights / counts is False.  rgb[s,r,c] is grid_rgb of the highest stored voxel of column (r,c) inside band s (zeros: none),
        height its h (-1: none), count the stored voxels of the column inside the band.  The resident cv_map / max_height and the
        results of the last localize call are untouched."""
        arr = band_array(bands)
        S, gs = 1 if arr is None else len(arr), self.cfg.grid_size
        rgb = torch.empty((S, gs, gs, 3), dtype=torch.uint8, device=self.device)
        height = torch.empty((S, gs, gs), dtype=torch.int32, device=self.device) if heights else None
        count = torch.empty((S, gs, gs), dtype=torch.int32, device=self.device) if counts else None
        self._enter(rgb, height, count)
        _lib.check(self.lib.bsc_topdown_slices(self.h, S, _hp(arr), _dp(rgb), _dp(height), _dp(count)))
        self._leave()
        return dict(rgb=rgb, height=height, count=count)

    def rebuild_topdown(self, band=None):
        """The slice of `band` ((lo, hi); None: every height) becomes the resident top-down state (bsc_topdown_rebuild): cv_map
        the slice colours, max_height the slice heights (-inf: none) with tie order 0 as after import_heightmap — what
        export_heightmap, frontier_mask and frontier_clusters read, and what a later ingest continues from."""
        b = band_array([band])[0]
        _lib.check(self.lib.bsc_topdown_rebuild(self.h, int(b["lo"]), int(b["hi"])))

    def render_views(self, transforms, size=None, kinv=None, band=None, t_range=None, want=("voxel", "depth", "rgb")):
        """The stored voxels seen from camera poses (bsc_render_views): transforms (V,4,4) or (4,4) f64, camera to map, as ingest
        takes them; size (H, W), None: the context's frame size; kinv the (3,3) inverse intrinsics with last row [0,0,1], None: the
        context's own; band (lo, hi) stored heights, None: every height; t_range (t_min, t_max) along the ray, in depth units,
        None: the configuration's (min_depth, max_depth)
        -> dict(voxel (V,H,W) i32, depth (V,H,W) f32, rgb (V,H,W,3) u8) of CUDA tensors, None for what `want` does not name.
        Per pixel the first stored voxel the ray meets: its id (-1: none), the depth where the ray enters its cell (0: none) and
        grid_rgb of it (zeros: none)."""
        T = np.ascontiguousarray(np.asarray(transforms, np.float64).reshape(-1, 16))
        V = len(T)
        H, W = (self.cfg.height, self.cfg.width) if size is None else (int(size[0]), int(size[1]))
        kinv = None if kinv is None else np.ascontiguousarray(np.asarray(kinv, np.float64).reshape(9))
        arr = band_array(None if band is None else [band])
        t_min, t_max = (self.cfg.min_depth, self.cfg.max_depth) if t_range is None else (float(t_range[0]), float(t_range[1]))
        unknown = set(want) - {"voxel", "depth", "rgb"}
        if unknown:
            raise ValueError(f"want: {sorted(unknown)} (voxel, depth, rgb)")
        shape = (V, max(H, 0), max(W, 0))                         # (a size the library refuses still reaches it)
        voxel = torch.empty(shape, dtype=torch.int32, device=self.device) if "voxel" in want else None
        depth = torch.empty(shape, dtype=torch.float32, device=self.device) if "depth" in want else None
        rgb = torch.empty(shape + (3,), dtype=torch.uint8, device=self.device) if "rgb" in want else None
        self._enter(voxel, depth, rgb)
        _lib.check(self.lib.bsc_render_views(self.h, V, _hp(T), _hp(kinv), H, W, t_min, t_max, _hp(arr), _dp(voxel), _dp(depth),
                                             _dp(rgb)))
        self._leave()
        return dict(voxel=voxel, depth=depth, rgb=rgb)

    def cluster_centers(self, pos=None, sim=None, K=None, query_index=0, eps=10.0, min_samples=5):
        """BSCAgent.weighted_cluster_centers on the GPU -> (centers (n,3) f64, labels (K,) int, sizes list).
        pos/sim None: cluster the first K results of query `query_index` of the last localize call (no host copy)."""
        if pos is not None:
            pos = np.ascontiguousarray(pos, np.int32)
            sim = np.ascontiguousarray(sim, np.float32)
            K = len(pos)
        centers, labels, sizes = np.zeros((K, 3), np.float64), np.zeros(K, np.int32), np.zeros(K, np.int32)
        n = np.zeros(1, np.int32)
        _lib.check(self.lib.bsc_cluster_centers(self.h, query_index, K, _hp(pos), _hp(sim), float(eps), int(min_samples),
                                                _hp(centers), _hp(labels), _hp(sizes), _hp(n)))
        return centers[:n[0]], labels.astype(np.int64), [int(v) for v in sizes[:n[0]]]

    def cluster_centers_batch(self, pos=None, sim=None, counts=None, K=None, eps=10.0, min_samples=5):
        """cluster_centers for every query of a batch in one call (bsc_cluster_centers_batch) -> one
        (centers (n,3) f64, labels (n_i,) int64, sizes list) per query.
        pos / sim None: the results of the last localize / localize_regions call, still on the GPU (no host copy); K
        (default: that call's K) and counts (default: what each query found, at most K) narrow them.
        Otherwise pos (Q,K,3) / sim (Q,K) arrays with counts (Q,) (None: K points each), or lists of per-query arrays of
        different lengths, padded here (see pad_cluster_batch); a query without points gives no clusters."""
        if (pos is None) != (sim is None):
            raise ValueError("pos and sim go together (both None: the resident results of the last localize call)")
        if pos is None:
            if self._last_localize is None:
                raise _lib.BscError("cluster_centers_batch: no localize call whose results could be clustered")
            Q, last_K, last_cnt = self._last_localize
            K = last_K if K is None else int(K)
            cnt = np.minimum(last_cnt, K).astype(np.int32) if counts is None else np.ascontiguousarray(counts, np.int32)
            counts_arg = None if counts is None else cnt
        else:
            pos, sim, cnt = pad_cluster_batch(pos, sim, counts)
            Q, K = sim.shape
            counts_arg = cnt
        if len(cnt) != Q:
            raise ValueError(f"counts: {len(cnt)} entries for {Q} queries")
        centers, labels = np.zeros((Q, K, 3), np.float64), np.full((Q, K), -1, np.int32)
        sizes, ncl = np.zeros((Q, K), np.int32), np.zeros(Q, np.int32)
        _lib.check(self.lib.bsc_cluster_centers_batch(self.h, Q, K, _hp(counts_arg), _hp(pos), _hp(sim), float(eps),
                                                      int(min_samples), _hp(centers), _hp(labels), _hp(sizes), _hp(ncl)))
        return [(centers[i, :ncl[i]].copy(), labels[i, :cnt[i]].astype(np.int64), [int(v) for v in sizes[i, :ncl[i]]])
                for i in range(Q)]

    # ---- FrontierExplorer helpers (memory_2.py:1147-1311) ----------------------------------------------
    def frontier_mask(self, navigable=None):
        """(gs,gs) u8: bit0 known (cv_map.sum(-1) != 0), bit1 frontier (known, navigable, an unknown 4-neighbour)."""
        gs = self.cfg.grid_size
        nav = None if navigable is None else np.ascontiguousarray(np.asarray(navigable) != 0, np.uint8)
        mask = np.zeros((gs, gs), np.uint8)
        _lib.check(self.lib.bsc_frontier_mask(self.h, _hp(nav), _hp(mask)))
        return mask

    def frontier_clusters(self, frontier=None, min_cluster_size=10, ig_radius=5, max_clusters=4096, labels=True):
        """4-connected frontier clusters in the reference's order -> dict(n, first, sizes, centers, gains, best, labels).
        frontier (gs,gs) nonzero = frontier cell; None = the cells of the last frontier_mask call."""
        gs = self.cfg.grid_size
        fr = None if frontier is None else np.ascontiguousarray(np.asarray(frontier) != 0, np.uint8)
        cap = int(max_clusters)
        n, best = np.zeros(1, np.int32), np.zeros(1, np.int32)
        lab = np.zeros((gs, gs), np.int32) if labels else None
        first, sizes = np.zeros((cap, 2), np.int32), np.zeros(cap, np.int32)
        centers, gains = np.zeros((cap, 2), np.float64), np.zeros(cap, np.float64)
        _lib.check(self.lib.bsc_frontier_clusters(self.h, _hp(fr), int(min_cluster_size), int(ig_radius), cap, _hp(n),
                                                  _hp(lab), _hp(first), _hp(sizes), _hp(centers), _hp(gains), _hp(best)))
        m = min(int(n[0]), cap)
        return dict(n=int(n[0]), first=first[:m], sizes=sizes[:m], centers=centers[:m], gains=gains[:m],
                    best=int(best[0]), labels=lab)

    def import_cv_map(self, cv_map):
        cv = np.ascontiguousarray(cv_map, np.uint8)
        assert cv.shape == (self.cfg.grid_size, self.cfg.grid_size, 3)
        _lib.check(self.lib.bsc_import_cv_map(self.h, _hp(cv)))

    def kernel_stats(self, which=0, reset=False):
        """HIP-event time of the dominant kernel: dict(ms, launches, bytes, launches_since_reset)."""
        out = np.zeros(4, np.float64)
        _lib.check(self.lib.bsc_kernel_stats(self.h, which, 1 if reset else 0, _hp(out)))
        return dict(ms=float(out[0]), launches=int(out[1]), bytes=float(out[2]), launches_since_reset=int(out[3]))

    # ---- multi-GPU helpers --------------------------------------------------------------------------
    def keys_tensor(self):
        """(max_id,3) int32 CUDA view of the voxel keys in id order (copy)."""
        ptr, n = C.c_void_p(), C.c_int64()
        _lib.check(self.lib.bsc_keys_dev(self.h, C.byref(ptr), C.byref(n)))
        out = torch.empty((n.value, 3), dtype=torch.int32, device=self.device)
        if n.value:
            pos, _, _ = self.export_rgb()
            out.copy_(torch.from_numpy(pos))
        return out

    def max_height_cv_map(self):
        """(max_height (gs,gs) f64 with -inf for empty cells, cv_map (gs,gs,3) u8) — the top-down map state."""
        return self.export_heightmap()

    def dense_gather(self, keys):
        keys = keys.contiguous()
        n = keys.shape[0]
        acc = torch.empty((n, self.cfg.token_dim), dtype=torch.float32, device=self.device)
        cnt = torch.empty(n, dtype=torch.int32, device=self.device)
        self._enter(keys, acc, cnt)
        _lib.check(self.lib.bsc_dense_gather(self.h, n, _dp(keys), _dp(acc), _dp(cnt)))
        self._leave()
        return acc, cnt

    def dense_gather_rgb(self, keys):
        """rgb (n,3) u8 and weight (n,) f32 of the voxels `keys` (weight 0 where this map has no such voxel)."""
        keys = keys.contiguous()
        n = keys.shape[0]
        rgb = torch.empty((n, 3), dtype=torch.uint8, device=self.device)
        w = torch.empty(n, dtype=torch.float32, device=self.device)
        self._enter(keys, rgb, w)
        _lib.check(self.lib.bsc_dense_gather_rgb(self.h, n, _dp(keys), _dp(rgb), _dp(w)))
        self._leave()
        return rgb, w

    def dense_replace(self, keys, acc, cnt, rgb=None, weight=None):
        """The map becomes exactly these voxels (ids in the given order); rgb / weight None -> zeroed colours."""
        keys, acc, cnt = keys.contiguous(), acc.contiguous(), cnt.contiguous()
        assert keys.dtype == torch.int32 and acc.dtype == torch.float32 and cnt.dtype == torch.int32
        if rgb is not None:
            rgb, weight = rgb.contiguous(), weight.contiguous()
            assert rgb.dtype == torch.uint8 and weight.dtype == torch.float32 and rgb.shape[0] == keys.shape[0]
        self._enter(keys, acc, cnt, rgb, weight)
        _lib.check(self.lib.bsc_dense_replace_full(self.h, keys.shape[0], _dp(keys), _dp(acc), _dp(cnt), _dp(rgb), _dp(weight)))

    # ---- exact colour across ranks: point log + replay (include/bscnav.h bsc_point_log_*, bsc_replay_colour) ----------
    def point_log_enable(self, capacity):
        """Keep (cell, alpha, rgb) of every ingested point — 16 B / point, for the sub-sampled modes; 0 disables."""
        _lib.check(self.lib.bsc_point_log_enable(self.h, int(capacity)))
        self.log_capacity = int(capacity)

    def point_log(self):
        """-> (cells (n,) int32, records (n,3) int32 [alpha lo, alpha hi, rgb]) CUDA copies of the log, order of ingestion."""
        n = C.c_int64()
        _lib.check(self.lib.bsc_point_log_read(self.h, None, None, 0, C.byref(n)))
        cells = torch.empty(n.value, dtype=torch.int32, device=self.device)
        recs = torch.empty((n.value, 3), dtype=torch.int32, device=self.device)
        self._enter(cells, recs)
        _lib.check(self.lib.bsc_point_log_read(self.h, _dp(cells), _dp(recs), n.value, C.byref(n)))
        self._leave()
        return cells, recs

    def replay_colour(self, vox_sorted, records, n_vox):
        """Records (n,3) int32 grouped by voxel (vox_sorted (n,) int32 ascending in [0, n_vox)), every voxel's in global point
        order -> (rgb (n_vox,3) u8, weight (n_vox,) f32): the sequential chain of memory_2.py:888-899 from the empty state."""
        vox_sorted, records = vox_sorted.contiguous(), records.contiguous()
        assert vox_sorted.dtype == torch.int32 and records.dtype == torch.int32 and records.shape == (vox_sorted.numel(), 3)
        rgb = torch.zeros((n_vox, 3), dtype=torch.uint8, device=self.device)
        w = torch.zeros(n_vox, dtype=torch.float32, device=self.device)
        st = torch.cuda.current_stream(self.device)
        _lib.check(self.lib.bsc_replay_colour(vox_sorted.numel(), _dp(vox_sorted), _dp(records), int(n_vox), _dp(rgb), _dp(w),
                                              C.c_void_p(st.cuda_stream)))
        return rgb, w

    def import_heightmap(self, max_height, cv_map):
        gs = self.cfg.grid_size
        mh = np.ascontiguousarray(max_height, np.float64)
        cv = np.ascontiguousarray(cv_map, np.uint8)
        assert mh.shape == (gs, gs) and cv.shape == (gs, gs, 3)
        _lib.check(self.lib.bsc_import_heightmap(self.h, _hp(mh), _hp(cv)))
