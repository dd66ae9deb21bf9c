"""Scenes, cameras and the expected result of bsc_render_views, shared by tests/test_ray_walk.py (the traversal header on the CPU)
and tests/test_gpu_render.py (the library on the GPU).  The expected result is a NumPy slab intersection of every ray with every
voxel's cell box in f64, with the truncation-cell intervals of the ingest (geometry_dev.h:113-119): along an axis, truncation cell
k covers [k cs, (k+1) cs) for k > 0, (-cs, cs) for k = 0 and ((k-1) cs, k cs] for k < 0."""
import numpy as np

TOL = 1e-9
AMBIGUOUS_CAP = 0.005           # of a view's pixels


def cam_mat_fov(h, w, fov=90):  # utils.py:181-186
    m = np.eye(3)
    m[0, 0] = m[1, 1] = w / (2.0 * np.tan(np.deg2rad(fov / 2)))
    m[0, 2] = w / 2.0
    m[1, 2] = h / 2.0
    return m


def kinv_fov(h, w, fov=90):
    return np.linalg.inv(cam_mat_fov(h, w, fov))


def _P(j, cs):
    """lower boundary of truncation cell j"""
    j = np.asarray(j, np.int64)
    return np.where(j > 0, j, j - 1).astype(np.float64) * cs


def cell_boxes(gs, min_h, cs, pos):
    """(lo (N,3), hi (N,3)) map coordinates of the cells of pos (N,3) = row, column, stored h"""
    pos = np.asarray(pos, np.int64).reshape(-1, 3)
    k = np.stack([gs // 2 - pos[:, 0], gs // 2 - pos[:, 1], pos[:, 2] + min_h], 1)
    return _P(k, cs), _P(k + 1, cs)


def rays(T, kinv, H, W):
    """o (3,), d (H*W,3): o = T[:3,3], d = T[:3,:3] (K^-1 (x+0.5, y+0.5, 1)), pixels row-major"""
    T, kinv = np.asarray(T, np.float64).reshape(4, 4), np.asarray(kinv, np.float64).reshape(3, 3)
    y, x = np.divmod(np.arange(H * W), W)
    px, py = x + 0.5, y + 0.5
    c = [(kinv[i, 0] * px + kinv[i, 1] * py) + kinv[i, 2] for i in range(3)]
    d = np.stack([(T[i, 0] * c[0] + T[i, 1] * c[1]) + T[i, 2] * c[2] for i in range(3)], 1)
    return T[:3, 3].copy(), d


def slab_reference(gs, nh, min_h, cs, pos, T, kinv, H, W, t_min, t_max, band=None, tol=TOL):
    """Per pixel: index into pos of the first voxel (-1: none), its depth max(t_in, t_min) (0: none), and whether the pixel is
    ambiguous: the winner's interval shorter than tol or within tol of t_min / t_max, or another voxel whose interval is longer than
    -tol entering within tol of the winner."""
    pos = np.asarray(pos, np.int64).reshape(-1, 3)
    P = H * W
    keep = np.ones(len(pos), bool)
    if band is not None and band[0] <= band[1]:
        keep = (pos[:, 2] >= band[0]) & (pos[:, 2] <= band[1])
    index = np.nonzero(keep)[0]
    idx, t, amb = np.full(P, -1, np.int64), np.zeros(P), np.zeros(P, bool)
    if len(index) == 0:
        return dict(idx=idx, t=t, ambiguous=amb)
    lo, hi = cell_boxes(gs, min_h, cs, pos[index])
    o, d = rays(T, kinv, H, W)
    t_in, t_out = np.full((P, len(index)), -np.inf), np.full((P, len(index)), np.inf)
    with np.errstate(divide="ignore", invalid="ignore"):
        for a in range(3):
            da = d[:, a:a + 1]
            ta, tb = (lo[None, :, a] - o[a]) / da, (hi[None, :, a] - o[a]) / da
            inside = np.broadcast_to((o[a] > lo[:, a]) & (o[a] < hi[:, a]), ta.shape)
            tn = np.where(da == 0, np.where(inside, -np.inf, np.inf), np.minimum(ta, tb))
            tf = np.where(da == 0, np.where(inside, np.inf, -np.inf), np.maximum(ta, tb))
            t_in, t_out = np.maximum(t_in, tn), np.minimum(t_out, tf)
    ok = (t_in < t_out) & (t_in <= t_max) & (t_out > t_min)
    key = np.where(ok, np.maximum(t_in, t_min), np.inf)
    w = np.argmin(key, 1)
    rows = np.arange(P)
    hit = np.isfinite(key[rows, w])
    idx[hit], t[hit] = index[w[hit]], key[rows, w][hit]
    wi, wo = t_in[rows, w], t_out[rows, w]
    amb = hit & ((wo - wi < tol) | (np.abs(wi - t_min) < tol) | (np.abs(wi - t_max) < tol) | (np.abs(wo - t_min) < tol))
    near = (t_out - t_in > -tol) & (t_out > t_min - tol) & (np.maximum(t_in, t_min) < key[rows, w][:, None] + tol)
    near[rows, w] = False
    amb |= hit & near.any(1)
    return dict(idx=idx, t=t, ambiguous=amb)


# ---- cameras ---------------------------------------------------------------------------------------------------------------
def _pose(centre, rot):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = rot, centre
    return T


def _euler(x, y, z):
    from scipy.spatial.transform import Rotation as R
    return R.from_euler("xyz", [x, y, z], degrees=True).as_matrix()


def _look(direction, up=(0.1, 0.2, 1.0)):
    """a rotation whose third column (the camera's depth axis) points along `direction`"""
    z = np.asarray(direction, np.float64) / np.linalg.norm(direction)
    x = np.cross(np.asarray(up, np.float64), z)
    x /= np.linalg.norm(x)
    return np.stack([x, np.cross(z, x), z], 1)


# case 1: gs 32, nh 12, cs 0.25, min_h -4 (x, y in (-4, 4.25), z in (-1.25, 2)), fov 90, t in [0.1, 10]
CASE1 = dict(gs=32, nh=12, min_h=-4, cs=0.25, t_min=0.1, t_max=10.0)
ROT_XZ90 = np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])      # Rz(90) Rx(90): every entry exactly 0 or 1


def case1_voxels(n=1500, seed=11):
    rng = np.random.RandomState(seed)
    g = CASE1
    codes = rng.permutation(g["gs"] * g["gs"] * g["nh"])[:n]
    pos = np.stack([codes // (g["gs"] * g["nh"]), (codes // g["nh"]) % g["gs"], codes % g["nh"]], 1).astype(np.int32)
    return pos, rng.randint(1, 256, size=(n, 3)).astype(np.uint8)


def case1_cameras():
    """(name, T, H, W): a generic; b next to the origin with the identity (exact zeros in the centre row and column, the camera in
    the double-width cells); c starting exactly on cell planes; d axis-aligned rays off the planes; e near a corner looking out;
    f 9 m outside the grid looking in."""
    return [
        ("a_generic", _pose((0.37, -0.81, 0.43), _euler(25.0, -40.0, 70.0)), 24, 32),
        ("b_origin_identity", _pose((0.013, -0.021, 0.017), np.eye(3)), 25, 33),
        ("c_on_planes", _pose((0.25, 0.5, -0.25), _euler(-63.0, 17.0, 131.0)), 24, 32),
        ("d_axis_aligned", _pose((0.263, 0.51, -0.27), ROT_XZ90), 25, 33),
        ("e_corner_outward", _pose((-3.9, 3.9, 1.9), _look((-0.3, 1.0, -0.5))), 24, 32),
        ("f_outside_inward", _pose((13.25, 0.7, 0.4), _look((-1.0, -0.06, 0.01))), 24, 32),
    ]


# case 2: gs 30 (even, no multiple of 4), nh 5
CASE2 = dict(gs=30, nh=5, min_h=-2, cs=0.25, t_min=0.1, t_max=10.0)


def case2_scenes():
    """name -> pos (N,3): voxels on all six faces of the grid; one voxel per brick with every one of the 64 bit positions in use;
    one full brick"""
    gs, nh = CASE2["gs"], CASE2["nh"]
    rng = np.random.RandomState(2)
    faces = set()
    for _ in range(60):
        u, v, w = int(rng.randint(gs)), int(rng.randint(gs)), int(rng.randint(nh))
        faces |= {(0, u, w), (gs - 1, v, w), (u, 0, w), (v, gs - 1, w), (u, v, 0), (v, u, nh - 1)}
    per_brick, used = [], set()
    for br in range((gs + 3) // 4):
        for bc in range((gs + 3) // 4):
            for bh in range((nh + 3) // 4):
                # the first bit position not used yet that exists in this (maybe partial) brick, else any that exists
                for p in [p for p in range(64) if p not in used] + list(range(64)):
                    r, c, h = 4 * br + (p >> 4), 4 * bc + (p >> 2 & 3), 4 * bh + (p & 3)
                    if r < gs and c < gs and h < nh:
                        per_brick.append((r, c, h))
                        used.add(p)
                        break
    assert len(used) == 64
    full = [(12 + r, 16 + c, h) for r in range(4) for c in range(4) for h in range(4)]
    return {"faces": np.array(sorted(faces), np.int32), "one_per_brick": np.array(per_brick, np.int32),
            "full_brick": np.array(full, np.int32)}


def case2_cameras():
    return [("g_generic", _pose((0.31, -0.17, 0.12), _euler(-20.0, 35.0, -100.0)), 24, 32),
            ("h_across", _pose((-3.1, -2.7, -0.4), _look((1.0, 0.85, 0.08))), 24, 32)]


def colours(n, seed=5):
    return np.random.RandomState(seed).randint(1, 256, size=(n, 3)).astype(np.uint8)


def clip_band(band, nh):
    """(lo, hi) as the library clips it: None or lo > hi as given is every height; lo > hi afterwards is empty"""
    if band is None or band[0] > band[1]:
        return 0, nh - 1
    return max(band[0], 0), min(band[1], nh - 1)


def write_scene_file(path, grid, pos, cases):
    """The scene file of tests/host/ray_walk_main.cpp; cases: (name, T, kinv, H, W, t_min, t_max, (lo, hi) clipped)"""
    with open(path, "w") as f:
        f.write("grid %d %d %d %s\n" % (grid["gs"], grid["nh"], grid["min_h"], float(grid["cs"]).hex()))
        f.write("voxels %d\n" % len(pos))
        for r, c, h in np.asarray(pos).tolist():
            f.write("%d %d %d\n" % (r, c, h))
        f.write("cases %d\n" % len(cases))
        for name, T, kinv, H, W, t_min, t_max, (lo, hi) in cases:
            f.write("%s %d %d %s %s %d %d\n" % (name, H, W, float(t_min).hex(), float(t_max).hex(), lo, hi))
            f.write("T " + " ".join(float(v).hex() for v in np.asarray(T).reshape(16)) + "\n")
            f.write("K " + " ".join(float(v).hex() for v in np.asarray(kinv).reshape(9)) + "\n")
