"""The generated surprise-flush cases (tests/surprise_cases.py) are honest inputs: the f64 replay keeps every decision at
least 1e-4 from its threshold (so the f32 kernel cannot legitimately disagree), the paths a case exists for fire, and the
schedule regimes (level table variant, depth) are the ones the case is named after.  No GPU."""
import numpy as np
import pytest

import surprise_cases as SC
import surprise_replay as R


def _run(name):
    z, rep = SC.case(name), SC.replayed(name)
    c, m = rep["counts"], rep["margins"]
    print(f"{name}: r={z['radius']} cs={z['cache_size']} D={z['D']} rows={z['iter_size']} {c} second flush {rep['counts2']} "
          f"margins surprise={m['surprise']:.3g} boring={m['boring']:.3g} argmin={m['argmin']:.3g}")
    return z, c, rep


@pytest.mark.parametrize("name", list(SC.CASES))
def test_margins(name):
    z, c, rep = _run(name)
    m = rep["margins"]
    assert m["surprise"] >= SC.MARGIN and m["boring"] >= SC.MARGIN and m["argmin"] >= SC.MARGIN, m
    assert sum(c.values()) - c["replace_nan"] - c["merge"] == int(z["iter_size"])      # every row took one path
    assert SC.lds_bytes(int(z["radius"]), int(z["cache_size"]), int(z["D"])) <= SC.SURP_TASK_LDS
    assert int(z["D"]) % 4 == 0 and 1 <= int(z["cache_size"]) <= 64
    # the layout the engine imports: name order, counts within cache_size, rows only where a voxel is
    keys = [R.name_key(p) for p in z["prior_pos"]]
    assert keys == sorted(keys) and int(z["prior_cnt"].sum()) == len(z["prior_feat"]) == len(z["prior_dis"])
    assert len(z["vox_pos"]) <= int(z["voxel_capacity"]) and len(np.unique(z["vox_pos"], axis=0)) == len(z["vox_pos"])
    assert z["cache_pos"].min() >= 0 and z["cache_pos"][:, :2].max() < int(z["gs"]) and z["cache_pos"][:, 2].max() < int(z["nh"])
    assert not z["cache_pos"][int(z["n_real"]):].any() and not z["cache_feat"][int(z["n_real"]):].any()


def test_radius0_paths():
    z, c, _ = _run("radius0")
    assert z["radius"] == 0 and c["append"] > 0 and c["replace"] > 0 and c["merge"] > 0
    assert c["reject"] == 0 and c["nan_reject"] == 0


def test_radius3_paths():
    z, c, _ = _run("radius3")
    assert z["radius"] == 3 and all(c[k] > 0 for k in ("create", "reject", "append", "replace", "merge")), c
    vox = [tuple(int(v) for v in p) for p in z["vox_pos"]]
    gs, nh = int(z["gs"]), int(z["nh"])
    assert (0, 0, 0) in vox and int(z["iter_size"]) > int(z["n_real"])           # the real voxel and a zero tail
    assert (gs - 1, gs - 1, nh - 1) in vox                                      # a corner other than [0,0,0]
    rows = {tuple(int(v) for v in p) for p in z["cache_pos"][:int(z["n_real"])]}
    assert any(p[2] == 0 for p in rows) and any(p[2] == nh - 1 for p in rows) and any(p[0] == gs - 1 for p in rows)
    assert any(p[1] == 0 for p in rows) and any(p[1] == gs - 1 for p in rows)
    assert any((p[0] in (0, gs - 1)) + (p[1] in (0, gs - 1)) + (p[2] in (0, nh - 1)) == 2 for p in rows)    # an edge
    for p in z["lone"]:                                                         # rows without any voxel within 3 ...
        assert p in rows and all(SC.cheb(p, q) > 3 for q in vox if q != p)
    assert sum(any(SC.cheb(p, q) <= 3 for q in vox if q != p) for p in rows) > 10        # ... and rows with some


@pytest.mark.parametrize("name,radius,cs,D", [("lds_r3", 3, 16, 1024), ("lds_r2", 2, 46, 768)])
def test_lds_bound_cases(name, radius, cs, D):
    z, c, _ = _run(name)
    assert (int(z["radius"]), int(z["cache_size"]), int(z["D"])) == (radius, cs, D)
    assert SC.lds_bytes(radius, cs, D) <= SC.SURP_TASK_LDS < SC.lds_bytes(radius, cs + 1, D)
    # the centre's neighbour list is full: every other position of its neighbourhood holds a group of cache_size tokens
    centre = (1 + radius,) * 3
    st = R.store_from_arrays(z["prior_pos"], z["prior_cnt"], z["prior_feat"], z["prior_dis"])
    w = range(-radius, radius + 1)
    n = sum(len(st[(centre[0] + a, centre[1] + b, centre[2] + h)][0]) for a in w for b in w for h in w if (a, b, h) != (0, 0, 0))
    assert n == ((2 * radius + 1) ** 3 - 1) * cs
    assert any(tuple(p) == centre for p in z["cache_pos"]) and c["reject"] > 0 and c["append"] > 0 and c["replace"] > 0


@pytest.mark.parametrize("name,radius", [("refused_r3", 3), ("refused_r2", 2)])
def test_refused_cases(name, radius):
    z, c, _ = _run(name)
    assert int(z["refused_radius"]) == radius and int(z["radius"]) == 1
    assert SC.lds_bytes(radius, int(z["cache_size"]), int(z["D"])) > SC.SURP_TASK_LDS
    assert c["append"] > 0 and c["reject"] > 0


def test_cache_size_extremes():
    z, c, rep = _run("cache64")
    assert int(z["cache_size"]) == 64 and c["replace"] > 20 and c["merge"] > 0 and c["reject"] > 0
    assert rep["store"][1].max() == 64                                          # full groups at the end
    z, c, _ = _run("cache1")
    assert int(z["cache_size"]) == 1 and c["replace"] > 0 and c["append"] == 0 and c["merge"] == 0


@pytest.mark.parametrize("name,D", [("dim4", 4), ("dim520", 520), ("dim2048", 2048)])
def test_token_dims(name, D):
    z, c, _ = _run(name)
    assert int(z["D"]) == D and int(z["radius"]) == 1
    assert all(c[k] > 0 for k in ("create", "reject", "append", "replace", "merge")), c
    if D == 4:
        assert int(z["cache_size"]) <= 3


def test_level_table_regimes():
    """surprise_flush: u16 table when n_tasks < 65535 and n_u <= SURP_TAB16 (81920); else u32 in LDS when n_u <= SURP_TAB32
    (40960); else the table in global memory."""
    z, c, _ = _run("table_u32")
    n_tasks, n_u, depth = SC.schedule(z)
    print(f"table_u32: n_tasks={n_tasks} n_u={n_u} levels={depth}")
    assert n_tasks >= SC.TAB16_TASKS and n_u <= SC.SURP_TAB32
    assert all(c[k] > 0 for k in ("create", "reject", "append", "replace", "merge")), c
    z, c, _ = _run("table_global")
    n_tasks, n_u, depth = SC.schedule(z)
    print(f"table_global: n_tasks={n_tasks} n_u={n_u} levels={depth}")
    assert n_u > SC.SURP_TAB16 and int(z["gs"]) >= 64 and int(z["nh"]) >= 32
    assert all(c[k] > 0 for k in ("create", "reject", "append", "merge")), c
    for name in SC.CASES:                                                       # every other case takes the u16 table
        if name not in ("table_u32", "table_global"):
            z = SC.case(name)
            head = 1 + int(np.any(z["cache_pos"][1:] != z["cache_pos"][:-1], axis=1).sum())
            assert head < SC.TAB16_TASKS and len(np.unique(z["cache_pos"], axis=0)) <= SC.SURP_TAB16


def test_deep_schedule():
    z, c, _ = _run("deep")
    n_tasks, n_u, depth = SC.schedule(z)
    print(f"deep: n_tasks={n_tasks} n_u={n_u} levels={depth}")
    assert n_tasks == int(z["iter_size"]) >= 4000 and n_u == 4 and depth == n_tasks // 2 >= 2000
    assert all(SC.cheb(a, b) == 1 for a, b in z["pairs"]) and SC.cheb(z["pairs"][0][0], z["pairs"][1][0]) > 2
    assert all(c[k] > 0 for k in ("reject", "append", "replace", "merge")), c


def test_long_task():
    z, c, _ = _run("long_task")
    pos = z["cache_pos"]
    at = np.all(pos == np.array(z["long_voxel"], np.int32), axis=1)
    i = np.nonzero(at)[0]
    assert len(i) > 600 and i[-1] - i[0] + 1 == len(i) and len(i) % 256 != 0 and i[0] % 64 != 0       # one run, partial last chunk
    accepted = c["append"] + c["replace"] - int(z["rows_elsewhere"])            # at least this many at the long voxel
    assert accepted > 130 and c["merge"] > 50 and c["replace"] > 20 and c["reject"] > 100, c


def test_zero_token_paths():
    z, c, rep = _run("zeros")
    assert c["nan_reject"] >= 4 and c["replace_nan"] >= 6 and c["append"] > 0 and c["merge"] > 0, c
    zero_rows = ~z["cache_feat"][:int(z["n_real"])].any(axis=1)
    assert zero_rows.sum() > 80
    pos, cnt, feat, dis, merged = rep["store"]
    assert (~feat.any(axis=1)).sum() >= 4                                       # zero tokens survive in the store


def test_infinite_thresholds():
    z, c, _ = _run("sthr_pinf")
    assert z["sthr"] == np.inf and c["create"] > 0 and c["reject"] > 0
    assert all(c[k] == 0 for k in R.PATHS if k not in ("create", "reject")), c
    rows = [tuple(int(v) for v in p) for p in z["cache_pos"][:int(z["n_real"])]]
    vox = [tuple(int(v) for v in p) for p in z["vox_pos"]]
    alone = [p for p in set(rows) if all(SC.cheb(p, q) > 1 for q in vox if q != p)]
    assert any(rows.count(p) > 1 for p in alone)                                # rows without neighbours after the creating one
    z, c, _ = _run("sthr_ninf")
    assert z["sthr"] == -np.inf and c["reject"] == 0 and c["append"] > 0 and c["replace"] > 0 and c["merge"] > 0, c
    z, c, _ = _run("bthr_pinf")
    assert z["bthr"] == np.inf and c["merge"] == 0 and c["append"] > 0 and c["reject"] > 0, c
