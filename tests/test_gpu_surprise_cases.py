"""bsc_flush_surprise on the GPU against the test-side replay (tests/surprise_replay.py) over the generated cases of
tests/surprise_cases.py: radius 0-3, cache_size 1 and 64, token_dim 4 .. 2048, the three level-table variants, the LDS
bound on both sides, deep schedules, long tasks, zero tokens and infinite thresholds.  tests/test_surprise_cases.py checks
on the CPU that every case keeps its decisions >= 1e-4 from the thresholds and takes the paths it is named after."""
import numpy as np
import pytest

import surprise_cases as SC
from test_gpu_surprise import _direct_engine, assert_store_matches

pytestmark = pytest.mark.gpu

REFUSED = ("refused_r3", "refused_r2")


def _check_state(eng, store, flushes, tag):
    pos, cnt, feat, dis, merged = store
    assert_store_matches(eng.export_store(), pos, cnt, feat, dis, merged, tag)
    c = eng.counters()
    assert c["iter_id"] == 0 and c["flushes"] == flushes, (tag, c)
    assert c["store_voxels"] == len(cnt) and c["store_tokens"] == int(cnt.sum()), (tag, c)
    assert len(eng.export_cache()[0]) == 0, tag


def _flush_twice(eng, z, rep, tag, between=None):
    """The case's flush, then a second one right after: the cache is iter_size zero rows at [0,0,0] by then."""
    c0 = eng.counters()
    assert c0["iter_id"] == int(z["iter_size"])
    eng.flush_surprise(int(z["radius"]), float(z["sthr"]), float(z["bthr"]))
    _check_state(eng, rep["store"], c0["flushes"] + 1, f"{tag} flush")
    if between:
        between()
    eng.flush_surprise(int(z["radius"]), float(z["sthr"]), float(z["bthr"]))
    _check_state(eng, rep["store2"], c0["flushes"] + 2, f"{tag} second flush over the zero cache")


def _localize_equal(eng, z):
    """localize over the flushed engine == over a fresh engine that imported the exported store: the flush marks the names
    and the row scales dirty, and a shrunken group leaves stale pool rows behind."""
    import torch
    got, rgbstate = eng.export_store(), eng.export_rgb()
    fresh = _direct_engine(z)
    try:
        fresh.import_rgb(*rgbstate)
        fresh.import_store(*got)
        rs = np.random.RandomState(7)
        live = got[2][got[2].any(axis=1)]
        q = live[rs.choice(len(live), 3, replace=False)] + 0.01 * rs.standard_normal((3, int(z["D"])))
        qv = torch.from_numpy(q.astype(np.float32)).cuda()
        a, b = eng.localize(qv, K=20), fresh.localize(qv, K=20)
        assert a[2].min() > 0
        for x, y in zip(a, b):
            assert np.array_equal(x, y, equal_nan=True), f"{z['name']}: localize differs from a freshly imported store"
    finally:
        fresh.close()


@pytest.mark.parametrize("name", [n for n in SC.CASES if n not in REFUSED])
def test_case_matches_replay(name):
    z, rep = SC.case(name), SC.replayed(name)
    print(f"{name}: {rep['counts']} margins {rep['margins']}")
    assert min(rep["margins"].values()) >= SC.MARGIN, rep["margins"]
    eng = _direct_engine(z)
    try:
        assert SC.LOCALIZE.get(name, int(z["radius"])) == int(z["radius"])
        _flush_twice(eng, z, rep, name, (lambda: _localize_equal(eng, z)) if name in SC.LOCALIZE else None)
    finally:
        eng.close()


@pytest.mark.parametrize("name", REFUSED)
def test_lds_bound_refused(name):
    """One cache_size beyond the LDS bound at radius 3 / 2: BSC_E_INVALID with store, cache and counters unchanged (the form
    of test_errors_leave_state_unchanged); the same context then flushes at radius 1 and equals the replay."""
    import bsc_nav_amd as B
    z, rep = SC.case(name), SC.replayed(name)
    assert SC.lds_bytes(int(z["refused_radius"]), int(z["cache_size"]), int(z["D"])) > SC.SURP_TASK_LDS
    assert min(rep["margins"].values()) >= SC.MARGIN, rep["margins"]
    eng = _direct_engine(z)
    try:
        before = eng.export_store(), eng.export_cache(), eng.counters()
        with pytest.raises(B._lib.BscError, match="status -1"):
            eng.flush_surprise(int(z["refused_radius"]), float(z["sthr"]), float(z["bthr"]))
        after = eng.export_store(), eng.export_cache(), eng.counters()
        for x, y in zip(before[:2], after[:2]):
            assert all(np.array_equal(a, b) for a, b in zip(x, y))
        assert before[2] == after[2]
        _flush_twice(eng, z, rep, name)
    finally:
        eng.close()
