"""CPU-side checks of bsc_score_map's boundary: the header text, the ctypes signature, the exported symbol, and how
VoxelEngine.score_map turns its region arguments into the pointer the library gets (needs no context)."""
import ctypes as C
import inspect
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_score_map():
    text = open(os.path.join(ROOT, "include", "bscnav.h")).read()
    m = re.search(r"bsc_status\s+bsc_score_map\s*\((.*?)\)\s*;", text, flags=re.S)
    assert m, "include/bscnav.h does not declare bsc_score_map"
    params = [p.strip() for p in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
    assert len(params) == 6
    assert params[0].startswith("bsc_ctx *") and params[1].startswith("const float *") and params[2].startswith("int32_t ")
    assert params[3].startswith("const bsc_region *") and params[4].startswith("float *") and params[5].startswith("int32_t *")
    assert "memory_2.py:623-671" in text[:m.start()].rsplit("/*", 1)[1]      # the comment above it cites the reference's scan


def test_signature_is_declared_and_exported():
    from bsc_nav_amd import _lib
    res, args = _lib.SIGNATURES["bsc_score_map"]
    assert res is C.c_int32 and len(args) == 6 and args[2] is C.c_int32
    assert all(a is C.c_void_p for i, a in enumerate(args) if i != 2)
    assert hasattr(_lib.load(), "bsc_score_map")


def test_no_region_arguments_give_a_null_pointer():
    from bsc_nav_amd.engine import _hp, score_map_regions
    assert score_map_regions(5) is None and _hp(score_map_regions(5)) is None
    assert score_map_regions(5, None, None, None) is None


def test_region_arguments_go_through_region_array(monkeypatch):
    from bsc_nav_amd import engine
    r = engine.score_map_regions(3, radius=[30, None, 50.5], curr=[[1, 2, 3], [4, 5, 6], [7, 8, 9]], floor=[None, (2, 5), None])
    ref = engine.region_array(3, radius=[30, None, 50.5], curr=[[1, 2, 3], [4, 5, 6], [7, 8, 9]], floor=[None, (2, 5), None])
    assert r.dtype == engine.REGION_DTYPE and r.tobytes() == ref.tobytes()
    r = engine.score_map_regions(2, floor=(4, 9))                   # one argument given is enough for an array
    assert r.shape == (2,) and r["floor_lo"].tolist() == [4, 4] and np.all(r["radius"] == -1.0)
    r = engine.score_map_regions(2, radius=np.inf)                  # voxel_localized's default radius: open regions, not NULL
    assert r.shape == (2,) and np.all(r["radius"] == -1.0)
    calls = []
    monkeypatch.setattr(engine, "region_array", lambda *a: calls.append(a) or "sentinel")
    assert engine.score_map_regions(4, 9.0, [1, 2, 3], None) == "sentinel" and calls == [(4, 9.0, [1, 2, 3], None)]


def test_engine_and_memory_methods_exist_with_the_documented_arguments():
    from bsc_nav_amd import engine, memory
    sig = inspect.signature(engine.VoxelEngine.score_map)
    assert list(sig.parameters) == ["self", "q", "radius", "curr", "floor", "heights"]
    assert [sig.parameters[k].default for k in ("radius", "curr", "floor", "heights")] == [None, None, None, True]
    assert "score_map_regions(" in inspect.getsource(engine.VoxelEngine.score_map)
    sig = inspect.signature(memory.VoxelTokenMemory.voxel_score_map)
    assert list(sig.parameters) == ["self", "prompts", "region_radius", "curr_grid", "floors"]
    assert sig.parameters["region_radius"].default == np.inf and sig.parameters["floors"].default is None
