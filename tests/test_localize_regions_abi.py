"""CPU-side checks of bsc_localize_regions' boundary: struct bsc_region in ctypes / NumPy against the header text, and the
argument normalisation of VoxelEngine.localize_regions (engine.region_array), which needs no context."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_C_TYPES = {"double": (C.c_double, 8), "int32_t": (C.c_int32, 4)}


def _header_fields():
    """[(name, ctype size, count)] of struct bsc_region as include/bscnav.h declares it."""
    text = open(os.path.join(ROOT, "include", "bscnav.h")).read()
    body = re.search(r"typedef struct bsc_region \{(.*?)\} bsc_region;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype, rest = decl.split(None, 1)
        for part in rest.split(","):
            m = re.fullmatch(r"\s*([A-Za-z_][A-Za-z_0-9]*)\s*(?:\[(\d+)\])?\s*", part)
            out.append((m.group(1), _C_TYPES[ctype][1], int(m.group(2) or 1)))
    return out


def test_region_struct_matches_header():
    from bsc_nav_amd import _lib, engine
    fields = _header_fields()
    assert [f[0] for f in fields] == ["radius", "curr", "floor_lo", "floor_hi", "reserved"]
    off = 0
    for name, size, count in fields:                       # natural alignment, no implicit padding
        assert off % size == 0, f"{name} would need padding"
        assert getattr(_lib.BscRegion, name).offset == off, name
        assert getattr(_lib.BscRegion, name).size == size * count, name
        assert engine.REGION_DTYPE.fields[name][1] == off, name
        off += size * count
    assert off == 32 == C.sizeof(_lib.BscRegion) == engine.REGION_DTYPE.itemsize
    assert [f[0] for f in _lib.BscRegion._fields_] == [f[0] for f in fields] == list(engine.REGION_DTYPE.names)


def test_signature_is_declared_and_exported():
    from bsc_nav_amd import _lib
    res, args = _lib.SIGNATURES["bsc_localize_regions"]
    assert res is C.c_int32 and len(args) == 8 and args[2] is C.c_int32 and args[3] is C.c_int32
    assert hasattr(_lib.load(), "bsc_localize_regions")


def test_region_array_scalar_for_all_and_none():
    from bsc_nav_amd.engine import region_array
    r = region_array(3)
    assert r.shape == (3,) and np.all(r["radius"] == -1.0) and np.all(r["floor_lo"] > r["floor_hi"]) and np.all(r["reserved"] == 0)
    r = region_array(3, radius=30, curr=[1, 2, 3], floor=(4, 9))
    assert r["radius"].tolist() == [30.0] * 3 and r["curr"].tolist() == [[1, 2, 3]] * 3
    assert r["floor_lo"].tolist() == [4] * 3 and r["floor_hi"].tolist() == [9] * 3
    r = region_array(2, radius=np.inf)                     # voxel_localized's default: no sphere, no curr needed
    assert r["radius"].tolist() == [-1.0, -1.0]
    assert region_array(0).shape == (0,)


def test_region_array_per_query():
    from bsc_nav_amd.engine import region_array
    r = region_array(3, radius=[30, None, 50.5], curr=[[1, 2, 3], [4, 5, 6], [7, 8, 9]], floor=[None, (2, 5), None])
    assert r["radius"].tolist() == [30.0, -1.0, 50.5]
    assert r["curr"].tolist() == [[1, 2, 3], [4, 5, 6], [7, 8, 9]]
    assert (r["floor_lo"][1], r["floor_hi"][1]) == (2, 5) and r["floor_lo"][0] > r["floor_hi"][0] and r["floor_lo"][2] > r["floor_hi"][2]
    r = region_array(2, floor=[(1, 2), (3, 4)])            # two pairs for two queries, not one pair for all
    assert r["floor_lo"].tolist() == [1, 3] and r["floor_hi"].tolist() == [2, 4]
    r = region_array(3, radius=(30, 40, 50), curr=np.array([5, 6, 7]))           # the adaptive-region loop: one position
    assert r["radius"].tolist() == [30.0, 40.0, 50.0] and r["curr"].tolist() == [[5, 6, 7]] * 3
    assert np.isnan(region_array(1, radius=[float("nan")], curr=[0, 0, 0])["radius"][0])      # the library refuses it


def test_region_array_wrong_lengths_raise():
    from bsc_nav_amd.engine import region_array
    with pytest.raises(ValueError):
        region_array(3, radius=[1, 2], curr=[0, 0, 0])
    with pytest.raises(ValueError):
        region_array(3, radius=1, curr=[[0, 0, 0], [1, 1, 1]])
    with pytest.raises(ValueError):
        region_array(3, floor=[(1, 2), None])
    with pytest.raises(ValueError):
        region_array(2, floor=[(1, 2, 3), None])
    with pytest.raises(ValueError):
        region_array(2, radius=[None, 3.0])                # a sphere without curr
