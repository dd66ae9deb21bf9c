"""CPU-side checks of the boundary of bsc_topdown_slices / bsc_topdown_rebuild: the header text, the ctypes signatures, the
exported symbols, the bsc_band layout, and how VoxelEngine.topdown_slices turns its bands into the array the library gets
(needs no context)."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declaration(text, name):
    m = re.search(r"bsc_status\s+%s\s*\((.*?)\)\s*;" % name, text, flags=re.S)
    assert m, f"include/bscnav.h does not declare {name}"
    params = [p.strip() for p in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
    comment = text[:m.start()].rsplit("\n/*", 1)[1].split("*/", 1)[0]        # the block comment above the declarations
    return params, comment


def test_header_declares_both_calls_and_the_band():
    text = open(os.path.join(ROOT, "include", "bscnav.h")).read()
    p, comment = _declaration(text, "bsc_topdown_slices")
    assert len(p) == 6
    assert p[0].startswith("bsc_ctx *") and p[1].startswith("int32_t ") and p[2].startswith("const bsc_band *")
    assert p[3].startswith("uint8_t *") and p[4].startswith("int32_t *") and p[5].startswith("int32_t *")
    for cite in ("BSCAgent.py:203-234", "memory_2.py:98-100,901-903", ":202-252"):
        assert cite in comment, cite
    p, comment = _declaration(text, "bsc_topdown_rebuild")
    assert len(p) == 3 and p[0].startswith("bsc_ctx *") and p[1].startswith("int32_t ") and p[2].startswith("int32_t ")
    assert "BSCAgent.py:203-234" in comment and "memory_2.py:901-903" in comment
    m = re.search(r"typedef struct bsc_band \{(.*?)\} bsc_band;", text, flags=re.S)
    assert m and [f.strip() for f in m.group(1).strip().rstrip(";").split(";")] == ["int32_t lo, hi"]


def test_signatures_are_declared_and_exported():
    from bsc_nav_amd import _lib
    res, args = _lib.SIGNATURES["bsc_topdown_slices"]
    assert res is C.c_int32 and len(args) == 6 and args[1] is C.c_int32
    assert all(a is C.c_void_p for i, a in enumerate(args) if i != 1)
    res, args = _lib.SIGNATURES["bsc_topdown_rebuild"]
    assert res is C.c_int32 and args == [C.c_void_p, C.c_int32, C.c_int32]
    L = _lib.load()
    assert hasattr(L, "bsc_topdown_slices") and hasattr(L, "bsc_topdown_rebuild")


def test_band_layout_is_eight_bytes():
    from bsc_nav_amd import _lib, engine
    assert C.sizeof(_lib.BscBand) == 8 and [f[0] for f in _lib.BscBand._fields_] == ["lo", "hi"]
    assert engine.BAND_DTYPE.itemsize == 8 and engine.BAND_DTYPE.names == ("lo", "hi")
    assert engine.BAND_DTYPE.fields["lo"][1] == 0 and engine.BAND_DTYPE.fields["hi"][1] == 4


def test_band_helper():
    from bsc_nav_amd.engine import BAND_DTYPE, _hp, band_array
    assert band_array(None) is None and _hp(band_array(None)) is None          # a NULL pointer: one open band
    b = band_array([None, (3, 9), (5, 5), (-4, 1000), None])
    assert b.dtype == BAND_DTYPE and b.shape == (5,) and b.flags["C_CONTIGUOUS"]
    assert np.all(b["lo"][[0, 4]] > b["hi"][[0, 4]])                            # None: lo > hi, every height
    assert b["lo"][1:4].tolist() == [3, 5, -4] and b["hi"][1:4].tolist() == [9, 5, 1000]
    assert band_array((2, 7)).tolist() == [(2, 7)]                              # one pair of numbers is one band
    b = band_array([(-2 ** 31, 4), (-2 ** 40, 2 ** 40)])                        # int32 limits pass, wider bounds are clamped
    assert b["lo"].tolist() == [-2 ** 31, -2 ** 31] and b["hi"].tolist() == [4, 2 ** 31 - 1]
    assert band_array([]).shape == (0,)
    with pytest.raises(ValueError):
        band_array([(1, 2, 3)])


def test_engine_and_memory_methods_exist_with_the_documented_arguments():
    from bsc_nav_amd import engine, memory
    sig = inspect.signature(engine.VoxelEngine.topdown_slices)
    assert list(sig.parameters) == ["self", "bands", "heights", "counts"]
    assert [sig.parameters[k].default for k in ("bands", "heights", "counts")] == [None, True, True]
    assert "band_array(" in inspect.getsource(engine.VoxelEngine.topdown_slices)
    sig = inspect.signature(engine.VoxelEngine.rebuild_topdown)
    assert list(sig.parameters) == ["self", "band"] and sig.parameters["band"].default is None
    sig = inspect.signature(memory.VoxelTokenMemory.topdown_maps)
    assert list(sig.parameters) == ["self", "bands"] and sig.parameters["bands"].default is None
    assert list(inspect.signature(memory.VoxelTokenMemory.rgb_2d_map).parameters) == ["self", "height"]
    sig = inspect.signature(memory.VoxelTokenMemory.rebuild_topdown_map)
    assert list(sig.parameters) == ["self", "band"] and sig.parameters["band"].default is None
    assert "_touch()" in inspect.getsource(memory.VoxelTokenMemory.rebuild_topdown_map)
