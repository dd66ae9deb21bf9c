"""CPU-side checks of the boundary of bsc_render_views: the header text, the ctypes signature, the exported symbol, and the
Python methods in front of it (needs no context)."""
import copy
import ctypes as C
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declaration(text, name):
    m = re.search(r"bsc_status\s+%s\s*\((.*?)\)\s*;" % name, text, flags=re.S)
    assert m, f"include/bscnav.h does not declare {name}"
    params = [p.strip() for p in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
    comment = text[:m.start()].rsplit("\n/*", 1)[1].split("*/", 1)[0]        # the block comment above the declaration
    return params, comment


def test_header_declares_the_call():
    text = open(os.path.join(ROOT, "include", "bscnav.h")).read()
    p, comment = _declaration(text, "bsc_render_views")
    assert len(p) == 12
    want = ["bsc_ctx *", "int32_t ", "const double *", "const double *", "int32_t ", "int32_t ", "double ", "double ",
            "const bsc_band *", "int32_t *", "float *", "uint8_t *"]
    for got, w in zip(p, want):
        assert got.startswith(w), (got, w)
    assert [re.search(r"(\w+)$", q).group(1) for q in p] == ["ctx", "n_views", "transforms_host", "kinv_host", "height", "width",
                                                            "t_min", "t_max", "band_host", "voxel_dev", "depth_dev", "rgb_dev"]
    for cite in ("utils.py:153-214", "memory_2.py:859-875"):
        assert cite in comment, cite
    for word in ("BSC_E_INVALID", "odd grid_size", "[0, 0, 1]", "(-cs, cs) for k = 0", "max(t_in, t_min)"):
        assert word in comment, word


def test_signature_is_declared_and_exported():
    from bsc_nav_amd import _lib
    res, args = _lib.SIGNATURES["bsc_render_views"]
    V, I, F = C.c_void_p, C.c_int32, C.c_double
    assert res is C.c_int32 and args == [V, I, V, V, I, I, F, F, V, V, V, V]
    assert hasattr(_lib.load(), "bsc_render_views")


def test_methods_exist_with_the_documented_arguments():
    from bsc_nav_amd import engine, geometry, memory
    sig = inspect.signature(engine.VoxelEngine.render_views)
    assert list(sig.parameters) == ["self", "transforms", "size", "kinv", "band", "t_range", "want"]
    assert [sig.parameters[k].default for k in ("size", "kinv", "band", "t_range")] == [None] * 4
    assert tuple(sig.parameters["want"].default) == ("voxel", "depth", "rgb")
    assert "band_array(" in inspect.getsource(engine.VoxelEngine.render_views)
    for name in ("render_view", "visible_voxels"):
        sig = inspect.signature(getattr(memory.VoxelTokenMemory, name))
        assert list(sig.parameters) == ["self", "pose", "size", "fov", "band", "max_range"], name
        assert all(sig.parameters[k].default is None for k in ("size", "fov", "band", "max_range")), name
    # the view must not move the map: pc_transform sets chain.tf and anchors an unanchored chain
    for fn in (memory.VoxelTokenMemory.render_view, memory.VoxelTokenMemory.visible_voxels, memory.VoxelTokenMemory._render):
        assert "pc_transform" not in inspect.getsource(fn)
    assert "transform_of(" in inspect.getsource(memory.VoxelTokenMemory._render)
    assert "_default_band()" in inspect.getsource(memory.VoxelTokenMemory._render)
    assert list(inspect.signature(geometry.PoseChain.transform_of).parameters) == ["self", "pose"]


def test_transform_of_is_pc_transform_without_its_side_effects():
    import numpy as np
    import pytest
    from bsc_nav_amd.geometry import PoseChain
    chain = PoseChain()
    poses = np.array([[0.3, 1.5, -0.2, 0.0, 0.38268343, 0.0, 0.92387953], [1.1, 1.5, 0.4, 0.0, -0.19509032, 0.0, 0.98078528],
                      [-0.6, 1.4, 2.0, 0.0, 0.70710678, 0.0, 0.70710678]])
    with pytest.raises(RuntimeError):
        chain.transform_of(poses[1])
    assert chain.inv_init_base_tf is None and chain.tf is None
    chain.pc_transform(poses[0])
    tf, anchor = chain.tf.copy(), chain.inv_init_base_tf.copy()
    got = chain.transform_of(poses[1])
    assert np.array_equal(chain.tf, tf) and np.array_equal(chain.inv_init_base_tf, anchor)
    assert got.shape == (4, 4) and got.flags["C_CONTIGUOUS"]
    assert np.array_equal(got, chain.pc_transform(poses[1]))                # the very bits
    assert np.array_equal(chain.transform_of(poses[2]), copy.deepcopy(chain).pc_transform(poses[2]))
