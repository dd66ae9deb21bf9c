"""CPU-side checks of bsc_cluster_centers_batch's boundary: the ctypes signature against the header and the library's
exports, and the padding of VoxelEngine.cluster_centers_batch's arguments (engine.pad_cluster_batch), which needs no context."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_signature_is_declared_and_exported():
    from bsc_nav_amd import _lib
    res, args = _lib.SIGNATURES["bsc_cluster_centers_batch"]
    assert res is C.c_int32 and len(args) == 12
    assert args[1] is C.c_int32 and args[2] is C.c_int32 and args[6] is C.c_double and args[7] is C.c_int32
    assert all(a is C.c_void_p for i, a in enumerate(args) if i not in (1, 2, 6, 7))
    assert hasattr(_lib.load(), "bsc_cluster_centers_batch")


def test_header_declares_the_twelve_arguments_in_order():
    text = open(os.path.join(ROOT, "include", "bscnav.h")).read()
    m = re.search(r"bsc_status\s+bsc_cluster_centers_batch\s*\((.*?)\)\s*;", text, flags=re.S)
    assert m, "include/bscnav.h does not declare bsc_cluster_centers_batch"
    params = [re.sub(r"/\*.*?\*/", "", p, flags=re.S).split()[-1].lstrip("*") for p in m.group(1).split(",")]
    assert params == ["ctx", "n_queries", "K", "counts_host", "pos_host", "sim_host", "eps", "min_samples", "centers_host",
                      "labels_host", "sizes_host", "n_clusters_host"]


def test_padding_of_ragged_lists():
    from bsc_nav_amd.engine import pad_cluster_batch
    rs = np.random.RandomState(0)
    lens = [5, 0, 12, 1]
    pos = [rs.randint(0, 200, size=(n, 3)).astype(np.int64) for n in lens]
    sim = [rs.rand(n) for n in lens]
    P, S, cnt = pad_cluster_batch(pos, sim)
    assert P.shape == (4, 12, 3) and P.dtype == np.int32 and P.flags["C_CONTIGUOUS"]
    assert S.shape == (4, 12) and S.dtype == np.float32 and S.flags["C_CONTIGUOUS"]
    assert cnt.dtype == np.int32 and cnt.tolist() == lens
    for i, n in enumerate(lens):
        assert np.array_equal(P[i, :n], pos[i]) and np.array_equal(S[i, :n], sim[i].astype(np.float32))
        assert not P[i, n:].any() and not S[i, n:].any()
    # every list empty: one padded column, so that the call still has K >= 1
    P, S, cnt = pad_cluster_batch([np.zeros((0, 3), np.int64)] * 2, [np.zeros(0)] * 2)
    assert P.shape == (2, 1, 3) and S.shape == (2, 1) and cnt.tolist() == [0, 0]


def test_padding_of_arrays_with_counts():
    from bsc_nav_amd.engine import pad_cluster_batch
    rs = np.random.RandomState(1)
    pos, sim = rs.randint(0, 50, size=(3, 7, 3)), rs.rand(3, 7)
    P, S, cnt = pad_cluster_batch(pos, sim)
    assert np.array_equal(P, pos) and P.dtype == np.int32 and S.dtype == np.float32 and cnt.tolist() == [7, 7, 7]
    P, S, cnt = pad_cluster_batch(pos, sim, counts=[7, 0, 3])
    assert cnt.dtype == np.int32 and cnt.tolist() == [7, 0, 3]


def test_padding_refuses_mismatched_lengths():
    from bsc_nav_amd.engine import pad_cluster_batch
    with pytest.raises(ValueError):
        pad_cluster_batch([np.zeros((4, 3))], [np.zeros(5)])                    # positions / similarities of one query
    with pytest.raises(ValueError):
        pad_cluster_batch([np.zeros((4, 3))] * 2, [np.zeros(4)])                # number of queries
    with pytest.raises(ValueError):
        pad_cluster_batch([], [])
    with pytest.raises(ValueError):
        pad_cluster_batch([np.zeros((4, 3))], [np.zeros(4)], counts=[4])        # ragged lists carry their lengths
    with pytest.raises(ValueError):
        pad_cluster_batch(np.zeros((2, 4, 3)), np.zeros((2, 5)))
    with pytest.raises(ValueError):
        pad_cluster_batch(np.zeros((2, 4, 3)), np.zeros((2, 4)), counts=[4])
    with pytest.raises(ValueError):
        pad_cluster_batch(np.zeros((2, 4, 3)), np.zeros((2, 4)), counts=[4, 5])
    with pytest.raises(ValueError):
        pad_cluster_batch(np.zeros((2, 4, 3)), np.zeros((2, 4)), counts=[-1, 2])
