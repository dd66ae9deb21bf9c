"""CPU-side checks of the flush-policy / store-compaction boundary: bsc_set_flush_policy, bsc_store_usage and
bsc_compact_store are declared in include/bscnav.h, bound in _lib.SIGNATURES and exported by the built library."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGC = {"bsc_set_flush_policy": 5, "bsc_store_usage": 2, "bsc_compact_store": 3, "bsc_compact_stats": 2}


def _header():
    return open(os.path.join(ROOT, "include", "bscnav.h")).read()


@pytest.mark.parametrize("name", sorted(ARGC))
def test_declared_bound_and_exported(name):
    import bsc_nav_amd
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    m = re.search(r"bsc_status\s+%s\s*\(([^)]*)\)\s*;" % name, text)
    assert m, f"{name} is not declared in bscnav.h"
    assert len(m.group(1).split(",")) == ARGC[name]
    assert name in bsc_nav_amd._lib.SIGNATURES, f"{name} has no ctypes signature"
    assert len(bsc_nav_amd._lib.SIGNATURES[name][1]) == ARGC[name]
    assert hasattr(bsc_nav_amd._lib.load(), name), f"libbscnav.so does not export {name}"


def test_policy_constants_match_the_header():
    import bsc_nav_amd
    defs = dict(re.findall(r"#define\s+(BSC_FLUSH_[A-Z]+)\s+(-?\d+)", _header()))
    assert set(defs) == {"BSC_FLUSH_DISTANCE", "BSC_FLUSH_SURPRISE"}
    L = bsc_nav_amd._lib
    assert int(defs["BSC_FLUSH_DISTANCE"]) == L.BSC_FLUSH_DISTANCE == L.FLUSH_POLICIES["dist"]
    assert int(defs["BSC_FLUSH_SURPRISE"]) == L.BSC_FLUSH_SURPRISE == L.FLUSH_POLICIES["surprise"]
