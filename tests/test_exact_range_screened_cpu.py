"""hs_index_exact_range_screened[_dev] without a device: the names are declared, exported and bound, the list capacity is published,
and the argument checks come before any use of the device."""
import os
import re

import numpy as np
import pytest

from hsutil import ROOT, load_product

NAMES = ("hs_index_exact_range_screened", "hs_index_exact_range_screened_dev")


@pytest.mark.parametrize("name", NAMES)
def test_name_is_declared_exported_and_bound(name):
    hs = load_product()
    hdr = open(os.path.join(ROOT, "include", "hnsw_slim_amd.h")).read()
    assert re.search(r"\b%s\s*\(" % name, hdr)
    assert name in hs.EXPORTS and hasattr(hs.lib(), name)
    assert callable(getattr(hs.Index, name[len("hs_index_"):]))
    assert int(re.search(r"#define\s+HS_EXACT_RANGE_SCREEN_LIST\s+(\d+)", hdr).group(1)) == hs.HS_EXACT_RANGE_SCREEN_LIST


# the index is null in every case: a null radius or out_offsets is refused for itself, before the index is looked at
@pytest.mark.parametrize("null,message", (("index", "null index"), ("radius", "radius, out_offsets"), ("offsets", "radius, out_offsets")))
def test_null_arguments_are_refused_before_the_device_is_touched(null, message):
    hs = load_product()
    L = hs.lib()
    f, u64 = np.zeros(16, np.float32), np.zeros(16, np.uint64)
    rad = None if null == "radius" else f.ctypes.data
    off = None if null == "offsets" else u64.ctypes.data
    assert L.hs_index_exact_range_screened(None, None, f.ctypes.data, 1, rad, None, 8, off, u64.ctypes.data, f.ctypes.data) == hs.HS_ERR_INVALID
    assert message in hs.last_error()
    assert L.hs_index_exact_range_screened_dev(None, None, f.ctypes.data, 1, rad, None, 8, off, u64.ctypes.data, f.ctypes.data, None) == hs.HS_ERR_INVALID
    assert message in hs.last_error()
