"""hs_index_exact_search_wide[_dev] without a device: the names are declared, exported and bound, and the argument checks come before
any use of the device."""
import os
import re

import numpy as np
import pytest

from hsutil import ROOT, load_product

NAMES = ("hs_index_exact_search_wide", "hs_index_exact_search_wide_dev")


@pytest.mark.parametrize("name", NAMES)
def test_name_is_declared_exported_and_bound(name):
    hs = load_product()
    hdr = open(os.path.join(ROOT, "include", "hnsw_slim_amd.h")).read()
    assert re.search(r"\b%s\s*\(" % name, hdr)
    assert name in hs.EXPORTS and hasattr(hs.lib(), name)
    assert callable(getattr(hs.Index, name[len("hs_index_"):]))


def test_a_null_index_is_refused_before_the_device_is_touched():
    hs = load_product()
    L = hs.lib()
    f, l64 = np.zeros(16, np.float32).ctypes.data, np.zeros(128, np.uint64).ctypes.data
    assert L.hs_index_exact_search_wide(None, None, f, 1, 100, None, l64, f, None) == hs.HS_ERR_INVALID
    assert L.hs_index_exact_search_wide_dev(None, None, f, 1, 100, None, l64, f, None, None) == hs.HS_ERR_INVALID
    assert "null index" in hs.last_error()


@pytest.mark.parametrize("k", (0, 1025))
def test_k_beyond_the_envelope_is_refused_without_an_index(k):
    hs = load_product()
    L = hs.lib()
    f, l64 = np.zeros(16, np.float32).ctypes.data, np.zeros(128, np.uint64).ctypes.data
    assert L.hs_index_exact_search_wide(None, None, f, 1, k, None, l64, f, None) == hs.HS_ERR_UNSUPPORTED
    assert "1 <= k <= 1024" in hs.last_error()
    assert L.hs_index_exact_search_wide_dev(None, None, f, 1, k, None, l64, f, None, None) == hs.HS_ERR_UNSUPPORTED
