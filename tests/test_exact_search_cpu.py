"""Exact search on a resident index (hs_index_exact_search[_dev]), the parts that need no device: the symbols are bound, a null
handle is refused before any device is touched, and the compiler's resource report holds the new scan kernels
(csrc/exact_search.hip) with no more scratch per lane than the exhaustive scan they share their geometry with
(hs::bf_scan_kernel, csrc/brute_force.hip) for the same metric."""
import numpy as np
import pytest

from hsutil import load_product
from test_f32_free_cpu import _report


@pytest.fixture(scope="module")
def hs():
    return load_product()


def test_exact_search_calls_are_bound(hs):
    lib = hs.lib()
    for name in ("hs_index_exact_search", "hs_index_exact_search_dev"):
        assert name in hs.EXPORTS and hasattr(lib, name)
    assert hasattr(hs.Index, "exact_search") and hasattr(hs.Index, "exact_search_dev")


def test_null_handle_is_refused_without_a_device(hs):
    lib = hs.lib()
    q, ol, od = np.zeros((2, 16), np.float32), np.zeros((2, 3), np.uint64), np.zeros((2, 3), np.float32)
    assert lib.hs_index_exact_search(None, None, q.ctypes.data, 2, 3, None, ol.ctypes.data, od.ctypes.data, None) == hs.HS_ERR_INVALID
    assert lib.hs_last_error().decode() == "null index"
    assert lib.hs_index_exact_search_dev(None, None, q.ctypes.data, 2, 3, None, ol.ctypes.data, od.ctypes.data, None, None) == hs.HS_ERR_INVALID
    assert lib.hs_index_exact_search(None, None, q.ctypes.data, 0, 3, None, ol.ctypes.data, od.ctypes.data, None) == hs.HS_ERR_INVALID


@pytest.mark.parametrize("metric", (0, 1))
def test_scan_kernels_are_reported_and_spill_no_more_than_bf_scan(metric):
    kern = _report()
    bf = kern[f"_ZN2hs14bf_scan_kernelILi{metric}EEEvPKfPKmjjS2_jjjPNS_7BfEntryE"]
    for name in ("17exact_scan_kernel", "20exact_scan_kernel_u8", "21exact_scan_kernel_f16", "25exact_scan_general_kernel"):
        full = f"_ZN2hs{name}ILi{metric}EEEvNS_9ExactScanE"
        assert full in kern, f"{full} missing from resource_usage.txt"
        assert kern[full][1] <= bf[1], f"{full}: {kern[full][1]} bytes of scratch per lane, bf_scan_kernel {bf[1]}"
