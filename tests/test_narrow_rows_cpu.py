"""Narrow rows (hs_index_set_row_format), the parts that need no device: what "representable" means for the u8 and fp16 row
formats (hs_rows_representable: x == (float)(T)x, NaN and +-inf never, -0.0 passes), the premise that the bench's and the smoke
run's data sets fit both formats, the register budgets of the narrow flat kernels against their fp32 twins, and the binding."""
import os
import re
import subprocess

import numpy as np
import pytest

from hsutil import ROOT, headline_data, load_product, mixture


@pytest.fixture(scope="module")
def hs():
    return load_product()


def _f32(v):
    return np.float32(v)


U8_FIT = [0.0, 255.0, -0.0, 1.0, 128.0]
U8_BAD = [256.0, -1.0, 0.5, 254.99998, np.nan, np.inf, -np.inf, 255.5, 1e9, -1e-30]
F16_FIT = [65504.0, -65504.0, 2.0 ** -24, 2.0 ** -14, 0.333251953125, -0.0, 0.0, 1.0, -2.0 ** -24, 2.0 ** -15, 1.0 + 2.0 ** -10]
F16_BAD = [65520.0, 2.0 ** -25, 0.1, 1.0 + 2.0 ** -11, np.nan, np.inf, -np.inf, 65505.0, 1e9, 2.0 ** -24 * 1.5]


@pytest.mark.parametrize("fmt_name,fit,bad", [("HS_ROWS_U8", U8_FIT, U8_BAD), ("HS_ROWS_F16", F16_FIT, F16_BAD)])
def test_rows_representable_edge_values(hs, fmt_name, fit, bad):
    fmt = getattr(hs, fmt_name)
    for v in fit:
        row = np.full((1, 16), 1.0, np.float32)
        row[0, 5] = _f32(v)
        assert hs.rows_representable(row, fmt) is None, f"{fmt_name}: {v!r} must be representable"
    for v in bad:
        row = np.full((1, 16), 1.0, np.float32)
        row[0, 11] = _f32(v)
        assert hs.rows_representable(row, fmt) == 0, f"{fmt_name}: {v!r} must not be representable"
    # every value fits fp32 rows
    assert hs.rows_representable(np.array([[np.nan, 0.1, 1e30, -3.0]], np.float32), hs.HS_ROWS_F32) is None


def test_rows_representable_matches_numpy_elementwise(hs):
    rng = np.random.default_rng(3)
    x = rng.standard_normal((4000, 16)).astype(np.float32)
    # a third of the entries rounded to fp16, some scaled into the subnormal and the overflow ranges
    m = rng.random(x.shape)
    x = np.where(m < 0.33, x.astype(np.float16).astype(np.float32), x)
    x = np.where((m >= 0.33) & (m < 0.4), (x * np.float32(2.0 ** -20)).astype(np.float32), x)
    x = np.where((m >= 0.4) & (m < 0.45), (x * np.float32(60000.0)).astype(np.float32), x)
    x = np.ascontiguousarray(x, np.float32)
    with np.errstate(over="ignore"):
        ok16 = (x.astype(np.float16).astype(np.float32) == x) & np.isfinite(x.astype(np.float16).astype(np.float32))
    y = np.ascontiguousarray(np.rint(rng.uniform(-3, 260, size=(4000, 16))).astype(np.float32))
    y[rng.random(y.shape) < 0.05] += np.float32(0.25)
    ok8 = (y >= 0) & (y <= 255) & (np.floor(y) == y)
    for fmt, data, ok in ((hs.HS_ROWS_F16, x, ok16), (hs.HS_ROWS_U8, y, ok8)):
        # element by element: a 1 x 1 matrix per value would be slow; one row per call with a single varying component
        for r in range(0, 4000, 97):
            for j in range(16):
                one = np.zeros((1, 16), np.float32)
                one[0, j] = data[r, j]
                assert (hs.rows_representable(one, fmt) is None) == bool(ok[r, j]), (fmt, data[r, j])
        # the first bad row is the first one, not any
        bad_rows = np.flatnonzero(~ok.all(axis=1))
        want = None if len(bad_rows) == 0 else int(bad_rows[0])
        assert hs.rows_representable(data, fmt) == want
        good = data[ok.all(axis=1)]
        assert hs.rows_representable(good, fmt) is None
        if len(good) > 10:
            spiked = good.copy()
            spiked[7, 3] = np.float32(0.1) if fmt == hs.HS_ROWS_F16 else np.float32(300.0)
            spiked[9, 0] = np.float32(np.nan)
            assert hs.rows_representable(spiked, fmt) == 7


def test_bench_and_smoke_data_fit_both_formats(hs):
    """The premise of the feature: the bench's data set and the smoke run's are integers in [0, 255] (with some -0.0 out of
    np.clip(np.rint(x), 0, 255)), so they fit u8 and, being below 2048, fp16."""
    for rows in (headline_data(20000, 128, 123), mixture(5000, 128, 1, integer=True)):
        assert hs.rows_representable(rows, hs.HS_ROWS_U8) is None
        assert hs.rows_representable(rows, hs.HS_ROWS_F16) is None
    assert np.signbit(headline_data(20000, 128, 123)[headline_data(20000, 128, 123) == 0]).any(), "the data no longer holds -0.0"
    assert hs.rows_representable(mixture(100, 128, 1), hs.HS_ROWS_U8) == 0        # continuous rows do not
    assert hs.rows_representable(mixture(100, 128, 1), hs.HS_ROWS_F16) == 0


def test_narrow_kernels_keep_their_fp32_twins_wave_budget():
    """resource_usage.txt: the narrow flat kernels of the compiled-in d = 128 / d = 96 shapes, both metrics, S = 1, 2: present,
    no scratch, at least the resident waves of the fp32 kernel of the same shape."""
    path = os.path.join(ROOT, "hnsw-slim_amd", "resource_usage.txt")
    if not os.path.exists(path):
        subprocess.check_call(["make", "-C", os.path.dirname(path), "-B", "libhnsw_slim_amd.so"])
    txt = open(path).read()
    kern = {}
    for m in re.finditer(r"Function Name: (\S+)\s+VGPRs: (\d+)\s+ScratchSize \[bytes/lane\]: (\d+)\s+Occupancy \[waves/SIMD\]: (\d+)", txt):
        kern[m.group(1)] = (int(m.group(2)), int(m.group(3)), int(m.group(4)))
    for metric in (0, 1):
        for s in (1, 2):
            for d16 in (8, 6):
                twin = f"_ZN2hs11flat_kernelILi{metric}ELi{s}ELi{d16}EEEvNS_8DevIndexENS_10SearchArgsE"
                assert twin in kern, f"{twin} missing from resource_usage.txt"
                for name in (f"_ZN2hs14flat_kernel_u8ILi{metric}ELi{s}ELi{d16}EEEvNS_8DevIndexENS_10SearchArgsEPKh",
                             f"_ZN2hs15flat_kernel_f16ILi{metric}ELi{s}ELi{d16}EEEvNS_8DevIndexENS_10SearchArgsEPKDF16_"):
                    assert name in kern, f"{name} missing from resource_usage.txt"
                    vgpr, scratch, occ = kern[name]
                    assert scratch == 0 and occ >= kern[twin][2], \
                        f"{name}: {vgpr} VGPRs, {scratch} B scratch, {occ} waves/SIMD (fp32 twin: {kern[twin][2]} waves/SIMD)"


def test_every_flat_shape_exists_narrow():
    """hs_index_set_row_format never changes the launch plan: every shape the fp32 flat kernel is compiled for exists as
    hs::flat_kernel_u8 and hs::flat_kernel_f16."""
    txt = open(os.path.join(ROOT, "hnsw-slim_amd", "resource_usage.txt")).read()
    shapes = set(re.findall(r"_ZN2hs11flat_kernelI(Li\d+ELi\d+ELin?\d+E)E", txt))
    assert len(shapes) == 60
    for tag in ("14flat_kernel_u8", "15flat_kernel_f16"):
        assert set(re.findall(rf"_ZN2hs{tag}I(Li\d+ELi\d+ELin?\d+E)E", txt)) == shapes, tag


def test_binding_exposes_row_formats(hs):
    assert (hs.HS_ROWS_F32, hs.HS_ROWS_F16, hs.HS_ROWS_U8) == (0, 1, 2)
    assert callable(hs.Index.set_row_format) and callable(hs.Index.row_format) and callable(hs.rows_representable)
    L = hs.lib()
    for sym in ("hs_index_set_row_format", "hs_index_row_format", "hs_rows_representable"):
        assert hasattr(L, sym) and sym in hs.EXPORTS
    hdr = open(os.path.join(ROOT, "include", "hnsw_slim_amd.h")).read()
    assert "HS_ROWS_F32 = 0, HS_ROWS_F16 = 1, HS_ROWS_U8 = 2" in hdr
    with pytest.raises(hs.HsError) as e:
        hs.rows_representable(np.zeros((2, 16), np.float32), 7)
    assert e.value.status == hs.HS_ERR_INVALID
