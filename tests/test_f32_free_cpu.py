"""fp32-free indexes (hs_index_set_f32_resident, hs_index_load_narrow), the parts that need no device: the host-side conversion
hs_rows_to_narrow against a numpy restatement of the lane-major layout (csrc/narrow_rows.hpp narrow_slot), its first_bad report and
status codes, and the compiler's resource report -- every kernel that existed before the strict / fast kernels were compiled for
narrow rows keeps its VGPR / scratch / occupancy line (tests/golden/resource_usage_before_f32_free.txt: name, VGPRs, scratch
bytes per lane, waves per SIMD of the build without them), and every required narrow shape is there."""
import os
import re
import subprocess

import numpy as np
import pytest

from hsutil import ROOT, load_product, mixture


@pytest.fixture(scope="module")
def hs():
    return load_product()


def narrow_slots(dim):
    """slot of element j of a row: j = 16 i + 2 s + e -> s * (dim / 8) + 2 i + e"""
    j = np.arange(dim)
    i, s, e = j >> 4, (j >> 1) & 7, j & 1
    return s * (dim >> 3) + 2 * i + e


def restated(rows, fmt_dtype):
    out = np.zeros(rows.shape, fmt_dtype)
    out[:, narrow_slots(rows.shape[1])] = rows.astype(fmt_dtype)
    return out


def fitting_rows(hs, fmt, n, d, seed):
    if fmt == hs.HS_ROWS_U8:
        rows = np.ascontiguousarray(np.random.default_rng(seed).integers(0, 256, size=(n, d)).astype(np.float32))
    else:
        rows = np.ascontiguousarray(mixture(n, d, seed, lo=-2, hi=2, sigma=0.7).astype(np.float16).astype(np.float32))
        rows[0, :4] = [2.0 ** -24, -0.0, 65504.0, -65504.0]
    assert hs.rows_representable(rows, fmt) is None
    return rows


@pytest.mark.parametrize("fmt_name,dtype", [("HS_ROWS_U8", np.uint8), ("HS_ROWS_F16", np.float16)])
@pytest.mark.parametrize("d", (16, 48, 128, 320, 960))
def test_rows_to_narrow_is_the_lane_major_layout(hs, d, fmt_name, dtype):
    fmt = getattr(hs, fmt_name)
    rows = fitting_rows(hs, fmt, 37, d, 5 + d)
    got, bad = hs.rows_to_narrow(rows, fmt)
    assert bad is None and got.dtype == dtype
    assert got.tobytes() == restated(rows, dtype).tobytes()
    # the slots are a permutation of the row, and lane s's elements of every step are one contiguous chunk of dim / 8 values
    assert sorted(narrow_slots(d).tolist()) == list(range(d))
    for s in range(8):
        chunk = [16 * i + 2 * s + e for i in range(d // 16) for e in (0, 1)]
        assert narrow_slots(d)[chunk].tolist() == list(range(s * d // 8, (s + 1) * d // 8))


@pytest.mark.parametrize("fmt_name,dtype,value", [("HS_ROWS_U8", np.uint8, 255.5), ("HS_ROWS_U8", np.uint8, -1.0), ("HS_ROWS_F16", np.float16, 0.1),
                                                  ("HS_ROWS_F16", np.float16, 65520.0), ("HS_ROWS_U8", np.uint8, np.nan), ("HS_ROWS_F16", np.float16, np.nan)])
def test_rows_to_narrow_reports_the_first_bad_row_and_stops_there(hs, fmt_name, dtype, value):
    fmt = getattr(hs, fmt_name)
    d, n, bad_row = 48, 60, 23
    rows = fitting_rows(hs, fmt, n, d, 11)
    rows[bad_row, 31] = np.float32(value)
    rows[bad_row + 9, 2] = np.float32(value)   # (a later offender: the first one is reported)
    sentinel = np.full((n, d), 0x5A if dtype == np.uint8 else 7.0, dtype)
    out = sentinel.copy()
    got, bad = hs.rows_to_narrow(rows, fmt, out=out)
    assert bad == bad_row
    assert got[:bad_row].tobytes() == restated(rows[:bad_row], dtype).tobytes()
    assert got[bad_row + 1:].tobytes() == sentinel[bad_row + 1:].tobytes(), "rows past the bad row were written"
    assert hs.rows_representable(rows, fmt) == bad_row


def test_rows_to_narrow_accepts_negative_zero(hs):
    for fmt, dtype in ((hs.HS_ROWS_U8, np.uint8), (hs.HS_ROWS_F16, np.float16)):
        rows = np.zeros((3, 16), np.float32)
        rows[1, 7] = np.float32(-0.0)
        assert np.signbit(rows[1, 7])
        got, bad = hs.rows_to_narrow(rows, fmt)
        assert bad is None
        slot = int(narrow_slots(16)[7])
        if dtype == np.uint8:
            assert not got.any()
        else:
            assert np.signbit(got[1, slot]) and got[1, slot] == 0 and not np.signbit(np.delete(got.ravel(), 16 + slot)).any()


def test_rows_to_narrow_status_codes(hs):
    rows = np.zeros((2, 16), np.float32)
    for bad_fmt in (hs.HS_ROWS_F32, 9, -1):
        with pytest.raises(hs.HsError) as e:
            hs.rows_to_narrow(rows, bad_fmt, out=np.zeros((2, 16), np.float16))
        assert e.value.status == hs.HS_ERR_INVALID
    for d in (20, 8, 100):
        with pytest.raises(hs.HsError) as e:
            hs.rows_to_narrow(np.zeros((2, d), np.float32), hs.HS_ROWS_U8)
        assert e.value.status == hs.HS_ERR_UNSUPPORTED
    got, bad = hs.rows_to_narrow(np.zeros((0, 32), np.float32), hs.HS_ROWS_U8)
    assert bad is None and got.shape == (0, 32)


def test_residency_calls_are_bound(hs):
    lib = hs.lib()
    for name in ("hs_index_set_f32_resident", "hs_index_f32_resident", "hs_rows_to_narrow", "hs_index_load_narrow"):
        assert hasattr(lib, name)
    assert lib.hs_index_set_f32_resident(None, 0) == hs.HS_ERR_INVALID and lib.hs_index_f32_resident(None) == 1


# ---- the compiler's resource report ---------------------------------------------------------------------------------------------
def _report():
    path = os.path.join(ROOT, "hnsw-slim_amd", "resource_usage.txt")
    if not os.path.exists(path):
        subprocess.check_call(["make", "-C", os.path.dirname(path), "-B", "libhnsw_slim_amd.so"])
    kern = {}
    for m in re.finditer(r"Function Name: (\S+)\s+VGPRs: (\d+)\s+ScratchSize \[bytes/lane\]: (\d+)\s+Occupancy \[waves/SIMD\]: (\d+)", open(path).read()):
        kern[m.group(1)] = (int(m.group(2)), int(m.group(3)), int(m.group(4)))
    return kern


def test_every_earlier_kernel_keeps_its_resource_line():
    kern = _report()
    before = [l.split() for l in open(os.path.join(ROOT, "tests", "golden", "resource_usage_before_f32_free.txt")).read().splitlines() if l.strip()]
    assert len(before) > 300
    changed = [(name, (int(v), int(s), int(o)), kern.get(name)) for name, v, s, o in before if kern.get(name) != (int(v), int(s), int(o))]
    assert not changed, f"{len(changed)} kernels moved, e.g. {changed[:3]}"


def test_required_narrow_strict_and_fast_shapes_exist():
    """strict x {L2, IP}; fast x {L2, IP} x S in {1, 2, 4, 8} x {bare, !bare} and the two ef == k shapes; all at the runtime dim,
    for u8 and fp16."""
    kern = _report()
    for tag, arg in (("u8", "PKh"), ("f16", "PKDF16_")):
        for metric in (0, 1):
            want = [f"_ZN2hs{13 + len(tag) + 1}strict_kernel_{tag}ILi{metric}EEEvNS_8DevIndexENS_10SearchArgsE{arg}"]
            shapes = [(s, 0, bare) for s in (1, 2, 4, 8) for bare in (0, 1)] + [(1, 1, 1), (2, 1, 1)]
            want += [f"_ZN2hs{11 + len(tag) + 1}fast_kernel_{tag}ILi{metric}ELi{s}ELi0ELb{wb}ELb{bare}EEEvNS_8DevIndexENS_10SearchArgsE{arg}"
                     for s, wb, bare in shapes]
            for name in want:
                assert name in kern, f"{name} missing from resource_usage.txt"
