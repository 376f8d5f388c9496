"""HS_ROWS_F8 on the host (no device): what is representable in OCP E4M3 "fn", and that the pack path writes the very byte."""
import numpy as np
import pytest

from hsutil import load_product


def e4m3_table():
    """the 256 bytes decoded per the encoding: sign, 4 exponent bits of bias 7, 3 fraction bits, subnormals k 2^-9, 0x7F / 0xFF NaN"""
    b = np.arange(256)
    sign, e, m = np.where(b & 0x80, -1.0, 1.0), (b >> 3) & 15, b & 7
    v = sign * np.where(e == 0, m * 2.0 ** -9, (1 + m / 8) * 2.0 ** (e - 7.0))
    v[[0x7F, 0xFF]] = np.nan
    return v.astype(np.float32)


@pytest.fixture(scope="module")
def hs():
    return load_product()


def test_every_finite_byte_round_trips(hs):
    assert hs.HS_ROWS_F8 == 5
    t = e4m3_table()
    finite = np.flatnonzero(~np.isnan(t)).astype(np.uint8)
    assert len(finite) == 254 and t[0x7E] == 448 and t[1] == 2.0 ** -9 and np.signbit(t[0x80]) and t[0x80] == 0
    rows = np.resize(t[finite], (16, 16))   # 256 slots: the 254 values and two of them again
    narrow, bad = hs.rows_to_narrow(rows, hs.HS_ROWS_F8)
    assert bad is None and hs.rows_representable(rows, hs.HS_ROWS_F8) is None and narrow.dtype == np.uint8
    # slot s * 2 + e of a 16-wide row holds element 2 s + e: the layout is the identity at dim 16
    assert np.array_equal(narrow, np.resize(finite, (16, 16)))
    with pytest.raises(hs.HsError) as e:   # (the new code did not open its neighbours)
        hs.rows_representable(rows, 7)
    assert e.value.status == hs.HS_ERR_INVALID


@pytest.mark.parametrize("v", [(1 + 1 / 16), 2.0 ** -9 * 1.5, 448 + 16, 449, 2.0 ** -10, np.inf, -np.inf, np.nan, 480], ids=str)
def test_values_off_the_grid_are_refused_with_their_row(hs, v):
    rows = np.resize(e4m3_table()[:0x7F], (40, 16))
    rows[23, 5] = v
    assert hs.rows_representable(rows, hs.HS_ROWS_F8) == 23 and hs.rows_to_narrow(rows, hs.HS_ROWS_F8)[1] == 23

