"""HS_ROWS_I8 without a device: the values it takes, the first offending row and element, the stored form of hs_rows_to_narrow."""
import numpy as np
import pytest

from hsutil import load_product


@pytest.fixture(scope="module")
def hs():
    return load_product()


def test_code_and_accepted_values(hs):
    rows = np.tile(np.array([-128, -1, -0.0, 0, 127, 5, -77, 1], np.float32), (3, 4))
    assert hs.HS_ROWS_I8 == 3 and hs.rows_representable(rows, hs.HS_ROWS_I8) is None and hs.rows_representable(rows, hs.HS_ROWS_U8) == 0


@pytest.mark.parametrize("bad", (-129.0, 128.0, 0.5, np.nan, np.inf))
def test_first_offending_row_and_element(hs, bad):
    rows = np.full((5, 16), -3.0, np.float32)
    rows[2, 11] = rows[4, 0] = bad
    assert hs.rows_representable(rows, hs.HS_ROWS_I8) == 2 and hs.rows_to_narrow(rows, hs.HS_ROWS_I8)[1] == 2
    assert hs.rows_representable(rows[2:3, :11], hs.HS_ROWS_I8) is None and hs.rows_representable(rows[2:3, :12], hs.HS_ROWS_I8) == 0


@pytest.mark.parametrize("d", (16, 208))
def test_stored_form_is_the_signed_byte_at_narrow_slot(hs, d):
    rows = np.random.default_rng(d).integers(-128, 128, (7, d)).astype(np.float32)
    out, bad = hs.rows_to_narrow(rows, hs.HS_ROWS_I8)
    j = np.arange(d)
    assert bad is None and out.dtype == np.int8 and np.array_equal(out[:, (j // 2 % 8) * (d // 8) + 2 * (j // 16) + j % 2], rows)
