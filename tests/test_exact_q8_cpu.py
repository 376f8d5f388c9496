"""The interval of the integer screen (csrc/exact_screen_margin.hpp exact_screen_q8_interval) held to float64, in the
style of test_exact_screen_cpu.py: byte rows and queries, the exact integer distance, the recipe (Oracle.dist) and two fp32 summation
orders of it.  e == 0 exactly where the stated conditions hold, and there all three fp32 results are the integer; elsewhere e bounds
their distance from it and from the screened value.  And the order the pack kernel writes a query in is the order a narrow row has."""
import numpy as np
import pytest

from hsutil import Oracle, load_product
from test_exact_screen_cpu import left_to_right, pairwise

L2, IP = 0, 1
PAIRS = 100
# (lo, hi) of rows and of queries: u8 and i8 over their range, the two inexact cases of tests/test_gpu_exact_q8.py
RANGES = {"u8": ((0, 255), (0, 255)), "i8": ((-128, 127), (-128, 127)), "u8 far": ((0, 15), (240, 255)), "i8 ends": None}


@pytest.mark.parametrize("values", RANGES, ids=lambda v: v.replace(" ", "_"))
@pytest.mark.parametrize("d", (32, 320, 1088))
@pytest.mark.parametrize("metric", (L2, IP), ids=("l2", "ip"))
def test_interval_is_a_point_where_the_recipe_is_exact_and_bounds_it_elsewhere(metric, d, values):
    hs, rng = load_product(), np.random.default_rng(d + metric)
    if RANGES[values] is None:
        x, q = rng.choice([-128, 127], (PAIRS, d)), rng.choice([-128, 127], (PAIRS, d))
    else:
        (xl, xh), (ql, qh) = RANGES[values]
        x, q = rng.integers(xl, xh + 1, (PAIRS, d)), rng.integers(ql, qh + 1, (PAIRS, d))
    qn, xn = (q * q).sum(1), (x * x).sum(1)
    v = ((q - x) ** 2).sum(1) if metric == L2 else (q * x).sum(1)
    true = (v if metric == L2 else 1 - v).astype(np.float64)
    exact = v < 2 ** 24 if metric == L2 else np.array([int(a) * int(b) < 2 ** 48 for a, b in zip(qn, xn)])
    a, e = (np.array(t) for t in zip(*(hs.exact_screen_q8_interval(metric, d, v[i], qn[i], xn[i]) for i in range(PAIRS))))
    assert a.dtype == np.float32 and np.array_equal(e == 0, exact) and np.all(np.isfinite(e)) and np.all(e >= 0)
    qf, xf = q.astype(np.float32), x.astype(np.float32)
    recipes = [Oracle().dist(metric, qf, xf)] + [total((qf - xf) ** 2) if metric == L2 else np.float32(1) - total(qf * xf) for total in (left_to_right, pairwise)]
    for r in recipes:
        assert r.dtype == np.float32
        assert np.array_equal(r[exact].astype(np.float64), true[exact]) and np.array_equal(a[exact], r[exact])
        assert np.all(np.abs(r.astype(np.float64) - true) <= e) and np.all(np.abs(a.astype(np.float64) - r) <= e)


@pytest.mark.parametrize("d", (32, 96))
def test_pack_order_is_the_narrow_row_s(d):
    hs = load_product()
    stored, bad = hs.rows_to_narrow(np.arange(d, dtype=np.float32)[None, :], hs.HS_ROWS_U8)
    assert bad is None and np.array_equal(hs.exact_q8_pack_order(d), stored[0])
