"""The margin of the screened exact search (csrc/exact_screen_margin.hpp) held to float64: for a screened value a --
fp32 norms and an fp32 dot product, emulated here under two summation orders -- and the recipe's distance r (Oracle.dist),
|a - r| <= e must hold, e finite and non-negative.  Gaussian rows, and the same rows shifted by +100 (norms that dwarf the distance)."""
import numpy as np
import pytest

from hsutil import Oracle, load_product

L2, IP = 0, 1
PAIRS = 300


def left_to_right(t):
    return np.cumsum(t, axis=1, dtype=np.float32)[:, -1]


def pairwise(t):
    t = t.astype(np.float32)
    while t.shape[1] > 1:
        if t.shape[1] & 1:
            t = np.concatenate([t, np.zeros((t.shape[0], 1), np.float32)], axis=1)
        t = t[:, 0::2] + t[:, 1::2]
    return t[:, 0]


@pytest.mark.parametrize("shift", (0.0, 100.0), ids=("gauss", "plus100"))
@pytest.mark.parametrize("d", (16, 128, 960))
@pytest.mark.parametrize("metric", (L2, IP), ids=("l2", "ip"))
def test_margin_bounds_the_screened_value(metric, d, shift):
    hs, rng = load_product(), np.random.default_rng(d + metric)
    q = (rng.standard_normal((PAIRS, d)) + shift).astype(np.float32)
    x = (rng.standard_normal((PAIRS, d)) + shift).astype(np.float32)
    r = Oracle().dist(metric, q, x).astype(np.float64)
    for total in (left_to_right, pairwise):
        qn, xn, dot = total(q * q), total(x * x), total(q * x)
        a = (qn + xn) - np.float32(2) * dot if metric == L2 else np.float32(1) - dot
        assert a.dtype == np.float32
        e = np.array([hs.exact_screen_margin(metric, d, qn[i], xn[i]) for i in range(PAIRS)], np.float64)
        assert np.all(np.isfinite(e)) and np.all(e >= 0)
        assert np.all(np.abs(a.astype(np.float64) - r) <= e), (total.__name__, float(np.max(np.abs(a - r) / e)))


def test_margin_gives_up_where_the_recipe_may_overflow():
    hs = load_product()
    for metric in (L2, IP):
        assert np.isposinf(hs.exact_screen_margin(metric, 16, np.float32(2.0 ** 126), np.float32(2.0 ** 126)))
        assert np.isposinf(hs.exact_screen_margin(metric, 16, np.float32(np.nan), np.float32(1)))
        assert np.isposinf(hs.exact_screen_margin(metric, 16, np.float32(np.inf), np.float32(1)))
