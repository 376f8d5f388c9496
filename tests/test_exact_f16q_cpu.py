"""The margin of the half-precision screen (csrc/exact_screen_margin.hpp exact_screen_f16_margin) held to float64, in
the style of test_exact_screen_cpu.py: pairs of fp16 vectors, the recipe (Oracle.dist) over their fp32 values, and the screened value
emulated in fp32 under every model the margin allows the matrix pipeline -- two summation orders, additions rounded to nearest or
truncated toward zero (one ulp off), subnormal inputs read or flushed to zero.  The norms are fp32 code of the project's own and
always see the values as they are."""
import numpy as np
import pytest

from hsutil import Oracle, load_product

L2, IP = 0, 1
PAIRS = 100


def add(a, b, trunc):
    """fp32 a + b, rounded to nearest or toward zero"""
    exact = a.astype(np.float64) + b.astype(np.float64)
    r = exact.astype(np.float32)
    return np.where(np.abs(r.astype(np.float64)) > np.abs(exact), np.nextafter(r, np.float32(0)), r) if trunc else r


def total(t, pairwise, trunc):
    t = t.astype(np.float32)
    if not pairwise:
        s = t[:, 0]
        for i in range(1, t.shape[1]):
            s = add(s, t[:, i], trunc)
        return s
    while t.shape[1] > 1:
        if t.shape[1] & 1:
            t = np.concatenate([t, np.zeros((t.shape[0], 1), np.float32)], axis=1)
        t = add(t[:, 0::2], t[:, 1::2], trunc)
    return t[:, 0]


def halves(rng, d, kind):
    v = rng.standard_normal((PAIRS, d)) + (100.0 if kind == "plus100" else 0.0)
    if kind == "subnormal":
        sub = rng.integers(1, 1024, v.shape) * 2.0 ** -24 * rng.choice([-1, 1], v.shape)
        v = np.where(rng.random(v.shape) < 1 / 3, sub, v * 2.0 ** -10)
    return v.astype(np.float16)


@pytest.mark.parametrize("kind", ("gauss", "plus100", "subnormal"))
@pytest.mark.parametrize("d", (16, 128, 960))
@pytest.mark.parametrize("metric", (L2, IP), ids=("l2", "ip"))
def test_margin_bounds_the_screened_value_under_every_model(metric, d, kind):
    hs, rng = load_product(), np.random.default_rng(d + metric)
    qh, xh = halves(rng, d, kind), halves(rng, d, kind)
    q, x = qh.astype(np.float32), xh.astype(np.float32)
    subnormal = lambda h: (h != 0) & (np.abs(h) < np.float16(2.0 ** -14))
    mq, mx = subnormal(qh).sum(1), subnormal(xh).sum(1)
    assert (kind == "subnormal") == bool(mq.mean() > 1 and mx.mean() > 1)
    r = Oracle().dist(metric, q, x).astype(np.float64)
    for pairwise in (False, True):
        qn, xn = total(q * q, pairwise, False), total(x * x, pairwise, False)
        e = np.array([hs.exact_screen_f16_margin(metric, d, qn[i], xn[i], mq[i], mx[i]) for i in range(PAIRS)], np.float64)
        assert np.all(np.isfinite(e)) and np.all(e >= 0)
        plain = np.array([hs.exact_screen_margin(metric, d, qn[i], xn[i]) for i in range(PAIRS)], np.float64)
        assert np.array_equal(e[(mq | mx) == 0], plain[(mq | mx) == 0]) and np.all(e[(mq | mx) != 0] > plain[(mq | mx) != 0])
        for trunc in (False, True):
            for flush in (False, True):
                qs, xs = (np.where(subnormal(qh), np.float32(0), q), np.where(subnormal(xh), np.float32(0), x)) if flush else (q, x)
                dot = total(qs * xs, pairwise, trunc)   # (a product of two halves is exact in fp32)
                a = (qn + xn) - np.float32(2) * dot if metric == L2 else np.float32(1) - dot
                assert a.dtype == np.float32
                worst = float(np.max(np.abs(a.astype(np.float64) - r) / e))
                assert worst <= 1, (pairwise, trunc, flush, worst)
