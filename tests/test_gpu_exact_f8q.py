"""Exact search for fp8 (E4M3) queries over fp8 rows (hs_index_exact_search_f8[_dev], csrc/exact_screen_f8q.hip): the screen on the fp8
matrix cores, exact_screen.hip's re-rank and fallback behind it.  Answers are compared with == on labels, fp32 bits, counts and
padding against Index.exact_search of the widened queries (the scan, which is not the code under test), and for small integers
against a float64 brute force."""
import numpy as np
import pytest

from hsutil import load_product
from test_f8_rows_cpu import e4m3_table
from test_gpu_exact_screen import same
from test_gpu_exact_search import filters, make_index

pytestmark = pytest.mark.gpu
T = e4m3_table()
ORDINARY = np.flatnonzero((np.abs(T) >= 0.125) & (np.abs(T) < 32) | (T == 0)).astype(np.uint8)   # no subnormals: the pre-test's pairs
INTS = np.flatnonzero((T == np.round(T)) & (np.abs(T) <= 8)).astype(np.uint8)
SUB = np.flatnonzero((T != 0) & (np.abs(T) < 2.0 ** -6)).astype(np.uint8)
_indexes = {}


@pytest.fixture(scope="module")
def hs():
    return load_product()


def index_of(hs, tmp_path_factory, key, n, d, metric, rows, marks=False):
    if (key, n, d, metric, marks) not in _indexes:
        ix = make_index(hs, tmp_path_factory, n, d, metric, np.arange(n, dtype=np.uint64) * 3 + 1, rows=T[rows],
                        deleted=(np.arange(n) % 3 == 0).astype(np.uint8) if marks else None)
        ix.set_row_format(hs.HS_ROWS_F8)
        _indexes[key, n, d, metric, marks] = ix
    return _indexes[key, n, d, metric, marks]


def pick(values, n, d, seed):
    return np.random.default_rng(seed).choice(values, (n, d))


# d: a lone partial step, a full step and a tail, two full steps, the sliced path; n: a unit and a tail, both parities and a tail, many
# units; nq: less than a tile, a tile and one; n < k in the first
SHAPES = [(16, 33, 1, 64), (16, 300, 65, 10), (80, 65, 65, 1), (80, 300, 1, 10), (128, 33, 65, 10), (128, 65, 1, 64), (128, 300, 65, 10),
          (128, 300, 65, 1), (320, 33, 1, 1), (320, 65, 65, 10), (320, 300, 65, 64)]


@pytest.mark.parametrize("metric,d,n,nq,k", [(m, *s) for m in (0, 1) for s in SHAPES])
def test_f8_queries_get_the_scan_s_answers(hs, tmp_path_factory, metric, d, n, nq, k):
    ix, qb = index_of(hs, tmp_path_factory, "ord", n, d, metric, pick(ORDINARY, n, d, n + d)), pick(ORDINARY, nq, d, 7 + d)
    r = ix.exact_search_f8(qb, k)
    name, st = ix.last_kernel(), ix.exact_screen_stats()
    same(r, ix.exact_search(T[qb], k), "the scan")
    assert name == "hs::xf_screen_kernel" and st["screened"] + st["fell_back"] == nq, (name, st)
    if n == 300:
        assert st["screened"] > 0, st   # (a screen that admits everything overflows its lists and falls back)


@pytest.mark.parametrize("metric,d", [(m, d) for m in (0, 1) for d in (80, 320)])
def test_small_integers_against_float64(hs, tmp_path_factory, metric, d):
    n, nq, k = 300, 65, 10
    xb, qb = pick(INTS, n, d, 11), pick(INTS, nq, d, 12)
    ix = index_of(hs, tmp_path_factory, "int", n, d, metric, xb)
    r = ix.exact_search_f8(qb, k)
    x, q = T[xb].astype(np.float64), T[qb].astype(np.float64)
    D = 1 - q @ x.T if metric else (q * q).sum(1)[:, None] + (x * x).sum(1)[None, :] - 2 * q @ x.T   # exact: integers below 2^53
    o = np.argsort(D, axis=1, kind="stable")
    S = np.take_along_axis(D, o, 1)
    assert np.array_equal(r["dists"].astype(np.float64), S[:, :k]) and np.all(r["cnt"] == k)
    gap = np.diff(S[:, :k + 1], axis=1) != 0
    uniq = gap & np.c_[np.ones(nq, bool), gap[:, :-1]]   # compared only where the float64 distance is distinct
    assert np.array_equal(r["labels"][uniq], (o[:, :k] * 3 + 1).astype(np.uint64)[uniq])


@pytest.mark.parametrize("kind", ("nan", "subnormal", "448", "zero", "ties"))
@pytest.mark.parametrize("metric", (0, 1))
def test_special_queries(hs, tmp_path_factory, metric, kind):
    n, d, k = 300, 320, 10
    xb = pick(ORDINARY, n, d, 21)
    xb[10:20] = pick(SUB, 10, d, 22)          # all-subnormal rows
    xb[20:24] = xb[24]                         # duplicate rows
    xb[30], xb[31] = 0x7E, 0xFE                # +448 and -448 in every component
    ix, qb = index_of(hs, tmp_path_factory, "special", n, d, metric, xb), pick(ORDINARY, 3, d, 23)
    if kind == "nan":
        qb[1, 7] = 0x7F
    elif kind != "ties":
        qb[1] = pick(SUB, 1, d, 24)[0] if kind == "subnormal" else 0x7E if kind == "448" else 0
        qb[2, ::2] = qb[1, ::2] ^ 0x80 if kind != "zero" else 0   # (both signs)
    else:
        qb[1] = xb[24]
    r = ix.exact_search_f8(qb, k)
    assert ix.last_kernel() == "hs::xf_screen_kernel" and (kind != "nan" or ix.exact_screen_stats()["fell_back"] >= 1)
    same(r, ix.exact_search(T[qb], k), "the scan")


def test_marks_filters_and_the_device_entry(hs, tmp_path_factory):
    import torch
    n, d, nq, k, dev = 300, 128, 65, 10, torch.device("cuda:0")
    ix, qb = index_of(hs, tmp_path_factory, "ord", n, d, 0, pick(ORDINARY, n, d, n + d), marks=True), pick(ORDINARY, nq, d, 31)
    fs = hs.FilterSet.create(ix, 5)
    fs.write(0, filters(n))
    foq = (np.arange(nq) % 2 * 4).astype(np.uint32)   # two filters across the queries: everything, a random tenth
    want = ix.exact_search(T[qb], k, fs, foq)
    same(ix.exact_search_f8(qb, k, fs, foq), want, "the host entry")
    o = (torch.zeros((nq, k), dtype=torch.int64, device=dev), torch.zeros((nq, k), dtype=torch.float32, device=dev), torch.zeros(nq, dtype=torch.int32, device=dev))
    ix.exact_search_f8_dev(torch.from_numpy(qb).to(dev), k, *o, fs=fs, d_filter_of_query=torch.from_numpy(foq.view(np.int32)).to(dev))
    ix.check(0)
    same(dict(labels=o[0].cpu().numpy().view(np.uint64), dists=o[1].cpu().numpy(), cnt=o[2].cpu().numpy().view(np.uint32)), want, "the device entry")

