"""Exact search for fp16 queries over fp16 rows (hs_index_exact_search_f16[_dev], csrc/exact_screen_f16q.hip): the screen on the
half-precision matrix cores, exact_screen.hip's re-rank and fallback behind it.  Every answer is compared with == on labels, fp32 bits
and counts against Oracle.dist + a lexsort over the widened rows and queries and against Index.exact_search of the widened queries;
neither is the code under test."""
import functools

import numpy as np
import pytest

from hsutil import Oracle, load_product
from test_gpu_exact_screen import expected, same
from test_gpu_exact_search import filters, make_index

pytestmark = pytest.mark.gpu
L2, IP = 0, 1
# (n, d, nq, k, metric): one matrix step, a partial tile, several chunks; two query tiles, k at its limit; three steps, IP; just above
# one bitmap word; n < k; sliced (3.75 slices of 256, the last step of units partly filled); whole slices, k = 64; the handover
SHAPES = [(777, 16, 37, 10, L2), (2003, 128, 70, 64, L2), (1501, 48, 21, 10, IP), (40, 16, 5, 10, L2), (9, 16, 3, 10, L2),
          (333, 960, 9, 10, L2), (300, 512, 5, 64, IP), (1203, 100, 13, 10, L2)]
KINDS = ("float", "neardup", "subnormal", "wide", "alldup")
CASES = [(s, kind) for s in SHAPES for kind in KINDS if kind != "alldup" or s[0] == 2003]


@pytest.fixture(scope="module")
def hs():
    return load_product()


@pytest.fixture(scope="module")
def oracle():
    return Oracle()


@functools.lru_cache(maxsize=None)
def halves_of(kind, n, d, nq):
    """(rows, queries) as float16"""
    rng = np.random.default_rng(n + d)
    both = rng.standard_normal((n + nq, d))
    if kind == "subnormal":   # a third of the elements from the fp16 subnormals, the rest small enough for lost products to matter
        sub = rng.integers(1, 1024, both.shape) * 2.0 ** -24 * rng.choice([-1, 1], both.shape)
        both = np.where(rng.random(both.shape) < 1 / 3, sub, both * 2.0 ** -10)
    if kind == "wide":
        both = rng.choice([-1, 1], both.shape) * 2.0 ** rng.uniform(-10, 14, both.shape)
    base, q = both[:n].astype(np.float16), both[n:].astype(np.float16)
    if kind == "neardup":   # every row three times, one copy one ulp off in coordinate 0
        base = np.repeat(base[:(n + 2) // 3], 3, axis=0)[:n].copy()
        base[2::3, 0] = np.nextafter(base[2::3, 0], np.float16(np.inf))
    if kind == "alldup":
        base = np.repeat(base[:1], n, axis=0)
    return np.ascontiguousarray(base), np.ascontiguousarray(q)


def index_of(hs, tmp_path_factory, shape, kind, deleted=None):
    n, d, nq, k, metric = shape
    rows, q = halves_of(kind, n, d, nq)
    labels = np.random.default_rng(3).permutation(n).astype(np.uint64) * 7 + 5
    ix = make_index(hs, tmp_path_factory, n, d, metric, labels, deleted=deleted, rows=rows.astype(np.float32))
    if d % 16 == 0:
        ix.set_row_format(hs.HS_ROWS_F16)
    return ix, rows, q, labels


@pytest.mark.parametrize("shape,kind", CASES, ids=lambda v: str(v))
def test_fp16_queries_get_the_scan_s_answers(hs, oracle, tmp_path_factory, shape, kind):
    n, d, nq, k, metric = shape
    ix, rows, q, labels = index_of(hs, tmp_path_factory, shape, kind)
    base, qw = rows.astype(np.float32), q.astype(np.float32)
    r = ix.exact_search_f16(q, k)
    name, st = ix.last_kernel(), ix.exact_screen_stats()
    same(r, expected(oracle, metric, base, qw, k, labels), "lexsort")
    same(r, ix.exact_search(qw, k), "the scan")
    if d % 16:   # no index of such a dim holds a narrow copy: widened, the fp32 queries' route, which hands it to the scan
        assert name == "hs::exact_scan_general_kernel" and st == dict(screened=0, fell_back=0, reranked_rows=0)
        return
    assert name == "hs::xh_screen_kernel"
    assert st["screened"] + st["fell_back"] == nq, st
    if kind in ("float", "neardup"):
        assert st["fell_back"] == 0 and st["screened"] == nq and nq * min(k, n) <= st["reranked_rows"] <= nq * (min(k, n) + 16), st
    if kind == "alldup":
        assert st["fell_back"] == nq


def test_nan_inf_and_zero_queries(hs, tmp_path_factory):
    n, d, nq, k, metric = SHAPES[0]
    ix, rows, q, _ = index_of(hs, tmp_path_factory, SHAPES[0], "float")
    q = q.copy()
    q[1, 3], q[4, 0], q[7] = np.nan, np.inf, 0
    r = ix.exact_search_f16(q, k)
    assert ix.last_kernel() == "hs::xh_screen_kernel" and ix.exact_screen_stats()["fell_back"] >= 2
    same(r, ix.exact_search(q.astype(np.float32), k), "the scan")


def test_filters_per_query_and_delete_marks(hs, tmp_path_factory):
    n, d, nq, k, metric = SHAPES[0]
    ix, rows, q, _ = index_of(hs, tmp_path_factory, SHAPES[0], "float", deleted=(np.arange(n) % 3 == 0).astype(np.uint8))
    fs = hs.FilterSet.create(ix, 5)
    fs.write(0, filters(n))
    foq = (np.arange(nq) % 5).astype(np.uint32)
    r = ix.exact_search_f16(q, k, fs, foq)
    assert ix.last_kernel() == "hs::xh_screen_kernel"
    same(r, ix.exact_search(q.astype(np.float32), k, fs, foq), "the scan")


def test_device_entry_on_a_stream(hs, tmp_path_factory):
    import torch
    n, d, nq, k, metric = SHAPES[0]
    ix, rows, q, _ = index_of(hs, tmp_path_factory, SHAPES[0], "float")
    dev = torch.device("cuda:0")
    st = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(st):
        o = (torch.zeros((nq, k), dtype=torch.int64, device=dev), torch.zeros((nq, k), dtype=torch.float32, device=dev),
             torch.zeros(nq, dtype=torch.int32, device=dev))
        ix.exact_search_f16_dev(torch.from_numpy(q.copy()).to(dev), k, *o, stream=st.cuda_stream)
        ix.check(st.cuda_stream)
        got = dict(labels=o[0].cpu().numpy().view(np.uint64), dists=o[1].cpu().numpy(), cnt=o[2].cpu().numpy().view(np.uint32))
    st.synchronize()
    assert ix.last_kernel() == "hs::xh_screen_kernel" and ix.exact_screen_stats()["screened"] == nq
    same(got, ix.exact_search(q.astype(np.float32), k), "device entry")


def test_refusals(hs, tmp_path_factory):
    n, d, nq, k, metric = SHAPES[0]
    ix, rows, q, labels = index_of(hs, tmp_path_factory, SHAPES[0], "float")
    plain = make_index(hs, tmp_path_factory, n, d, metric, labels)
    bytes_ = make_index(hs, tmp_path_factory, n, d, metric, labels)
    bytes_.set_row_format(hs.HS_ROWS_U8)
    for index, queries, text in ((plain, q, "holds no fp16 copy of its rows"), (bytes_, q, "holds no fp16 copy of its rows"),
                                 (ix, q.astype(np.float32), "exact_search_f16 takes float16 queries, not float32")):
        with pytest.raises(hs.HsError) as e:
            index.exact_search_f16(queries, k)
        assert e.value.status == hs.HS_ERR_INVALID and text in str(e.value)
