"""Exact search for byte queries over byte rows (hs_index_exact_search_q8[_dev], csrc/exact_screen_q8.hip): the screen on the integer
matrix cores, exact_screen.hip's re-rank and fallback behind it.  Every answer is compared with == on labels, fp32 bits and counts
against Oracle.dist + a lexsort over the widened rows and queries and against Index.exact_search of the widened queries; neither is
the code under test."""
import functools

import numpy as np
import pytest

from hsutil import Oracle, load_product
from test_gpu_exact_screen import expected, same
from test_gpu_exact_search import filters, make_index

pytestmark = pytest.mark.gpu
L2, IP = 0, 1
# (n, d, nq, k, metric): one matrix step, a partial tile, several row chunks; more than one 64-query tile and k at its limit; three
# matrix steps; just above one bitmap word; n < k
EXACT = [(777, 32, 37, 10, L2), (2003, 128, 70, 64, L2), (1501, 96, 21, 10, IP), (40, 32, 5, 10, L2), (9, 32, 3, 10, L2)]
CASES = ([(f, s, "exact") for f in ("u8", "i8") for s in EXACT]
         + [("u8", (333, 960, 9, 10, L2), "exact"),        # staged in slices, still exact: the largest sum is 0.71 x 2^24
            ("u8", (160, 320, 9, 10, L2), "inexact"),      # every D >= 2^24
            ("i8", (300, 1088, 5, 10, IP), "inexact"),     # qn xn >= 2^48 for every pair; sliced
            ("u8", (1203, 48, 13, 10, L2), "handover")])   # dim % 32 != 0: widened, the fp32 screen's


@pytest.fixture(scope="module")
def hs():
    return load_product()


@pytest.fixture(scope="module")
def oracle():
    return Oracle()


@functools.lru_cache(maxsize=None)
def bytes_of(fmt, n, d, nq, kind):
    rng, dt = np.random.default_rng(n + d), np.uint8 if fmt == "u8" else np.int8
    if (kind, fmt) == ("inexact", "i8"):
        return rng.choice([-128, 127], (n, d)).astype(dt), rng.choice([-128, 127], (nq, d)).astype(dt)
    (rlo, rhi), (qlo, qhi) = ((0, 15), (240, 255)) if kind == "inexact" else ((0, 255),) * 2 if fmt == "u8" else ((-128, 127),) * 2
    return rng.integers(rlo, rhi + 1, (n, d)).astype(dt), rng.integers(qlo, qhi + 1, (nq, d)).astype(dt)


def index_of(hs, tmp_path_factory, fmt, shape, kind, deleted=None):
    n, d, nq, k, metric = shape
    rows, q = bytes_of(fmt, n, d, nq, kind)
    labels = np.random.default_rng(3).permutation(n).astype(np.uint64) * 7 + 5
    ix = make_index(hs, tmp_path_factory, n, d, metric, labels, deleted=deleted, rows=rows.astype(np.float32))
    ix.set_row_format(hs.HS_ROWS_U8 if fmt == "u8" else hs.HS_ROWS_I8)
    return ix, rows, q, labels


@pytest.mark.parametrize("fmt,shape,kind", CASES, ids=lambda v: str(v))
def test_byte_queries_get_the_scan_s_answers(hs, oracle, tmp_path_factory, fmt, shape, kind):
    n, d, nq, k, metric = shape
    ix, rows, q, labels = index_of(hs, tmp_path_factory, fmt, shape, kind)
    base, qw = rows.astype(np.float32), q.astype(np.float32)
    r = ix.exact_search_q8(q, k)
    name, st = ix.last_kernel(), ix.exact_screen_stats()
    same(r, expected(oracle, metric, base, qw, k, labels), "lexsort")
    same(r, ix.exact_search(qw, k), "the scan")
    if kind == "handover":
        assert name == "hs::xs_screen_kernel_u8"
        return
    assert name == f"hs::xq_screen_kernel_{fmt}"
    assert st["fell_back"] == 0 and st["screened"] == nq, st
    if kind == "exact":   # e = 0: k rows plus ties, and no query of these inputs has a tie at its k-th distance
        assert nq * min(k, n) <= st["reranked_rows"] <= nq * (min(k, n) + 16), st
    else:
        x0, q0 = rows[0].astype(np.int64), q[0].astype(np.int64)
        v = int(((q0 - x0) ** 2).sum()) if metric == L2 else int((q0 * x0).sum())
        assert hs.exact_screen_q8_interval(metric, d, v, int((q0 * q0).sum()), int((x0 * x0).sum()))[1] > 0


def test_filters_per_query_and_delete_marks(hs, tmp_path_factory):
    n, d, nq, k, metric = EXACT[0]
    ix, rows, q, _ = index_of(hs, tmp_path_factory, "u8", EXACT[0], "exact", deleted=(np.arange(n) % 3 == 0).astype(np.uint8))
    fs = hs.FilterSet.create(ix, 5)
    fs.write(0, filters(n))
    foq = (np.arange(nq) % 5).astype(np.uint32)
    r = ix.exact_search_q8(q, k, fs, foq)
    assert ix.last_kernel() == "hs::xq_screen_kernel_u8"
    same(r, ix.exact_search(q.astype(np.float32), k, fs, foq), "the scan")


def test_device_entry_on_a_stream(hs, tmp_path_factory):
    import torch
    n, d, nq, k, metric = EXACT[0]
    ix, rows, q, _ = index_of(hs, tmp_path_factory, "i8", EXACT[0], "exact")
    dev = torch.device("cuda:0")
    st = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(st):
        o = (torch.zeros((nq, k), dtype=torch.int64, device=dev), torch.zeros((nq, k), dtype=torch.float32, device=dev),
             torch.zeros(nq, dtype=torch.int32, device=dev))
        ix.exact_search_q8_dev(torch.from_numpy(q.copy()).to(dev), k, *o, stream=st.cuda_stream)
        ix.check(st.cuda_stream)
        got = dict(labels=o[0].cpu().numpy().view(np.uint64), dists=o[1].cpu().numpy(), cnt=o[2].cpu().numpy().view(np.uint32))
    st.synchronize()
    assert ix.last_kernel() == "hs::xq_screen_kernel_i8" and ix.exact_screen_stats()["screened"] == nq
    same(got, ix.exact_search(q.astype(np.float32), k), "device entry")


def test_refusals(hs, tmp_path_factory):
    n, d, nq, k, metric = EXACT[0]
    ix, rows, q, labels = index_of(hs, tmp_path_factory, "u8", EXACT[0], "exact")
    plain = make_index(hs, tmp_path_factory, n, d, metric, labels, rows=rows.astype(np.float32))
    for index, queries, text in ((ix, q.astype(np.int8), "not the format of the index's narrow copy"), (plain, q, "holds no u8 / i8 copy"),
                                 (ix, q.astype(np.float32), "uint8 or int8 queries")):
        with pytest.raises(hs.HsError) as e:
            index.exact_search_q8(queries, k)
        assert e.value.status == hs.HS_ERR_INVALID and text in str(e.value)
    with pytest.raises(hs.HsError) as e:
        ix.exact_search_q8(q, k, query_format=hs.HS_ROWS_F16)
    assert e.value.status == hs.HS_ERR_INVALID and "query_format must be HS_ROWS_U8 or HS_ROWS_I8" in str(e.value)
