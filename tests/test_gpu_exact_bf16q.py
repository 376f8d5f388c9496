"""Exact search for bf16 queries over bf16 rows (hs_index_exact_search_bf16[_dev], csrc/exact_screen_bf16q.hip): the screen on the bf16
matrix cores, exact_screen.hip's re-rank and fallback behind it.  Every answer is compared with == on labels, fp32 bits and counts
against Index.exact_search of the widened queries (the scan, which is not the code under test)."""
import numpy as np
import pytest

from hsutil import load_product
from test_gpu_bf16_rows import bf16_rows, bf16_words
from test_gpu_exact_screen import same
from test_gpu_exact_search import filters, make_index

pytestmark = pytest.mark.gpu
N, NQ = 3000, 70   # one full tile of 64 queries and a partial one
_indexes = {}


@pytest.fixture(scope="module")
def hs():
    return load_product()


def index_of(hs, tmp_path_factory, d, metric, marks=False, huge=False):
    if (d, metric, marks, huge) not in _indexes:
        rows = bf16_rows(N, d, 300 + d, planted=8)   # (fewer far rows than a k = 1 list holds: 64 of them at the head would overflow it)
        if huge:   # squared norms of +inf and of about 2^125: rows the pre-test meets with a margin that is not finite
            rows[41] *= np.float32(2.0 ** 63)
            rows[42] *= np.float32(2.0 ** 58)
        labels = np.random.default_rng(3).permutation(N).astype(np.uint64) * 7 + 5
        ix = make_index(hs, tmp_path_factory, N, d, metric, labels, deleted=(np.arange(N) % 3 == 0).astype(np.uint8) if marks else None, rows=rows)
        if d % 16 == 0:
            ix.set_row_format(hs.HS_ROWS_BF16)
        _indexes[d, metric, marks, huge] = ix
    return _indexes[d, metric, marks, huge]


# d: one slice of the screen, several steps, a partial last slice; every k at d = 128, the others with one k each
@pytest.mark.parametrize("metric,d,k", [(m, d, k) for m in (0, 1) for d, k in ((16, 64), (128, 1), (128, 10), (128, 64), (272, 10 - 9 * m))])
def test_bf16_queries_get_the_scan_s_answers(hs, tmp_path_factory, metric, d, k):
    filtered = k == 10   # a filter per query and delete marks
    ix, q = index_of(hs, tmp_path_factory, d, metric, filtered), bf16_rows(NQ, d, 400 + d, planted=8)
    a = ()
    if filtered:
        fs = hs.FilterSet.create(ix, 5)
        fs.write(0, filters(N))
        a = (fs, (np.arange(NQ) % 5).astype(np.uint32))
    r = ix.exact_search_bf16(bf16_words(q), k, *a)
    name, st = ix.last_kernel(), ix.exact_screen_stats()
    same(r, ix.exact_search(q, k, *a), "the scan")
    assert name == "hs::xb_screen_kernel" and st["screened"] > 0 and st["screened"] + st["fell_back"] == NQ, (name, st)


@pytest.mark.parametrize("metric", (0, 1))
def test_nan_inf_subnormal_and_huge_queries_and_huge_rows(hs, tmp_path_factory, metric):
    d, k = 128, 10
    ix, q = index_of(hs, tmp_path_factory, d, metric, huge=True), bf16_rows(NQ, d, 500, planted=8)
    q[1, 3], q[4, 0] = np.nan, np.inf
    q[7] = np.float32(5 * 2.0 ** -133) * np.sign(q[7])   # nothing but bf16 subnormals
    q[9] *= np.float32(2.0 ** 62)                        # |q|^2 above 2^125: the L2 recipe overflows
    assert np.array_equal(q.view(np.uint32) & 0xFFFF, np.zeros(q.shape, np.uint32))
    r = ix.exact_search_bf16(bf16_words(q), k)
    assert ix.last_kernel() == "hs::xb_screen_kernel" and ix.exact_screen_stats()["fell_back"] > 0
    same(r, ix.exact_search(q, k), "the scan")


def test_device_entry_and_hand_over_of_dim_24(hs, tmp_path_factory):
    import torch
    k, dev = 10, torch.device("cuda:0")
    for d, kernel in ((128, "hs::xb_screen_kernel"), (24, None)):   # dim % 16 != 0: widened on the device, the fp32 queries' route
        ix, q = index_of(hs, tmp_path_factory, d, 0), bf16_rows(NQ, d, 600 + d, planted=8)
        want = ix.exact_search_screened(q, k)
        kernel = kernel or ix.last_kernel()
        same(ix.exact_search_bf16(bf16_words(q), k), want, "the host entry")
        assert ix.last_kernel() == kernel
        o = (torch.zeros((NQ, k), dtype=torch.int64, device=dev), torch.zeros((NQ, k), dtype=torch.float32, device=dev), torch.zeros(NQ, dtype=torch.int32, device=dev))
        ix.exact_search_bf16_dev(torch.from_numpy(bf16_words(q).view(np.int16)).view(torch.bfloat16).to(dev), k, *o)
        ix.check(0)
        same(dict(labels=o[0].cpu().numpy().view(np.uint64), dists=o[1].cpu().numpy(), cnt=o[2].cpu().numpy().view(np.uint32)), want, "the device entry")
        assert ix.last_kernel() == kernel


def test_an_index_without_a_bf16_copy_is_refused(hs, tmp_path_factory):
    labels = np.arange(N, dtype=np.uint64)
    plain, halves = (make_index(hs, tmp_path_factory, N, 16, 0, labels, rows=np.ones((N, 16), np.float32)) for _ in range(2))
    halves.set_row_format(hs.HS_ROWS_F16)
    for ix in (plain, halves):
        with pytest.raises(hs.HsError, match="holds no bf16 copy of its rows") as e:
            ix.exact_search_bf16(np.zeros((3, 16), np.uint16), 5)
        assert e.value.status == hs.HS_ERR_INVALID
