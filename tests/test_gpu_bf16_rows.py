"""HS_ROWS_BF16 on the device.  The reference of every case is the fp32 format on the same loaded index: equal labels, distance bits,
counts and stats, no tolerance.  Rows are a Gaussian mixture truncated to bf16 (numpy has no such dtype: the words are the upper 16
bits of the fp32 value), each of the first 64 holding values no fp16 holds (1e6, 1e-30), a bf16 subnormal and a -0."""
import functools

import numpy as np
import pytest

from hsutil import load_product, mixture
from test_gpu_exact_search import make_index

pytestmark = pytest.mark.gpu
N, NQ, K = 2000, 64, 10
CAP = N + 8   # (an index that can be saved is loaded with room)
DIMS = (16, 48, 128, 960)   # the smallest; a runtime dim whose rounds end part-way; the compiled shape; long rows


@pytest.fixture(scope="module")
def hs():
    return load_product()


def bf16_words(x):
    return (np.ascontiguousarray(x, np.float32).view(np.uint32) >> 16).astype(np.uint16)


def widen(words):
    return (words.astype(np.uint32) << 16).view(np.float32)


def bf16_rows(n, d, seed, planted=64):
    x = widen(bf16_words(mixture(n, d, seed, lo=-4, hi=4, sigma=1.0)))
    rng = np.random.default_rng(seed)
    for i in range(min(n, planted)):
        x[i, rng.permutation(d)[:4]] = widen(bf16_words(np.float32([1e6, 1e-30, 3 * 2.0 ** -133, -0.0])))
    return x


@pytest.fixture(scope="module")
def graphs(hs, tmp_path_factory):
    @functools.lru_cache(maxsize=None)
    def make(d, metric, n=N):
        g = dict(base=bf16_rows(n, d, 100 + d), q=bf16_rows(NQ, d, 200 + d), path=str(tmp_path_factory.mktemp("bf16") / "g.bin"))
        hs.build_hnsw_batched(g["base"], g["path"], metric=metric, M=8, ef_construction=40, threads=4)
        return g
    return make


def answers(hs, ix, q, n=N):
    """[(kernel, labels, distance bits, counts, stats)]: the default search, a filter set, exact order, delete marks"""
    out, marked = [], np.arange(0, n, 7)
    fs = hs.FilterSet.create(ix, 2)
    fs.write(0, np.stack([np.arange(n) % 3 != 0, np.arange(n) % 2 == 0]).astype(np.uint8))
    ix.set_ef(64)
    for mode in ("flat", "filter", "order", "marks"):
        ix.set_exact_order(mode == "order")
        if mode == "marks":
            ix.mark_deleted(marked)
        r = ix.search_filter_set(q, K, fs, np.arange(len(q), dtype=np.uint32) % 2, want_stats=True) if mode == "filter" else ix.search_pq(q, K, want_stats=True)
        keep = np.arange(K)[None, :] < r["cnt"][:, None]
        out.append((ix.last_kernel(), np.where(keep, r["labels"], 0), np.where(keep, r["dists"].view(np.uint32), 0), r["cnt"], r["stats"]))
    ix.mark_deleted(marked, on=False)
    return out


def same(got, want, narrow, what):
    for i, (g, w) in enumerate(zip(got, want)):
        assert g[0] == w[0] + ("_bf16" if i in narrow else ""), f"{what}, mode {i}: ran {g[0]}"
        assert all(np.array_equal(a, b) for a, b in zip(g[1:], w[1:])), f"{what}, mode {i} ({g[0]}) differs from the fp32 format"


@pytest.mark.parametrize("d,metric", [(d, m) for d in DIMS for m in (0, 1) if d >= 128 or m == (d == 48)])   # both metrics where a dim is compiled in
def test_search_kernels_and_exact_search_read_bf16_rows(hs, graphs, d, metric, tmp_path):
    g = graphs(d, metric)
    base, q = g["base"], g["q"]
    ix = hs.Index(g["path"], hs.HS_KIND_HNSW, d, metric=metric, max_elements=CAP)
    want, bytes_f32 = answers(hs, ix, q), ix.info()["device_bytes"]
    assert [w[0] for w in want] == ["hs::flat_kernel", "hs::fast_kernel", "hs::strict_kernel", "hs::fast_kernel"]
    fs = hs.FilterSet.create(ix, 2)
    fs.write(0, np.stack([np.arange(N) % 10 == 3, np.arange(N) % 2 == 0]).astype(np.uint8))
    ix.mark_deleted(np.arange(0, N, 5))
    xargs = ((), (fs, np.arange(NQ, dtype=np.uint32) % 2))
    xwant = [ix.exact_search(q, K, *a) for a in xargs]
    ix.mark_deleted(np.arange(0, N, 5), on=False)
    ix.set_row_format(hs.HS_ROWS_BF16)
    same(answers(hs, ix, q), want, (0,), "bf16 beside fp32")
    ix.set_f32_resident(False)
    ix.save(str(tmp_path / "saved.bin"))
    nx = hs.Index.load_narrow(str(tmp_path / "saved.bin"), hs.HS_KIND_HNSW, d, hs.HS_ROWS_BF16, metric=metric, max_elements=CAP)
    assert nx.info() == ix.info() and nx.info()["device_bytes"] == bytes_f32 - 2 * CAP * d and nx.row_format() == hs.HS_ROWS_BF16 and not nx.f32_resident()
    for x, what in ((ix, "fp32 rows dropped"), (nx, "load_narrow")):
        same(answers(hs, x, q), want, range(4), what)
        assert all(x.get_row(lab).tobytes() == base[lab].tobytes() for lab in (0, 63, N - 1))
    ix.mark_deleted(np.arange(0, N, 5))
    for a, w in zip(xargs, xwant):
        for call, kernel in ((ix.exact_search, "hs::exact_scan_kernel_bf16"), (ix.exact_search_screened, "hs::xs_screen_kernel_bf16")):
            r = call(q, K, *a)
            assert ix.last_kernel() == kernel and all(r[key].tobytes() == w[key].tobytes() for key in ("cnt", "labels", "dists")), (kernel, len(a))


def test_live_updates_write_the_bf16_copy(hs, graphs, tmp_path):
    n, extra, d = 600, 20, 32
    g = graphs(d, 0, n)
    q, more, new = g["q"], bf16_rows(extra, d, 7), bf16_rows(3, d, 8)
    ix, fx = (hs.Index(g["path"], hs.HS_KIND_HNSW, d, max_elements=n + extra) for _ in range(2))
    ix.set_row_format(hs.HS_ROWS_BF16)
    ix.set_f32_resident(False)
    bad = more[:3].copy()
    bad[1, 5] = np.float32(1 + 2.0 ** -9)
    with pytest.raises(hs.HsError, match="row 1 .*component 5.*HS_ROWS_BF16"):
        ix.add_points(bad, np.arange(n, n + 3))
    for x in (ix, fx):
        x.seed_levels(100, n)
        x.add_points(more, np.arange(n, n + extra))
        x.upsert_points(new, [5, n + 1, 300])
        x.mark_deleted([8, n + 4])   # (neither is among the labels answers() marks)
        x.save(str(tmp_path / ("bf16" if x is ix else "f32")))
    assert open(tmp_path / "bf16", "rb").read() == open(tmp_path / "f32", "rb").read()
    assert all(ix.get_row(lab).tobytes() == row.tobytes() for lab, row in zip((5, n + 1, 300, n + 3), (*new, more[3])))
    same(answers(hs, ix, q, n + extra), answers(hs, fx, q, n + extra), range(4), "after the updates")


def test_refusals(hs, tmp_path, tmp_path_factory):
    for v in (np.float32(1 + 2.0 ** -9), np.float32(np.inf), np.float32(np.nan)):
        rows = bf16_rows(300, 16, 9)
        rows[123, 7] = v
        assert hs.rows_representable(rows, hs.HS_ROWS_BF16) == 123 and hs.rows_to_narrow(rows, hs.HS_ROWS_BF16)[1] == 123
        ix = make_index(hs, tmp_path_factory, 300, 16, 0, np.arange(300, dtype=np.uint64), rows=rows)   # (rows loaded as given: the device check meets them)
        with pytest.raises(hs.HsError, match="row 123 .*component 7") as e:
            ix.set_row_format(hs.HS_ROWS_BF16)
        assert e.value.status == hs.HS_ERR_UNSUPPORTED and ix.row_format() == hs.HS_ROWS_F32
    rows = bf16_rows(300, 16, 9)
    assert hs.rows_representable(rows, hs.HS_ROWS_BF16) is None
    with pytest.raises(hs.HsError, match="bad row format") as e:
        hs.build_hnsw_batched_rows(bf16_words(rows), str(tmp_path / "b.bin"), M=8, ef_construction=40, row_format=hs.HS_ROWS_BF16)
    assert e.value.status == hs.HS_ERR_INVALID
