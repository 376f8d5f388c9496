"""HS_ROWS_F8 on the device.  The reference of every case is the fp32 format on the same loaded index: equal labels, distance bits,
counts and stats, no tolerance.  Rows are random finite E4M3 bytes (both signs, subnormals and -0 among them) through the decode table."""
import functools

import numpy as np
import pytest

from hsutil import load_product
from test_f8_rows_cpu import e4m3_table
from test_gpu_bf16_rows import K, answers
from test_gpu_exact_search import make_index

pytestmark = pytest.mark.gpu
N, NQ = 600, 64
CAP = N + 8
T = e4m3_table()
FINITE = np.flatnonzero(~np.isnan(T)).astype(np.uint8)


def f8_bytes(n, d, seed):
    return np.random.default_rng(seed).choice(FINITE, (n, d))


@pytest.fixture(scope="module")
def hs():
    return load_product()


@pytest.fixture(scope="module")
def graphs(hs, tmp_path_factory):
    @functools.lru_cache(maxsize=None)
    def make(d, metric):
        g = dict(base=T[f8_bytes(N, d, 100 + d)], q=T[f8_bytes(NQ, d, 200 + d)], path=str(tmp_path_factory.mktemp("f8") / "g.bin"))
        hs.build_hnsw_batched(g["base"], g["path"], metric=metric, M=8, ef_construction=40, threads=4)
        return g
    return make


def same(got, want, narrow, what):
    for i, (g, w) in enumerate(zip(got, want)):
        assert g[0] == w[0] + ("_f8" if i in narrow else ""), f"{what}, mode {i}: ran {g[0]}"
        assert all(np.array_equal(a, b) for a, b in zip(g[1:], w[1:])), f"{what}, mode {i} ({g[0]}) differs from the fp32 format"


@pytest.mark.parametrize("metric", (0, 1))
def test_all_256_bytes_decode_on_the_device(hs, tmp_path_factory, metric):
    """16 rows x dim 16 hold every byte (the two NaN bytes replaced by 0x3C); v_cvt_pk_f32_fp8 in the kernels against the OCP decode"""
    b = np.arange(256, dtype=np.uint8).reshape(16, 16)
    b[b & 0x7F == 0x7F] = 0x3C
    q = T[f8_bytes(NQ, 16, 5)]
    ix = make_index(hs, tmp_path_factory, 16, 16, metric, np.arange(16, dtype=np.uint64), rows=T[b])
    want, xwant = ix.search_pq(q, K), ix.exact_search(q, K)
    ix.set_row_format(hs.HS_ROWS_F8)
    ix.set_f32_resident(False)
    assert all(ix.get_row(r).tobytes() == T[b[r]].tobytes() for r in range(16))
    got, xgot = ix.search_pq(q, K), ix.exact_search(q, K)
    assert ix.last_kernel() == "hs::exact_scan_kernel_f8"
    for g, w in ((got, want), (xgot, xwant)):
        keep = np.arange(K)[None, :] < w["cnt"][:, None]
        assert all(np.array_equal(np.where(keep, g[key].view(np.uint32 if key == "dists" else g[key].dtype), 0),
                                  np.where(keep, w[key].view(np.uint32 if key == "dists" else w[key].dtype), 0)) for key in ("labels", "dists"))
        assert np.array_equal(g["cnt"], w["cnt"])


@pytest.mark.parametrize("metric,d", [(m, d) for m in (0, 1) for d in (16, 128, 320)])
def test_search_kernels_and_exact_search_read_f8_rows(hs, graphs, d, metric, tmp_path):
    g = graphs(d, metric)
    base, q = g["base"], g["q"]
    ix = hs.Index(g["path"], hs.HS_KIND_HNSW, d, metric=metric, max_elements=CAP)
    want, bytes_f32 = answers(hs, ix, q, N), ix.info()["device_bytes"]
    assert [w[0] for w in want] == ["hs::flat_kernel", "hs::fast_kernel", "hs::strict_kernel", "hs::fast_kernel"]
    ix.mark_deleted(np.arange(0, N, 5))
    xwant = ix.exact_search(q, K)
    ix.mark_deleted(np.arange(0, N, 5), on=False)
    ix.set_row_format(hs.HS_ROWS_F8)
    same(answers(hs, ix, q, N), want, (0,), "f8 beside fp32")
    ix.set_f32_resident(False)
    ix.save(str(tmp_path / "saved.bin"))
    nx = hs.Index.load_narrow(str(tmp_path / "saved.bin"), hs.HS_KIND_HNSW, d, hs.HS_ROWS_F8, metric=metric, max_elements=CAP)
    assert nx.info() == ix.info() and nx.info()["device_bytes"] == bytes_f32 - 3 * CAP * d and nx.row_format() == hs.HS_ROWS_F8 and not nx.f32_resident()
    for x, what in ((ix, "fp32 rows dropped"), (nx, "load_narrow")):
        same(answers(hs, x, q, N), want, range(4), what)
        assert all(x.get_row(lab).tobytes() == base[lab].tobytes() for lab in (0, 63, N - 1))
    ix.mark_deleted(np.arange(0, N, 5))
    for call, kernel in ((ix.exact_search, "hs::exact_scan_kernel_f8"), (ix.exact_search_screened, "hs::xs_screen_kernel_f8")):
        r = call(q, K)
        assert ix.last_kernel() == kernel and all(r[key].tobytes() == xwant[key].tobytes() for key in ("cnt", "labels", "dists")), kernel


def test_live_updates_write_the_f8_copy(hs, graphs, tmp_path):
    d, extra = 16, 20
    g = graphs(d, 0)
    more, new = T[f8_bytes(extra, d, 7)], T[f8_bytes(3, d, 8)]
    ix, fx = (hs.Index(g["path"], hs.HS_KIND_HNSW, d, max_elements=N + extra) for _ in range(2))
    ix.set_row_format(hs.HS_ROWS_F8)
    ix.set_f32_resident(False)
    bad = more[:3].copy()
    bad[1, 5] = np.float32(1 + 1 / 16)
    with pytest.raises(hs.HsError, match="row 1 .*component 5.*HS_ROWS_F8"):
        ix.add_points(bad, np.arange(N, N + 3))
    for x in (ix, fx):
        x.seed_levels(100, N)
        x.add_points(more, np.arange(N, N + extra))
        x.upsert_points(new, [5, N + 1, 300])
        x.save(str(tmp_path / ("f8" if x is ix else "f32")))
    assert open(tmp_path / "f8", "rb").read() == open(tmp_path / "f32", "rb").read()
    assert all(ix.get_row(lab).tobytes() == row.tobytes() for lab, row in zip((5, N + 1, 300, N + 3), (*new, more[3])))
    same(answers(hs, ix, g["q"], N + extra), answers(hs, fx, g["q"], N + extra), range(4), "after the updates")


def test_refusals(hs, tmp_path, tmp_path_factory):
    rows = T[f8_bytes(300, 16, 9)]
    with pytest.raises(hs.HsError, match="bad row format") as e:
        hs.build_hnsw_batched_rows(f8_bytes(300, 16, 9), str(tmp_path / "b.bin"), M=8, ef_construction=40, row_format=hs.HS_ROWS_F8)
    assert e.value.status == hs.HS_ERR_INVALID
    rows[123, 7] = 449
    ix = make_index(hs, tmp_path_factory, 300, 16, 0, np.arange(300, dtype=np.uint64), rows=rows)
    with pytest.raises(hs.HsError, match="row 123 .*component 7") as e:
        ix.set_row_format(hs.HS_ROWS_F8)
    assert e.value.status == hs.HS_ERR_UNSUPPORTED and ix.row_format() == hs.HS_ROWS_F32
