"""HS_ROWS_I8 on the device.  The reference of every case is the fp32 format on the same loaded index (equal labels, distance bits,
counts, stats) and the oracle for the default search.  Rows are integers from [-128, 127], each of the first 64 holding -128, -1, 0
and 127.  The dims reach every load shape of NarrowRound at 8 and 4 lanes per row: 2-byte loads (16), one 8-byte load (64), one 16-byte
load and the compiled d = 128 shape (128), 16 + 8 bytes + a single pair (208)."""
import functools

import numpy as np
import pytest

from hsutil import Oracle, load_product, mixture
from test_gpu_parity import _pq_sorted

pytestmark = pytest.mark.gpu
N, EXTRA, NQ, K, DIMS = 3000, 40, 64, 10, (16, 64, 128, 208)
MODES = ("flat", "flat", "fast", "strict", "fast", "strict")   # flat at ef 10 and 64, filter set, exact order, delete marks, marks at ef == k


@pytest.fixture(scope="module")
def hs():
    return load_product()


def int8_rows(n, d, seed):
    rng = np.random.default_rng(seed)
    x = rng.integers(-128, 128, (n, d)).astype(np.float32)
    for i in range(min(n, 64)):
        x[i, rng.permutation(d)[:4]] = (-128, -1, 0, 127)
    return x


@pytest.fixture(scope="module")
def graphs(hs, tmp_path_factory):
    @functools.lru_cache(maxsize=None)
    def make(d, metric):   # rows, queries and the serial builder's files of the first N rows and of all of them
        g = dict(base=int8_rows(N + EXTRA, d, 100 + d), q=int8_rows(NQ, d, 200 + d), tmp=tmp_path_factory.mktemp("i8"))
        for name, n in (("part", N), ("whole", N + EXTRA)):
            g[name] = str(g["tmp"] / name)
            hs.build_hnsw(g["base"][:n], g[name], metric=metric, M=8, ef_construction=60, branching_factor="4", seed=100, threads=1)
        return g
    return make


def load(hs, g, d, metric, path="part"):
    return hs.Index(g[path], hs.HS_KIND_HNSW, d, metric=metric, max_elements=N + EXTRA)


def answers(hs, ix, q, modes=MODES):
    """[(kernel, labels, distance bits, counts, stats)] of the first len(modes) MODES on ix; nothing is written beyond cnt entries."""
    marked, out = np.arange(0, N, 7), []
    if len(modes) > 2:
        fs = hs.FilterSet.create(ix, 2)
        fs.write(0, np.stack([np.arange(N) % 3 != 0, np.arange(N) % 2 == 0]).astype(np.uint8))
    for i, ef in enumerate((10, 64, 64, 64, 64, K)[:len(modes)]):
        ix.set_ef(ef)
        ix.set_exact_order(i == 3)
        if i == 4:
            ix.mark_deleted(marked)
        r = ix.search_filter_set(q, K, fs, np.arange(NQ, dtype=np.uint32) % 2, want_stats=True) if i == 2 else ix.search_pq(q, K, want_stats=True)
        keep = np.arange(K)[None, :] < r["cnt"][:, None]
        out.append((ix.last_kernel(), np.where(keep, r["labels"], 0), np.where(keep, r["dists"].view(np.uint32), 0), r["cnt"], r["stats"]))
    if len(modes) > 4:
        ix.mark_deleted(marked, on=False)
    return out


def same(got, want, narrow, what):
    for i, (g, w) in enumerate(zip(got, want)):
        assert g[0] == f"hs::{MODES[i]}_kernel" + ("_i8" if i in narrow else "") and w[0].replace("_i8", "") == f"hs::{MODES[i]}_kernel", f"{what}, mode {i}: ran {g[0]}"
        assert all(np.array_equal(a, b) for a, b in zip(g[1:], w[1:])), f"{what}, mode {i} ({g[0]}) differs from the fp32 format"


@pytest.mark.parametrize("metric", (0, 1))
@pytest.mark.parametrize("d", DIMS)
def test_search_kernels_and_exact_search_read_i8_rows(hs, graphs, d, metric):
    g = graphs(d, metric)
    base, q, cap = g["base"][:N], g["q"], N + EXTRA
    ix, ox = load(hs, g, d, metric), Oracle().load(g["part"], "hnsw", metric, d)
    want, bytes_f32 = answers(hs, ix, q), ix.info()["device_bytes"]
    for w, ef in zip(want, (10, 64)):   # the default search against the oracle
        ox.set_ef(ef)
        o = ox.search_pq(q, K)
        assert np.array_equal(w[4][:, :3], o["counters"][:, :3]) and _pq_sorted(w[2].view(np.float32), w[1], w[3]) == _pq_sorted(o["dists"], o["labels"], o["cnt"])
    fs = hs.FilterSet.create(ix, 1)
    fs.write(0, (np.arange(N) % 10 == 3).astype(np.uint8))   # a 10 % filter
    xargs = ((), (fs, np.zeros(NQ, np.uint32)))
    xwant = [ix.exact_search(q, K, *a) for a in xargs]
    ix.set_row_format(hs.HS_ROWS_I8)
    same(answers(hs, ix, q), want, (0, 1), "i8 beside fp32")
    ix.set_f32_resident(False)
    nx = hs.Index.load_narrow(g["part"], hs.HS_KIND_HNSW, d, hs.HS_ROWS_I8, metric=metric, max_elements=cap)
    assert nx.info() == ix.info() and nx.info()["device_bytes"] == bytes_f32 - 3 * cap * d and nx.row_format() == hs.HS_ROWS_I8 and not nx.f32_resident()
    for x, what in ((ix, "fp32 rows dropped"), (nx, "load_narrow")):
        same(answers(hs, x, q), want, range(6), what)
        assert all(x.get_row(lab).tobytes() == base[lab].tobytes() for lab in (0, 63, N - 1))
    for a, w in zip(xargs, xwant):
        for call, kernel in ((ix.exact_search, "hs::exact_scan_kernel_i8"), (ix.exact_search_screened, "hs::xs_screen_kernel_i8")):
            r = call(q, K, *a)
            assert ix.last_kernel() == kernel and all(r[key].tobytes() == w[key].tobytes() for key in ("cnt", "labels", "dists")), (kernel, len(a))
    if metric == 0:   # a shift by 128 keeps every L2 distance, so the serial builder makes the same graph: the same index in u8 form
        hs.build_hnsw(base + np.float32(128), g["whole"] + ".u8", M=8, ef_construction=60, branching_factor="4", seed=100, threads=1)
        assert hs.Index.load_narrow(g["whole"] + ".u8", hs.HS_KIND_HNSW, d, hs.HS_ROWS_U8, max_elements=cap).info()["device_bytes"] == nx.info()["device_bytes"]


@pytest.mark.parametrize("free", (False, True))
@pytest.mark.parametrize("d", DIMS)
def test_live_updates_write_the_i8_copy(hs, graphs, d, free):
    g = graphs(d, 0)
    base, q, new = g["base"], g["q"], int8_rows(3, d, 300 + d)
    ix, fx = load(hs, g, d, 0), load(hs, g, d, 0)
    ix.set_row_format(hs.HS_ROWS_I8)
    ix.set_f32_resident(not free)
    prior, bad = answers(hs, ix, q, MODES[:2]), base[N:N + 3].copy()
    bad[1, 5] = 128
    with pytest.raises(hs.HsError, match="row 1 .*component 5.*HS_ROWS_I8"):
        ix.add_points(bad, np.arange(N, N + 3))
    same(answers(hs, ix, q, MODES[:2]), prior, (0, 1), "after the refused add")
    for x in (ix, fx):
        x.seed_levels(100, N)
        x.add_points(base[N:], np.arange(N, N + EXTRA))
    same(answers(hs, ix, q, MODES[:2]), answers(hs, load(hs, g, d, 0, "whole"), q, MODES[:2]), (0, 1), "added, against the index loaded whole")
    for x in (ix, fx):
        x.upsert_points(new, [5, N + 1, 1000])
    same(answers(hs, ix, q, MODES[:2]), answers(hs, fx, q, MODES[:2]), (0, 1), "upserted")
    assert all(ix.get_row(lab).tobytes() == row.tobytes() for lab, row in zip((5, N + 1, 1000, N + 2), (*new, base[N + 2])))


def test_refusals(hs, tmp_path):
    from test_gpu_slimq import build

    def index_of(rows):
        hs.build_hnsw(rows, str(tmp_path / "r.bin"), M=8, ef_construction=40, threads=1)
        return hs.Index(str(tmp_path / "r.bin"), hs.HS_KIND_HNSW, rows.shape[1])
    rows = int8_rows(300, 16, 9)
    rows[123, 7] = 0.5
    ix = index_of(rows)
    for x, msg in ((ix, "row 123 .*component 7"), (index_of(int8_rows(300, 20, 11)), "dim % 16"),
                   (hs.Index(build(hs, tmp_path, "q", mixture(3000, 128, 1, integer=True), 0, 8), hs.HS_KIND_SLIMQ, 128), "SlimQ")):
        with pytest.raises(hs.HsError, match=msg) as e:
            x.set_row_format(hs.HS_ROWS_I8)
        assert e.value.status == hs.HS_ERR_UNSUPPORTED and x.row_format() == hs.HS_ROWS_F32
