"""Narrow rows on the device (hs_index_set_row_format): an index whose flat kernel reads a u8 or fp16 copy of the rows
(hs::flat_kernel_u8 / hs::flat_kernel_f16, csrc/flat_search.hip + csrc/narrow_rows.hip) answers exactly like the same index in
fp32 format -- labels in output order, distance bits, all four stats columns (so the same queries take the tie re-run) -- and like
the oracle: label sets, the three traversal counters, sorted fp32 distances bit for bit.  Every comparison is equality on every
query.  Refusals (a value the format cannot represent, SlimQ, dim % 16 != 0, an unrepresentable patch) are status codes and leave
the index as it was."""
import os
import subprocess

import numpy as np
import pytest

from hsutil import ROOT, Oracle, headline_data, load_chal_encode, load_product, mixture
from test_gpu_parity import _pq_sorted

pytestmark = pytest.mark.gpu
L2, IP = 0, 1
K = 10


@pytest.fixture(scope="module")
def hs():
    m = load_product()
    assert m.device_count() > 0, "no HIP device visible"
    return m


def kernel_name(hs, fmt):
    return {hs.HS_ROWS_F32: "hs::flat_kernel", hs.HS_ROWS_U8: "hs::flat_kernel_u8", hs.HS_ROWS_F16: "hs::flat_kernel_f16"}[fmt]


def same_bytes(a, b, what):
    """Two result dicts of the same call, byte for byte (labels in output order, distances, counts, all four stats columns)."""
    for key in a:
        if a[key] is None:
            assert b[key] is None
            continue
        assert a[key].dtype == b[key].dtype and a[key].tobytes() == b[key].tobytes(), f"{what}: {key} differs from the fp32-format run"


def narrow_vs_f32(hs, ix, fmt, run, what, flat=True):
    """run() on ix in fp32 format, then in `fmt`: identical outputs; with flat=True each run was served by its format's flat kernel.
    Returns the narrow run's result."""
    ix.set_row_format(hs.HS_ROWS_F32)
    assert ix.row_format() == hs.HS_ROWS_F32
    a = run()
    if flat:
        assert ix.last_kernel() == "hs::flat_kernel", what
    ix.set_row_format(fmt)
    assert ix.row_format() == fmt
    b = run()
    if flat:
        assert ix.last_kernel() == kernel_name(hs, fmt), what
    else:
        assert not ix.last_kernel().startswith("hs::flat_kernel"), what
    same_bytes(a, b, what)
    return b


# ---- 1. the bench's search shape -------------------------------------------------------------------------------------------
N, D = 50_000, 128
EFS = (64, 70, 129, 200, 300, 512)   # S = 1, 2, 3, 4, 6, 8


@pytest.fixture(scope="module")
def bench_index(hs, oracle, tmp_path_factory):
    d = tmp_path_factory.mktemp("narrow_bench_shape")
    base = headline_data(N, D, 123)
    hp, sp = str(d / "hnsw.bin"), str(d / "slim.bin")
    hs.build_hnsw(base, hp, M=16, ef_construction=200, branching_factor="4", seed=100, threads=16)
    hs.convert_slim(hp, sp, D, threads=16)
    return hs.Index(sp, hs.HS_KIND_SLIM, D, hs.HS_METRIC_L2), oracle.load(sp, "slim", 0, D), base


_want_cache = {}


def oracle_answer(ox, q, ef, key):
    """Sorted labels, counters and sorted distances of the oracle (as tests/test_gpu_bench_shape.py::oracle_answer)."""
    if (key, ef) not in _want_cache:
        ox.set_ef(ef)
        ids = ox.search_ids(q, K, threads=16)
        ox.set_mark_ep(0)
        try:
            pq = ox.search_pq(q, K, threads=16)
        finally:
            ox.set_mark_ep(-1)
        assert np.all(pq["cnt"] == K)
        _want_cache[(key, ef)] = dict(labels=np.sort(ids["labels"], axis=1), counters=ids["counters"][:, :3], dists=np.sort(pq["dists"], axis=1))
    return _want_cache[(key, ef)]


def same_as_oracle(want, labels, dists, stats, what):
    assert np.array_equal(np.sort(labels.astype(np.uint32), axis=1), want["labels"]), f"{what}: label sets differ"
    assert np.array_equal(stats[:, :3].astype(np.uint32), want["counters"]), f"{what}: counters differ"
    assert np.sort(dists, axis=1).view(np.uint32).tobytes() == want["dists"].view(np.uint32).tobytes(), f"{what}: distances differ"


@pytest.mark.parametrize("nq", (6143, 10_000))
def test_bench_shape_host_entry(hs, bench_index, nq):
    ix, ox, _ = bench_index
    q = headline_data(nq, D, 456)
    for ef in EFS:
        ix.set_ef(ef)
        want = oracle_answer(ox, q, ef, ("host", nq))
        for fmt in (hs.HS_ROWS_U8, hs.HS_ROWS_F16):
            what = f"nq={nq} ef={ef} fmt={fmt}"
            r = narrow_vs_f32(hs, ix, fmt, lambda: ix.search_ids(q, K, want_dists=True, want_stats=True), what)
            same_as_oracle(want, r["labels"], r["dists"], r["stats"], what)
    ix.set_row_format(hs.HS_ROWS_F32)


def test_bench_shape_device_entry_two_streams(hs, bench_index):
    """search_ids_dev on torch device tensors, two 10 000-query batches in flight on two non-default streams, u8 rows."""
    import torch
    ix, ox, _ = bench_index
    dev = torch.device("cuda", 0)
    qs = [headline_data(10_000, D, 456 + b) for b in range(2)]
    q_dev = [torch.from_numpy(q).to(dev) for q in qs]
    streams = [torch.cuda.Stream(device=dev) for _ in range(2)]
    torch.cuda.synchronize()
    ix.set_ef(70)
    res = {}
    for fmt in (hs.HS_ROWS_F32, hs.HS_ROWS_U8, hs.HS_ROWS_F16):
        ix.set_row_format(fmt)
        outs = []
        for b in range(2):
            lab = torch.full((10_000, K), -1, dtype=torch.int32, device=dev)
            dst = torch.full((10_000, K), float("nan"), dtype=torch.float32, device=dev)
            cnt = torch.zeros((10_000,), dtype=torch.int32, device=dev)
            sts = torch.zeros((10_000, 4), dtype=torch.int32, device=dev)
            streams[b].wait_stream(torch.cuda.current_stream())
            ix.search_ids_dev(q_dev[b], K, lab, dst, cnt, sts, streams[b].cuda_stream)
            outs.append((lab, dst, cnt, sts))
        for b in range(2):
            ix.check(streams[b].cuda_stream)
        assert ix.last_kernel() == kernel_name(hs, fmt) and ix.row_format() == fmt
        res[fmt] = [tuple(t.cpu().numpy() for t in outs[b]) for b in range(2)]
    for fmt in (hs.HS_ROWS_U8, hs.HS_ROWS_F16):
        for b in range(2):
            for x, y in zip(res[hs.HS_ROWS_F32][b], res[fmt][b]):
                assert x.tobytes() == y.tobytes(), f"device entry, batch {b}, fmt={fmt}: differs from the fp32-format run"
            lab, dst, cnt, sts = res[fmt][b]
            assert np.all(cnt == K)
            same_as_oracle(oracle_answer(ox, qs[b], 70, ("dev", b)), lab, dst, sts, f"device entry, batch {b}, fmt={fmt}")
    ix.set_row_format(hs.HS_ROWS_F32)


# ---- 2. tie-heavy small-integer rows, every compiled shape --------------------------------------------------------------
def _int_rows(n, d, seed):
    """tests/test_gpu_flat_wide.py::_rows(..., integer=True): values 0 .. ~12, ties at the bound on most queries."""
    return np.ascontiguousarray(mixture(n, d, seed, n_clusters=12, lo=0, hi=6, sigma=1.5, integer=True))


@pytest.mark.parametrize("metric", (L2, IP))
@pytest.mark.parametrize("d", (16, 48, 64, 96, 128, 320, 512, 960))
def test_tie_heavy_integer_rows_every_shape(hs, oracle, tmp_path, d, metric):
    n = 6000 if d <= 128 else 2500
    base, q = _int_rows(n, d, 31 + d), _int_rows(64, d, 77 + d)
    hp, sp = str(tmp_path / "h.bin"), str(tmp_path / "s.bin")
    hs.build_hnsw(base, hp, metric=metric, M=12, ef_construction=80, threads=8)
    hs.convert_slim(hp, sp, d, metric=metric, threads=8)
    for kind, path, okind in ((hs.HS_KIND_SLIM, sp, "slim"), (hs.HS_KIND_HNSW, hp, "hnsw")):
        ix = hs.Index(path, kind, d, metric=metric)
        ox = oracle.load(path, okind, metric, d)
        pairs = ((129, 10), (160, 33), (192, 64), (257, 10), (320, 40), (384, 10), (385, 64), (500, 10), (512, 64)) if kind == hs.HS_KIND_SLIM \
            else ((192, 10), (300, 10), (512, 20))
        for ef, k in pairs:
            ix.set_ef(ef); ox.set_ef(ef)
            o = ox.search_pq(q, k, threads=8)
            oi = ox.search_ids(q, k, threads=8) if kind == hs.HS_KIND_SLIM else None
            for fmt in (hs.HS_ROWS_U8, hs.HS_ROWS_F16):
                cfg = f"d={d} metric={metric} kind={okind} ef={ef} k={k} fmt={fmt}"
                g = narrow_vs_f32(hs, ix, fmt, lambda: ix.search_pq(q, k, want_stats=True), cfg)
                assert np.array_equal(g["cnt"], o["cnt"]), cfg
                assert _pq_sorted(g["dists"], g["labels"], g["cnt"]) == _pq_sorted(o["dists"], o["labels"], o["cnt"]), cfg
                if kind == hs.HS_KIND_SLIM:
                    r = narrow_vs_f32(hs, ix, fmt, lambda: ix.search_ids(q, k, want_dists=True, want_stats=True), cfg + " ids")
                    assert np.array_equal(np.sort(r["labels"], 1), np.sort(oi["labels"], 1)), cfg
                    assert np.array_equal(r["stats"][:, :3], oi["counters"][:, :3]), cfg


def test_long_logs_at_ef_512_u8(hs, oracle, tmp_path):
    """tests/test_gpu_flat_wide.py::test_flat_kernel_long_logs_at_ef_512 with u8 rows (d = 48: the runtime-dim narrow loads)."""
    d = 48
    base = np.ascontiguousarray(mixture(20000, d, 5, n_clusters=6, lo=0, hi=4, sigma=1.2, integer=True))
    q = np.ascontiguousarray(mixture(128, d, 6, n_clusters=6, lo=0, hi=4, sigma=1.2, integer=True))
    hp, sp = str(tmp_path / "h.bin"), str(tmp_path / "s.bin")
    hs.build_hnsw(base, hp, M=16, ef_construction=100, threads=8)
    hs.convert_slim(hp, sp, d, threads=8)
    ix, ox = hs.Index(sp, hs.HS_KIND_SLIM, d), oracle.load(sp, "slim", L2, d)
    for ef in (400, 512):
        ix.set_ef(ef); ox.set_ef(ef)
        o = ox.search_ids(q, 10, threads=8)
        r = narrow_vs_f32(hs, ix, hs.HS_ROWS_U8, lambda: ix.search_ids(q, 10, want_dists=True, want_stats=True), f"ef={ef}")
        assert np.array_equal(np.sort(r["labels"], 1), np.sort(o["labels"], 1)), ef
        assert np.array_equal(r["stats"][:, :3], o["counters"][:, :3]), ef


# ---- 3. fp16 on real values ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", (L2, IP))
def test_fp16_rows_on_rounded_unit_vectors(hs, oracle, tmp_path, metric):
    """DEEP-like: unit-norm d = 96 rows rounded through float16 BEFORE the build, so build, convert and search are all the
    reference on that data set.  A few dozen rows carry fp16 subnormals, -0.0 and +-65504 (the conversion's denormal and range
    handling).  u8 on this index is refused."""
    d, n = 96, 6000
    rng = np.random.default_rng(96 + metric)
    x = mixture(n, d, 41, n_clusters=12, lo=-1, hi=1, sigma=0.4)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    base = x.astype(np.float16).astype(np.float32)
    special = np.array([2.0 ** -24, 2.0 ** -20, 2.0 ** -15, 3 * 2.0 ** -24, -2.0 ** -24, -0.0, 65504.0, -65504.0], np.float32)
    rows = rng.choice(n, 40, replace=False)
    for i, r in enumerate(rows):
        cols = rng.choice(d, 3, replace=False)
        base[r, cols] = special[(i + np.arange(3)) % (len(special) if i % 4 == 0 else len(special) - 2)]   # (every fourth row may take +-65504)
    base = np.ascontiguousarray(base)
    assert hs.rows_representable(base, hs.HS_ROWS_F16) is None
    q = mixture(200, d, 43, n_clusters=12, lo=-1, hi=1, sigma=0.4)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    q = np.ascontiguousarray(np.concatenate([q, base[rows[:20]]]).astype(np.float32))   # (some queries ARE the special rows)
    hp, sp = str(tmp_path / "h.bin"), str(tmp_path / "s.bin")
    hs.build_hnsw(base, hp, metric=metric, M=12, ef_construction=80, threads=8)
    hs.convert_slim(hp, sp, d, metric=metric, threads=8)
    ix, ox = hs.Index(sp, hs.HS_KIND_SLIM, d, metric=metric), oracle.load(sp, "slim", metric, d)
    for ef, k in ((48, 10), (100, 10), (192, 64), (400, 10)):
        ix.set_ef(ef); ox.set_ef(ef)
        cfg = f"metric={metric} ef={ef} k={k}"
        o = ox.search_pq(q, k, threads=8)
        g = narrow_vs_f32(hs, ix, hs.HS_ROWS_F16, lambda: ix.search_pq(q, k, want_stats=True), cfg)
        assert np.array_equal(g["cnt"], o["cnt"]), cfg
        assert _pq_sorted(g["dists"], g["labels"], g["cnt"]) == _pq_sorted(o["dists"], o["labels"], o["cnt"]), cfg
        oi = ox.search_ids(q, k, threads=8)
        r = narrow_vs_f32(hs, ix, hs.HS_ROWS_F16, lambda: ix.search_ids(q, k, want_dists=True, want_stats=True), cfg)
        assert np.array_equal(np.sort(r["labels"], 1), np.sort(oi["labels"], 1)), cfg
        assert np.array_equal(r["stats"][:, :3], oi["counters"][:, :3]), cfg
    before = ix.search_ids(q, 10, want_dists=True, want_stats=True)
    with pytest.raises(hs.HsError) as e:
        ix.set_row_format(hs.HS_ROWS_U8)
    assert e.value.status == hs.HS_ERR_UNSUPPORTED
    assert ix.row_format() == hs.HS_ROWS_F16
    same_bytes(before, ix.search_ids(q, 10, want_dists=True, want_stats=True), "after the refused u8 request")
    assert ix.last_kernel() == "hs::flat_kernel_f16"


# ---- 4. refusals leave the index as it was ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_int_index(hs, tmp_path_factory):
    """(slim file, parsed graph, base rows, queries) of a 3000 x 64 integer index."""
    t = tmp_path_factory.mktemp("narrow_small")
    base, q = mixture(3000, 64, 1, integer=True), mixture(100, 64, 2, integer=True)
    hp, sp = str(t / "h.bin"), str(t / "s.bin")
    hs.build_hnsw(base, hp, M=16, ef_construction=100, threads=8)
    hs.convert_slim(hp, sp, 64, threads=8)
    return sp, load_chal_encode().parse_slim(open(sp, "rb").read(), 64), base, q


@pytest.mark.parametrize("fmt_name,value", [("HS_ROWS_U8", 255.5), ("HS_ROWS_U8", 256.0), ("HS_ROWS_U8", -1.0), ("HS_ROWS_F16", 0.1), ("HS_ROWS_F16", 65520.0)])
def test_unrepresentable_value_is_refused(hs, small_int_index, fmt_name, value):
    _, s, _, q = small_int_index
    fmt = getattr(hs, fmt_name)
    rows = np.array(s["rows"], np.float32, copy=True)
    bad_row = 1234
    rows[bad_row, 17] = np.float32(value)
    rows[2500, 3] = np.float32(value)   # (a later offender: the first one is reported)
    ix = hs.Index.from_arrays(hs.HS_KIND_SLIM, hs.HS_METRIC_L2, rows, s["level"], s["lists"], s["enterpoint"], s["maxlevel"], labels=s["labels"])
    ix.set_ef(64)
    bytes_before = ix.info()["device_bytes"]
    before = ix.search_ids(q, K, want_dists=True, want_stats=True)
    with pytest.raises(hs.HsError) as e:
        ix.set_row_format(fmt)
    assert e.value.status == hs.HS_ERR_UNSUPPORTED
    assert str(bad_row) in str(e.value), str(e.value)
    assert ix.row_format() == hs.HS_ROWS_F32
    assert ix.info()["device_bytes"] == bytes_before
    same_bytes(before, ix.search_ids(q, K, want_dists=True, want_stats=True), "after the refusal")
    assert ix.last_kernel() == "hs::flat_kernel"
    # the other format still takes it when the value fits there (255.5 and 256 are fp16 values)
    if fmt == hs.HS_ROWS_U8 and value in (255.5, 256.0):
        ix.set_row_format(hs.HS_ROWS_F16)
        same_bytes(before, ix.search_ids(q, K, want_dists=True, want_stats=True), "fp16 rows")
        assert ix.last_kernel() == "hs::flat_kernel_f16"


def test_slimq_and_odd_dims_are_refused(hs, tmp_path):
    from test_gpu_slimq import build
    base = mixture(3000, 128, 1, integer=True)
    qx = hs.Index(build(hs, tmp_path, "q", base, L2, 8), hs.HS_KIND_SLIMQ, 128)
    for fmt in (hs.HS_ROWS_U8, hs.HS_ROWS_F16):
        with pytest.raises(hs.HsError) as e:
            qx.set_row_format(fmt)
        assert e.value.status == hs.HS_ERR_UNSUPPORTED and qx.row_format() == hs.HS_ROWS_F32
    b20, q20 = mixture(2000, 20, 3, integer=True), mixture(50, 20, 4, integer=True)
    hp, sp = str(tmp_path / "h20.bin"), str(tmp_path / "s20.bin")
    hs.build_hnsw(b20, hp, M=16, ef_construction=100, threads=8)
    hs.convert_slim(hp, sp, 20, threads=8)
    ix = hs.Index(sp, hs.HS_KIND_SLIM, 20)
    ix.set_ef(40)
    before, bytes_before = ix.search_ids(q20, K, want_dists=True, want_stats=True), ix.info()["device_bytes"]
    for fmt in (hs.HS_ROWS_U8, hs.HS_ROWS_F16):
        with pytest.raises(hs.HsError) as e:
            ix.set_row_format(fmt)
        assert e.value.status == hs.HS_ERR_UNSUPPORTED and ix.row_format() == hs.HS_ROWS_F32
    assert ix.info()["device_bytes"] == bytes_before
    same_bytes(before, ix.search_ids(q20, K, want_dists=True, want_stats=True), "d = 20 after the refusals")
    with pytest.raises(hs.HsError) as e:
        ix.set_row_format(9)
    assert e.value.status == hs.HS_ERR_INVALID


# ---- 5. switching formats on one index -----------------------------------------------------------------------------------
def test_switching_formats_keeps_results_and_accounts_for_the_copy(hs, small_int_index):
    sp, _, _, q = small_int_index
    n, d = 3000, 64
    ix = hs.Index(sp, hs.HS_KIND_SLIM, d)
    ix.set_ef(100)
    start = ix.info()["device_bytes"]
    first = ix.search_ids(q, K, want_dists=True, want_stats=True)
    # documented size of the copy (include/hnsw_slim_amd.h): max(n, max_elements) x dim x 1 or 2 bytes; max_elements = 0 here
    for fmt, extra in ((hs.HS_ROWS_U8, n * d), (hs.HS_ROWS_F16, 2 * n * d), (hs.HS_ROWS_U8, n * d), (hs.HS_ROWS_F32, 0), (hs.HS_ROWS_F16, 2 * n * d),
                       (hs.HS_ROWS_F32, 0)):
        ix.set_row_format(fmt)
        assert ix.row_format() == fmt and ix.info()["device_bytes"] == start + extra
        same_bytes(first, ix.search_ids(q, K, want_dists=True, want_stats=True), f"fmt={fmt}")
        assert ix.last_kernel() == kernel_name(hs, fmt)
    roomy = hs.Index(sp, hs.HS_KIND_SLIM, d, max_elements=n + 500)
    s0 = roomy.info()["device_bytes"]
    roomy.set_row_format(hs.HS_ROWS_U8)
    assert roomy.info()["device_bytes"] == s0 + (n + 500) * d


# ---- 6. the paths that keep reading the fp32 rows ------------------------------------------------------------------------
@pytest.mark.parametrize("fmt_name", ("HS_ROWS_U8", "HS_ROWS_F16"))
def test_fp32_paths_on_a_narrow_index(hs, oracle, small_int_index, fmt_name):
    sp, _, _, q = small_int_index
    fmt = getattr(hs, fmt_name)
    ix = hs.Index(sp, hs.HS_KIND_SLIM, 64)
    ox = oracle.load(sp, "slim", L2, 64)
    ix.set_ef(64); ox.set_ef(64)
    allowed = (np.arange(3000) % 3 != 0).astype(np.uint8)
    r = narrow_vs_f32(hs, ix, fmt, lambda: ix.search_filtered(q, K, allowed, want_stats=True), "filtered", flat=False)
    ox.set_filter(allowed)
    o = ox.search_pq(q, K)
    ox.set_filter(None)
    assert _pq_sorted(r["dists"], r["labels"], r["cnt"]) == _pq_sorted(o["dists"], o["labels"], o["cnt"])
    ix.set_exact_order(True)
    r = narrow_vs_f32(hs, ix, fmt, lambda: ix.search_ids(q, K, want_dists=True, want_stats=True), "exact order", flat=False)
    ix.set_exact_order(False)
    assert np.array_equal(r["labels"], ox.search_ids(q, K)["labels"])

    def raw_valid():   # (the arrays beyond raw_sz[i] entries are not written)
        r = ix.search_raw(q, K)
        keep = np.arange(r["raw_d"].shape[1])[None, :] < r["raw_sz"][:, None]
        return dict(raw_d=np.where(keep, r["raw_d"], np.float32(0)), raw_i=np.where(keep, r["raw_i"], np.uint32(0)), raw_sz=r["raw_sz"], stats=r["stats"])
    r = narrow_vs_f32(hs, ix, fmt, raw_valid, "search_raw", flat=False)
    assert np.array_equal(r["raw_sz"], ox.search_ids(q, K)["raw_sz"])
    ix.set_ef(600); ox.set_ef(600)
    r = narrow_vs_f32(hs, ix, fmt, lambda: ix.search_ids(q, K, want_dists=True, want_stats=True), "ef = 600", flat=False)
    o = ox.search_ids(q, K)
    assert np.array_equal(np.sort(r["labels"], 1), np.sort(o["labels"], 1)) and np.array_equal(r["stats"][:, :3], o["counters"][:, :3])


# ---- 7. patch -----------------------------------------------------------------------------------------------------------------
def test_patch_on_a_u8_index(hs, oracle, tmp_path):
    """The d = 128 integer case of tests/test_gpu_patch.py with the patched index in u8 format; a patch whose new rows hold 300.0
    is refused and the index answers as before."""
    ce = load_chal_encode()
    dim, n0, delta = 128, 8000, 1500
    base = mixture(n0 + delta, dim, 17, integer=True)
    bad = base.copy()
    bad[n0 + 700, 5] = np.float32(300.0)
    files = {}
    for tag, rows in (("old", base[:n0]), ("new", base), ("bad", bad)):
        hp, sp = str(tmp_path / f"{tag}.hnsw"), str(tmp_path / f"{tag}.slim")
        hs.build_hnsw(rows, hp, M=16, ef_construction=100, threads=1)   # serial: the first n0 insertions are the same in all three
        hs.convert_slim(hp, sp, dim, threads=1)
        files[tag] = open(sp, "rb").read()
    patch, n_changed, n_added = ce.make_patch(files["old"], files["new"], dim, to_add=True)
    bad_patch, _, bad_added = ce.make_patch(files["old"], files["bad"], dim, to_add=True)
    assert n_added == delta and bad_added == delta and n_changed > 0
    want_file = str(tmp_path / "expect.slim")
    open(want_file, "wb").write(ce.with_entry_of(files["new"], files["old"]))
    q = mixture(300, dim, 18, integer=True)
    ix = hs.Index(str(tmp_path / "old.slim"), hs.HS_KIND_SLIM, dim, max_elements=n0 + delta + 16)
    ix.set_row_format(hs.HS_ROWS_U8)
    ix.set_ef(48)
    before = ix.search_ids(q, 10, want_dists=True, want_stats=True)
    assert ix.last_kernel() == "hs::flat_kernel_u8"
    bytes_before = ix.info()["device_bytes"]
    with pytest.raises(hs.HsError) as e:
        ix.patch(bad_patch, to_add=True)
    assert e.value.status == hs.HS_ERR_UNSUPPORTED and str(n0 + 700) in str(e.value), str(e.value)
    assert ix.info()["n"] == n0 and ix.row_format() == hs.HS_ROWS_U8 and ix.info()["device_bytes"] == bytes_before
    same_bytes(before, ix.search_ids(q, 10, want_dists=True, want_stats=True), "after the refused patch")
    ix.patch(patch, to_add=True)
    assert ix.info()["n"] == n0 + delta and ix.row_format() == hs.HS_ROWS_U8
    ref = hs.Index(want_file, hs.HS_KIND_SLIM, dim)
    ox = oracle.load(want_file, "slim", 0, dim)
    for ef in (10, 48, 100):
        for x in (ix, ref, ox):
            x.set_ef(ef)
        a, b = ix.search_ids(q, 10, want_dists=True, want_stats=True), ref.search_ids(q, 10, want_dists=True, want_stats=True)
        assert ix.last_kernel() == "hs::flat_kernel_u8" and ref.last_kernel() == "hs::flat_kernel"
        same_bytes(b, a, f"patched u8 index vs the index loaded whole, ef={ef}")
        o = ox.search_ids(q, 10)
        assert np.array_equal(np.sort(a["labels"], 1), np.sort(o["labels"], 1)) and np.array_equal(a["stats"][:, :3], o["counters"][:, :3])
    ix.set_ef(48)
    assert not np.array_equal(ix.search_ids(q, 10)["labels"], before["labels"]), "the patch changed nothing?"
    # the refused rows do fit fp16: the same index in fp16 format takes the patch
    jx = hs.Index(str(tmp_path / "old.slim"), hs.HS_KIND_SLIM, dim, max_elements=n0 + delta + 16)
    jx.set_row_format(hs.HS_ROWS_F16)
    jx.patch(bad_patch, to_add=True)
    bad_file = str(tmp_path / "expect_bad.slim")
    open(bad_file, "wb").write(ce.with_entry_of(files["bad"], files["old"]))
    rx = hs.Index(bad_file, hs.HS_KIND_SLIM, dim)
    jx.set_ef(48); rx.set_ef(48)
    same_bytes(rx.search_ids(q, 10, want_dists=True, want_stats=True), jx.search_ids(q, 10, want_dists=True, want_stats=True), "fp16 index, patched")
    assert jx.last_kernel() == "hs::flat_kernel_f16"


# ---- 8. sharded ---------------------------------------------------------------------------------------------------------------
def test_sharded_loopback_with_u8_replicas(hs, small_int_index):
    sp, _, _, q = small_int_index
    reps = [hs.Index(sp, hs.HS_KIND_SLIM, 64) for _ in range(2)]
    single = hs.Index(sp, hs.HS_KIND_SLIM, 64)
    comm = hs.Comm([0, 0])
    for x in reps + [single]:
        x.set_ef(48)
    for r in reps:
        r.set_row_format(hs.HS_ROWS_U8)
    want = single.search_ids(q, K, want_dists=True)
    got = comm.search_ids(reps, q, K, want_dists=True)
    assert all(r.last_kernel() == "hs::flat_kernel_u8" for r in reps) and single.last_kernel() == "hs::flat_kernel"
    assert np.array_equal(got["labels"], want["labels"]) and got["dists"].tobytes() == want["dists"].tobytes()
    assert np.array_equal(got["cnt"], want["cnt"])
    comm.close()


# ---- 9. facade ----------------------------------------------------------------------------------------------------------------
def test_cpp_facade_with_u8_rows(hs, oracle, tmp_path):
    exe = os.path.join(ROOT, "hnsw-slim_amd", "facade_narrow")
    assert os.path.exists(exe)
    n, d, nq, k, ef = 3000, 64, 100, 10, 80
    base, q = mixture(n, d, 1, integer=True), mixture(nq, d, 2, integer=True)
    bf, qf, out = (str(tmp_path / f) for f in ("b.f32", "q.f32", "o.bin"))
    base.tofile(bf); q.tofile(qf)
    subprocess.check_call([exe, bf, str(n), str(d), qf, str(nq), str(k), str(ef), out])
    raw = np.fromfile(out, np.uint32)
    assert raw[:6].tolist() == [hs.HS_ROWS_U8, 1, hs.HS_ROWS_U8, hs.HS_ROWS_U8, 1, 1], raw[:6]
    slim_labels, hnsw_labels = raw[6:6 + nq * k].reshape(nq, k), raw[6 + nq * k:].reshape(nq, k)
    hp, sp = str(tmp_path / "h.bin"), str(tmp_path / "s.bin")
    hs.build_hnsw(base, hp, M=16, ef_construction=100, branching_factor="4", seed=100, threads=1)   # what the facade built
    hs.convert_slim(hp, sp, d)
    ox, ov = oracle.load(sp, "slim", L2, d), oracle.load(hp, "hnsw", L2, d)
    ox.set_ef(ef); ov.set_ef(ef)
    assert np.array_equal(np.sort(slim_labels, 1), np.sort(ox.search_ids(q, k)["labels"], 1))
    w = ov.search_pq(q, k)
    assert np.all(w["cnt"] == k)
    assert np.array_equal(np.sort(hnsw_labels, 1), np.sort(w["labels"].astype(np.uint32), 1))
