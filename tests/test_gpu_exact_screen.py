"""The screened exact search (hs_index_exact_search_screened[_dev], csrc/exact_screen.hip): an MFMA screen with a proven margin, a
re-rank in the reference's arithmetic, the scan per query where the screen cannot decide.  Every answer is compared with == on
labels, fp32 bits and counts against Oracle.dist + a lexsort on (dist, label) over the admitted ids (test_gpu_bruteforce._expect) and
against Index.exact_search on the same index; neither is the code under test."""
import functools
import os
import subprocess

import numpy as np
import pytest

import value_range as vr
from hsutil import ROOT, Oracle, load_product
from test_gpu_bruteforce import _expect
from test_gpu_exact_search import data, filters, graph, make_index

pytestmark = pytest.mark.gpu
L2, IP = 0, 1
NONE64 = np.iinfo(np.uint64).max
# (n, d, nq, k, metric): more than one 64-query tile and not a multiple of it, more than one row chunk and k at its limit (2003); just
# above one bitmap word (40); n < k (9); a delegated dim (100)
SHAPES = [(777, 32, 37, 10, L2), (2003, 128, 70, 64, L2), (40, 16, 5, 10, L2), (9, 16, 3, 10, L2), (1501, 48, 21, 10, IP),
          (1203, 100, 13, 10, L2)]
# a tile that does not fit the LDS whole and is staged in slices of 128: 7.5 slices and two steps of units, the second partly filled
# (960); whole slices, k at its limit, IP (512)
SLICED = [(333, 960, 9, 10, L2), (300, 512, 5, 64, IP)]
KINDS = ("integer", "float", "neardup", "offset", "alldup")


@pytest.fixture(scope="module")
def hs():
    return load_product()


@pytest.fixture(scope="module")
def oracle():
    return Oracle()


@functools.lru_cache(maxsize=None)
def rows_of(kind, n, d, nq):
    """(base, queries, labels); labels are a permutation x 7 + 5."""
    base, q, labels = data(n, d, nq)
    if kind != "integer":
        rng = np.random.default_rng(n + d)
        base, q = rng.standard_normal((n, d)).astype(np.float32), rng.standard_normal((nq, d)).astype(np.float32)
    if kind == "neardup":   # every row three times, one copy one ulp off in coordinate 0
        base = np.repeat(base[:(n + 2) // 3], 3, axis=0)[:n].copy()
        base[2::3, 0] = np.nextafter(base[2::3, 0], np.float32(np.inf))
    if kind == "offset":
        base, q = base + np.float32(100), q + np.float32(100)
    if kind == "alldup":
        base = np.repeat(base[:1], n, axis=0)
    return np.ascontiguousarray(base), np.ascontiguousarray(q), labels


def expected(oracle, metric, base, q, k, labels, mask=None):
    ids = np.arange(len(base)) if mask is None else np.flatnonzero(mask)
    c = min(k, len(ids))
    L, D = np.full((len(q), k), NONE64, np.uint64), np.full((len(q), k), np.inf, np.float32)
    if c:
        L[:, :c], D[:, :c] = _expect(oracle, metric, np.ascontiguousarray(base[ids]), q, c, np.ascontiguousarray(labels[ids]))
    return dict(labels=L, dists=D, cnt=np.full(len(q), c, np.uint32))


def same(got, want, what, sel=slice(None)):
    for key in ("cnt", "labels", "dists"):
        assert got[key][sel].tobytes() == want[key].tobytes(), f"{what}: {key}"


CASES = [(s, kind) for s in SHAPES + SLICED for kind in KINDS if kind != "alldup" or s[0] == 2003]


@pytest.mark.parametrize("shape,kind", CASES, ids=lambda v: str(v))
def test_screened_answers_are_the_scan_s(hs, oracle, tmp_path_factory, shape, kind):
    n, d, nq, k, metric = shape
    base, q, labels = rows_of(kind, n, d, nq)
    ix = make_index(hs, tmp_path_factory, n, d, metric, labels, rows=base)
    r = ix.exact_search_screened(q, k)
    st = ix.exact_screen_stats()
    same(r, expected(oracle, metric, base, q, k, labels), "lexsort")
    same(r, ix.exact_search(q, k), "the scan")
    if d % 16:
        assert st == dict(screened=0, fell_back=0, reranked_rows=0)
        return
    assert st["screened"] + st["fell_back"] == nq
    if kind in ("float", "neardup"):
        assert st["fell_back"] == 0 and st["screened"] == nq and nq * min(k, n) <= st["reranked_rows"] <= nq * (min(k, n) + 16), st
    if kind == "alldup":
        assert st["fell_back"] == nq


@pytest.mark.parametrize("shape", SHAPES[:2], ids=lambda v: str(v))
def test_filters_per_query_and_delete_marks(hs, oracle, tmp_path_factory, shape):
    n, d, nq, k, metric = shape
    base, q, labels = rows_of("integer", n, d, nq)
    deleted = (np.arange(n) % 3 == 0).astype(np.uint8)
    ix = make_index(hs, tmp_path_factory, n, d, metric, labels, deleted=deleted)
    fs, filt = hs.FilterSet.create(ix, 5), filters(n)
    fs.write(0, filt)
    foq = (np.arange(nq) % 5).astype(np.uint32)
    r = ix.exact_search_screened(q, k, fs, foq)
    assert ix.last_kernel() == "hs::xs_screen_kernel"
    same(r, ix.exact_search(q, k, fs, foq), "the scan")
    for f in range(5):
        sel = foq == f
        same(r, expected(oracle, metric, base, np.ascontiguousarray(q[sel]), k, labels, (filt[f] != 0) & (deleted == 0)), f"filter {f}", sel)


@pytest.mark.parametrize("shape", (SHAPES[0], SLICED[0]), ids=("whole", "sliced"))
@pytest.mark.parametrize("fmt_name,kernel", (("HS_ROWS_U8", "hs::xs_screen_kernel_u8"), ("HS_ROWS_F16", "hs::xs_screen_kernel_f16")))
def test_narrow_rows_and_an_fp32_free_index(hs, oracle, tmp_path_factory, fmt_name, kernel, shape):
    n, d, nq, k, metric = shape
    base, q, _ = rows_of("integer", n, d, nq)
    want = expected(oracle, metric, base, q, k, np.arange(n, dtype=np.uint64))
    ix = hs.Index(graph(hs, tmp_path_factory, n, d, metric)[0], hs.HS_KIND_SLIM, d, metric=metric)
    ix.set_row_format(getattr(hs, fmt_name))
    for resident in (True, False):
        if not resident:
            ix.set_f32_resident(False)
        r = ix.exact_search_screened(q, k)
        assert ix.last_kernel() == kernel
        same(r, want, f"lexsort, fp32 resident {resident}")
        same(r, ix.exact_search(q, k), f"the scan, fp32 resident {resident}")


def test_l2_distances_that_overflow_fall_back(hs, oracle, tmp_path):
    base, q = vr.overflow_rows_and_queries()
    k, hp = vr.OVERFLOW_K, str(tmp_path / "h.bin")
    hs.build_hnsw(base, hp, metric=L2, M=8, ef_construction=40, threads=4)
    ix = hs.Index(hp, hs.HS_KIND_HNSW, vr.OVERFLOW_DIM, metric=L2)
    r = ix.exact_search_screened(q, k)
    same(r, expected(oracle, L2, base, q, k, np.arange(len(base), dtype=np.uint64)), "lexsort")
    same(r, ix.exact_search(q, k), "the scan")
    assert np.isposinf(r["dists"]).any()


def test_device_entry_on_a_stream(hs, tmp_path_factory):
    import torch
    n, d, nq, k, metric = SHAPES[0]
    base, q, labels = rows_of("float", n, d, nq)
    ix = make_index(hs, tmp_path_factory, n, d, metric, labels, rows=base)
    fs = hs.FilterSet.create(ix, 5)
    fs.write(0, filters(n))
    foq = (np.arange(nq) % 5).astype(np.uint32)
    dev = torch.device("cuda:0")
    st = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(st):
        dq = torch.from_numpy(q.copy()).to(dev)
        for use_fs in (False, True):
            o = (torch.zeros((nq, k), dtype=torch.int64, device=dev), torch.zeros((nq, k), dtype=torch.float32, device=dev),
                 torch.zeros(nq, dtype=torch.int32, device=dev))
            ix.exact_search_screened_dev(dq, k, *o, fs=fs if use_fs else None,
                                         d_filter_of_query=torch.from_numpy(foq.astype(np.int32)).to(dev) if use_fs else None, stream=st.cuda_stream)
            ix.check(st.cuda_stream)
            got = dict(labels=o[0].cpu().numpy().view(np.uint64), dists=o[1].cpu().numpy(), cnt=o[2].cpu().numpy().view(np.uint32))
            assert ix.exact_screen_stats()["screened"] == nq
            same(got, ix.exact_search(q, k, fs, foq) if use_fs else ix.exact_search(q, k), f"device entry, filter set {use_fs}")
    st.synchronize()


@pytest.mark.parametrize("kind", ["hnsw", "slim"])
def test_facade_set_exact_screened(hs, tmp_path, kind):
    """searchKnnExact (a functor for every other query) and searchKnnExactBatch after setExactScreened(true): the binding's answers."""
    exe = os.path.join(ROOT, "hnsw-slim_amd", "facade_exact_screened")
    assert os.path.exists(exe), "facade_exact_screened is built by `make -C hnsw-slim_amd all`"
    n, d, nq, k = 777, 32, 13, 10
    base, q, _ = data(n, d, nq)
    hp, qf, out = str(tmp_path / "h.bin"), str(tmp_path / "q.f32"), str(tmp_path / "out.bin")
    hs.build_hnsw(base, hp, M=8, ef_construction=40, threads=4)
    if kind == "slim":
        hs.convert_slim(hp, hp + ".slim", d, threads=4)
        hp += ".slim"
    q.tofile(qf)
    subprocess.check_call([exe, kind, hp, str(d), qf, str(nq), str(k), out])
    ix = hs.Index(hp, hs.HS_KIND_HNSW if kind == "hnsw" else hs.HS_KIND_SLIM, d)
    fs = hs.FilterSet.create(ix, 2)
    fs.write(0, np.stack([np.ones(n, bool), np.arange(n) % 2 == 0]).astype(np.uint8))
    want, batch = ix.exact_search(q, k, fs, (np.arange(nq) % 2).astype(np.uint32)), ix.exact_search(q, k)
    buf, off = open(out, "rb").read(), 0
    for i in range(nq):
        c = int(np.frombuffer(buf, np.uint32, 1, off)[0]); off += 4
        rec = np.frombuffer(buf, np.dtype([("d", "<f4"), ("l", "<u8")]), c, off); off += 12 * c
        assert c == k and np.array_equal(rec["l"], want["labels"][i]) and rec["d"].tobytes() == want["dists"][i].tobytes(), i
    assert buf[off:] == batch["labels"].tobytes() + batch["dists"].tobytes() + batch["cnt"].tobytes()
