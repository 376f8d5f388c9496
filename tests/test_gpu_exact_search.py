"""Exact search on a resident index (hs_index_exact_search[_dev], csrc/exact_search.hip): filtered brute force over the rows the
index holds, in the format it holds them.

Every answer is pinned twice, and neither reference is the code under test: Oracle.dist followed by a lexsort on (dist, label)
over the query's candidate ids (test_gpu_bruteforce._expect), and hs_brute_force -- the scan that existed before -- over
base[mask] with labels[mask].  Labels, fp32 bits and counts must match exactly.  Indexes come from the project's own builder
(build_hnsw + convert_slim, re-assembled by Index.from_arrays to give them custom labels and delete marks); rows are tiny-range
integers so that labels decide ties, and labels are a permutation times 7 plus 5 so that the tie-break is by label, not by id."""
import functools
import os
import subprocess

import numpy as np
import pytest

from hsutil import GOLDEN, ROOT, Oracle, load_chal_encode, load_product, mixture
from test_gpu_bruteforce import _expect

pytestmark = pytest.mark.gpu
L2, IP = 0, 1
NONE64 = np.iinfo(np.uint64).max
# (n, d, nq, k, metric): d = 32 / 128 / 16 / 48 the 4-lanes-per-row scan, d = 100 / 7 the one-lane-per-row recipes; n = 40 just above
# one 32-row bitmap word, n = 9 below k; n = 2003 with nq = 9 is more than one row chunk; nq never a multiple of the 8-query tile
SHAPES = [(777, 32, 37, 10, L2), (2003, 128, 9, 64, L2), (40, 16, 5, 10, L2), (9, 16, 3, 10, L2), (1501, 48, 21, 10, IP),
          (1203, 100, 13, 10, L2), (900, 7, 11, 10, L2)]


@pytest.fixture(scope="module")
def hs():
    return load_product()


@pytest.fixture(scope="module")
def oracle():
    return Oracle()


@functools.lru_cache(maxsize=None)
def data(n, d, nq):
    base = mixture(n, d, 5, lo=0, hi=4, sigma=1.0, integer=True)
    q = mixture(nq, d, 6, lo=0, hi=4, sigma=1.0, integer=True)
    labels = np.random.default_rng(3).permutation(n).astype(np.uint64) * 7 + 5
    for a in (base, q, labels):
        a.setflags(write=False)
    return base, q, labels


@functools.lru_cache(maxsize=None)
def filters(n):
    """all allowed, none allowed, fewer than k (3 ids), the ids on either side of the 32-row unit boundaries and the last one, random 10 %"""
    f = np.zeros((5, n), np.uint8)
    f[0] = 1
    f[2, [i for i in (1, n // 2, n - 2) if 0 <= i < n]] = 1
    f[3, [i for i in (0, 31, 32, 63, 64, n - 1) if i < n]] = 1
    f[4] = np.random.default_rng(1).random(n) < 0.1
    f.setflags(write=False)
    return f


_graphs = {}


def graph(hs, tmp_path_factory, n, d, metric):
    """(Slim file, parsed Slim graph) over data(n, d, .)'s rows, built once per shape."""
    key = (n, d, metric)
    if key not in _graphs:
        t = tmp_path_factory.mktemp(f"exact_{n}_{d}_{metric}")
        hp, sp = str(t / "h.bin"), str(t / "s.bin")
        hs.build_hnsw(data(n, d, 1)[0], hp, metric=metric, M=8, ef_construction=40, threads=4)
        hs.convert_slim(hp, sp, d, metric=metric, threads=4)
        _graphs[key] = (sp, load_chal_encode().parse_slim(open(sp, "rb").read(), d))
    return _graphs[key]


def make_index(hs, tmp_path_factory, n, d, metric, labels, deleted=None, rows=None):
    _, s = graph(hs, tmp_path_factory, n, d, metric)
    return hs.Index.from_arrays(hs.HS_KIND_SLIM, metric, s["rows"] if rows is None else rows, s["level"], s["lists"], s["enterpoint"],
                                s["maxlevel"], labels=labels, deleted=deleted)


_refs = {}


def references(hs, oracle, metric, base, q, k, labels, mask, key):
    """The two expected answers of queries q over the candidates mask, padded to k: (labels, dists, count) twice.  Cached by key."""
    if key not in _refs:
        ids = np.flatnonzero(mask)
        c = min(k, len(ids))
        out = []
        for how in ("lexsort", "brute_force"):
            L = np.full((len(q), k), NONE64, np.uint64)
            D = np.full((len(q), k), np.inf, np.float32)
            if c:
                if how == "lexsort":
                    el, ed = _expect(oracle, metric, np.ascontiguousarray(base[ids]), q, c, np.ascontiguousarray(labels[ids]))
                else:
                    el, ed, ec = hs.brute_force(np.ascontiguousarray(base[ids]), q, c, metric, labels=np.ascontiguousarray(labels[ids]))
                    assert np.all(ec == c)
                L[:, :c], D[:, :c] = el, ed
            L.setflags(write=False); D.setflags(write=False)
            out.append((L, D, c))
        _refs[key] = out
    return _refs[key]


def same(r, sel, refs, what):
    for L, D, c in refs:
        assert np.all(r["cnt"][sel] == c), what
        assert np.array_equal(r["labels"][sel], L), what
        assert r["dists"][sel].tobytes() == D.tobytes(), what


def same_bits(a, b, what):
    for key in ("labels", "dists", "cnt"):
        assert a[key].tobytes() == b[key].tobytes(), f"{what}: {key}"


# ---- 1. every shape: unfiltered, five filters interleaved, the same call sorted -------------------------------------------------------
@pytest.mark.parametrize("n,d,nq,k,metric", SHAPES, ids=lambda v: str(v))
def test_exact_search_matches_both_references(hs, oracle, tmp_path_factory, n, d, nq, k, metric):
    base, q, labels = data(n, d, nq)
    ix = make_index(hs, tmp_path_factory, n, d, metric, labels)
    filt = filters(n)
    r = ix.exact_search(q, k)
    assert ix.last_kernel() == ("hs::exact_scan_kernel" if d % 16 == 0 else "hs::exact_scan_general_kernel")
    same(r, slice(None), references(hs, oracle, metric, base, q, k, labels, filt[0], (n, d, nq, k, "all")), "unfiltered")
    fs = hs.FilterSet.create(ix, 5)
    fs.write(0, filt)
    foq = (np.arange(nq) % 5).astype(np.uint32)
    r = ix.exact_search(q, k, fs, foq)
    for f in range(5):
        sel = foq == f
        if sel.any():
            same(r, sel, references(hs, oracle, metric, base, np.ascontiguousarray(q[sel]), k, labels, filt[f], (n, d, nq, k, f)), f"filter {f}")
    assert np.all(r["cnt"][foq == 1] == 0) and np.all(r["cnt"][foq == 0] == min(k, n))
    # the same call with filter_of_query sorted: the permutation and the skip change nothing per query
    order = np.argsort(foq, kind="stable")
    rs = ix.exact_search(np.ascontiguousarray(q[order]), k, fs, foq[order])
    same_bits({key: v[order] for key, v in r.items()}, rs, "sorted")


def test_more_queries_than_one_launch_group(hs, tmp_path_factory):
    """262 144 queries are one launch group (grid.y counts tiles of 8): 37 more make a second one, at an offset into the queries, the
    filter indices, the order and the outputs.  The queries are the 5 of the n = 40 shape over and over, so the answers repeat."""
    n, d, nq, k, metric = SHAPES[2]
    base, q, labels = data(n, d, nq)
    ix = make_index(hs, tmp_path_factory, n, d, metric, labels)
    fs = hs.FilterSet.create(ix, 5)
    fs.write(0, filters(n))
    big = 262144 + 37
    reps = big // 5 + 1                                   # query i is q[i % 5] under filter (i // 5) % 5
    foq = np.repeat(np.arange(reps) % 5, 5)[:big].astype(np.uint32)
    qq = np.ascontiguousarray(np.tile(q, (reps, 1))[:big])
    small = ix.exact_search(np.ascontiguousarray(np.tile(q, (5, 1))), k, fs, np.repeat(np.arange(5), 5).astype(np.uint32))   # the 25 (filter, query) pairs
    r = ix.exact_search(qq, k, fs, foq)
    pick = (foq * 5 + np.arange(big) % 5).astype(np.int64)
    same_bits({key: v[pick] for key, v in small.items()}, r, "two launch groups")
    same_bits({key: v[:5] for key, v in ix.exact_search(q, k).items()}, {key: v[big - big % 5 - 5:big - big % 5] for key, v in ix.exact_search(qq, k).items()},
              "two launch groups, unfiltered")


# ---- 2. delete marks, alone and with a filter ------------------------------------------------------------------------------------
def test_delete_marks_alone_and_with_a_filter(hs, oracle, tmp_path_factory):
    n, d, nq, k, metric = SHAPES[0]
    base, q, labels = data(n, d, nq)
    deleted = (np.random.default_rng(8).random(n) < 0.3).astype(np.uint8)
    deleted[[0, 31, 32, n - 1]] = (1, 0, 1, 1)
    ix = make_index(hs, tmp_path_factory, n, d, metric, labels, deleted=deleted)
    assert ix.info()["has_deleted"] == 1
    filt = filters(n)
    same(ix.exact_search(q, k), slice(None), references(hs, oracle, metric, base, q, k, labels, deleted == 0, ("del", "alone")), "delete marks")
    fs = hs.FilterSet.create(ix, 5)
    fs.write(0, filt)
    foq = (np.arange(nq) % 5).astype(np.uint32)
    r = ix.exact_search(q, k, fs, foq)
    for f in range(5):
        sel = foq == f
        same(r, sel, references(hs, oracle, metric, base, np.ascontiguousarray(q[sel]), k, labels, (filt[f] != 0) & (deleted == 0), ("del", f)),
             f"delete marks and filter {f}")
    assert np.array_equal(fs.read(0), np.ones(n, np.uint8))   # the marks are not folded into the rows


# ---- 3. narrow rows ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt_name", ("HS_ROWS_U8", "HS_ROWS_F16"))
@pytest.mark.parametrize("shape", (SHAPES[0], SHAPES[4]), ids=("l2_d32", "ip_d48"))
def test_narrow_rows_give_the_same_bits(hs, tmp_path_factory, shape, fmt_name):
    """Both copies resident, fp32 dropped, load_narrow: the bits of the fp32 index, by the narrow scan.  d = 32 has a dword-aligned
    u8 chunk per lane, d = 48 (three 16-element steps) has not."""
    n, d, nq, k, metric = shape
    fmt, name = getattr(hs, fmt_name), "hs::exact_scan_kernel" + ("_u8" if fmt_name == "HS_ROWS_U8" else "_f16")
    base, q, labels = data(n, d, nq)
    sp, _ = graph(hs, tmp_path_factory, n, d, metric)
    filt = filters(n)
    foq = (np.arange(nq) % 5).astype(np.uint32)

    def run(ix):
        fs = hs.FilterSet.create(ix, 5)
        fs.write(0, filt)
        return ix.exact_search(q, k), ix.exact_search(q, k, fs, foq)

    ix = hs.Index(sp, hs.HS_KIND_SLIM, d, metric=metric)
    a = run(ix)
    assert ix.last_kernel() == "hs::exact_scan_kernel"
    ix.set_row_format(fmt)
    b = run(ix)
    assert ix.last_kernel() == name
    ix.set_f32_resident(False)
    c = run(ix)
    assert ix.last_kernel() == name
    nx = hs.Index.load_narrow(sp, hs.HS_KIND_SLIM, d, fmt, metric=metric)
    e = run(nx)
    assert nx.last_kernel() == name
    for other, what in ((b, "both copies"), (c, "fp32 dropped"), (e, "load_narrow")):
        same_bits(a[0], other[0], what)
        same_bits(a[1], other[1], what + ", filtered")


# ---- 4. device entry -------------------------------------------------------------------------------------------------------------
def test_device_entry_on_a_stream_and_a_bad_filter_index(hs, tmp_path_factory):
    """The device entry forms its tiles in the order given: with filters interleaved every tile mixes all five.  One filter index
    >= nf: count 0 and padding for that query, HS_ERR_INVALID from check, the other queries intact."""
    import torch
    n, d, nq, k, metric = SHAPES[0]
    base, q, labels = data(n, d, nq)
    ix = make_index(hs, tmp_path_factory, n, d, metric, labels)
    fs = hs.FilterSet.create(ix, 5)
    fs.write(0, filters(n))
    foq = (np.arange(nq) % 5).astype(np.uint32)
    want = ix.exact_search(q, k, fs, foq)
    want0 = ix.exact_search(q, k)
    dev = torch.device("cuda:0")
    st = torch.cuda.Stream(device=dev)

    def out():
        return (torch.zeros((nq, k), dtype=torch.int64, device=dev), torch.zeros((nq, k), dtype=torch.float32, device=dev),
                torch.zeros(nq, dtype=torch.int32, device=dev))

    def host(lab, dist, cnt):
        return dict(labels=lab.cpu().numpy().view(np.uint64), dists=dist.cpu().numpy(), cnt=cnt.cpu().numpy().view(np.uint32))

    with torch.cuda.stream(st):
        dq = torch.from_numpy(q.copy()).to(dev)
        o = out()
        ix.exact_search_dev(dq, k, *o, fs=fs, d_filter_of_query=torch.from_numpy(foq.astype(np.int32)).to(dev), stream=st.cuda_stream)
        ix.check(st.cuda_stream)
        same_bits(want, host(*o), "device entry, filters interleaved")
        o = out()
        ix.exact_search_dev(dq, k, *o, stream=st.cuda_stream)
        ix.check(st.cuda_stream)
        same_bits(want0, host(*o), "device entry, unfiltered")
        bad = foq.copy()
        bad[11] = 5
        o = out()
        ix.exact_search_dev(dq, k, *o, fs=fs, d_filter_of_query=torch.from_numpy(bad.astype(np.int32)).to(dev), stream=st.cuda_stream)
        with pytest.raises(hs.HsError) as e:
            ix.check(st.cuda_stream)
        assert e.value.status == hs.HS_ERR_INVALID
        got = host(*o)
        assert got["cnt"][11] == 0 and np.all(got["labels"][11] == NONE64) and np.all(np.isinf(got["dists"][11]))
        keep = np.arange(nq) != 11
        same_bits({key: v[keep] for key, v in want.items()}, {key: v[keep] for key, v in got.items()}, "the other queries")
        ix.check(st.cuda_stream)   # read and cleared
    st.synchronize()


# ---- 5. the compiled reference ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,metric", (("l2_cont", L2), ("l2_int", L2), ("ip", IP)))
def test_unfiltered_vs_compiled_bruteforce(hs, tmp_path, name, metric):
    """An index built over each base of tests/golden/bruteforce_ref.npz, unfiltered: the outputs of the COMPILED
    hnswlib::BruteforceSearch::searchKnn (bruteforce.h:106-135), labels and fp32 bits (d = 24, 8, 48)."""
    g = np.load(os.path.join(GOLDEN, "bruteforce_ref.npz"))
    base, q = g[f"{name}_base"], g[f"{name}_queries"]
    hp = str(tmp_path / "h.bin")
    hs.build_hnsw(base, hp, metric=metric, M=8, ef_construction=40, threads=4)
    ix = hs.Index(hp, hs.HS_KIND_HNSW, base.shape[1], metric=metric)
    for k in (1, 10, 33):
        r = ix.exact_search(q, k)
        assert np.all(r["cnt"] == k)
        assert np.array_equal(r["labels"], g[f"{name}_k{k}_labels"][:, ::-1]), f"{name} k={k}"   # pop order is farthest first
        assert r["dists"].tobytes() == np.ascontiguousarray(g[f"{name}_k{k}_dists"][:, ::-1]).tobytes(), f"{name} k={k}"


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_index_untouched(hs, tmp_path_factory, tmp_path):
    import ctypes
    from test_gpu_slimq import build
    n, d, nq, k, metric = SHAPES[0]
    base, q, labels = data(n, d, nq)
    ix = make_index(hs, tmp_path_factory, n, d, metric, labels)
    other = make_index(hs, tmp_path_factory, 40, 16, L2, data(40, 16, 5)[2])
    fs, fs_other = hs.FilterSet.create(ix, 2), hs.FilterSet.create(other, 2)
    fs.write(0, filters(n)[[0, 4]])
    foq = (np.arange(nq) % 2).astype(np.uint32)
    before, info = (ix.exact_search(q, k), ix.exact_search(q, k, fs, foq)), ix.info()

    def refused(status, call):
        with pytest.raises(hs.HsError) as e:
            call()
        assert e.value.status == status

    refused(hs.HS_ERR_UNSUPPORTED, lambda: ix.exact_search(q, 65))
    refused(hs.HS_ERR_UNSUPPORTED, lambda: ix.exact_search(q, 0))
    refused(hs.HS_ERR_INVALID, lambda: ix.exact_search(q, k, fs_other, foq))          # a set of another n
    refused(hs.HS_ERR_INVALID, lambda: ix.exact_search(q, k, fs, None))               # a set without filter_of_query
    refused(hs.HS_ERR_INVALID, lambda: ix.exact_search(q, k, None, foq))              # and the reverse
    refused(hs.HS_ERR_INVALID, lambda: ix.exact_search(q, k, fs, np.where(np.arange(nq) == 3, 2, foq)))   # a host filter index >= nf
    L = hs.lib()
    ol, od = np.zeros((nq, k), np.uint64), np.zeros((nq, k), np.float32)
    assert L.hs_index_exact_search(ix._h, None, None, nq, k, None, ol.ctypes.data, od.ctypes.data, None) == hs.HS_ERR_INVALID
    assert L.hs_index_exact_search(ix._h, None, q.ctypes.data, nq, k, None, None, od.ctypes.data, None) == hs.HS_ERR_INVALID
    assert L.hs_index_exact_search(ix._h, None, q.ctypes.data, nq, k, None, ol.ctypes.data, None, None) == hs.HS_ERR_INVALID
    assert L.hs_index_exact_search_dev(ix._h, None, None, nq, k, None, ol.ctypes.data, od.ctypes.data, None, None) == hs.HS_ERR_INVALID
    assert L.hs_index_exact_search(ix._h, None, q.ctypes.data, 0, k, None, ol.ctypes.data, od.ctypes.data, None) == hs.HS_OK   # nq == 0
    assert L.hs_index_exact_search(ix._h, None, q.ctypes.data, nq, k, None, ol.ctypes.data, od.ctypes.data, None) == hs.HS_OK   # counts are optional
    assert np.array_equal(ol, before[0]["labels"])
    b128 = mixture(1500, 128, 1, integer=True)
    qx = hs.Index(build(hs, tmp_path, "q", b128, L2, 8), hs.HS_KIND_SLIMQ, 128)
    qx.slimq_set_dataset(b128)
    refused(hs.HS_ERR_UNSUPPORTED, lambda: qx.exact_search(b128[:3], k))
    assert ix.info() == info
    after = (ix.exact_search(q, k), ix.exact_search(q, k, fs, foq))
    same_bits(before[0], after[0], "after the refusals")
    same_bits(before[1], after[1], "after the refusals, filtered")


# ---- 7. facade -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["hnsw", "slim"])
def test_facade_exact_equals_the_binding(hs, tmp_path, kind):
    """searchKnnExact(q, k[, isIdAllowed]) one call per query (no functor, label % 2 == 0, label % 3 != 0 taking turns; labels are
    row indices here) and searchKnnExactBatch through hnswlib_amd.h: the binding's answers."""
    exe = os.path.join(ROOT, "hnsw-slim_amd", "facade_exact")
    assert os.path.exists(exe), "facade_exact is built by `make -C hnsw-slim_amd all`"
    n, d, nq, k = 777, 32, 13, 10
    base, q, _ = data(n, d, nq)
    hp, sp = str(tmp_path / "h.bin"), str(tmp_path / "s.bin")
    hs.build_hnsw(base, hp, M=8, ef_construction=40, threads=4)
    hs.convert_slim(hp, sp, d, threads=4)
    path = hp if kind == "hnsw" else sp
    qf, out = str(tmp_path / "q.f32"), str(tmp_path / "out.bin")
    q.tofile(qf)
    subprocess.check_call([exe, kind, path, str(d), qf, str(nq), str(k), out])
    ix = hs.Index(path, hs.HS_KIND_HNSW if kind == "hnsw" else hs.HS_KIND_SLIM, d)
    ids = np.arange(n)
    fs = hs.FilterSet.create(ix, 3)
    fs.write(0, np.stack([np.ones(n, bool), ids % 2 == 0, ids % 3 != 0]).astype(np.uint8))
    want = ix.exact_search(q, k, fs, (np.arange(nq) % 3).astype(np.uint32))
    buf, off = open(out, "rb").read(), 0
    for i in range(nq):
        c = int(np.frombuffer(buf, np.uint32, 1, off)[0]); off += 4
        rec = np.frombuffer(buf, np.dtype([("d", "<f4"), ("l", "<u8")]), c, off); off += 12 * c
        assert c == int(want["cnt"][i]) == k, i
        assert np.array_equal(rec["l"], want["labels"][i]) and rec["d"].tobytes() == want["dists"][i].tobytes(), i
    batch = ix.exact_search(q, k)
    assert buf[off:off + nq * k * 8] == batch["labels"].tobytes(); off += nq * k * 8
    assert buf[off:off + nq * k * 4] == batch["dists"].tobytes(); off += nq * k * 4
    assert buf[off:off + nq * 4] == batch["cnt"].tobytes(); off += nq * 4
    assert off == len(buf)
