"""Exact range search (hs_index_exact_range[_dev], csrc/exact_range.hip) against a float64 distance table with d <= r, sorted by
(dist, label).

Rows and queries are small integers (mixture(integer=True), at most 15: every narrow format holds them): every partial sum of the
fp32 recipes is an integer below 2^24, so the float64 table has the distance bits and membership at a radius equal to an achieved
distance is crisp.  Where n <= 1024 the result is also held against exact_search_wide(k = n): a range result is a prefix of that
list.  The exact search never follows an edge, so the indexes are a ring over the rows; labels are 1000 + a permutation."""
import numpy as np
import pytest

from hsutil import load_product, mixture, write_vanilla_level0

pytestmark = pytest.mark.gpu
L2, IP = 0, 1
SUFFIX = {"HS_ROWS_F32": "", "HS_ROWS_U8": "_u8", "HS_ROWS_I8": "_i8", "HS_ROWS_F16": "_f16", "HS_ROWS_BF16": "_bf16", "HS_ROWS_F8": "_f8"}


@pytest.fixture(scope="module")
def hs():
    return load_product()


def ints(n, d, seed):
    return np.minimum(mixture(n, d, seed, lo=2.0, hi=9.0, sigma=2.5, integer=True), 15.0)


def perm_labels(n):
    return np.random.default_rng(3).permutation(n).astype(np.uint64) + 1000


def ring(hs, metric, rows, labels=None, deleted=None):
    n = len(rows)
    lists = [[[(j + 1) % n] if n > 1 else []] for j in range(n)]
    return hs.Index.from_arrays(hs.HS_KIND_HNSW, metric, rows, np.zeros(n, np.int32), lists, 0, 0, labels=labels, deleted=deleted)


def table(metric, base, q):
    b, qq = base.astype(np.float64), q.astype(np.float64)
    return ((qq[:, None, :] - b[None]) ** 2).sum(-1) if metric == L2 else 1.0 - qq @ b.T


def radii(d):
    """One radius per query, the kinds taking turns: an achieved distance that the most rows share, NaN, below every distance,
    +inf, the achieved distance a third of the way up."""
    r = np.empty(len(d), np.float32)
    for i, row in enumerate(d):
        vals, counts = np.unique(row, return_counts=True)
        r[i] = (vals[np.argmax(counts)], np.nan, row.min() - 1.0, np.inf, np.sort(row)[len(row) // 3])[i % 5]
    return r


def reference(d, radius, labels, masks=None):
    """(offsets, labels, dists) from the table `d`; masks[i]: the candidates of query i (None: every row)."""
    off, L, D = [0], [], []
    for i, row in enumerate(d):
        ids = np.arange(len(row)) if masks is None else np.flatnonzero(masks[i])
        ids = ids[row[ids] <= np.float64(radius[i])]
        o = ids[np.lexsort((labels[ids], row[ids]))]
        L.append(labels[o]); D.append(row[o].astype(np.float32)); off.append(off[-1] + len(o))
    return np.array(off, np.uint64), np.concatenate(L).astype(np.uint64), np.concatenate(D).astype(np.float32)


def same(want, got, what):
    for w, g, key in zip(want, got, ("offsets", "labels", "dists")):
        assert w.tobytes() == g.tobytes(), f"{what}: {key}"


def prefix_of_wide(ix, q, got, fs=None, foq=None):
    """Every segment is the head of exact_search_wide's list for k = n: the same labels, the same distance bits."""
    w = ix.exact_search_wide(q, min(ix.info()["n"], 1024), fs, foq)
    off, lab, dist = got
    for i in range(len(q)):
        m = int(off[i + 1] - off[i])
        assert m <= w["cnt"][i]
        assert lab[int(off[i]):int(off[i + 1])].tobytes() == w["labels"][i, :m].tobytes()
        assert dist[int(off[i]):int(off[i + 1])].tobytes() == w["dists"][i, :m].tobytes()


# ---- 1. unit and wave boundaries, a partial tile and a tile plus one, three row formats, both metrics ------------------------------
@pytest.mark.parametrize("fmt_name", ("HS_ROWS_F32", "HS_ROWS_U8", "HS_ROWS_F16"))
@pytest.mark.parametrize("metric", (L2, IP))
@pytest.mark.parametrize("nq", (1, 9))
def test_small_n_at_dim_16(hs, fmt_name, metric, nq):
    for n in (1, 63, 65, 300):
        base, q, labels = ints(n, 16, 5), ints(nq, 16, 6), perm_labels(n)
        ix = ring(hs, metric, base, labels)
        if fmt_name != "HS_ROWS_F32":
            ix.set_row_format(getattr(hs, fmt_name))
        d = table(metric, base, q)
        r = radii(d) if nq > 1 else radii(d[[0] * 5])[n % 5:n % 5 + 1]
        got = ix.exact_range(q, r)
        same(reference(d, r, labels), got, f"n = {n}")
        assert ix.last_kernel() == "hs::exact_range_kernel" + SUFFIX[fmt_name]
        prefix_of_wide(ix, q, got)


# ---- 2. the one-lane-per-row recipes (d = 20), a longer row (d = 128), the other narrow formats, an fp32-free index ------------------
@pytest.mark.parametrize("d,metric,fmt_name", ((20, L2, "HS_ROWS_F32"), (20, IP, "HS_ROWS_F32"), (128, L2, "HS_ROWS_F32"), (128, IP, "HS_ROWS_U8"),
                                              (128, IP, "HS_ROWS_I8"), (128, L2, "HS_ROWS_BF16"), (128, L2, "HS_ROWS_F8")))
def test_dims_and_formats(hs, d, metric, fmt_name):
    n, nq = 300, 9
    base, q, labels = ints(n, d, 5), ints(nq, d, 6), perm_labels(n)
    ix = ring(hs, metric, base, labels)
    if fmt_name != "HS_ROWS_F32":
        ix.set_row_format(getattr(hs, fmt_name))
    t = table(metric, base, q)
    r = radii(t)
    got = ix.exact_range(q, r)
    same(reference(t, r, labels), got, fmt_name)
    assert ix.last_kernel() == ("hs::exact_range_general_kernel" if d % 16 else "hs::exact_range_kernel" + SUFFIX[fmt_name])
    prefix_of_wide(ix, q, got)


def test_load_narrow(hs, tmp_path):
    n, d, nq = 300, 32, 9
    base, q = ints(n, d, 5), ints(nq, d, 6)
    path = str(tmp_path / "ring.bin")
    write_vanilla_level0(path, base, [[(j + 1) % n] for j in range(n)], 4)   # (the file's labels are the row indices)
    ix = hs.Index.load_narrow(path, hs.HS_KIND_HNSW, d, hs.HS_ROWS_U8)
    t = table(L2, base, q)
    r = radii(t)
    same(reference(t, r, np.arange(n, dtype=np.uint64)), ix.exact_range(q, r), "load_narrow")
    assert ix.last_kernel() == "hs::exact_range_kernel_u8"


# ---- 3. several row chunks; with radius = +inf a segment beyond the sort's LDS capacity ----------------------------------------------
@pytest.mark.parametrize("metric", (L2, IP))
def test_row_chunks_and_long_segments(hs, metric):
    n, nq = 5003, 9
    base, q, labels = ints(n, 16, 5), ints(nq, 16, 6), perm_labels(n)
    t = table(metric, base, q)
    r = radii(t)
    off, lab, dist = got = ring(hs, metric, base, labels).exact_range(q, r)
    same(reference(t, r, labels), got, "five chunks")
    assert off[4] - off[3] == n and off[2] == off[1] == off[3]   # +inf: every candidate; NaN and below every distance: none


# ---- 4. continuous data: the scan's bits, radii halfway between neighbouring distances ------------------------------------------------
@pytest.mark.parametrize("metric", (L2, IP))
def test_floats_have_the_scans_bits(hs, metric):
    n, d, nq = 300, 128, 9
    base, q, labels = mixture(n, d, 5), mixture(nq, d, 6), perm_labels(n)
    t = table(metric, base, q)
    s = np.sort(t, axis=1)
    r = np.array([(s[i, 20 * i + 3] + s[i, 20 * i + 4]) / 2 for i in range(nq)], np.float32)
    ix = ring(hs, metric, base, labels)
    got = ix.exact_range(q, r)
    want = reference(t, r, labels)
    assert want[0].tobytes() == got[0].tobytes()
    # fp32 rounding may order two nearly equal distances unlike float64: the reference decides the members, the scan the order and the bits
    for i in range(nq):
        a, b = int(want[0][i]), int(want[0][i + 1])
        assert np.array_equal(np.sort(want[1][a:b]), np.sort(got[1][a:b])), f"query {i}"
    prefix_of_wide(ix, q, got)


# ---- 5. delete marks, a filter per query (one allows nothing), the capacity rule on both entries -------------------------------------
def test_marks_filters_capacity_and_the_device_entry(hs):
    import torch
    n, d, nq = 700, 16, 9
    base, q, labels = ints(n, d, 5), ints(nq, d, 6), perm_labels(n)
    deleted = (np.random.default_rng(8).random(n) < 0.3).astype(np.uint8)
    deleted[[0, 31, 32, n - 1]] = (1, 0, 1, 1)
    ix = ring(hs, L2, base, labels, deleted)
    t = table(L2, base, q)
    r = radii(t)
    got = ix.exact_range(q, r)
    same(reference(t, r, labels, [deleted == 0] * nq), got, "delete marks")
    prefix_of_wide(ix, q, got)
    filt = np.zeros((3, n), np.uint8)
    filt[0] = np.random.default_rng(1).random(n) < 0.6
    filt[1, [1, 31, 32, 33, 350, n - 2]] = 1
    fs = hs.FilterSet.create(ix, 3)
    fs.write(0, filt)
    foq = np.array([0, 2, 1, 1, 0, 2, 0, 0, 1], np.uint32)
    r[[1, 2]] = np.inf   # (also under the filter that allows nothing, and the one that allows six rows)
    want = reference(t, r, labels, [(filt[f] != 0) & (deleted == 0) for f in foq])
    got = ix.exact_range(q, r, fs, foq)
    same(want, got, "filters")
    assert got[0][2] == got[0][1] and 1 <= got[0][3] - got[0][2] <= 5   # filter 2 allows nothing; filter 1: six rows, row 32 is deleted
    prefix_of_wide(ix, q, got, fs, foq)
    # capacity, host entry: one short -> HS_ERR_CAPACITY with the total in the message, offsets written, outputs untouched
    total = int(want[0][-1])
    L = hs.lib()
    for cap in (total - 1, total):
        off, lab, dist = np.zeros(nq + 1, np.uint64), np.full(total, 77, np.uint64), np.full(total, -5.0, np.float32)
        st = L.hs_index_exact_range(ix._h, fs._h, q.ctypes.data, nq, r.ctypes.data, foq.ctypes.data, cap, off.ctypes.data, lab.ctypes.data, dist.ctypes.data)
        assert off.tobytes() == want[0].tobytes()
        if cap < total:
            assert st == hs.HS_ERR_CAPACITY and str(total) in hs.last_error() and np.all(lab == 77) and np.all(dist == -5.0)
        else:
            assert st == hs.HS_OK
            same(want, (off, lab, dist), "cap = total")
    # the device entry on a stream, tiles in the order given: the same, reported by check()
    dev = torch.device("cuda:0")
    st = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(st):
        dq, dr, df = (torch.from_numpy(a).to(dev) for a in (q, r, foq.astype(np.int32)))
        for cap in (total - 1, total):
            o = (torch.zeros(nq + 1, dtype=torch.int64, device=dev), torch.full((cap,), 77, dtype=torch.int64, device=dev),
                 torch.full((cap,), -5.0, dtype=torch.float32, device=dev))
            ix.exact_range_dev(dq, dr, *o, fs=fs, d_filter_of_query=df, stream=st.cuda_stream)
            if cap < total:
                with pytest.raises(hs.HsError) as e:
                    ix.check(st.cuda_stream)
                assert e.value.status == hs.HS_ERR_CAPACITY
                assert bool((o[1] == 77).all()) and bool((o[2] == -5.0).all())
            else:
                ix.check(st.cuda_stream)
                same(want, (o[0].cpu().numpy().view(np.uint64), o[1].cpu().numpy().view(np.uint64), o[2].cpu().numpy()), "device entry")
            assert o[0].cpu().numpy().view(np.uint64).tobytes() == want[0].tobytes()
    st.synchronize()
