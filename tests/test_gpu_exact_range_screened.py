"""The screened exact range search (hs_index_exact_range_screened[_dev], csrc/exact_range_screen.hip): an MFMA screen against the
radius, a re-rank of the survivors in the recipe's arithmetic, exact_range's passes for the queries the screen cannot decide.  Every
answer is compared byte for byte -- offsets, labels, fp32 distance bits -- with the float64 table of tests/test_gpu_exact_range.py
where rows and queries are small integers, and with exact_range itself on continuous data."""
import numpy as np
import pytest

from hsutil import mixture
from test_gpu_exact_range import IP, L2, SUFFIX, hs, ints, perm_labels, radii, reference, ring, same, table  # noqa: F401 (hs: the fixture)

pytestmark = pytest.mark.gpu


def index(hs, metric, base, labels, fmt_name="HS_ROWS_F32", deleted=None):
    ix = ring(hs, metric, base, labels, deleted)
    if fmt_name != "HS_ROWS_F32":
        ix.set_row_format(getattr(hs, fmt_name))
    return ix


def stats(ix, nq, fell_back):
    s = ix.exact_screen_stats()
    assert (s["screened"], s["fell_back"]) == (nq - fell_back, fell_back), s


# ---- 1. unit and wave boundaries, a partial tile and a tile plus one, the six row formats, both metrics -------------------------------
@pytest.mark.parametrize("fmt_name", tuple(SUFFIX))
@pytest.mark.parametrize("metric", (L2, IP))
def test_small_integers(hs, fmt_name, metric):
    for n, d, nq in [(n, 16, nq) for n in (1, 63, 65, 300) for nq in (1, 9, 65)] + [(300, 128, 9)]:
        base, q, labels = ints(n, d, 5), ints(nq, d, 6), perm_labels(n)
        ix = index(hs, metric, base, labels, fmt_name)
        t = table(metric, base, q)
        r = radii(t) if nq > 1 else radii(t[[0] * 5])[n % 5:n % 5 + 1]
        off, lab, dist = got = ix.exact_range_screened(q, r)
        same(reference(t, r, labels), got, f"n = {n}, d = {d}, nq = {nq}")
        assert ix.last_kernel() == "hs::xrs_screen_kernel" + SUFFIX[fmt_name]
        stats(ix, nq, 0)   # (n <= the list capacity: the +inf radii stay screened too)
        assert all(off[i + 1] - off[i] == n for i in range(nq) if np.isposinf(r[i]))


# ---- 2. continuous data: radii between neighbouring distances, then equal to a distance the scan returned -----------------------------
@pytest.mark.parametrize("metric", (L2, IP))
def test_floats_and_radii_on_the_boundary(hs, metric):
    n, d, nq = 300, 128, 9
    base, q, labels = mixture(n, d, 5), mixture(nq, d, 6), perm_labels(n)
    ix = index(hs, metric, base, labels)
    t = table(metric, base, q)
    s = np.sort(t, axis=1)
    r = np.array([(s[i, 20 * i + 3] + s[i, 20 * i + 4]) / 2 for i in range(nq)], np.float32)
    off, lab, dist = scan = ix.exact_range(q, r)
    got = ix.exact_range_screened(q, r)
    same(scan, got, "halfway radii")
    want = reference(t, r, labels)
    assert want[0].tobytes() == got[0].tobytes()
    for i in range(nq):   # (fp32 rounding may order two nearly equal distances unlike float64: the reference decides the members)
        a, b = int(off[i]), int(off[i + 1])
        assert np.array_equal(np.sort(want[1][a:b]), np.sort(got[1][a:b])), f"query {i}"
    # the boundary the margin must not cut: each query's radius is the fp32 distance of its own last result
    rb = np.array([dist[int(off[i + 1]) - 1] for i in range(nq)], np.float32)
    scan = ix.exact_range(q, rb)
    assert scan[0].tobytes() == off.tobytes()   # (the row at the radius is in)
    same(scan, ix.exact_range_screened(q, rb), "radii equal to a returned distance")
    stats(ix, nq, 0)


# ---- 3. the list capacity: as many survivors as the list holds, and one more -----------------------------------------------------------
@pytest.mark.parametrize("extra", (0, 1))
def test_list_capacity_edge(hs, extra):
    n = hs.HS_EXACT_RANGE_SCREEN_LIST + extra
    row = ints(1, 16, 5)
    base, labels = np.repeat(row, n, axis=0), perm_labels(n)
    q = np.concatenate([row, row + 1.0])           # the second query: distance 16 to every row
    r = np.array([0.0, 0.5], np.float32)
    ix = index(hs, L2, base, labels)
    off, lab, dist = got = ix.exact_range_screened(q, r)
    same(reference(table(L2, base, q), r, labels), got, f"n = {n}")
    assert off[1] == n and off[2] == n
    stats(ix, 2, extra)


# ---- 4. several row chunks (the +inf radii overflow their lists); the longest tile staged whole, and one staged in slices ---------------
@pytest.mark.parametrize("n,d", ((5003, 16), (300, 624), (300, 640)))
@pytest.mark.parametrize("metric", (L2, IP))
def test_row_chunks_and_a_sliced_tile(hs, metric, n, d):
    nq = 9
    base, q, labels = ints(n, d, 5), ints(nq, d, 6), perm_labels(n)
    t = table(metric, base, q)
    r = radii(t)
    ix = index(hs, metric, base, labels)
    same(reference(t, r, labels), ix.exact_range_screened(q, r), f"n = {n}, d = {d}")
    s = ix.exact_screen_stats()
    assert s["screened"] + s["fell_back"] == nq
    assert s["fell_back"] >= 2 if n > hs.HS_EXACT_RANGE_SCREEN_LIST else s["fell_back"] == 0   # queries 3 and 8: radius +inf


# ---- 5. delete marks, a filter per query (one allows nothing), the capacity rule on both entries ----------------------------------------
def test_marks_filters_capacity_and_the_device_entry(hs):
    import torch
    n, d, nq = 700, 16, 9
    base, q, labels = ints(n, d, 5), ints(nq, d, 6), perm_labels(n)
    deleted = (np.random.default_rng(8).random(n) < 0.3).astype(np.uint8)
    deleted[[0, 31, 32, n - 1]] = (1, 0, 1, 1)
    ix = index(hs, L2, base, labels, deleted=deleted)
    t = table(L2, base, q)
    r = radii(t)
    same(reference(t, r, labels, [deleted == 0] * nq), ix.exact_range_screened(q, r), "delete marks")
    filt = np.zeros((3, n), np.uint8)
    filt[0] = np.random.default_rng(1).random(n) < 0.6
    filt[1, [1, 31, 32, 33, 350, n - 2]] = 1
    fs = hs.FilterSet.create(ix, 3)
    fs.write(0, filt)
    foq = np.array([0, 2, 1, 1, 0, 2, 0, 0, 1], np.uint32)
    r[[1, 2]] = np.inf   # (also under the filter that allows nothing, and the one that allows six rows)
    want = reference(t, r, labels, [(filt[f] != 0) & (deleted == 0) for f in foq])
    same(want, ix.exact_range_screened(q, r, fs, foq), "filters")
    stats(ix, nq, 0)
    # capacity, host entry: one short -> HS_ERR_CAPACITY with the total in the message, offsets written, outputs untouched
    total = int(want[0][-1])
    L = hs.lib()
    for cap in (total - 1, total):
        off, lab, dist = np.zeros(nq + 1, np.uint64), np.full(total, 77, np.uint64), np.full(total, -5.0, np.float32)
        st = L.hs_index_exact_range_screened(ix._h, fs._h, q.ctypes.data, nq, r.ctypes.data, foq.ctypes.data, cap, off.ctypes.data, lab.ctypes.data,
                                             dist.ctypes.data)
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
            ix.exact_range_screened_dev(dq, dr, *o, fs=fs, d_filter_of_query=df, stream=st.cuda_stream)
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


# ---- 6. a query the screen cannot decide: its norm overflows, every interval of it is infinite ------------------------------------------
def test_a_query_of_overflowing_norm_falls_back_alone(hs):
    n, d, nq = 300, 16, 9
    base, q, labels = ints(n, d, 5), ints(nq, d, 6), perm_labels(n)
    r = radii(table(L2, base, q))
    q[4], r[4] = 1e19, np.inf   # |q|^2 = 1.6e39 = +inf in fp32, and so is every L2 distance of the query
    ix = index(hs, L2, base, labels)
    off, lab, dist = scan = ix.exact_range(q, r)
    assert off[5] - off[4] == n and np.all(np.isposinf(dist[int(off[4]):int(off[5])]))
    same(scan, ix.exact_range_screened(q, r), "overflowing query")
    stats(ix, nq, 1)
