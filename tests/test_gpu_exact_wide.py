"""Exact search for 64 < k <= 1024 (hs_index_exact_search_wide[_dev], csrc/exact_wide.hip).

Two references, neither the code under test:
 (a) integer rows and queries with d <= 256: every partial sum of the fp32 recipes is an integer below 2^24, so numpy in float64 gives
     the distance bits, and np.lexsort((label, dist)) the answer, ties included -- the values come from [0, 4), so ties are the rule;
 (b) Gaussian rows: the oracle's brute_force for the labels, its dist for the bits of every returned pair, exact_search for the
     first 64 positions.
The exact search never follows an edge, so the indexes are a ring over the rows.  Labels are a permutation times 7 plus 5: the
tie-break must follow the label, not the internal id."""
import numpy as np
import pytest

from hsutil import Oracle, load_product

pytestmark = pytest.mark.gpu
L2, IP = 0, 1
NONE64 = np.iinfo(np.uint64).max


@pytest.fixture(scope="module")
def hs():
    return load_product()


def ints(n, d, seed, hi=4):
    return np.random.default_rng(seed).integers(0, hi, (n, d)).astype(np.float32)


def perm_labels(n):
    return np.random.default_rng(3).permutation(n).astype(np.uint64) * 7 + 5


def ring(hs, metric, rows, labels=None, deleted=None):
    n = len(rows)
    nxt = (np.arange(n, dtype=np.uint32) + 1) % n
    if deleted is None:
        return hs.Index.from_csr(hs.HS_KIND_HNSW, metric, rows, np.zeros(n, np.int32), np.arange(n + 1, dtype=np.uint64), nxt, 0, 0, labels=labels)
    return hs.Index.from_arrays(hs.HS_KIND_HNSW, metric, rows, np.zeros(n, np.int32), [[[j]] for j in nxt], 0, 0, labels=labels, deleted=deleted)


def exact(metric, base, q, k, labels, mask=None):
    """Reference (a) over the candidates `mask`, padded to k."""
    ids = np.arange(len(base)) if mask is None else np.flatnonzero(mask)
    b, lab = base[ids].astype(np.float64), labels[ids]
    qq = q.astype(np.float64)
    d = ((qq[:, None, :] - b[None]) ** 2).sum(-1) if metric == L2 else 1.0 - qq @ b.T
    c = min(k, len(ids))
    L, D = np.full((len(q), k), NONE64, np.uint64), np.full((len(q), k), np.inf, np.float32)
    for i in range(len(q)):
        o = np.lexsort((lab, d[i]))[:c]
        L[i, :c], D[i, :c] = lab[o], d[i][o]
    return dict(labels=L, dists=D, cnt=np.full(len(q), c, np.uint32))


def same_bits(a, b, what):
    for key in ("labels", "dists", "cnt"):
        assert a[key].tobytes() == b[key].tobytes(), f"{what}: {key}"


# ---- 1. reference (a): n around k (count < k, exact fit, one to drop), several row chunks, the one-lane-per-row recipes ---------------
# (k, ns, nq, d, metric): nq = 1 a partial tile, nq = 9 more than one; n = 3001 / 4099 with these nq are 3 / 5 row chunks and a merge;
# d = 20 is hs::exact_wide_general_kernel; k = 65 / 128 / 1024 sit on the edges of the kept list's power of two; k <= 256 is a tile
# of 8 queries (k = 200: more than 64 KB of LDS), k = 400 one of 4, k >= 1000 one of 2
CASES = [(65, (64, 65, 66), 9, 16, L2), (100, (99, 100, 101), 1, 128, IP), (128, (127, 128, 129), 9, 128, L2),
         (1000, (999, 1000, 1001), 9, 16, IP), (1024, (1023, 1024, 1025), 1, 128, L2),
         (100, (3001,), 1, 128, L2), (400, (3001,), 9, 128, IP), (1000, (4099,), 9, 16, IP), (200, (3001,), 9, 20, L2), (100, (3001,), 9, 20, IP)]


@pytest.mark.parametrize("k,ns,nq,d,metric", CASES, ids=lambda v: str(v).replace(" ", ""))
def test_wide_matches_the_float64_lexsort(hs, k, ns, nq, d, metric):
    for n in ns:
        base, q, labels = ints(n, d, 5), ints(nq, d, 6), perm_labels(n)
        ix = ring(hs, metric, base, labels)
        same_bits(exact(metric, base, q, k, labels), ix.exact_search_wide(q, k), f"n = {n}")
        assert ix.last_kernel() == ("hs::exact_wide_kernel" if d % 16 == 0 else "hs::exact_wide_general_kernel")


# ---- 2. rows sorted farthest first: every row is admitted, every round compacts, the threshold moves each time ---------------------
@pytest.mark.parametrize("k", (100, 1000))
def test_rows_farthest_first(hs, k):
    n, d, nq = 3001, 16, 2
    base, q, labels = ints(n, d, 7, hi=256), ints(nq, d, 8, hi=256), perm_labels(n)
    base = np.ascontiguousarray(base[np.argsort(-((base - q[0]) ** 2).sum(1), kind="stable")])
    same_bits(exact(L2, base, q, k, labels), ring(hs, L2, base, labels).exact_search_wide(q, k), "farthest first")


# ---- 3. delete marks and two filters in one batch, one of them allowing fewer than k rows; the device entry on a stream ----------------
def test_delete_marks_filters_and_the_device_entry(hs):
    import torch
    n, d, nq, k = 700, 16, 9, 100
    base, q, labels = ints(n, d, 5), ints(nq, d, 6), perm_labels(n)
    deleted = (np.random.default_rng(8).random(n) < 0.3).astype(np.uint8)
    deleted[[0, 31, 32, n - 1]] = (1, 0, 1, 1)
    ix = ring(hs, L2, base, labels, deleted)
    same_bits(exact(L2, base, q, k, labels, deleted == 0), ix.exact_search_wide(q, k), "delete marks")
    filt = np.zeros((2, n), np.uint8)
    filt[0] = np.random.default_rng(1).random(n) < 0.6
    filt[1, [1, 31, 32, 33, 350, n - 2]] = 1
    fs = hs.FilterSet.create(ix, 2)
    fs.write(0, filt)
    foq = (np.arange(nq) % 2).astype(np.uint32)
    want = ix.exact_search_wide(q, k, fs, foq)
    for f in range(2):
        sel = foq == f
        same_bits(exact(L2, base, q[sel], k, labels, (filt[f] != 0) & (deleted == 0)), {key: v[sel] for key, v in want.items()}, f"filter {f}")
    assert np.all(want["cnt"][foq == 1] < k)
    # the device entry, tiles in the order given (both filters in every tile), query 4 with a filter index >= nf
    dev = torch.device("cuda:0")
    st = torch.cuda.Stream(device=dev)
    bad = foq.copy()
    bad[4] = 2
    with torch.cuda.stream(st):
        dq = torch.from_numpy(q.copy()).to(dev)
        o = (torch.zeros((nq, k), dtype=torch.int64, device=dev), torch.zeros((nq, k), dtype=torch.float32, device=dev),
             torch.zeros(nq, dtype=torch.int32, device=dev))
        ix.exact_search_wide_dev(dq, k, *o, fs=fs, d_filter_of_query=torch.from_numpy(bad.astype(np.int32)).to(dev), stream=st.cuda_stream)
        with pytest.raises(hs.HsError) as e:
            ix.check(st.cuda_stream)
        assert e.value.status == hs.HS_ERR_INVALID
        got = dict(labels=o[0].cpu().numpy().view(np.uint64), dists=o[1].cpu().numpy(), cnt=o[2].cpu().numpy().view(np.uint32))
    st.synchronize()
    assert got["cnt"][4] == 0 and np.all(got["labels"][4] == NONE64) and np.all(np.isinf(got["dists"][4]))
    keep = np.arange(nq) != 4
    same_bits({key: v[keep] for key, v in want.items()}, {key: v[keep] for key, v in got.items()}, "device entry")


# ---- 4. reference (b): Gaussian rows against the oracle ------------------------------------------------------------------------------
@pytest.mark.parametrize("k,metric", ((100, L2), (1000, IP)))
def test_gaussian_rows_against_the_oracle(hs, k, metric):
    n, d, nq = 3001, 128, 9
    rng = np.random.default_rng(11)
    base, q = rng.standard_normal((n, d)).astype(np.float32), rng.standard_normal((nq, d)).astype(np.float32)
    oracle = Oracle()
    ix = ring(hs, metric, base)
    r = ix.exact_search_wide(q, k)
    assert np.all(r["cnt"] == k)
    assert np.array_equal(np.sort(r["labels"], axis=1), np.sort(oracle.brute_force(metric, base, q, k).astype(np.uint64), axis=1))
    pairs = oracle.dist(metric, np.repeat(q, k, axis=0), base[r["labels"].reshape(-1).astype(np.int64)])
    assert r["dists"].tobytes() == pairs.tobytes()
    same_bits({key: v[:, :64] if v.ndim == 2 else np.minimum(v, 64) for key, v in r.items()}, ix.exact_search(q, 64), "first 64")


# ---- 5. every narrow format: beside the fp32 rows and without them, the fp32 index's bytes ---------------------------------------------
@pytest.mark.parametrize("fmt_name,suffix", (("HS_ROWS_U8", "_u8"), ("HS_ROWS_I8", "_i8"), ("HS_ROWS_F16", "_f16"), ("HS_ROWS_BF16", "_bf16"),
                                             ("HS_ROWS_F8", "_f8")))
def test_narrow_rows_give_the_same_bits(hs, fmt_name, suffix):
    n, d, nq, k = 1500, 128, 9, 100
    base, q, labels = ints(n, d, 5, hi=8), ints(nq, d, 6, hi=8), perm_labels(n)   # integers below 8: every format holds them
    ix = ring(hs, L2, base, labels)
    want = ix.exact_search_wide(q, k)
    same_bits(exact(L2, base, q, k, labels), want, "fp32 rows")
    ix.set_row_format(getattr(hs, fmt_name))
    same_bits(want, ix.exact_search_wide(q, k), "both copies")
    assert ix.last_kernel() == "hs::exact_wide_kernel" + suffix
    ix.set_f32_resident(False)
    same_bits(want, ix.exact_search_wide(q, k), "fp32 dropped")
    assert ix.last_kernel() == "hs::exact_wide_kernel" + suffix


# ---- 6. the edges of the envelope --------------------------------------------------------------------------------------------------
def test_k_64_is_the_scan_and_k_0_and_1025_are_refused(hs):
    n, d = 200, 16
    base, q, labels = ints(n, d, 5), ints(3, d, 6), perm_labels(n)
    ix = ring(hs, L2, base, labels)
    same_bits(ix.exact_search(q, 64), ix.exact_search_wide(q, 64), "k = 64")
    assert ix.last_kernel() == "hs::exact_scan_kernel"
    for k in (0, 1025):
        with pytest.raises(hs.HsError) as e:
            ix.exact_search_wide(q, k)
        assert e.value.status == hs.HS_ERR_UNSUPPORTED and "1 <= k <= 1024" in str(e.value)
