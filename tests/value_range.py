"""Value families at the edges of the fp32 range (tests/test_gpu_value_range.py and its CPU twin tests/test_value_range_cpu.py).

Every family is one base draw -- hsutil.mixture(n, d, seed, n_clusters=12, lo=-1, hi=1, sigma=0.4), |x| < 4 -- multiplied by
np.float32(2.0 ** s).  The multiply is exact (no element leaves the normal range: |x| 2^s stays between 2^-126 and 2^128 for every
s used here, zeros stay zeros), so all families share the base draw's mantissas and only the exponent range of the distances moves:

  ip_cross      IP   x 2^c (IP_CROSS_EXP, per dim)   1 - <q, x> changes sign inside one query's result set
  l2_subnormal  L2   x 2^-70                          every nonzero distance is a subnormal float
  large         L2, IP   x 2^50                       distances above 2^100, all finite
  ip_ones       IP   x 2^-70                          <q, x> is below half an ulp of 1: every distance is exactly 1.0f
  l2_overflow   L2   x 2^62, d = 16                   squared differences overflow: +inf distances (exhaustive scans only)

The premises are asserted on the ORACLE's answers before a kernel's answer is looked at; a premise that fails is a failure of the
test.  Pure numpy: the oracle's answers come in as the dicts OracleIndex.search_pq / search_ids return."""
import numpy as np

from hsutil import mixture

L2, IP = 0, 1
N, NQ = 2000, 64
DIMS = (128, 20, 23)          # SIMD16 (the flat and fast kernels' compiled shape), SIMD4 on the any-dim path, SIMD16 + scalar rest
M, EF_CONSTRUCTION = 12, 80
SUBNORMAL = np.float32(2.0 ** -126)

# ip_cross: the power of two per dim that puts 1 - <q, x> on both sides of zero inside the result sets.  Found on the CPU with the
# host builder and the oracle (build_hnsw + convert_slim, search_ids at ef = 200, k = 64): for every c in -6 .. 2, the number of
# queries whose raw result array holds both signs.  At every dim exactly one exponent has any (63, 45 and 31 of 64 queries at the
# first seeds tried; none at the other eight exponents).  Why one: the draw's twelve clusters put <q, x> of a query and a row of
# its own cluster at about |centre|^2 = d / 3 (43 at d = 128, 7 at d = 20) and that of a row of another cluster at about 0 +- 5, and
# ef = 200 reaches past the ~167 rows of the own cluster; <q, x> 4^c is then about 2.7 / 1.7 / 1.9 inside the cluster and below 1
# outside it (the median over all pairs is 0.26 / 0.39 / 0.44).
# The k = 64 results of a query are rows of its own cluster alone, whose <q, x> lie in a band narrower than the factor 4 between two
# exponents: at d = 128 (43 +- 4 against 16 and 64) no seed and no power of two makes them cross zero, at d = 23 one query seed of
# thirty did, at d = 20 (7 +- 1.6 against 4) one seed in three does.  So that premise is asserted where the draw can meet it, at
# d = 20, which makes it hold for the family; the result ARRAYS cross zero at every dim, and it is the array that the key order of a
# kernel decides.
IP_CROSS_EXP = {128: -2, 20: -1, 23: -1}
IP_CROSS_K64_DIM = 20

# (ef, k) of the bare legs: the flat kernel's (k <= 64, ef <= 512), the fast kernel's (k = 100), the strict kernel's (ef = 600)
FLAT_PAIRS = ((10, 10), (70, 10), (200, 64), (512, 10))
FAST_PAIRS = ((100, 100), (300, 100))
STRICT_PAIRS = ((600, 10),)
NOT_BARE_PAIRS = ((100, 10), (300, 10))      # filter and delete marks
LEAN_PAIRS = ((70, 10), (200, 10))

# (metric, exponent of the scale); ip_cross takes its exponent from IP_CROSS_EXP
FAMILIES = {
    "ip_cross": ((IP, None),),
    "l2_subnormal": ((L2, -70),),
    "large": ((L2, 50), (IP, 50)),
    "ip_ones": ((IP, -70),),
}
OVERFLOW_EXP, OVERFLOW_DIM = 62, 16
OVERFLOW_N, OVERFLOW_K = 130, 64    # 130 rows: three row chunks of the scans (twelve runs to merge), the last one partly filled;
                                     # per query 25 .. 130 of the distances are finite, so k = 64 has queries on both sides
SEEDS = (31, 96)              # rows, queries (plus the dim); chosen on the CPU so that the oracle alone meets every premise


def scale(s):
    return np.float32(2.0 ** s)


def base_draw(n, d, seed):
    x = mixture(n, d, seed, n_clusters=12, lo=-1, hi=1, sigma=0.4)
    assert np.abs(x).max() < 4
    return x


def scaled(x, s):
    """x 2^s, exactly: dividing the scale out again gives x back bit for bit."""
    y = np.ascontiguousarray(x * scale(s), np.float32)
    assert np.array_equal((y / scale(s)).view(np.uint32), x.view(np.uint32)), f"the multiply by 2^{s} is not exact"
    return y


def cases():
    """(family, metric, dim, s) of every graph-kernel case."""
    out = []
    for family, legs in FAMILIES.items():
        for metric, s in legs:
            for d in DIMS:
                out.append((family, metric, d, IP_CROSS_EXP[d] if s is None else s))
    return out


def case_name(case):
    family, metric, d, s = case
    return f"{family}-{'l2' if metric == L2 else 'ip'}-d{d}"


def rows_and_queries(case, n=N, nq=NQ):
    _, _, d, s = case
    return scaled(base_draw(n, d, SEEDS[0] + d), s), scaled(base_draw(nq, d, SEEDS[1] + d), s)


def overflow_rows_and_queries(n=OVERFLOW_N, nq=NQ):
    d = OVERFLOW_DIM
    return scaled(base_draw(n, d, SEEDS[0] + d), OVERFLOW_EXP), scaled(base_draw(nq, d, SEEDS[1] + d), OVERFLOW_EXP)


def allowed_half(labels):
    """The filter of the not-bare legs: half the labels, scattered (uint8 per label)."""
    return ((labels * 7 + 3) % 10 < 5).astype(np.uint8)


def marked_tenth(labels):
    """The labels the delete-marks leg marks."""
    return labels[labels % 10 == 3]


def result_dists(o):
    """Per query, every distance the oracle's answer holds: the raw result array (raw_sz entries of raw_d)."""
    return [o["raw_d"][i, :n] for i, n in enumerate(o["raw_sz"])]


def check_premise(family, o, k, what):
    """The family's premise on one oracle answer (search_pq or search_ids, ef = len of the raw array's row, k asked)."""
    rows = result_dists(o)
    assert all(len(r) >= k for r in rows), f"{what}: a query has fewer than k results"
    alld = np.concatenate(rows)
    assert np.all(np.isfinite(alld)), f"{what}: a non-finite distance"
    if family == "l2_subnormal":
        assert np.all(alld >= 0) and np.all(alld[alld != 0] < SUBNORMAL), f"{what}: a nonzero distance is a normal float"
        assert (alld != 0).any(), f"{what}: every distance is zero"
        if k == 10:
            assert min(len(np.unique(np.sort(r)[:k])) for r in rows) >= 8, f"{what}: a query with fewer than 8 distinct result distances"
    elif family == "large":
        assert min(np.abs(r).max() for r in rows) > np.float32(2.0 ** 100), f"{what}: a query whose results stay below 2^100"
    elif family == "ip_ones":
        assert np.all(alld.view(np.uint32) == np.float32(1.0).view(np.uint32)), f"{what}: a distance that is not exactly 1.0f"


def crossing(o, k=None):
    """Queries whose result distances hold both a negative and a positive value: over the raw array, or over the k smallest."""
    out = []
    for r in result_dists(o):
        r = np.sort(r)[:k] if k else r
        out.append(bool((r < 0).any() and (r > 0).any()))
    return np.array(out)


def check_ip_cross(o_ids_ef200_k64, dim, what):
    """ip_cross on the oracle's search_ids answer at ef = 200, k = 64."""
    o = o_ids_ef200_k64
    assert o["raw_d"].shape[1] == 200 and o["labels"].shape[1] == 64
    assert 2 * crossing(o).sum() >= len(o["raw_sz"]), f"{what}: fewer than half of the queries have both signs in their result array"
    if dim == IP_CROSS_K64_DIM:
        assert crossing(o, 64).any(), f"{what}: no query's 64 results cross zero"


def kth_ties(o, k):
    """Queries whose k-th and (k+1)-th result distances are equal."""
    return np.array([len(r) > k and np.sort(r)[k - 1] == np.sort(r)[k] for r in result_dists(o)])


def reference(ox, family, dim, q, ef, k, ids, what):
    """The oracle's answer of one leg, the family's premise checked on it.  ids: also the (q, k, tableint*) overload (Slim files).
    "replay": whether a kernel that selects must report a tie re-run (stats column 3 == 1) on some query of this leg -- on ip_ones
    every key is equal, so with ef > k every query ties across the k-th boundary (asserted); with ef == k nothing is selected and a
    full heap admits no equal key, so there is a re-run only if the oracle counts an eviction of a key equal to the last one kept."""
    ox.set_ef(ef)
    ref = dict(pq=ox.search_pq(q, k, threads=8), ids=ox.search_ids(q, k, threads=8) if ids else None)
    replay = family == "ip_ones"
    for name, o in ref.items():
        if o is None:
            continue
        check_premise(family, o, k, f"{what} {name}")
        if family == "ip_ones" and ef > k:
            assert kth_ties(o, k).all(), f"{what} {name}: a query without a tie across the k-th boundary"
        if family == "ip_ones" and ef == k:
            replay = replay and bool((ox.tie_evictions(q, k, name == "pq", threads=8) > 0).any())
    assert np.all(ref["pq"]["cnt"] == k), f"{what}: a query has fewer than k results"
    if family == "ip_cross" and ids and (ef, k) == (200, 64):
        check_ip_cross(ref["ids"], dim, what)
    ref["replay"] = replay
    return ref


def build_files(hs, case, folder, threads=8):
    """The vanilla file and its convert_slim file over a case's rows (the host builder and the host convert).  The build is the
    serial one, so the graph -- and with it whether the oracle meets the premises -- is the same on every machine."""
    import os
    _, metric, d, _ = case
    base, q = rows_and_queries(case)
    hp, sp = (os.path.join(folder, f"{case_name(case)}.{x}") for x in ("h.bin", "s.bin"))
    hs.build_hnsw(base, hp, metric=metric, M=M, ef_construction=EF_CONSTRUCTION, threads=1)
    hs.convert_slim(hp, sp, d, metric=metric, threads=threads)
    return dict(name=case_name(case), family=case[0], metric=metric, dim=d, n=len(base), hp=hp, sp=sp, base=base, q=q)


def check_overflow(table, k, what):
    """l2_overflow on the oracle's full (query, row) distance table."""
    assert not np.isnan(table).any(), f"{what}: NaN"
    inf = np.isposinf(table)
    assert inf.any(), f"{what}: no +inf distance"
    finite = (~inf).sum(1)
    assert (finite < k).any(), f"{what}: every query has k finite distances"
    assert (finite >= k).any(), f"{what}: no query has k finite distances"


def dist_table(oracle, metric, base, q):
    """Oracle.dist over every (query, row) pair: nq x n."""
    n = base.shape[0]
    return np.stack([oracle.dist(metric, np.repeat(q[i:i + 1], n, axis=0), base) for i in range(q.shape[0])])
