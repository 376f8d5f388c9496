"""The flat kernel's rank-free sorted insert (csrc/sorted_insert.hpp, used by csrc/flat_search.hip) where equal keys are the rule:
integer rows from a narrow value range, every third row stored twice, so that almost every insertion meets entries of its own
key, entries leave the result set at exactly the bound, and the k-th boundary is tied.  Against the oracle (hsutil.Oracle: the
CPU restatement of hnswalg_slim.h:321-457), for every query, by equality: the label set, the (distance bits, label) pairs of the
priority-queue overload, the sorted fp32 distance bits of the id overload, and the three traversal counters.

ef covers every slot count S of the kernel with and without spare ranks behind rank ef - 1 (the exact-fit sets ef == 64 S take the
branch that looks at the evicted entry before the insertion): 64 (S = 1, exact), 70 (S = 2), 128 (S = 2, exact), 192 (S = 3,
exact), 256 (S = 4, exact), 384 (S = 6, exact), 512 (S = 8, exact), and 100 / 160 / 200 / 300 / 500 for the spare-rank body of
S = 2, 3, 4, 6, 8; ef == k (where a tie at the bound decides the answer); L2 and inner product; the three row formats at d = 128."""
import numpy as np
import pytest

from hsutil import Oracle, load_product, mixture
from test_gpu_parity import _pq_sorted

pytestmark = pytest.mark.gpu
L2, IP = 0, 1
D, N, NQ = 128, 6000, 96
EFS = (64, 70, 128, 192, 256, 384, 512, 100, 160, 200, 300, 500)


def _tied_rows(n, seed):
    x = mixture(n, D, seed, n_clusters=8, lo=0, hi=5, sigma=1.2, integer=True)
    x[1::3] = x[0::3][:len(x[1::3])]   # duplicated rows: distance ties between different ids, whatever the query
    return np.ascontiguousarray(x, np.float32)


@pytest.fixture(scope="module", params=[L2, IP], ids=["l2", "ip"])
def tied(request, tmp_path_factory):
    P, O = load_product(), Oracle()
    metric = request.param
    tmp = tmp_path_factory.mktemp(f"ties{metric}")
    base, q = _tied_rows(N, 11), _tied_rows(NQ, 12)
    q[::4] = base[5:5 + len(q[::4])]   # queries that ARE rows: distance 0 twice (the row and its duplicate)
    hp, sp = str(tmp / "h.bin"), str(tmp / "s.bin")
    P.build_hnsw(base, hp, metric=metric, M=16, ef_construction=100, threads=8)
    P.convert_slim(hp, sp, D, metric=metric, threads=8)
    return P, P.Index(sp, P.HS_KIND_SLIM, D, metric=metric), O.load(sp, "slim", metric, D), q, metric


def _check(P, ix, ox, q, ef, k, kernel, cfg):
    ix.set_ef(ef); ox.set_ef(ef)
    oi, op = ox.search_ids(q, k, threads=8), ox.search_pq(q, k, threads=8)
    g = ix.search_pq(q, k, want_stats=True)
    assert ix.last_kernel() == kernel, cfg
    assert np.array_equal(g["cnt"], op["cnt"]), cfg
    got, want = _pq_sorted(g["dists"], g["labels"], g["cnt"]), _pq_sorted(op["dists"], op["labels"], op["cnt"])
    bad = [i for i in range(len(q)) if got[i] != want[i]]
    assert not bad, f"{cfg}: (distance bits, label) pairs differ for queries {bad[:8]} ({len(bad)} of {len(q)})"
    r = ix.search_ids(q, k, want_dists=True, want_stats=True)
    assert ix.last_kernel() == kernel, cfg
    bad = np.flatnonzero((np.sort(r["labels"], axis=1) != np.sort(oi["labels"], axis=1)).any(axis=1))
    assert bad.size == 0, f"{cfg}: label sets differ for queries {bad[:8].tolist()} ({bad.size} of {len(q)})"
    assert np.array_equal(np.sort(r["dists"], axis=1).view(np.uint32), np.sort(op["dists"], axis=1).view(np.uint32)), f"{cfg}: distance bits differ"
    bad = np.flatnonzero((r["stats"][:, :3] != oi["counters"][:, :3]).any(axis=1))
    assert bad.size == 0, f"{cfg}: traversal counters differ for queries {bad[:8].tolist()} ({bad.size} of {len(q)})"
    return r


@pytest.mark.parametrize("ef", EFS)
def test_tied_keys_every_slot_count_and_both_bodies(tied, ef):
    P, ix, ox, q, metric = tied
    ix.set_row_format(P.HS_ROWS_F32)
    _check(P, ix, ox, q, ef, 10, "hs::flat_kernel", f"metric={metric} ef={ef} k=10")


@pytest.mark.parametrize("ef", [64, 33, 10])
def test_tied_keys_ef_equal_k(tied, ef):
    """ef == k: an entry evicted at a key equal to the last kept key decides the answer (btie -> the log is replayed)."""
    P, ix, ox, q, metric = tied
    ix.set_row_format(P.HS_ROWS_F32)
    _check(P, ix, ox, q, ef, ef, "hs::flat_kernel", f"metric={metric} ef=k={ef}")


@pytest.mark.parametrize("fmt,kernel", [("HS_ROWS_F32", "hs::flat_kernel"), ("HS_ROWS_U8", "hs::flat_kernel_u8"), ("HS_ROWS_F16", "hs::flat_kernel_f16")])
def test_tied_keys_every_row_format(tied, fmt, kernel):
    P, ix, ox, q, metric = tied
    ix.set_row_format(getattr(P, fmt))
    try:
        for ef, k in ((70, 10), (128, 10), (64, 64)):
            _check(P, ix, ox, q, ef, k, kernel, f"metric={metric} fmt={fmt} ef={ef} k={k}")
    finally:
        ix.set_row_format(P.HS_ROWS_F32)
