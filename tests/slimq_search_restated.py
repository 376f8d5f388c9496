"""searchKnn(q, k, result) of HNSW-SlimQ in plain Python, read from the reference's source (third_party/hnswlib/hnswalg_slimq.h and
the rabitqlib headers it calls), over the fields parse_slimq gives.  An independent statement: neither oracle/hs_oracle_slimq.hpp nor
csrc/slimq_search.hip was consulted for the control flow, only for the encoding of what is returned (so the two can be compared).

Taken as given, because they are pinned elsewhere: the prepared query (OracleSlimQ.prepare: delta, vl, k1xsumq, g_add per cluster, the
four bit planes -- pinned against the compiled rabitqlib by tests/golden/rabitq_ref.npz) and the exact distance (Oracle.dist -- pinned
against the compiled hnswlib space).  Stated here: the estimate, the descent, the SearchBuffer, the visited array, the re-rank and
the heap array that libstdc++'s push_heap / pop_heap leave.

Source lines (hnswalg_slimq.h unless another file is named):
  estimate       :408-440 get_bin_est -> rabitqlib/index/estimator.hpp:164-188 split_single_estdist
                 -> rabitqlib/utils/warmup_space.hpp:93-101 (the scalar loop; the AVX-512 one sums the same integers)
  SearchBuffer   :80-151
  descent        :1850-1901
  level 0        :688-759 searchBaseLayerST<true>, entered from :1914-1918
  heap           bits/stl_heap.h __push_heap / __adjust_heap / __pop_heap, comparator :322-328 (a.first < b.first)

:1917 hands searchBaseLayerST the program's global K (include/core.h:30) where its own argument k stands; the reference's callers set
both to the same number, and so does this reading ("global K").

`wrong` names one deliberately wrong reading; tests use it to show that a case can tell the readings apart."""
import numpy as np

WRONG = ("descent_last_min", "is_full_once", "pool_refuses_held_id", "rerank_empty_node", "equal_key_behind")
CHECKED = 1 << 31


def popcount_rows(x):
    """x: (n, w) uint64 -> (n,) int64, the set bits of each row"""
    return np.unpackbits(np.ascontiguousarray(x).view(np.uint8), axis=1).sum(axis=1, dtype=np.int64)


def estimates(p, q3, g_add, planes):
    """est_dist of every node for one prepared query, float32 (n,).  warmup_space.hpp:93-101: ppc += popcount(x),
    ip += popcount(x & query[i * 4 + j]) << j over the blocks; return delta * float(ip) + vl * float(ppc).  estimator.hpp:185:
    est_dist = f_add + g_add + f_rescale * (ip_x0_qr + k1xsumq), left to right, every operation rounded to float32 (the oracle and
    the kernels build without contraction).  g_add is the per-cluster value get_bin_est passes: norm * norm (L2), -norm (IP)."""
    code = p["code"]
    n, nblk = code.shape
    planes = np.asarray(planes, np.uint64).reshape(nblk, 4)
    ip = np.zeros(n, np.int64)
    for j in range(4):
        ip += popcount_rows(code & planes[None, :, j]) << j
    pc = popcount_rows(code)
    f32 = np.float32
    delta, vl, k1 = f32(q3[0]), f32(q3[1]), f32(q3[2])
    a = delta * ip.astype(f32)
    b = vl * pc.astype(f32)
    ipq = a + b
    f_add, f_rescale = p["factors"][:, 0], p["factors"][:, 1]
    g = np.asarray(g_add, f32)[p["cluster"]]
    left = f_add + g
    inner = ipq + k1
    right = f_rescale * inner
    out = left + right
    assert out.dtype == np.float32
    return out


class SearchBuffer:
    """:80-151.  data_ holds capacity + 1 pairs; an id's bit 31 marks it checked."""

    def __init__(self, capacity, wrong=None):
        self.d = [(0.0, 0)] * (capacity + 1)
        self.size, self.cur, self.cap, self.wrong = 0, 0, capacity, wrong

    def binary_search(self, dist):   # :87-97
        d, lo, ln = self.d, 0, self.size
        if self.wrong == "equal_key_behind":
            while lo < self.size and d[lo][0] <= dist:
                lo += 1
            return lo
        while ln > 1:
            half = ln >> 1
            ln -= half
            lo += half if d[lo + half - 1][0] < dist else 0
        return lo + 1 if lo < self.size and d[lo][0] < dist else lo

    def insert(self, data_id, dist):   # :112-119
        lo = self.binary_search(dist)
        self.d[lo + 1:self.size + 1] = self.d[lo:self.size]   # memmove of size_ - lo pairs
        self.d[lo] = (dist, data_id)
        self.size += 1 if self.size < self.cap else 0
        self.cur = lo if lo < self.cur else self.cur

    def is_full(self, dist):   # :121-123
        return self.size == self.cap and dist > self.d[self.size - 1][0]

    def pop(self):   # :126-134
        dist, cur_id = self.d[self.cur]
        self.d[self.cur] = (dist, cur_id | CHECKED)
        self.cur += 1
        while self.cur < self.size and self.d[self.cur][1] & CHECKED:
            self.cur += 1
        return cur_id

    def has_next(self):   # :143
        return self.cur < self.size

    def holds(self, data_id):
        return any((self.d[i][1] & ~CHECKED) == data_id for i in range(self.size))


def _push_heap(h, hole, top, value):   # stl_heap.h __push_heap, comp = a.first < b.first
    parent = (hole - 1) // 2
    while hole > top and h[parent][0] < value[0]:
        h[hole] = h[parent]
        hole = parent
        parent = (hole - 1) // 2
    h[hole] = value


def push_heap(h):   # the new element is h[-1]
    _push_heap(h, len(h) - 1, 0, h[-1])


def pop_heap(h):
    """stl_heap.h __pop_heap + __adjust_heap over [first, last): the root goes to the last place, the rest is a heap again"""
    value = h[-1]
    h[-1] = h[0]
    ln = len(h) - 1
    hole = child = 0
    while child < (ln - 1) // 2:
        child = 2 * (child + 1)
        if h[child][0] < h[child - 1][0]:
            child -= 1
        h[hole] = h[child]
        hole = child
    if ln & 1 == 0 and child == (ln - 2) // 2:
        child = 2 * (child + 1)
        h[hole] = h[child - 1]
        hole = child - 1
    _push_heap(h, hole, 0, value)


def level_list(p, i, level):
    """The ids of `level` in node i's blob, or None where the node has no blob (get_neighbors() == nullptr).  parse_slimq cuts the
    blob at the u16 offsets exactly as :1873-1884 does (offset[level - 1] .. offset[level], the total for the node's own level)."""
    ls = p["lists"][i]
    if len(ls) == 0:
        return None
    return ls[level]


def search(p, ef, k, est, exact, enterpoint, maxlevel, threshold_level=0, wrong=None):
    """One query.  est: estimates() of this query; exact: float32 (n,) exact distances of the query to every row (:747-749 computes
    them on demand; which rows are asked for shows in what is returned).  ef is the capacity setEf gave the SearchBuffer (:346-349).
    Returns dict(ids, dists (float32), count, counters [expansions with a list, estimates, inserts, revisits], trace (uint32))
    -- ids / dists are the first min(k, count) places of the heap array, which :1921-1923 reads as the result."""
    assert wrong is None or wrong in WRONG
    n = p["n"]
    if n == 0:   # :1811
        return dict(ids=[], dists=np.zeros(0, np.float32), count=0, counters=[0, 0, 0, 0], trace=np.zeros(0, np.uint32))
    e = [float(x) for x in est]          # float32 values, exact as Python floats: comparisons are the float32 ones
    ebits = np.asarray(est, np.float32).view(np.uint32)
    n_hops = n_ins = n_rev = 0
    cur, curdist, n_est = enterpoint, e[enterpoint], 1   # :1850-1856
    for level in range(maxlevel, threshold_level, -1):   # :1862
        changed = True
        while changed:
            changed = False
            ids = level_list(p, cur, level)
            if ids is None or len(ids) == 0:   # :1869, :1879
                continue
            start = curdist
            for c in ids:   # :1889-1899
                c = int(c)
                n_est += 1
                d = e[c]
                if d < curdist or (wrong == "descent_last_min" and d == curdist and d < start):
                    curdist, cur, changed = d, c, True
    pool = SearchBuffer(ef, wrong)
    visited = bytearray(n)
    heap, trace = [], []
    pool.insert(cur, curdist)   # :1914
    while pool.has_next():   # :696
        node = pool.pop()
        trace += [node | (CHECKED if visited[node] else 0), pool.size]
        if visited[node]:   # :700
            n_rev += 1
            continue
        visited[node] = 1
        ids = level_list(p, node, 0)   # :712-713: the total for a level-0 node, offset[0] otherwise
        empty = ids is None or len(ids) == 0
        if empty and wrong != "rerank_empty_node":   # :708, :714
            continue
        if not empty:
            n_hops += 1
            full_at_start = pool.size == pool.cap
            last_at_start = pool.d[pool.size - 1][0]
            for c in ids:   # :728-746
                c = int(c)
                n_est += 1
                d = e[c]
                full = (full_at_start and d > last_at_start) if wrong == "is_full_once" else pool.is_full(d)
                if full or visited[c]:   # :741-744
                    continue
                if wrong == "pool_refuses_held_id" and pool.holds(c):
                    continue
                pool.insert(c, d)
                n_ins += 1
                trace += [c | (1 << 30), int(ebits[c])]
        heap.append((float(exact[node]), node))   # :747-757
        push_heap(heap)
        while len(heap) > k:
            pop_heap(heap)
            heap.pop()
    return dict(ids=[i for _, i in heap], dists=np.array([d for d, _ in heap], np.float32), count=len(heap),
                counters=[n_hops, n_est, n_ins, n_rev], trace=np.array(trace, np.uint32))
