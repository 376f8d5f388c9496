"""Plain-Python reading of the batched addPoint of DESIGN.md 4m (a build from nothing) and 4n (continued from a saveIndex file),
shared by tests/test_batch_build_restated_cpu.py (the host twin against this reading) and tests/test_gpu_batch_build_restated.py
(the device against this reading).  It is written from the reference's HierarchicalNSW (hnswalg.h: the constructor :90-159,
CompareByFirst :176-182, searchBaseLayer :231-322, getNeighborsByHeuristic2 :481-523, mutuallyConnectNewElement :549-687,
saveIndex :748-779, loadIndex :781-862, addPoint :1248-1376) and the five points of 4m; it imports nothing from the product.

Integer-valued rows only.  Every distance is an exact integer -- L2 the sum of squared differences, IP 1 - <a, b> -- and the
caller asserts `exact_range(rows, metric) < EXACT`: every partial sum of either recipe is then below 2^24 in magnitude, fp32
holds each of them exactly, and no summation order can change a decision.

What decides among EQUAL keys is modelled, not approximated: the two heaps under CompareByFirst are libstdc++'s
std::push_heap / std::pop_heap (bits/stl_heap.h: __push_heap, __adjust_heap), written out in `Heap`; queue_closest compares whole
(-dist, id) pairs, a total order over distinct ids, so a sort serves there.  Lists are their fixed slots of maxM0 + 1 / maxM + 1
words, so the ids a shortened count leaves behind are where the reference's memory has them, and reach the file.
"""
import math
import struct

import numpy as np

L2, IP = 0, 1
NONE = 0xFFFFFFFF
GROW_DIV, BATCH_MAX = 16, 16384          # what grow_div = 0 / batch_max = 0 stand for ("Defaults")
EXACT = 1 << 24
HEADER = "<6QiI3QdQ"                     # saveIndex :752-765


def exact_range(rows, metric):
    """The largest magnitude any partial sum of a distance between two of the rows can reach: the largest L2 distance, or for IP
    1 + the largest sum of |a_i| |b_i| (partial sums of a dot product of mixed signs can exceed the whole)."""
    x = np.asarray(rows)
    assert np.array_equal(x, np.rint(x)), "integer-valued rows only"
    x = x.astype(np.int64)
    if metric == IP:
        return 1 + int((np.abs(x) @ np.abs(x).T).max())
    dot = x @ x.T
    sq = np.diag(dot)
    return int((sq[:, None] + sq[None, :] - 2 * dot).max())      # squares only grow a sum: the whole bounds every part


class Distances:
    """dist(a, b) for every pair of rows as exact Python ints; one table, a row of it turned into a list when first asked for."""

    def __init__(self, rows, metric):
        x = np.asarray(rows)
        assert np.array_equal(x, np.rint(x)), "integer-valued rows only"
        x = x.astype(np.int64)
        dot = x @ x.T
        if metric == L2:
            sq = np.diag(dot)
            self.table = sq[:, None] + sq[None, :] - 2 * dot      # the int64 sum of squared differences, expanded
        else:
            assert metric == IP
            self.table = 1 - dot
        self.lists = {}

    def row(self, i):
        r = self.lists.get(i)
        if r is None:
            r = self.lists[i] = self.table[i].tolist()
        return r


class Heap:
    """std::priority_queue<std::pair<dist_t, tableint>, std::vector<...>, CompareByFirst>: a max-heap on the key alone, kept by
    libstdc++'s heap functions.  `ties[0]` counts the comparisons of two equal keys -- the ones an id-aware or otherwise different
    heap could decide differently."""
    __slots__ = ("a", "ties")

    def __init__(self, ties):
        self.a = []
        self.ties = ties

    def _push(self, hole, top, value):
        """__push_heap(first, holeIndex, topIndex, value, comp): the hole moves up while comp(parent, value), i.e. parent.first <
        value.first; an equal parent stops it."""
        a, key = self.a, value[0]
        while hole > top:
            parent = (hole - 1) // 2
            pk = a[parent][0]
            if pk == key:
                self.ties[0] += 1
            if not pk < key:
                break
            a[hole] = a[parent]
            hole = parent
        a[hole] = value

    def emplace(self, key, ident):
        """c.emplace_back(...); std::push_heap(c.begin(), c.end(), comp)"""
        self.a.append(None)
        self._push(len(self.a) - 1, 0, (key, ident))

    def pop(self):
        """std::pop_heap(c.begin(), c.end(), comp); c.pop_back().  __pop_heap moves the last element out, puts the first in its
        place, and __adjust_heap(first, 0, len - 1, value) walks the hole down along the larger child -- comp(right, left) picks
        the left one only when right.first < left.first, so equal children send the hole RIGHT -- then pushes the value up."""
        a = self.a
        value = a.pop()
        n = len(a)
        if n == 0:
            return
        hole = child = 0
        while child < (n - 1) // 2:
            child = 2 * (child + 1)
            rk, lk = a[child][0], a[child - 1][0]
            if rk == lk:
                self.ties[0] += 1
            if rk < lk:
                child -= 1
            a[hole] = a[child]
            hole = child
        if n & 1 == 0 and child == (n - 2) // 2:
            child = 2 * (child + 1)
            a[hole] = a[child - 1]
            hole = child - 1
        self._push(hole, 0, value)

    def drain_ids(self):
        """while (size() > 0) { out.push_back(top().second); pop(); }"""
        out = []
        while self.a:
            out.append(self.a[0][1])
            self.pop()
        return out


class Graph:
    """The members of HierarchicalNSW that saveIndex writes.  l0[i]: the level-0 slot of node i, maxM0 + 1 words, word 0 the
    count (a u16 count and two zero bytes: there are no delete marks); upper[i][l - 1]: its slot at level l, maxM + 1 words."""

    def __init__(self, M, ef_construction, mult, max_elements):
        self.M = self.maxM = M                                   # :97-109
        self.maxM0 = 2 * M
        self.efc = max(ef_construction, M)                       # :110
        self.mult = mult
        self.max_elements = max_elements
        self.l0, self.upper, self.labels = [], [], []
        self.ep, self.maxlevel = NONE, -1                        # :134-135

    def slot(self, i, level):
        return self.upper[i][level - 1] if level else self.l0[i]      # get_linklist0 / get_linklist :525-541

    def begin(self, level, label):
        """addPoint :1279-1312: the next internal id, its slots zeroed."""
        self.l0.append([0] * (self.maxM0 + 1))
        self.upper.append([[0] * (self.maxM + 1) for _ in range(level)])
        self.labels.append(int(label))


def search_base_layer(g, d, ep, layer, ties):
    """searchBaseLayer :231-322 for the query whose distances to every row are the list d; nothing is marked deleted."""
    top, cand = Heap(ties), Heap(ties)
    dist = d[ep]
    top.emplace(dist, ep)
    lower = dist
    cand.emplace(-dist, ep)
    visited = {ep}
    efc = g.efc
    while cand.a:
        ck, cur = cand.a[0]
        if -ck > lower and len(top.a) == efc:      # :260-263
            break
        cand.pop()
        slot = g.slot(cur, layer)
        for j in range(1, 1 + slot[0]):
            e = slot[j]
            if e in visited:
                continue
            visited.add(e)
            d1 = d[e]
            if len(top.a) < efc or lower > d1:     # :301
                cand.emplace(-d1, e)
                top.emplace(d1, e)
                if len(top.a) > efc:
                    top.pop()
                lower = top.a[0][0]
    return top


def heuristic(heap, M, D):
    """getNeighborsByHeuristic2 :481-523.  Below M entries the heap is returned untouched (:486-488).  Otherwise queue_closest
    -- std::priority_queue<std::pair<dist_t, tableint>> of (-dist, id), std::less on the PAIR -- hands them out nearest first,
    the larger id first among equal distances; a candidate is kept unless a kept one is strictly closer to it than the query is
    (:506-514); the kept ones are emplaced into the emptied heap in the order kept (:520-522)."""
    if len(heap.a) < M:
        return
    closest = sorted(heap.a, key=lambda t: (t[0], -t[1]))
    heap.a = []
    kept = []
    for dq, c in closest:
        if len(kept) >= M:
            break
        dc = D.row(c)
        for _, s in kept:
            if dc[s] < dq:
                break
        else:
            kept.append((dq, c))
    for dq, c in kept:
        heap.emplace(dq, c)


def phase_a(g, D, p, lp, ep, top, ties):
    """Point 3 of 4m, addPoint :1314-1352 and the head of mutuallyConnectNewElement :555-568 for row p of level lp, from the
    batch's entry point and top level: {level: selectedNeighbors}.  It reads g and writes nothing."""
    d = D.row(p)
    cur = ep
    if lp < top:
        curdist = d[cur]                             # :1316
        for level in range(top, lp, -1):
            changed = True
            while changed:
                changed = False
                slot = g.slot(cur, level)            # the list of currObj as the while body finds it (:1324)
                for j in range(1, 1 + slot[0]):
                    c = slot[j]
                    if d[c] < curdist:
                        curdist, cur, changed = d[c], c, True
    sels = {}
    for level in range(min(lp, top), -1, -1):        # :1345
        heap = search_base_layer(g, d, cur, level, ties)
        heuristic(heap, g.M, D)                      # :556
        sels[level] = heap.drain_ids()               # :563-566
        cur = sels[level][-1]                        # :568
    return sels


def phase_b(g, D, p, sels, ties, incoming, stats):
    """Point 4 of 4m, the rest of mutuallyConnectNewElement (:588-684) for row p on each of its levels."""
    for level, sel in sels.items():
        mcur = g.maxM if level else g.maxM0          # :555
        own = g.slot(p, level)
        assert own[0] == 0
        own[0] = len(sel)
        own[1:1 + len(sel)] = sel
        for nb in sel:
            other = g.slot(nb, level)
            incoming[(nb, level)] = incoming.get((nb, level), 0) + 1
            sz = other[0]
            if sz < mcur:                            # :637-639
                other[1 + sz] = p
                other[0] = sz + 1
                continue
            dn = D.row(nb)
            cands = Heap(ties)
            cands.emplace(dn[p], p)                  # :650
            for j in range(1, 1 + sz):
                cands.emplace(dn[other[j]], other[j])
            heuristic(cands, mcur, D)                # :660
            ids = cands.drain_ids()                  # :662-667; the words behind ids stay as they were
            other[1:1 + len(ids)] = ids
            other[0] = len(ids)                      # :669
            if len(ids) < sz:
                stats["stale_words"] += sz - len(ids)


def schedule(levels, n0=0, ep=NONE, top=-1, grow_div=0, batch_max=0):
    """Point 2 of 4m (n0 = 0) and of 4n (from a loaded graph): [(first row id, size, entry point, top level before the batch)].
    levels: those of the rows n0, n0 + 1, ..."""
    div, cap = grow_div or GROW_DIV, batch_max or BATCH_MAX
    n = n0 + len(levels)
    out, done = [], n0
    while done < n:
        size = min(cap, max(1, done // div), n - done)
        for i in range(size):
            if levels[done - n0 + i] > top:
                size = i + 1
                break
        out.append((done, size, ep, top))
        last = done + size - 1
        if levels[last - n0] > top:                  # addPoint :1364-1374
            ep, top = last, levels[last - n0]
        done += size
    return out


def insert_batch(g, D, begin, size, levels, labels, ep, top, ties, stats):
    """One batch: every search of phase A sees the graph as it stood when the batch began, then phase B in ascending row id."""
    for i in range(size):
        g.begin(levels[i], labels[i])
    sels = []
    for i in range(size):
        sels.append(phase_a(g, D, begin + i, levels[i], ep, top, ties) if ep != NONE else {})
    incoming = {}
    for i in range(size):
        phase_b(g, D, begin + i, sels[i], ties, incoming, stats)
    if incoming:
        stats["max_incoming"] = max(stats["max_incoming"], max(incoming.values()))


def run(g, D, n0, levels, labels, grow_div, batch_max):
    ties = [0]
    stats = dict(stale_words=0, max_incoming=0)
    sched = schedule(levels, n0, g.ep, g.maxlevel, grow_div, batch_max)
    for begin, size, ep, top in sched:
        lo = begin - n0
        insert_batch(g, D, begin, size, levels[lo:lo + size], labels[lo:lo + size], ep, top, ties, stats)
        last = lo + size - 1
        if levels[last] > top:
            g.ep, g.maxlevel = begin + size - 1, levels[last]
    stats.update(ties=ties[0], batches=len(sched))
    return stats


def save(g, rows):
    """saveIndex :748-779"""
    rows = np.ascontiguousarray(rows, np.float32)
    n, dim = rows.shape
    assert n == len(g.l0)
    links0 = 4 * g.maxM0 + 4                          # size_links_level0_ :116
    spe = links0 + 4 * dim + 8                        # :117-118
    hdr = struct.pack(HEADER, 0, g.max_elements, n, spe, links0 + 4 * dim, links0, g.maxlevel, g.ep, g.maxM, g.maxM0, g.M, g.mult, g.efc)
    el = np.zeros((n, spe), np.uint8)
    el[:, :links0] = np.array(g.l0, np.uint32).reshape(n, g.maxM0 + 1).view(np.uint8)
    el[:, links0:links0 + 4 * dim] = rows.view(np.uint8)
    el[:, links0 + 4 * dim:] = np.array(g.labels, np.uint64).reshape(n, 1).view(np.uint8)
    out = [hdr, el.tobytes()]
    for ups in g.upper:
        blob = np.array(ups, np.uint32).tobytes() if ups else b""
        out.append(struct.pack("<I", len(blob)) + blob)            # :771-776
    return b"".join(out)


def levels_of(raw):
    """element_levels_ as loadIndex recovers them (:864-875): linkListSize / size_links_per_element_ per node."""
    (_, _, count, spe, _, _, _, _, maxM) = struct.unpack_from("<6QiIQ", raw, 0)
    off = 96 + count * spe
    out = []
    for _ in range(count):
        (sz,) = struct.unpack_from("<I", raw, off)
        assert sz % (4 * maxM + 4) == 0
        out.append(sz // (4 * maxM + 4))
        off += 4 + sz
    assert off == len(raw)
    return out


def build(rows, levels, metric=L2, M=16, ef_construction=200, branching_factor=4, grow_div=0, batch_max=0, labels=None):
    """4m: the whole file of the batched build of `rows` with the given levels, and what the run met: batches, ties (comparisons
    of equal keys in the heaps), stale_words (ids left behind a shortened count), max_incoming (the most ids one (target, level)
    list received within one batch)."""
    n = len(rows)
    assert len(levels) == n
    g = Graph(M, ef_construction, 1 / math.log(float(branching_factor)), n)      # mult_ :149
    labels = list(range(n)) if labels is None else [int(x) for x in labels]
    stats = run(g, Distances(rows, metric), 0, [int(x) for x in levels], labels, grow_div, batch_max)
    return save(g, rows), stats


def load(raw, dim, max_elements):
    """loadIndex :781-875: the graph of a file, with its rows."""
    (off0, file_max, count, spe, label_off, data_off, maxlevel, ep, maxM, maxM0, M, mult, efc) = struct.unpack_from(HEADER, raw, 0)
    assert off0 == 0 and data_off == 4 * maxM0 + 4 and label_off == data_off + 4 * dim and spe == label_off + 8
    g = Graph(M, efc, mult, max_elements if max_elements >= count else file_max)      # :798-801
    assert (g.maxM, g.maxM0, g.efc) == (maxM, maxM0, efc)
    g.ep, g.maxlevel = ep, maxlevel
    el = np.frombuffer(raw, np.uint8, count * spe, 96).reshape(count, spe)
    g.l0 = el[:, :data_off].copy().view(np.uint32).tolist()
    rows = el[:, data_off:label_off].copy().view(np.float32)
    g.labels = el[:, label_off:].copy().view(np.uint64)[:, 0].tolist()
    off = 96 + count * spe
    for _ in range(count):
        (sz,) = struct.unpack_from("<I", raw, off)
        g.upper.append(np.frombuffer(raw, np.uint32, sz // 4, off + 4).reshape(-1, maxM + 1).tolist())
        off += 4 + sz
    assert off == len(raw)
    return g, rows


def resume(raw, dim, rows, levels, labels, metric=L2, max_elements=0, grow_div=0, batch_max=0):
    """4n: the file `raw` loaded with room for max_elements, `rows` added in the batched order with the given levels and labels,
    saved.  M, ef_construction and mult are the header's."""
    g, old = load(raw, dim, max_elements)
    allrows = np.ascontiguousarray(np.concatenate([old, np.asarray(rows, np.float32)]))
    assert len(allrows) <= g.max_elements and len(levels) == len(rows) == len(labels)
    stats = run(g, Distances(allrows, metric), len(old), [int(x) for x in levels], [int(x) for x in labels], grow_div, batch_max)
    return save(g, allrows), stats
