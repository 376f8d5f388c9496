"""Plain-Python reading of the batched build of HNSW-SlimQ's base graph, shared by tests/test_rq_batch_build_cpu.py
(the host twin against this reading) and tests/test_gpu_rq_batch_build.py (the device against this reading).  It is written from
rabitqlib's HierarchicalNSW (third_party/rabitqlib/index/hnsw/hnsw.hpp: the heaps :33-36, the constructor :427-500, construct
:667-704, add_point :706-825, search_base_layer :827-905, mutually_connect_new_element :907-1014, get_neighbors_by_heuristic2
:1016-1054), the five points of DESIGN.md 4m and the file layout of hnswlib's saveIndex (hnswalg.h:748-779); it imports nothing
from the product.

Integer-valued rows only.  Every distance is an exact integer -- L2 the sum of squared differences, IP 1 - <a, b> -- and the
caller asserts `exact_range(rows, metric) < EXACT`: every partial sum of the recipe, in any order and fused or not, is then below
2^24 in magnitude, fp32 holds each of them exactly, and no summation order can change a decision.

Both heaps hold (distance, id) pairs under the pair's own order, which is total over distinct ids: no heap mechanics decide
anything, so the heaps are written as sorted lists.  Lists are their fixed slots of maxM0 + 1 / maxM + 1 words, so the ids a
shortened count leaves behind are where the reference's memory has them, and reach the file.

RULES names the rules a test may switch off, one at a time, to show that the comparison notices: the reading then follows
hnswlib's rule (or, for `batch`, the serial order) instead.
"""
import bisect
import math
import struct

import numpy as np

L2, IP = 0, 1
NONE = 0xFFFFFFFF
GROW_DIV, BATCH_MAX = 16, 16384          # what grow_div = 0 / batch_max = 0 stand for ("Defaults")
EXACT = 1 << 24
HEADER = "<6QiI3QdQ"                     # saveIndex :752-765
RULES = ("pair_top", "pair_cand", "cand_order", "pop_order", "present", "batch")


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
    return int((sq[:, None] + sq[None, :] - 2 * dot).max())


class Distances:
    """dist(a, b) for every pair of rows as exact Python ints; one table, a row of it turned into a list when first asked for."""

    def __init__(self, rows, metric):
        x = np.asarray(rows)
        assert np.array_equal(x, np.rint(x)), "integer-valued rows only"
        x = x.astype(np.int64)
        dot = x @ x.T
        if metric == L2:
            sq = np.diag(dot)
            self.table = sq[:, None] + sq[None, :] - 2 * dot
        else:
            assert metric == IP
            self.table = 1 - dot
        self.lists = {}

    def row(self, i):
        r = self.lists.get(i)
        if r is None:
            r = self.lists[i] = self.table[i].tolist()
        return r


class Graph:
    """The members saveIndex writes.  l0[i]: the level-0 slot of node i, maxM0 + 1 words, word 0 the count; upper[i][l - 1]: its
    slot at level l, maxM + 1 words."""

    def __init__(self, M, ef_construction, n):
        self.M = self.maxM = M                                   # hnsw.hpp:445-447
        self.maxM0 = 2 * M
        self.efc = max(ef_construction, M)                       # :448
        self.mult = 1 / math.log(1.0 * M)                        # :493
        self.max_elements = n
        self.l0, self.upper = [], []
        self.ep, self.maxlevel = NONE, -1

    def slot(self, i, level):
        return self.upper[i][level - 1] if level else self.l0[i]

    def begin(self, level):
        self.l0.append([0] * (self.maxM0 + 1))
        self.upper.append([[0] * (self.maxM + 1) for _ in range(level)])


def search_base_layer(g, d, ep, layer, off):
    """search_base_layer :827-905 for the row whose distances to every row are the list d.  top: the result max-heap as an ascending
    list of (d, id), its maximum last; cand: the candidate min-heap as an ascending list, its minimum first.  With a pair rule off,
    that heap orders by distance alone and lets the LATER arrival win among equals -- one of the orders a heap without ids may take."""
    seq = [0]

    def key(dist, ident, rule):
        if rule in off:
            seq[0] += 1
            return (dist, -seq[0], ident)
        return (dist, ident, ident)

    top = [key(d[ep], ep, "pair_top")]
    cand = [key(d[ep], ep, "pair_cand")]
    lower = d[ep]
    visited = {ep}
    efc = g.efc
    while cand:
        c = cand[0]
        if c[0] > lower and len(top) == efc:          # :855-857
            break
        cand.pop(0)
        slot = g.slot(c[2], layer)
        for j in range(1, 1 + slot[0]):               # adjacency order
            e = slot[j]
            if e in visited:
                continue
            visited.add(e)
            d1 = d[e]
            if len(top) < efc or lower > d1:          # :884, on the distance only
                bisect.insort(cand, key(d1, e, "pair_cand"))
                bisect.insort(top, key(d1, e, "pair_top"))
                if len(top) > efc:
                    top.pop()
                lower = top[-1][0]
    return [(t[0], t[2]) for t in top]


def heuristic(pairs, M, D, off):
    """get_neighbors_by_heuristic2 :1016-1054 on the set `pairs` of (d, id): nothing below M entries; otherwise the candidates go
    by ascending (d, id), one is kept unless a kept one is strictly closer to it than the node is, until M are kept.  Returns the
    set that is left."""
    if len(pairs) < M:
        return list(pairs)
    order = sorted(pairs, key=(lambda t: (t[0], -t[1])) if "cand_order" in off else None)
    kept = []
    for dq, c in order:
        if len(kept) >= M:
            break
        dc = D.row(c)
        for _, s in kept:
            if dc[s] < dq:
                break
        else:
            kept.append((dq, c))
    return kept


def pop_order(pairs, off):
    """What popping the max-heap of pairs yields: descending (d, id)."""
    if "pop_order" in off:
        return [c for _, c in sorted(pairs, key=lambda t: (-t[0], t[1]))]
    return [c for _, c in sorted(pairs, reverse=True)]


def phase_a(g, D, p, lp, ep, top, off):
    """add_point :733-800 and the head of mutually_connect_new_element :912-925 for row p of level lp from the batch's entry point
    and top level: {level: sel}.  It reads g and writes nothing."""
    d = D.row(p)
    cur = ep
    if lp < top:
        curdist = d[cur]
        for level in range(top, lp, -1):
            changed = True
            while changed:
                changed = False
                slot = g.slot(cur, level)
                for j in range(1, 1 + slot[0]):
                    c = slot[j]
                    if d[c] < curdist:
                        curdist, cur, changed = d[c], c, True
    sels = {}
    for level in range(min(lp, top), -1, -1):
        found = search_base_layer(g, d, cur, level, off)
        sels[level] = pop_order(heuristic(found, g.M, D, off), off)
        cur = sels[level][-1]
    return sels


def phase_b(g, D, p, sels, off, incoming, stats):
    """The writes of mutually_connect_new_element (:926-1011) for row p on each of its levels, top level first."""
    for level, sel in sels.items():
        mcur = g.maxM if level else g.maxM0
        own = g.slot(p, level)
        assert own[0] == 0
        own[0] = len(sel)
        own[1:1 + len(sel)] = sel
        for nb in sel:
            other = g.slot(nb, level)
            incoming[(nb, level)] = incoming.get((nb, level), 0) + 1
            sz = other[0]
            if "present" not in off and p in other[1:1 + sz]:      # :973-980
                stats["present_hits"] += 1
                continue
            if sz < mcur:
                other[1 + sz] = p
                other[0] = sz + 1
                continue
            dn = D.row(nb)
            cands = [(dn[p], p)] + [(dn[other[j]], other[j]) for j in range(1, 1 + sz)]
            ids = pop_order(heuristic(cands, mcur, D, off), off)
            other[1:1 + len(ids)] = ids                            # the words behind ids stay as they were
            other[0] = len(ids)
            if len(ids) < sz:
                stats["stale_words"] += sz - len(ids)
            stats["full_lists"] = max(stats["full_lists"], sz + 1)


def schedule(levels, grow_div=0, batch_max=0):
    """Point 2 of 4m: [(first row id, size, entry point, top level before the batch)]."""
    div, cap = grow_div or GROW_DIV, batch_max or BATCH_MAX
    n = len(levels)
    out, done, ep, top = [], 0, NONE, -1
    while done < n:
        size = min(cap, max(1, done // div), n - done)
        for i in range(size):
            if levels[done + i] > top:
                size = i + 1
                break
        out.append((done, size, ep, top))
        last = done + size - 1
        if levels[last] > top:
            ep, top = last, levels[last]
        done += size
    return out


def save(g, rows):
    """saveIndex (hnswalg.h:748-779); labels are the row index"""
    rows = np.ascontiguousarray(rows, np.float32)
    n, dim = rows.shape
    assert n == len(g.l0)
    links0 = 4 * g.maxM0 + 4
    spe = links0 + 4 * dim + 8
    hdr = struct.pack(HEADER, 0, g.max_elements, n, spe, links0 + 4 * dim, links0, g.maxlevel, g.ep, g.maxM, g.maxM0, g.M, g.mult, g.efc)
    el = np.zeros((n, spe), np.uint8)
    el[:, :links0] = np.array(g.l0, np.uint32).reshape(n, g.maxM0 + 1).view(np.uint8)
    el[:, links0:links0 + 4 * dim] = rows.view(np.uint8)
    el[:, links0 + 4 * dim:] = np.arange(n, dtype=np.uint64).reshape(n, 1).view(np.uint8)
    out = [hdr, el.tobytes()]
    for ups in g.upper:
        blob = np.array(ups, np.uint32).tobytes() if ups else b""
        out.append(struct.pack("<I", len(blob)) + blob)
    return b"".join(out)


def levels_of(raw):
    """The level of every node of a saveIndex file: its upper lists' bytes / (4 maxM + 4)."""
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


def edges_of(g):
    """The fixture's form of a graph (tests/golden/rabitq_hnsw_ref.npz): [maxlevel, enterpoint, per node: label, level, per level
    count + ids]."""
    out = [g.maxlevel, g.ep]
    for i in range(len(g.l0)):
        out += [i, len(g.upper[i])]
        for slot in [g.l0[i]] + g.upper[i]:
            out.append(slot[0])
            out += slot[1:1 + slot[0]]
    return np.array(out, np.uint32)


def build(rows, levels, metric=L2, M=32, ef_construction=128, grow_div=0, batch_max=0, off=(), want_graph=False):
    """4o: the whole file of the batched build of `rows` with the given levels, and what the run met: batches, stale_words (ids
    left behind a shortened count), max_incoming (the most ids one (target, level) list received within one batch), full_lists
    (the most candidates one reverse-link heuristic saw), present_hits.  off: rules of RULES to switch off."""
    assert all(r in RULES for r in off)
    n = len(rows)
    levels = [int(x) for x in levels]
    assert len(levels) == n
    g = Graph(M, ef_construction, n)
    D = Distances(rows, metric)
    stats = dict(stale_words=0, max_incoming=0, full_lists=0, present_hits=0)
    sched = schedule(levels, grow_div, batch_max)
    for begin, size, ep, top in sched:
        for i in range(size):
            g.begin(levels[begin + i])
        incoming = {}
        if "batch" in off:                                   # the serial order: every row sees the rows before it
            for i in range(size):
                if g.ep != NONE:
                    sels = phase_a(g, D, begin + i, levels[begin + i], ep, top, off)
                    phase_b(g, D, begin + i, sels, off, incoming, stats)
        else:
            sels = [phase_a(g, D, begin + i, levels[begin + i], ep, top, off) if ep != NONE else {} for i in range(size)]
            for i in range(size):
                phase_b(g, D, begin + i, sels[i], off, incoming, stats)
        if incoming:
            stats["max_incoming"] = max(stats["max_incoming"], max(incoming.values()))
        last = begin + size - 1
        if levels[last] > top:
            g.ep, g.maxlevel = last, levels[last]
    stats["batches"] = len(sched)
    raw = save(g, rows)
    return (raw, stats, g) if want_graph else (raw, stats)
