"""Plain-Python reading of the graph passes of convertFromHNSW, shared by tests/test_slimq_graph_cpu.py (HierarchicalNSWSlimQ,
hnswalg_slimq.h:1546-1762) and tests/test_slim_convert_restated_cpu.py (HierarchicalNSWSlim, hnswalg_slim.h:867-1108).  The two
classes run the same passes and differ in their PruneByHeuristic only.

Integer-valued L2 rows only: every distance is an exact int64, so no summation order can change a decision.  Python's sort is
stable; std::sort's order among equal keys is introsort's beyond 16 elements, which this reading does not model: the caller
asserts that no such list occurs (the `unstable` count).
"""
import numpy as np


def int_rows(n, d, seed, centre=600, spread=250, clusters=12):
    """Integer-valued rows: `clusters` integer centres in [-centre, centre) plus integer noise in [-spread, spread]."""
    rng = np.random.default_rng(seed)
    centres = rng.integers(-centre, centre, (clusters, d))
    return (centres[rng.integers(0, clusters, n)] + rng.integers(-spread, spread + 1, (n, d))).astype(np.float32)


def hub_top_n(level_cnt, pct):
    """static_cast<size_t>(level_cnts[l] * top_degree_percent + 0.5) (hnswalg_slim.h:926,937; hnswalg_slimq.h:1531,1542): size_t
    times float is a FLOAT product of float(level_cnts[l]) and alpha; only the + 0.5 is done in double."""
    return int(float(np.float32(level_cnt) * np.float32(pct)) + 0.5)


def hub_threshold(hist_row, top_n):
    """degree_threshold[l] (hnswalg_slim.h:927-944): buckets from maxM0 + 1 down to 1, first degree where the running count
    reaches topN; 0 when it never does."""
    acc = 0
    for deg in range(len(hist_row) - 1, 0, -1):
        acc += int(hist_row[deg])
        if acc >= top_n:
            return deg
    return 0


def degree_histogram(g):
    """(hist[level][degree], level_cnts) as the reference counts them: level_cnts[0] is never incremented (hnswalg_slim.h:908-922)."""
    n, maxlevel, maxM0, lists = g["count"], g["maxlevel"], g["maxM0"], g["lists"]
    hist = np.zeros((maxlevel + 1, maxM0 + 2), np.int64)
    level_cnts = np.zeros(maxlevel + 1, np.int64)
    for i in range(n):
        for l in range(1, len(lists[i])):
            level_cnts[l] += 1
            hist[l][len(lists[i][l])] += 1
        hist[0][len(lists[i][0])] += 1
    return hist, level_cnts


def convert_graph_restated(g, rows, thr_level, pct0, pct, top_M0, low_m0, top_M, low_m, prune):
    """Per-node, per-level neighbour lists of the converted graph, and the number of by-distance sorts over more than 16 ids with
    equal keys.  prune="slim": HierarchicalNSWSlim::PruneByHeuristic (hnswalg_slim.h:836-865), a candidate is dropped when a
    neighbour kept so far is strictly closer to it; prune="slimq": HierarchicalNSWSlimQ's (hnswalg_slimq.h:1334-1362), which
    measures against the node whose internal id is the LOOP INDEX, and only once something has been kept."""
    assert prune in ("slim", "slimq")
    n, maxlevel, maxM, maxM0 = g["count"], g["maxlevel"], g["maxM"], g["maxM0"]
    lists = g["lists"]
    r64 = rows.astype(np.int64)

    def dist(a, b):
        x = r64[a] - r64[b]
        return int((x * x).sum())
    hist, level_cnts = degree_histogram(g)
    thr = [hub_threshold(hist[l], hub_top_n(level_cnts[l], pct0 if l == 0 else pct)) for l in range(maxlevel + 1)]
    unstable = 0

    def prune_list(v_sorted, lim):
        out = []
        for i, (dd, nb) in enumerate(v_sorted):
            if len(out) >= lim:
                break
            if prune == "slim":
                good = all(dist(kept, nb) >= dd for kept in out)
            else:
                good = not (out and dist(i, nb) < dd)
            if good:
                out.append(nb)
        return out

    def by_dist(v, ids):
        nonlocal unstable
        pairs = sorted(((dist(v, int(u)), k, int(u)) for k, u in enumerate(ids)), key=lambda t: (t[0], t[1]))   # stable
        if len(pairs) > 16 and len({p[0] for p in pairs}) != len(pairs):
            unstable += 1   # std::sort's order among equal keys is introsort's beyond 16 elements: outside this restatement
        return [(p[0], p[2]) for p in pairs]
    nn = [[None] * len(lists[v]) for v in range(n)]
    rev = [[[] for _ in lists[v]] for v in range(n)]
    for v in range(n):
        for l, ids in enumerate(lists[v]):
            size = len(ids)
            lim = (top_M0 if size > thr[l] else low_m0) if l == 0 else (top_M if size > thr[l] else low_m)
            nn[v][l] = prune_list(by_dist(v, ids), lim)
    for v in range(n):
        for l in range(len(lists[v])):
            for u in nn[v][l]:
                rev[u][l].append(v)
    out = []
    for v in range(n):
        node = []
        for l in range(len(lists[v])):
            ids = sorted(set(nn[v][l]) | set(rev[v][l]))
            lim = maxM0 if l == 0 else maxM
            if len(ids) > lim:
                ids = prune_list(by_dist(v, ids), lim)
            if l != thr_level:   # hierarchical filter: off the threshold level only neighbours whose top level is l stay
                ids = [u for u in ids if len(lists[u]) - 1 == l]
            node.append(ids)
        out.append(node)
    return out, unstable
