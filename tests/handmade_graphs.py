"""A catalogue of hand-made graphs for the search kernels: every list, level, label and mark chosen here, none by a builder.

Rows hold small integers in [0, 255], so every L2 distance is exact in fp32, every row is representable in u8 and fp16, and every
tie is there on purpose.  dim 16 (the flat kernel's) throughout; `chain`, `dup` and `levels` also come with dim 20 (D20), where
four more columns -- the parity of the node index -- take the graph to the runtime-dim fast and strict shapes.  16 queries per graph:
eight stored rows (distance 0 to a node) and eight stored rows moved by an integer step.

graphs() returns {name: Graph}; a Graph writes itself as a vanilla index file (hsutil.vanilla_bytes); the Slim file of the same graph
is chal_encode.vanilla_to_slim_verbatim of those bytes.  tests/golden/make_golden.py runs the compiled reference over the vanilla
files and records its answers in tests/golden/handmade.npz (the key scheme is key() below).  expected_kernel() restates, for the
shapes of this catalogue, which kernel a call runs: the CPU test holds hs_debug_search_plan to it, the GPU test hs_last_kernel.
"""
import numpy as np

from hsutil import vanilla_bytes

DIM = 16
D20 = ("chain", "dup", "levels")     # the graphs that also exist with dim 20, as <name>_d20
MARKDEL_EVERY = 7
ALLOW_ALL = (1 << 20, (1 << 20) - 1)  # (mod, rem) of the reference driver's filter "label % mod != rem" that no label of the catalogue fails
# (graph, k) whose queries reach fewer than k nodes: searchKnn(q, k, tableint*) runs nth_element past the end there
# (hnswalg_slim.h:2126), so HS_MODE_SLIM_IDS has no defined answer and these are compared in HS_MODE_PQ only.  (Vanilla files are
# searched in HS_MODE_PQ anyway -- the count-0 cases of the marks are theirs: a Slim file carries no mark, oracle/chal_encode.py.)
PQ_ONLY = {("one", 5), ("pair", 5), ("island", 30), ("marks_filters", 30)}


class Graph:
    def __init__(self, name, rows, lists, queries, ks, efs, M, upper=None, enterpoint=0, maxlevel=0, labels=None, marks=None, filters=()):
        self.name, self.rows, self.lists, self.queries = name, np.ascontiguousarray(rows, np.float32), lists, np.ascontiguousarray(queries, np.float32)
        self.ks, self.efs, self.M, self.upper, self.enterpoint, self.maxlevel = tuple(ks), tuple(efs), M, upper, enterpoint, maxlevel
        self.n, self.dim = self.rows.shape
        self.labels = np.arange(self.n, dtype=np.uint64) if labels is None else np.asarray(labels, np.uint64)
        self.marks = np.zeros(self.n, np.uint8) if marks is None else np.asarray(marks, np.uint8)
        self.filters = tuple(filters)   # (mod, rem) pairs beyond ALLOW_ALL: the filter allows label % mod != rem
        assert self.queries.shape == (16, self.dim) and self.n <= 130
        assert self.rows.min() >= 0 and self.rows.max() <= 255 and np.array_equal(self.rows, np.rint(self.rows))

    def vanilla(self):
        return vanilla_bytes(self.rows, self.lists, self.M, upper=self.upper, enterpoint=self.enterpoint, maxlevel=self.maxlevel,
                             labels=self.labels, marks=self.marks)

    def levels(self):
        return [0 if self.upper is None else len(self.upper[i]) for i in range(self.n)]

    def node_lists(self):
        """lists[i][l], l = 0..level of i (what Index.from_arrays and chal_encode.parse_vanilla speak)."""
        return [[self.lists[i]] + ([] if self.upper is None else list(self.upper[i])) for i in range(self.n)]

    def cases(self):
        return [(k, ef) for k in self.ks for ef in self.efs]

    def has_dup0(self):
        return any(len(set(l)) != len(l) for l in self.lists)

    def allowed(self, flt):
        """uint8[n] by internal id for the filter (mod, rem)."""
        return (self.labels % np.uint64(flt[0]) != np.uint64(flt[1])).astype(np.uint8)

    def with_dim20(self):
        tail = lambda a, par: np.concatenate([a, np.repeat(par[:, None], 4, axis=1).astype(np.float32)], axis=1)
        rows = tail(self.rows, np.arange(self.n) % 2)
        q = tail(self.queries, np.arange(16) % 2)
        return Graph(self.name + "_d20", rows, self.lists, q, self.ks, self.efs, self.M, self.upper, self.enterpoint, self.maxlevel,
                     self.labels, self.marks, self.filters)


def key(name, what, k, field, flt=None):
    """Key of handmade.npz; every array has a leading axis over the graph's efs.  what: "ref" = written by the compiled reference (vanilla searchKnn; with flt, under the driver's filter
    label % mod != rem); "oracle_slim_pq" / "oracle_slim_ids" / "oracle_slimdel_pq" = the oracle restatement of the Slim overloads
    (searchKnn(q, k), searchKnn(q, k, tableint*), and searchKnn(q, k) on the Slim file with has_deleted_elements set), which the
    compiled reference does not hold; with flt, searchKnn(q, k, isIdAllowed); "oracle_hnsw_pq" = the oracle's vanilla searchKnn, kept
    for its counters alone (the compiled reference counts distance calls only).  field: cnt, dists, labels, calls (ref), counters."""
    f = "" if flt is None else f"_f{flt[0]}r{flt[1]}"
    return f"{name}_{what}{f}_k{k}_{field}"


def _line(n, step, dim=DIM):
    """n rows on a line: 10 everywhere, column 0 = step * i."""
    rows = np.full((n, dim), 10.0, np.float32)
    rows[:, 0] = step * np.arange(n)
    return rows


def _queries(rows, picks, moved, shift=1.0):
    """Eight stored rows and eight stored rows moved by `shift` on column 0 and 1."""
    assert len(picks) == 8 and len(moved) == 8
    q = np.concatenate([rows[list(picks)], rows[list(moved)]]).astype(np.float32)
    q[8:, 0] += shift
    q[8:, 1] += shift
    return q


def _ring(ids, reach):
    """Ring lattice over `ids`: each names its `reach` successors and predecessors, nearest first."""
    m = len(ids)
    out = {}
    for p, i in enumerate(ids):
        out[i] = [ids[(p + s * d) % m] for d in range(1, reach + 1) for s in (1, -1)]
    return out


def _star(n_spokes, tie):
    """A hub (node 0) naming n_spokes spokes whose lists are empty.  tie: every spoke at squared distance 36 from the hub
    (equal_key_star's geometry: +-6 on an axis; from 33 spokes on also (4, 4, 2) on three consecutive axes, either sign).
    Otherwise spoke s sits s + 1 away on axis s % 16: all distances from the hub differ."""
    rows = np.full((n_spokes + 1, DIM), 100.0, np.float32)
    for s in range(n_spokes):
        if not tie:
            rows[1 + s, s % DIM] += s + 1
        elif s < 32:
            rows[1 + s, s % DIM] += 6 if s < 16 else -6
        else:
            sign, j = (1, s - 32) if s < 48 else (-1, s - 48)
            for o, v in enumerate((4, 4, 2)):
                rows[1 + s, (j + o) % DIM] += sign * v
    lists = [list(range(1, n_spokes + 1))] + [[] for _ in range(n_spokes)]
    sp = [1 + (i * 5) % n_spokes for i in range(7)]
    return rows, lists, _queries(rows, [0] + sp, [0] + sp)


def _chain():
    rows = _line(70, 3)
    lists = [[i + 1] for i in range(69)] + [[]]
    # queries at the far end: every hop of the chain is forced
    return rows, lists, _queries(rows, [69, 68, 67, 66, 60, 50, 69, 65], [69, 68, 67, 66, 60, 50, 64, 63])


def _island():
    rows = _line(40, 6)
    nb = {**_ring(list(range(20)), 2), **_ring(list(range(20, 40)), 2)}
    lists = [nb[i] for i in range(40)]
    return rows, lists, _queries(rows, [0, 5, 10, 19, 20, 25, 30, 39], [0, 7, 13, 19, 20, 27, 33, 39])


# The lists of `dup`, by node; every other node of its 76 has an empty list.  What each repeat is for:
DUP_LISTS = {
    0: [1, 2, 1, 3],                              # a repeat in the enter point's own list
    1: [4, 4, 5],                                 # twice, in neighbouring positions
    2: [6] + list(range(7, 69)) + [6],            # 64 ids: twice, at positions 0 and 63
    3: [69, 70, 69, 71, 69],                      # three times
    4: [0, 0, 1, 1, 72],                          # repeats of ids visited in earlier hops
    5: [5, 73],                                   # a self-loop
    6: [74] * 64,                                 # 64 copies of one id
    74: [75],
}
DUP_REPEATED = (1, 4, 6, 69, 74)                  # ids that are new when they are met twice in one list


def graphs():
    g = {}

    def add(*a, **kw):
        gr = Graph(*a, **kw)
        g[gr.name] = gr

    one = np.full((1, DIM), 10.0, np.float32)
    add("one", one, [[]], _queries(one, [0] * 8, [0] * 8), (1, 5), (1, 10), 2)
    pair = _line(2, 3)
    add("pair", pair, [[1], [0]], _queries(pair, [0, 1] * 4, [0, 1] * 4), (1, 2, 5), (1, 4), 2)
    rows, lists, q = _chain()
    add("chain", rows, lists, q, (1, 5), (1, 4, 70), 2)
    for ns in (16, 17, 32, 33, 64):   # tile strides 16, 32, 32, 48, 64: a list that ends on, one past, and fills the stride
        for tie in (True, False):
            rows, lists, q = _star(ns, tie)
            add(f"star{ns}" + ("" if tie else "_distinct"), rows, lists, q, (1, 10), (10, 64, 100), 32)
    rows = _line(76, 3)
    add("dup", rows, [DUP_LISTS.get(i, []) for i in range(76)], _queries(rows, [1, 4, 6, 69, 74, 5, 0, 40], [1, 4, 6, 69, 74, 5, 2, 72]),
        (1, 3, 10), (1, 10, 80), 32)
    rows, lists, q = _island()
    add("island", rows, lists, q, (30,), (10, 40), 2)
    same = np.full((100, DIM), 7.0, np.float32)
    nb = _ring(list(range(100)), 4)
    add("same", same, [nb[i] for i in range(100)], _queries(same, [0] * 8, [0] * 8, shift=2.0), (1, 10), (10, 50, 100), 4)
    # levels: column 0 of the 12 nodes; node 0 (level 3) is the enter point, nodes 1, 2 reach level 2, nodes 3, 4, 5 level 1
    pos = [100, 60, 40, 80, 20, 0, 10, 30, 50, 70, 90, 110]
    rows = np.full((12, DIM), 10.0, np.float32)
    rows[:, 0] = pos
    nb = _ring(list(range(12)), 2)
    upper = [[] for _ in range(12)]
    upper[0] = [[1, 3], [1, 1, 2], []]          # level 2 repeats id 1 (the descent has no visited set: two distance calls); level 3 is empty
    upper[1] = [[2, 3, 4], [0, 2]]
    upper[2] = [[1, 4, 5], [1, 0]]              # level 1 from node 2, query at column 0 = 30: node 4 ties with node 2 and must not win
    upper[3] = [[]]                             # an upper node with an empty upper list
    upper[4] = [[2, 5, 3]]
    upper[5] = [[4, 2]]
    q = _queries(rows, [0, 1, 2, 3, 4, 5, 7, 11], [0, 2, 4, 5, 6, 8, 9, 10])
    q[6] = rows[7]                              # column 0 = 30: between node 2 (40) and node 4 (20)
    add("levels", rows, [nb[i] for i in range(12)], q, (1, 5), (1, 10, 12), 4, upper=upper, maxlevel=3)
    # ---- marks and filters -----------------------------------------------------------------------------------------------------
    rows, lists, q = _chain()
    add("marks_chain_ep", rows, lists, q, (1, 5), (4, 70), 2, marks=[1] + [0] * 69)
    # the marks the reference driver's `markdel <every = 7>` sets on chain's file (labels 3, 10, 17, ...): make_golden.py holds the file
    # the compiled reference saves after markDelete to the bytes written here
    add("marks_chain_every7", rows, lists, q, (1, 5), (4, 70), 2, marks=[1 if i % MARKDEL_EVERY == MARKDEL_EVERY // 2 else 0 for i in range(70)])
    rows, lists, q = _star(32, True)
    add("marks_star32_ep", rows, lists, q, (1, 10), (10, 64), 32, marks=[1] + [0] * 32)
    rows, lists, q = _star(16, False)
    add("marks_allbut1", rows, lists, q, (1, 5), (10, 20), 32, marks=[0 if i == 6 else 1 for i in range(17)])
    add("marks_all", rows, lists, q, (1, 5), (10, 20), 32, marks=[1] * 17)
    # island again, labelled so that the driver's one-residue filter can allow nothing (label % 1 != 0), only the unreachable nodes
    # (label % 3 != 0) or only the enter point (label % 2 != 0): enter point 6 i + 3, reachable 6 i, unreachable 6 i + 4
    rows, lists, q = _island()
    labels = [6 * i + (3 if i == 0 else 0 if i < 20 else 4) for i in range(40)]
    add("marks_filters", rows, lists, q, (5, 30), (10, 40), 2, labels=labels, filters=((1, 0), (3, 0), (2, 0)))
    for name in D20:
        d = g[name].with_dim20()
        g[d.name] = d
    return g


# ---- which kernel a call of the catalogue runs (a restatement for these shapes: n <= 130, every list <= 64 ids, threshold_level 0,
# ef <= 512, k <= 64, the upper lists tiled) ---------------------------------------------------------------------------------------
def expected_kernel(g, k, ef, exact=False, marks=False, filt=False, rows="f32", f32_resident=True, raw=False):
    """marks: the index carries delete marks (or a Slim file's has_deleted_elements); filt: the call names a filter or a filter set."""
    run_ef = max(ef, k)
    bare = not (marks or filt)
    fast = not exact and not raw and (run_ef > k or (run_ef == k and run_ef <= 128 and bare))
    flat = fast and bare and g.dim % 16 == 0 and not g.has_dup0()
    family = "flat" if flat else "fast" if fast else "strict"
    narrow = rows != "f32" and (flat or not f32_resident)
    return f"hs::{family}_kernel" + (f"_{rows}" if narrow else "")


# ---- the routes of tests/test_gpu_handmade_graphs.py: how the index is set up and searched, as expected_kernel's keywords (`nq`, `cap`
# and `setup` are the test's own) ------------------------------------------------------------------------------------------------------
ROUTES = {
    "bare": dict(),                                            # the index as loaded: the flat kernel wherever it serves
    "u8": dict(rows="u8"), "f16": dict(rows="f16"),            # set_row_format: the flat kernel's narrow twins
    "u8_free": dict(rows="u8", f32_resident=False), "f16_free": dict(rows="f16", f32_resident=False),   # ... every kernel's
    "strict": dict(exact=True),                                # set_exact_order(True)
    "marks": dict(marks=True),                                 # the fast kernel through delete marks (Slim: has_deleted_elements alone)
    "filtered": dict(filt=True),                               # hs_search_batch_filtered
    "filter_set": dict(filt=True),                             # the fast kernel through a filter set
    "split": dict(nq=6144),                                    # the 16 queries tiled to the split pass's threshold
    "starved": dict(cap=(80, 256)),                            # set_capacity(80, 256): the re-run pass
    "arrays": dict(setup="arrays"),                            # Index.from_arrays
    "patch": dict(setup="patch"),                              # dup only: the repeats arrive through hs_index_patch
}


def routes_of(g, kind):
    """The routes a graph takes as index kind "hnsw" / "slim"."""
    marked = bool(g.marks.any())
    out = []
    for r in ROUTES:
        if r in ("u8", "f16", "u8_free", "f16_free") and g.dim % 16:
            continue   # narrow rows need dim % 16 == 0
        if r == "marks" and kind == "hnsw":
            continue   # a vanilla file says it with its marks: the marks_* graphs, on every route
        if r == "arrays" and kind == "slim" and marked:
            continue   # (arrays with marks would mark the nodes; the Slim file of a marked graph only sets has_deleted_elements)
        if r == "patch" and not (kind == "slim" and g.name.split("_d20")[0] == "dup"):
            continue
        out.append(r)
    return out


def route_kernel(g, kind, route, k, ef, exact=None):
    """hs_last_kernel after a search of graph g (kind "hnsw" / "slim") on `route`."""
    kw = {a: v for a, v in ROUTES[route].items() if a in ("rows", "f32_resident", "exact", "marks", "filt")}
    if exact is not None:
        kw["exact"] = exact
    kw["marks"] = kw.get("marks", False) or bool(g.marks.any())
    return expected_kernel(g, k, ef, **kw)
