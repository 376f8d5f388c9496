"""Every search kernel on the hand-made graphs of tests/handmade_graphs.py (an index smaller than a wavefront, an enter point with an
empty list, fewer reachable nodes than k, lists that fill the 64-id tile, lists that repeat an id, ...), one test per (graph, index
kind, route).  Expected: tests/golden/handmade.npz -- the compiled reference's answers on the vanilla files, the oracle restatement
(held to the compiled reference by tests/test_handmade_graphs_cpu.py) for the Slim overloads and the three counters.  Compared per
(k, ef): counts, sorted (dist bits, label) multisets, stats[:, :3], the reference's distance-call count, and hs_last_kernel.
HS_MODE_SLIM_IDS is compared wherever every query reaches k nodes (handmade_graphs.PQ_ONLY names the rest: undefined in the
reference, hnswalg_slim.h:2126)."""
import os

import numpy as np
import pytest

import handmade_graphs as hg
from hsutil import GOLDEN, load_chal_encode, load_product

pytestmark = pytest.mark.gpu
CATALOGUE = hg.graphs()
ce = load_chal_encode()
CASES = [(n, kind, r) for n, g in CATALOGUE.items() for kind in ("hnsw", "slim") for r in hg.routes_of(g, kind)]


@pytest.fixture(scope="module")
def hs():
    m = load_product()
    assert os.path.exists(m.LIB_PATH), "HIP extension missing: run __graft_entry__.build()"
    assert m.device_count() > 0, "no HIP device visible"
    return m


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "handmade.npz"))


def canon(d, l, c):
    """Per query the sorted keys (dist bits << 32 | label) of its first c[i] pairs, ~0 beyond (distances are >= 0, labels < 2^32)."""
    key = (np.ascontiguousarray(d, np.float32).view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.asarray(l).astype(np.uint64)
    key[np.arange(key.shape[1])[None, :] >= np.asarray(c)[:, None]] = np.iinfo(np.uint64).max
    return np.sort(key, axis=1)


def slim_bytes(g, raw=None, **kw):
    return ce.vanilla_to_slim_verbatim(g.vanilla() if raw is None else raw, **kw)


def make_index(hs, g, kind, route, tmp_path):
    r = hg.ROUTES[route]
    hkind = hs.HS_KIND_HNSW if kind == "hnsw" else hs.HS_KIND_SLIM
    if r.get("setup") == "arrays":
        ix = hs.Index.from_arrays(hkind, hs.HS_METRIC_L2, g.rows, g.levels(), g.node_lists(), g.enterpoint, g.maxlevel, labels=g.labels,
                                  deleted=g.marks if g.marks.any() else None)
    elif r.get("setup") == "patch":   # the same graph without its repeats, then the repeats as a genPatch stream
        import handmade_graphs
        plain = handmade_graphs.Graph(g.name, g.rows, [list(dict.fromkeys(l)) for l in g.lists], g.queries, g.ks, g.efs, g.M)
        old, new = slim_bytes(plain), slim_bytes(g)
        ix = hs.Index(old, hkind, g.dim, max_elements=g.n + 1)
        if g.dim % 16 == 0:
            ix.set_ef(10)
            ix.search_pq(g.queries, 3)
            assert ix.last_kernel() == "hs::flat_kernel" and hs.debug_plan_input(ix, 3, 16).has_dup0 == 0
        stream, n_old, n_new = ce.make_patch(old, new, g.dim)
        assert n_old == sum(len(set(l)) != len(l) for l in g.lists) and n_new == 0
        ix.patch(stream)
        assert hs.debug_plan_input(ix, 3, 16).has_dup0 == 1
    elif kind == "hnsw":
        ix = hs.Index(os.path.join(GOLDEN, f"handmade_{g.name}.hnsw.bin"), hkind, g.dim)
    else:
        ix = hs.Index(slim_bytes(g, has_deleted=True) if route == "marks" else slim_bytes(g), hkind, g.dim)
    assert ix.info()["n"] == g.n and hs.debug_plan_input(ix, 1, 16).has_dup0 == int(g.has_dup0())
    if "rows" in r:
        ix.set_row_format(hs.HS_ROWS_U8 if r["rows"] == "u8" else hs.HS_ROWS_F16)
        if not r.get("f32_resident", True):
            ix.set_f32_resident(False)
    if "cap" in r:
        ix.set_capacity(*r["cap"])
    return ix


@pytest.mark.parametrize("name,kind,route", CASES, ids=[f"{n}-{k}-{r}" for n, k, r in CASES])
def test_handmade_graph(hs, gold, tmp_path, name, kind, route):
    g = CATALOGUE[name]
    r = hg.ROUTES[route]
    ix = make_index(hs, g, kind, route, tmp_path)
    reps = r.get("nq", 16) // 16
    q = np.tile(g.queries, (reps, 1))
    tiled = lambda a: np.tile(a, (reps,) + (1,) * (a.ndim - 1))
    filtered = route in ("filtered", "filter_set")
    flts = ((hg.ALLOW_ALL,) + g.filters) if filtered else (None,)
    pq_what = "ref" if kind == "hnsw" else "oracle_slimdel_pq" if route == "marks" else "oracle_slim_pq"
    ids_what = "oracle_slimdel_ids" if route == "marks" else "oracle_slim_ids"
    ctr_what = "oracle_hnsw_pq" if kind == "hnsw" else pq_what
    fs = None
    if route == "filter_set":
        fs = hs.FilterSet(ix, len(flts))
        fs.write(0, np.stack([g.allowed(f) for f in flts]))
    for k in g.ks:
        for e, ef in enumerate(g.efs):
            ix.set_ef(ef)
            for fi, flt in enumerate(flts):
                for exact in ((False, True) if route == "starved" else (r.get("exact", False),)):
                    what = (name, kind, route, k, ef, flt, exact)
                    ix.set_exact_order(exact)
                    kernel = hg.route_kernel(g, kind, route, k, ef, exact=exact)
                    want = {f: tiled(gold[hg.key(name, pq_what, k, f, flt)][e]) for f in ("cnt", "dists", "labels")}
                    counters = tiled(gold[hg.key(name, ctr_what, k, "counters", flt)][e])
                    if route == "filtered":
                        got = ix.search_filtered(q, k, g.allowed(flt), want_stats=True)
                    elif route == "filter_set":
                        got = ix.search_filter_set(q, k, fs, np.full(len(q), fi, np.uint32), want_stats=True)
                    else:
                        got = ix.search_pq(q, k, want_stats=True)
                    assert ix.last_kernel() == kernel, (what, ix.last_kernel())
                    assert np.array_equal(got["cnt"], want["cnt"]), what
                    assert np.array_equal(canon(got["dists"], got["labels"], got["cnt"]), canon(want["dists"], want["labels"], want["cnt"])), what
                    assert np.array_equal(got["stats"][:, :3], counters), what
                    if kind == "hnsw":
                        assert np.array_equal(got["stats"][:, 0], tiled(gold[hg.key(name, "ref", k, "calls", flt)][e])), what
                    if kind != "slim" or filtered or (name.split("_d20")[0], k) in hg.PQ_ONLY:
                        continue
                    # searchKnn(q, k, tableint*): the k-set with its distances and the counters; under exact order also the array order
                    want = {f: tiled(gold[hg.key(name, ids_what, k, f)][e]) for f in ("labels", "dists", "counters")}
                    got = ix.search_ids(q, k, want_dists=True, want_stats=True)
                    assert ix.last_kernel() == kernel, (what, ix.last_kernel())
                    full = np.full(len(q), k)
                    assert np.array_equal(got["cnt"], full), what
                    assert np.array_equal(canon(got["dists"], got["labels"], full), canon(want["dists"], want["labels"], full)), what
                    assert np.array_equal(got["stats"][:, :3], want["counters"]), what
                    if exact:
                        assert np.array_equal(got["labels"], want["labels"]), what


@pytest.mark.parametrize("kind", ("hnsw", "slim"))
def test_empty_index_answers_nothing_and_launches_nothing(hs, kind):
    """cur_element_count == 0 (hnswalg.h:1382, hnswalg_slim.h:2031-2032 return an empty result): every search entry returns count 0
    and padding -- labels ~0, distances +inf, counters 0, empty raw heaps -- from the host, without a kernel (hs_last_kernel "")."""
    from hsutil import vanilla_bytes
    hkind = hs.HS_KIND_HNSW if kind == "hnsw" else hs.HS_KIND_SLIM
    empty = np.zeros((0, 16), np.float32)
    raw = vanilla_bytes(empty, [], 4, enterpoint=0xFFFFFFFF, maxlevel=-1)
    q = hg.graphs()["pair"].queries
    for ix in (hs.Index.from_arrays(hkind, hs.HS_METRIC_L2, empty, [], [], 0, 0), hs.Index(raw if kind == "hnsw" else slim_bytes(None, raw), hkind, 16)):
        assert ix.info()["n"] == 0
        ix.set_ef(10)
        outs = [ix.search_pq(q, 5, want_stats=True), ix.search_filtered(q, 5, np.zeros(0, np.uint8), want_stats=True)]
        for exact in (True, False):
            ix.set_exact_order(exact)
            outs.append(ix.search_pq(q, 5, want_stats=True))
        for o in outs:
            assert ix.last_kernel() == ""
            assert not o["cnt"].any() and not o["stats"].any()
            assert np.all(o["labels"] == np.iinfo(np.uint64).max) and np.all(np.isposinf(o["dists"]))
        raw_out = ix.search_raw(q, 5, mode=hs.HS_MODE_PQ)
        assert not raw_out["raw_sz"].any() and not raw_out["stats"].any() and ix.last_kernel() == ""
        if kind == "slim":
            o = ix.search_ids(q, 5, want_dists=True, want_stats=True)
            assert not o["cnt"].any() and np.all(o["labels"] == 0xFFFFFFFF) and np.all(np.isposinf(o["dists"])) and ix.last_kernel() == ""
