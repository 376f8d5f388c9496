"""The hand-made graph catalogue (tests/handmade_graphs.py) without a GPU: the files written by the extended writer parse back to
what was asked for and are the committed fixtures; the oracle restatement equals the compiled reference's recorded answers on
every graph (so it may stand in for it where the reference driver cannot reach: the Slim overloads, recorded under oracle_* keys);
the premises the graphs were made for hold on the reference's own output; and the launch plan names, for every route of the GPU
test, the kernel that test expects."""
import os

import numpy as np
import pytest

import handmade_graphs as hg
from hsutil import GOLDEN, load_chal_encode, load_product

CATALOGUE = hg.graphs()
ce = load_chal_encode()


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "handmade.npz"))


def path_of(name):
    return os.path.join(GOLDEN, f"handmade_{name}.hnsw.bin")


def multisets(d, l, c):
    """Per query the sorted (dist bits, label) pairs of the first c[i] entries."""
    return [sorted(zip(d[i, :int(c[i])].view(np.uint32).tolist(), np.asarray(l[i, :int(c[i])], np.uint64).tolist())) for i in range(len(c))]


@pytest.mark.parametrize("name", list(CATALOGUE))
def test_written_file_parses_back_and_is_the_fixture(name):
    g = CATALOGUE[name]
    raw = g.vanilla()
    assert raw == open(path_of(name), "rb").read(), "tests/golden is out of date: python tests/golden/make_golden.py handmade"
    p = ce.parse_vanilla(raw)
    assert (p["count"], p["dim"], p["maxlevel"], p["enterpoint"], p["M"], p["maxM0"]) == (g.n, g.dim, g.maxlevel, g.enterpoint, g.M, 2 * g.M)
    assert [len(node) - 1 for node in p["lists"]] == g.levels()
    want = g.node_lists()
    for i in range(g.n):
        assert [x.tolist() for x in p["lists"][i]] == [list(x) for x in want[i]], i
    assert np.array_equal(p["labels"], g.labels) and np.array_equal(p["marks"], g.marks) and np.array_equal(p["rows"], g.rows)
    s = ce.parse_slim(ce.vanilla_to_slim_verbatim(raw), g.dim)   # the Slim file of the same graph: the same lists
    assert all([x.tolist() for x in s["lists"][i]] == [list(x) for x in want[i]] for i in range(g.n))
    assert bool(s["has_deleted"]) == bool(g.marks.any())


def test_existing_writer_callers_get_the_same_bytes(tmp_path):
    """write_vanilla_level0 (now a call of vanilla_bytes): one level, label i, enter point 0, a zero linkLists_ word per node."""
    from hsutil import equal_key_star, write_vanilla_level0
    rows, lists = equal_key_star(20)
    write_vanilla_level0(str(tmp_path / "v.bin"), rows, lists, 16)
    raw = open(tmp_path / "v.bin", "rb").read()
    p = ce.parse_vanilla(raw)
    assert p["maxlevel"] == 0 and p["enterpoint"] == 0 and p["labels"].tolist() == list(range(21)) and not p["marks"].any()
    assert raw[-4 * 21:] == bytes(4 * 21) and [x[0].tolist() for x in p["lists"]] == lists


@pytest.mark.parametrize("name", list(CATALOGUE))
def test_oracle_equals_compiled_reference(oracle, gold, tmp_path, name):
    g = CATALOGUE[name]
    raw = open(path_of(name), "rb").read()
    sp, sd = str(tmp_path / "s.bin"), str(tmp_path / "sd.bin")
    open(sp, "wb").write(ce.vanilla_to_slim_verbatim(raw))
    open(sd, "wb").write(ce.vanilla_to_slim_verbatim(raw, has_deleted=True))
    ox = {"hnsw": oracle.load(path_of(name), "hnsw", 0, g.dim), "slim": oracle.load(sp, "slim", 0, g.dim), "slimdel": oracle.load(sd, "slim", 0, g.dim)}
    bare = not g.marks.any()
    for flt in (None, hg.ALLOW_ALL) + g.filters:
        for o in ox.values():
            o.set_filter(None if flt is None else g.allowed(flt))
        for k in g.ks:
            ref = {f: gold[hg.key(name, "ref", k, f, flt)] for f in ("cnt", "dists", "labels", "calls")}
            for e, ef in enumerate(g.efs):
                what = (name, flt, k, ef)
                for o in ox.values():
                    o.set_ef(ef)
                want = multisets(ref["dists"][e], ref["labels"][e], ref["cnt"][e])
                # vanilla: the oracle is the compiled reference, pair for pair and call for call
                v = ox["hnsw"].search_pq(g.queries, k)
                assert np.array_equal(v["cnt"], ref["cnt"][e]), what
                assert multisets(v["dists"], v["labels"], v["cnt"]) == want, what
                assert np.array_equal(v["counters"][:, 0], ref["calls"][e]), what
                assert np.array_equal(v["counters"][:, :3], gold[hg.key(name, "oracle_hnsw_pq", k, "counters", flt)][e]), what
                # the Slim overloads: what the fixture records under oracle_* is what the oracle says today ...
                for kind in ("slim",) + (("slimdel",) if flt is None else ()):
                    p = ox[kind].search_pq(g.queries, k)
                    rec = {f: gold[hg.key(name, f"oracle_{kind}_pq", k, f, flt)][e] for f in ("cnt", "dists", "labels", "counters")}
                    assert np.array_equal(p["cnt"], rec["cnt"]) and np.array_equal(p["counters"][:, :3], rec["counters"]), what
                    assert multisets(p["dists"], p["labels"], p["cnt"]) == multisets(rec["dists"], rec["labels"], rec["cnt"]), what
                    ids_key = hg.key(name, f"oracle_{kind}_ids", k, "labels")
                    assert (ids_key in gold.files) == (flt is not None or (name.split("_d20")[0], k) not in hg.PQ_ONLY) or flt is not None, what
                    if flt is not None or ids_key not in gold.files:
                        assert flt is not None or np.any(p["raw_sz"] < k), what   # PQ only exactly where fewer than k nodes are reached
                        continue
                    s = ox[kind].search_ids(g.queries, k)
                    assert np.array_equal(s["labels"], gold[ids_key][e]), what
                    assert np.array_equal(s["counters"][:, :3], gold[hg.key(name, f"oracle_{kind}_ids", k, "counters")][e]), what
                    # ... and, on the same verbatim graph, the compiled vanilla reference's: its distance multiset and (where no
                    # tie at the k-th place leaves the choice to nth_element / pop_heap) its k-set; on a bare file its call count
                    # less the entry distance only vanilla computes twice (hnswalg.h:347-351)
                    sd_ = gold[hg.key(name, f"oracle_{kind}_ids", k, "dists")][e]
                    got = multisets(sd_, s["labels"], np.full(16, k))
                    for i in range(16):
                        top = np.sort(s["raw_d"][i, :int(s["raw_sz"][i])])
                        tie = len(top) > k and top[k] == top[k - 1]
                        if bare:
                            assert [x[0] for x in got[i]] == [x[0] for x in want[i]], (what, i)
                            assert tie or got[i] == want[i], (what, i)
                    if bare and kind == "slim":
                        assert np.array_equal(s["counters"][:, 0], ref["calls"][e] - 1), what


def test_pq_only_cases_are_the_named_ones(gold):
    derived = {(n.split("_d20")[0], k) for n, g in CATALOGUE.items() for k in g.ks if hg.key(n, "oracle_slim_ids", k, "labels") not in gold.files}
    assert derived == hg.PQ_ONLY


def test_dup_premise_on_the_reference_output(gold):
    """There is a query whose reference k-set holds an id that a list repeats -- once -- with all k places taken: inserted twice, the
    id would take two places and push the k-th neighbour out."""
    for name in ("dup", "dup_d20"):
        g, found = CATALOGUE[name], []
        assert g.has_dup0() and all(any(l.count(r) > 1 for l in g.lists) for r in hg.DUP_REPEATED)
        for k in g.ks:
            if k < 2:
                continue
            lab, cnt, d = (gold[hg.key(name, "ref", k, f)] for f in ("labels", "cnt", "dists"))
            for e in range(len(g.efs)):
                for i in range(16):
                    once = [r for r in hg.DUP_REPEATED if (lab[e, i, :cnt[e, i]] == r).sum() == 1]
                    assert all((lab[e, i, :cnt[e, i]] == r).sum() <= 1 for r in range(g.n)), "the reference returned a label twice"
                    have = sorted(zip(d[e, i].tolist(), lab[e, i].tolist()))
                    for r in once if cnt[e, i] == k else []:
                        doubled = sorted(have + [x for x in have if x[1] == r])[:k]
                        if doubled != have:   # (a repeated id in the k-th place itself would only push its own copy out)
                            found.append((k, g.efs[e], i, r))
        assert found, name
        assert {r for *_, r in found} >= {1, 4}, found   # the enter point's repeat and the neighbouring-positions repeat both decide a k-set


def _descent(g, q, strict=True, dedup=False):
    """Greedy descent over the upper levels (hnswalg.h:1389-1415): (entry of level 0, distance calls)."""
    dist = lambda i: float(((g.rows[i] - q) ** 2).sum())
    cur, curd, calls, been = g.enterpoint, dist(g.enterpoint), 0, {g.enterpoint}
    for lvl in range(g.maxlevel, 0, -1):
        changed = True
        while changed:
            changed = False
            ids = g.upper[cur][lvl - 1]
            for c in (list(dict.fromkeys(ids)) if dedup else ids):
                calls += 1
                if dist(c) < curd or (not strict and dist(c) == curd and c not in been):
                    cur, curd, changed = c, dist(c), True
                    been.add(c)
    return cur, calls


def test_levels_premises_on_the_reference_output(gold):
    """levels: with ef = n the level-0 beam visits all 12 nodes of the ring, so the reference's call count is the entry, the descent's
    calls, the entry again (searchBaseLayerST) and the 11 other nodes -- the descent's calls counted with the repeated id computed
    twice.  And a neighbour at exactly the current distance does not move the descent."""
    g = CATALOGUE["levels"]
    assert any(len(u) and not len(u[-1]) for u in g.upper) and any(len(set(l)) != len(l) for u in g.upper for l in u)
    twice = moved = 0
    for i, q in enumerate(g.queries):
        entry, calls = _descent(g, q)
        twice += calls != _descent(g, q, dedup=True)[1]
        moved += entry != _descent(g, q, strict=False)[0]
        for k in g.ks:
            assert gold[hg.key("levels", "ref", k, "calls")][g.efs.index(12), i] == 1 + calls + 1 + 11, (i, k)
    assert twice > 0 and moved > 0


KIND = {"hnsw": 0, "slim": 1}
ROWS = {"f32": 0, "f16": 1, "u8": 2}


@pytest.mark.parametrize("name", list(CATALOGUE))
def test_plan_names_the_kernel_the_gpu_test_expects(name):
    hs = load_product()
    assert (hs.HS_ROWS_F32, hs.HS_ROWS_F16, hs.HS_ROWS_U8) == (0, 1, 2)
    g = CATALOGUE[name]
    n_checked = 0
    for kind in KIND:
        for route in hg.routes_of(g, kind):
            r = hg.ROUTES[route]
            cap = r.get("cap", (0, 0))
            for k, ef in g.cases():
                for exact in ((False, True) if route == "starved" else (r.get("exact", False),)):
                    p = hs.plan_input(n=g.n, dim=g.dim, has_tile0=1, has_uptile=int(g.maxlevel > 0), maxlevel=g.maxlevel, kind=KIND[kind],
                                      ef=ef, k=k, nq=r.get("nq", 16), has_deleted=int(bool(g.marks.any()) or r.get("marks", False)),
                                      has_filter=int(r.get("filt", False) and route == "filter_set"), exact_order=int(exact),
                                      row_fmt=ROWS[r.get("rows", "f32")], f32_resident=int(r.get("f32_resident", True)),
                                      has_dup0=int(g.has_dup0()), user_cand_cap=cap[0], user_hash_slots=cap[1])
                    if route == "filtered":   # hs_search_batch_filtered folds the filter into the delete marks
                        p.has_deleted = 1
                    plan = hs.debug_search_plan(p)
                    assert plan["name"] == hg.route_kernel(g, kind, route, k, ef, exact=exact), (kind, route, k, ef, exact, plan)
                    assert plan["split"] == int(r.get("nq", 16) >= 6144 and plan["family"] != hs.HS_PLAN_STRICT), (kind, route, k, ef)
                    n_checked += 1
    assert n_checked >= 2 * len(g.cases()) * 8
    if g.has_dup0():   # the same index without the repeats is the flat kernel's
        p = hs.plan_input(n=g.n, dim=g.dim, has_uptile=0, maxlevel=0, ef=10, k=3, nq=16)
        assert hs.debug_search_plan(p)["name"] == ("hs::flat_kernel" if g.dim % 16 == 0 else "hs::fast_kernel")
        p.has_dup0 = 1
        assert hs.debug_search_plan(p)["name"] == "hs::fast_kernel"
