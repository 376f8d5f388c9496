"""The graph under HNSW-SlimQ, built the way the reference builds it (CPU harness, SURVEY.md 8 row a12/"next"):

  * hs_build_rabitq_hnsw  == rabitqlib::hnsw::HierarchicalNSW::construct's edges (third_party/rabitqlib/index/hnsw/hnsw.hpp:667-1054),
    pinned edge for edge against the compiled rabitqlib (tests/golden/rabitq_hnsw_ref.npz, made by make_golden.py rqhnsw from
    oracle/_ref/ref_rabitq's `hnsw` command; serial build, seed 100);
  * hs_convert_slimq_graph == HierarchicalNSWSlimQ::convertFromHNSW's graph passes (hnswalg_slimq.h:1546-1762) with its own
    PruneByHeuristic (:1334-1362).  hnswalg_slimq.h needs folly and cannot be compiled here, so this half is checked against the
    plain-Python restatement of tests/slim_restated.py on integer-valued rows (every distance exact in any summation order).
"""
import os
import sys

import numpy as np
import pytest

from hsutil import GOLDEN, load_chal_encode, load_product
from slim_restated import convert_graph_restated

sys.path.insert(0, GOLDEN)
from make_golden import RQ_HNSW_CASES, rq_hnsw_base  # noqa: E402


@pytest.fixture(scope="module")
def hs():
    return load_product()


def flat_graph(g):
    out = [g["maxlevel"], g["enterpoint"]]
    for i in range(g["count"]):
        out += [int(g["labels"][i]), len(g["lists"][i]) - 1]
        for l in g["lists"][i]:
            out.append(len(l))
            out += [int(x) for x in l]
    return np.array(out, np.uint32)


@pytest.mark.parametrize("case", RQ_HNSW_CASES, ids=[c[0] for c in RQ_HNSW_CASES])
def test_rabitq_builder_matches_compiled_rabitqlib(hs, tmp_path, case):
    name, n, d, metric, M, efc, integer = case
    ref = np.load(os.path.join(GOLDEN, "rabitq_hnsw_ref.npz"))
    base = rq_hnsw_base(n, d, metric, integer)
    assert float(base.astype(np.float64).sum()) == float(ref[name + "_rowsum"]), "regenerated rows differ from the fixture's"
    p = str(tmp_path / "rq.bin")
    hs.build_rabitq_hnsw(base, p, metric=metric, M=M, ef_construction=efc, seed=100, threads=1)
    g = load_chal_encode().parse_vanilla(open(p, "rb").read())
    assert g["M"] == M and g["maxM"] == M and g["maxM0"] == 2 * M and g["efC"] == max(efc, M)
    assert np.array_equal(g["rows"], base)
    got = flat_graph(g)
    want = ref[name]
    assert got.shape == want.shape and np.array_equal(got, want)


def test_rabitq_builder_parallel_keeps_ids_and_is_connected(hs, tmp_path):
    name, n, d, metric, M, efc, integer = RQ_HNSW_CASES[0]
    base = rq_hnsw_base(n, d, metric, integer)
    p = str(tmp_path / "rq.bin")
    hs.build_rabitq_hnsw(base, p, metric=metric, M=M, ef_construction=efc, seed=100, threads=4)
    g = load_chal_encode().parse_vanilla(open(p, "rb").read())
    assert np.array_equal(g["labels"], np.arange(n, dtype=np.uint64)) and np.array_equal(g["rows"], base)
    seen = {int(g["enterpoint"])}
    todo = [int(g["enterpoint"])]
    while todo:   # reachability over all levels from the entry point
        u = todo.pop()
        for l in g["lists"][u]:
            for v in l:
                if int(v) not in seen:
                    seen.add(int(v))
                    todo.append(int(v))
    assert len(seen) > 0.99 * n


def test_slimq_graph_conversion_matches_python_restatement(hs, tmp_path):
    rng = np.random.default_rng(77)
    n, d, M = 700, 64, 8
    centres = rng.integers(-60, 60, (12, d))
    base = (centres[rng.integers(0, 12, n)] + rng.integers(-25, 26, (n, d))).astype(np.float32)
    hp, sp, vp = (str(tmp_path / x) for x in ("h.bin", "s.bin", "v.bin"))
    hs.build_rabitq_hnsw(base, hp, M=M, ef_construction=40, threads=1)
    kw = dict(threshold_level=0, top_degree_percent0=0.02, top_degree_percent=0.02, top_degree_M0=12, low_degree_m0=5, top_degree_M=6,
              low_degree_m=3)
    hs.convert_slimq_graph(hp, sp, d, threads=2, **kw)
    ce = load_chal_encode()
    g = ce.parse_vanilla(open(hp, "rb").read())
    s = ce.parse_slim(open(sp, "rb").read(), d)
    want, unstable = convert_graph_restated(g, base, kw["threshold_level"], kw["top_degree_percent0"], kw["top_degree_percent"],
                                            kw["top_degree_M0"], kw["low_degree_m0"], kw["top_degree_M"], kw["low_degree_m"], prune="slimq")
    assert unstable == 0, "premise: no equal keys in a list of more than 16 (choose another seed)"
    n_reprune = 0
    for v in range(n):
        assert len(s["lists"][v]) == len(want[v])
        for l in range(len(want[v])):
            assert [int(x) for x in s["lists"][v][l]] == want[v][l], (v, l)
            n_reprune += want[v][l] != sorted(want[v][l])
    assert sum(len(w) > 1 and any(w[1:]) for w in want) > 0, "no upper-level list survived the filter"
    assert n_reprune > 0, "the re-prune path (:1690-1716) was not exercised"
    # and it is NOT what Slim's own heuristic (hnswalg_slim.h:836-865) gives on the same input
    hs.convert_slim(hp, vp, d, threads=2, **kw)
    v = ce.parse_slim(open(vp, "rb").read(), d)
    assert any([int(x) for x in v["lists"][i][0]] != want[i][0] for i in range(n))
