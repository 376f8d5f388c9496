"""The oracle's HierarchicalNSWSlim::convertFromHNSW (oracle/hs_oracle_convert.hpp) against a second, independent reading of
hnswalg_slim.h:836-1108: the plain-Python passes of tests/slim_restated.py with Slim's own PruneByHeuristic.

The class needs folly and cannot be compiled here, so two readings that agree list for list are what pins the conversion.  The
rows are integer-valued L2, so every distance is an exact int64 in any summation order and only the decisions are compared.
Python's sort is stable, std::sort is not beyond 16 elements: the graphs are chosen so that no list longer than 16 holds two
equal keys, and the test asserts that from the oracle's statistics rather than tolerating it.
"""
import numpy as np
import pytest

from hsutil import load_chal_encode, load_product
from slim_restated import convert_graph_restated, degree_histogram, hub_threshold, hub_top_n, int_rows

KW = dict(top_degree_percent0=0.02, top_degree_percent=0.02, top_degree_M0=12, low_degree_m0=5, top_degree_M=16, low_degree_m=1)
# (M, n, d, seed).  The first 1191 rows of the builder's seed-100 level draws put 75 nodes on level 2: the count where the
# reference's float topN (2) and a double one (1) differ; this M=16 graph's two largest level-2 degrees differ, so the two
# readings also give different thresholds.  The M=6 graph fills its unions beyond maxM0, so the re-prune runs.
GRAPHS = [(16, 1191, 16, 1), (6, 1191, 16, 2)]


@pytest.fixture(scope="module")
def hs():
    return load_product()


def test_oracle_convert_matches_python_restatement(hs, oracle, tmp_path):
    ce = load_chal_encode()
    covered, n_reprune, hub_levels, rounding_cases = set(), 0, set(), 0
    for M, n, d, seed in GRAPHS:
        base = int_rows(n, d, seed)
        hp = str(tmp_path / f"h{M}.bin")
        hs.build_hnsw(base, hp, M=M, ef_construction=40, threads=1)
        g = ce.parse_vanilla(open(hp, "rb").read())
        hist, cnts = degree_histogram(g)
        for l in range(1, g["maxlevel"] + 1):
            c = int(cnts[l])
            if c % 50 == 25 and c >= 75:
                top_f = hub_top_n(c, 0.02)
                top_d = int(c * np.float64(np.float32(0.02)) + 0.5)   # the same product taken in double
                print(f"M={M} level {l}: {c} nodes, topN float {top_f} double {top_d}, thresholds "
                      f"{hub_threshold(hist[l], top_f)} / {hub_threshold(hist[l], top_d)}")
                rounding_cases += top_f != top_d and hub_threshold(hist[l], top_f) != hub_threshold(hist[l], top_d)
        for thr_level in (0, 1, 2):
            sp = str(tmp_path / f"s{M}_{thr_level}.slim")
            st = oracle.convert_slim(hp, sp, d, threshold_level=thr_level, **KW)
            assert st["n_eqkey_over16"] == 0, "premise: no equal keys in a sorted list of more than 16 (choose another seed)"
            s = ce.parse_slim(open(sp, "rb").read(), d)
            want, unstable = convert_graph_restated(g, base, thr_level, KW["top_degree_percent0"], KW["top_degree_percent"],
                                                    KW["top_degree_M0"], KW["low_degree_m0"], KW["top_degree_M"], KW["low_degree_m"],
                                                    prune="slim")
            assert unstable == 0
            hist_thr = [hub_threshold(hist[l], hub_top_n(cnts[l], 0.02)) for l in range(g["maxlevel"] + 1)]
            assert list(st["thr"]) == hist_thr, (M, thr_level)
            assert s["threshold_level"] == thr_level and s["maxlevel"] == g["maxlevel"]
            for v in range(n):
                assert len(s["lists"][v]) == len(want[v]), (M, thr_level, v)
                for l in range(len(want[v])):
                    assert [int(x) for x in s["lists"][v][l]] == want[v][l], (M, thr_level, v, l)
            covered.add(thr_level)
            n_reprune += st["n_reprune"]
            hub_levels |= {l for l in range(1, len(st["hubs"])) if st["hubs"][l] > 0}
    assert covered == {0, 1, 2}
    assert n_reprune > 0, "the re-prune path (hnswalg_slim.h:1038-1062) was not exercised"
    assert hub_levels, "no hub at any level >= 1"
    assert rounding_cases > 0, "no level count where the float and double hub counts give different thresholds"
