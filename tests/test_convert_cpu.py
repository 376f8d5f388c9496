"""The product's CPU convertFromHNSW (hs_convert_slim, csrc/host_graph.hpp) against the oracle's independent restatement
(oracle/hs_oracle_convert.hpp): the Slim FILE must be byte-identical, at one thread and at eight.  The oracle sorts raw
(distance, id) arrays with std::sort as the reference does, so libstdc++'s order among equal keys is part of what is compared."""
import os

import numpy as np
import pytest

from hsutil import GOLDEN, equal_key_star, load_chal_encode, load_product, mixture, write_vanilla_level0
from slim_restated import degree_histogram, hub_threshold, int_rows

L2, IP = 0, 1
GOLDEN_GRAPHS = [("l2_cont_d32", L2, 32), ("l2_int_d16", L2, 16), ("ip_d48", IP, 48), ("l2_cont_d20", L2, 20), ("l2_cont_d21", L2, 21),
                 ("l2_cont_d10", L2, 10), ("ip_d20", IP, 20), ("ip_d21", IP, 21), ("ip_d10", IP, 10), ("l2_int_d16_del", L2, 16)]
PARAMS = {
    "default": {},                                   # the three parameter sets of test_gpu_convert.py
    "thr1": dict(threshold_level=1),
    "budgets": dict(top_degree_M0=16, low_degree_m0=4, top_degree_M=8, low_degree_m=2, top_degree_percent=0.3),
    "thr2": dict(threshold_level=2),
    "thr_above_maxlevel": dict(threshold_level=40),
    "alpha0": dict(top_degree_percent0=0.0, top_degree_percent=0.0),
    "alpha1": dict(top_degree_percent0=1.0, top_degree_percent=1.0),
    "wide_budgets": dict(top_degree_M0=64, low_degree_m0=48, top_degree_M=40, low_degree_m=33),   # larger than any list
}


@pytest.fixture(scope="module")
def hs():
    return load_product()


def same_as_oracle(hs, oracle, hp, dim, metric, tmp_path, **kw):
    """Oracle file == product file at threads 1 and 8; returns the oracle's premise statistics."""
    ref, got = str(tmp_path / "oracle.slim"), str(tmp_path / "product.slim")
    st = oracle.convert_slim(hp, ref, dim, metric=metric, **kw)
    want = open(ref, "rb").read()
    for threads in (1, 8):
        hs.convert_slim(hp, got, dim, metric=metric, threads=threads, **kw)
        assert open(got, "rb").read() == want, f"threads={threads} {kw}: product file != oracle file"
    return st


@pytest.mark.parametrize("params", list(PARAMS), ids=list(PARAMS))
@pytest.mark.parametrize("name,metric,dim", GOLDEN_GRAPHS, ids=[g[0] for g in GOLDEN_GRAPHS])
def test_convert_golden_graphs_match_oracle(hs, oracle, tmp_path, name, metric, dim, params):
    hp = os.path.join(GOLDEN, f"{name}.hnsw.bin")
    kw = PARAMS[params]
    st = same_as_oracle(hs, oracle, hp, dim, metric, tmp_path, **kw)
    g = load_chal_encode().parse_vanilla(open(hp, "rb").read())
    if params == "thr_above_maxlevel":
        assert kw["threshold_level"] > g["maxlevel"]
    if params == "wide_budgets":
        assert kw["low_degree_m0"] >= g["maxM0"] and kw["low_degree_m"] >= g["maxM"]
    assert st["thr"][0] == g["maxM0"] + 1   # level_cnts[0] is never counted: no level-0 hub


def _build(hs, tmp_path, base, metric=L2, M=16, efc=100, threads=8):
    hp = str(tmp_path / "h.bin")
    hs.build_hnsw(np.ascontiguousarray(base, np.float32), hp, metric=metric, M=M, ef_construction=efc, threads=threads)
    return hp


@pytest.mark.parametrize("dim,metric,integer", [(128, L2, True), (96, L2, False), (64, IP, False), (100, L2, True)])
def test_convert_m16_graphs_with_ties_match_oracle(hs, oracle, tmp_path, dim, metric, integer):
    """The tie-heavy M=16 graphs of test_gpu_convert_m16_graphs_with_ties: level-0 lists of up to 32 ids, many equal distances."""
    if integer:
        base = mixture(30000, dim, 5, lo=0, hi=6, sigma=1.5, integer=True, n_clusters=8)
    else:
        base = mixture(30000, dim, 6, lo=-1, hi=1, sigma=0.4, n_clusters=8)
    if metric == IP:
        base /= np.linalg.norm(base, axis=1, keepdims=True)
    hp = _build(hs, tmp_path, base, metric)
    st = same_as_oracle(hs, oracle, hp, dim, metric, tmp_path)
    same_as_oracle(hs, oracle, hp, dim, metric, tmp_path, low_degree_m0=24, top_degree_percent=0.1)
    if integer:
        assert st["n_eqkey_over16"] > 0, "expected lists of more than 16 ids with equal keys"


def test_convert_duplicated_rows_match_oracle(hs, oracle, tmp_path):
    """A cluster of 60 identical rows: their lists of 17..32 ids are all at distance 0, so std::sort's tie order decides."""
    base = mixture(3000, 16, 41, integer=True)
    base[100:160] = base[100]
    hp = _build(hs, tmp_path, base)
    st = same_as_oracle(hs, oracle, hp, 16, L2, tmp_path)
    same_as_oracle(hs, oracle, hp, 16, L2, tmp_path, low_degree_m0=32, top_degree_M0=32)
    assert st["n_eqkey_over16"] > 0


def test_convert_inner_product_unnormalised_matches_oracle(hs, oracle, tmp_path):
    """IP on rows that are not normalised: distances 1 - <a, b> far below zero."""
    base = mixture(4000, 32, 43, lo=-3, hi=3, sigma=2.0)
    hp = _build(hs, tmp_path, base, IP)
    same_as_oracle(hs, oracle, hp, 32, IP, tmp_path)
    same_as_oracle(hs, oracle, hp, 32, IP, tmp_path, threshold_level=1, top_degree_percent=0.2)
    assert oracle.dist(IP, base[:64], base[64:128]).min() < -1.0


@pytest.mark.parametrize("dim", (3, 4, 17, 100))
@pytest.mark.parametrize("metric", (L2, IP))
def test_convert_dims_off_simd16_match_oracle(hs, oracle, tmp_path, dim, metric):
    base = mixture(2000, dim, 45 + dim, lo=-1, hi=1, sigma=0.5)
    hp = _build(hs, tmp_path, base, metric, M=8, efc=60)
    same_as_oracle(hs, oracle, hp, dim, metric, tmp_path)
    same_as_oracle(hs, oracle, hp, dim, metric, tmp_path, threshold_level=1, top_degree_percent=0.5)


@pytest.mark.parametrize("n", (1, 2, 1037))
def test_convert_small_and_odd_counts_match_oracle(hs, oracle, tmp_path, n):
    base = mixture(n, 24, 47)
    hp = _build(hs, tmp_path, base, M=8, efc=40, threads=1)
    same_as_oracle(hs, oracle, hp, 24, L2, tmp_path)
    same_as_oracle(hs, oracle, hp, 24, L2, tmp_path, threshold_level=1, top_degree_percent=1.0)


def test_convert_float_hub_count_matches_oracle(hs, oracle, tmp_path):
    """The graph of test_slim_convert_restated_cpu.py with 75 nodes on level 2: the reference's float topN is 2 where a double one
    is 1, and the two give different level-2 thresholds, so a double product changes the hubs and the file."""
    base = int_rows(1191, 16, 1)
    hp = _build(hs, tmp_path, base, efc=40, threads=1)
    hist, cnts = degree_histogram(load_chal_encode().parse_vanilla(open(hp, "rb").read()))
    top_d = int(cnts[2] * np.float64(np.float32(0.02)) + 0.5)
    for thr in (0, 2):
        st = same_as_oracle(hs, oracle, hp, 16, L2, tmp_path, threshold_level=thr, top_degree_M0=12, low_degree_m0=5, top_degree_M=16,
                            low_degree_m=1)
        assert cnts[2] == 75 and st["topN"][2] == 2 and top_d == 1
        assert st["thr"][2] == hub_threshold(hist[2], 2) != hub_threshold(hist[2], top_d) and st["hubs"][2] > 0


@pytest.mark.parametrize("spokes", (16, 17, 32))
def test_convert_equal_key_lists_at_the_insertion_sort_boundary(hs, oracle, tmp_path, spokes):
    """A level-0 list of exactly `spokes` ids, all at the same distance, pruned to 8: std::sort of <= 16 elements is a pure
    insertion sort (the list order survives), beyond 16 introsort's partition reorders the ties and decides which 8 stay."""
    rows, lists = equal_key_star(spokes)
    hp = str(tmp_path / "star.bin")
    write_vanilla_level0(hp, rows, lists, M=16)
    st = same_as_oracle(hs, oracle, hp, 16, L2, tmp_path, low_degree_m0=8)
    kept = [int(x) for x in load_chal_encode().parse_slim(open(str(tmp_path / "oracle.slim"), "rb").read(), 16)["lists"][0][0]]
    assert len(kept) == 8
    assert (kept == list(range(1, 9))) == (spokes <= 16)
    assert st["n_eqkey_over16"] == (spokes > 16)
