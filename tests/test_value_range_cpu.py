"""CPU twin of tests/test_gpu_value_range.py: what that file takes for granted, checked without a device.

  * the premises of every value family (tests/value_range.py) on the oracle alone, on the very files and (ef, k) pairs the GPU legs
    use -- a seed or an exponent that stops meeting its premise fails here, before a GPU box is spent on it;
  * the multiply by 2^s is exact, so every family has the base draw's mantissas;
  * the host builder and the host convertFromHNSW on subnormal and 2^100-sized distances: the built graph is searchable to the
    recall the same draw has unscaled, and the Slim file is the oracle's byte for byte (test_convert_cpu.same_as_oracle);
  * the l2_overflow premise on the oracle's distance table."""
import numpy as np
import pytest

import value_range as vr
from hsutil import load_product
from test_convert_cpu import same_as_oracle

L2, IP = vr.L2, vr.IP
CASES = vr.cases()


@pytest.fixture(scope="module")
def hs():
    return load_product()


@pytest.fixture(scope="module")
def files(hs, tmp_path_factory):
    folder = str(tmp_path_factory.mktemp("value_range_cpu"))
    return {case: vr.build_files(hs, case, folder) for case in CASES}


def test_scaling_is_exact_and_in_range():
    for case in CASES + [("l2_overflow", L2, vr.OVERFLOW_DIM, vr.OVERFLOW_EXP)]:
        _, _, d, s = case
        x = vr.base_draw(vr.N, d, vr.SEEDS[0] + d)
        y = vr.scaled(x, s)
        m, e = np.frexp(x)
        m2, e2 = np.frexp(y)
        assert np.array_equal(m, m2) and np.all((e2 - e)[x != 0] == s), vr.case_name(case)
        assert np.all(np.isfinite(y)) and np.all(np.abs(y[y != 0]) >= vr.SUBNORMAL), f"{vr.case_name(case)}: a subnormal or non-finite input"


@pytest.mark.parametrize("case", CASES, ids=[vr.case_name(c) for c in CASES])
def test_family_premises_hold_on_the_oracle(oracle, files, case):
    f = files[case]
    family, metric, d, _ = case
    for kind, path in (("slim", f["sp"]), ("hnsw", f["hp"])):
        ox = oracle.load(path, kind, metric, d)
        for ef, k in vr.FLAT_PAIRS + vr.FAST_PAIRS + vr.STRICT_PAIRS + vr.LEAN_PAIRS:
            vr.reference(ox, family, d, f["q"], ef, k, kind == "slim", f"{f['name']} {kind} ef={ef} k={k}")
    # the filter of the not-bare legs (by label == internal id here): half the rows
    ox = oracle.load(f["hp"], "hnsw", metric, d)
    ox.set_filter(vr.allowed_half(np.arange(f["n"], dtype=np.uint64)))
    for ef, k in vr.NOT_BARE_PAIRS:
        vr.reference(ox, family, d, f["q"], ef, k, False, f"{f['name']} filter ef={ef} k={k}")


def test_ip_cross_family_has_a_k64_crossing(oracle, files):
    """The family-level premise: at k = 64 at least one query's results cross zero (value_range.IP_CROSS_EXP says where it can)."""
    n = 0
    for case in CASES:
        if case[0] == "ip_cross":
            f = files[case]
            ox = oracle.load(f["sp"], "slim", IP, case[2])
            ox.set_ef(200)
            n += int(vr.crossing(ox.search_ids(f["q"], 64, threads=8), 64).sum())
    assert n >= 1


@pytest.mark.parametrize("case", [c for c in CASES if c[0] in ("l2_subnormal", "large")], ids=lambda c: vr.case_name(c))
def test_host_builder_and_convert_at_the_range_edges(hs, oracle, files, case, tmp_path):
    """The scale is a power of two, so every comparison the builder makes has the outcome it has on the base draw unless a distance
    leaves the normal range: recall against the exhaustive answer stays what a 2000-row M = 12 graph gives, and the host convert
    writes the oracle's bytes."""
    f = files[case]
    family, metric, d, _ = case
    ox = oracle.load(f["hp"], "hnsw", metric, d)
    ox.set_ef(200)
    r = ox.search_pq(f["q"], 10, threads=8)
    gt = oracle.brute_force(metric, f["base"], f["q"], 10)
    hits = sum(len(set(map(int, r["labels"][i])) & set(map(int, gt[i]))) for i in range(len(gt)))
    assert hits / gt.size > 0.9
    same_as_oracle(hs, oracle, f["hp"], d, metric, tmp_path)
    same_as_oracle(hs, oracle, f["hp"], d, metric, tmp_path, threshold_level=1, top_degree_percent=0.2)


def test_l2_overflow_premise(oracle):
    base, q = vr.overflow_rows_and_queries()
    vr.check_overflow(vr.dist_table(oracle, L2, base, q), vr.OVERFLOW_K, "l2_overflow")
