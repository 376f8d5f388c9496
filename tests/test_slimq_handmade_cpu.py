"""The oracle's SlimQ traversal (oracle/hs_oracle_slimq.hpp) against the plain-Python reading of the reference's source
(slimq_search_restated.py) on the hand-made files of slimq_handmade.py.  No GPU.

Everything is compared exactly: labels, distance bits, counts, the four traversal counters and the event traces.  The premises --
that a case really reaches the path it was built for -- are asserted on the oracle's answers alone, and each deliberately wrong
reading has to differ from the right one on the case built for it, which shows that the case can tell them apart."""
import hashlib

import numpy as np
import pytest

import slimq_search_restated as restated
from hsutil import Oracle
from slimq_handmade import HASH_SLOTS, NAMES, cases, probe_lengths
from slimq_resident_util import HANDMADE, numpy_arrays, parse_slimq, write_slimq

TRACE_CAP = 32768

# sha256 of every HANDMADE file (ncl = 2, as the resident tests write them) as the writer wrote them before it took explicit records
SHA256_BEFORE = {
    "deg16": "134a2e1dc7768b2cee4d8bfd87b40810cdd41454d407850f9f6e3df8d80d0fb8",
    "deg17": "dbd04acbb0fdb0ecf762ebfb4234f24168ab405767b0e5df2c5161d1ac85382d",
    "empty_level2": "4c688c5bf95813f15ce7de145e44b10f592ff7916c5076e6f80aa128965ae241",
    "hub64": "8e780d3e4f9a326dd1dc002ffb35d514f59ea81b0965f68474d3196c33022e26",
    "hub65": "6c4f5e25c246ead2eda64c7dd827c0a67d6c81c38d9f86ae32f3588ca077484d",
    "single": "0f6175d9ff7d9fe7970a2081fe365313502f1cae675f609163d63f12c457f59d",
    "upper17_d192": "581eb986a5c9434d1969cf07dc9035b15a74e222972fac3a3281a0c0f3ebe8e8",
    "upper65": "f67fd2fb12e151ad74c471b8ce04fa08d4d5e04a52b75d48912165b11959559a",
}


def test_write_slimq_same_bytes_as_before(tmp_path):
    assert sorted(SHA256_BEFORE) == sorted(HANDMADE)
    for name in sorted(HANDMADE):
        dim, lists, ep = HANDMADE[name]
        p = str(tmp_path / name)
        write_slimq(p, dim, lists, enterpoint=ep, ncl=2)
        assert hashlib.sha256(open(p, "rb").read()).hexdigest() == SHA256_BEFORE[name], name


def test_write_slimq_explicit_records(tmp_path):
    """explicit factors / cluster / code land in the records and move no other byte"""
    dim, lists, ep = HANDMADE["deg17"]
    n = len(lists)
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    write_slimq(a, dim, lists, enterpoint=ep, ncl=2)
    want = parse_slimq(a)
    fac = np.arange(3 * n, dtype=np.float32).reshape(n, 3)
    code = np.arange(n * 2, dtype=np.uint64).reshape(n, 2) * np.uint64(0x0123456789ABCDF)
    write_slimq(b, dim, lists, enterpoint=ep, ncl=2, factors=fac, cluster=np.ones(n, np.uint32), code=code)
    got = parse_slimq(b)
    assert np.array_equal(got["factors"], fac) and np.array_equal(got["code"], code) and np.all(got["cluster"] == 1)
    assert np.array_equal(got["level"], want["level"])
    write_slimq(b, dim, lists, enterpoint=ep, ncl=2, factors=want["factors"], cluster=want["cluster"], code=want["code"])
    assert open(a, "rb").read() == open(b, "rb").read()


class Loaded:
    """One case: its file, the oracle over it, the parsed fields, and per (ef, k) the oracle's answers and traces, computed once."""

    def __init__(self, O, case, path):
        self.O, self.case = O, case
        case.write(path)
        self.p = parse_slimq(path)
        self.ox = O.load_slimq(path)
        self.nq = 4 if case.n >= 1000 else len(case.queries)
        self.q = case.queries[:self.nq]
        self.prep = None
        self.labels = np.arange(case.n, dtype=np.uint64) * np.uint64(3) + np.uint64(1000)
        self._runs = {}

    def oracle(self, ef, k):
        if (ef, k) not in self._runs:
            self.ox.set(ef, self.case.t_const, self.case.rows)
            if self.prep is None:
                self.prep = self.ox.prepare(self.q)
            r = self.ox.search(self.q, k)
            r["trace"] = [self.ox.trace(self.q[i], k, TRACE_CAP) for i in range(self.nq)]
            self._runs[(ef, k)] = r
        return self._runs[(ef, k)]

    def python(self, qi, ef, k, wrong=None):
        self.oracle(ef, k)
        c, ox = self.case, self.ox
        est = restated.estimates(self.p, self.prep["q3"][qi], self.prep["g_add"][qi], self.prep["planes"][qi])
        exact = self.O.dist(c.metric, np.repeat(self.q[qi][None], c.n, 0), c.rows)
        return restated.search(self.p, ef, k, est, exact, ox.enterpoint, ox.maxlevel, ox.threshold_level, wrong=wrong)

    def same(self, qi, ef, k, got):
        """does a Python answer equal the oracle's, in everything?"""
        ref = self.oracle(ef, k)
        cnt = int(ref["counts"][qi])
        return (got["count"] == cnt and np.array_equal(self.labels[got["ids"]], ref["labels"][qi, :cnt])
                and np.all(ref["labels"][qi, cnt:] == np.uint64(0xFFFFFFFFFFFFFFFF))
                and np.array_equal(got["dists"].view(np.uint32), ref["dists"][qi, :cnt].view(np.uint32))
                and np.array_equal(np.array(got["counters"], np.uint64), ref["counters"][qi])
                and np.array_equal(got["trace"][:TRACE_CAP], ref["trace"][qi]))

    def events(self, qi, ef, k):
        """the oracle's trace as [(node, revisit, [inserted ids])] per pop"""
        tr = self.oracle(ef, k)["trace"][qi]
        assert len(tr) < TRACE_CAP
        out = []
        for a, b in tr.reshape(-1, 2).tolist():
            if a & (1 << 30):
                out[-1][2].append(a & ~(1 << 30))
            else:
                out.append((a & 0x7FFFFFFF, bool(a >> 31), []))
        return out

    def expansions(self, qi, ef, k):
        return [node for node, rev, _ in self.events(qi, ef, k) if not rev]


@pytest.fixture(scope="module")
def loaded(tmp_path_factory):
    O, tmp, memo = Oracle(), tmp_path_factory.mktemp("slimq_handmade"), {}

    def get(name):
        if name not in memo:
            memo[name] = Loaded(O, cases()[name], str(tmp / f"{name}.slimq"))
        return memo[name]
    return get


@pytest.mark.parametrize("name", NAMES)
def test_oracle_equals_python_reading(loaded, name):
    L = loaded(name)
    for ef, k in L.case.runs:
        for qi in range(L.nq):
            assert L.same(qi, ef, k, L.python(qi, ef, k)), f"{name}: query {qi} at ef={ef} k={k}"


@pytest.mark.parametrize("name", NAMES)
def test_expected_layout(tmp_path, name):
    """the strides each case states are the ones the stride rules give its file (numpy_arrays, an independent reading)"""
    c = cases()[name]
    p = str(tmp_path / "f.slimq")
    c.write(p)
    a = numpy_arrays(p)
    assert (a[1][1], a[2][1]) == c.strides


@pytest.mark.parametrize("name", ["hubs", "wide0", "wide0_up", "wide_both", "wide_both_d128_l2", "wide_both_d100_l2", "wide_both_d320_ip",
                                  "wide_both_d768_ip"])
def test_premise_wide_level0(loaded, name):
    """a query expands a node whose level-0 list is wider than 64 ids, and an insertion comes from a list index >= 64"""
    L = loaded(name)
    ef, k = L.case.runs[0]
    hit = False
    for qi in range(L.nq):
        for node, rev, ins in L.events(qi, ef, k):
            ids = [int(x) for x in L.p["lists"][node][0]] if len(L.p["lists"][node]) else []
            if not rev and len(ids) > 64 and any(ids.index(x) >= 64 for x in ins):
                hit = True
    assert hit


@pytest.mark.parametrize("name", ["wide_up", "wide_both"])
def test_premise_wide_upper(loaded, name):
    """the descent leaves a list of 130 ids through an index >= 64 for some query: the level-0 search starts there"""
    L = loaded(name)
    ef, k = L.case.runs[0]
    wide = [[int(x) for x in ls[1]] for ls in L.p["lists"] if len(ls) > 1 and len(ls[1]) == 130]
    assert wide
    firsts = {L.events(qi, ef, k)[0][0] for qi in range(L.nq)}
    assert any(f in w and w.index(f) >= 64 for f in firsts for w in wide)


@pytest.mark.parametrize("name", ["descent_ties_63", "descent_ties_64", "descent_ties_129", "descent_ties_9_69"])
def test_premise_descent_first_pop(loaded, name):
    L = loaded(name)
    ef, k = L.case.runs[0]
    for qi in range(L.nq):
        assert L.events(qi, ef, k)[0][0] == L.case.first_pop


def test_premise_all_equal_fills_the_default_table(loaded):
    """expansions against 75 % of the kernel's default expanded-node set, next_pow2(max(256, 4 ef)) slots: beyond it up to ef = 256
    (the second pass runs), below it at ef = 1024"""
    L = loaded("all_equal")
    for ef, k in L.case.runs:
        slots = 1 << (max(256, 4 * ef) - 1).bit_length()
        for qi in range(L.nq):
            e = len(L.expansions(qi, ef, k))
            print(f"all_equal ef={ef} k={k} query {qi}: {e} expansions, table {slots}")
            if ef <= 256:
                assert e * 4 > slots * 3
            if ef == 1024:
                assert e * 4 < slots * 3


@pytest.mark.parametrize("name", ["all_equal", "four_values"])
def test_premise_equal_exact_distances(loaded, name):
    L = loaded(name)
    for ef, k in L.case.runs:
        if k >= 63:
            d = L.oracle(ef, k)["dists"]
            assert all(len(set(d[qi].tolist())) < k for qi in range(L.nq))


def test_premise_duplicates_revisit(loaded):
    L = loaded("duplicates")
    ef, k = L.case.runs[0]
    assert np.all(L.oracle(ef, k)["counters"][:, 3] > 0)


def test_premise_n_lt_k(loaded):
    L = loaded("n_lt_k")
    for ef, k in L.case.runs:
        assert np.all(L.oracle(ef, k)["counts"] < k)
    assert np.all(L.oracle(16, 10)["counts"] == 3)   # nodes 0, 1, 2; node 3 has no list and is not re-ranked


@pytest.mark.parametrize("name,over", [("hash90", False), ("hash110", True)])
def test_premise_hash_chain(loaded, name, over):
    L = loaded(name)
    ef, k = L.case.runs[0]
    for qi in range(L.nq):
        ex = L.expansions(qi, ef, k)
        assert sorted(ex) == sorted(L.case.chain)
        longest, wrapped = probe_lengths(ex[:HASH_SLOTS * 3 // 4])
        print(f"{name} query {qi}: longest probe {longest}, wrapped {wrapped}")
        assert longest > 64 and wrapped
        assert (len(ex) * 4 > HASH_SLOTS * 3) == over   # beyond 75 % of 128 slots the first pass gives the query up


@pytest.mark.parametrize("wrong,name", [("descent_last_min", "descent_ties_9_69"), ("is_full_once", "four_values"),
                                        ("pool_refuses_held_id", "duplicates"), ("rerank_empty_node", "n_lt_k"),
                                        ("equal_key_behind", "all_equal")])
def test_wrong_reading_is_told_apart(loaded, wrong, name):
    L = loaded(name)
    differs = []
    for ef, k in L.case.runs:
        for qi in range(L.nq):
            differs.append(not L.same(qi, ef, k, L.python(qi, ef, k, wrong=wrong)))
    assert any(differs), f"{name} cannot tell the reading '{wrong}' from the right one"
