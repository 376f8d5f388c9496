"""hs::slimq_kernel against the oracle on the hand-made files of slimq_handmade.py: lists wider than a tile on level 0, on the upper
levels or both (the CSR paths and their second 64-lane chunk, alone and mixed with fused tiles), steered ties of the estimates, every
shape of the register SearchBuffer and both result heaps, duplicate ids, n < k, and probe sequences of the expanded-node set longer
than 64 slots that wrap the table's end.  test_slimq_handmade_cpu.py pins the oracle's side of every case to a plain-Python reading
of the reference and asserts that each case reaches its path.

Nothing carries a tolerance: labels, distance bits, counts, the four traversal counters and the event traces are compared exactly."""
import numpy as np
import pytest

from hsutil import Oracle, load_product
from slimq_handmade import NAMES, cases

pytestmark = pytest.mark.gpu

TRACE_CAP, TRACE_Q = 32768, 8
LAYOUT = [n for n in NAMES if cases()[n].family == "layout"]


@pytest.fixture(scope="module")
def env(tmp_path_factory):
    """-> (product, get): get(name) = (case, path, oracle index, answers) with the oracle's answers per (ef, k) computed once"""
    P, O, tmp, memo = load_product(), Oracle(), tmp_path_factory.mktemp("slimq_handmade_gpu"), {}

    def get(name):
        if name not in memo:
            c = cases()[name]
            path = str(tmp / f"{name}.slimq")
            c.write(path)
            ox = O.load_slimq(path)
            ref = {}
            for ef, k in c.runs:
                ox.set(ef, c.t_const, c.rows)
                r = ox.search(c.queries, k, threads=8)
                r["trace"] = [ox.trace(c.queries[i], k, TRACE_CAP) for i in range(TRACE_Q)]
                ref[(ef, k)] = r
            memo[name] = (c, path, ox, ref)
        return memo[name]
    return P, get


def open_index(P, c, path, strides):
    ix = P.Index(path, P.HS_KIND_SLIMQ, c.dim, metric=c.metric)
    ix.slimq_set_dataset(c.rows)
    ix.slimq_set_tconst(c.t_const)
    if c.hash_slots:
        ix.set_capacity(0, c.hash_slots)
    got = (ix.debug_slimq_arrays(1)[1], ix.debug_slimq_arrays(2)[1])
    assert got == strides, f"{c.name}: tile strides {got}, the case is built for {strides}"
    return ix


def same_answers(got, ref, what):
    assert np.array_equal(got["stats"].astype(np.uint64), ref["counters"]), f"traversal differs: {what}"
    assert np.array_equal(got["cnt"], ref["counts"]), f"counts differ: {what}"
    assert np.array_equal(got["labels"], ref["labels"]), f"labels differ: {what}"
    assert np.array_equal(got["dists"].view(np.uint32), ref["dists"].view(np.uint32)), f"distance bits differ: {what}"


def run_case(P, get, name, strides=None):
    c, path, _, ref = get(name)
    ix = open_index(P, c, path, c.strides if strides is None else strides)
    for ef, k in c.runs:
        what = f"{name} ef={ef} k={k}"
        ix.set_ef(ef)
        same_answers(ix.slimq_search(c.queries, k, want_stats=True), ref[(ef, k)], what)
        assert ix.last_kernel() == "hs::slimq_kernel"
        tr, st = ix.slimq_trace(c.queries[:TRACE_Q], k, TRACE_CAP)
        assert np.array_equal(st.astype(np.uint64), ref[(ef, k)]["counters"][:TRACE_Q]), f"traced traversal differs: {what}"
        for i in range(TRACE_Q):
            want = ref[(ef, k)]["trace"][i]
            assert np.array_equal(tr[i][:len(want)], want) and np.all(tr[i][len(want):] == 0xFFFFFFFF), f"trace of query {i} differs: {what}"


@pytest.mark.parametrize("name", NAMES)
def test_slimq_handmade(env, name):
    P, get = env
    run_case(P, get, name)


@pytest.mark.parametrize("name", LAYOUT)
def test_slimq_handmade_without_tiles(env, monkeypatch, name):
    """the layout family once more over CSR lists and the record array alone (HS_SLIMQ_FUSED=0 is read at every load)"""
    P, get = env
    monkeypatch.setenv("HS_SLIMQ_FUSED", "0")
    run_case(P, get, name, strides=(0, 0))


@pytest.mark.parametrize("name", ["wide_both", "hub65", "upper65", "empty_level2"])
def test_slimq_handmade_ordered_two_launch_pass(env, name):
    """from 6144 queries on: descent, order by the entry's estimate, level-0 search -- over CSR lists and over mixed layouts"""
    P, get = env
    c, path, ox, _ = get(name)
    q = c.many_queries(6200)
    ix = open_index(P, c, path, c.strides)
    ix.set_ef(48)
    ox.set(48, c.t_const, c.rows)
    same_answers(ix.slimq_search(q, 10, want_stats=True), ox.search(q, 10, threads=8), f"{name}, 6200 queries")
    assert ix.last_kernel() == "hs::slimq_kernel"
