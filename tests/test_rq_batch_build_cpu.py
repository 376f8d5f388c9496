"""The batched build of HNSW-SlimQ's base graph on the host (hs_build_rabitq_hnsw_batched with device = -1,
csrc/host_rq_batch_build.hpp): the compiled rabitqlib's edges at batch_max = 1, determinism, the plain-Python reading
of tests/rq_batch_build_restated.py (anchored to the compiled rabitqlib first), recall, shapes outside the device envelope."""
import os
import subprocess
import sys

import numpy as np
import pytest

import rq_batch_build_cases as C
import rq_batch_build_restated as R
from hsutil import GOLDEN, ROOT, load_chal_encode, load_product, mixture

sys.path.insert(0, GOLDEN)
from make_golden import RQ_HNSW_CASES, rq_hnsw_base  # noqa: E402

L2, IP = 0, 1


@pytest.fixture(scope="module")
def hs():
    m = load_product()
    m.build_library()
    return m


def flat_graph(g):
    out = [g["maxlevel"], g["enterpoint"]]
    for i in range(g["count"]):
        out += [int(g["labels"][i]), len(g["lists"][i]) - 1]
        for l in g["lists"][i]:
            out.append(len(l))
            out += [int(x) for x in l]
    return np.array(out, np.uint32)


def golden_levels(flat):
    """The level of every node of a fixture graph: [maxlevel, enterpoint, per node: label, level, per level count + ids]."""
    out, i = [], 2
    while i < len(flat):
        level = int(flat[i + 1])
        out.append(level)
        i += 2
        for _ in range(level + 1):
            i += 1 + int(flat[i])
    return out


@pytest.mark.parametrize("case", RQ_HNSW_CASES, ids=[c[0] for c in RQ_HNSW_CASES])
def test_batch_1_writes_the_compiled_rabitqlibs_edges(hs, tmp_path, case):
    """batch_max = 1 is the serial construct(): edge for edge the compiled rabitqlib's graph, byte for byte the serial builder's file."""
    name, n, d, metric, M, efc, integer = case
    ref = np.load(os.path.join(GOLDEN, "rabitq_hnsw_ref.npz"))
    base = rq_hnsw_base(n, d, metric, integer)
    assert float(base.astype(np.float64).sum()) == float(ref[name + "_rowsum"]), "regenerated rows differ from the fixture's"
    a, b = str(tmp_path / "batched.bin"), str(tmp_path / "serial.bin")
    st = hs.build_rabitq_hnsw_batched(base, a, metric=metric, M=M, ef_construction=efc, seed=100, threads=4, batch_max=1)
    assert not st["used_gpu"] and st["batches"] == n and st["flagged_rows"] == 0
    got = flat_graph(load_chal_encode().parse_vanilla(C.read(a)))
    assert got.shape == ref[name].shape and np.array_equal(got, ref[name])
    hs.build_rabitq_hnsw(base, b, metric=metric, M=M, ef_construction=efc, seed=100, threads=1)
    assert C.read(a) == C.read(b)


@pytest.mark.parametrize("kw", [{}, dict(batch_max=64, grow_div=1)], ids=["default", "small_batches"])
def test_schedule_is_deterministic(hs, tmp_path, kw):
    """The same bytes at 1, 4 and 16 threads and twice in a row; as many batches as the schedule of 4m point 2 gives for the file's levels."""
    base = mixture(2000, 24, 11)
    out = str(tmp_path / "o.bin")
    files = []
    for threads in (1, 4, 16, 16):
        st = hs.build_rabitq_hnsw_batched(base, out, M=8, ef_construction=60, threads=threads, **kw)
        files.append(C.read(out))
        assert st["batches"] == len(R.schedule(R.levels_of(files[-1]), **kw)) < 2000 and not st["used_gpu"]
    assert files[0] == files[1] == files[2] == files[3]


def test_reading_writes_the_compiled_rabitqlibs_edges_at_batch_1():
    """The anchor of the reading: the tie-heavy integer fixture the compiled rabitqlib built, edge for edge.  (The levels are the
    fixture's own here: it IS the reference.)"""
    name, n, d, metric, M, efc, integer = next(c for c in RQ_HNSW_CASES if c[0] == "l2_int_d64")
    ref = np.load(os.path.join(GOLDEN, "rabitq_hnsw_ref.npz"))
    base = rq_hnsw_base(n, d, metric, integer)
    assert float(base.astype(np.float64).sum()) == float(ref[name + "_rowsum"])
    assert R.exact_range(base, metric) < R.EXACT
    _, st, g = R.build(base, golden_levels(ref[name]), metric, M, efc, batch_max=1, want_graph=True)
    print(st)
    assert st["batches"] == n
    got = R.edges_of(g)
    assert got.shape == ref[name].shape and np.array_equal(got, ref[name])


@pytest.mark.parametrize("name", list(C.CASES))
def test_twin_equals_reading(hs, tmp_path, tmp_path_factory, name):
    _, metric, M, efc, kw = C.CASES[name]
    rows, levels, want, st = C.reading(hs, tmp_path_factory.mktemp("reading"), name)
    out = str(tmp_path / "twin.bin")
    tw = hs.build_rabitq_hnsw_batched(rows, out, metric=metric, M=M, ef_construction=efc, seed=C.SEED, device=-1, threads=8, **kw)
    got = C.read(out)
    print(f"{name}: stale words {st['stale_words']}, most incoming ids {st['max_incoming']}, largest candidate set {st['full_lists']}, batches {st['batches']}")
    assert not tw["used_gpu"] and tw["batches"] == st["batches"]
    assert R.levels_of(got) == levels
    assert got == want


@pytest.mark.parametrize("rule", R.RULES)
def test_the_comparison_notices_a_missing_rule(hs, tmp_path_factory, rule):
    """The reading with one rule switched off writes another file on a tie-heavy case (or, for the batch rule, on any case with a
    batch of two rows) -- except the present-check, which a build from nothing cannot reach: no old list names a new row."""
    differs = []
    for name in ("same_row", "grid_tight"):
        _, metric, M, efc, kw = C.CASES[name]
        rows, levels, want, st = C.reading(hs, tmp_path_factory.mktemp("reading"), name)
        raw, _ = R.build(rows, levels, metric, M, efc, off=(rule,), **kw)
        differs.append(raw != want)
    print(rule, differs)
    assert any(differs) == (rule != "present")


def recall(oracle, path, base, q, ef, k=10):
    ix = oracle.load(path, "hnsw", L2, base.shape[1])
    ix.set_ef(ef)
    r = ix.search_pq(q, k)
    gt = oracle.brute_force(L2, base, q, k)
    hits = sum(len(set(map(int, r["labels"][i][:r["cnt"][i]])) & set(map(int, gt[i]))) for i in range(len(q)))
    return hits / (k * len(q))


def test_recall_same_bar_as_the_parallel_builder(hs, oracle, tmp_path):
    """The bar of test_batch_build_cpu.py::test_recall_same_bar_as_the_parallel_builder: at ef 12, where nothing saturates, not more
    than 0.02 below the reference-equal serial graph of the same rows; 200 queries through the oracle's vanilla search."""
    base = mixture(3000, 32, 11)
    bp, sp = str(tmp_path / "batched.bin"), str(tmp_path / "serial.bin")
    hs.build_rabitq_hnsw_batched(base, bp, M=8, ef_construction=100, threads=8)
    hs.build_rabitq_hnsw(base, sp, M=8, ef_construction=100, threads=1)
    q = mixture(200, 32, 12)
    rb, rs = recall(oracle, bp, base, q, 12), recall(oracle, sp, base, q, 12)
    print(f"recall@10 ef 12, 200 queries: batched {rb:.4f} serial {rs:.4f}")
    assert rs < 0.99, "ef 12 saturates"
    assert rb >= rs - 0.02


@pytest.mark.parametrize("M,efc", [(33, 100), (8, 513)])
def test_shapes_outside_the_device_envelope_build_on_the_twin(hs, tmp_path, M, efc):
    base = mixture(300, 16, 5, integer=True)
    a, b = str(tmp_path / "a.bin"), str(tmp_path / "b.bin")
    st = hs.build_rabitq_hnsw_batched(base, a, M=M, ef_construction=efc, threads=4, batch_max=1)
    assert not st["used_gpu"] and st["batches"] == 300
    hs.build_rabitq_hnsw(base, b, M=M, ef_construction=efc, threads=1)
    assert C.read(a) == C.read(b)
    st = hs.build_rabitq_hnsw_batched(base, a, M=M, ef_construction=efc, threads=4)
    assert not st["used_gpu"] and st["batches"] == len(R.schedule(R.levels_of(C.read(a))))


def test_host_distance_entry_is_the_builders_distance(hs):
    """hs.rq_raw_dist(device=-1) on integer rows: the exact integers."""
    rows = C.signed_rows(200, 37)
    a, b = rows[:100], rows[100:]
    want = ((a.astype(np.int64) - b.astype(np.int64)) ** 2).sum(1)
    assert np.array_equal(hs.rq_raw_dist(a, b, L2).astype(np.int64), want)
    assert np.array_equal(hs.rq_raw_dist(a, b, IP).astype(np.int64), 1 - (a.astype(np.int64) * b.astype(np.int64)).sum(1))


def test_refusals_write_nothing(hs, tmp_path):
    import ctypes
    L = hs.lib()
    base = mixture(50, 16, 5)
    out = str(tmp_path / "never.bin")

    def call(base_p=base.ctypes.data, n=50, dim=16, metric=L2, M=8, opts=None, path=out.encode(), null_opts=False):
        o = opts or hs.HsBatchBuildOpts(-1, 1, 0, 0, 0)
        return L.hs_build_rabitq_hnsw_batched(base_p, n, dim, metric, M, 40, 100, None if null_opts else ctypes.byref(o), path, None)

    assert call() == hs.HS_OK and os.path.exists(out)
    os.remove(out)
    for what, rc in [("null base", call(base_p=None)), ("null path", call(path=None)), ("null options", call(null_opts=True)), ("n = 0", call(n=0)),
                     ("dim = 0", call(dim=0)), ("metric", call(metric=7)), ("M = 1", call(M=1)),
                     ("device below -1", call(opts=hs.HsBatchBuildOpts(-3, 1, 0, 0, 0))),
                     ("scratch_ids not a power of two", call(opts=hs.HsBatchBuildOpts(-1, 1, 0, 0, 100)))]:
        assert rc == hs.HS_ERR_INVALID, what
        assert L.hs_last_error(), what
        assert not os.path.exists(out), what


def test_rq_batch_build_under_sanitizers(hs):
    """csrc/rq_batch_build_test.cpp under AddressSanitizer + UBSan, as its own binary (never inside Python): batch_max = 1 against the
    serial builder, 1 against 4 workers, both metrics on tie-heavy rows."""
    d = os.path.join(ROOT, "hnsw-slim_amd")
    subprocess.check_call(["make", "-C", d, "rq_batch_build_test"])
    out = subprocess.run([os.path.join(d, "rq_batch_build_test")], capture_output=True, text=True)
    assert out.returncode == 0 and "rq_batch_build ok" in out.stdout, out.stdout + out.stderr
