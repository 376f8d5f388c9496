"""Batched addPoint on the host (hs_build_hnsw_batched with device = -1, csrc/host_batch_build.hpp) and its schedule
(hs_build_schedule): the reference's bytes at batch_max = 1, the schedule's rules, determinism, structure, recall, refusals."""
import ctypes
import os
import struct

import numpy as np
import pytest

from hsutil import GOLDEN, load_product, mixture

L2, IP = 0, 1
NONE = 0xFFFFFFFF


@pytest.fixture(scope="module")
def hs():
    m = load_product()
    m.build_library()
    return m


def parse_hnsw(raw, dim):
    """Independent parse of a saveIndex file (hnswalg.h:748-779): header, per node level-0 list, label, upper lists."""
    (off0, max_el, count, spe, label_off, data_off, maxlevel, ep, maxM, maxM0, M, mult, efc) = struct.unpack_from("<6QiI3QdQ", raw, 0)
    assert off0 == 0 and spe == maxM0 * 4 + 4 + 4 * dim + 8 and data_off == maxM0 * 4 + 4
    el = np.frombuffer(raw, np.uint8, count * spe, 96).reshape(count, spe)
    words = el[:, :data_off].copy().view(np.uint32)
    cnt0 = words[:, 0] & 0xFFFF
    labels = el[:, label_off:label_off + 8].copy().view(np.uint64)[:, 0]
    lists = [[words[i, 1:1 + cnt0[i]]] for i in range(count)]
    off = 96 + count * spe
    for i in range(count):
        (sz,) = struct.unpack_from("<I", raw, off); off += 4
        assert sz % (maxM * 4 + 4) == 0
        for l in range(sz // (maxM * 4 + 4)):
            w = np.frombuffer(raw, np.uint32, maxM + 1, off + l * (maxM * 4 + 4))
            lists[i].append(w[1:1 + (w[0] & 0xFFFF)])
        off += sz
    assert off == len(raw)
    return dict(count=count, maxlevel=maxlevel, ep=ep, maxM=maxM, maxM0=maxM0, M=M, efc=efc, lists=lists, labels=labels, cnt0=cnt0)


@pytest.mark.parametrize("name,metric", [("l2_cont_d32", L2), ("l2_int_d16", L2), ("ip_d48", IP), ("l2_cont_d20", L2),
                                         ("l2_cont_d21", L2), ("l2_cont_d10", L2), ("ip_d20", IP), ("ip_d21", IP),
                                         ("ip_d10", IP)])
def test_batch_1_writes_reference_bytes(hs, tmp_path, name, metric):
    """batch_max = 1 is the reference's serial addPoint loop: the golden file of the serial builder's test, byte for byte."""
    g = np.load(os.path.join(GOLDEN, f"{name}.npz"))
    out = str(tmp_path / "mine.bin")
    st = hs.build_hnsw_batched(g["base"], out, metric=metric, M=int(g["M"]), ef_construction=int(g["efC"]), branching_factor="4", seed=100,
                               threads=4, batch_max=1)
    assert not st["used_gpu"] and st["batches"] == len(g["base"]) and st["flagged_rows"] == 0
    assert open(out, "rb").read() == open(os.path.join(GOLDEN, f"{name}.hnsw.bin"), "rb").read()


def test_batch_build_under_sanitizers(hs):
    """csrc/batch_build_test.cpp under AddressSanitizer + UBSan, as its own binary (never inside Python): batch_max = 1 against the
    serial builder, 1 against 4 workers, both metrics on tie-heavy rows; the schedule's sums and cuts."""
    import subprocess
    from hsutil import ROOT
    d = os.path.join(ROOT, "hnsw-slim_amd")
    subprocess.check_call(["make", "-C", d, "batch_build_test"])
    out = subprocess.run([os.path.join(d, "batch_build_test")], capture_output=True, text=True)
    assert out.returncode == 0 and "batch_build ok" in out.stdout, out.stdout + out.stderr


def raisers(hs, n, M, seed):
    """Per row, whether it raises the top level of a serial build: the serial schedule reports the top level before every row
    (the last row's own level stays unknown: None)."""
    s = hs.build_schedule(n, M=M, seed=seed, batch_max=1)
    assert list(s["sizes"]) == [1] * n
    tops = s["top_levels"]
    return [bool(tops[i + 1] > tops[i]) for i in range(n - 1)] + [None], s


def check_schedule(hs, n, M, seed, grow_div, batch_max):
    rz, serial = raisers(hs, n, M, seed)
    s = hs.build_schedule(n, M=M, seed=seed, grow_div=grow_div, batch_max=batch_max)
    sizes = [int(x) for x in s["sizes"]]
    assert sum(sizes) == n and min(sizes) >= 1
    div, cap = grow_div or 16, batch_max or 16384
    begin = 0
    for b, sz in enumerate(sizes):
        allowed = min(cap, max(1, begin // div), n - begin)
        assert sz <= allowed
        assert not any(rz[begin:begin + sz - 1]), "a row inside the batch raises the top level"
        if sz < allowed:
            assert rz[begin + sz - 1], "a batch below its size ends at a row that raises the top level"
        # entry point and top level before the batch: those before row `begin` of the serial order
        assert s["entry_points"][b] == serial["entry_points"][begin] and s["top_levels"][b] == serial["top_levels"][begin]
        begin += sz
    return s


@pytest.mark.parametrize("n,grow_div,batch_max", [(1, 0, 0), (2, 0, 0), (3000, 0, 0), (3000, 4, 0), (3000, 1, 0), (3000, 16, 64), (500, 0, 1),
                                                  (40000, 16, 1000)])
def test_schedule_rules(hs, n, grow_div, batch_max):
    s = check_schedule(hs, n, 8, 100, grow_div, batch_max)
    assert s["entry_points"][0] == NONE and s["top_levels"][0] == -1 and s["sizes"][0] == 1
    if n > 1:
        assert s["entry_points"][1] == 0


def test_schedule_entry_equals_a_serial_build_of_the_prefix(hs, tmp_path):
    """The entry point and top level the schedule reports before a batch are the header of a serial build of the rows before it."""
    base = mixture(400, 8, 3)
    s = hs.build_schedule(400, M=4, seed=100)
    begins = [0] + [int(x) for x in np.cumsum(s["sizes"])[:-1]]
    out = str(tmp_path / "p.bin")
    checked = 0
    for b in list(range(1, 12)) + list(range(12, len(begins), 7)):
        hs.build_hnsw(base[:begins[b]], out, M=4, ef_construction=10, branching_factor="4", seed=100, threads=1)
        maxlevel, ep = struct.unpack_from("<iI", open(out, "rb").read(), 48)
        assert (s["top_levels"][b], s["entry_points"][b]) == (maxlevel, ep), f"batch {b}"
        checked += 1
    assert checked > 12


def test_schedule_when_the_first_rows_raise_the_level_repeatedly(hs):
    found = None
    for seed in range(4000):
        tops = hs.build_schedule(6, M=4, seed=seed, batch_max=1)["top_levels"]
        if tops[1] < tops[2] < tops[3]:
            found = seed
            break
    assert found is not None, "no seed below 4000 raises the level at rows 1 and 2"
    s = check_schedule(hs, 200, 4, found, 1, 0)   # grow_div 1: batches as large as the rule lets them, were it not for the cuts
    assert list(s["sizes"][:3]) == [1, 1, 1] and list(s["entry_points"][:4]) == [NONE, 0, 1, 2]


def test_default_schedule_is_deterministic(hs, tmp_path):
    base = mixture(3000, 32, 11)
    out = str(tmp_path / "o.bin")
    files = []
    for threads in (1, 4, 16, 16):
        st = hs.build_hnsw_batched(base, out, M=8, ef_construction=100, threads=threads)
        assert st["batches"] == len(hs.build_schedule(3000, M=8)["sizes"]) < 3000
        files.append(open(out, "rb").read())
    assert files[0] == files[1] == files[2] == files[3]


@pytest.fixture(scope="module")
def built(hs, tmp_path_factory):
    """mixture(3000, 32, 11) at M 8, efc 100: the default schedule's file and the serial builder's"""
    d = tmp_path_factory.mktemp("built")
    base = mixture(3000, 32, 11)
    bp, sp = str(d / "batched.bin"), str(d / "serial.bin")
    hs.build_hnsw_batched(base, bp, M=8, ef_construction=100, threads=8)
    hs.build_hnsw(base, sp, M=8, ef_construction=100, threads=1)
    return base, bp, sp


def check_structure(raw, dim, n):
    g = parse_hnsw(raw, dim)
    assert g["count"] == n
    level = [len(l) - 1 for l in g["lists"]]
    assert level[g["ep"]] == g["maxlevel"] == max(level)
    for i, per_level in enumerate(g["lists"]):
        for l, ids in enumerate(per_level):
            assert len(ids) <= (g["maxM"] if l else g["maxM0"])
            assert i not in ids, f"self loop at node {i} level {l}"
            assert len(set(map(int, ids))) == len(ids), f"duplicate at node {i} level {l}"
            assert all(level[int(j)] >= l for j in ids), f"node {i} level {l} names a node below that level"
    return g


def test_structure_continuous(hs, oracle, built):
    base, bp, _ = built
    assert oracle.load(bp, "hnsw", L2, 32).count == 3000
    g = check_structure(open(bp, "rb").read(), 32, 3000)
    assert np.array_equal(g["labels"], np.arange(3000, dtype=np.uint64))


def test_structure_integer_rows(hs, oracle, tmp_path):
    base = mixture(3000, 16, 11, integer=True)
    out = str(tmp_path / "i.bin")
    hs.build_hnsw_batched(base, out, M=8, ef_construction=100, threads=8)
    assert oracle.load(out, "hnsw", L2, 16).count == 3000
    check_structure(open(out, "rb").read(), 16, 3000)


def recall(oracle, path, base, q, ef, k=10):
    ix = oracle.load(path, "hnsw", L2, base.shape[1])
    ix.set_ef(ef)
    r = ix.search_pq(q, k)
    gt = oracle.brute_force(L2, base, q, k)
    hits = sum(len(set(map(int, r["labels"][i][:r["cnt"][i]])) & set(map(int, gt[i]))) for i in range(len(q)))
    return hits / (k * len(q))


def test_recall_same_bar_as_the_parallel_builder(hs, oracle, built):
    """The bar of test_parallel_builder_is_searchable at ef 64; at ef 12, where nothing saturates, not more than 0.02 (about three
    standard deviations of a 2000-pair recall estimate near 0.9) below the reference-equal serial graph of the same rows.
    Measured: ef 64 / 50 queries 1.0000; ef 12 / 200 queries 0.8985 batched, 0.8965 serial."""
    base, bp, sp = built
    r64 = recall(oracle, bp, base, mixture(50, 32, 12), 64)
    print(f"recall@10 ef 64: batched {r64:.4f}")
    assert r64 > 0.9
    q = mixture(200, 32, 12)
    rb, rs = recall(oracle, bp, base, q, 12), recall(oracle, sp, base, q, 12)
    print(f"recall@10 ef 12, 200 queries: batched {rb:.4f} serial {rs:.4f}")
    assert rb >= rs - 0.02


def test_labels_are_kept(hs, tmp_path):
    base = mixture(500, 16, 5)
    labels = (np.arange(500, dtype=np.uint64) * 7 + 3)[::-1].copy()
    a, b = str(tmp_path / "a.bin"), str(tmp_path / "b.bin")
    hs.build_hnsw_batched(base, a, M=8, ef_construction=40, threads=4, labels=labels)
    assert np.array_equal(parse_hnsw(open(a, "rb").read(), 16)["labels"], labels)
    hs.build_hnsw_batched(base, b, M=8, ef_construction=40, threads=4, batch_max=1, labels=labels)
    hs.build_hnsw(base, a, M=8, ef_construction=40, threads=1, labels=labels)
    assert open(a, "rb").read() == open(b, "rb").read()


def test_refusals_write_nothing(hs, tmp_path):
    L = hs.lib()
    base = mixture(50, 16, 5)
    out = str(tmp_path / "never.bin")

    def call(base_p=base.ctypes.data, n=50, dim=16, metric=L2, M=8, bf=b"4", opts=None, path=out.encode(), null_opts=False):
        o = opts or hs.HsBatchBuildOpts(-1, 1, 0, 0, 0)
        return L.hs_build_hnsw_batched(base_p, None, n, dim, metric, M, 40, bf, 100, None if null_opts else ctypes.byref(o), path, None)

    assert call() == hs.HS_OK and os.path.exists(out)
    os.remove(out)
    for what, rc in [("null base", call(base_p=None)), ("null path", call(path=None)), ("null branching factor", call(bf=None)),
                     ("null options", call(null_opts=True)), ("n = 0", call(n=0)), ("dim = 0", call(dim=0)), ("metric", call(metric=7)),
                     ("M = 0", call(M=0)), ("device below -1", call(opts=hs.HsBatchBuildOpts(-3, 1, 0, 0, 0))),
                     ("scratch_ids not a power of two", call(opts=hs.HsBatchBuildOpts(-1, 1, 0, 0, 100))),
                     ("scratch_ids below a wavefront", call(opts=hs.HsBatchBuildOpts(-1, 1, 0, 0, 32))),
                     ("grow_div beyond 32 bits", call(opts=hs.HsBatchBuildOpts(-1, 1, 1 << 40, 0, 0))),
                     ("batch_max beyond 32 bits", call(opts=hs.HsBatchBuildOpts(-1, 1, 0, 1 << 40, 0)))]:
        assert rc == hs.HS_ERR_INVALID, what
        assert L.hs_last_error(), what
        assert not os.path.exists(out), what
    nb = ctypes.c_size_t(0)
    assert L.hs_build_schedule(0, 8, b"4", 100, 0, 0, 0, None, None, None, ctypes.byref(nb)) == hs.HS_ERR_INVALID
    assert L.hs_build_schedule(10, 8, b"4", 100, 0, 0, 0, None, None, None, None) == hs.HS_ERR_INVALID
