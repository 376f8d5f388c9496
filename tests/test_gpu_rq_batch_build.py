"""The batched build of HNSW-SlimQ's base graph on the GPU (hs_build_rabitq_hnsw_batched with a device, the BgRabitq flavour of the
kernels of csrc/build_gpu.hip): the distance alone against the host recipe, bit for bit; whole files against the host twin
(csrc/host_rq_batch_build.hpp); at batch_max = 1 the compiled rabitqlib's edges; against the plain-Python reading of
tests/rq_batch_build_restated.py, never through the twin; outside the device envelope; the facade's build chain."""
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

pytestmark = pytest.mark.gpu
L2, IP = 0, 1


@pytest.fixture(scope="module")
def hs():
    m = load_product()
    assert m.device_count() > 0, "no HIP device"
    return m


# ---- the distance alone ---------------------------------------------------------------------------------------------------------------
DIMS = [1, 3, 15, 16, 17, 31, 32, 48, 63, 64, 65, 80, 112, 128, 130, 768, 960]


def same_bits(hs, a, b, metric):
    host, dev = hs.rq_raw_dist(a, b, metric, device=-1), hs.rq_raw_dist(a, b, metric, device=0)
    assert not np.isnan(host).any(), "NaN is outside the definition: the pair order is not total with it"
    assert np.array_equal(host.view(np.uint32), dev.view(np.uint32)), f"{int((host.view(np.uint32) != dev.view(np.uint32)).sum())} of {len(host)} pairs differ"
    return host


@pytest.mark.parametrize("metric", [L2, IP], ids=["l2", "ip"])
@pytest.mark.parametrize("dim", DIMS)
def test_distance_bits(hs, dim, metric):
    rng = np.random.default_rng(1000 + dim)
    a, b = rng.standard_normal((300, dim)).astype(np.float32), rng.standard_normal((300, dim)).astype(np.float32)
    b[:20] = a[:20]                                     # equal rows
    d = same_bits(hs, a, b, metric)
    assert len(set(d.tolist())) > 200
    ai, bi = rng.integers(-9, 10, (300, dim)).astype(np.float32), rng.integers(-9, 10, (300, dim)).astype(np.float32)
    same_bits(hs, ai, bi, metric)                       # integer rows: plenty of equal distances


@pytest.mark.parametrize("dim", [15, 16, 65, 130, 768])
def test_distance_bits_at_the_edges_of_fp32(hs, dim):
    rng = np.random.default_rng(2000 + dim)
    a, b = rng.standard_normal((200, dim)).astype(np.float32), rng.standard_normal((200, dim)).astype(np.float32)
    big = same_bits(hs, a * np.float32(1e20), b * np.float32(1e20), L2)            # squares overflow
    assert np.isinf(big).all() and (big > 0).all()
    tiny = same_bits(hs, a * np.float32(1e-21), b * np.float32(1e-21), L2)         # subnormal squares
    assert (tiny < np.finfo(np.float32).tiny).all() and (tiny > 0).any()
    tip = same_bits(hs, a * np.float32(1e-21), b * np.float32(1e-21), IP)          # subnormal products under the 1 - x
    assert (tip == 1).all()
    same_bits(hs, a * np.float32(1e15), b * np.float32(1e15), IP)                  # large finite products of both signs
    mid = same_bits(hs, a * np.float32(1e-19), b * np.float32(1e-21), IP)          # products around 1e-40
    assert (mid == 1).all()
    row = np.full((50, dim), np.float32(3.25))
    assert (same_bits(hs, row, row.copy(), L2) == 0).all()                         # all-equal rows
    same_bits(hs, row, row.copy(), IP)


# ---- device == twin, whole files -------------------------------------------------------------------------------------------------------
SHAPES = {c[0]: (lambda c=c: (rq_hnsw_base(c[1], c[2], c[3], c[6]), dict(metric=c[3], M=c[4], ef_construction=c[5]))) for c in RQ_HNSW_CASES}
SHAPES.update({
    "d8": lambda: (mixture(600, 8, 11), dict(M=8, ef_construction=40)),
    "d48": lambda: (mixture(600, 48, 11), dict(M=8, ef_construction=40)),
    "d80_ip": lambda: (mixture(600, 80, 11), dict(metric=IP, M=8, ef_construction=40)),
    "d768_m32": lambda: (mixture(400, 768, 11), dict(M=32, ef_construction=128)),
    "rerun": lambda: (mixture(1500, 32, 11), dict(M=8, ef_construction=100, scratch_ids=64)),
    "scratch8192": lambda: (mixture(1000, 32, 11), dict(M=8, ef_construction=100, scratch_ids=8192)),
    "M2": lambda: (mixture(1000, 16, 11), dict(M=2, ef_construction=10)),
    "efc512": lambda: (mixture(1200, 32, 11), dict(M=16, ef_construction=512)),
    "efc_M_32": lambda: (mixture(800, 32, 11), dict(M=32, ef_construction=32)),
    "hub_m32": lambda: (C.hub_rows(), dict(M=32, ef_construction=128)),
    "small_batches": lambda: (mixture(1500, 32, 11, integer=True), dict(M=8, ef_construction=60, batch_max=64, grow_div=1)),
})


def both(hs, tmp_path, base, **kw):
    """(twin bytes, device bytes, device stats) of one build"""
    t, d = str(tmp_path / "t.bin"), str(tmp_path / "d.bin")
    tw = hs.build_rabitq_hnsw_batched(base, t, device=-1, threads=16, **{k: v for k, v in kw.items() if k != "scratch_ids"})
    st = hs.build_rabitq_hnsw_batched(base, d, device=0, **kw)
    assert not tw["used_gpu"] and tw["batches"] == st["batches"]
    return C.read(t), C.read(d), st


@pytest.mark.parametrize("name", list(SHAPES))
def test_device_equals_twin(hs, tmp_path, name):
    base, kw = SHAPES[name]()
    t, d, st = both(hs, tmp_path, base, **kw)
    print(name, st)
    assert st["used_gpu"]
    assert (st["flagged_rows"] > 0) == (name == "rerun")
    if name in ("hub_m32", "l2_d112_m32", "d768_m32"):
        g = load_chal_encode().parse_vanilla(d)
        most = max(len(l[0]) for l in g["lists"])
        print(name, "longest level-0 list", most)
        if name == "hub_m32":
            assert most == 64, "no level-0 list reached 2 M ids: the 65-candidate link path did not run"
    assert t == d


def test_twice_in_a_row(hs, tmp_path):
    base, kw = SHAPES["l2_d100"]()
    a, b = str(tmp_path / "a.bin"), str(tmp_path / "b.bin")
    assert hs.build_rabitq_hnsw_batched(base, a, device=0, **kw)["used_gpu"]
    assert hs.build_rabitq_hnsw_batched(base, b, device=0, **kw)["used_gpu"]
    assert C.read(a) == C.read(b)


@pytest.mark.parametrize("scratch_ids", [0, 8192], ids=["default", "scratch8192"])
def test_both_builders_in_one_process(hs, tmp_path, scratch_ids):
    """The two builders are instantiations of the same two kernels: hnswlib's build, rabitqlib's, hnswlib's again and a batched add
    onto the first file, one after the other on one device, each against its host twin.  At scratch_ids = 8192 the on-chip search
    kernel of either builder asks for more than 64 KiB of LDS, so each instantiation sets its own function attribute."""
    base, extra = mixture(600, 32, 11), mixture(200, 32, 12)
    kw = dict(M=8, ef_construction=40)
    p = {k: str(tmp_path / f"{k}.bin") for k in ("h1", "h1_twin", "rq", "rq_twin", "h2", "add_twin")}
    assert hs.build_hnsw_batched(base, p["h1"], device=0, scratch_ids=scratch_ids, **kw)["used_gpu"]
    assert hs.build_rabitq_hnsw_batched(base, p["rq"], device=0, scratch_ids=scratch_ids, **kw)["used_gpu"]
    assert hs.build_hnsw_batched(base, p["h2"], device=0, scratch_ids=scratch_ids, **kw)["used_gpu"]
    ix = hs.Index(p["h1"], hs.HS_KIND_HNSW, 32, max_elements=800)
    ix.seed_levels(100, 600)
    assert ix.add_points_batched(extra, np.arange(600, 800), device=0, scratch_ids=scratch_ids)["used_gpu"]
    added = str(tmp_path / "added.bin")
    ix.save(added)
    hs.build_hnsw_batched(base, p["h1_twin"], device=-1, threads=16, **kw)
    hs.build_rabitq_hnsw_batched(base, p["rq_twin"], device=-1, threads=16, **kw)
    hs.hnsw_resume_batched(p["h1"], p["add_twin"], extra, np.arange(600, 800), max_elements=800, seed=100, drawn=600, threads=16)
    assert C.read(p["h1"]) == C.read(p["h1_twin"])
    assert C.read(p["rq"]) == C.read(p["rq_twin"])
    assert C.read(p["h2"]) == C.read(p["h1"])
    assert C.read(added) == C.read(p["add_twin"])


@pytest.mark.parametrize("name", ["l2_d64", "l2_d112_m32"])
def test_batch_1_on_the_device_writes_the_compiled_rabitqlibs_edges(hs, tmp_path, name):
    _, n, d, metric, M, efc, integer = next(c for c in RQ_HNSW_CASES if c[0] == name)
    ref = np.load(os.path.join(GOLDEN, "rabitq_hnsw_ref.npz"))
    base = rq_hnsw_base(n, d, metric, integer)
    assert float(base.astype(np.float64).sum()) == float(ref[name + "_rowsum"]), "regenerated rows differ from the fixture's"
    out = str(tmp_path / "d.bin")
    st = hs.build_rabitq_hnsw_batched(base, out, metric=metric, M=M, ef_construction=efc, seed=100, device=0, batch_max=1)
    assert st["used_gpu"] and st["batches"] == n
    g = load_chal_encode().parse_vanilla(C.read(out))
    flat = [g["maxlevel"], g["enterpoint"]]
    for i in range(g["count"]):
        flat += [int(g["labels"][i]), len(g["lists"][i]) - 1]
        for l in g["lists"][i]:
            flat.append(len(l))
            flat += [int(x) for x in l]
    got = np.array(flat, np.uint32)
    assert got.shape == ref[name].shape and np.array_equal(got, ref[name])


# ---- device == the Python reading, never through the twin ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(C.GPU_CASES) + ["default_rerun"])
def test_device_equals_reading(hs, tmp_path, tmp_path_factory, name):
    case = "default" if name == "default_rerun" else name
    _, metric, M, efc, kw = C.CASES[case]
    rows, levels, want, st = C.reading(hs, tmp_path_factory.mktemp("reading"), case)
    out = str(tmp_path / "d.bin")
    extra = dict(scratch_ids=64) if name == "default_rerun" else {}
    dv = hs.build_rabitq_hnsw_batched(rows, out, metric=metric, M=M, ef_construction=efc, seed=C.SEED, device=0, **kw, **extra)
    print(name, dv, st)
    assert dv["used_gpu"] and dv["batches"] == st["batches"]
    assert (dv["flagged_rows"] > 0) == (name == "default_rerun")
    assert C.read(out) == want


# ---- outside the envelope ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,efc", [(33, 100), (8, 513)])
def test_outside_the_envelope_builds_on_the_twin(hs, tmp_path, M, efc):
    base = mixture(400, 16, 8)
    t, d, st = both(hs, tmp_path, base, M=M, ef_construction=efc)
    assert not st["used_gpu"] and st["flagged_rows"] == 0 and st["kernel_ms"] == 0
    assert t == d


# ---- the facade ---------------------------------------------------------------------------------------------------------------------------
def test_facade_rq_build(hs, tmp_path):
    """tests/facade_rq_build.cpp: construct (on the device) -> save -> convertFromHNSW -> saveIndex -> setDataset -> searchKnn.  The saved
    graph is the C ABI's, the labels are those of hs_slimq_search_batch on the converted file the program saved."""
    exe = os.path.join(ROOT, "hnsw-slim_amd", "facade_rq_build")
    n, d, M, efc, nq, k, ef = 800, 64, 32, 128, 40, 10, 64
    base, q = mixture(n, d, 11), mixture(nq, d, 12)
    cen = np.ascontiguousarray(base[:16])
    rf, cf, qf = (str(tmp_path / x) for x in ("rows.f32", "cen.f32", "q.f32"))
    base.tofile(rf); cen.tofile(cf); q.tofile(qf)
    out, hp, qp, mine = (str(tmp_path / x) for x in ("out.bin", "hnsw.bin", "slimq.bin", "capi.bin"))
    run = subprocess.run([exe, rf, str(n), str(d), str(M), str(efc), "0", "0", cf, "16", qf, str(nq), str(k), str(ef), out, hp, qp],
                         capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    st = hs.build_rabitq_hnsw_batched(base, mine, M=M, ef_construction=efc, seed=100, device=0)
    assert st["used_gpu"]
    assert run.stdout.split()[:3] == ["build:", "1", str(st["batches"])], run.stdout
    assert C.read(hp) == C.read(mine)
    qx = hs.Index(qp, hs.HS_KIND_SLIMQ, d)
    qx.slimq_set_dataset(base)
    qx.set_ef(ef)
    want = qx.slimq_search(q, k)["labels"]
    got = np.frombuffer(C.read(out), np.uint32).reshape(nq, k)
    assert np.array_equal(got.astype(np.int64), np.asarray(want).astype(np.int64))
    assert got.max() < n
