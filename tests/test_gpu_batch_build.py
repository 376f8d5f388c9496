"""Batched addPoint on the GPU (hs_build_hnsw_batched with a device, csrc/build_gpu.hip) against its host twin
(csrc/host_batch_build.hpp): whole files, byte for byte; at batch_max = 1 against the reference-equal serial builder; at the edges
of the device path's envelope and of the fp32 range.  (Against an independent reading: tests/test_gpu_batch_build_restated.py.)"""
import os
import subprocess

import numpy as np
import pytest

import batch_build_cases as C
from hsutil import GOLDEN, ROOT, Oracle, load_product, mixture

pytestmark = pytest.mark.gpu
L2, IP = 0, 1


@pytest.fixture(scope="module")
def hs():
    m = load_product()
    assert m.device_count() > 0, "no HIP device"
    return m


SHAPES = {
    "l2_d32": lambda: (mixture(3000, 32, 11), L2, 8, 100),
    "l2_d64": lambda: (mixture(4000, 64, 11), L2, 16, 200),
    "ip_d48": lambda: (mixture(2000, 48, 11), IP, 8, 100),
    "l2_int_d16": lambda: (mixture(3000, 16, 11, integer=True), L2, 8, 100),
    "l2_d20": lambda: (mixture(1500, 20, 11), L2, 8, 100),     # a dim outside the % 16 recipes
}
_twin = {}


def twin_bytes(hs, tmp_path_factory, name, batch_max):
    """The host twin's file for one shape and schedule, built once for the module."""
    key = (name, batch_max)
    if key not in _twin:
        base, metric, M, efc = SHAPES[name]()
        out = str(tmp_path_factory.mktemp("twin") / "t.bin")
        st = hs.build_hnsw_batched(base, out, metric=metric, M=M, ef_construction=efc, device=-1, threads=16, batch_max=batch_max)
        assert not st["used_gpu"]
        _twin[key] = open(out, "rb").read()
    return _twin[key]


def both(hs, tmp_path, base, **kw):
    """(twin bytes, device bytes, device stats) of one build"""
    t, d = str(tmp_path / "t.bin"), str(tmp_path / "d.bin")
    hs.build_hnsw_batched(base, t, device=-1, threads=8, **{k: v for k, v in kw.items() if k != "scratch_ids"})
    st = hs.build_hnsw_batched(base, d, device=0, **kw)
    return open(t, "rb").read(), open(d, "rb").read(), st


@pytest.mark.parametrize("batch_max", [0, 64])
@pytest.mark.parametrize("name", list(SHAPES))
def test_device_equals_twin(hs, tmp_path, tmp_path_factory, name, batch_max):
    base, metric, M, efc = SHAPES[name]()
    out = str(tmp_path / "d.bin")
    st = hs.build_hnsw_batched(base, out, metric=metric, M=M, ef_construction=efc, device=0, batch_max=batch_max)
    assert st["used_gpu"] and st["batches"] == len(hs.build_schedule(len(base), M=M, batch_max=batch_max)["sizes"])
    assert open(out, "rb").read() == twin_bytes(hs, tmp_path_factory, name, batch_max)


@pytest.mark.parametrize("name", ["l2_cont_d32", "l2_int_d16"])
def test_batch_1_on_the_device_equals_the_reference(hs, tmp_path, name):
    g = np.load(os.path.join(GOLDEN, f"{name}.npz"))
    base = np.ascontiguousarray(g["base"][:600])
    ser, dev = str(tmp_path / "s.bin"), str(tmp_path / "d.bin")
    hs.build_hnsw(base, ser, M=int(g["M"]), ef_construction=int(g["efC"]), branching_factor="4", seed=100, threads=1)
    st = hs.build_hnsw_batched(base, dev, M=int(g["M"]), ef_construction=int(g["efC"]), device=0, batch_max=1)
    assert st["used_gpu"] and st["batches"] == 600
    assert open(dev, "rb").read() == open(ser, "rb").read()


@pytest.mark.parametrize("n", [1, 2, 3, 9, 65])   # 9 = maxM0 + 1 at M 4
def test_tiny_inputs(hs, tmp_path, n):
    base = mixture(n, 16, 3)
    t, d, st = both(hs, tmp_path, base, M=4, ef_construction=20)
    assert st["used_gpu"] and t == d


def test_every_row_the_same_vector(hs, tmp_path):
    base = np.tile(mixture(1, 16, 4), (300, 1))
    t, d, st = both(hs, tmp_path, base, M=4, ef_construction=20)
    assert st["used_gpu"] and t == d


def test_a_batch_into_the_same_few_targets(hs, tmp_path):
    """A spread-out prefix, then rows from one tight cluster: whole batches pick the same few targets, whose lists overflow more
    than once per batch and whose incoming ids outnumber a wavefront (the link kernel's long-segment path)."""
    n = 3000
    sizes = hs.build_schedule(n, M=4)["sizes"]   # (the schedule follows from the levels, not from the rows)
    begins = np.concatenate([[0], np.cumsum(sizes, dtype=np.int64)[:-1]])
    b = int(np.argmax(begins >= 1500))
    prefix = int(begins[b])
    # the cluster begins with a batch: every row of that batch finds row 7 nearest among the rows before it and links to it, so
    # the level-0 list of row 7 (maxM0 = 8) takes more incoming ids than a wavefront has lanes and overflows again and again
    assert sizes[b] > 64 and prefix + sizes[b] <= n
    rng = np.random.default_rng(5)
    spread = mixture(prefix, 16, 6)
    tight = (spread[7] + rng.normal(0, 0.01, (n - prefix, 16))).astype(np.float32)
    base = np.ascontiguousarray(np.concatenate([spread, tight]))
    t, d, st = both(hs, tmp_path, base, M=4, ef_construction=40)
    assert st["used_gpu"] and t == d


def test_rerun_path(hs, tmp_path):
    base, metric, M, efc = SHAPES["l2_d32"]()
    t, d, st = both(hs, tmp_path, base, metric=metric, M=M, ef_construction=efc, scratch_ids=64)
    assert st["used_gpu"] and st["flagged_rows"] > 0
    assert t == d


def test_fallback_above_the_device_cap(hs, tmp_path):
    base = mixture(400, 16, 8)
    t, d, st = both(hs, tmp_path, base, M=32, ef_construction=64)
    assert not st["used_gpu"] and t == d


def test_built_file_loads_and_searches(hs, tmp_path):
    base, q = mixture(3000, 32, 11), mixture(64, 32, 12)
    hp, sp = str(tmp_path / "h.bin"), str(tmp_path / "s.bin")
    st = hs.build_hnsw_batched(base, hp, M=8, ef_construction=100, device=0)
    assert st["used_gpu"]
    O = Oracle()
    hx, ohx = hs.Index(hp, hs.HS_KIND_HNSW, 32), O.load(hp, "hnsw", L2, 32)
    hx.set_ef(64); ohx.set_ef(64)
    g, o = hx.search_pq(q, 10), ohx.search_pq(q, 10)
    assert np.array_equal(np.sort(g["labels"], axis=1), np.sort(o["labels"], axis=1))
    hs.convert_slim(hp, sp, 32, threads=8)
    ix, ox = hs.Index(sp, hs.HS_KIND_SLIM, 32), O.load(sp, "slim", L2, 32)
    ix.set_ef(64); ox.set_ef(64)
    want = ox.search_ids(q, 10)
    assert np.array_equal(np.sort(ix.search_ids(q, 10)["labels"], axis=1), np.sort(want["labels"], axis=1))
    ix.set_exact_order(True)
    assert np.array_equal(ix.search_ids(q, 10)["labels"], want["labels"])


def test_facade_build(hs, tmp_path):
    """tests/facade_build.cpp: setBuildOnDevice(0, 1) before the first search returns the labels of a run without it."""
    exe = os.path.join(ROOT, "hnsw-slim_amd", "facade_build")
    base, q = mixture(800, 32, 11), mixture(40, 32, 12)
    rf, qf = str(tmp_path / "rows.f32"), str(tmp_path / "q.f32")
    base.tofile(rf); q.tofile(qf)
    outs, saved = [], []
    for device in ("0", "-1"):
        out, sav = str(tmp_path / f"out{device}.bin"), str(tmp_path / f"saved{device}.bin")
        run = subprocess.run([exe, rf, "800", "32", "8", "100", device, "1", qf, "40", "10", out, sav], capture_output=True, text=True)
        assert run.returncode == 0, run.stdout + run.stderr
        if device == "0":
            assert run.stdout.split()[:3] == ["build:", "1", "800"], run.stdout
        outs.append(open(out, "rb").read()); saved.append(open(sav, "rb").read())
    assert outs[0] == outs[1] and saved[0] == saved[1]
    labels = np.frombuffer(outs[0], np.uint64, 40 * 10).reshape(40, 10)
    assert labels.min() >= 1000 and labels.max() < 1800


# ---- the edges of the device path's envelope, and of the fp32 range (device against twin: these need fp32 rows) -------------------------
def device_supported(dim, M, efc, scratch_ids=0):
    """gpu_build_supported of csrc/build_gpu.hip, restated from its text: M <= kBgMaxM = 31, max(efc, M) <= kBgMaxEfc = 512, and the LDS
    of one row -- bg_search_lds = 8 dpad + 8 topcap + 5 * 256 + 12 scratch_ids with dpad = dim rounded up to 4 and topcap the power of
    two (64 at least) that holds efc + 1 entries; bg_link_lds = 8 dpad + 64 * 8 + 7 * 256 -- within kBgLdsLimit = 160 KiB."""
    s, e = scratch_ids or 4096, max(efc, M)
    if M == 0 or M > 31 or e > 512:
        return False
    dpad, topcap = (dim + 3) // 4 * 4, 64
    while topcap < e + 1:
        topcap *= 2
    return 8 * dpad + 8 * topcap + 5 * 256 + 12 * s <= 160 * 1024 and 8 * dpad + 64 * 8 + 7 * 256 <= 160 * 1024


# The LDS limit: at scratch_ids = 8192 (98304 bytes) and ef_construction = 100 (topcap 128: 1024 bytes) bg_search_lds is
# 8 dpad + 100608, which is 160 KiB = 163840 exactly at dpad = 7904 and above it at the next dpad, 7908.
LDS_EDGE_DIM = 7904
ENVELOPE = {
    "M31_efc512": (lambda: mixture(1500, 32, 11), dict(M=31, ef_construction=512), True),
    "M31_efc31": (lambda: mixture(1500, 32, 11), dict(M=31, ef_construction=31), True),
    "M2": (lambda: mixture(1000, 16, 11), dict(M=2, ef_construction=10), True),
    "dim1": (lambda: mixture(600, 1, 11), dict(M=8, ef_construction=40), True),
    "dim3": (lambda: mixture(600, 3, 11), dict(M=8, ef_construction=40), True),
    "dim23": (lambda: mixture(600, 23, 11), dict(M=8, ef_construction=40), True),
    "dim960": (lambda: mixture(600, 960, 11), dict(M=8, ef_construction=40), True),
    "scratch8192": (lambda: mixture(1000, 32, 11), dict(M=8, ef_construction=100, scratch_ids=8192), True),
    "lds_at_the_limit": (lambda: mixture(200, LDS_EDGE_DIM, 11), dict(M=8, ef_construction=100, scratch_ids=8192), True),
    "lds_above_the_limit": (lambda: mixture(200, LDS_EDGE_DIM + 4, 11), dict(M=8, ef_construction=100, scratch_ids=8192), False),
    "M32": (lambda: mixture(400, 16, 8), dict(M=32, ef_construction=64), False),
    "efc513": (lambda: mixture(600, 16, 8), dict(M=8, ef_construction=513), False),
}


@pytest.mark.parametrize("name", list(ENVELOPE))
def test_envelope(hs, tmp_path, name):
    make, kw, on_device = ENVELOPE[name]
    base = make()
    assert device_supported(base.shape[1], kw["M"], kw["ef_construction"], kw.get("scratch_ids", 0)) == on_device
    t, d, st = both(hs, tmp_path, base, **kw)
    assert bool(st["used_gpu"]) == on_device
    assert t == d


@pytest.mark.parametrize("batch_max", [0, 64])
@pytest.mark.parametrize("case", C.vr_cases(), ids=C.vr_name)
def test_value_range(hs, oracle, tmp_path, case, batch_max):
    """The families of tests/value_range.py as a build meets them: distances above 2^100, subnormal, all equal, of both signs,
    +inf.  600 rows at M 8, ef_construction 60; the family's premise holds on the rows' own distance table (asserted)."""
    rows = C.vr_rows(case)
    C.vr_check_premise(oracle, case, rows)
    t, d, st = both(hs, tmp_path, rows, metric=case[1], M=C.VR_M, ef_construction=C.VR_EFC, batch_max=batch_max)
    assert st["used_gpu"] and t == d
