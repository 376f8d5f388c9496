"""The host twin of the batched addPoint (hs_build_hnsw_batched with device = -1, hs_hnsw_resume_batched, hs_build_schedule) against
the plain-Python reading of DESIGN.md 4m / 4n (tests/batch_build_restated.py): whole files, byte for byte.  The reading is first
anchored to the compiled reference at batch_max = 1; the levels of every case come from the serial builder's file, never from the
file under test.  Every test prints how many comparisons of equal keys the reading's heaps made."""
import os

import numpy as np
import pytest

import batch_build_cases as C
import batch_build_restated as R
import value_range as vr
from hsutil import GOLDEN, load_product

L2, IP = 0, 1
SEED = C.SEED


@pytest.fixture(scope="module")
def hs():
    m = load_product()
    m.build_library()
    return m


def test_reading_writes_the_reference_file_at_batch_1():
    """batch_max = 1 is the reference's serial loop: the tie-heavy golden file written by the compiled reference, every word of it,
    stale tails included.  (The levels are the golden file's own here: it IS the reference.)"""
    g = np.load(os.path.join(GOLDEN, "l2_int_d16.npz"))
    want = C.read(os.path.join(GOLDEN, "l2_int_d16.hnsw.bin"))
    assert R.exact_range(g["base"], L2) < R.EXACT
    got, st = R.build(g["base"], R.levels_of(want), L2, int(g["M"]), int(g["efC"]), batch_max=1)
    print(st)
    assert st["batches"] == len(g["base"]) and st["ties"] > 10000 and st["stale_words"] > 0
    assert got == want


def test_reading_equals_the_serial_builder_on_integer_ip_rows(hs, tmp_path):
    """The goldens hold no integer-valued IP fixture (ip_d10 / d20 / d21 / d48 are continuous: asserted), so: integer rows of both
    signs, the reading at batch_max = 1 against hs.build_hnsw(threads=1), which the compiled reference pins on those fixtures."""
    for name in ("ip_d10", "ip_d20", "ip_d21", "ip_d48"):
        b = np.load(os.path.join(GOLDEN, f"{name}.npz"))["base"]
        assert not np.array_equal(b, np.rint(b)), f"{name} is integer-valued: anchor the reading to its golden file instead"
    rows = C.signed_rows(1200)
    assert R.exact_range(rows, IP) < R.EXACT
    p = str(tmp_path / "s.bin")
    hs.build_hnsw(rows, p, metric=IP, M=8, ef_construction=100, seed=SEED, threads=1)
    want = C.read(p)
    got, st = R.build(rows, R.levels_of(want), IP, 8, 100, batch_max=1)
    print(st)
    assert st["ties"] > 0
    assert got == want


@pytest.mark.parametrize("name", list(C.CASES))
def test_twin_equals_reading(hs, tmp_path, tmp_path_factory, name):
    _, metric, M, efc, kw = C.CASES[name]
    rows, levels, want, st = C.reading(hs, tmp_path_factory.mktemp("reading"), name)
    out = str(tmp_path / "twin.bin")
    tw = hs.build_hnsw_batched(rows, out, metric=metric, M=M, ef_construction=efc, seed=SEED, device=-1, threads=8, **kw)
    got = C.read(out)
    print(f"{name}: ties {st['ties']}, stale words {st['stale_words']}, most incoming ids {st['max_incoming']}, batches {st['batches']}")
    assert not tw["used_gpu"] and tw["batches"] == st["batches"]
    assert R.levels_of(got) == levels
    assert got == want


def resume_base(hs, folder):
    rows, levels, whole, _ = C.reading(hs, folder, "default")
    sched = R.schedule(levels)
    return rows, levels, whole, sched


@pytest.mark.parametrize("cut", ["boundary", "inside", "raises"])
def test_resume_equals_reading(hs, tmp_path, tmp_path_factory, cut):
    """hs_hnsw_resume_batched against the reading continued from the same prefix file (the twin's build of the prefix, itself held
    to the reading above).  Cut at a batch boundary the result is also the whole build's file (4n, point 2)."""
    rows, levels, whole, sched = resume_base(hs, tmp_path_factory.mktemp("reading"))
    n = len(rows)
    n0 = C.resume_cuts(levels, sched)[cut]
    assert 0 < n0 < n
    part, out = str(tmp_path / "part.bin"), str(tmp_path / "out.bin")
    hs.build_hnsw_batched(rows[:n0], part, M=8, ef_construction=100, seed=SEED, device=-1, threads=8)
    prefix = C.read(part)
    assert R.levels_of(prefix) == levels[:n0]
    labels = np.arange(n0, n) * 3 + 5000
    tw = hs.hnsw_resume_batched(part, out, rows[n0:], labels, max_elements=n, seed=SEED, drawn=n0, threads=8)
    want, st = R.resume(prefix, 16, rows[n0:], levels[n0:], labels, L2, max_elements=n)
    print(f"{cut} at {n0}: {st}")
    got = C.read(out)
    assert R.levels_of(got) == levels and tw["batches"] == st["batches"]
    assert got == want
    if cut == "raises":
        assert max(levels[n0:]) > max(levels[:n0])
    if cut == "boundary":
        again, _ = R.resume(prefix, 16, rows[n0:], levels[n0:], np.arange(n0, n), L2, max_elements=n)
        assert again == whole


@pytest.fixture(scope="module")
def levels_40000(hs, tmp_path_factory):
    """The levels of 40000 rows at M 8, seed 100, from the serial builder's file (levels are drawn in row order: a prefix of them
    is the levels of a shorter build)."""
    rows = np.random.default_rng(1).integers(0, 50, (40000, 2)).astype(np.float32)
    return C.serial_levels(hs, tmp_path_factory.mktemp("levels"), rows, L2, 8, 8)


@pytest.mark.parametrize("n,grow_div,batch_max", [(1, 0, 0), (2, 0, 0), (3000, 0, 0), (3000, 4, 0), (3000, 1, 0), (3000, 16, 64), (500, 0, 1),
                                                  (40000, 16, 1000)])
def test_schedule_equals_reading(hs, levels_40000, n, grow_div, batch_max):
    """hs_build_schedule against the reading's schedule (rule 2 of 4m) for the parameter rows of test_schedule_rules."""
    s = hs.build_schedule(n, M=8, seed=SEED, grow_div=grow_div, batch_max=batch_max)
    mine = R.schedule(levels_40000[:n], grow_div=grow_div, batch_max=batch_max)
    assert [int(x) for x in s["sizes"]] == [sz for _, sz, _, _ in mine]
    assert [int(x) for x in s["entry_points"]] == [ep for _, _, ep, _ in mine]
    assert [int(x) for x in s["top_levels"]] == [top for _, _, _, top in mine]


@pytest.mark.parametrize("case", C.vr_cases(), ids=C.vr_name)
def test_twin_at_batch_1_equals_the_serial_builder_at_the_edges_of_fp32(hs, oracle, tmp_path, case):
    """The value-range families (large, subnormal, all-equal, both signs, +inf keys) need fp32 rows, which the reading cannot take:
    here the twin's arithmetic at batch_max = 1 is tied to the serial builder, which the compiled reference pins."""
    _, metric, _, _ = case
    rows = C.vr_rows(case)
    C.vr_check_premise(oracle, case, rows)
    a, b = str(tmp_path / "a.bin"), str(tmp_path / "b.bin")
    hs.build_hnsw(rows, a, metric=metric, M=C.VR_M, ef_construction=C.VR_EFC, seed=SEED, threads=1)
    st = hs.build_hnsw_batched(rows, b, metric=metric, M=C.VR_M, ef_construction=C.VR_EFC, seed=SEED, device=-1, threads=4, batch_max=1)
    assert st["batches"] == len(rows)
    assert C.read(a) == C.read(b)
