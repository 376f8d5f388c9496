"""CPU-only tests of the live-update host core: VanillaGraph resume (hs_hnsw_resume) against the compiled reference's index
files, its refusals, and the sanitised stand-alone program csrc/resume_test.cpp."""
import os
import re
import subprocess

import numpy as np
import pytest

from hsutil import GOLDEN, ROOT, load_product

L2, IP = 0, 1
CASES = [("l2_cont_d32", L2), ("l2_int_d16", L2), ("ip_d48", IP), ("l2_cont_d20", L2), ("l2_cont_d21", L2), ("l2_cont_d10", L2),
         ("ip_d20", IP), ("ip_d21", IP), ("ip_d10", IP)]


@pytest.fixture(scope="module")
def hs():
    m = load_product()
    m.build_library()
    return m


def _header(raw):
    """(max_elements, count, maxlevel, enterpoint) of a vanilla index file (hnswalg.h:748-762)."""
    u = np.frombuffer(raw, np.uint64, 6, 0)
    return int(u[1]), int(u[2]), int(np.frombuffer(raw, np.int32, 1, 48)[0]), int(np.frombuffer(raw, np.uint32, 1, 52)[0])


@pytest.mark.parametrize("name,metric", CASES)
def test_resumed_build_writes_reference_bytes(hs, tmp_path, name, metric):
    """build_hnsw of the first n0 rows, then hnsw_resume of the rest with the generator put where that build left it == the
    compiled reference's file of the whole build, byte for byte; n0 = 1 (everything but the first point is resumed), 10 (the top
    level and the enter point move during the resume; degrees cross 16 on the M = 16 graphs) and n / 2."""
    g = np.load(os.path.join(GOLDEN, f"{name}.npz"))
    base, M, efC = g["base"], int(g["M"]), int(g["efC"])
    n, dim = base.shape
    ref = open(os.path.join(GOLDEN, f"{name}.hnsw.bin"), "rb").read()
    for n0 in (1, 10, n // 2):
        part, out = str(tmp_path / f"part{n0}.bin"), str(tmp_path / f"out{n0}.bin")
        hs.build_hnsw(base[:n0], part, metric=metric, M=M, ef_construction=efC, branching_factor="4", seed=100, threads=1)
        hs.hnsw_resume(part, out, base[n0:], np.arange(n0, n), metric=metric, max_elements=n, seed=100, drawn=n0, threads=1)
        assert open(out, "rb").read() == ref, (name, n0)
    # what n0 = 10 is there for: the prefix's top level is below the whole graph's, and its enter point is another node
    _, _, lvl10, ep10 = _header(open(str(tmp_path / "part10.bin"), "rb").read())
    _, _, lvl, ep = _header(ref)
    assert lvl10 < lvl and ep10 != ep and ep >= 10, (name, lvl10, lvl, ep10, ep)


def test_resume_in_several_calls(hs, tmp_path):
    """Two resumes in a row (drawn moves on with the element count) write the one-shot bytes too."""
    g = np.load(os.path.join(GOLDEN, "l2_int_d16.npz"))
    base, M, efC = g["base"], int(g["M"]), int(g["efC"])
    n = base.shape[0]
    a, b, c = (str(tmp_path / f) for f in ("a.bin", "b.bin", "c.bin"))
    hs.build_hnsw(base[:100], a, M=M, ef_construction=efC, branching_factor="4", seed=100, threads=1)
    hs.hnsw_resume(a, b, base[100:250], np.arange(100, 250), max_elements=n, seed=100, drawn=100)
    assert _header(open(b, "rb").read())[:2] == (n, 250)
    hs.hnsw_resume(b, c, base[250:], np.arange(250, n), max_elements=n, seed=100, drawn=250)
    assert open(c, "rb").read() == open(os.path.join(GOLDEN, "l2_int_d16.hnsw.bin"), "rb").read()


def test_resume_refusals_leave_the_input_untouched(hs, tmp_path):
    g = np.load(os.path.join(GOLDEN, "l2_cont_d10.npz"))
    base, M, efC = g["base"], int(g["M"]), int(g["efC"])
    part, out = str(tmp_path / "part.bin"), str(tmp_path / "out.bin")
    hs.build_hnsw(base[:50], part, M=M, ef_construction=efC, branching_factor="4", seed=100, threads=1)
    before = open(part, "rb").read()
    cases = [
        (base[50:53], [50, 51, 50], 60, hs.HS_ERR_INVALID, "appears twice"),           # a label twice in the call
        (base[50:53], [50, 7, 52], 60, hs.HS_ERR_UNSUPPORTED, "already exists"),         # a label the file already holds
        (base[50:61], list(range(50, 61)), 60, hs.HS_ERR_CAPACITY, "The number of elements exceeds the specified limit"),
        (base[50:51], [50], 0, hs.HS_ERR_CAPACITY, "The number of elements exceeds the specified limit"),   # loaded without room
    ]
    for rows, labels, cap, status, text in cases:
        with pytest.raises(hs.HsError) as e:
            hs.hnsw_resume(part, out, rows, labels, max_elements=cap, seed=100, drawn=50)
        assert e.value.status == status and text in str(e.value), (labels, str(e.value))
        assert not os.path.exists(out)
        assert open(part, "rb").read() == before
    hs.hnsw_resume(part, out, base[50:60], np.arange(50, 60), max_elements=60, seed=100, drawn=50)   # exactly full is fine
    assert _header(open(out, "rb").read())[:2] == (60, 60)
    assert open(part, "rb").read() == before


def test_labelled_build_keeps_ids_in_insertion_order(hs, tmp_path):
    """hs_build_hnsw_labeled with labels that are not the row index: internal ids stay the insertion index, the labels are
    stored -- the same file as the unlabelled build except for the label fields."""
    g = np.load(os.path.join(GOLDEN, "l2_cont_d10.npz"))
    base = np.ascontiguousarray(g["base"][:120])
    lab = (np.arange(120, dtype=np.uint64) * 7 + 1000)
    a, b = str(tmp_path / "a.bin"), str(tmp_path / "b.bin")
    hs.build_hnsw(base, a, M=8, ef_construction=40, branching_factor="4")
    hs.build_hnsw(base, b, M=8, ef_construction=40, branching_factor="4", labels=lab)
    ra, rb = bytearray(open(a, "rb").read()), bytearray(open(b, "rb").read())
    assert len(ra) == len(rb)
    spe, loff = int(np.frombuffer(ra, np.uint64, 1, 24)[0]), int(np.frombuffer(ra, np.uint64, 1, 32)[0])
    for i in range(120):
        o = 96 + i * spe + loff
        assert int(np.frombuffer(rb, np.uint64, 1, o)[0]) == int(lab[i]) and int(np.frombuffer(ra, np.uint64, 1, o)[0]) == i
        rb[o:o + 8] = ra[o:o + 8]
    assert ra == rb


def test_sanitised_resume_program():
    """csrc/resume_test.cpp under AddressSanitizer + UBSan, as its own binary (never inside Python)."""
    d = os.path.join(ROOT, "hnsw-slim_amd")
    subprocess.check_call(["make", "-C", d, "resume_test"])
    out = subprocess.run([os.path.join(d, "resume_test")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    m = re.search(r"resume ok: (\d+) bytes compared", out.stdout)
    assert m and int(m.group(1)) > 100_000, out.stdout
