"""CPU-only tests of the update path of the live-update host core: hs_hnsw_replay (updatePoint, addPoint with replace_deleted,
markDelete / unmarkDelete, resizeIndex on VanillaGraph) against the compiled reference's files and search results in
tests/golden/updates_*.npz, its refusals, and the sanitised stand-alone program csrc/upsert_test.cpp."""
import os
import re
import subprocess

import numpy as np
import pytest

from hsutil import GOLDEN, ROOT, load_product

L2 = 0
ADD, MARK, UNMARK, RESIZE = 0, 1, 2, 3
GRAPHS = [("l2_cont_d32", 32), ("l2_int_d16", 16)]
SCENARIOS = ["update", "replace", "resize"]


@pytest.fixture(scope="module")
def hs():
    m = load_product()
    m.build_library()
    return m


def _fixture(name, scenario):
    return np.load(os.path.join(GOLDEN, f"updates_{scenario}_{name}.npz"))


def _header(raw):
    """(max_elements, count) of a vanilla index file (hnswalg.h:748-762)."""
    u = np.frombuffer(raw, np.uint64, 3, 0)
    return int(u[1]), int(u[2])


def _pq_sorted(d, l, c):
    return [sorted(zip(d[i, :int(c[i])].view(np.uint32).tolist(), l[i, :int(c[i])].tolist())) for i in range(len(c))]


@pytest.mark.parametrize("scenario", SCENARIOS)
@pytest.mark.parametrize("name,dim", GRAPHS)
def test_replay_writes_reference_bytes(hs, oracle, tmp_path, name, dim, scenario):
    """hs_hnsw_replay of the fixture's operations == the compiled reference's saved file, byte for byte -- in one call, and split
    over several calls, each of which loads the previous call's file -- and the oracle's search on the replayed file gives the
    reference's results after the operations."""
    f = _fixture(name, scenario)
    src, out = os.path.join(GOLDEN, f"{name}.hnsw.bin"), str(tmp_path / "out.bin")
    ops, rows, cap, allow = f["ops"], f["rows"], int(f["max_elements"]), bool(f["allow"])
    want = f["saved"].tobytes()
    hs.hnsw_replay(src, out, ops, rows, dim, max_elements=cap, allow_replace_deleted=allow)
    assert open(out, "rb").read() == want
    # what the scenario is there for
    n = _header(open(src, "rb").read())[1]
    adds = ops[ops[:, 0] == ADD]
    if scenario == "update":
        marked = ops[ops[:, 0] == MARK][:, 1]
        assert len(adds) >= 40 and (adds[:, 1] < n).all() and np.isin(marked, adds[:, 1]).all() and len(marked) == 2
        assert int(np.frombuffer(want, np.uint32, 1, 52)[0]) in adds[:, 1]            # the enter point among the updated labels
        assert _header(want) == (cap, n)
    elif scenario == "replace":
        assert (adds[:, 2] == 1).all() and len(adds) == 40 and _header(want) == (cap, n + 10)
    else:
        assert int(ops[0, 0]) == RESIZE and _header(want) == (n + 50, n + 50)
    # split over several calls
    # (a call starts with loadIndex: deleted_elements is filled from the file's marks in increasing id -- not the order the marks
    # were set in -- and the level generator starts afresh, in the reference as here.  So the replace scenario is cut where no mark
    # is set, once its 30 vacancies are refilled, and no scenario is cut between two appends.)
    cuts = {"update": [0, 2, 20, len(ops)], "replace": [0, 60, len(ops) - 2, len(ops)], "resize": [0, 1, 51, 53, len(ops)]}[scenario]
    cur = src
    for i, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
        nxt = str(tmp_path / f"step{i}.bin")
        hs.hnsw_replay(cur, nxt, ops[a:b], rows, dim, max_elements=cap if cur == src else 0, allow_replace_deleted=allow)
        cur = nxt
    assert open(cur, "rb").read() == want
    # the oracle on the replayed file answers as the reference answered after its own operations
    q, k = np.load(os.path.join(GOLDEN, f"{name}.npz"))["queries"], int(f["k"])
    ox = oracle.load(out, "hnsw", L2, dim)
    for ef in f["efs"]:
        ef = int(ef)
        ox.set_ef(ef)
        o = ox.search_pq(q, k)
        assert np.array_equal(o["cnt"], f[f"ef{ef}_cnt"])
        assert _pq_sorted(o["dists"], o["labels"], o["cnt"]) == _pq_sorted(f[f"ef{ef}_dists"], f[f"ef{ef}_labels"], f[f"ef{ef}_cnt"])


def test_replay_refusals_write_nothing(hs, tmp_path):
    g = np.load(os.path.join(GOLDEN, "l2_int_d16.npz"))
    base = g["base"]
    n = base.shape[0]
    src, out = os.path.join(GOLDEN, "l2_int_d16.hnsw.bin"), str(tmp_path / "out.bin")
    before = open(src, "rb").read()
    rows = np.ascontiguousarray(base[:4] + 1)
    limit = "The number of elements exceeds the specified limit"
    cases = [   # (ops, max_elements, allow_replace_deleted, status, text)
        ([(ADD, 7, 1, 0)], n + 2, False, hs.HS_ERR_INVALID, "Replacement of deleted elements is disabled in constructor"),
        ([(MARK, 7, 0, 0), (ADD, 7, 0, 0)], n + 2, True, hs.HS_ERR_INVALID,
         "Can't use addPoint to update deleted elements if replacement of deleted elements is enabled."),
        ([(ADD, n, 0, 0), (ADD, n + 1, 0, 1), (ADD, n + 2, 0, 2)], n + 2, False, hs.HS_ERR_CAPACITY, limit),
        ([(ADD, n, 0, 0)], 0, False, hs.HS_ERR_CAPACITY, limit),                                  # loaded without room
        ([(MARK, 7, 0, 0), (ADD, n, 1, 0), (ADD, n + 1, 1, 1)], 0, True, hs.HS_ERR_CAPACITY, limit),   # one vacancy, no room
        ([(RESIZE, n - 1, 0, 0)], 0, False, hs.HS_ERR_INVALID, "Cannot resize, max element is less than the current number of elements"),
        ([(MARK, n + 99, 0, 0)], 0, False, hs.HS_ERR_INVALID, "Label not found"),
        ([(MARK, 7, 0, 0), (MARK, 7, 0, 0)], 0, False, hs.HS_ERR_INVALID, "The requested to delete element is already deleted"),
        ([(UNMARK, 7, 0, 0)], 0, False, hs.HS_ERR_INVALID, "The requested to undelete element is not deleted"),
        ([(9, 7, 0, 0)], 0, False, hs.HS_ERR_INVALID, "bad operation kind 9"),
    ]
    for ops, cap, allow, status, text in cases:
        with pytest.raises(hs.HsError) as e:
            hs.hnsw_replay(src, out, ops, rows, 16, max_elements=cap, allow_replace_deleted=allow)
        assert e.value.status == status and str(e.value) == text, (ops, str(e.value))
        assert not os.path.exists(out)
    with pytest.raises(hs.HsError) as e:
        hs.hnsw_replay(src, out, [(ADD, 7, 0, 4)], rows, 16)      # a row the caller did not pass
    assert e.value.status == hs.HS_ERR_INVALID and not os.path.exists(out)
    # the accepted neighbours of the refused lists: an update without replacement un-marks; a full index takes a replacement
    hs.hnsw_replay(src, out, [(MARK, 7, 0, 0), (ADD, 7, 0, 0)], rows, 16)
    raw = open(out, "rb").read()
    spe = int(np.frombuffer(raw, np.uint64, 1, 24)[0])
    assert raw[96 + 7 * spe + 2] & 1 == 0 and raw[96 + 7 * spe + 68:96 + 7 * spe + 132] == rows[0].tobytes()
    hs.hnsw_replay(src, out, [(MARK, 7, 0, 0), (ADD, n + 5, 1, 1)], rows, 16, allow_replace_deleted=True)
    raw = open(out, "rb").read()
    assert _header(raw) == (n, n) and int(np.frombuffer(raw, np.uint64, 1, 96 + 7 * spe + 132)[0]) == n + 5
    assert raw[96 + 7 * spe + 2] & 1 == 0 and raw[96 + 7 * spe + 68:96 + 7 * spe + 132] == rows[1].tobytes()
    assert open(src, "rb").read() == before


@pytest.mark.parametrize("name,dim", GRAPHS)
def test_sanitised_upsert_program(tmp_path, name, dim):
    """csrc/upsert_test.cpp under AddressSanitizer + UBSan, as its own binary (never inside Python): the replace scenario through
    the host code, against the compiled reference's file."""
    d = os.path.join(ROOT, "hnsw-slim_amd")
    subprocess.check_call(["make", "-C", d, "upsert_test"])
    f = _fixture(name, "replace")
    of, rf, wf = (str(tmp_path / x) for x in ("ops.u64", "rows.f32", "want.bin"))
    f["ops"].tofile(of)
    f["rows"].tofile(rf)
    f["saved"].tofile(wf)
    out = subprocess.run([os.path.join(d, "upsert_test"), os.path.join(GOLDEN, f"{name}.hnsw.bin"), "0", str(dim), str(int(f["max_elements"])),
                          str(int(f["allow"])), of, rf, wf], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    m = re.search(r"upsert ok: (\d+) bytes compared, (\d+) touched", out.stdout)
    assert m and int(m.group(1)) == len(f["saved"]) and int(m.group(2)) > 40, out.stdout
