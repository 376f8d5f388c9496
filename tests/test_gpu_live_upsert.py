"""GPU tests (MI355X) of upsert, replace_deleted and resizeIndex on a resident vanilla index: hs_index_upsert_points,
hs_index_set_replace_deleted, hs_index_resize through the Python binding and the C++ facade.

Everything is pinned to the compiled reference through tests/golden/updates_*.npz (tests/golden/make_golden_updates.py: the
reference's own addPoint / markDelete / resizeIndex driven by an operation list, its saved file and its searchKnn results): the
resident index that takes the same operations must save the reference's bytes and answer with the reference's labels and fp32
bits, and must equal -- in every output, counter and info() field -- a fresh load of its own saved file, in every row format."""
import os
import subprocess

import numpy as np
import pytest

from hsutil import GOLDEN, ROOT, load_product, mixture

pytestmark = pytest.mark.gpu
ADD, MARK, UNMARK, RESIZE = 0, 1, 2, 3
GRAPHS = [("l2_cont_d32", 32), ("l2_int_d16", 16)]
SCENARIOS = ["update", "replace", "resize"]
INFO_FIELDS = ("n", "maxlevel", "enterpoint", "n_edges", "max_degree0", "index_size", "has_deleted")


@pytest.fixture(scope="module")
def hs():
    m = load_product()
    assert os.path.exists(m.LIB_PATH), "HIP extension missing: run __graft_entry__.build()"
    assert m.device_count() > 0, "no HIP device visible"
    return m


def _fixture(name, scenario):
    return np.load(os.path.join(GOLDEN, f"updates_{scenario}_{name}.npz"))


def _pq_sorted(d, l, c):
    return [sorted(zip(d[i, :int(c[i])].view(np.uint32).tolist(), l[i, :int(c[i])].tolist())) for i in range(len(c))]


def _answers(ix, q, k, efs=(10, 32), modes=(True, False)):
    """Every output bit and counter of search_pq over both exact-order modes and the efs, as one comparable list."""
    out = []
    for exact in modes:
        ix.set_exact_order(exact)
        for ef in efs:
            ix.set_ef(ef)
            r = ix.search_pq(q, k, want_stats=True)
            out.append((exact, ef, r["labels"].tobytes(), r["dists"].tobytes(), r["cnt"].tobytes(), r["stats"].tobytes()))
    ix.set_exact_order(False)
    return out


def _info(ix):
    i = ix.info()
    return {f: i[f] for f in INFO_FIELDS}


def _fmt(hs, name):
    return {"f32": hs.HS_ROWS_F32, "u8": hs.HS_ROWS_U8, "f16": hs.HS_ROWS_F16}[name]


def _load(hs, path, dim, fmt, free, max_elements=0):
    if free:
        return hs.Index.load_narrow(path, hs.HS_KIND_HNSW, dim, fmt, max_elements=max_elements)
    ix = hs.Index(path, hs.HS_KIND_HNSW, dim, max_elements=max_elements)
    if fmt != hs.HS_ROWS_F32:
        ix.set_row_format(fmt)
    return ix


def _apply(ix, ops, rows):
    """The operation list of hs_hnsw_replay on a resident index: runs of adds as one upsert_points call each, runs of marks as
    one mark_deleted call each."""
    i = 0
    while i < len(ops):
        kind = int(ops[i, 0])
        j = i
        while j < len(ops) and int(ops[j, 0]) == kind and kind != RESIZE:
            j += 1
        j = max(j, i + 1)
        run = ops[i:j]
        if kind == ADD:
            ix.upsert_points(rows[run[:, 3].astype(np.int64)], run[:, 1], run[:, 2] != 0)
        elif kind in (MARK, UNMARK):
            ix.mark_deleted(run[:, 1], on=kind == MARK)
        else:
            ix.resize(int(run[0, 1]))
        i = j


def _resident(hs, name, dim, f, fmt=None, free=False):
    """The golden graph loaded with the fixture's room (a fixture that loads full gets one spare slot: without it no host image
    is kept) and its replacement flag."""
    src = os.path.join(GOLDEN, f"{name}.hnsw.bin")
    n = int(np.frombuffer(open(src, "rb").read(24), np.uint64)[2])
    ix = _load(hs, src, dim, hs.HS_ROWS_F32 if fmt is None else fmt, free, max_elements=int(f["max_elements"]) or n + 1)
    if int(f["allow"]):
        ix.set_replace_deleted(True)
    return ix, n


def _check_against_reference(ix, f, q):
    k = int(f["k"])
    for exact in (True, False):
        ix.set_exact_order(exact)
        for ef in f["efs"]:
            ef = int(ef)
            ix.set_ef(ef)
            r = ix.search_pq(q, k, want_stats=True)
            assert np.array_equal(r["cnt"], f[f"ef{ef}_cnt"])
            assert _pq_sorted(r["dists"], r["labels"], r["cnt"]) == _pq_sorted(f[f"ef{ef}_dists"], f[f"ef{ef}_labels"], f[f"ef{ef}_cnt"])
            assert np.array_equal(r["stats"][:, 0], f[f"ef{ef}_calls"])
    ix.set_exact_order(False)


def _kernel(ix, q, k, ef):
    ix.set_ef(ef)
    ix.search_pq(q, k)
    return ix.last_kernel()


@pytest.mark.parametrize("scenario", SCENARIOS)
@pytest.mark.parametrize("name,dim", GRAPHS)
def test_resident_replay_vs_compiled_reference(hs, tmp_path, name, dim, scenario):
    """The fixture's operations on a resident fp32 index: save() gives the reference's file, searches give the reference's labels,
    fp32 distance bits, counts and distance-call counts (both exact-order modes, ef 10 and 64), and the kernel follows the marks:
    the flat kernel in a state without marks, a fast / strict one in the replace scenario's final state with its two marks."""
    f = _fixture(name, scenario)
    q, k = np.load(os.path.join(GOLDEN, f"{name}.npz"))["queries"], int(f["k"])
    ops, rows = f["ops"], f["rows"]
    ix, n = _resident(hs, name, dim, f)
    if scenario == "replace":
        # up to the two marks that stay: every vacancy was refilled, no mark is left, the flat kernel is back
        assert (ops[-2:, 0] == MARK).all() and int(ops[-3, 0]) == ADD
        _apply(ix, ops[:30], rows)
        assert ix.deleted_count() == 30 and ix.info()["has_deleted"] == 1 and _kernel(ix, q, k, 32) == "hs::fast_kernel"
        _apply(ix, ops[30:-2], rows)
        assert ix.deleted_count() == 0 and ix.info()["has_deleted"] == 0 and _kernel(ix, q, k, 32) == "hs::flat_kernel"
        assert ix.info()["n"] == n + 10          # 30 of the 40 flagged adds took a vacancy, 10 were appended
        _apply(ix, ops[-2:], rows)
        assert ix.deleted_count() == 2 and ix.info()["has_deleted"] == 1
        assert _kernel(ix, q, k, 32) == "hs::fast_kernel" and _kernel(ix, q, k, k) == "hs::strict_kernel"
    else:
        _apply(ix, ops, rows)
        assert ix.deleted_count() == 0 and ix.info()["has_deleted"] == 0 and _kernel(ix, q, k, 32) == "hs::flat_kernel"
    saved = str(tmp_path / "saved.bin")
    ix.save(saved)
    assert open(saved, "rb").read() == f["saved"].tobytes()
    _check_against_reference(ix, f, q)
    # rows and labels: the last row written under a label is what get_row returns
    adds = ops[ops[:, 0] == ADD]
    final = {int(lab): int(r) for lab, r in zip(adds[:, 1], adds[:, 3])}
    marked = set(ops[-2:, 1].tolist()) if scenario == "replace" else set()
    for lab, r in final.items():
        if lab not in marked:
            assert ix.get_row(lab).tobytes() == rows[r].tobytes()
    if scenario == "replace":
        # the labels of the 30 slots that were reused are gone, their successors are found
        gone = [int(m) for m in ops[:30, 1]]
        assert set(gone).isdisjoint(ix.labels().tolist()) and set(final) <= set(ix.labels().tolist())
        for lab in gone[:5] + sorted(marked):
            with pytest.raises(hs.HsError) as e:
                ix.get_row(lab)
            assert e.value.status == hs.HS_ERR_INVALID and str(e.value) == "Label not found"
        with pytest.raises(hs.HsError) as e:
            ix.mark_deleted([gone[0]])
        assert str(e.value) == "Label not found"
    if scenario == "resize":
        assert ix.capacity() == n + 50 == ix.info()["n"]


CASES = [("l2_cont_d32", 32, "f32", False), ("l2_int_d16", 16, "u8", False), ("l2_int_d16", 16, "u8", True), ("l2_int_d16", 16, "f16", True)]


@pytest.mark.parametrize("scenario", SCENARIOS)
@pytest.mark.parametrize("name,dim,fmt,free", CASES)
def test_resident_equals_load_whole(hs, tmp_path, name, dim, fmt, free, scenario):
    """After each scenario the resident index and a fresh load of its saved file (same capacity, same row format) agree in every
    output, counter and info() field -- fp32, u8 beside fp32, u8 and fp16 without fp32 rows (the update kernel writes the
    lane-major narrow rows of rewritten nodes itself) -- and the file is the reference's."""
    fmt = _fmt(hs, fmt)
    f = _fixture(name, scenario)
    q, k = np.load(os.path.join(GOLDEN, f"{name}.npz"))["queries"], int(f["k"])
    ix, n = _resident(hs, name, dim, f, fmt, free)
    _apply(ix, f["ops"], f["rows"])
    saved = str(tmp_path / "saved.bin")
    ix.save(saved)
    assert open(saved, "rb").read() == f["saved"].tobytes()
    again = _load(hs, saved, dim, fmt, free, max_elements=ix.capacity())
    assert _info(ix) == _info(again) and ix.info()["device_bytes"] == again.info()["device_bytes"]
    assert ix.capacity() == again.capacity() and ix.deleted_count() == again.deleted_count()
    assert np.array_equal(ix.labels(), again.labels())
    assert ix.row_format() == fmt and ix.f32_resident() == (not free)
    assert _answers(ix, q, k, efs=(10, 32, 64)) == _answers(again, q, k, efs=(10, 32, 64))
    a, b = ix.exact_search(q, k), again.exact_search(q, k)
    assert a["labels"].tobytes() == b["labels"].tobytes() and a["dists"].tobytes() == b["dists"].tobytes()
    _check_against_reference(ix, f, q)
    adds = f["ops"][f["ops"][:, 0] == ADD]
    for lab in adds[:, 1].tolist()[:6]:
        try:
            mine = ix.get_row(lab)
        except hs.HsError:
            with pytest.raises(hs.HsError):
                again.get_row(lab)
            continue
        assert mine.tobytes() == again.get_row(lab).tobytes()
    if not free and fmt != hs.HS_ROWS_F32:      # both copies were rewritten: drop the fp32 rows and ask the narrow one alone
        want = _answers(ix, q, k)
        ix.set_f32_resident(False)
        assert _answers(ix, q, k) == want


@pytest.mark.parametrize("fmt,free", [("f32", False), ("u8", False), ("f16", True)])
def test_bare_resize(hs, fmt, free):
    """hs_index_resize alone: search outputs are bit-identical before and after, a filter set created before it still works,
    capacity and index_size follow, device_bytes changes by the narrow copy's capacity term only; shrinking lowers the reported
    capacity; rows appended beyond the old capacity are found."""
    fmt = _fmt(hs, fmt)
    g = np.load(os.path.join(GOLDEN, "l2_int_d16.npz"))
    base, q, k = g["base"], g["queries"], int(g["k"])
    n = base.shape[0]
    ix = _load(hs, os.path.join(GOLDEN, "l2_int_d16.hnsw.bin"), 16, fmt, free, max_elements=n + 1)
    fs = hs.FilterSet(ix, 1)
    fs.write(0, (ix.labels() % 3 != 1).astype(np.uint8))
    fq = np.zeros(len(q), np.uint32)
    ix.set_ef(32)
    before, before_fs, i0 = _answers(ix, q, k), ix.search_filter_set(q, k, fs, fq), ix.info()
    ix.resize(n + 300)
    i1 = ix.info()
    assert ix.capacity() == n + 300 and _answers(ix, q, k) == before
    ix.set_ef(32)
    after_fs = ix.search_filter_set(q, k, fs, fq)
    assert after_fs["labels"].tobytes() == before_fs["labels"].tobytes() and after_fs["dists"].tobytes() == before_fs["dists"].tobytes()
    width = {hs.HS_ROWS_F32: 0, hs.HS_ROWS_U8: 1, hs.HS_ROWS_F16: 2}[fmt]
    if free:     # without fp32 rows device_bytes is also short of the fp32 array's capacity, as after a load of that capacity
        whole = _load(hs, os.path.join(GOLDEN, "l2_int_d16.hnsw.bin"), 16, fmt, free, max_elements=n + 300)
        assert i1["device_bytes"] == whole.info()["device_bytes"]
    else:
        assert i1["device_bytes"] - i0["device_bytes"] == 299 * 16 * width
    assert i1["index_size"] - i0["index_size"] == 299 * (16 * 4 + 4 + 4)      # level-0 link block + element_levels_ per slot
    assert {f: i1[f] for f in INFO_FIELDS if f != "index_size"} == {f: i0[f] for f in INFO_FIELDS if f != "index_size"}
    # appends beyond the old capacity
    new = np.clip(base[:200] + 1, base.min(), base.max())
    ix.add_points(new[:100], np.arange(n, n + 100))
    ix.upsert_points(new[100:], np.arange(n + 100, n + 200))
    assert ix.info()["n"] == n + 200
    for lab in (n, n + 99, n + 100, n + 199):
        assert ix.get_row(lab).tobytes() == (new[lab - n] + np.float32(0.0)).tobytes()
    ix.resize(n + 200)      # shrinking to the element count: only the reported capacity
    assert ix.capacity() == n + 200
    with pytest.raises(hs.HsError) as e:
        ix.upsert_points(new[:1], [n + 500])
    assert e.value.status == hs.HS_ERR_CAPACITY and str(e.value) == "The number of elements exceeds the specified limit"
    with pytest.raises(hs.HsError) as e:
        ix.resize(n + 199)
    assert e.value.status == hs.HS_ERR_INVALID and str(e.value) == "Cannot resize, max element is less than the current number of elements"
    ix.resize(n + 201)
    ix.upsert_points(new[:1], [n + 500])
    assert ix.get_row(n + 500).tobytes() == (new[0] + np.float32(0.0)).tobytes()


@pytest.mark.parametrize("fmt,free", [("f32", False), ("u8", True)])
def test_update_through_the_retile_path(hs, tmp_path, fmt, free):
    """Twenty points with M = 16 (every level-0 list at most 16 ids: tile stride 16); twelve updates push a list past 16, so the
    call re-tiles everything at stride 32 (and rebuilds the narrow copy).  Equal to the host replay's file loaded whole."""
    fmt = _fmt(hs, fmt)
    base = mixture(1500, 16, 311, integer=True)
    part, want = str(tmp_path / "part.bin"), str(tmp_path / "want.bin")
    hs.build_hnsw(base[:20], part, M=16, ef_construction=80, branching_factor="4", seed=100, threads=1)
    labs = np.random.default_rng(5).integers(0, 20, 12)
    rows = np.ascontiguousarray(base[1000:1012])
    hs.hnsw_replay(part, want, [(ADD, int(l), 0, i) for i, l in enumerate(labs)], rows, 16, max_elements=21)
    ix = _load(hs, part, 16, fmt, free, max_elements=21)
    assert ix.info()["max_degree0"] <= 16
    ix.upsert_points(rows, labs)
    assert ix.info()["max_degree0"] > 16
    saved = str(tmp_path / "saved.bin")
    ix.save(saved)
    assert open(saved, "rb").read() == open(want, "rb").read()
    whole = _load(hs, want, 16, fmt, free, max_elements=21)
    q = mixture(32, 16, 312, integer=True)
    assert _info(ix) == _info(whole) and ix.info()["device_bytes"] == whole.info()["device_bytes"]
    assert _answers(ix, q, 5) == _answers(whole, q, 5)
    # a second call at the new stride takes the record path
    ix.upsert_points(rows[:3] + 1, labs[:3])
    whole.upsert_points(rows[:3] + 1, labs[:3])
    assert _answers(ix, q, 5) == _answers(whole, q, 5)


def test_refusals_leave_the_index_as_it_was(hs, tmp_path):
    g = np.load(os.path.join(GOLDEN, "l2_int_d16.npz"))
    base, q, k = g["base"], g["queries"], int(g["k"])
    n = base.shape[0]
    hp, sp = os.path.join(GOLDEN, "l2_int_d16.hnsw.bin"), str(tmp_path / "s.bin")
    ix = hs.Index(hp, hs.HS_KIND_HNSW, 16, max_elements=n + 2)
    ix.set_row_format(hs.HS_ROWS_U8)
    full = hs.Index(hp, hs.HS_KIND_HNSW, 16)
    ix.mark_deleted([5, 6])
    new = np.clip(base[:4] + 1, base.min(), base.max())
    a, b = str(tmp_path / "a.bin"), str(tmp_path / "b.bin")
    ix.save(a)

    def state():
        ix.save(b)
        return _answers(ix, q, k), ix.info(), ix.deleted_count(), ix.capacity(), open(b, "rb").read()

    prior, prior_full = state(), _answers(full, q, k)
    assert prior[4] == open(a, "rb").read()

    def refused(fn, status, text):
        with pytest.raises(hs.HsError) as e:
            fn()
        assert e.value.status == status and str(e.value) == text, str(e.value)
        assert state() == prior

    off = "Replacement of deleted elements is disabled in constructor"
    limit = "The number of elements exceeds the specified limit"
    refused(lambda: ix.upsert_points(new[:2], [7, n], [False, True]), hs.HS_ERR_INVALID, off)     # the first point alone would be fine
    refused(lambda: ix.upsert_points(new[:4], [7, n, n + 1, n + 2]), hs.HS_ERR_CAPACITY, limit)
    refused(lambda: ix.upsert_points(new[:4], [n, n, n + 1, n + 2]), hs.HS_ERR_CAPACITY, limit)   # n twice: one append and one update
    bad = new[:3].copy()
    bad[2, 5] = 0.5
    with pytest.raises(hs.HsError) as e:
        ix.upsert_points(bad, [7, 8, 9])
    assert e.value.status == hs.HS_ERR_UNSUPPORTED and "row 2 " in str(e.value) and "component 5" in str(e.value) and state() == prior
    refused(lambda: ix.resize(n - 1), hs.HS_ERR_INVALID, "Cannot resize, max element is less than the current number of elements")
    ix.set_replace_deleted(True)
    refused(lambda: ix.upsert_points(new[:2], [7, 5]), hs.HS_ERR_INVALID,
            "Can't use addPoint to update deleted elements if replacement of deleted elements is enabled.")
    # two vacancies, two spare slots: a fifth new label has nowhere to go -- and nothing of the four before it happens
    refused(lambda: ix.upsert_points(np.repeat(new, 2, axis=0)[:5], np.arange(n, n + 5), True), hs.HS_ERR_CAPACITY, limit)
    ix.set_replace_deleted(False)
    # an index without a host image
    for fn, status, text in ((lambda: full.upsert_points(new[:1], [3]), hs.HS_ERR_CAPACITY, limit),
                             (lambda: full.upsert_points(new[:1], [3], True), hs.HS_ERR_INVALID, "no host image")):
        with pytest.raises(hs.HsError) as e:
            fn()
        assert e.value.status == status and text in str(e.value)
    for fn in (lambda: full.resize(n + 10), lambda: full.set_replace_deleted(True)):
        with pytest.raises(hs.HsError) as e:
            fn()
        assert e.value.status == hs.HS_ERR_INVALID and "no host image" in str(e.value)
    assert _answers(full, q, k) == prior_full
    # Slim indexes take none of it
    hs.convert_slim(hp, sp, 16)
    sx = hs.Index(sp, hs.HS_KIND_SLIM, 16, max_elements=n + 10)
    sx.set_ef(32)
    s_prior = sx.search_ids(q, k, want_dists=True)
    for fn in (lambda: sx.upsert_points(new[:1], [3]), lambda: sx.resize(n + 20), lambda: sx.set_replace_deleted(True)):
        with pytest.raises(hs.HsError) as e:
            fn()
        assert e.value.status == hs.HS_ERR_UNSUPPORTED and "vanilla" in str(e.value)
    s_after = sx.search_ids(q, k, want_dists=True)
    assert np.array_equal(s_prior["labels"], s_after["labels"]) and s_prior["dists"].tobytes() == s_after["dists"].tobytes()
    # and the accepted forms of the refused calls go through
    ix.set_replace_deleted(True)
    ix.upsert_points(np.repeat(new, 2, axis=0)[:4], np.arange(n, n + 4), True)
    assert ix.info()["n"] == n + 2 and ix.deleted_count() == 0 and ix.info()["has_deleted"] == 0


def test_facade_upsert(hs, tmp_path):
    """tests/facade_upsert.cpp: a caller of hnswlib's own API -- the allow_replace_deleted constructor flag, addPoint of an existing
    label, addPoint(.., true), resizeIndex -- with the reference's exception texts; its saved file and answers are the binding's."""
    exe = os.path.join(ROOT, "hnsw-slim_amd", "facade_upsert")
    f = _fixture("l2_cont_d32", "replace")
    src = os.path.join(GOLDEN, "l2_cont_d32.hnsw.bin")
    q = np.ascontiguousarray(np.load(os.path.join(GOLDEN, "l2_cont_d32.npz"))["queries"][:40])
    of, rf, qf, out, saved = (str(tmp_path / x) for x in ("ops.u64", "rows.f32", "q.f32", "out.bin", "saved.bin"))
    f["ops"].tofile(of)
    f["rows"].tofile(rf)
    q.tofile(qf)
    run = subprocess.run([exe, src, "32", str(int(f["max_elements"])), of, str(len(f["ops"])), rf, qf, str(len(q)), "10", out, saved],
                         capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = dict(l.split(": ", 1) for l in run.stdout.strip().splitlines())
    assert lines["replace without the flag"] == "Replacement of deleted elements is disabled in constructor"
    assert lines["update of a deleted label"] == "Can't use addPoint to update deleted elements if replacement of deleted elements is enabled."
    assert lines["resize below the count"] == "Cannot resize, max element is less than the current number of elements"
    assert lines["add beyond max_elements"] == "The number of elements exceeds the specified limit"
    assert lines["after resize"] == "ok"
    assert lines["resize of an index loaded full"] == "ok"
    assert lines["resize of an index loaded full after a mark"].startswith("hnswlib_amd: resizeIndex of an index loaded without spare capacity")
    assert open(saved, "rb").read() == f["saved"].tobytes()
    ix, _ = _resident(hs, "l2_cont_d32", 32, f)
    _apply(ix, f["ops"], f["rows"])
    ix.set_ef(32)
    r = ix.search_pq(q, 10)
    raw = open(out, "rb").read()
    assert raw == r["labels"].tobytes() + r["dists"].tobytes() + r["cnt"].tobytes()
