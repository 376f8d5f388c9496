"""GPU tests (MI355X) of live updates on a resident vanilla index: hs_index_mark_deleted, hs_index_add_points, hs_index_save,
hs_index_get_row through the Python binding and the C++ facade.

Marks are pinned to the compiled reference (the `_del` goldens: the reference's own markDelete + saveIndex + searchKnn).  Adds are
pinned through the files: a resident index that grew from a prefix must equal, in every output bit and counter, the index loaded
whole from the reference's file of the full build, and save() must give that file back.  The golden graphs have M = 8, whose
level-0 capacity (16) is the smallest tile stride, so none of them can outgrow its tiles: the re-tile path is driven by an M = 16
graph of our own, compared with its one-shot build (the builder itself is pinned byte for byte in tests/test_host_cpu.py)."""
import os
import subprocess

import numpy as np
import pytest

from hsutil import GOLDEN, ROOT, load_product, mixture

pytestmark = pytest.mark.gpu
L2 = 0


@pytest.fixture(scope="module")
def hs():
    m = load_product()
    assert os.path.exists(m.LIB_PATH), "HIP extension missing: run __graft_entry__.build()"
    assert m.device_count() > 0, "no HIP device visible"
    return m


def _pq_sorted(d, l, c):
    out = []
    for i in range(len(c)):
        n = int(c[i])
        out.append(sorted(zip(d[i, :n].view(np.uint32).tolist(), l[i, :n].tolist())))
    return out


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


def _marked_labels(n, every):
    return np.arange(every // 2, n, every, dtype=np.uint64)


INFO_FIELDS = ("n", "maxlevel", "enterpoint", "n_edges", "max_degree0", "index_size", "has_deleted")


def _info(ix):
    i = ix.info()
    return {f: i[f] for f in INFO_FIELDS}


def _check_against_del_golden(ix, g):
    k = int(g["k"])
    for exact in (True, False):
        ix.set_exact_order(exact)
        for ef in g["efs"]:
            ef = int(ef)
            ix.set_ef(ef)
            r = ix.search_pq(g["queries"], k, want_stats=True)
            assert np.array_equal(r["cnt"], g[f"ef{ef}_cnt"])
            assert _pq_sorted(r["dists"], r["labels"], r["cnt"]) == _pq_sorted(g[f"ef{ef}_dists"], g[f"ef{ef}_labels"], g[f"ef{ef}_cnt"])
            assert np.array_equal(r["stats"][:, 0], g[f"ef{ef}_calls"])
    ix.set_exact_order(False)


@pytest.mark.parametrize("name,dim", [("l2_cont_d32", 32), ("l2_int_d16", 16)])
def test_live_marks_vs_compiled_reference(hs, oracle, tmp_path, name, dim):
    """The unmarked golden index, marked live as the reference's `markdel` run marked it, answers as the reference answered on its
    marked index (labels, fp32 distances, counts, distance-call counts; every ef; both exact-order modes); the kernel choice
    follows num_deleted_ > 0 in both directions; a filter set on top gives the reference's filtered answers; the saved file is the
    reference's marked file but for the max_elements field, and the oracle on it reproduces the golden."""
    g = np.load(os.path.join(GOLDEN, f"{name}_del.npz"))
    q, k, every = g["queries"], int(g["k"]), int(g["every"])
    src = os.path.join(GOLDEN, f"{name}.hnsw.bin")
    plain = hs.Index(src, hs.HS_KIND_HNSW, dim)
    n = plain.info()["n"]
    untouched = _answers(plain, q, k)
    ix = hs.Index(src, hs.HS_KIND_HNSW, dim, max_elements=n + 1)    # one spare slot: keeps the host image
    assert ix.capacity() == n + 1 and plain.capacity() == n and ix.deleted_count() == 0
    assert _answers(ix, q, k) == untouched
    ix.set_ef(32)
    ix.search_pq(q, k)
    assert ix.last_kernel() == "hs::flat_kernel" and hs.debug_plan_input(ix, k, len(q)).has_deleted == 0
    fs = None
    if name == "l2_int_d16":     # a filter set created BEFORE the marks survives them untouched
        gf = np.load(os.path.join(GOLDEN, "l2_int_d16_del_filter.npz"))
        fs = hs.FilterSet(ix, 1)
        fs.write(0, (ix.labels() % int(gf["mod"]) != int(gf["rem"])).astype(np.uint8))
    marks = _marked_labels(n, every)
    ix.mark_deleted(marks)
    assert ix.deleted_count() == len(marks) and ix.info()["has_deleted"] == 1
    assert hs.debug_plan_input(ix, k, len(q)).has_deleted == 1
    _check_against_del_golden(ix, g)
    ix.set_ef(32)
    ix.search_pq(q, k)
    assert ix.last_kernel() == "hs::fast_kernel"
    ix.set_ef(k)
    ix.search_pq(q, k)
    assert ix.last_kernel() == "hs::strict_kernel"
    if fs is not None:
        for ef in gf["efs"]:
            ef = int(ef)
            ix.set_ef(ef)
            r = ix.search_filter_set(gf["queries"], k, fs, np.zeros(len(gf["queries"]), np.uint32), want_stats=True)
            assert np.array_equal(r["cnt"], gf[f"ef{ef}_cnt"])
            assert _pq_sorted(r["dists"], r["labels"], r["cnt"]) == _pq_sorted(gf[f"ef{ef}_dists"], gf[f"ef{ef}_labels"], gf[f"ef{ef}_cnt"])
            assert np.array_equal(r["stats"][:, 0], gf[f"ef{ef}_calls"])
    # the exact scan sees the live marks: as on the index loaded from the reference's marked file
    loaded = hs.Index(os.path.join(GOLDEN, f"{name}_del.hnsw.bin"), hs.HS_KIND_HNSW, dim)
    a, b = ix.exact_search(q, k), loaded.exact_search(q, k)
    assert a["labels"].tobytes() == b["labels"].tobytes() and a["dists"].tobytes() == b["dists"].tobytes() and np.array_equal(a["cnt"], b["cnt"])
    assert not np.isin(a["labels"], marks).any()
    # saveIndex: the reference's marked file, except the 8-byte max_elements field of the header
    saved = str(tmp_path / "saved.bin")
    ix.save(saved)
    mine, ref = open(saved, "rb").read(), open(os.path.join(GOLDEN, f"{name}_del.hnsw.bin"), "rb").read()
    assert len(mine) == len(ref) and mine[:8] == ref[:8] and mine[16:] == ref[16:]
    assert int(np.frombuffer(mine, np.uint64, 1, 8)[0]) == n + 1 and int(np.frombuffer(ref, np.uint64, 1, 8)[0]) == n
    ox = oracle.load(saved, "hnsw", L2, dim)
    for ef in g["efs"]:
        ef = int(ef)
        ox.set_ef(ef)
        o = ox.search_pq(q, k)
        assert _pq_sorted(o["dists"], o["labels"], o["cnt"]) == _pq_sorted(g[f"ef{ef}_dists"], g[f"ef{ef}_labels"], g[f"ef{ef}_cnt"])
    # unmark everything: the flat kernel again, and every output and counter bit-equal to the untouched index
    ix.mark_deleted(marks, on=False)
    assert ix.deleted_count() == 0 and ix.info()["has_deleted"] == 0 and hs.debug_plan_input(ix, k, len(q)).has_deleted == 0
    assert _answers(ix, q, k) == untouched
    ix.set_ef(32)
    ix.search_pq(q, k)
    assert ix.last_kernel() == "hs::flat_kernel"
    # marks work without a host image too (an index loaded without room)
    plain.mark_deleted(marks)
    _check_against_del_golden(plain, g)
    plain.mark_deleted(marks, on=False)
    assert _answers(plain, q, k) == untouched


@pytest.mark.parametrize("calls", [1, 4])
@pytest.mark.parametrize("n0", [10, None])
@pytest.mark.parametrize("name,dim", [("l2_cont_d32", 32), ("l2_int_d16", 16), ("l2_cont_d21", 21)])
def test_add_equals_load_whole(hs, tmp_path, name, dim, n0, calls):
    """A prefix build loaded with room, its generator put where the build left it, grown with add_points (one call / several) ==
    the reference's file of the whole build loaded whole: outputs, counters, info(), and save() gives the file back.
    (d = 21: rows that are not 16-byte aligned take the 4-byte copy of the update kernel.)"""
    g = np.load(os.path.join(GOLDEN, f"{name}.npz"))
    base, q, k = g["base"], g["queries"], int(g["k"])
    n = base.shape[0]
    n0 = n // 2 if n0 is None else n0
    ref_path = os.path.join(GOLDEN, f"{name}.hnsw.bin")
    part = str(tmp_path / "part.bin")
    hs.build_hnsw(base[:n0], part, M=int(g["M"]), ef_construction=int(g["efC"]), branching_factor="4", seed=100, threads=1)
    whole = hs.Index(ref_path, hs.HS_KIND_HNSW, dim)
    ix = hs.Index(part, hs.HS_KIND_HNSW, dim, max_elements=n)
    assert ix.info()["n"] == n0 and ix.capacity() == n
    fs_old = hs.FilterSet(ix, 1)
    ix.seed_levels(100, n0)
    cuts = np.linspace(n0, n, calls + 1).astype(int)
    for a, b in zip(cuts[:-1], cuts[1:]):
        ix.add_points(base[a:b], np.arange(a, b))
    assert _info(ix) == _info(whole)
    assert np.array_equal(ix.labels(), whole.labels())
    assert _answers(ix, q, k) == _answers(whole, q, k)
    ex_a, ex_b = ix.exact_search(q, k), whole.exact_search(q, k)
    assert ex_a["labels"].tobytes() == ex_b["labels"].tobytes() and ex_a["dists"].tobytes() == ex_b["dists"].tobytes()
    saved = str(tmp_path / "saved.bin")
    ix.save(saved)
    assert open(saved, "rb").read() == open(ref_path, "rb").read()
    for lab in (0, n0 - 1, n0, n - 1):
        assert ix.get_row(lab).tobytes() == base[lab].tobytes()
    # a filter set created for the old n is refused after the add (the existing rule), one for the new n works
    with pytest.raises(hs.HsError) as e:
        ix.search_filter_set(q, k, fs_old, np.zeros(len(q), np.uint32))
    assert e.value.status == hs.HS_ERR_INVALID and "created for" in str(e.value)
    # the index is full now
    with pytest.raises(hs.HsError) as e:
        ix.add_points(base[:1], [n + 5])
    assert e.value.status == hs.HS_ERR_CAPACITY and str(e.value) == "The number of elements exceeds the specified limit"


def _int_rows(n, d, seed):
    return mixture(n, d, seed, integer=True)


@pytest.fixture(scope="module")
def m16(hs, tmp_path_factory):
    """An M = 16 graph over integer rows (level-0 lists grow past 16 ids): the whole build and its first 10 points, shared."""
    d = tmp_path_factory.mktemp("m16")
    base = _int_rows(1500, 16, 311)
    q = _int_rows(64, 16, 312)
    whole, part = str(d / "whole.bin"), str(d / "part.bin")
    hs.build_hnsw(base, whole, M=16, ef_construction=80, branching_factor="4", seed=100, threads=1)
    hs.build_hnsw(base[:10], part, M=16, ef_construction=80, branching_factor="4", seed=100, threads=1)
    return dict(base=base, q=q, whole=whole, part=part)


def _load(hs, path, dim, fmt, free, max_elements=0):
    if free:
        return hs.Index.load_narrow(path, hs.HS_KIND_HNSW, dim, fmt, max_elements=max_elements)
    ix = hs.Index(path, hs.HS_KIND_HNSW, dim, max_elements=max_elements)
    if fmt != hs.HS_ROWS_F32:
        ix.set_row_format(fmt)
    return ix


FORMATS = [("f32", False), ("u8", False), ("f16", False), ("u8", True), ("f16", True)]


def _fmt(hs, name):
    return {"f32": hs.HS_ROWS_F32, "u8": hs.HS_ROWS_U8, "f16": hs.HS_ROWS_F16}[name]


@pytest.mark.parametrize("fmt,free", FORMATS)
def test_add_through_the_retile_path(hs, m16, tmp_path, fmt, free):
    """Ten points (degrees below 16: tile stride 16) grown to 1500 in two calls: a level-0 list outgrows the stride during the first
    call, everything is re-tiled (and the narrow copy rebuilt); the second call then takes the record path at the new stride."""
    fmt = _fmt(hs, fmt)
    base, q = m16["base"], m16["q"]
    n = base.shape[0]
    assert hs.rows_representable(base, hs.HS_ROWS_U8) is None and hs.rows_representable(base, hs.HS_ROWS_F16) is None
    whole = _load(hs, m16["whole"], 16, fmt, free)
    ix = _load(hs, m16["part"], 16, fmt, free, max_elements=n)
    before = ix.info()
    assert before["max_degree0"] <= 16          # tile stride 16
    ix.seed_levels(100, 10)
    ix.add_points(base[10:700], np.arange(10, 700))
    mid = ix.info()
    assert mid["max_degree0"] > 16               # tile stride 32: the stride grew inside this call
    ix.add_points(base[700:], np.arange(700, n))
    assert ix.info()["max_degree0"] > 16 and _info(ix) == _info(whole)
    assert ix.info()["device_bytes"] == whole.info()["device_bytes"]     # n tile rows of the whole index's stride among them
    assert ix.row_format() == fmt and ix.f32_resident() == (not free)
    assert _answers(ix, q, 10) == _answers(whole, q, 10)
    saved = str(tmp_path / "saved.bin")
    ix.save(saved)
    assert open(saved, "rb").read() == open(m16["whole"], "rb").read()
    for lab in (0, 9, 10, 699, 700, n - 1):     # (a u8 copy reads +0.0f where -0.0f was stored: the documented widening)
        want_row = base[lab] + np.float32(0.0) if (free and fmt == hs.HS_ROWS_U8) else base[lab]
        assert ix.get_row(lab).tobytes() == want_row.tobytes()


@pytest.mark.parametrize("fmt,free", FORMATS)
def test_add_in_every_row_format(hs, tmp_path, fmt, free):
    """The record path (no re-tile: M = 8) on an index in a narrow format beside fp32 and on an fp32-free one: the update kernel
    writes the lane-major narrow row itself.  An unrepresentable row is refused and changes nothing; get_row returns the stored
    row bit for bit."""
    fmt = _fmt(hs, fmt)
    g = np.load(os.path.join(GOLDEN, "l2_int_d16.npz"))
    base, q, k = g["base"], g["queries"], int(g["k"])
    n, n0 = base.shape[0], base.shape[0] // 2
    assert hs.rows_representable(base, hs.HS_ROWS_U8) is None and hs.rows_representable(base, hs.HS_ROWS_F16) is None
    part = str(tmp_path / "part.bin")
    hs.build_hnsw(base[:n0], part, M=int(g["M"]), ef_construction=int(g["efC"]), branching_factor="4", seed=100, threads=1)
    whole = _load(hs, os.path.join(GOLDEN, "l2_int_d16.hnsw.bin"), 16, fmt, free)
    ix = _load(hs, part, 16, fmt, free, max_elements=n)
    ix.seed_levels(100, n0)
    if fmt != hs.HS_ROWS_F32:
        prior = _answers(ix, q, k)
        bad = base[n0:n0 + 3].copy()
        bad[1, 5] = 0.5 if fmt == hs.HS_ROWS_U8 else np.float32(1.0 + 2.0 ** -12)
        with pytest.raises(hs.HsError) as e:
            ix.add_points(bad, np.arange(n0, n0 + 3))
        assert e.value.status == hs.HS_ERR_UNSUPPORTED and "row 1 " in str(e.value) and "component 5" in str(e.value)
        assert ix.info()["n"] == n0 and _answers(ix, q, k) == prior
    ix.add_points(base[n0:n0 + 1], [n0])
    ix.add_points(base[n0 + 1:], np.arange(n0 + 1, n))
    assert _info(ix) == _info(whole) and ix.info()["device_bytes"] == whole.info()["device_bytes"]
    want = _answers(whole, q, k)
    assert _answers(ix, q, k) == want
    names = {hs.HS_ROWS_F32: "hs::flat_kernel", hs.HS_ROWS_U8: "hs::flat_kernel_u8", hs.HS_ROWS_F16: "hs::flat_kernel_f16"}
    ix.set_ef(32)
    ix.search_pq(q, k)
    assert ix.last_kernel() == names[fmt]
    # what is stored: the row itself, except that a u8 copy holds 0 for -0.0f and reads back +0.0f (these rows do hold -0.0f:
    # np.rint of small negatives) -- the documented widening of hs_index_set_f32_resident, which cannot change a distance
    assert np.signbit(base[base == 0]).any()
    stored = lambda lab, narrow_only: (base[lab] + np.float32(0.0)) if (narrow_only and fmt == hs.HS_ROWS_U8) else base[lab]   # noqa: E731
    for lab in list(range(0, n, 97)) + [n0 - 1, n0, n - 1]:
        assert ix.get_row(lab).tobytes() == stored(lab, free).tobytes()
    if not free and fmt != hs.HS_ROWS_F32:      # both copies were written: drop the fp32 rows and ask the narrow one alone
        ix.set_f32_resident(False)
        assert _answers(ix, q, k) == want
        for lab in (0, n0 - 1, n0, n - 1):
            assert ix.get_row(lab).tobytes() == stored(lab, True).tobytes()
    saved = str(tmp_path / "saved.bin")
    ix.save(saved)
    assert open(saved, "rb").read() == open(os.path.join(GOLDEN, "l2_int_d16.hnsw.bin"), "rb").read()


def test_add_onto_an_index_that_carries_marks(hs, oracle, tmp_path):
    """addPoint with marked nodes in the graph (searchBaseLayer keeps them as stepping stones but never links to them, the deleted
    enter point is offered as a candidate: hnswalg.h:246-255, 308-309, 1344-1360).  Restated from the source, not pinned to a
    compiled run: the resident index must answer exactly as its own saved file reloaded does, and the oracle on that file agrees."""
    g = np.load(os.path.join(GOLDEN, "l2_cont_d32.npz"))
    base, q, k = g["base"], g["queries"], int(g["k"])
    n, n0 = base.shape[0], 1200
    part = str(tmp_path / "part.bin")
    hs.build_hnsw(base[:n0], part, M=8, ef_construction=100, branching_factor="4", seed=100, threads=1)
    ix = hs.Index(part, hs.HS_KIND_HNSW, 32, max_elements=n)
    ep_label = int(ix.labels()[ix.info()["enterpoint"]])
    marks = np.unique(np.concatenate([np.arange(3, n0, 7), [ep_label]])).astype(np.uint64)
    ix.mark_deleted(marks)
    ix.add_points(base[n0:1600], np.arange(n0, 1600))
    ix.mark_deleted(np.arange(n0, 1600, 9))
    ix.add_points(base[1600:], np.arange(1600, n), threads=1)
    assert ix.info()["has_deleted"] == 1 and ix.deleted_count() == len(marks) + len(np.arange(n0, 1600, 9))
    saved = str(tmp_path / "saved.bin")
    ix.save(saved)
    again = hs.Index(saved, hs.HS_KIND_HNSW, 32)
    assert _info(ix) == _info(again)
    assert _answers(ix, q, k, efs=(10, 32, 64)) == _answers(again, q, k, efs=(10, 32, 64))
    ox = oracle.load(saved, "hnsw", L2, 32)
    for ef in (10, 64):
        ix.set_ef(ef)
        ox.set_ef(ef)
        r, o = ix.search_pq(q, k, want_stats=True), ox.search_pq(q, k)
        assert np.array_equal(r["cnt"], o["cnt"])
        assert _pq_sorted(r["dists"], r["labels"], r["cnt"]) == _pq_sorted(o["dists"], o["labels"], o["cnt"])
        assert np.array_equal(r["stats"][:, :3], o["counters"][:, :3])
    deleted = set(marks.tolist()) | set(range(n0, 1600, 9))
    r = ix.search_pq(q, k)
    assert not (set(r["labels"].ravel().tolist()) & deleted)


def test_refusals_leave_the_index_as_it_was(hs, tmp_path):
    g = np.load(os.path.join(GOLDEN, "l2_int_d16.npz"))
    base, q, k = g["base"], g["queries"], int(g["k"])
    n = base.shape[0]
    hp, sp = os.path.join(GOLDEN, "l2_int_d16.hnsw.bin"), str(tmp_path / "s.bin")
    ix = hs.Index(hp, hs.HS_KIND_HNSW, 16, max_elements=n + 10)
    full = hs.Index(hp, hs.HS_KIND_HNSW, 16)
    prior, prior_full = _answers(ix, q, k), _answers(full, q, k)
    new = base[:3] + 1

    def refused(fn, status, text):
        with pytest.raises(hs.HsError) as e:
            fn()
        assert e.value.status == status and text in str(e.value), str(e.value)

    refused(lambda: full.add_points(new, [n, n + 1, n + 2]), hs.HS_ERR_CAPACITY, "The number of elements exceeds the specified limit")
    refused(lambda: ix.add_points(np.repeat(new, 4, axis=0), np.arange(n, n + 12)), hs.HS_ERR_CAPACITY, "exceeds the specified limit")
    refused(lambda: ix.add_points(new, [n, 5, n + 2]), hs.HS_ERR_UNSUPPORTED, "already exists")
    refused(lambda: ix.add_points(new, [n, n + 1, n]), hs.HS_ERR_INVALID, "appears twice")
    refused(lambda: ix.mark_deleted([3, n + 99]), hs.HS_ERR_INVALID, "Label not found")
    refused(lambda: ix.mark_deleted([3, 4, 3]), hs.HS_ERR_INVALID, "The requested to delete element is already deleted")
    refused(lambda: ix.mark_deleted([3], on=False), hs.HS_ERR_INVALID, "The requested to undelete element is not deleted")
    refused(lambda: ix.get_row(n + 99), hs.HS_ERR_INVALID, "Label not found")
    refused(lambda: full.save(str(tmp_path / "no.bin")), hs.HS_ERR_INVALID, "no host image")
    refused(lambda: full.seed_levels(100, 0), hs.HS_ERR_INVALID, "not growable")
    assert not os.path.exists(str(tmp_path / "no.bin"))
    assert ix.deleted_count() == 0 and ix.info()["n"] == n and ix.info()["has_deleted"] == 0
    assert _answers(ix, q, k) == prior and _answers(full, q, k) == prior_full
    ix.mark_deleted([3])
    refused(lambda: ix.mark_deleted([4, 3]), hs.HS_ERR_INVALID, "already deleted")
    refused(lambda: ix.get_row(3), hs.HS_ERR_INVALID, "Label not found")
    assert ix.deleted_count() == 1
    ix.mark_deleted([3], on=False)
    assert _answers(ix, q, k) == prior
    # Slim and SlimQ indexes take neither adds nor marks
    hs.convert_slim(hp, sp, 16)
    sx = hs.Index(sp, hs.HS_KIND_SLIM, 16, max_elements=n + 10)
    sx.set_ef(32)
    s_prior = sx.search_ids(q, k, want_dists=True)
    refused(lambda: sx.add_points(new, [n, n + 1, n + 2]), hs.HS_ERR_UNSUPPORTED, "vanilla")
    refused(lambda: sx.mark_deleted([3]), hs.HS_ERR_UNSUPPORTED, "vanilla")
    refused(lambda: sx.save(str(tmp_path / "no.bin")), hs.HS_ERR_INVALID, "no host image")
    s_after = sx.search_ids(q, k, want_dists=True)
    assert np.array_equal(s_prior["labels"], s_after["labels"]) and s_prior["dists"].tobytes() == s_after["dists"].tobytes()
    b128 = mixture(300, 128, 5, integer=True)
    h128, s128, q128 = (str(tmp_path / f) for f in ("h128.bin", "s128.bin", "q128.bin"))
    hs.build_hnsw(b128, h128, M=8, ef_construction=40, threads=4)
    hs.convert_slim(h128, s128, 128)
    hs.convert_slimq(s128, 0, 128, b128[:4].copy(), q128, threads=4)
    qx = hs.Index(q128, hs.HS_KIND_SLIMQ, 128)
    refused(lambda: qx.add_points(b128[:1], [999]), hs.HS_ERR_UNSUPPORTED, "vanilla")
    refused(lambda: qx.mark_deleted([3]), hs.HS_ERR_UNSUPPORTED, "vanilla")


def test_facade_live(hs, tmp_path):
    """tests/facade_live.cpp: loadIndex with room, markDelete / unmarkDelete / getDataByLabel / addPoint / saveIndex with the
    reference's exception texts; its answers and its saved file are the Python path's."""
    exe = os.path.join(ROOT, "hnsw-slim_amd", "facade_live")
    g = np.load(os.path.join(GOLDEN, "l2_cont_d32.npz"))
    base, q, k, every = g["base"], np.ascontiguousarray(g["queries"][:40]), 10, 7
    n, n0 = 1000, 800
    part, rf, qf, out, saved = (str(tmp_path / f) for f in ("part.bin", "rows.f32", "q.f32", "out.bin", "saved.bin"))
    hs.build_hnsw(base[:n0], part, M=8, ef_construction=100, branching_factor="4", seed=100, threads=1)
    np.ascontiguousarray(base[n0:n]).tofile(rf)
    q.tofile(qf)
    run = subprocess.run([exe, part, "32", str(n), rf, str(n - n0), str(n0), qf, str(len(q)), str(k), str(every), out, saved],
                         capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = dict(l.split(": ", 1) for l in run.stdout.strip().splitlines())
    assert lines["mark twice"] == "The requested to delete element is already deleted"
    assert lines["unmark unmarked"] == "The requested to undelete element is not deleted"
    assert lines["mark unknown"] == "Label not found" and lines["data of a deleted label"] == "Label not found"
    assert lines["add beyond max_elements"] == "The number of elements exceeds the specified limit"
    assert lines["counts"] == f"{n} {n} 0"
    # the same steps through the binding (no seed_levels: the generator after a load is the default-constructed engine in both)
    ix = hs.Index(part, hs.HS_KIND_HNSW, 32, max_elements=n)
    ix.set_ef(32)
    marks = _marked_labels(n0, every)
    ix.mark_deleted(marks)
    a = ix.search_pq(q, k)
    ix.mark_deleted(marks, on=False)
    row = ix.get_row(1)
    ix.add_points(base[n0:n], np.arange(n0, n))
    b = ix.search_pq(q, k)
    mine = str(tmp_path / "mine.bin")
    ix.save(mine)
    raw = open(out, "rb").read()
    nq, off = len(q), 0
    for r in (a, None, b):
        if r is None:
            assert raw[off:off + 128] == row.tobytes() == base[1].tobytes()
            off += 128
            continue
        assert raw[off:off + nq * k * 8] == r["labels"].tobytes(); off += nq * k * 8
        assert raw[off:off + nq * k * 4] == r["dists"].tobytes(); off += nq * k * 4
        assert raw[off:off + nq * 4] == r["cnt"].tobytes(); off += nq * 4
    assert off == len(raw)
    assert open(saved, "rb").read() == open(mine, "rb").read()


def test_facade_build_search_add_save_equals_one_build(hs, tmp_path):
    """A build-then-search caller that goes on adding: 600 rows, a search, 200 more, saveIndex == hs.build_hnsw of the 800 rows
    (the constructor's seed and the points already drawn carry over into the incremental adds)."""
    exe = os.path.join(ROOT, "hnsw-slim_amd", "facade_live")
    base = np.ascontiguousarray(np.load(os.path.join(GOLDEN, "l2_cont_d32.npz"))["base"][:800])
    rf, saved, want = (str(tmp_path / f) for f in ("rows.f32", "saved.bin", "want.bin"))
    base.tofile(rf)
    subprocess.check_call([exe, "grow", rf, "800", "32", "600", saved])
    hs.build_hnsw(base, want, M=16, ef_construction=100, branching_factor="4", seed=100, threads=1)
    assert open(saved, "rb").read() == open(want, "rb").read()
