"""GPU tests (MI355X) of the batched add into a resident vanilla index (hs_index_add_points_batched): the device path
against its host twin (hs_hnsw_resume_batched) byte for byte through Index.save(), a split build against the whole device build,
batch_max = 1 against add_points(threads=1) and the compiled reference's file, the resident index against its own saved file loaded
afresh, the re-run / long-segment / re-tile paths, tiny inputs, the compaction of the changed lists, refusals, the facade, and the
edges of the device path's envelope and of the fp32 range."""
import os
import struct
import subprocess

import numpy as np
import pytest

import batch_build_cases as C
from hsutil import GOLDEN, ROOT, load_product, mixture

pytestmark = pytest.mark.gpu
L2, IP = 0, 1
SEED = 100


@pytest.fixture(scope="module")
def hs():
    m = load_product()
    assert m.device_count() > 0, "no HIP device"
    return m


def read(p):
    with open(p, "rb") as f:
        return f.read()


SHAPES = {
    "l2_d32": lambda: (mixture(3000, 32, 11), L2, 8, 100),
    "l2_d64": lambda: (mixture(4000, 64, 11), L2, 16, 200),
    "ip_d48": lambda: (mixture(2000, 48, 11), IP, 8, 100),
    "l2_int_d16": lambda: (mixture(3000, 16, 11, integer=True), L2, 8, 100),
    "l2_d20": lambda: (mixture(1500, 20, 11), L2, 8, 100),     # a dim outside the % 16 recipes
}
_prefix = {}


def prefix_file(hs, tmp_path_factory, name):
    """The host twin's build of the first half of a shape, once for the module (read only afterwards)."""
    if name not in _prefix:
        base, metric, M, efc = SHAPES[name]()
        p = str(tmp_path_factory.mktemp("prefix") / "p.bin")
        hs.build_hnsw_batched(base[:len(base) // 2], p, metric=metric, M=M, ef_construction=efc, seed=SEED, device=-1, threads=16)
        _prefix[name] = p
    return _prefix[name]


def add_both(hs, tmp_path, part, base, n0, metric=L2, labels=None, load=None, **kw):
    """The rows base[n0:] added to the index file `part`: (twin's file bytes, the resident index after the device add, its stats)."""
    n, dim = base.shape
    labels = np.arange(n0, n) if labels is None else labels
    t = str(tmp_path / "twin.bin")
    hs.hnsw_resume_batched(part, t, base[n0:], labels, metric=metric, max_elements=n, seed=SEED, drawn=n0, threads=16,
                           **{k: v for k, v in kw.items() if k != "scratch_ids"})
    ix = load() if load else hs.Index(part, hs.HS_KIND_HNSW, dim, metric=metric, max_elements=n)
    ix.seed_levels(SEED, n0)
    st = ix.add_points_batched(base[n0:], labels, device=0, **kw)
    return read(t), ix, st


def saved(ix, tmp_path, name="saved.bin"):
    p = str(tmp_path / name)
    ix.save(p)
    return read(p)


@pytest.mark.parametrize("batch_max", [0, 64])
@pytest.mark.parametrize("name", list(SHAPES))
def test_device_equals_twin(hs, tmp_path, tmp_path_factory, name, batch_max):
    base, metric, M, efc = SHAPES[name]()
    n0 = len(base) // 2
    t, ix, st = add_both(hs, tmp_path, prefix_file(hs, tmp_path_factory, name), base, n0, metric=metric, batch_max=batch_max)
    assert st["used_gpu"] and st["batches"] > 1 and ix.info()["n"] == len(base)
    assert saved(ix, tmp_path) == t


def test_split_equals_whole_on_the_device(hs, tmp_path):
    """The prefix up to a batch boundary built, loaded with room for the rest, seeded, the rest added on the device == the whole
    build on the device.  Row 1310 (level 5) raises the top level inside the add: info() shows the moved entry point."""
    base = mixture(3000, 32, 11)
    s = hs.build_schedule(3000, M=8, seed=SEED)
    begins = [0] + [int(x) for x in np.cumsum(s["sizes"])]
    assert 1029 in begins and 1310 in begins and int(s["sizes"][begins.index(1310)]) == 1
    part, whole = str(tmp_path / "part.bin"), str(tmp_path / "whole.bin")
    hs.build_hnsw_batched(base[:1029], part, M=8, ef_construction=100, seed=SEED, device=-1, threads=16)
    st = hs.build_hnsw_batched(base, whole, M=8, ef_construction=100, seed=SEED, device=0)
    assert st["used_gpu"]
    ix = hs.Index(part, hs.HS_KIND_HNSW, 32, max_elements=3000)
    before = ix.info()
    assert before["maxlevel"] == 4 and before["enterpoint"] < 1029
    ix.seed_levels(SEED, 1029)
    st = ix.add_points_batched(base[1029:], np.arange(1029, 3000), device=0)
    assert st["used_gpu"] and st["batches"] == len(begins) - 1 - begins.index(1029)
    assert saved(ix, tmp_path) == read(whole)
    assert ix.info()["enterpoint"] == 1310 and ix.info()["maxlevel"] == 5


@pytest.mark.parametrize("name,dim", [("l2_cont_d32", 32), ("l2_int_d16", 16)])
def test_batch_1_on_the_device(hs, tmp_path, name, dim):
    """batch_max = 1 is the serial addPoint loop: rows 300 .. 600 on the device == add_points(threads=1) on a second index loaded
    from the same prefix file; carried on to the fixture's last row it is the compiled reference's file."""
    g = np.load(os.path.join(GOLDEN, f"{name}.npz"))
    base, M, efc = g["base"], int(g["M"]), int(g["efC"])
    n = base.shape[0]
    part = str(tmp_path / "part.bin")
    hs.build_hnsw(base[:300], part, M=M, ef_construction=efc, branching_factor="4", seed=100, threads=1)
    ix, other = (hs.Index(part, hs.HS_KIND_HNSW, dim, max_elements=n) for _ in range(2))
    ix.seed_levels(100, 300); other.seed_levels(100, 300)
    st = ix.add_points_batched(base[300:600], np.arange(300, 600), device=0, batch_max=1)
    other.add_points(base[300:600], np.arange(300, 600), threads=1)
    assert st["used_gpu"] and st["batches"] == 300
    assert saved(ix, tmp_path, "a.bin") == saved(other, tmp_path, "b.bin")
    st = ix.add_points_batched(base[600:], np.arange(600, n), device=0, batch_max=1)
    assert st["used_gpu"] and st["batches"] == n - 600
    assert saved(ix, tmp_path, "a.bin") == read(os.path.join(GOLDEN, f"{name}.hnsw.bin"))


def answers(ix, q, k=10, ef=64):
    ix.set_ef(ef)
    r = ix.search_pq(q, k, want_stats=True)
    return r["labels"].tobytes(), r["dists"].tobytes(), r["cnt"].tobytes(), np.ascontiguousarray(r["stats"][:, :3]).tobytes()


INFO_FIELDS = ("n", "maxlevel", "enterpoint", "n_edges", "max_degree0", "index_size", "has_deleted")


def info(ix):
    i = ix.info()
    return {f: i[f] for f in INFO_FIELDS}


def load_as(hs, path, dim, fmt, free, max_elements=0):
    if free:
        return hs.Index.load_narrow(path, hs.HS_KIND_HNSW, dim, fmt, max_elements=max_elements)
    ix = hs.Index(path, hs.HS_KIND_HNSW, dim, max_elements=max_elements)
    if fmt != hs.HS_ROWS_F32:
        ix.set_row_format(fmt)
    return ix


@pytest.mark.parametrize("name,fmt,free", [("l2_d32", "f32", False), ("l2_int_d16", "f32", False), ("l2_int_d16", "u8", False),
                                           ("l2_int_d16", "u8", True)])
def test_add_equals_load_whole(hs, tmp_path, tmp_path_factory, name, fmt, free):
    """After the add the resident index answers as a fresh index loaded from its own saved file: labels, fp32 distance bits, counts
    and the three counters at ef 64, on the flat kernel on both sides.  With u8 rows beside the fp32 rows the device path writes the
    narrow rows too; an fp32-free index has no rows for the build kernels: the twin serves it, with the same bytes and answers."""
    base, metric, M, efc = SHAPES[name]()
    n, dim = base.shape
    n0 = n // 2
    q = mixture(64, dim, 12, integer=(name == "l2_int_d16"))
    f = {"f32": hs.HS_ROWS_F32, "u8": hs.HS_ROWS_U8}[fmt]
    part = prefix_file(hs, tmp_path_factory, name)
    t, ix, st = add_both(hs, tmp_path, part, base, n0, metric=metric, load=lambda: load_as(hs, part, dim, f, free, max_elements=n))
    assert bool(st["used_gpu"]) == (not free)
    sp = str(tmp_path / "saved.bin")
    ix.save(sp)
    assert read(sp) == t
    fresh = load_as(hs, sp, dim, f, free)
    assert info(ix) == info(fresh) and np.array_equal(ix.labels(), fresh.labels())
    assert answers(ix, q) == answers(fresh, q)
    flat = {"f32": "hs::flat_kernel", "u8": "hs::flat_kernel_u8"}[fmt]
    assert ix.last_kernel() == flat and fresh.last_kernel() == flat
    for lab in (0, n0 - 1, n0, n - 1):
        assert ix.get_row(lab).tobytes() == fresh.get_row(lab).tobytes()


def test_rerun_path(hs, tmp_path, tmp_path_factory):
    base, metric, M, efc = SHAPES["l2_d32"]()
    t, ix, st = add_both(hs, tmp_path, prefix_file(hs, tmp_path_factory, "l2_d32"), base, len(base) // 2, scratch_ids=64)
    assert st["used_gpu"] and st["flagged_rows"] > 0
    assert saved(ix, tmp_path) == t


def test_added_rows_into_the_same_few_targets(hs, tmp_path):
    """A spread-out resident prefix, then the added rows from one tight cluster: whole batches pick the same few targets, whose
    lists overflow more than once per batch and whose incoming ids outnumber a wavefront (the link kernel's long-segment path)."""
    n = 3000
    sizes = hs.build_schedule(n, M=4, seed=SEED)["sizes"]
    begins = np.concatenate([[0], np.cumsum(sizes, dtype=np.int64)[:-1]])
    b = int(np.argmax(begins >= 1500))
    prefix = int(begins[b])
    assert sizes[b] > 64 and prefix + sizes[b] <= n     # the add begins with a batch of more than 64 rows
    rng = np.random.default_rng(5)
    spread = mixture(prefix, 16, 6)
    tight = (spread[7] + rng.normal(0, 0.01, (n - prefix, 16))).astype(np.float32)
    base = np.ascontiguousarray(np.concatenate([spread, tight]))
    part = str(tmp_path / "part.bin")
    hs.build_hnsw_batched(spread, part, M=4, ef_construction=40, seed=SEED, device=-1, threads=16)
    t, ix, st = add_both(hs, tmp_path, part, base, prefix)
    assert st["used_gpu"] and st["batches"] == len(sizes) - b
    assert saved(ix, tmp_path) == t


def test_add_through_the_retile_path(hs, tmp_path):
    """An M = 16 graph of ten points (level-0 degrees below 16: tile stride 16) grown past it inside one batched add: write_changed
    re-tiles everything; the index then equals its saved file loaded afresh."""
    base, q = mixture(1500, 16, 311, integer=True), mixture(64, 16, 312, integer=True)
    part = str(tmp_path / "part.bin")
    hs.build_hnsw_batched(base[:10], part, M=16, ef_construction=80, seed=SEED, device=-1)
    probe = hs.Index(part, hs.HS_KIND_HNSW, 16, max_elements=1500)
    assert probe.info()["max_degree0"] <= 16
    t, ix, st = add_both(hs, tmp_path, part, base, 10)
    assert st["used_gpu"] and ix.info()["max_degree0"] > 16
    sp = str(tmp_path / "saved.bin")
    ix.save(sp)
    assert read(sp) == t
    fresh = hs.Index(sp, hs.HS_KIND_HNSW, 16)
    assert info(ix) == info(fresh) and ix.info()["device_bytes"] == fresh.info()["device_bytes"]
    assert answers(ix, q) == answers(fresh, q)


@pytest.mark.parametrize("n0,count", [(1, 1), (2, 300)])
def test_tiny(hs, tmp_path, n0, count):
    base = mixture(n0 + count, 16, 3)
    part = str(tmp_path / "part.bin")
    hs.build_hnsw_batched(base[:n0], part, M=4, ef_construction=20, seed=SEED, device=-1)
    t, ix, st = add_both(hs, tmp_path, part, base, n0)
    assert st["used_gpu"] and ix.info()["n"] == n0 + count
    assert saved(ix, tmp_path) == t


def test_identical_rows_added_to_identical_rows(hs, tmp_path):
    base = np.tile(mixture(1, 16, 4), (600, 1))
    part = str(tmp_path / "part.bin")
    hs.build_hnsw_batched(base[:300], part, M=4, ef_construction=20, seed=SEED, device=-1)
    t, ix, st = add_both(hs, tmp_path, part, base, 300)
    assert st["used_gpu"] and saved(ix, tmp_path) == t


def list_bytes(raw, dim):
    """Per node of a saveIndex file: the bytes of its level-0 list slot and of its upper lists."""
    (_, _, count, spe, _, data_off) = struct.unpack_from("<6Q", raw, 0)
    out = []
    off = 96 + count * spe
    for i in range(count):
        (sz,) = struct.unpack_from("<I", raw, off)
        out.append((raw[96 + i * spe:96 + i * spe + data_off], raw[off + 4:off + 4 + sz]))
        off += 4 + sz
    assert off == len(raw)
    return out


@pytest.mark.parametrize("count", [10, 1500])
def test_only_the_changed_lists_come_back(hs, tmp_path, count):
    """What the device path downloads beside the new nodes: exactly the old nodes whose level-0 or upper list bytes differ between
    the host image before and after -- far fewer than the index holds when ten rows are added to 2990."""
    base = mixture(3000, 32, 11)
    n0 = 3000 - count
    part = str(tmp_path / "part.bin")
    hs.build_hnsw_batched(base[:n0], part, M=8, ef_construction=100, seed=SEED, device=-1, threads=16)
    ix = hs.Index(part, hs.HS_KIND_HNSW, 32, max_elements=3000)
    ix.seed_levels(SEED, n0)
    before = list_bytes(saved(ix, tmp_path, "before.bin"), 32)
    st = ix.add_points_batched(base[n0:], np.arange(n0, 3000), device=0)
    assert st["used_gpu"]
    after = list_bytes(saved(ix, tmp_path, "after.bin"), 32)
    differ = [i for i in range(n0) if before[i] != after[i]]
    got, downloaded = ix.batched_add_changed()
    print(f"{count} rows into {n0}: {downloaded} old lists downloaded, {len(got)} old nodes changed, {len(differ)} differ")
    assert list(map(int, got)) == differ
    # every changed list received an id (a list that received one and came back with its old bytes -- a full list whose re-prune
    # turned the new id away -- is downloaded and left alone); a row sends at most M = 8 ids per level it is inserted on
    assert len(differ) <= downloaded <= count * 8 * (ix.info()["maxlevel"] + 1)
    if count == 10:
        assert 0 < downloaded < 3000 // 4     # far fewer than the 2990 level-0 lists the index holds
    # the host twin downloads nothing
    other = hs.Index(part, hs.HS_KIND_HNSW, 32, max_elements=3000)
    other.seed_levels(SEED, n0)
    st = other.add_points_batched(base[n0:], np.arange(n0, 3000), device=-1, threads=8)
    assert not st["used_gpu"] and (len(other.batched_add_changed()[0]), other.batched_add_changed()[1]) == (0, 0)
    assert saved(other, tmp_path, "twin.bin") == saved(ix, tmp_path, "after.bin")


def test_refusals_leave_the_index_bit_identical(hs, tmp_path):
    g = np.load(os.path.join(GOLDEN, "l2_int_d16.npz"))
    base, q = g["base"], g["queries"]
    n = base.shape[0]
    hp, sp = os.path.join(GOLDEN, "l2_int_d16.hnsw.bin"), str(tmp_path / "s.bin")
    ix = hs.Index(hp, hs.HS_KIND_HNSW, 16, max_elements=n + 10)
    full = hs.Index(hp, hs.HS_KIND_HNSW, 16)
    new = base[:3] + 1
    prior, prior_full, prior_file = answers(ix, q), answers(full, q), saved(ix, tmp_path, "prior.bin")

    def refused(fn, status, text):
        with pytest.raises(hs.HsError) as e:
            fn()
        assert e.value.status == status and text in str(e.value), str(e.value)

    for device in (0, -1):
        refused(lambda: full.add_points_batched(new, [n, n + 1, n + 2], device=device), hs.HS_ERR_CAPACITY, "exceeds the specified limit")
        refused(lambda: ix.add_points_batched(np.repeat(new, 4, axis=0), np.arange(n, n + 12), device=device), hs.HS_ERR_CAPACITY,
                "exceeds the specified limit")
        refused(lambda: ix.add_points_batched(new, [n, 5, n + 2], device=device), hs.HS_ERR_UNSUPPORTED, "already exists")
        refused(lambda: ix.add_points_batched(new, [n, n + 1, n], device=device), hs.HS_ERR_INVALID, "appears twice")
    refused(lambda: ix.add_points_batched(new, [n, n + 1, n + 2], device=1 + ix.device), hs.HS_ERR_INVALID, "own device")
    refused(lambda: ix.add_points_batched(new, [n, n + 1, n + 2], scratch_ids=100), hs.HS_ERR_INVALID, "scratch_ids")
    assert ix.info()["n"] == n and answers(ix, q) == prior and saved(ix, tmp_path, "now.bin") == prior_file
    assert answers(full, q) == prior_full
    # delete marks: refused on the device and on the twin alike, the message names the call that takes such an index
    ix.mark_deleted([3])
    marked, marked_file = answers(ix, q), saved(ix, tmp_path, "marked.bin")
    for device in (0, -1):
        refused(lambda: ix.add_points_batched(new, [n, n + 1, n + 2], device=device), hs.HS_ERR_UNSUPPORTED, "hs_index_add_points")
    assert ix.info()["n"] == n and ix.deleted_count() == 1
    assert answers(ix, q) == marked and saved(ix, tmp_path, "now.bin") == marked_file
    ix.mark_deleted([3], on=False)
    assert answers(ix, q) == prior
    st = ix.add_points_batched(new, [n, n + 1, n + 2])     # with the mark gone the same call goes through, on the index's device
    assert st["used_gpu"] and ix.info()["n"] == n + 3
    # a Slim index
    hs.convert_slim(hp, sp, 16)
    sx = hs.Index(sp, hs.HS_KIND_SLIM, 16, max_elements=n + 10)
    sx.set_ef(32)
    s_prior = sx.search_ids(q, 10, want_dists=True)
    refused(lambda: sx.add_points_batched(new, [n, n + 1, n + 2]), hs.HS_ERR_UNSUPPORTED, "vanilla")
    s_after = sx.search_ids(q, 10, want_dists=True)
    assert np.array_equal(s_prior["labels"], s_after["labels"]) and s_prior["dists"].tobytes() == s_after["dists"].tobytes()


def test_facade_batched_add(hs, tmp_path):
    """tests/facade_batched_add.cpp: addPoints with setBuildOnDevice(0, 1) in force is the batched add at batch_max = 1 -- the serial
    order, so the labels and the saved bytes of a run without it (a loop of addPoint); at the default schedule the device's stats."""
    exe = os.path.join(ROOT, "hnsw-slim_amd", "facade_batched_add")
    base, q = mixture(800, 32, 11), mixture(40, 32, 12)
    part, rf, qf = (str(tmp_path / f) for f in ("part.bin", "rows.f32", "q.f32"))
    hs.build_hnsw(base[:500], part, M=8, ef_construction=100, branching_factor="4", seed=100, threads=1)
    base[500:].tofile(rf); q.tofile(qf)
    outs, files = [], []
    for device in ("0", "-1"):
        out, sav = str(tmp_path / f"out{device}.bin"), str(tmp_path / f"saved{device}.bin")
        run = subprocess.run([exe, part, "800", rf, "300", "32", device, "1", qf, "40", "10", out, sav], capture_output=True, text=True)
        assert run.returncode == 0, run.stdout + run.stderr
        assert run.stdout.split() == (["add:", "1", "300", "0", "800"] if device == "0" else ["add:", "0", "0", "0", "800"]), run.stdout
        outs.append(read(out)); files.append(read(sav))
    assert outs[0] == outs[1] and files[0] == files[1]
    labels = np.frombuffer(outs[0], np.uint64, 40 * 10).reshape(40, 10)
    assert labels.max() >= 5000 and set(labels.ravel().tolist()) <= set(range(500)) | set(range(5000, 5300))
    out, sav = str(tmp_path / "out_d.bin"), str(tmp_path / "saved_d.bin")
    run = subprocess.run([exe, part, "800", rf, "300", "32", "0", "0", qf, "40", "10", out, sav], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    w = run.stdout.split()
    assert w[:2] == ["add:", "1"] and 1 < int(w[2]) < 300 and w[4] == "800", run.stdout


# ---- the edges of the device path's envelope, and of the fp32 range (device against twin: these need fp32 rows) -------------------------
@pytest.mark.parametrize("name,M,efc,dim,scratch_ids", [("M31_efc512", 31, 512, 32, 0), ("M31_efc31", 31, 31, 32, 0), ("M2", 2, 10, 16, 0),
                                                        ("dim1", 8, 40, 1, 0), ("dim23", 8, 40, 23, 0), ("dim960", 8, 40, 960, 0),
                                                        ("scratch8192", 8, 100, 32, 8192)])
def test_envelope(hs, tmp_path, name, M, efc, dim, scratch_ids):
    """The edges of gpu_build_supported (M = kBgMaxM, ef_construction = kBgMaxEfc and = M, M = 2, odd and large dims, the largest
    scratch_ids) as an add of the second half of 1000 rows."""
    base = mixture(1000, dim, 11)
    part = str(tmp_path / "part.bin")
    hs.build_hnsw_batched(base[:500], part, M=M, ef_construction=efc, seed=SEED, device=-1, threads=16)
    kw = dict(scratch_ids=scratch_ids) if scratch_ids else {}
    t, ix, st = add_both(hs, tmp_path, part, base, 500, **kw)
    assert st["used_gpu"] and ix.info()["n"] == 1000
    assert saved(ix, tmp_path) == t


def test_envelope_fallback_at_M_32(hs, tmp_path):
    base = mixture(400, 16, 8)
    part = str(tmp_path / "part.bin")
    hs.build_hnsw_batched(base[:200], part, M=32, ef_construction=64, seed=SEED, device=-1, threads=16)
    t, ix, st = add_both(hs, tmp_path, part, base, 200)
    assert not st["used_gpu"] and saved(ix, tmp_path) == t


@pytest.mark.parametrize("batch_max", [0, 64])
@pytest.mark.parametrize("case", C.vr_cases(), ids=C.vr_name)
def test_value_range(hs, oracle, tmp_path, case, batch_max):
    """The families of tests/value_range.py as an add of the second half of 600 rows meets them (M 8, ef_construction 60); the
    family's premise holds on the rows' own distance table (asserted)."""
    rows = C.vr_rows(case)
    C.vr_check_premise(oracle, case, rows)
    part = str(tmp_path / "part.bin")
    hs.build_hnsw_batched(rows[:300], part, metric=case[1], M=C.VR_M, ef_construction=C.VR_EFC, seed=SEED, device=-1, threads=16)
    t, ix, st = add_both(hs, tmp_path, part, rows, 300, metric=case[1], batch_max=batch_max)
    assert st["used_gpu"] and saved(ix, tmp_path) == t
