"""convertFromHNSWWithDiff / genPatch on two resident indexes (hs_slim_convert_diff, csrc/convert_diff.hip + capi_diff.cpp) against
the host entry hs_slim_convert_diff_files, which tests/test_slim_diff_cpu.py holds to the independent Python reading: the saved Slim
image, both changed lists, the whole stream and a chunked genPatch drain, byte for byte; the shapes where the kernels can go wrong;
the fallbacks; the whole server -> client loop through hs_index_patch; marks and replace_deleted; refusals."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from hsutil import GOLDEN, ROOT, equal_key_star, load_chal_encode, load_product, mixture, write_vanilla_level0

pytestmark = pytest.mark.gpu
L2, IP = 0, 1


@pytest.fixture(scope="module")
def hs():
    m = load_product()
    m.build_library()
    return m


def _bits(ix, q, k=10, efs=(16, 70)):
    out = []
    for ef in efs:
        ix.set_ef(ef)
        r = ix.search_ids(q, k, want_dists=True, want_stats=True) if ix.kind == 1 else ix.search_pq(q, k, want_stats=True)
        out.append((r["labels"].tobytes(), r["dists"].tobytes(), r["stats"][:, :3].tobytes()))
    return out


def _drain(d, limit, to_add):
    chunks = []
    for _ in range(100000):
        b, ow, nw, fin = d.next(limit, to_add)
        chunks.append(b)
        if fin:
            return chunks
    raise AssertionError("genPatch never finished")


def _same(hs, sx, hx, old_slim, tmp, dim, metric=L2, expect_gpu=True, limit=3000, **kw):
    """One round on the resident pair (sx <- hx) against the host entry on the files of the same state.  Returns (resident diff,
    the new Slim file's path)."""
    tmp.mkdir(exist_ok=True)
    hp, res, ref = str(tmp / "now.hnsw"), str(tmp / "resident.slim"), str(tmp / "files.slim")
    hx.save(hp)
    d = sx.convert_diff(hx, **kw)
    assert d.used_gpu == expect_gpu, f"list passes on the GPU: {d.used_gpu}, expected {expect_gpu}"
    f = hs.slim_convert_diff_files(old_slim, hp, ref, dim, metric=metric, threads=4, **kw)
    sx.save_slim(res)
    assert open(res, "rb").read() == open(ref, "rb").read(), "saved Slim image"
    (go, gn), (wo, wn) = d.ids(), f.ids()
    assert go.tolist() == wo.tolist() and gn.tolist() == wn.tolist(), "changed lists"
    assert d.info() == f.info()
    assert d.stream() == f.stream(), "stream"
    d.drained = _drain(d, limit, True)     # (one drain per object: the cursors live in it; kept for a caller that patches a client)
    assert d.drained == _drain(f, limit, True), "chunked drain"
    return d, res


def _pair(hs, hp, sp, dim, metric, cap):
    return hs.Index(sp, hs.HS_KIND_SLIM, dim, metric=metric, max_elements=cap), hs.Index(hp, hs.HS_KIND_HNSW, dim, metric=metric, max_elements=cap)


@pytest.mark.parametrize("name,metric,dim", [("l2_int_d16", L2, 16), ("l2_cont_d32", L2, 32), ("ip_d48", IP, 48), ("l2_cont_d20", L2, 20)])
def test_resident_diff_equals_host_entry_on_golden_graphs(hs, tmp_path, name, metric, dim):
    """dim % 16 == 0: four lanes per row; d20: the general path; both metrics.  Two parameter sets: the defaults (level-0 lists pass
    the first prune untouched or are cut to 8) and budgets at the capacities (hubs re-pruned)."""
    hp, sp = os.path.join(GOLDEN, f"{name}.hnsw.bin"), str(tmp_path / "old.slim")
    n = int(np.frombuffer(open(hp, "rb").read(24), np.uint64)[2])
    reprunes = 0
    for r, kw in enumerate((dict(), dict(top_degree_M0=32, low_degree_m0=28, top_degree_M=16, low_degree_m=12, top_degree_percent=0.2))):
        hs.convert_slim(hp, sp, dim, metric=metric)
        sx, hx = _pair(hs, hp, sp, dim, metric, n + 8)
        d, _ = _same(hs, sx, hx, sp, tmp_path / f"r{r}", dim, metric, **kw)
        reprunes += d.info()["n_reprune"]
        assert d.info()["n_old"] > 0 and d.info()["n_new"] == 0
    assert reprunes > 0


@pytest.mark.parametrize("integer", (True, False))
def test_resident_diff_after_add_points_m16(hs, tmp_path, integer):
    dim, n0, add = 32, 2000, 64
    base = mixture(n0 + add, dim, 21, integer=integer) if integer else mixture(n0 + add, dim, 22, lo=-1, hi=1, sigma=0.4, n_clusters=4)
    hp, sp = str(tmp_path / "h.bin"), str(tmp_path / "s.bin")
    hs.build_hnsw(base[:n0], hp, M=16, ef_construction=80, threads=1)
    hs.convert_slim(hp, sp, dim)
    sx, hx = _pair(hs, hp, sp, dim, L2, n0 + add + 4)
    hx.seed_levels(100, n0)
    hx.add_points(base[n0:], np.arange(n0, n0 + add))
    kw = dict(top_degree_M0=32, low_degree_m0=30, top_degree_M=16, low_degree_m=14)
    d, new_slim = _same(hs, sx, hx, sp, tmp_path / "r1", dim, **kw)
    assert d.ids()[1].tolist() == list(range(n0, n0 + add)) and d.info()["n_reprune"] > 0
    # a second round in which nothing changed: both lists empty, the stream is its header, the device arrays are what they were
    q = base[:200]
    before = _bits(sx, q)
    d2, _ = _same(hs, sx, hx, new_slim, tmp_path / "r2", dim, **kw)
    assert d2.info()["n_old"] == 0 and d2.info()["n_new"] == 0 and d2.stream() == struct.pack("<3Q", n0 + add, 0, 0)
    assert _bits(sx, q) == before
    whole = hs.Index(new_slim, hs.HS_KIND_SLIM, dim)
    assert _bits(whole, q) == before


def _star_pair(hs, tmp_path, spokes, dim, spokes_list_centre, **kw):
    rows, lists = equal_key_star(spokes, dim=dim)
    if spokes_list_centre:
        lists = [lists[0][:32]] + [[0] for _ in range(spokes)]   # (a stored list holds at most maxM0 = 32 ids)
    hp, sp = str(tmp_path / "star.bin"), str(tmp_path / "star.slim")
    write_vanilla_level0(hp, rows, lists, M=16)
    hs.convert_slim(hp, sp, dim, **kw)
    return _pair(hs, hp, sp, dim, L2, spokes + 9) + (sp,)


@pytest.mark.parametrize("spokes", (7, 8, 9, 16, 17, 32))
def test_equal_distance_lists_around_the_budget(hs, tmp_path, spokes):
    """Node 0's level-0 list holds `spokes` ids, all at one distance, budget 8: below it the list passes untouched, from it on the
    candidates leave by descending id and the 8 largest ids stay."""
    sx, hx, sp = _star_pair(hs, tmp_path, spokes, 16, False, low_degree_m0=8)
    d, new_slim = _same(hs, sx, hx, sp, tmp_path / "r", 16, low_degree_m0=8)
    kept = load_chal_encode().parse_slim(open(new_slim, "rb").read(), 16)["lists"][0][0].tolist()
    assert kept == (list(range(1, spokes + 1)) if spokes < 8 else list(range(spokes - 7, spokes + 1)))


@pytest.mark.parametrize("spokes", (32, 33, 40))
def test_equal_distance_union_at_and_above_the_capacity(hs, tmp_path, spokes):
    """Every spoke lists the centre, so the centre's union holds `spokes` ids at one distance: exactly maxM0 = 32 is not re-pruned and
    stays in id order; above it the 32 largest ids stay, stored in the pop order of libstdc++'s heap (the emulation on one lane)."""
    kw = dict(top_degree_M0=32, low_degree_m0=32)
    sx, hx, sp = _star_pair(hs, tmp_path, spokes, 32, True, **kw)
    d, new_slim = _same(hs, sx, hx, sp, tmp_path / "r", 32, **kw)
    got = load_chal_encode().parse_slim(open(new_slim, "rb").read(), 32)["lists"][0][0].tolist()
    assert d.info()["n_reprune"] == (spokes > 32) and sorted(got) == list(range(spokes - 31, spokes + 1))
    assert (got == sorted(got)) == (spokes == 32)


def test_fallbacks_run_the_host_path_with_the_same_bytes(hs, tmp_path):
    # degree capacities above 32
    base = mixture(1500, 32, 7)
    hp, sp = str(tmp_path / "h40.bin"), str(tmp_path / "s40.bin")
    hs.build_hnsw(base, hp, M=40, ef_construction=80, threads=8)
    hs.convert_slim(hp, sp, 32)
    sx, hx = _pair(hs, hp, sp, 32, L2, 1508)
    _same(hs, sx, hx, sp, tmp_path / "m40", 32, expect_gpu=False)
    # a union beyond the on-chip buffer: one centre, 3000 points on a sphere around it, every point keeps the centre
    rng = np.random.default_rng(9)
    pts = rng.standard_normal((3000, 128)).astype(np.float32)
    pts *= np.float32(10.0) / np.linalg.norm(pts, axis=1, keepdims=True).astype(np.float32)
    base = np.concatenate([np.zeros((1, 128), np.float32), pts])
    hp, sp = str(tmp_path / "hu.bin"), str(tmp_path / "su.bin")
    hs.build_hnsw(base, hp, M=16, ef_construction=100, threads=8)
    hs.convert_slim(hp, sp, 128)
    sx, hx = _pair(hs, hp, sp, 128, L2, 3009)
    _same(hs, sx, hx, sp, tmp_path / "union", 128, expect_gpu=False)
    # a vanilla index without resident fp32 rows
    base = mixture(1200, 32, 8, integer=True)
    hp, sp = str(tmp_path / "hn.bin"), str(tmp_path / "sn.bin")
    hs.build_hnsw(base, hp, M=16, ef_construction=80, threads=8)
    hs.convert_slim(hp, sp, 32)
    sx, hx = _pair(hs, hp, sp, 32, L2, 1208)
    hx.set_row_format(hs.HS_ROWS_U8)
    hx.set_f32_resident(False)
    _same(hs, sx, hx, sp, tmp_path / "narrow", 32, expect_gpu=False)


@pytest.mark.parametrize("fmt", ("f32", "u8"))
def test_server_to_client_loop(hs, tmp_path, fmt):
    """The reference's server loop on two resident indexes: addPoint, convertFromHNSWWithDiff, genPatch chunks (with the record
    each chunk sends again) applied by hs_index_patch on a client loaded from the old file.  The client, the server's Slim index
    and an index loaded whole from the server's saved file answer alike."""
    ce = load_chal_encode()
    dim, n0, add = 32, 2000, 300
    base = mixture(n0 + add, dim, 31, integer=True)
    q = mixture(200, dim, 32, integer=True)
    hp, sp = str(tmp_path / "h.bin"), str(tmp_path / "s.bin")
    hs.build_hnsw(base[:n0], hp, M=16, ef_construction=80, threads=1)
    hs.convert_slim(hp, sp, dim)
    sx, hx = _pair(hs, hp, sp, dim, L2, n0 + add + 4)
    client = hs.Index(sp, hs.HS_KIND_SLIM, dim, max_elements=n0 + add + 4)
    if fmt == "u8":
        sx.set_row_format(hs.HS_ROWS_U8)
    before = _bits(client, q)
    hx.seed_levels(100, n0)
    hx.add_points(base[n0:], np.arange(n0, n0 + add))
    d = sx.convert_diff(hx)
    assert d.used_gpu and d.info()["n_new"] == add and d.info()["n_old"] > 0
    chunks = _drain(d, 20000, True)
    assert len(chunks) >= 3
    sent = 0
    for c in chunks:
        sent += sum(struct.unpack_from("<2Q", c, 8))
        client.patch(c, to_add=True)
    assert sent == d.info()["n_old"] + d.info()["n_new"] + len(chunks) - 1   # every chunk but the last sends its last record again
    saved = str(tmp_path / "server.slim")
    sx.save_slim(saved)
    whole = hs.Index(saved, hs.HS_KIND_SLIM, dim)
    if fmt == "u8":
        whole.set_row_format(hs.HS_ROWS_U8)
    assert sx.info()["n"] == n0 + add and _bits(sx, q) == _bits(whole, q)
    # the patch stream does not move the enter point: the client answers as the new file with the old entry
    want = str(tmp_path / "expect.slim")
    open(want, "wb").write(ce.with_entry_of(open(saved, "rb").read(), open(sp, "rb").read()))
    ref = hs.Index(want, hs.HS_KIND_SLIM, dim)
    got = _bits(client, q)
    assert got == _bits(ref, q) and got != before


def test_marks_and_replace_deleted_on_the_vanilla_side(hs, tmp_path):
    dim, n0 = 32, 1500
    base = mixture(n0 + 1, dim, 41, integer=True)
    hp, sp = str(tmp_path / "h.bin"), str(tmp_path / "s.bin")
    hs.build_hnsw(base[:n0], hp, M=16, ef_construction=80, threads=1)
    hs.convert_slim(hp, sp, dim)
    sx, hx = _pair(hs, hp, sp, dim, L2, n0 + 4)
    _same(hs, sx, hx, sp, tmp_path / "r0", dim)
    sx.save_slim(str(tmp_path / "s1.bin"))
    assert sx.info()["has_deleted"] == 0
    hx.set_replace_deleted(True)
    hx.mark_deleted([7])
    new_row = np.clip(base[n0:] + 3, 0, 255)
    hx.upsert_points(new_row, [9000], replace_deleted=[1])   # takes slot 7
    hx.mark_deleted([11])
    d, new_slim = _same(hs, sx, hx, str(tmp_path / "s1.bin"), tmp_path / "r1", dim)
    assert sx.info()["has_deleted"] == 1 and sx.info()["n"] == n0
    raw = open(new_slim, "rb").read()
    g = load_chal_encode().parse_slim(raw, dim)
    assert g["has_deleted"] and int(g["labels"][7]) == 9000 and d.ids()[1].tolist() == []
    # the reused slot's row and label were rewritten on the server's device copy (its row came from the vanilla index's resident
    # array); no Slim node is marked: node 11, marked on the vanilla side, is still found, under has_deleted = 1
    sx.set_ef(32)
    r = sx.search_ids(np.concatenate([new_row, base[11:12]]), 1, want_dists=True)
    assert r["labels"][:, 0].tolist() == [9000, 11] and r["dists"][:, 0].tolist() == [0.0, 0.0]


def test_refusals_leave_both_indexes_untouched(hs, tmp_path):
    dim, n0 = 16, 600
    base = mixture(n0 + 20, dim, 51, integer=True)
    q = base[:100]
    hp, sp = str(tmp_path / "h.bin"), str(tmp_path / "s.bin")
    hs.build_hnsw(base[:n0], hp, M=16, ef_construction=60, threads=1)
    hs.convert_slim(hp, sp, dim)
    sx, hx = _pair(hs, hp, sp, dim, L2, n0 + 10)
    big = hs.Index(hp, hs.HS_KIND_HNSW, dim, max_elements=n0 + 30)
    big.add_points(base[n0:], np.arange(n0, n0 + 20))
    fixed_s, fixed_h = hs.Index(sp, hs.HS_KIND_SLIM, dim), hs.Index(hp, hs.HS_KIND_HNSW, dim)
    state = lambda: (_bits(sx, q), _bits(hx, q), _bits(big, q), sx.info(), hx.info())   # noqa: E731
    prior = state()

    def refused(fn, status):
        with pytest.raises(hs.HsError) as e:
            fn()
        assert e.value.status == status, str(e.value)
        assert state() == prior

    refused(lambda: sx.convert_diff(big), hs.HS_ERR_CAPACITY)      # 620 elements into a Slim index with room for 610
    refused(lambda: sx.convert_diff(sx), hs.HS_ERR_INVALID)        # wrong kinds
    refused(lambda: hx.convert_diff(hx), hs.HS_ERR_INVALID)
    refused(lambda: fixed_s.convert_diff(hx), hs.HS_ERR_INVALID)   # loaded without room
    refused(lambda: sx.convert_diff(fixed_h), hs.HS_ERR_INVALID)
    # a Slim index in u8 row format and a new row it cannot hold: refused after the diff kernel named the rows, nothing changed
    sx8, hx8 = _pair(hs, hp, sp, dim, L2, n0 + 10)
    sx8.set_row_format(hs.HS_ROWS_U8)
    bad = base[n0:n0 + 1].copy()
    bad[0, 3] = 300.5
    hx8.add_points(bad, [n0])
    prior8 = (_bits(sx8, q), sx8.info())
    with pytest.raises(hs.HsError) as e:
        sx8.convert_diff(hx8)
    assert e.value.status == hs.HS_ERR_UNSUPPORTED and "300.5" in str(e.value), str(e.value)
    assert (_bits(sx8, q), sx8.info()) == prior8
    # `cap` too small in next, on the resident diff: the needed size comes back, its cursors stay, the index is untouched
    d = sx.convert_diff(hx)
    after = _bits(sx, q)
    info = d.info()
    assert info["n_old"] > 0
    with pytest.raises(hs.HsError) as e:
        d.next(1 << 20, True, cap=8)
    assert e.value.status == hs.HS_ERR_CAPACITY
    need = int(re.search(r"(\d+) bytes needed", str(e.value)).group(1))
    with pytest.raises(hs.HsError) as e:
        d.next(1 << 20, True, cap=need - 1)
    assert e.value.status == hs.HS_ERR_CAPACITY and str(need) in str(e.value)
    got, ow, nw, fin = d.next(1 << 20, True, cap=need)
    assert (len(got), ow, nw, fin) == (need, info["n_old"], info["n_new"], True) and _bits(sx, q) == after
    assert got == hs.slim_convert_diff_files(sp, hp, str(tmp_path / "o.bin"), dim).next(1 << 20, True)[0]
    # a diff object serves until the next conversion of its index
    d_next = sx.convert_diff(hx)
    with pytest.raises(hs.HsError) as e:
        d.stream()
    assert e.value.status == hs.HS_ERR_INVALID and d_next.info()["n_old"] == 0 and d_next.stream() == struct.pack("<3Q", n0, 0, 0)


def test_facade_server_loop(hs, tmp_path):
    """tests/facade_diff.cpp: the three facade methods against the expectations of test_server_to_client_loop, for one graph."""
    ce = load_chal_encode()
    exe = os.path.join(ROOT, "hnsw-slim_amd", "facade_diff")
    dim, n0, add, k = 32, 2000, 300, 10
    base = mixture(n0 + add, dim, 61, integer=True)
    q = mixture(100, dim, 62, integer=True)
    hp, sp, rf, qf, prefix = (str(tmp_path / x) for x in ("h.bin", "s.bin", "rows.f32", "q.f32", "out"))
    hs.build_hnsw(base[:n0], hp, M=16, ef_construction=80, threads=1)
    hs.convert_slim(hp, sp, dim)
    base[n0:].tofile(rf)
    q.tofile(qf)
    run = subprocess.run([exe, hp, sp, str(dim), str(n0 + add + 4), rf, str(add), str(n0), "20000", qf, str(len(q)), str(k), prefix],
                         capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    fig = {a: int(b) for a, b in (l.split(": ", 1) for l in run.stdout.strip().splitlines())}
    assert fig["n_new"] == add and fig["ids"] == add and fig["n_old"] > 0 and fig["chunks"] >= 3
    assert fig["sent"] == fig["n_old"] + fig["n_new"] + fig["chunks"] - 1
    # the whole stream and the saved Slim file are the host entry's on the same files
    f = hs.slim_convert_diff_files(sp, prefix + ".hnsw", str(tmp_path / "files.slim"), dim, threads=4)
    assert open(prefix + ".stream", "rb").read() == f.stream()
    assert open(prefix + ".slim", "rb").read() == open(str(tmp_path / "files.slim"), "rb").read()
    assert (f.info()["n_old"], f.info()["n_new"]) == (fig["n_old"], fig["n_new"])
    # server == the saved file loaded whole; client == that file with the old entry
    want = str(tmp_path / "expect.slim")
    open(want, "wb").write(ce.with_entry_of(open(prefix + ".slim", "rb").read(), open(sp, "rb").read()))
    whole, ref = hs.Index(prefix + ".slim", hs.HS_KIND_SLIM, dim), hs.Index(want, hs.HS_KIND_SLIM, dim)
    res = open(prefix + ".res", "rb").read()
    per = len(q) * k * 8 + len(q) * 16
    assert len(res) == 4 * per
    for e, ef in enumerate((16, 70)):
        for j, x in enumerate((whole, ref)):
            x.set_ef(ef)
            r = x.search_ids(q, k, want_dists=True, want_stats=True)
            blk = res[(2 * e + j) * per:(2 * e + j + 1) * per]
            assert blk[:len(q) * k * 4] == r["labels"].tobytes() and blk[len(q) * k * 4:len(q) * k * 8] == r["dists"].tobytes()
            got_stats = np.frombuffer(blk, np.uint32, len(q) * 4, len(q) * k * 8).reshape(-1, 4)
            assert np.array_equal(got_stats[:, :3], r["stats"][:, :3])


def test_device_diff_equals_host_diff_through_relabelled_slots(hs, tmp_path):
    """The diff kernel + compaction + the label lookup of the flagged nodes against the host classification over ALL nodes, on two
    server pairs that take the same operations: one on the device path, one whose vanilla index has dropped its fp32 rows (host
    path).  The operations move labels between slots: label 7 leaves slot 7 (which takes label 9000) and later comes back at slot
    20.  The Slim index's label_lookup_ still maps 7 -> 7 (merge never overwrites), so node 20 is NEW although its id is old
    (hnswalg_slim.h:1360-1362) -- which two files cannot tell, and both resident paths must."""
    dim, n0 = 32, 1500
    base = mixture(n0 + 40, dim, 71, integer=True)
    q = base[:100]
    hp, sp = str(tmp_path / "h.bin"), str(tmp_path / "s.bin")
    hs.build_hnsw(base[:n0], hp, M=16, ef_construction=80, threads=1)
    hs.convert_slim(hp, sp, dim)
    pairs = []
    for on_device in (True, False):
        sx, hx = _pair(hs, hp, sp, dim, L2, n0 + 44)
        hx.set_replace_deleted(True)
        hx.seed_levels(100, n0)
        if not on_device:
            hx.set_row_format(hs.HS_ROWS_U8)
            hx.set_f32_resident(False)
        pairs.append((sx, hx))
    rows = np.clip(base[n0:n0 + 2] + 2, 0, 255)
    steps = [lambda hx: hx.add_points(base[n0 + 2:], np.arange(n0 + 2, n0 + 40)),
             lambda hx: (hx.mark_deleted([7]), hx.upsert_points(rows[:1], [9000], replace_deleted=[1])),
             lambda hx: (hx.mark_deleted([20]), hx.upsert_points(rows[1:], [7], replace_deleted=[1])),
             lambda hx: None]
    for k, step in enumerate(steps):
        res = []
        for (sx, hx), on_device in zip(pairs, (True, False)):
            step(hx)
            d = sx.convert_diff(hx)
            assert d.used_gpu == on_device
            out = str(tmp_path / f"s{k}_{int(on_device)}.bin")
            sx.save_slim(out)
            res.append((d.ids()[0].tolist(), d.ids()[1].tolist(), d.info(), d.stream(), _drain(d, 4000, True), open(out, "rb").read(),
                        _bits(sx, q)))
        assert res[0] == res[1], f"step {k}"
        old_ids, new_ids = res[0][0], res[0][1]
        if k == 0:
            assert new_ids == list(range(n0, n0 + 38)) and old_ids
        elif k == 1:
            assert new_ids == []               # slot 7 took a label the Slim index had never seen: an old node
        elif k == 2:
            assert new_ids == [20] and 20 not in old_ids
        else:
            assert new_ids == [20] and old_ids == []   # nothing changed, and node 20 is new again: the lookup still disagrees
