"""GPU tests (MI355X) of random update sequences on a resident vanilla index: >= 100 interleaved marks, unmarks, updates, appends,
bursts of addPoint(.., true) and resizes (tests/golden/updates_seq_<name>.npz, see tests/live_sequences.py), pinned to the compiled
reference at two or three checkpoints each.

What the hand-written scenarios of test_gpu_live_upsert.py leave open is what these are there for: the update kernel's narrow-row
writer off the identity permutation (W32 .. W960: d = 32, 128, 320, 960; at d = 16 narrow_slot(j) == j), start graphs that carry
marks with replacement on (G3, G4), mixed flagged / unflagged adds in one hs_index_upsert_points call, a tile stride that grows in
mid-sequence (T), and the device copy behind write_changed: the saved file comes from the host image, so every checkpoint also
searches -- the flat kernel reads tile0, the others the re-packed CSR -- and compares with a fresh load of that file."""
import os
import struct

import numpy as np
import pytest

from hsutil import Oracle, load_chal_encode, load_product
from live_sequences import ADD, INTEGER, NAMES, RESIZE, file_sha, pq_sorted, sequence, start_file
from test_gpu_exact_search import references, same
from test_gpu_live_upsert import _answers, _apply, _check_against_reference, _info, _load
from test_gpu_slim_diff import _bits, _same

pytestmark = pytest.mark.gpu
L2 = 0
# row state -> (format, without fp32 rows)
STATES = {"f32": ("f32", False), "u8+f32": ("u8", False), "u8": ("u8", True), "f16": ("f16", True)}
CASES = [(n, st) for n in NAMES for st in (STATES if n in INTEGER and n != "W960" else ("f32", "u8") if n == "W960" else ("f32",))]
FLAT = {"f32": "hs::flat_kernel", "u8": "hs::flat_kernel_u8", "f16": "hs::flat_kernel_f16"}


@pytest.fixture(scope="module")
def hs():
    m = load_product()
    assert os.path.exists(m.LIB_PATH), "HIP extension missing: run __graft_entry__.build()"
    assert m.device_count() > 0, "no HIP device visible"
    return m


@pytest.fixture(scope="module")
def oracle():
    return Oracle()


def _fmt(hs, name):
    return {"f32": hs.HS_ROWS_F32, "u8": hs.HS_ROWS_U8, "f16": hs.HS_ROWS_F16}[name]


def _open(hs, s, src, fmt="f32", free=False):
    ix = _load(hs, src, s.dim, _fmt(hs, fmt), free, max_elements=s.cap)
    if s.allow:
        ix.set_replace_deleted(True)
    return ix


def _parse(raw, dim):
    """(rows, labels, marked) of a vanilla index file (hnswalg.h:748-779)."""
    u = np.frombuffer(raw, np.uint64, 6, 0)
    count, spe, label_off, data_off = int(u[2]), int(u[3]), int(u[4]), int(u[5])
    el = np.frombuffer(raw, np.uint8, count * spe, 96).reshape(count, spe)
    rows = np.ascontiguousarray(el[:, data_off:data_off + 4 * dim]).view(np.float32)
    return rows, np.ascontiguousarray(el[:, label_off:label_off + 8]).view(np.uint64)[:, 0], (el[:, 2] & 1) != 0


def _high_water(s, c):
    """The largest capacity the index had in its first c operations: what its device arrays are allocated for."""
    r = s.ops[:c]
    return max([s.cap] + r[r[:, 0] == RESIZE][:, 1].tolist())


def _reference_view(s, c):
    """The fixture's checkpoint in the shape _check_against_reference reads."""
    f = {"k": s.k, "efs": s.efs}
    for ef in s.efs:
        f.update({f"ef{ef}_{key}": v for key, v in s.reference(c, ef).items()})
    return f


_filters = {}


def _two_filters(n):
    if n not in _filters:
        f = np.stack([np.arange(n) % 3 != 1, np.random.default_rng(n).random(n) < 0.3]).astype(np.uint8)
        f.setflags(write=False)
        _filters[n] = f
    return _filters[n]


def _known_rows(s, c):
    """label -> index of the last row written under it by the first c operations."""
    adds = s.ops[:c][s.ops[:c, 0] == ADD]
    return {int(lab): int(r) for lab, r in zip(adds[:, 1], adds[:, 3])}


def _check_rows(hs, ix, s, c, labels, marked, widened):
    """get_row of every label whose last written row is known: that row bit for bit (a u8-only row comes back widened, as
    row + 0.0f); a label that left the index or is marked is not found."""
    present = {int(l) for l, m in zip(labels, marked) if not m}
    gone = 0
    for lab, r in _known_rows(s, c).items():
        if lab in present:
            want = s.rows[r] + np.float32(0.0) if widened else s.rows[r]
            assert ix.get_row(lab).tobytes() == want.tobytes(), f"row of label {lab}"
        elif gone < 4:
            gone += 1
            with pytest.raises(hs.HsError) as e:
                ix.get_row(lab)
            assert str(e.value) == "Label not found"


def _same_as_oracle(r, o, what):
    assert np.array_equal(r["cnt"], o["cnt"]), what
    assert pq_sorted(r["dists"], r["labels"], r["cnt"]) == pq_sorted(o["dists"], o["labels"], o["cnt"]), what
    assert np.array_equal(r["stats"][:, :3], o["counters"][:, :3]), what


def _check_checkpoint(hs, oracle, ix, s, c, fmt, free, tmp_path, last):
    what = f"{s.name} after {c} operations"
    q, k, dim = s.queries, s.k, s.dim
    # 1. the host image is the reference's
    saved = str(tmp_path / f"saved{c}.bin")
    ix.save(saved)
    raw = open(saved, "rb").read()
    assert file_sha(saved) == s.digest(c), what
    rows, labels, marked = _parse(raw, dim)
    n = len(labels)
    # 2. the device copy answers as the reference did
    _check_against_reference(ix, _reference_view(s, c), q)
    # 6. the kernel follows the marks
    assert ix.deleted_count() == int(marked.sum()) and ix.info()["has_deleted"] == int(marked.any()), what
    ix.set_ef(32)
    ix.search_pq(q, k)
    if marked.any():
        assert ix.last_kernel().startswith(("hs::fast_kernel", "hs::strict_kernel")), what
    else:
        assert ix.last_kernel() == FLAT[fmt], what
    # 3. a fresh load of the saved file in the same format, with the same allocated and reported capacity (a shrinking resize
    # lowers the reported capacity alone, and device_bytes counts the narrow copy by what is allocated)
    again = _load(hs, saved, dim, _fmt(hs, fmt), free, max_elements=_high_water(s, c))
    if again.capacity() != ix.capacity():
        again.resize(ix.capacity())
    assert _info(ix) == _info(again) and ix.info()["device_bytes"] == again.info()["device_bytes"], what
    assert ix.capacity() == again.capacity() and ix.deleted_count() == again.deleted_count(), what
    assert np.array_equal(ix.labels(), again.labels()) and np.array_equal(ix.labels(), labels), what
    assert ix.row_format() == _fmt(hs, fmt) and ix.f32_resident() == (not free)
    assert _answers(ix, q, k, efs=(10, 32, 64, 200)) == _answers(again, q, k, efs=(10, 32, 64, 200)), what
    a, b = ix.exact_search(q, k), again.exact_search(q, k)
    assert a["labels"].tobytes() == b["labels"].tobytes() and a["dists"].tobytes() == b["dists"].tobytes() and a["cnt"].tobytes() == b["cnt"].tobytes()
    # 4. the oracle on the saved file: plain searches, and one batch that mixes two filters
    ox = oracle.load(saved, "hnsw", L2, dim)
    filt = _two_filters(n)
    fs = hs.FilterSet.create(ix, 2)
    fs.write(0, filt)
    foq = (np.arange(len(q)) % 2).astype(np.uint32)
    for ef in (10, 64):
        ox.set_ef(ef)
        ix.set_ef(ef)
        ox.set_filter(None)
        _same_as_oracle(ix.search_pq(q, k, want_stats=True), ox.search_pq(q, k, threads=4), what)
        got = ix.search_filter_set(q, k, fs, foq, want_stats=True)
        for f in (0, 1):
            sel = foq == f
            ox.set_filter(filt[f])
            _same_as_oracle({key: v[sel] for key, v in got.items() if v is not None}, ox.search_pq(np.ascontiguousarray(q[sel]), k, threads=4),
                            f"{what}, ef {ef}, filter {f}")
    # exact search, with and without a filter, against brute force over the file's unmarked rows (computed once per checkpoint)
    same(ix.exact_search(q, k), slice(None), references(hs, oracle, L2, rows, q, k, labels, ~marked, ("seq", s.name, c, "all")), what)
    r = ix.exact_search(q, k, fs, foq)
    for f in (0, 1):
        sel = foq == f
        same(r, sel, references(hs, oracle, L2, rows, np.ascontiguousarray(q[sel]), k, labels, (filt[f] != 0) & ~marked, ("seq", s.name, c, f)), what)
    # 5. the rows on the device are the rows that were written
    _check_rows(hs, ix, s, c, labels, marked, widened=free and fmt == "u8")
    if last and fmt != "f32" and not free:      # both copies were written: drop the fp32 rows and ask the narrow one alone
        want = _answers(ix, q, k)
        ix.set_f32_resident(False)
        assert _answers(ix, q, k) == want, what
        _check_rows(hs, ix, s, c, labels, marked, widened=fmt == "u8")


@pytest.mark.parametrize("name,state", CASES)
def test_sequence_pinned_at_every_checkpoint(hs, oracle, tmp_path_factory, tmp_path, name, state):
    """The sequence in maximal runs (adds of a run, flagged or not, in one hs_index_upsert_points call): at every checkpoint the
    saved file has the reference's digest, searches give its labels, fp32 bits, counts and distance-call counts, a fresh load of
    the saved file agrees in every output, counter and info() field, the oracle agrees on plain and filtered searches, exact search
    agrees with brute force, and every row reads back as written -- in every row state the graph's rows allow."""
    fmt, free = STATES[state]
    s = sequence(name)
    ix = _open(hs, s, start_file(hs, name, tmp_path_factory), fmt, free)
    if name == "T":
        assert ix.info()["max_degree0"] <= 16
    prev = 0
    for c in s.checkpoints:
        _apply(ix, s.ops[prev:c], s.rows)
        _check_checkpoint(hs, oracle, ix, s, c, fmt, free, tmp_path, last=c == s.checkpoints[-1])
        prev = c
    if name == "T":
        assert ix.info()["max_degree0"] > 16      # the tiles went from stride 16 to 32 on the way
    elif name.startswith("W"):
        assert ix.info()["max_degree0"] <= 16     # never left the record path


@pytest.mark.parametrize("name", NAMES)
def test_call_boundaries_change_nothing(hs, tmp_path_factory, tmp_path, name):
    """One operation per call, and calls cut at seeded random points (which split runs of adds and of marks anywhere): the saved
    file has the reference's digest at every checkpoint, as in maximal runs (above), and the final answers are those of a fresh load."""
    s = sequence(name)
    src = start_file(hs, name, tmp_path_factory)
    rng = np.random.default_rng(len(s.ops))
    for how in ("single", "random"):
        ix = _open(hs, s, src)
        prev = 0
        for c in s.checkpoints:
            inner = np.arange(prev + 1, c) if how == "single" else np.sort(rng.choice(np.arange(prev + 1, c), size=(c - prev) // 4, replace=False))
            cuts = [prev] + inner.tolist() + [c]
            for a, b in zip(cuts[:-1], cuts[1:]):
                _apply(ix, s.ops[a:b], s.rows)
            saved = str(tmp_path / f"{how}{c}.bin")
            ix.save(saved)
            assert file_sha(saved) == s.digest(c), f"{name}, {how} calls, after {c} operations"
            prev = c
        again = _load(hs, saved, s.dim, hs.HS_ROWS_F32, False, max_elements=ix.capacity())
        assert _info(ix) == _info(again) and _answers(ix, s.queries, s.k, efs=(10, 64)) == _answers(again, s.queries, s.k, efs=(10, 64))


@pytest.mark.parametrize("name", INTEGER)
def test_row_format_changes_between_update_calls(hs, tmp_path_factory, tmp_path, name):
    """fp32 up to the first checkpoint, u8 beside fp32 up to the second, u8 without fp32 rows from there: ends equal, in every
    output, counter and info() field, to the index that was u8 without fp32 rows from the start."""
    s = sequence(name)
    src = start_file(hs, name, tmp_path_factory)
    ix, whole = _open(hs, s, src), _open(hs, s, src, "u8", True)
    _apply(whole, s.ops, s.rows)
    cps = s.checkpoints + [len(s.ops)]
    _apply(ix, s.ops[:cps[0]], s.rows)
    ix.set_row_format(hs.HS_ROWS_U8)
    _apply(ix, s.ops[cps[0]:cps[1]], s.rows)
    ix.set_f32_resident(False)
    _apply(ix, s.ops[cps[1]:], s.rows)
    a, b = str(tmp_path / "a.bin"), str(tmp_path / "b.bin")
    ix.save(a)
    whole.save(b)
    assert file_sha(a) == file_sha(b) == s.digest(len(s.ops))
    assert _info(ix) == _info(whole) and ix.info()["device_bytes"] == whole.info()["device_bytes"]
    assert (ix.capacity(), ix.deleted_count(), ix.row_format(), ix.f32_resident()) == (whole.capacity(), whole.deleted_count(), hs.HS_ROWS_U8, False)
    assert np.array_equal(ix.labels(), whole.labels())
    assert _answers(ix, s.queries, s.k, efs=(10, 32, 64, 200)) == _answers(whole, s.queries, s.k, efs=(10, 32, 64, 200))
    ea, eb = ix.exact_search(s.queries, s.k), whole.exact_search(s.queries, s.k)
    assert ea["labels"].tobytes() == eb["labels"].tobytes() and ea["dists"].tobytes() == eb["dists"].tobytes()
    rows, labels, marked = _parse(open(a, "rb").read(), s.dim)
    _check_rows(hs, ix, s, len(s.ops), labels, marked, widened=True)


def _client_file(ce, new_raw, first_raw, dim, held, new_ids):
    """The Slim file a patched client amounts to: the server's new file with what the patch stream does not carry left as the client
    holds it -- the enter point, the max level and has_deleted of the file it was loaded from (hnswalg_slim.h:2292-2340), and the
    label and row of every node that no record announced as new (a changed old node's record carries its lists alone, so a row
    that updatePoint rewrote, or a slot that took another label without becoming a new node, reaches no client).  `held`: the
    client's elements before the round.  Returns (file, the client's elements after it)."""
    hdr = struct.calcsize(ce.SLIM_HDR)
    h_old, h_new = list(struct.unpack_from(ce.SLIM_HDR, first_raw, 0)), list(struct.unpack_from(ce.SLIM_HDR, new_raw, 0))
    n, spe = h_new[0], 24 + 4 * dim
    el = np.frombuffer(new_raw, np.uint8, n * spe, hdr).reshape(n, spe).copy()
    keep = np.ones(len(held), bool)
    keep[new_ids[new_ids < len(held)]] = False
    el[:len(held)][keep, 8:16] = held[keep, 8:16]
    el[:len(held)][keep, 24:] = held[keep, 24:]
    h_new[6], h_new[8], h_new[13] = h_old[6], h_old[8], h_old[13]
    return struct.pack(ce.SLIM_HDR, *h_new) + el.tobytes() + new_raw[hdr + n * spe:], el


@pytest.mark.parametrize("name", ["G1", "W128"])
def test_slim_index_follows_through_convert_diff(hs, tmp_path_factory, tmp_path, name):
    """A resident Slim index follows the vanilla one through convertFromHNSWWithDiff at every checkpoint: its bytes, both changed
    lists, the stream and the chunked drain equal hs_slim_convert_diff_files on the saved files, and the server answers as its
    saved file loaded whole.  A client patched with the drained chunks answers as that file loaded whole with the old entry and
    with what the stream does not carry as the client had it (_client_file).  The Slim indexes are loaded with the sequence's
    largest capacity, so that no round is refused for room."""
    ce = load_chal_encode()
    s = sequence(name)
    src, sp = start_file(hs, name, tmp_path_factory), str(tmp_path / "old.slim")
    hs.convert_slim(src, sp, s.dim)
    first = open(sp, "rb").read()
    room = _high_water(s, len(s.ops)) + 1
    sx = hs.Index(sp, hs.HS_KIND_SLIM, s.dim, max_elements=room)
    client = hs.Index(sp, hs.HS_KIND_SLIM, s.dim, max_elements=room)
    hx = _open(hs, s, src)
    n0 = struct.unpack_from(ce.SLIM_HDR, first, 0)[0]
    held = np.frombuffer(first, np.uint8, n0 * (24 + 4 * s.dim), struct.calcsize(ce.SLIM_HDR)).reshape(n0, -1).copy()
    old, prev, changed, stale = sp, 0, 0, 0
    for c in s.checkpoints:
        _apply(hx, s.ops[prev:c], s.rows)
        d, new = _same(hs, sx, hx, old, tmp_path / f"r{c}", s.dim)
        assert file_sha(str(tmp_path / f"r{c}" / "now.hnsw")) == s.digest(c)
        changed += d.info()["n_old"] + d.info()["n_new"]
        for chunk in d.drained:
            client.patch(chunk, to_add=True)
        whole = hs.Index(new, hs.HS_KIND_SLIM, s.dim)
        assert sx.info()["n"] == int(s.f["facts"][c - 1, 4]) and _bits(sx, s.queries) == _bits(whole, s.queries)
        new_raw = open(new, "rb").read()
        expect, held = _client_file(ce, new_raw, first, s.dim, held, d.ids()[1])
        stale += expect != ce.with_entry_of(new_raw, first)
        want = str(tmp_path / f"expect{c}.slim")
        open(want, "wb").write(expect)
        assert _bits(client, s.queries) == _bits(hs.Index(want, hs.HS_KIND_SLIM, s.dim), s.queries), f"client after {c} operations"
        old, prev = new, c
    assert changed > 0 and stale > 0      # (the sequences update rows in place: the client's copy of them does go stale)
