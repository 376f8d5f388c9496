"""patchFromStream on a device-resident index (hs_index_patch): an index grown by further insertions, shipped as the reference's
diff stream (genPatch wire format), must answer exactly like the index loaded whole.  dim 10 and 20 take the record kernel's
4-byte row path (dim % 4 != 0, row_words rounded up) and its 16-byte path on rows that are no multiple of 64 bytes."""
import os
import struct

import numpy as np
import pytest

from hsutil import Oracle, load_chal_encode, load_product, mixture

pytestmark = pytest.mark.gpu


def _old_and_new(hs, tmp_path, dim, n0, delta, integer):
    """The Slim files of the first n0 rows and of all n0 + delta rows (old.slim / new.slim under tmp_path), as bytes."""
    base = mixture(n0 + delta, dim, 17, integer=integer)
    files = {}
    for tag, n in (("old", n0), ("new", n0 + delta)):
        hp, sp = str(tmp_path / f"{tag}.hnsw"), str(tmp_path / f"{tag}.slim")
        hs.build_hnsw(base[:n], hp, M=16, ef_construction=100, threads=1)   # serial: the first n0 insertions are the same in both
        hs.convert_slim(hp, sp, dim, threads=1)
        files[tag] = open(sp, "rb").read()
    return files


def _same_rows_and_labels(ix, ref):
    """hs_labels, and getDataByLabel of every label (the changed and the added ones among them), byte for byte."""
    labels = ix.labels()
    assert np.array_equal(labels, ref.labels())
    for lab in labels:
        assert ix.get_row(int(lab)).tobytes() == ref.get_row(int(lab)).tobytes(), int(lab)


@pytest.mark.parametrize("dim,n0,delta,integer", [(32, 3000, 400, False), (128, 8000, 1500, True), (10, 2000, 300, False), (20, 2000, 300, False)])
def test_patched_index_equals_index_loaded_whole(tmp_path, dim, n0, delta, integer):
    hs, ce, O = load_product(), load_chal_encode(), Oracle()
    files = _old_and_new(hs, tmp_path, dim, n0, delta, integer)
    patch, n_changed, n_added = ce.make_patch(files["old"], files["new"], dim, to_add=True)
    assert n_added == delta and n_changed > 0
    want_file = str(tmp_path / "expect.slim")
    open(want_file, "wb").write(ce.with_entry_of(files["new"], files["old"]))
    q = mixture(300, dim, 18, integer=integer)
    ix = hs.Index(str(tmp_path / "old.slim"), hs.HS_KIND_SLIM, dim, max_elements=n0 + delta + 16)
    ix.set_ef(48)
    before = ix.search_ids(q, 10)["labels"]
    ix.patch(patch, to_add=True)
    assert ix.info()["n"] == n0 + delta
    ref = hs.Index(want_file, hs.HS_KIND_SLIM, dim)
    ox = O.load(want_file, "slim", 0, dim)
    for ef in (10, 48, 100):
        for x in (ix, ref, ox):
            x.set_ef(ef)
        for exact in (True, False):
            ix.set_exact_order(exact); ref.set_exact_order(exact)
            a, b = ix.search_ids(q, 10, want_dists=True, want_stats=True), ref.search_ids(q, 10, want_dists=True, want_stats=True)
            assert np.array_equal(a["labels"], b["labels"]) and a["dists"].tobytes() == b["dists"].tobytes()
            assert np.array_equal(a["stats"][:, :3], b["stats"][:, :3])
        o = ox.search_ids(q, 10)
        assert np.array_equal(np.sort(a["labels"], 1), np.sort(o["labels"], 1)) and np.array_equal(a["stats"][:, :3], o["counters"][:, :3])
    ix.set_ef(48)
    assert not np.array_equal(ix.search_ids(q, 10)["labels"], before), "the patch changed nothing?"
    _same_rows_and_labels(ix, ref)
    # refusals: not patchable / over capacity / truncated stream leaves the index as it was
    with pytest.raises(hs.HsError):
        ref.patch(patch)
    small = hs.Index(str(tmp_path / "old.slim"), hs.HS_KIND_SLIM, dim, max_elements=n0 + 1)
    with pytest.raises(hs.HsError):
        small.patch(patch, to_add=True)
    again = hs.Index(str(tmp_path / "old.slim"), hs.HS_KIND_SLIM, dim, max_elements=n0 + delta)
    again.set_ef(48)
    with pytest.raises(hs.HsError):
        again.patch(patch[: len(patch) // 2], to_add=True)
    assert np.array_equal(again.search_ids(q, 10)["labels"], before)


def test_patch_without_vectors_leaves_zero_rows(tmp_path):
    """to_add = False: the stream carries no vectors, so the added nodes' rows are the zeros the host image holds (hnswalg_slim.h:2292-2340
    reads a vector only with to_add).  A search that reaches an added node measures its distance to a zero row, and which queries
    reach one cannot be told from outside, so the comparison with the index loaded whole from the new file is made where it is
    exact: hs_labels equal, getDataByLabel of every added label all zeros and of every other label the new file's row.  (Run on the
    code before the one write path, on the GPU: the same holds there, while 213 of 300 queries answer differently from the index
    loaded whole at ef 48.)  The same file with the added rows zeroed, loaded whole, is the patched index: hs_info, hs_labels and
    the searches' labels, distances and three counters are equal."""
    hs, ce = load_product(), load_chal_encode()
    dim, n0, delta = 32, 3000, 400
    files = _old_and_new(hs, tmp_path, dim, n0, delta, False)
    patch, n_changed, n_added = ce.make_patch(files["old"], files["new"], dim, to_add=False)
    assert n_added == delta and n_changed > 0
    want = ce.with_entry_of(files["new"], files["old"])
    zeroed = bytearray(want)
    h, spe = struct.calcsize(ce.SLIM_HDR), 24 + 4 * dim
    for i in range(n0, n0 + delta):
        zeroed[h + i * spe + 24:h + (i + 1) * spe] = bytes(4 * dim)
    for name, raw in (("expect.slim", want), ("zeroed.slim", zeroed)):
        open(str(tmp_path / name), "wb").write(raw)
    ix = hs.Index(str(tmp_path / "old.slim"), hs.HS_KIND_SLIM, dim, max_elements=n0 + delta + 16)
    ix.patch(patch, to_add=False)
    whole, zero = (hs.Index(str(tmp_path / name), hs.HS_KIND_SLIM, dim) for name in ("expect.slim", "zeroed.slim"))
    labels = ix.labels()
    assert ix.info()["n"] == n0 + delta and np.array_equal(labels, whole.labels())
    for i, lab in enumerate(labels):
        row = ix.get_row(int(lab))
        assert row.tobytes() == (bytes(4 * dim) if i >= n0 else whole.get_row(int(lab)).tobytes()), i
    assert ix.info() == zero.info()
    _same_rows_and_labels(ix, zero)
    q = mixture(300, dim, 18)
    differ = 0
    for ef in (10, 48):
        for x in (ix, whole, zero):
            x.set_ef(ef)
        for exact in (True, False):
            for x in (ix, whole, zero):
                x.set_exact_order(exact)
            a, b, w = (x.search_ids(q, 10, want_dists=True, want_stats=True) for x in (ix, zero, whole))
            assert np.array_equal(a["labels"], b["labels"]) and a["dists"].tobytes() == b["dists"].tobytes()
            assert np.array_equal(a["stats"][:, :3], b["stats"][:, :3])
            differ = int((a["labels"] != w["labels"]).any(1).sum())
    print(f"to_add=False: {differ} of {len(q)} queries answer differently from the index loaded whole with its rows (ef 48, fast kernel)")
