"""What a loader guarantees, on the device: a hostile file, conversion input or patch stream (tests/hostile_graphs.py) is refused
with HS_ERR_CORRUPT before anything reaches a device array, a refused patch leaves the index and its host image byte for byte as
they were, and the guard changes nothing a legal graph answers.

Ordering rule: no test searches, converts or builds on the device from an input it expects to be refused.  The refusal assert comes
first and everything after it depends on it; tests/test_load_guard_cpu.py holds the same verdicts without a device and must be
green before this file is run."""
import os

import numpy as np
import pytest

import hostile_graphs as hg
from hsutil import Oracle, load_chal_encode, load_product, mixture

pytestmark = pytest.mark.gpu
KIND = {"hnsw": "HS_KIND_HNSW", "slim": "HS_KIND_SLIM", "slimq": "HS_KIND_SLIMQ"}


@pytest.fixture(scope="module")
def hs():
    m = load_product()
    assert os.path.exists(m.LIB_PATH), "HIP extension missing: run __graft_entry__.build()"
    assert m.device_count() > 0, "no HIP device visible"
    return m


@pytest.fixture(scope="module")
def bases(hs, tmp_path_factory):
    return hg.base_files(hs, tmp_path_factory.mktemp("bases"))


def test_every_hostile_file_is_refused_before_the_device(hs, bases, tmp_path):
    """hs.Index of every catalogue file, all three kinds, and hs.convert_slim_gpu of the hostile vanilla files: the status only."""
    n = 0
    for (kind, name), (raw, dim) in bases.items():
        for m, bad, _ in hg.mutations(kind, raw, dim):
            status, text = hg.product_status(hs, kind, bad, dim)
            assert status == hs.HS_ERR_CORRUPT, (name, m, status, text)
            n += 1
            if kind == "hnsw":
                f = str(tmp_path / "v.bin")
                open(f, "wb").write(bad)
                with pytest.raises(hs.HsError) as e:
                    hs.convert_slim_gpu(f, str(tmp_path / "o.bin"), dim)
                assert e.value.status == hs.HS_ERR_CORRUPT, (name, m)
    assert n > 100


def canon(d, l, c):
    """Per query the sorted keys (dist bits << 32 | label) of its first c[i] pairs, ~0 beyond."""
    key = (np.ascontiguousarray(d, np.float32).view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.asarray(l).astype(np.uint64)
    key[np.arange(key.shape[1])[None, :] >= np.asarray(c)[:, None]] = np.iinfo(np.uint64).max
    return np.sort(key, axis=1)


def test_near_misses_load_and_answer_as_the_oracle(hs, bases, tmp_path):
    """Positive control: the legal look-alikes of the catalogue load, and 20 queries each are answered as the oracle answers them on
    the same file -- the guard did not change what a legal graph answers."""
    O = Oracle()
    n = 0
    for (kind, name), (raw, dim) in bases.items():
        q = mixture(20, dim, 91)
        for m, ok in hg.near_misses(kind, raw, dim):
            assert hg.violations(hg.read(kind, ok, dim)) == []
            f = str(tmp_path / "ok.bin")
            status, ix = hg.product_status(hs, kind, ok, dim, f)
            assert status == hs.HS_OK, (name, m, status, ix)
            ix.set_ef(10)
            if kind == "slimq":
                rows = np.random.default_rng(5).normal(0, 1, (ix.info()["n"], dim)).astype(np.float32)
                ix.slimq_set_dataset(rows)
                ox = O.load_slimq(f)
                ox.set(10, ix.slimq_tconst(), rows)
                a, b = ix.slimq_search(q, 3, want_stats=True), ox.search(q, 3)
                assert np.array_equal(a["cnt"], b["counts"]), (name, m)
                assert np.array_equal(canon(a["dists"], a["labels"], a["cnt"]), canon(b["dists"], b["labels"], b["counts"])), (name, m)
                assert np.array_equal(a["stats"].astype(np.uint64), b["counters"]), (name, m)
            else:
                ox = O.load(f, kind, 0, dim)
                ox.set_ef(10)
                a, b = ix.search_pq(q, 3), ox.search_pq(q, 3)
                assert np.array_equal(a["cnt"], b["cnt"]), (name, m)
                assert np.array_equal(canon(a["dists"], a["labels"], a["cnt"]), canon(b["dists"], b["labels"], b["cnt"])), (name, m)
            n += 1
    assert n >= 30


def _answers(ix, q):
    out = []
    for exact in (True, False):
        ix.set_exact_order(exact)
        a = ix.search_ids(q, 10, want_dists=True, want_stats=True)
        out.append((a["labels"].copy(), a["dists"].tobytes(), a["stats"][:, :3].copy()))
    return out


def test_refused_patch_leaves_index_and_host_image_untouched(hs, tmp_path):
    """Each hostile patch (well framed: the staging pass alone does not catch it) on a client loaded from the old file with room is
    refused with HS_ERR_CORRUPT; info(), labels() and the bytes save_slim writes are what they were; only then 50 queries at ef 48
    are answered as before in both order modes; then the valid patch applies and the client equals the index loaded whole.
    (Before the check moved in front of the image write, a refused stream left its records in the host image: save_slim wrote them.)"""
    ce, O = load_chal_encode(), Oracle()
    dim = hg.DIM
    old, new, patch = hg.patch_pair(hs, tmp_path)
    n0 = ce.parse_slim(old, dim)["count"]
    q = mixture(50, dim, 18)
    ix = hs.Index(str(tmp_path / "old.slim"), hs.HS_KIND_SLIM, dim, max_elements=n0 + 56)
    ix.set_ef(48)
    info, labels, before = ix.info(), ix.labels().copy(), _answers(ix, q)
    ix.save_slim(str(tmp_path / "saved0.slim"))
    assert open(str(tmp_path / "saved0.slim"), "rb").read() == old
    for name, stream, item in hg.hostile_patches(ce.parse_slim(old, dim), patch, dim):
        with pytest.raises(hs.HsError) as e:
            ix.patch(stream, to_add=True)
        assert e.value.status == hs.HS_ERR_CORRUPT, (name, e.value.status)
        assert ix.info() == info and np.array_equal(ix.labels(), labels), name
        ix.save_slim(str(tmp_path / "saved.slim"))
        assert open(str(tmp_path / "saved.slim"), "rb").read() == old, f"{name}: the refused patch changed the host image"
        for (l0, d0, s0), (l1, d1, s1) in zip(before, _answers(ix, q)):
            assert np.array_equal(l0, l1) and d0 == d1 and np.array_equal(s0, s1), name
    # the valid patch still applies, and the client is the index loaded whole (as test_gpu_patch.py compares them)
    ix.patch(patch, to_add=True)
    want_file = str(tmp_path / "expect.slim")
    open(want_file, "wb").write(ce.with_entry_of(new, old))
    ref = hs.Index(want_file, hs.HS_KIND_SLIM, dim)
    ox = O.load(want_file, "slim", 0, dim)
    assert ix.info()["n"] == ce.parse_slim(new, dim)["count"]
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
    labels = ix.labels()
    assert np.array_equal(labels, ref.labels())
    for lab in labels:
        assert ix.get_row(int(lab)).tobytes() == ref.get_row(int(lab)).tobytes(), int(lab)
