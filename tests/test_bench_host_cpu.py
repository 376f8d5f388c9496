"""Host-side logic of bench.py that runs before any GPU work: the label checksum every timed batch is checked with, and the
hardware-queue hint for runs whose per-rank shards are small (profiles/r03_small_batch_queues.log)."""
import os
import sys

import numpy as np

from hsutil import ROOT

sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_checksum_is_order_independent_within_a_query_and_sensitive_to_a_changed_label():
    rng = np.random.default_rng(1)
    lab = rng.integers(0, 1_000_000, (500, 10)).astype(np.uint32)
    perm = np.stack([rng.permutation(row) for row in lab])
    assert bench.checksum(lab) == bench.checksum(perm)
    bad = lab.copy()
    bad[17, 3] += 1
    assert bench.checksum(lab) != bench.checksum(bad)


def test_hardware_queue_hint(monkeypatch):
    def hint(nq, world, scaling, preset=None, one_device=False):
        monkeypatch.delenv("GPU_MAX_HW_QUEUES", raising=False)
        monkeypatch.delenv("HS_BENCH_ONE_DEVICE", raising=False)
        if preset:
            monkeypatch.setenv("GPU_MAX_HW_QUEUES", preset)
        if one_device:
            monkeypatch.setenv("HS_BENCH_ONE_DEVICE", "1")
        bench.hip_queue_hint(nq, world, scaling)
        return os.environ.get("GPU_MAX_HW_QUEUES")
    assert hint(10000, 1, "auto") is None              # the default command: runtime default
    assert hint(10000, 2, "auto") is None              # 5000 queries per rank
    assert hint(10000, 4, "auto") == "8"               # 2500 per rank, one process per GPU
    assert hint(10000, 8, "auto") == "8"
    assert hint(10000, 8, "weak") is None              # every rank its own 10k batches
    assert hint(1250, 1, "auto") == "16"               # a single process issuing small batches
    assert hint(10000, 8, "auto", preset="4") == "4"   # the caller's setting wins
    assert hint(2000, 2, "auto", one_device=True) is None   # ranks rehearsing on one GPU: never


def test_dump_outputs_writes_exact_float64_and_stays_within_the_limit(tmp_path):
    rng = np.random.default_rng(2)
    arrays = {f"labels_qset{b}": rng.integers(0, 1_000_000, (1000, 10)).astype(np.uint32) for b in range(3)}
    names = bench.dump_outputs(str(tmp_path / "all"), arrays)
    assert names == sorted(arrays)
    for name, a in arrays.items():
        got = np.load(tmp_path / "all" / f"{name}.npy")
        assert got.dtype == np.float64 and np.array_equal(got, a)
    # over the limit: the same seeded row sample on every run, and the files stay within it
    limit = 100_000
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), arrays, limit=limit)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == sorted([f"{n}.npy" for n in arrays] + [f"{n}_rows.npy" for n in arrays])
    payload = sum(np.load(tmp_path / "a" / f).nbytes for f in files)
    assert 0 < payload <= limit
    for name, a in arrays.items():
        rows = np.load(tmp_path / "a" / f"{name}_rows.npy")
        got = np.load(tmp_path / "a" / f"{name}.npy")
        assert np.array_equal(rows, np.load(tmp_path / "b" / f"{name}_rows.npy"))
        assert np.array_equal(got, a[rows.astype(np.int64)])


def test_index_cache_is_built_once_reproducibly_and_only_published_complete(tmp_path, monkeypatch):
    from hsutil import load_product
    hs = load_product()
    files = {}
    for root in ("a", "b"):   # two separate builds of the default (serial) index: the same bytes
        monkeypatch.setenv("XDG_CACHE_HOME", str(tmp_path / root))
        idir, t_build, _ = bench.prepare_cached(2000, 16, 1, hs)
        assert idir == bench.index_cache_dir(2000, 16) and idir.startswith(str(tmp_path / root))
        assert sorted(os.listdir(idir)) == ["base.npy", "ready", "slim.bin"]
        assert t_build > 0
        assert [d for d in os.listdir(os.path.dirname(idir)) if ".part" in d] == []   # the staging directory was renamed into place
        assert bench.prepare_cached(2000, 16, 1, hs) == (idir, 0.0, 0.0)              # second call: reused as it is
        files[root] = {f: open(os.path.join(idir, f), "rb").read() for f in ("base.npy", "slim.bin")}
    assert files["a"] == files["b"]
    assert np.array_equal(np.load(os.path.join(idir, "base.npy")), bench.headline_data(2000, 16, 123))
    assert bench.index_cache_dir(2000, 16, 4) != bench.index_cache_dir(2000, 16)      # a parallel build never shares its cache
