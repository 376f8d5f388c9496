"""GPU tests (MI355X): the kernels of csrc/build_gpu.hip directly against the plain-Python reading of DESIGN.md 4m / 4n
(tests/batch_build_restated.py) -- never against the host twin: hs_build_hnsw_batched(device=0) and Index.add_points_batched(device=0)
followed by save(), whole files byte for byte.  The reading runs on the host, once per case for the module; the levels come from the
serial builder's file."""
import numpy as np
import pytest

import batch_build_cases as C
import batch_build_restated as R
from hsutil import load_product

pytestmark = pytest.mark.gpu
L2, IP = 0, 1
SEED = C.SEED


@pytest.fixture(scope="module")
def hs():
    m = load_product()
    assert m.device_count() > 0, "no HIP device"
    return m


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    return tmp_path_factory.mktemp("reading")


@pytest.mark.parametrize("name", C.GPU_CASES)
def test_device_build_equals_reading(hs, tmp_path, folder, name):
    _, metric, M, efc, kw = C.CASES[name]
    rows, levels, want, st = C.reading(hs, folder, name)
    out = str(tmp_path / "d.bin")
    dev = hs.build_hnsw_batched(rows, out, metric=metric, M=M, ef_construction=efc, seed=SEED, device=0, **kw)
    got = C.read(out)
    print(f"{name}: ties {st['ties']}, stale words {st['stale_words']}, most incoming ids {st['max_incoming']}, batches {st['batches']}")
    assert dev["used_gpu"] and dev["batches"] == st["batches"]
    assert R.levels_of(got) == levels
    assert got == want


def test_rerun_path_equals_reading(hs, tmp_path, folder):
    """scratch_ids = 64: rows outgrow the on-chip visited set and run again in the second launch; the same file."""
    _, metric, M, efc, kw = C.CASES["default"]
    rows, levels, want, st = C.reading(hs, folder, "default")
    out = str(tmp_path / "d.bin")
    dev = hs.build_hnsw_batched(rows, out, metric=metric, M=M, ef_construction=efc, seed=SEED, device=0, scratch_ids=64, **kw)
    assert dev["used_gpu"] and dev["flagged_rows"] > 0 and dev["batches"] == st["batches"]
    assert C.read(out) == want


_continued = {}


def continued(hs, folder, cut):
    """(n0, labels of the added rows, the reading's prefix file, the reading continued from it), once for the module."""
    if cut not in _continued:
        rows, levels, _, _ = C.reading(hs, folder, "default")
        n = len(rows)
        n0 = C.resume_cuts(levels, R.schedule(levels))[cut]
        prefix, _ = R.build(rows[:n0], levels[:n0], L2, 8, 100)
        labels = np.arange(n0, n) * 3 + 5000
        want, st = R.resume(prefix, 16, rows[n0:], levels[n0:], labels, L2, max_elements=n)
        print(f"{cut} at {n0}: {st}")
        _continued[cut] = (n0, labels, prefix, want, st)
    return _continued[cut]


@pytest.mark.parametrize("cut", ["boundary", "inside", "raises"])
def test_device_add_equals_reading(hs, tmp_path, folder, cut):
    """The prefix file is the reading's own; the index loads it with room, its level generator is put where a build of the prefix
    left it, the rest is added on the device, and save() writes the reading's continued file."""
    rows, levels, _, _ = C.reading(hs, folder, "default")
    n0, labels, prefix, want, st = continued(hs, folder, cut)
    n = len(rows)
    assert 0 < n0 < n
    part, out = str(tmp_path / "part.bin"), str(tmp_path / "saved.bin")
    with open(part, "wb") as f:
        f.write(prefix)
    ix = hs.Index(part, hs.HS_KIND_HNSW, 16, max_elements=n)
    ix.seed_levels(SEED, n0)
    dev = ix.add_points_batched(rows[n0:], labels, device=0)
    ix.save(out)
    got = C.read(out)
    assert dev["used_gpu"] and dev["batches"] == st["batches"]
    assert R.levels_of(got) == levels
    assert got == want
    if cut == "raises":
        assert ix.info()["maxlevel"] == max(levels) > max(levels[:n0])
