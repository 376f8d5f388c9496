"""What a loader guarantees (csrc/index_check.hpp), pinned without a GPU: every place where outside bytes become a graph refuses
a graph that would send a kernel, or the host code that packs for one, out of bounds -- and refuses nothing else.  The reference of
every verdict is tests/hostile_graphs.py::violations, a plain-Python reading of the same preconditions over what
oracle/chal_encode.py parses.  The loaders parse and check before they ask for a device, so on a machine without one a refused
input reports HS_ERR_CORRUPT / HS_ERR_INVALID and an accepted one HS_ERR_DEVICE."""
import glob
import os
import subprocess

import numpy as np
import pytest

import hostile_graphs as hg
from hsutil import GOLDEN, ROOT, load_chal_encode, load_product, mixture, vanilla_bytes

CORRUPT_TEXT = "Index seems to be corrupted or unsupported"


@pytest.fixture(scope="module")
def hs():
    return load_product()


@pytest.fixture(scope="module")
def bases(hs, tmp_path_factory):
    return hg.base_files(hs, tmp_path_factory.mktemp("bases"))


@pytest.fixture(scope="module")
def catalogue(bases):
    """[(kind, dim, name, bytes, violation)] and the near misses [(kind, dim, name, bytes)]"""
    bad, ok = [], []
    for (kind, name), (raw, dim) in bases.items():
        bad += [(kind, dim, f"{name}:{m}", b, item) for m, b, item in hg.mutations(kind, raw, dim)]
        ok += [(kind, dim, f"{name}:{m}", b) for m, b in hg.near_misses(kind, raw, dim)]
    return bad, ok


# ---- premises ---------------------------------------------------------------------------------------------------------------
def test_premise_every_valid_file_violates_nothing(hs, bases, tmp_path):
    ce = load_chal_encode()
    for (kind, name), (raw, dim) in bases.items():
        assert hg.violations(hg.read(kind, raw, dim)) == [], (kind, name)
    for path in sorted(glob.glob(os.path.join(GOLDEN, "*.hnsw.bin"))):
        raw = open(path, "rb").read()
        g = ce.parse_vanilla(raw)
        assert hg.violations(g) == [], path
        slim = ce.vanilla_to_slim_verbatim(raw)
        assert hg.violations(hg.read("slim", slim, g["dim"])) == [], path
        sp = str(tmp_path / "c.slim")
        hs.convert_slim(path, sp, g["dim"], metric=hs.HS_METRIC_IP if os.path.basename(path).startswith("ip_") else hs.HS_METRIC_L2, threads=1)
        assert hg.violations(hg.read("slim", open(sp, "rb").read(), g["dim"])) == [], path


def test_premise_each_mutation_is_its_one_violation(catalogue):
    bad, ok = catalogue
    seen = set()
    for kind, dim, name, raw, item in bad:
        assert hg.violations(hg.read(kind, raw, dim)) == [item], name
        seen.add((kind, item))
    for kind, dim, name, raw in ok:
        assert hg.violations(hg.read(kind, raw, dim)) == [], name
    # the catalogue covers every item for every kind it applies to
    for kind in ("hnsw", "slim", "slimq"):
        want = {"enterpoint", "maxlevel", "ep_level", "count", "id", "owner", hg.ARITH}
        want |= {"threshold"} if kind != "hnsw" else set()
        want |= {"cluster"} if kind == "slimq" else set()
        assert want <= {i for k, i in seen if k == kind}, kind
    assert ("slim", "level") in seen and ("hnsw", "level") in seen
    assert {n.split(":")[1] for _, _, n, _ in ok} >= {"id_other_valid_l0", "id_other_valid_up", "duplicate_id", "count_minus_one",
                                                      "count_at_capacity", "taller_than_maxlevel"}


# ---- verdicts ---------------------------------------------------------------------------------------------------------------
def test_every_hostile_file_is_refused_as_corrupt(hs, catalogue, tmp_path):
    for kind, dim, name, raw, _ in catalogue[0]:
        for path in (None, tmp_path / "f.bin"):   # hs_index_load_mem, hs_index_load
            status, text = hg.product_status(hs, kind, raw, dim, path)
            assert status == hs.HS_ERR_CORRUPT and CORRUPT_TEXT in text, (name, status, text)
        if kind != "slimq":   # with room, the path of a patchable / growable index
            status, text = hg.product_status(hs, kind, raw, dim, max_elements=5000)
            assert status == hs.HS_ERR_CORRUPT, (name, status, text)


def test_every_base_file_and_near_miss_is_accepted(hs, bases, catalogue, tmp_path):
    for (kind, name), (raw, dim) in bases.items():
        for path in (None, tmp_path / "f.bin"):
            status, _ = hg.product_status(hs, kind, raw, dim, path)
            assert hg.accepted(hs, status), (kind, name, status)
    for kind, dim, name, raw in catalogue[1]:
        status, text = hg.product_status(hs, kind, raw, dim)
        assert hg.accepted(hs, status), (name, status, text)


def test_hostile_vanilla_files_are_refused_by_every_consumer(hs, catalogue, tmp_path):
    """VanillaGraph::load is the one door: conversion, resume and the SlimQ graph conversion refuse what hs_index_load refuses."""
    rows = mixture(3, hg.DIM, 5)
    for kind, dim, name, raw, _ in catalogue[0]:
        if kind != "hnsw":
            continue
        f, o = str(tmp_path / "v.bin"), str(tmp_path / "o.bin")
        open(f, "wb").write(raw)
        for call in (lambda: hs.convert_slim(f, o, dim, threads=1),
                     lambda: hs.hnsw_resume(f, o, rows, np.arange(3, dtype=np.uint64) + 10 ** 6, dim=dim, max_elements=5000),
                     lambda: hs.convert_slimq_graph(f, o, dim, threads=1)):
            with pytest.raises(hs.HsError, match=CORRUPT_TEXT) as e:
                call()
            assert e.value.status == hs.HS_ERR_CORRUPT, name


def _from_csr(hs, a, kind):
    try:
        hs.Index.from_csr(kind, hs.HS_METRIC_L2, a["vectors"], a["levels"], a["list_ptr"], a["list_ids"], a["enterpoint"], a["maxlevel"],
                          threshold_level=a["threshold_level"])
    except hs.HsError as e:
        return e.status
    return hs.HS_OK


def test_hostile_arrays_are_invalid(hs, bases):
    ce = load_chal_encode()
    a = hg.arrays_of(ce.parse_vanilla(bases[("hnsw", "handmade_levels")][0]))
    assert hg.arrays_violations(a) == []
    bad, ok = hg.array_cases(a)
    assert {item for _, _, item in bad} == {"enterpoint", "id", "ep_level", "threshold", "count", "owner"}
    for name, b, item in bad:
        assert hg.arrays_violations(b) == [item], name
        kinds = (hs.HS_KIND_SLIM,) if item == "threshold" else (hs.HS_KIND_HNSW, hs.HS_KIND_SLIM)   # a vanilla index has no threshold level
        for kind in kinds:
            assert _from_csr(hs, b, kind) == hs.HS_ERR_INVALID, name
    for extra in (dict(maxlevel=-1), dict(levels=np.where(np.arange(len(a["levels"])) == 7, -1, a["levels"]).astype(np.int32))):
        b = dict(a, **extra)
        assert hg.arrays_violations(b) != []
        assert _from_csr(hs, b, hs.HS_KIND_HNSW) == hs.HS_ERR_INVALID
    for name, b in ok + [("as it is", a)]:
        assert hg.arrays_violations(b) == [], name
        for kind in (hs.HS_KIND_HNSW, hs.HS_KIND_SLIM):
            assert hg.accepted(hs, _from_csr(hs, b, kind)), name


# ---- the empty index: what the loaders did before the guard, they do now -------------------------------------------------------
@pytest.mark.parametrize("kind", ["hnsw", "slim", "slimq"])
def test_empty_index_is_taken_as_it_is(hs, kind, tmp_path):
    """n == 0: nothing is checked, whatever the header's enter point and max level say (the reference writes -1 and -1)."""
    ce = load_chal_encode()
    for ep, maxlevel in ((0xFFFFFFFF, -1), (0, 0), (7, 3)):
        van = vanilla_bytes(np.zeros((0, hg.DIM), np.float32), [], 4, enterpoint=ep, maxlevel=maxlevel)
        if kind == "hnsw":
            raw, dim = van, hg.DIM
        elif kind == "slim":
            raw, dim = ce.vanilla_to_slim_verbatim(van), hg.DIM
        else:
            from slimq_resident_util import write_slimq
            write_slimq(str(tmp_path / "e.slimq"), hg.SLIMQ_DIM, [], enterpoint=ep)
            raw, dim = open(str(tmp_path / "e.slimq"), "rb").read(), hg.SLIMQ_DIM
        assert hg.violations(hg.read(kind, raw, dim)) == []
        status, text = hg.product_status(hs, kind, raw, dim)
        assert hg.accepted(hs, status), (ep, maxlevel, status, text)


# ---- patch streams: the premise (the verdicts need a resident index: tests/test_gpu_load_guard.py) -----------------------------
def test_premise_each_hostile_patch_is_its_one_violation(hs, tmp_path):
    ce = load_chal_encode()
    old, new, patch = hg.patch_pair(hs, tmp_path)
    before = ce.parse_slim(old, hg.DIM)
    assert hg.violations(hg.patched(before, patch, hg.DIM), unlisted_ok=True) == []
    cases = hg.hostile_patches(before, patch, hg.DIM)
    assert [item for _, _, item in cases] == ["id", "count", "owner", hg.ARITH]
    for name, stream, item in cases:
        assert len(stream) == len(patch)
        assert hg.violations(hg.patched(before, stream, hg.DIM), unlisted_ok=True) == [item], name
    # a diff delivered in chunks: the first half of the records as a stream of its own names new nodes that have no record yet --
    # legal under the reading of a patched image, and only under it
    (new_count, n_old, n_new), recs = hg.patch_records(patch, hg.DIM)
    cut = recs[n_old][0]
    first = hg.put(patch[:cut], 16, 0, "<Q")
    image = hg.patched(before, first, hg.DIM)
    assert hg.violations(image, unlisted_ok=True) == [] and hg.violations(image) == ["owner"]


# ---- seeded sweep --------------------------------------------------------------------------------------------------------------
def test_sweep_of_single_word_edits_matches_the_reading(hs, bases):
    """300 random single-word edits of handmade_levels, its Slim twin and its SlimQ twin: the product's accept / refuse verdict equals
    violations(...) == [] on every one -- a check that is too strict fails here as one that is too lax does.  An edit that only
    breaks the file's arithmetic counts as refused by both."""
    rng = np.random.default_rng(20261)
    drawn = {True: 0, False: 0}
    for key in (("hnsw", "handmade_levels"), ("slim", "handmade_levels_verbatim"), ("slimq", "handmade_levels_twin")):
        kind = key[0]
        raw, dim = bases[key]
        w = hg.locate(kind, raw, dim)
        n = w["n"]
        slots = {"header": [(w[k], "<I") for k in ("ep", "maxlevel", "threshold") if w[k] is not None],
                 "ids": [(at + 4 * j, "<I") for (at, cnt) in w["ids"].values() for j in range(cnt)]}
        if kind == "hnsw":
            slots["count"] = [(at, "<I") for at in w["count_word"].values()]
        else:
            slots["level"] = [(at, "<I") for at in w["level_word"].values()]
            slots["offset"] = [(at, "<H") for at in w["off_slot"].values()]
        for _ in range(100):
            fam = sorted(slots)[rng.integers(len(slots))]
            at, fmt = slots[fam][rng.integers(len(slots[fam]))]
            value = int([0, n - 1, n, rng.integers(n), 0xFFFF, 0xFFFFFFFF][rng.integers(6)])
            edited = hg.put(raw, at, value & (0xFFFF if fmt == "<H" else 0xFFFFFFFF), fmt)
            want = hg.violations(hg.read(kind, edited, dim))
            status, text = hg.product_status(hs, kind, edited, dim)
            assert status in (hs.HS_OK, hs.HS_ERR_DEVICE, hs.HS_ERR_CORRUPT), (kind, fam, at, value, status, text)
            assert hg.accepted(hs, status) == (want == []), (kind, fam, at, value, want, status, text)
            drawn[want == []] += 1
    print(f"sweep: {drawn[True]} edits accepted by both, {drawn[False]} refused by both")
    assert drawn[True] >= 30 and drawn[False] >= 30


# ---- the stand-alone program under AddressSanitizer / UBSan --------------------------------------------------------------------
def test_standalone_chain_under_sanitizers(hs, bases, catalogue, tmp_path):
    """csrc/load_guard_test.cpp: load -> check -> pack -> upper-level tiles -> level-0 tiles on the host.  Every catalogue file must be
    refused by the check before a sanitizer has anything to report, every base file and near miss must run the whole chain clean."""
    exe = os.path.join(ROOT, "hnsw-slim_amd", "load_guard_test")
    subprocess.check_call(["make", "-C", os.path.dirname(exe), "load_guard_test"])
    lines = []

    def emit(kind, dim, raw, expect):
        path = str(tmp_path / f"f{len(lines)}.bin")
        open(path, "wb").write(raw)
        lines.append(f"{kind} {dim} {expect} {path}")

    for (kind, _), (raw, dim) in bases.items():
        emit(kind, dim, raw, "accept")
    for kind, dim, _, raw, _ in catalogue[0]:
        emit(kind, dim, raw, "refuse")
    for kind, dim, _, raw in catalogue[1]:
        emit(kind, dim, raw, "accept")
    manifest = tmp_path / "manifest.txt"
    manifest.write_text("\n".join(lines) + "\n")
    out = subprocess.run([exe, str(manifest)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert f"{len(lines)} files" in out.stdout, out.stdout[-500:]
