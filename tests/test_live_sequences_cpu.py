"""CPU-only tests of random update sequences on the live-update host core.  tests/golden/updates_seq_<name>.npz holds seeded legal
lists of >= 100 interleaved operations -- marks, unmarks, updates, appends, bursts of addPoint(.., true), resizes -- that ran through
the compiled reference, which left the SHA-256 of its saved file after every operation, its searchKnn results at two or three
checkpoints and its own account of every operation.  hs_hnsw_replay must reach the same digests, the oracle the same answers; the
fixtures must cover what they are there for; and the sanitised stand-alone program csrc/upsert_test.cpp runs two of the lists."""
import os
import re
import subprocess

import numpy as np
import pytest

from hsutil import GOLDEN, ROOT, load_product
from live_sequences import ADD, GOLDEN_START, NAMES, file_sha, generator, pq_sorted, sequence, start_file

L2 = 0


@pytest.fixture(scope="module")
def hs():
    m = load_product()
    m.build_library()
    return m


def _replay(hs, s, src, out, c):
    hs.hnsw_replay(src, out, s.ops[:c], s.rows, s.dim, max_elements=s.cap, allow_replace_deleted=s.allow)
    return file_sha(out)


@pytest.mark.parametrize("name", NAMES)
def test_replay_reaches_the_reference_digests(hs, oracle, tmp_path_factory, tmp_path, name):
    """hs_hnsw_replay of ops[:c] from the start file == the reference's digest after c operations, at every checkpoint and at the
    end; the oracle on the replayed file answers as the reference did there (labels, fp32 bits, counts, distance calls)."""
    s = sequence(name)
    src, out = start_file(hs, name, tmp_path_factory), str(tmp_path / "out.bin")
    assert len(s.ops) >= 100 and s.checkpoints == sorted(set(s.checkpoints)) and s.checkpoints[-1] == len(s.ops)
    for c in s.checkpoints:
        if _replay(hs, s, src, out, c) != s.digest(c):
            # (every prefix from the start file: a call begins with loadIndex, which orders deleted_elements by id)
            first = next(i for i in range(1, c + 1) if _replay(hs, s, src, out, i) != s.digest(i))
            pytest.fail(f"{name}: checkpoint {c}: the first operation whose file differs from the reference's is {first - 1}: {s.ops[first - 1].tolist()}")
        ox = oracle.load(out, "hnsw", L2, s.dim)
        for ef in s.efs:
            ox.set_ef(ef)
            o, want = ox.search_pq(s.queries, s.k), s.reference(c, ef)
            assert np.array_equal(o["cnt"], want["cnt"]), (c, ef)
            assert pq_sorted(o["dists"], o["labels"], o["cnt"]) == pq_sorted(want["dists"], want["labels"], want["cnt"]), (c, ef)
            assert np.array_equal(o["counters"][:, 0], want["calls"]), (c, ef)
    if name == "T":      # from tile stride 16 (no level-0 list above 16 ids) to 32 on the way
        gen = generator()
        assert gen.max_degree0(open(src, "rb").read()) <= 16 < gen.max_degree0(open(out, "rb").read())


@pytest.mark.parametrize("name", NAMES)
def test_fixture_covers_what_it_is_there_for(name):
    """The coverage conditions, from the reference's own account of every operation (`facts`), not from the generator's belief: at
    least 10 updates of existing labels with the enter point's and a node of level > 0 among them, 5 unmarks, a growing resize
    followed by an append beyond the old capacity, a resize to exactly the element count, a mark of the enter point; with
    replacement on, 10 flagged adds that reused a vacancy and -- from a start graph without marks -- 3 that appended."""
    gen, s = generator(), sequence(name)
    f = s.f
    cap0 = int(f["max_elements"])
    n0 = len(f["base"]) if "base" in f else int(np.fromfile(os.path.join(GOLDEN, GOLDEN_START[name] + ".hnsw.bin"), np.uint64, 3)[2])
    marks0 = name in ("G3", "G4")
    cov = gen.coverage(s.ops, f["facts"], n0, cap0)
    assert cov == {k: int(f[f"cov_{k}"]) for k in cov}
    need = dict(n_updates=10, updated_ep=1, updated_upper=1, n_unmarks=5, grow_then_append=1, exact_resize=1, marked_ep=1)
    if s.allow:
        need["n_reused"] = 10
        if not marks0:
            need["n_flag_appended"] = 3
    assert need == gen.needed(s.allow, marks0)
    assert all(cov[k] >= v for k, v in need.items()), cov
    # the checkpoints: one inside the random phase with marks present, one at its end, one after a clean-up that left no mark
    marks = f["facts"][:, 5]
    assert marks[s.checkpoints[0] - 1] > 0 and len(s.checkpoints) == (2 if marks0 else 3)
    if not marks0:
        assert marks[s.checkpoints[1] - 1] > 0 and marks[-1] == 0 and s.checkpoints[1] >= 100
    if s.allow:     # flagged and unflagged adds next to each other: one hs_index_upsert_points call of the resident index takes both
        kinds, flags = s.ops[:, 0], s.ops[:, 2]
        assert any(kinds[i] == ADD and kinds[i + 1] == ADD and flags[i] != flags[i + 1] for i in range(len(kinds) - 1))
    # what the start graphs are there for
    if name in GOLDEN_START:
        assert s.cap > n0
    elif name == "T":
        assert int(f["M"]) == 16 and n0 == 16 and s.cap == 400 and (s.ops[:, 0] == ADD).sum() > len(s.ops) // 2
    else:
        assert int(f["M"]) == 8 and n0 == 400 and f["base"].dtype == np.uint8 and f["base"].max() <= 6 and s.rows.max() <= 6


def test_generator_reproduces_the_sequences(hs, tmp_path_factory):
    """The committed operation lists, rows, bases and queries are what the generator's seeds give (the reference itself is only
    needed for what it answered)."""
    gen = generator()
    assert [q[0] for q in gen.SEQS] == NAMES
    for name, start, allow, seed0, n_random, w_append in gen.SEQS:
        s = sequence(name)
        raw = open(start_file(hs, name, tmp_path_factory), "rb").read()
        if name in GOLDEN_START:
            base = np.load(os.path.join(GOLDEN, GOLDEN_START[name].replace("_del", "") + ".npz"))["base"]
        else:
            b8, q8 = gen.seq_base(start)
            assert np.array_equal(b8, s.f["base"]) and np.array_equal(q8, s.f["queries"]), name
            base = b8.astype(np.float32)
        rng = np.random.default_rng(int(s.f["seed"]))
        ops, checkpoints = gen.gen_sequence(rng, raw, s.cap, allow, n_random, w_append, cleanup=not gen.file_marks(raw)[1].any())
        assert np.array_equal(ops, s.ops) and checkpoints == s.checkpoints and bool(allow) == s.allow, name
        assert np.array_equal(gen.new_rows(rng, base, int((ops[:, 0] == ADD).sum()), "_cont_" not in GOLDEN_START.get(name, "")), s.rows), name


@pytest.mark.parametrize("name", ["G3", "W128"])
def test_sanitised_upsert_program_on_sequences(hs, tmp_path_factory, tmp_path, name):
    """csrc/upsert_test.cpp under AddressSanitizer + UBSan, as its own binary (never inside Python), on a start graph that carries
    marks and on d = 128: the whole sequence against the reference's file (which hs_hnsw_replay reproduces, see above), every changed
    level-0 list among the touched ids, and the refusals from whatever marks the loaded graph has."""
    d = os.path.join(ROOT, "hnsw-slim_amd")
    subprocess.check_call(["make", "-C", d, "upsert_test"])
    s = sequence(name)
    src = start_file(hs, name, tmp_path_factory)
    of, rf, wf = (str(tmp_path / x) for x in ("ops.u64", "rows.f32", "want.bin"))
    s.ops.tofile(of)
    s.rows.tofile(rf)
    assert _replay(hs, s, src, wf, len(s.ops)) == s.digest(len(s.ops))
    out = subprocess.run([os.path.join(d, "upsert_test"), src, "0", str(s.dim), str(s.cap), str(int(s.allow)), of, rf, wf], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    m = re.search(r"upsert ok: (\d+) bytes compared, (\d+) touched", out.stdout)
    assert m and int(m.group(1)) == os.path.getsize(wf) and int(m.group(2)) > 100, out.stdout
