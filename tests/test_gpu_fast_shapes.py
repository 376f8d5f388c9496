"""The fast kernel (csrc/beam_search.hip hs::fast_kernel) at every dim it has a distance pass compiled for, through the calls that
reach it.  The flat kernel answers a bare index with dim % 16 == 0 only up to k = 64, so a plain top-100 call on a SIFT-, DEEP-,
GIST- or COHERE-shaped index is a fast-kernel call: the compile-time-dim branch of the fp32 fast launchers (fast_launch_d16), S = 2, 4, 8
slots per lane by ef, the boundary-watching variant when ef == k.

The dims are not typed in: every (metric, dim) hs_debug_fast_shape reports as compiled (the table the launchers dispatch on), one
runtime-dim control per metric, and two extra data kinds.  Per case a Slim file and the vanilla file it was converted from
(as tests/test_gpu_flat_wide.py builds them), 64 queries, against the oracle:
  * in process, the (ef, k) pairs of PAIRS -- the kernel name, the counts, the sorted (fp32 distance bits, label) lists of the
    (q, k) overload on both files, and on the Slim file the sorted label sets, distance bits and traversal counters of search_ids;
  * S = 1 and the boundary watch at S = 1 (ef <= 64 with k <= 64 is a flat-kernel call) in ONE child process per module run with
    HS_KERNEL=fast, the same files and assertions, CHILD_PAIRS;
  * on the d = 128 L2 and the d = 768 IP vanilla files (and the runtime-dim shapes those leave out): delete marks on a tenth of
    the rows and a filter that allows half of them (the !bare shapes, S = 1, 2, 4, 8), and the d = 128 L2 Slim index as u8 rows
    alone (hs::fast_kernel_u8).
Everything is bit for bit; there is no tolerance in this file.  Premises, asserted on the oracle's side before anything is compared:
every query of every leg gets exactly k results; on integer rows every ef > k leg has a query whose k-th and (k+1)-th distances are
equal and every ef == k leg has a query that evicts a key equal to the last kept one (the oracle's tie_evictions) -- and the kernel
reports a tie replay (stats column 3 == 1) on those legs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from hsutil import ROOT, Oracle, load_product
from test_gpu_flat_wide import _rows
from test_gpu_parity import _pq_sorted

pytestmark = pytest.mark.gpu
L2, IP = 0, 1
P = load_product()
FAST = "hs::fast_kernel"
# (ef, k): the boundary watch at S = 2 (twice), S = 2, S = 4 at both ends, S = 8 at both ends
PAIRS = ((100, 100), (70, 70), (128, 65), (129, 100), (256, 100), (257, 100), (512, 200))
# HS_KERNEL=fast only: the boundary watch at S = 1 (twice), S = 1 (twice)
CHILD_PAIRS = ((10, 10), (64, 64), (32, 10), (64, 10))
NOT_BARE_PAIRS = ((100, 10), (100, 100), (300, 10), (300, 100), (64, 10), (200, 10))   # S = 2, (strict), 8, 8, 1, 4
NQ = 64


def _cases():
    """(metric, dim, integer rows): L2 dims on tie-heavy integer rows, IP dims on continuous unit vectors."""
    out = []
    for metric in (L2, IP):
        compiled = [d for d in range(4, 1601) if P.debug_fast_shape(metric, d, 100, 100, True)["d16"] not in (0, -1)]
        assert compiled, "hs_debug_fast_shape reports no compiled dim"
        out += [(metric, d, metric == L2) for d in compiled]
    out += [(L2, 160, True), (IP, 384, False)]       # the runtime-dim shape of each metric: the control
    out += [(L2, 70, True), (IP, 70, False)]         # ... and the any-dim one (dim % 16 != 0), so that every shape there is runs here
    out += [(L2, 128, False), (IP, 768, True)]       # the other data kind at the two headline dims
    return out


CASES = _cases()
# the cases that also run the !bare legs: d = 128 L2 (the one compiled-dim !bare shape), an IP index with dim % 16 == 0, and the two
# runtime-dim shapes of each metric that those leave out
NOT_BARE = ((L2, 128, True), (IP, 768, False), (L2, 160, True), (L2, 70, True), (IP, 70, False))
NARROW = (L2, 128, True)                            # ... and the u8 leg


def _name(case):
    metric, d, integer = case
    return f"{'l2' if metric == L2 else 'ip'}-d{d}-{'int' if integer else 'cont'}"


def build_case(case, folder):
    """The two files and the queries of a case."""
    metric, d, integer = case
    n = 6000 if d <= 128 else 2500
    base, q = _rows(n, d, 31 + d, integer, metric), _rows(NQ, d, 77 + d, integer, metric)
    hp, sp, qf = (os.path.join(folder, f"{_name(case)}.{x}") for x in ("h.bin", "s.bin", "q.f32"))
    P.build_hnsw(base, hp, metric=metric, M=12, ef_construction=80, threads=8)
    P.convert_slim(hp, sp, d, metric=metric, threads=8)
    q.tofile(qf)
    return dict(name=_name(case), metric=metric, dim=d, integer=integer, n=n, hp=hp, sp=sp, qf=qf, q=q)


def kth_ties(raw_d, raw_sz, k):
    """Queries whose k-th and (k+1)-th result distances are equal (raw result arrays of the oracle, raw_sz entries each)."""
    out = np.zeros(len(raw_sz), bool)
    for i, n in enumerate(raw_sz):
        d = np.sort(raw_d[i, :n])
        out[i] = n > k and d[k - 1] == d[k]
    return out


def k_smallest_bits(raw_d, raw_sz, k):
    return np.stack([np.sort(raw_d[i, :n])[:k] for i, n in enumerate(raw_sz)]).view(np.uint32)


def reference(ox, q, ef, k, integer, ids, what):
    """The oracle's answer of one leg with the premises checked: exactly k results everywhere, and on integer rows the ties that
    make the kernel replay.  ids: also the (q, k, tableint*) overload (Slim files)."""
    ox.set_ef(ef)
    ref = dict(pq=ox.search_pq(q, k, threads=8), ids=ox.search_ids(q, k, threads=8) if ids else None)
    for name, o in ref.items():
        if o is None:
            continue
        assert np.all(o["raw_sz"] >= k) and (name != "pq" or np.all(o["cnt"] == k)), f"{what} {name}: a query has fewer than k results"
        if integer and ef > k:
            assert kth_ties(o["raw_d"], o["raw_sz"], k).any(), f"{what} {name}: no query ties across the k-th boundary"
        if integer and ef == k:
            assert (ox.tie_evictions(q, k, name == "pq", threads=8) > 0).any(), f"{what} {name}: no query evicts a key equal to the last kept one"
    return ref


def compare(ref, got_pq, got_ids, integer, what):
    """One leg of the kernel against reference(): got_pq / got_ids as Index.search_pq / search_ids return them (with stats)."""
    o = ref["pq"]
    assert np.array_equal(got_pq["cnt"], o["cnt"]), what
    assert _pq_sorted(got_pq["dists"], got_pq["labels"], got_pq["cnt"]) == _pq_sorted(o["dists"], o["labels"], o["cnt"]), what
    assert np.array_equal(got_pq["stats"][:, :3], o["counters"][:, :3]), what
    if integer:
        assert (got_pq["stats"][:, 3] == 1).any(), f"{what}: no tie replay"
    if got_ids is not None:
        oi = ref["ids"]
        k = oi["labels"].shape[1]
        assert np.array_equal(np.sort(got_ids["labels"], 1), np.sort(oi["labels"], 1)), what
        assert np.array_equal(np.sort(got_ids["dists"], 1).view(np.uint32), k_smallest_bits(oi["raw_d"], oi["raw_sz"], k)), what
        assert np.array_equal(got_ids["stats"][:, :3], oi["counters"][:, :3]), what
        if integer:
            assert (got_ids["stats"][:, 3] == 1).any(), f"{what} ids: no tie replay"


_CHILD = r"""
import json
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from hsutil import load_product
hs = load_product()
jobs = json.load(open(sys.argv[2]))
res = {}
for c in jobs["cases"]:
    q = np.fromfile(c["qf"], np.float32).reshape(-1, c["dim"])
    for kind, path in (("slim", c["sp"]), ("hnsw", c["hp"])):
        ix = hs.Index(path, hs.HS_KIND_SLIM if kind == "slim" else hs.HS_KIND_HNSW, c["dim"], c["metric"])
        for ef, k in jobs["pairs"]:
            key = f"{c['name']}/{kind}/{ef}/{k}"
            ix.set_ef(ef)
            calls = [("pq", ix.search_pq(q, k, want_stats=True))]
            kernels = [ix.last_kernel()]
            if kind == "slim":
                calls.append(("ids", ix.search_ids(q, k, want_dists=True, want_stats=True)))
                kernels.append(ix.last_kernel())
            res[key + "/kernels"] = np.array(kernels)
            for call, r in calls:
                for field in ("labels", "dists", "cnt", "stats"):
                    res[f"{key}/{call}/{field}"] = r[field]
        ix.close()
np.savez(sys.argv[3], **res)
"""


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    """Every case's files, and the answers of the one HS_KERNEL=fast child (the knob is read once per process) over all of them.
    A child that fails fails this fixture, and with it every test of the module before it touches the device."""
    folder = str(tmp_path_factory.mktemp("fast_shapes"))
    files = {case: build_case(case, folder) for case in CASES}
    jobs, out = os.path.join(folder, "jobs.json"), os.path.join(folder, "child.npz")
    json.dump(dict(cases=[{k: v for k, v in f.items() if k != "q"} for f in files.values()], pairs=CHILD_PAIRS), open(jobs, "w"))
    child = subprocess.run([sys.executable, "-c", _CHILD, os.path.join(ROOT, "tests"), jobs, out], env=dict(os.environ, HS_KERNEL="fast"),
                           timeout=300)
    assert child.returncode == 0, f"the HS_KERNEL=fast child ended with status {child.returncode}"
    return files, np.load(out)


@pytest.fixture(scope="module")
def oracle_lib():
    return Oracle()


@pytest.mark.parametrize("case", CASES, ids=[_name(c) for c in CASES])
def test_fast_kernel_shape(built, oracle_lib, case, tmp_path):
    files, child = built
    f = files[case]
    metric, d, integer = case
    q = f["q"]
    for kind, path, pkind in (("slim", f["sp"], P.HS_KIND_SLIM), ("hnsw", f["hp"], P.HS_KIND_HNSW)):
        ix, ox = P.Index(path, pkind, d, metric), oracle_lib.load(path, kind, metric, d)
        slim = kind == "slim"
        for ef, k in PAIRS:
            what = f"{f['name']} {kind} ef={ef} k={k}"
            ref = reference(ox, q, ef, k, integer, slim, what)
            ix.set_ef(ef)
            g = ix.search_pq(q, k, want_stats=True)
            assert ix.last_kernel() == FAST, what
            r = None
            if slim:
                r = ix.search_ids(q, k, want_dists=True, want_stats=True)
                assert ix.last_kernel() == FAST, what
            compare(ref, g, r, integer, what)
            if slim and case == NARROW and (ef, k) == (256, 100):   # the same index as u8 rows alone: the same bits
                ix.set_row_format(P.HS_ROWS_U8)
                ix.set_f32_resident(False)
                g8 = ix.search_pq(q, k, want_stats=True)
                assert ix.last_kernel() == FAST + "_u8", what
                r8 = ix.search_ids(q, k, want_dists=True, want_stats=True)
                assert ix.last_kernel() == FAST + "_u8", what
                for a, b in ((g, g8), (r, r8)):
                    for field in ("labels", "dists", "cnt", "stats"):
                        assert a[field].dtype == b[field].dtype and a[field].tobytes() == b[field].tobytes(), f"{what} u8 {field}"
                ix.set_f32_resident(True)
                ix.set_row_format(P.HS_ROWS_F32)
        for ef, k in CHILD_PAIRS:   # what the HS_KERNEL=fast child got on the same file
            what = f"{f['name']} {kind} ef={ef} k={k} (HS_KERNEL=fast)"
            key = f"{f['name']}/{kind}/{ef}/{k}"
            assert child[key + "/kernels"].tolist() == [FAST] * (2 if slim else 1), what
            ref = reference(ox, q, ef, k, integer, slim, what)
            got = {call: {field: child[f"{key}/{call}/{field}"] for field in ("labels", "dists", "cnt", "stats")} for call in (("pq", "ids") if slim else ("pq",))}
            compare(ref, got["pq"], got.get("ids"), integer, what)
    if case in NOT_BARE:
        not_bare_legs(oracle_lib, f, str(tmp_path))


def not_bare_legs(oracle_lib, f, folder):
    """The vanilla file with a tenth of its rows delete-marked (against the oracle on the marked file as saved) and under a filter
    that allows half of them: the !bare shapes, S = 1, 2, 4, 8.  ef == k is not a fast-kernel call here -- the boundary watch is
    compiled for bare indexes only, fast_supported hands it to the strict kernel -- and is compared all the same."""
    metric, d, integer, n = f["metric"], f["dim"], f["integer"], f["n"]
    q = f["q"]
    ix = P.Index(f["hp"], P.HS_KIND_HNSW, d, metric, max_elements=n + 1)    # a spare slot keeps the host image for save()
    labels = ix.labels()
    allowed = ((labels * 7 + 3) % 10 < 5).astype(np.uint8)
    marks = labels[labels % 10 == 3]
    fx = oracle_lib.load(f["hp"], "hnsw", metric, d)
    fx.set_filter(allowed)
    mx = None
    for leg in ("filter", "marks"):
        if leg == "marks":
            ix.mark_deleted(marks)
            assert ix.info()["has_deleted"] == 1 and ix.deleted_count() == len(marks)
            saved = os.path.join(folder, "marked.bin")
            ix.save(saved)
            mx = oracle_lib.load(saved, "hnsw", metric, d)
        for ef, k in NOT_BARE_PAIRS:
            what = f"{f['name']} {leg} ef={ef} k={k}"
            ox = fx if leg == "filter" else mx
            ox.set_ef(ef)
            o = ox.search_pq(q, k, threads=8)
            assert np.all(o["cnt"] == k), f"{what}: a query has fewer than k results"
            if integer and ef > k:
                assert kth_ties(o["raw_d"], o["raw_sz"], k).any(), f"{what}: no query ties across the k-th boundary"
            ix.set_ef(ef)
            g = ix.search_filtered(q, k, allowed, want_stats=True) if leg == "filter" else ix.search_pq(q, k, want_stats=True)
            assert ix.last_kernel() == (FAST if ef > k else "hs::strict_kernel"), what
            compare(dict(pq=o, ids=None), g, None, integer and ef > k, what)
