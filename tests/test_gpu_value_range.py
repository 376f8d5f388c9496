"""Every distance kernel at the edges of the fp32 range, bit for bit against the oracle (whose recipes tests/test_oracle_golden.py
pins to the compiled reference at the same ranges, tests/golden/dist_ref_range.npz).

The rest of the suite runs on integers 0..255, mixtures with |x| in the tens, or unit vectors: L2 distances are normal floats
between 1 and 1e6, IP distances all in [0, 2] or all far below zero.  Here (tests/value_range.py) one base draw is multiplied by a
power of two, exactly, so that
  * ip_cross: 1 - <q, x> changes sign inside one query's result array -- the sign-folded int32 key images of the flat and lean
    kernels (dkey<METRIC_IP>) order a set that holds both signs;
  * l2_subnormal: every product, partial sum and distance is a subnormal float -- the packed-f32 multiplies and adds, the fma chains,
    the DPP reductions and cross-lane sums keep them, as the reference compiled without fast-math does;
  * large: distances above 2^100 next to the FLT_MAX sentinels and reduction identities;
  * ip_ones: <q, x> vanishes against 1, every distance is exactly 1.0f: all ties, the tie replay decides everything;
  * l2_overflow (exhaustive scans only): squared differences overflow, +inf distances are answers like any other.

The distance table: hs_brute_force with k = n returns every (query, row) distance, nothing hidden behind a top-k, at every recipe
(scalar, SIMD4, SIMD4 + rest, SIMD16 + rest, SIMD16; both metrics; both scan kernels), and hs_index_exact_search the same at one dim
per scan kernel.  The graph kernels: flat, fast (k = 100, filter, delete marks), strict (exact order, ef = 600), lean (a child
process), SlimQ, and convertFromHNSW on the GPU, each leg asserting the kernel it ran on.  No tolerance anywhere in this file.

Not run on a device, by contract (include/hnsw_slim_amd.h): non-finite inputs, IP distances that overflow, +inf in a graph kernel."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import value_range as vr
from hsutil import GOLDEN, ROOT, Oracle, load_product
from test_gpu_bruteforce import _expect
from test_gpu_convert import _same_file
from test_gpu_fast_shapes import compare
from test_gpu_slimq import build as slimq_build, check as slimq_check
from test_oracle_golden import range_pairs

pytestmark = pytest.mark.gpu
L2, IP = vr.L2, vr.IP
P = load_product()
FLAT, FAST, STRICT, LEAN = "hs::flat_kernel", "hs::fast_kernel", "hs::strict_kernel", "hs::lean_kernel"
CASES = vr.cases()
IDS = [vr.case_name(c) for c in CASES]
TABLE = list(range_pairs())
EXACT_DIMS = {128: "hs::exact_scan_kernel", 100: "hs::exact_scan_general_kernel"}


@pytest.fixture(scope="module")
def oracle_lib():
    return Oracle()


# ---- the distance table ---------------------------------------------------------------------------------------------------

def table_of(labels, dists, cnt, n):
    """The n x n table of a k = n answer, by (query, label)."""
    assert np.all(cnt == n)
    order = np.argsort(labels, axis=1, kind="stable")
    assert np.array_equal(np.take_along_axis(labels, order, 1), np.tile(np.arange(n, dtype=np.uint64), (len(labels), 1)))
    return np.take_along_axis(dists, order, 1)


def check_table(oracle_lib, got, metric, a, b, fixture, what):
    """got = (labels, dists, cnt) of queries a over rows b with k = n: the lexsort on (dist, label) of Oracle.dist's table, the whole
    table bit for bit, the diagonal the compiled reference's."""
    n = len(b)
    labels, dists, cnt = got
    table = table_of(labels, dists, cnt, n)
    want = vr.dist_table(oracle_lib, metric, b, a)
    assert np.array_equal(table.view(np.uint32), want.view(np.uint32)), what
    assert np.diagonal(table).tobytes() == fixture.tobytes(), what
    el, ed = _expect(oracle_lib, metric, b, a, n)
    assert np.array_equal(labels, el) and np.array_equal(dists.view(np.uint32), ed.view(np.uint32)), what
    return want


@pytest.mark.parametrize("key,metric,a,b", TABLE, ids=[t[0][:-4] for t in TABLE])
def test_distance_table_brute_force(oracle_lib, key, metric, a, b):
    """bf_scan_kernel (dim % 16 == 0) and bf_scan_general_kernel at every recipe and scale; s = 62 is the +inf leg."""
    assert len(TABLE) >= 60
    fixture = np.load(os.path.join(GOLDEN, "dist_ref_range.npz"))[key]
    n = len(b)
    assert n in (16, 64)
    want = check_table(oracle_lib, P.brute_force(b, a, n, metric), metric, a, b, fixture, key)
    if key.endswith("_s62_ref"):
        assert np.isposinf(want).any() and not np.isnan(want).any(), f"{key}: premise: +inf distances, no NaN"
    else:
        assert np.all(np.isfinite(want)), key
        if key.endswith("_s-70_ref") and metric == L2:
            assert ((want != 0) & (want < vr.SUBNORMAL)).any(), f"{key}: premise: subnormal distances"


EXACT_TABLE = [t for t in TABLE if int(t[0].split("_")[1]) in EXACT_DIMS]


@pytest.mark.parametrize("key,metric,a,b", EXACT_TABLE, ids=[t[0][:-4] for t in EXACT_TABLE])
def test_distance_table_exact_search(oracle_lib, tmp_path, key, metric, a, b):
    """The same table through hs_index_exact_search on an index built over the scaled rows, one dim per scan kernel."""
    assert len(EXACT_TABLE) == 10
    d, n = b.shape[1], len(b)
    fixture = np.load(os.path.join(GOLDEN, "dist_ref_range.npz"))[key]
    hp, sp = str(tmp_path / "h.bin"), str(tmp_path / "s.bin")
    P.build_hnsw(b, hp, metric=metric, M=8, ef_construction=40, threads=1)
    P.convert_slim(hp, sp, d, metric=metric, threads=4)
    ix = P.Index(sp, P.HS_KIND_SLIM, d, metric)
    assert np.array_equal(ix.labels(), np.arange(n, dtype=np.uint64))
    r = ix.exact_search(a, n)
    assert ix.last_kernel() == EXACT_DIMS[d], key
    check_table(oracle_lib, (r["labels"], r["dists"], r["cnt"]), metric, a, b, fixture, key)
    ix.close()


def test_l2_overflow_family(oracle_lib, tmp_path):
    """130 rows, k = 64: per query 25 .. 130 distances are finite, so some answers end in +inf entries (ordered by label) and
    some do not; three row chunks, twelve sorted runs to merge.  hnswlib::BruteforceSearch::searchKnn keeps a +inf distance like
    any other (`inf <= inf`), so every query has k results."""
    base, q = vr.overflow_rows_and_queries()
    k, d = vr.OVERFLOW_K, vr.OVERFLOW_DIM
    vr.check_overflow(vr.dist_table(oracle_lib, L2, base, q), k, "l2_overflow")
    el, ed = _expect(oracle_lib, L2, base, q, k)
    assert np.isposinf(ed[:, -1]).any() and np.isfinite(ed[:, -1]).any()
    gl, gd, gc = P.brute_force(base, q, k, L2)
    assert np.all(gc == k)
    assert np.array_equal(gl, el) and np.array_equal(gd.view(np.uint32), ed.view(np.uint32))
    hp, sp = str(tmp_path / "h.bin"), str(tmp_path / "s.bin")
    P.build_hnsw(base, hp, metric=L2, M=8, ef_construction=40, threads=1)
    P.convert_slim(hp, sp, d, metric=L2, threads=4)
    ix = P.Index(sp, P.HS_KIND_SLIM, d, L2)
    r = ix.exact_search(q, k)
    assert ix.last_kernel() == "hs::exact_scan_kernel"
    assert np.all(r["cnt"] == k)
    assert np.array_equal(r["labels"], el) and np.array_equal(r["dists"].view(np.uint32), ed.view(np.uint32))
    ix.close()


# ---- the graph kernels ----------------------------------------------------------------------------------------------------

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
            planned = hs.debug_search_plan(hs.debug_plan_input(ix, k, len(q)))["name"]
            calls = [("pq", ix.search_pq(q, k, want_stats=True))]
            kernels = [planned, ix.last_kernel()]
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
    """Every case's two files, and the answers of the one HS_KERNEL=lean child (the knob is read once per process) over all of them.
    A child that fails fails this fixture, and with it every graph test of the module before it touches the device."""
    folder = str(tmp_path_factory.mktemp("value_range"))
    files = {case: vr.build_files(P, case, folder) for case in CASES}
    for f in files.values():
        f["qf"] = os.path.join(folder, f["name"] + ".q.f32")
        f["q"].tofile(f["qf"])
    jobs, out = os.path.join(folder, "jobs.json"), os.path.join(folder, "child.npz")
    keep = ("name", "metric", "dim", "hp", "sp", "qf")
    json.dump(dict(cases=[{k: f[k] for k in keep} for f in files.values()], pairs=vr.LEAN_PAIRS), open(jobs, "w"))
    child = subprocess.run([sys.executable, "-c", _CHILD, os.path.join(ROOT, "tests"), jobs, out], env=dict(os.environ, HS_KERNEL="lean"),
                           timeout=300)
    assert child.returncode == 0, f"the HS_KERNEL=lean child ended with status {child.returncode}"
    return files, np.load(out)


def searched(ix, q, k, slim, kernel, what):
    g = ix.search_pq(q, k, want_stats=True)
    assert ix.last_kernel() == kernel, what
    r = None
    if slim:
        r = ix.search_ids(q, k, want_dists=True, want_stats=True)
        assert ix.last_kernel() == kernel, what
    return g, r


def tie_replays(ref, g, r, what):
    """ip_ones: every key is equal, so nothing but the re-run with the reference's heap mechanics gives its k-subset; the kernel
    must report it (stats column 3 == 1) wherever vr.reference says the leg has one."""
    if ref["replay"]:
        for name, x in (("pq", g), ("ids", r)):
            assert x is None or (x["stats"][:, 3] == 1).any(), f"{what} {name}: no tie replay"


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_bare_legs(built, oracle_lib, case):
    """flat (dim % 16 == 0; the any-dim shapes are the fast kernel's), fast at k = 100, strict by exact order and by ef = 600."""
    f = built[0][case]
    family, metric, d, _ = case
    q = f["q"]
    flat = FLAT if d % 16 == 0 else FAST
    for kind, path, pkind in (("slim", f["sp"], P.HS_KIND_SLIM), ("hnsw", f["hp"], P.HS_KIND_HNSW)):
        ix, ox = P.Index(path, pkind, d, metric), oracle_lib.load(path, kind, metric, d)
        slim = kind == "slim"
        legs = [(p, flat, False) for p in vr.FLAT_PAIRS] + [(p, FAST, False) for p in vr.FAST_PAIRS]
        legs += [((70, 10), STRICT, True)] + [(p, STRICT, False) for p in vr.STRICT_PAIRS]
        for (ef, k), kernel, exact_order in legs:
            what = f"{f['name']} {kind} ef={ef} k={k} {kernel}"
            ref = vr.reference(ox, family, d, q, ef, k, slim, what)
            ix.set_ef(ef)
            ix.set_exact_order(exact_order)
            g, r = searched(ix, q, k, slim, kernel, what)
            ix.set_exact_order(False)
            compare(ref, g, r, False, what)
            if kernel != STRICT:   # (the strict kernel keeps the reference's order itself: it has no replay to report)
                tie_replays(ref, g, r, what)
        ix.close()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_filter_and_delete_mark_legs(built, oracle_lib, case, tmp_path):
    """The vanilla file under a filter that allows half the labels, then with a tenth of them delete-marked (against the oracle on
    the marked file as saved): the fast kernel's !bare shapes."""
    f = built[0][case]
    family, metric, d, _ = case
    q, n = f["q"], f["n"]
    ix = P.Index(f["hp"], P.HS_KIND_HNSW, d, metric, max_elements=n + 1)    # a spare slot keeps the host image for save()
    labels = ix.labels()
    allowed, marks = vr.allowed_half(labels), vr.marked_tenth(labels)
    fx = oracle_lib.load(f["hp"], "hnsw", metric, d)
    fx.set_filter(allowed)
    for leg in ("filter", "marks"):
        if leg == "marks":
            ix.mark_deleted(marks)
            assert ix.info()["has_deleted"] == 1 and ix.deleted_count() == len(marks)
            saved = str(tmp_path / "marked.bin")
            ix.save(saved)
            ox = oracle_lib.load(saved, "hnsw", metric, d)
        else:
            ox = fx
        for ef, k in vr.NOT_BARE_PAIRS:
            what = f"{f['name']} {leg} ef={ef} k={k}"
            ref = vr.reference(ox, family, d, q, ef, k, False, what)
            ix.set_ef(ef)
            g = ix.search_filtered(q, k, allowed, want_stats=True) if leg == "filter" else ix.search_pq(q, k, want_stats=True)
            assert ix.last_kernel() == FAST, what
            compare(ref, g, None, False, what)
            tie_replays(ref, g, None, what)
    ix.close()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_lean_legs(built, oracle_lib, case):
    """What the HS_KERNEL=lean child got on the same files: the lean kernel where the plan has one (dim % 16 == 0), the fast kernel
    elsewhere -- the name the plan reports in that process, and the kernel that then ran."""
    files, child = built
    f = files[case]
    family, metric, d, _ = case
    for kind, path in (("slim", f["sp"]), ("hnsw", f["hp"])):
        ox = oracle_lib.load(path, kind, metric, d)
        slim = kind == "slim"
        for ef, k in vr.LEAN_PAIRS:
            what = f"{f['name']} {kind} ef={ef} k={k} (HS_KERNEL=lean)"
            key = f"{f['name']}/{kind}/{ef}/{k}"
            assert child[key + "/kernels"].tolist() == [LEAN if d % 16 == 0 else FAST] * (3 if slim else 2), what
            ref = vr.reference(ox, family, d, f["q"], ef, k, slim, what)
            got = {call: {field: child[f"{key}/{call}/{field}"] for field in ("labels", "dists", "cnt", "stats")} for call in (("pq", "ids") if slim else ("pq",))}
            compare(ref, got["pq"], got.get("ids"), False, what)
            tie_replays(ref, got["pq"], got.get("ids"), what)


def test_slimq_ip_cross(oracle_lib, tmp_path):
    """HNSW-SlimQ over the ip_cross rows at d = 128 (not normalised, <q, x> on both sides of 1 across the rows the beam re-ranks).
    t_const is stated (31.0, as tests/test_gpu_slimq.py states it for its other 128-bit-code IP index): both sides use that value."""
    case = next(c for c in CASES if c[0] == "ip_cross" and c[2] == 128)
    base, q = vr.rows_and_queries(case)
    path = slimq_build(P, tmp_path, "ip_cross", base, IP, 8)
    ix, ox = slimq_check(P, oracle_lib, path, base, q, IP, 10, (40, 200), t_const=31.0)
    assert ix.last_kernel() == "hs::slimq_kernel"
    assert np.all(ox.search(q, 10, threads=8)["counts"] == 10)


CONVERT = [c for c in CASES if c[0] in ("ip_cross", "l2_subnormal", "large") and c[2] in (128, 20)]


@pytest.mark.parametrize("case", CONVERT, ids=[vr.case_name(c) for c in CONVERT])
def test_convert_on_the_gpu(built, oracle_lib, case, tmp_path):
    """getNeighborsByHeuristic2's prune through the same ranges: GPU file == host file == oracle file."""
    f = built[0][case]
    _same_file(P, oracle_lib, f["hp"], f["dim"], f["metric"], tmp_path)
