"""Every search kernel answers a boundary tie through the one replay (csrc/search_finish.hpp), and says so.

The other tie tests compare answers; this one also asserts the PATH: on the doubled-rows graph of tests/tie_replay.py every query
of every leg is one whose k-subset hangs on the layout of the reference's result heap (tests/test_tie_replay_cpu.py holds that
premise on the oracle alone, for all 32 queries), so the flat, fast and lean kernels must each report stats column 3 == 1
("answered by the replay") for every query, with labels, distance bits, counts and the three counters equal to the oracle's on
both overloads.  The strict kernel keeps the reference's heap itself (select_and_write on it): no mark, the reference's order.

The HS_KERNEL knob is read once per process: one child per knob (fast, lean), as tests/test_gpu_value_range.py does."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import tie_replay as tr
from hsutil import ROOT, Oracle, load_product
from test_gpu_fast_shapes import compare

pytestmark = pytest.mark.gpu
P = load_product()
FLAT, FAST, STRICT, LEAN = "hs::flat_kernel", "hs::fast_kernel", "hs::strict_kernel", "hs::lean_kernel"
FIELDS = ("labels", "dists", "cnt", "stats")

_CHILD = r"""
import json
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from hsutil import load_product
hs = load_product()
jobs = json.load(open(sys.argv[2]))
q = np.fromfile(jobs["qf"], np.float32).reshape(-1, jobs["dim"])
res = {}
for c in jobs["files"]:
    for kind, path in (("slim", c["sp"]), ("hnsw", c["hp"])):
        ix = hs.Index(path, hs.HS_KIND_SLIM if kind == "slim" else hs.HS_KIND_HNSW, jobs["dim"], c["metric"])
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


def _child(folder, files, q, knob, pairs):
    qf, jobs, out = (os.path.join(folder, f"{knob}.{x}") for x in ("q.f32", "jobs.json", "npz"))
    q.tofile(qf)
    json.dump(dict(qf=qf, dim=tr.D, pairs=pairs, files=[{k: f[k] for k in ("name", "metric", "hp", "sp")} for f in files.values()]), open(jobs, "w"))
    child = subprocess.run([sys.executable, "-c", _CHILD, os.path.join(ROOT, "tests"), jobs, out], env=dict(os.environ, HS_KERNEL=knob), timeout=120)
    assert child.returncode == 0, f"the HS_KERNEL={knob} child ended with status {child.returncode}"
    return np.load(out)


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    """The files, the oracle's answers and the premise's query list per (metric, kind, ef, k), and what the two children got."""
    folder = str(tmp_path_factory.mktemp("tie_replay"))
    files, _, q = tr.build_files(P, folder)
    oracle = Oracle()
    refs = {}
    for f in files.values():
        for kind, path, call in tr.overloads(f):
            ox = oracle.load(path, kind, f["metric"], tr.D)
            for ef, k in tr.ALL_PAIRS:
                o = tr.reference(ox, q, ef, k, call)
                refs[f["name"], kind, ef, k, call] = (o, tr.through_replay(ox, q, ef, k, call, o))
    children = dict(fast=_child(folder, files, q, "fast", tr.FAST_PAIRS), lean=_child(folder, files, q, "lean", tr.LEAN_PAIRS))
    return files, q, refs, children


def check_leg(refs, name, kind, ef, k, got, kernels, kernel, replays):
    """got: {call: answer}; the answers against the oracle's (compare), the kernel that ran, and the replay mark on every query."""
    what = f"{name} {kind} ef={ef} k={k} {kernel}"
    calls = ("pq", "ids") if kind == "slim" else ("pq",)
    assert list(kernels) == [kernel] * len(calls), what
    ref = {c: refs[name, kind, ef, k, c][0] for c in calls}
    ref.setdefault("ids", None)
    compare(ref, got["pq"], got.get("ids"), False, what)
    if "ids" in got:
        assert np.array_equal(got["ids"]["cnt"], np.minimum(ref["ids"]["raw_sz"], k)), what
    for c in calls:
        need = refs[name, kind, ef, k, c][1]
        assert need.shape == (tr.NQ,) and need.all(), f"{what} {c}: the premise does not name every query"
        if replays:
            assert np.array_equal(got[c]["stats"][:, 3] == 1, need), f"{what} {c}: queries not answered by the replay: {np.flatnonzero(got[c]['stats'][:, 3] != 1).tolist()}"


def _searched(ix, q, k, slim):
    got, kernels = {"pq": ix.search_pq(q, k, want_stats=True)}, [ix.last_kernel()]
    if slim:
        got["ids"] = ix.search_ids(q, k, want_dists=True, want_stats=True)
        kernels.append(ix.last_kernel())
    return got, kernels


@pytest.mark.parametrize("name", [m for m, _ in tr.METRICS])
def test_flat_and_strict_legs(built, name):
    """The default plan (flat kernel) at both pairs, and the strict kernel by exact order: the reference's array order, no mark."""
    files, q, refs, _ = built
    f = files[name]
    for kind, path, pkind in (("slim", f["sp"], P.HS_KIND_SLIM), ("hnsw", f["hp"], P.HS_KIND_HNSW)):
        ix = P.Index(path, pkind, tr.D, f["metric"])
        for ef, k in tr.FLAT_PAIRS:
            ix.set_ef(ef)
            got, kernels = _searched(ix, q, k, kind == "slim")
            check_leg(refs, name, kind, ef, k, got, kernels, FLAT, True)
        for ef, k in tr.STRICT_PAIRS:
            ix.set_ef(ef)
            ix.set_exact_order(True)
            got, kernels = _searched(ix, q, k, kind == "slim")
            ix.set_exact_order(False)
            check_leg(refs, name, kind, ef, k, got, kernels, STRICT, False)
            if kind == "slim":
                assert np.array_equal(got["ids"]["labels"], refs[name, kind, ef, k, "ids"][0]["labels"]), f"{name} ef={ef} k={k}: strict order"
        ix.close()


@pytest.mark.parametrize("knob,kernel,pairs", [("fast", FAST, tr.FAST_PAIRS), ("lean", LEAN, tr.LEAN_PAIRS)])
@pytest.mark.parametrize("name", [m for m, _ in tr.METRICS])
def test_knob_legs(built, name, knob, kernel, pairs):
    """What the HS_KERNEL=fast / HS_KERNEL=lean children got on the same files."""
    _, _, refs, children = built
    child = children[knob]
    for kind in ("slim", "hnsw"):
        for ef, k in pairs:
            key = f"{name}/{kind}/{ef}/{k}"
            got = {c: {field: child[f"{key}/{c}/{field}"] for field in FIELDS} for c in (("pq", "ids") if kind == "slim" else ("pq",))}
            check_leg(refs, name, kind, ef, k, got, child[key + "/kernels"].tolist(), kernel, True)
