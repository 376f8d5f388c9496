#!/usr/bin/env python3
"""Generate tests/golden/updates_*.npz by RUNNING THE COMPILED REFERENCE through tests/golden/ref_updates.cpp: the reference's
own addPoint (update, replace_deleted) / markDelete / unmarkDelete / resizeIndex on the golden graphs, its saved file and its
search results afterwards.  Run by hand where the reference's headers lie (REF=...); the outputs (data, not source) are
committed, the driver's binary is built into a temporary directory and never kept.

    python tests/golden/make_golden_updates.py
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hsutil import GOLDEN, read_ref_search  # noqa: E402

REF = os.environ.get("REF", "/root/reference")
# oracle/Makefile's flags for the compiled reference (target `ref`)
REF_FLAGS = ["-std=c++17", "-O2", "-march=native", "-ffp-contract=off", "-w"]
ADD, MARK, UNMARK, RESIZE = 0, 1, 2, 3
K, EFS = 10, (10, 64)


def graph_facts(raw):
    """(count, enterpoint, levels[count]) of a vanilla index file (hnswalg.h:748-779)."""
    u = np.frombuffer(raw, np.uint64, 6, 0)
    count, spe = int(u[2]), int(u[3])
    ep = int(np.frombuffer(raw, np.uint32, 1, 52)[0])
    maxM = int(np.frombuffer(raw, np.uint64, 1, 56)[0])
    off = 96 + count * spe
    levels = np.zeros(count, np.int64)
    for i in range(count):
        sz = int(np.frombuffer(raw, np.uint32, 1, off)[0])
        levels[i] = sz // (maxM * 4 + 4)
        off += 4 + sz
    return count, ep, levels


def new_rows(rng, base, m, integer):
    """Rows near existing ones: an existing row plus noise; the integer graph's stay integers inside the fixture's own range."""
    src = base[rng.integers(0, base.shape[0], m)]
    if integer:
        return np.clip(src + rng.integers(-2, 3, src.shape), base.min(), base.max()).astype(np.float32)
    return (src + rng.standard_normal(src.shape).astype(np.float32) * 0.3 * base.std()).astype(np.float32)


def scenario_update(rng, base, raw, integer):
    """Replacement off; two marks, then 40 existing labels get new rows: the enter point, four nodes of level > 0, the two
    marked labels (which the update un-marks), the rest random; one label twice."""
    n, ep, levels = graph_facts(raw)
    upper = [int(i) for i in np.flatnonzero(levels > 0) if i != ep][:4]
    pool = [int(i) for i in rng.permutation(n) if i != ep and i not in upper]
    marked = pool[:2]
    targets = [ep] + upper + marked + pool[2:34]
    targets = [int(t) for t in rng.permutation(targets)] + [upper[0]]   # the last one a second update of the same label
    rows = new_rows(rng, base, len(targets), integer)
    ops = [(MARK, m, 0, 0) for m in marked] + [(ADD, t, 0, r) for r, t in enumerate(targets)]
    return dict(ops=ops, rows=rows, max_elements=n + 8, allow=0)


def scenario_replace(rng, base, raw, integer):
    """Loaded with room, replacement on; 30 marks, then 40 addPoint(.., true) of new labels -- 30 fill the vacancies in the
    reference's order, 10 append -- then two more marks, which stay."""
    n, ep, levels = graph_facts(raw)
    marks = [int(i) for i in rng.permutation(n)[:30]]
    if ep not in marks:
        marks[7] = ep            # the enter point among the replaced slots
    labels = [100000 + 3 * i for i in range(40)]
    rows = new_rows(rng, base, 40, integer)
    ops = [(MARK, m, 0, 0) for m in marks] + [(ADD, lab, 1, r) for r, lab in enumerate(labels)]
    stay = [labels[3], int(next(i for i in rng.permutation(n) if int(i) not in marks))]   # a successor label and an old one
    ops += [(MARK, s, 0, 0) for s in stay]
    return dict(ops=ops, rows=rows, max_elements=n + 64, allow=1)


def scenario_resize(rng, base, raw, integer):
    """Loaded full; resizeIndex(count + 50), 50 appends, then five updates (one of them of an appended label)."""
    n, ep, levels = graph_facts(raw)
    rows = new_rows(rng, base, 55, integer)
    ops = [(RESIZE, n + 50, 0, 0)] + [(ADD, 200000 + i, 0, i) for i in range(50)]
    upd = [int(i) for i in rng.permutation(n)[:4]] + [200000 + 17]
    ops += [(ADD, u, 0, 50 + j) for j, u in enumerate(upd)]
    return dict(ops=ops, rows=rows, max_elements=0, allow=0)


def main():
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "ref_updates")
        subprocess.check_call([os.environ.get("CXX", "g++"), *REF_FLAGS, "-I" + os.path.join(REF, "third_party", "hnswlib"),
                               os.path.join(GOLDEN, "ref_updates.cpp"), "-o", exe])
        for name, integer, seed in (("l2_cont_d32", False, 31), ("l2_int_d16", True, 32)):
            g = np.load(os.path.join(GOLDEN, f"{name}.npz"))
            base, queries = g["base"], np.ascontiguousarray(g["queries"], np.float32)
            src = os.path.join(GOLDEN, f"{name}.hnsw.bin")
            raw = open(src, "rb").read()
            for si, (sname, make) in enumerate((("update", scenario_update), ("replace", scenario_replace), ("resize", scenario_resize))):
                sc = make(np.random.default_rng(seed * 10 + si), base, raw, integer)
                ops = np.array(sc["ops"], np.uint64).reshape(-1, 4)
                f = {k: os.path.join(tmp, k) for k in ("ops", "rows", "out", "q", "res")}
                ops.tofile(f["ops"]); sc["rows"].tofile(f["rows"]); queries.tofile(f["q"])
                subprocess.check_call([exe, "l2", str(base.shape[1]), src, str(sc["max_elements"]), str(sc["allow"]), f["ops"], f["rows"],
                                       f["out"], f["q"], str(len(queries)), f["res"], str(K), *map(str, EFS)])
                out = {"ops": ops, "rows": sc["rows"], "max_elements": np.array(sc["max_elements"]), "allow": np.array(sc["allow"]),
                       "saved": np.frombuffer(open(f["out"], "rb").read(), np.uint8), "k": np.array(K), "efs": np.array(EFS)}
                for ef, r in read_ref_search(f["res"]).items():
                    for key, v in r.items():
                        out[f"ef{ef}_{key}"] = v
                dst = os.path.join(GOLDEN, f"updates_{sname}_{name}.npz")
                np.savez_compressed(dst, **out)
                print(dst, os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    main()
