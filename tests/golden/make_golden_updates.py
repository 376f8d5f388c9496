#!/usr/bin/env python3
"""Generate tests/golden/updates_*.npz by RUNNING THE COMPILED REFERENCE through tests/golden/ref_updates.cpp: the reference's
own addPoint (update, replace_deleted) / markDelete / unmarkDelete / resizeIndex on the golden graphs, its saved file and its
search results afterwards -- for the three hand-written scenarios (updates_<scenario>_<graph>.npz), and for seeded random legal
sequences of 100+ interleaved operations (updates_seq_<name>.npz: the SHA-256 of the reference's saved file after every operation, its
search results at two or three checkpoints, its own account of every operation; no saved file).  Run by hand where the reference's headers lie (REF=...); the outputs (data, not source) are
committed, the driver's binary is built into a temporary directory and never kept.

    python tests/golden/make_golden_updates.py [scenarios] [seq]
"""
import hashlib
import os
import subprocess
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hsutil import GOLDEN, ROOT, mixture, read_ref_search, write_fvecs  # noqa: E402

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


# ---- random legal sequences (updates_seq_<name>.npz) ------------------------------------------------------------------------------
# (name, start graph: a golden name or (n, dim, M, efC, data seed), replacement, seed, operations in the random phase, weight of appends)
W_ROWS = dict(lo=1.0, hi=5.0, sigma=1.0)      # tie-heavy integer rows, clipped to 0..6
SEQS = [
    ("G1", "l2_int_d16", 1, 101, 110, 2), ("G1off", "l2_int_d16", 0, 102, 110, 2), ("G2", "l2_cont_d32", 1, 103, 110, 2),
    ("G3", "l2_int_d16_del", 1, 104, 110, 2), ("G4", "l2_cont_d32_del", 1, 105, 110, 2),
    ("W32", (400, 32, 8, 60, 51), 1, 106, 100, 2), ("W128", (400, 128, 8, 60, 52), 1, 107, 100, 2),
    ("W320", (400, 320, 8, 60, 53), 1, 108, 100, 2), ("W960", (400, 960, 8, 60, 54), 1, 109, 100, 2),
    ("T", (16, 32, 16, 80, 55), 0, 110, 100, 14),
]
FACTS = ("reused", "id", "level", "ep_before", "count", "marks", "capacity", "maxlevel")
# what every sequence that allows it must hold (the CPU test asserts the same figures from the fixture's own fields)
NEED = dict(n_updates=10, updated_ep=1, updated_upper=1, n_unmarks=5, n_reused=10, n_flag_appended=3, grow_then_append=1,
            exact_resize=1, marked_ep=1)


def seq_base(start):
    """(base, queries) of a W / T start graph: uint8-valued rows."""
    n, dim, M, efc, seed = start
    kw = W_ROWS if M == 8 else {}
    hi = 6 if M == 8 else 255
    return (np.clip(mixture(n, dim, seed, integer=True, **kw), 0, hi).astype(np.uint8),
            np.clip(mixture(40, dim, seed + 100, integer=True, **kw), 0, hi).astype(np.uint8))


def file_marks(raw):
    """(labels[count], marked[count]) of a vanilla index file."""
    u = np.frombuffer(raw, np.uint64, 6, 0)
    count, spe, label_off = int(u[2]), int(u[3]), int(u[4])
    el = np.frombuffer(raw, np.uint8, count * spe, 96).reshape(count, spe)
    return el[:, label_off:label_off + 8].copy().view(np.uint64)[:, 0], (el[:, 2] & 1) != 0


def max_degree0(raw):
    u = np.frombuffer(raw, np.uint64, 6, 0)
    count, spe = int(u[2]), int(u[3])
    return int(np.frombuffer(raw, np.uint8, count * spe, 96).reshape(count, spe)[:, 0:2].copy().view(np.uint16).max())


def gen_sequence(rng, raw, cap0, allow, n_random, w_append, cleanup):
    """A legal operation list: (ops, checkpoints).  Which vacancy a flagged add takes is the reference's to decide, so once one may
    have reused a slot no label that was marked at that moment is named again (`marked` holds the marked labels that still may)."""
    n0, ep, levels = graph_facts(raw)
    labels, is_marked = file_marks(raw)
    live = [int(l) for l, m in zip(labels, is_marked) if not m]
    marked = [int(l) for l, m in zip(labels, is_marked) if m]
    st = dict(n_marked=len(marked), count=n0, cap=cap0, next_label=1000000, rows=0)
    ops, marks_after = [], []

    def emit(kind, arg, flag=0):
        ops.append((kind, arg, flag, st["rows"] if kind == ADD else 0))
        st["rows"] += kind == ADD
        marks_after.append(st["n_marked"])

    def take(pool):
        return pool.pop(int(rng.integers(0, len(pool))))

    def mark(lab=None):
        lab = take(live) if lab is None else live.pop(live.index(lab))
        marked.append(lab); st["n_marked"] += 1
        emit(MARK, lab)

    def unmark(lab=None):
        lab = take(marked) if lab is None else marked.pop(marked.index(lab))
        live.append(lab); st["n_marked"] -= 1
        emit(UNMARK, lab)

    def update(lab=None):
        emit(ADD, live[int(rng.integers(0, len(live)))] if lab is None else lab)

    def update_marked():
        lab = take(marked)
        live.append(lab); st["n_marked"] -= 1
        emit(ADD, lab)

    def new_label():
        st["next_label"] += int(rng.integers(1, 4))
        return st["next_label"]

    def append():
        lab = new_label()
        live.append(lab); st["count"] += 1
        emit(ADD, lab)

    def flagged():
        if st["n_marked"] > 0:
            marked.clear(); st["n_marked"] -= 1
        elif st["count"] < st["cap"]:
            st["count"] += 1
        else:
            return False
        lab = new_label()
        live.append(lab)
        emit(ADD, lab, 1)
        return True

    def resize(to=None):
        st["cap"] = st["count"] + int(rng.integers(0, 20)) if to is None else to
        emit(RESIZE, st["cap"])

    # the enter point's label and a node of level > 0: updated, and the enter point marked, before any slot can change its label
    ep_label = int(labels[ep])
    upper = int(labels[next(i for i in np.flatnonzero(levels > 0) if i != ep and not is_marked[i])])
    if ep_label in marked:
        unmark(ep_label)
    update(ep_label); update(upper); mark(ep_label)
    start, resized = len(ops), False
    while len(ops) < start + n_random:
        if not resized and len(ops) >= start + n_random // 3:      # a resize to exactly the count, a growing one, an append beyond the old capacity
            resize(st["count"]); resize(st["count"] + int(rng.integers(1, 20))); append()
            resized = True
            continue
        kinds = [("mark", 4 if len(live) > 12 else 0), ("unmark", 3 if marked else 0), ("update", 3),
                 ("update_marked", 1 if marked and not allow else 0), ("append", w_append if st["count"] < st["cap"] else 0),
                 ("burst", 3 if allow else 0), ("resize", 1)]
        w = np.array([k[1] for k in kinds], np.float64)
        kind = kinds[int(rng.choice(len(kinds), p=w / w.sum()))][0]
        if kind == "burst":
            for _ in range(int(rng.integers(1, 6))):
                if not flagged():
                    break
        else:
            dict(mark=mark, unmark=unmark, update=update, update_marked=update_marked, append=append, resize=resize)[kind]()
    end_random = len(ops)
    half = start + n_random // 2
    inside = next(i + 1 for i in range(half, end_random) if marks_after[i] > 0)
    checkpoints = [inside, end_random]
    if cleanup:
        while marked:
            unmark()
        while st["n_marked"] > 0:
            flagged()
        checkpoints.append(len(ops))
    return np.array(ops, np.uint64).reshape(-1, 4), checkpoints


def coverage(ops, facts, n0, cap0):
    """The coverage counts of a sequence from the reference's own account of it (facts: FACTS per operation)."""
    c = dict.fromkeys(NEED, 0)
    count, cap, old_cap = n0, cap0, None
    for (kind, arg, flag, _), f in zip(ops.tolist(), facts.tolist()):
        f = dict(zip(FACTS, f))
        if kind == ADD and f["count"] == count and not f["reused"]:
            c["n_updates"] += 1
            c["updated_ep"] += f["id"] == f["ep_before"]
            c["updated_upper"] += f["level"] > 0
        if kind == ADD and f["count"] > count and old_cap is not None and f["id"] >= old_cap:
            c["grow_then_append"] += 1
            old_cap = None
        c["n_unmarks"] += kind == UNMARK
        c["n_reused"] += f["reused"]
        c["n_flag_appended"] += kind == ADD and flag and not f["reused"]
        c["marked_ep"] += kind == MARK and f["id"] == f["ep_before"]
        if kind == RESIZE:
            c["exact_resize"] += arg == count
            old_cap = cap if arg > cap else None
        count, cap = f["count"], f["capacity"]
    return c


def needed(allow, start_marks):
    """NEED without what a sequence cannot hold: flagged adds need replacement on, and a flagged add only appends once every
    vacancy is refilled, which the hundreds of marks of a `_del` start graph never allow within a sequence."""
    return {k: v for k, v in NEED.items() if (allow or k not in ("n_reused", "n_flag_appended")) and (not start_marks or k != "n_flag_appended")}


def sequences(exe, tmp):
    limit = os.path.getsize(os.path.join(GOLDEN, "dist_ref.npz"))
    ref_hnsw = os.path.join(ROOT, "oracle", "_ref", "ref_hnsw")
    for name, start, allow, seed0, n_random, w_append in SEQS:
        extra = {}
        if isinstance(start, str):
            src = os.path.join(GOLDEN, f"{start}.hnsw.bin")
            g = np.load(os.path.join(GOLDEN, f"{start.replace('_del', '')}.npz"))
            base, queries, dim = g["base"], np.ascontiguousarray(g["queries"], np.float32), g["base"].shape[1]
            integer = "_int_" in start
        else:
            n, dim, M, efc, _ = start
            b8, q8 = seq_base(start)
            base, queries, integer = b8.astype(np.float32), q8.astype(np.float32), True
            fb, src = os.path.join(tmp, "b.fvecs"), os.path.join(tmp, f"{name}.start.bin")
            write_fvecs(fb, base)
            subprocess.check_call([ref_hnsw, "build", "l2", fb, src, str(M), str(efc), "4", "100"])
            extra = {"base": b8, "queries": q8, "M": np.array(M), "efC": np.array(efc)}
        raw = open(src, "rb").read()
        n0 = graph_facts(raw)[0]
        # T starts at tile stride 16: no level-0 list above 16 ids (with M = 16 and rows like these, 24 points already give 17 - 21)
        assert name != "T" or max_degree0(raw) <= 16
        start_marks = int(file_marks(raw)[1].sum())
        cap0 = 400 if name == "T" else n0 + 8
        for seed in range(seed0 * 1000, seed0 * 1000 + 200):
            rng = np.random.default_rng(seed)
            ops, checkpoints = gen_sequence(rng, raw, cap0, allow, n_random, w_append, cleanup=start_marks == 0)
            rows = new_rows(rng, base, int((ops[:, 0] == ADD).sum()), integer)
            steps = os.path.join(tmp, f"steps_{name}")
            os.makedirs(steps, exist_ok=True)
            f = {k: os.path.join(tmp, k) for k in ("ops", "rows", "out", "q", "res")}
            ops.tofile(f["ops"]); rows.tofile(f["rows"]); queries.tofile(f["q"])
            subprocess.check_call([exe, "l2", str(dim), src, str(cap0), str(allow), f["ops"], f["rows"], f["out"], f["q"], str(len(queries)),
                                   f["res"], str(K), *map(str, EFS), "--", steps, *map(str, checkpoints)], stdout=subprocess.DEVNULL)
            facts = np.fromfile(os.path.join(steps, "facts.u32"), np.uint32).reshape(-1, len(FACTS))
            cov = coverage(ops, facts, n0, cap0)
            need = needed(allow, start_marks)
            # (a sequence with a clean-up phase ends its random phase with marks, so that the phase has something to do)
            if all(cov[k] >= v for k, v in need.items()) and (len(checkpoints) < 3 or checkpoints[2] > checkpoints[1]):
                break
            print(f"{name}: seed {seed} misses", {k: cov[k] for k, v in need.items() if cov[k] < v})
        else:
            raise SystemExit(f"{name}: no seed meets the coverage conditions")
        assert len(facts) == len(ops) and facts[checkpoints[0] - 1, 5] > 0 and (len(checkpoints) < 3 or facts[-1, 5] == 0)
        digest = np.array([np.frombuffer(hashlib.sha256(open(os.path.join(steps, f"op{i}.bin"), "rb").read()).digest(), np.uint8)
                           for i in range(len(ops))])
        assert digest[-1].tobytes() == hashlib.sha256(open(f["out"], "rb").read()).digest()
        out = {"ops": ops, "rows": rows.astype(np.uint8) if extra else rows, "max_elements": np.array(cap0), "allow": np.array(allow),
               "seed": np.array(seed), "start_digest": np.frombuffer(hashlib.sha256(raw).digest(), np.uint8), "digest": digest,
               "checkpoints": np.array(checkpoints), "facts": facts, "k": np.array(K), "efs": np.array(EFS), **extra}
        if extra:
            assert np.array_equal(out["rows"].astype(np.float32), rows)
        out.update({f"cov_{k}": np.array(v) for k, v in cov.items()})
        for c in checkpoints:
            for ef, r in read_ref_search(os.path.join(steps, f"res{c}.bin")).items():
                for key, v in r.items():
                    out[f"cp{c}_ef{ef}_{key}"] = v
        dst = os.path.join(GOLDEN, f"updates_seq_{name}.npz")
        np.savez_compressed(dst, **out)
        assert os.path.getsize(dst) <= limit, f"{dst} is larger than dist_ref.npz"
        print(dst, os.path.getsize(dst), "bytes; seed", seed, "ops", len(ops), "checkpoints", checkpoints, cov)
        for fn in os.listdir(steps):
            os.remove(os.path.join(steps, fn))

def compile_driver(tmp):
    exe = os.path.join(tmp, "ref_updates")
    subprocess.check_call([os.environ.get("CXX", "g++"), *REF_FLAGS, "-I" + os.path.join(REF, "third_party", "hnswlib"),
                           os.path.join(GOLDEN, "ref_updates.cpp"), "-o", exe])
    return exe


def scenarios(exe, tmp):
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


def main():
    only = set(sys.argv[1:])    # `make_golden_updates.py seq`: the random sequences alone; `scenarios`: the three hand-written ones
    with tempfile.TemporaryDirectory() as tmp:
        exe = compile_driver(tmp)
        if not only or "scenarios" in only:
            scenarios(exe, tmp)
        if not only or "seq" in only:
            sequences(exe, tmp)


if __name__ == "__main__":
    main()
