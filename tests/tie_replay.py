"""Data and premise of tests/test_gpu_tie_replay.py and tests/test_tie_replay_cpu.py: a graph on which EVERY query's answer hangs on
the layout of the reference's result heap, so that every kernel that selects must answer it through the boundary replay
(csrc/search_finish.hpp replay_boundary) and say so (stats column 3 == 1).

256 distinct integer rows of d = 16, each stored twice (n = 512): every distance occurs an even number of times, so with k odd the
k-th boundary falls inside a pair.  Built by the serial host builder, so the graph -- and with it whether the premise holds -- is the
same on every machine."""
import os

import numpy as np

L2, IP = 0, 1
METRICS = (("l2", L2), ("ip", IP))
D, N_DISTINCT, NQ, M, EF_CONSTRUCTION = 16, 256, 32, 8, 40
POOL = 300                       # candidate queries drawn; PICK names the 32 that are used
SEED, QSEED, LO, HI = 5, 1, 0, 8   # rows (SEED) and queries (QSEED): integers in [LO, HI)
# (ef, k) per leg.  ef > k: a tie across the k-th boundary; ef == k: nothing is selected, an eviction at the bound decides.
FLAT_PAIRS = [(12, 5), (5, 5)]
FAST_PAIRS = [(12, 5), (5, 5)]
LEAN_PAIRS = [(70, 5)]           # (71, 71) is not a lean shape: lean_supported admits k <= 64 only
STRICT_PAIRS = [(12, 5)]
# The premise is a condition on the data: of the pool's queries these 32 are the ones it holds for on every leg (at ef == k only
# one random query in five ends on an eviction at the bound).  tests/test_tie_replay_cpu.py asserts it for all 32, none exempted.
PICK = [3, 19, 25, 26, 29, 41, 64, 67, 72, 87, 88, 90, 96, 106, 107, 114, 135, 143, 145, 160, 171, 172, 184, 208, 211, 260, 269, 274, 277,
        283, 295, 297]
ALL_PAIRS = sorted(set(FLAT_PAIRS + FAST_PAIRS + LEAN_PAIRS + STRICT_PAIRS))


def rows_and_queries():
    rng = np.random.default_rng(SEED)
    seen, rows = set(), []
    while len(rows) < N_DISTINCT:
        r = rng.integers(LO, HI, D)
        if tuple(r) not in seen:
            seen.add(tuple(r))
            rows.append(r)
    rows = np.array(rows, np.float32)
    base = np.repeat(rows, 2, axis=0)          # row i stored at 2 i and 2 i + 1
    q = np.random.default_rng(QSEED).integers(LO, HI, (POOL, D)).astype(np.float32)[PICK]
    return np.ascontiguousarray(base), np.ascontiguousarray(q)


def build_files(hs, folder):
    """{metric name: dict(metric, hp, sp)}: the vanilla file and its Slim file, per metric."""
    base, q = rows_and_queries()
    files = {}
    for name, metric in METRICS:
        hp, sp = (os.path.join(folder, f"tie_{name}.{x}") for x in ("h.bin", "s.bin"))
        hs.build_hnsw(base, hp, metric=metric, M=M, ef_construction=EF_CONSTRUCTION, threads=1)
        hs.convert_slim(hp, sp, D, metric=metric, threads=4)
        files[name] = dict(name=name, metric=metric, hp=hp, sp=sp)
    return files, base, q


def overloads(f):
    """(kind, path, call) of the three answers a file pair gives: HS_MODE_PQ on both kinds, HS_MODE_SLIM_IDS on the Slim file."""
    return [("slim", f["sp"], "pq"), ("slim", f["sp"], "ids"), ("hnsw", f["hp"], "pq")]


def reference(ox, q, ef, k, call):
    ox.set_ef(ef)
    return ox.search_pq(q, k, threads=4) if call == "pq" else ox.search_ids(q, k, threads=4)


def through_replay(ox, q, ef, k, call, o):
    """Per query, from the oracle alone: must a kernel that selects answer it through the replay?  ef > k: the result array holds
    more than k entries and the distances of ranks k - 1 and k have the same bits.  ef == k: the reference's last eviction from the
    full heap removed an entry whose key equals the new worst kept key (what the kernels watch as `btie`)."""
    if ef == k:
        ox.set_ef(ef)
        return ox.tie_evictions(q, k, call == "pq", threads=4, last=True) == 1
    out = []
    for i, n in enumerate(o["raw_sz"]):
        r = np.sort(o["raw_d"][i, :n]).view(np.uint32)
        out.append(bool(n > k and r[k - 1] == r[k]))
    return np.array(out)
