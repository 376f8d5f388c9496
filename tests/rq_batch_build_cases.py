"""The shapes at which the batched build of HNSW-SlimQ's base graph is held against tests/rq_batch_build_restated.py,
shared by tests/test_rq_batch_build_cpu.py (the host twin) and tests/test_gpu_rq_batch_build.py (the device).  Integer-valued rows,
2000 at most: the reading's distances are exact and one call of it takes seconds.  The levels of every case come from the serial
builder's file (hs.build_rabitq_hnsw(threads=1), which the compiled rabitqlib pins), never from the file under test."""
import numpy as np

import rq_batch_build_restated as R
from hsutil import mixture

L2, IP = 0, 1
SEED = 100


def int_mixture(n, d=16, seed=11):
    return mixture(n, d, seed, integer=True)


def signed_rows(n, d=16, seed=11):
    """Integer rows in [-40, 40]: 1 - <a, b> takes both signs."""
    x = np.clip(np.rint(mixture(n, d, seed, lo=-30.0, hi=30.0, sigma=8.0)), -40, 40).astype(np.float32)
    assert x.min() < -20 and x.max() > 20
    return x


def grid_rows(n=1000, side=12, seed=21):
    """Two-dimensional rows on a side x side integer grid: n rows on side^2 points, so most rows have copies and most pairs tie."""
    return np.random.default_rng(seed).integers(0, side, (n, 2)).astype(np.float32)


def hub_rows(n=400, d=16, a=3, seed=31):
    """Row 0 at the origin, the others distinct points with two coordinates of +-a: each is 2 a^2 from the origin and at least
    that far from every other, so nothing the heuristic keeps occludes anything and the origin's level-0 list fills to 2 M and is
    then pruned with 2 M + 1 candidates."""
    pts = [(i, j, si, sj) for i in range(d) for j in range(i + 1, d) for si in (-a, a) for sj in (-a, a)]
    assert len(pts) >= n - 1
    x = np.zeros((n, d), np.float32)
    for r, k in enumerate(np.random.default_rng(seed).permutation(len(pts))[:n - 1]):
        i, j, si, sj = pts[k]
        x[r + 1, i], x[r + 1, j] = si, sj
    return x


MANY_N, MANY_FROM = 2000, 1100


def many_targets_rows(levels):
    """A batch that sends more than 64 ids into one list: a spread-out prefix that ends where the first batch at or after row 1100
    begins (more than 64 rows: 1100 / 16 = 68), then integer noise in [-2, 2] round row 7.  Every row of that batch finds row 7
    nearest among the rows before it, so row 7's level-0 list takes the whole batch."""
    sched = R.schedule([int(x) for x in levels])
    begin, size = next((b, s) for b, s, _, _ in sched if b >= MANY_FROM)
    assert size > 64 and begin + size <= MANY_N
    spread = int_mixture(begin, 16, 6)
    noise = np.random.default_rng(5).integers(-2, 3, (MANY_N - begin, 16))
    return np.ascontiguousarray(np.concatenate([spread, spread[7] + noise]), np.float32)


# name -> (rows, metric, M, ef_construction, schedule keywords).  "many_targets" needs the levels: see rows_of.
CASES = {
    "default": (lambda: int_mixture(1500), L2, 8, 40, {}),
    "small_batches": (lambda: int_mixture(1200), L2, 4, 40, dict(batch_max=64, grow_div=1)),
    "m32": (hub_rows, L2, 32, 128, {}),                                  # the reference's own M and ef_construction; n 400, d 16
    "efc_below_M": (lambda: int_mixture(800), L2, 8, 4, {}),             # the constructor raises ef_construction to M
    "smallest_M": (lambda: int_mixture(600), L2, 2, 10, {}),
    "ip_both_signs": (lambda: signed_rows(1200), IP, 8, 60, {}),
    "n1": (lambda: int_mixture(1, 16, 3), L2, 4, 20, {}),
    "n2": (lambda: int_mixture(2, 16, 3), L2, 4, 20, {}),
    "n3": (lambda: int_mixture(3, 16, 3), L2, 4, 20, {}),
    "n65": (lambda: int_mixture(65, 16, 3), L2, 4, 20, {}),
    "same_row": (lambda: np.tile(int_mixture(1, 16, 4), (300, 1)), L2, 4, 20, {}),
    "grid": (lambda: grid_rows(144 * 5), L2, 6, 50, {}),
    "grid_tight": (lambda: grid_rows(144 * 5), L2, 6, 6, {}),            # ef_construction = M: what the full result heap evicts among equals is kept or lost
    "many_targets": (None, L2, 4, 40, {}),
}
GPU_CASES = ("default", "small_batches", "m32", "efc_below_M", "smallest_M", "ip_both_signs", "n1", "n2", "n3", "n65", "same_row", "grid",
             "grid_tight", "many_targets")


def read(p):
    with open(p, "rb") as f:
        return f.read()


def serial_levels(hs, folder, rows, metric, M, efc):
    p = str(folder / "serial.bin")
    hs.build_rabitq_hnsw(rows, p, metric=metric, M=M, ef_construction=efc, seed=SEED, threads=1)
    return R.levels_of(read(p))


def rows_of(hs, folder, name):
    """(rows, levels) of a case; the rows are inside the reading's exact range."""
    make, metric, M, efc, _ = CASES[name]
    if name == "many_targets":
        rows = many_targets_rows(serial_levels(hs, folder, int_mixture(MANY_N, 16, 6), metric, M, efc))   # (levels hang on no row)
    else:
        rows = make()
    rows = np.ascontiguousarray(rows, np.float32)
    assert len(rows) <= 2000 and R.exact_range(rows, metric) < R.EXACT
    return rows, serial_levels(hs, folder, rows, metric, M, efc)


_reading = {}


def reading(hs, folder, name):
    """(rows, levels, the reading's file, its stats) of a case, computed once per process and never changed."""
    if name not in _reading:
        _, metric, M, efc, kw = CASES[name]
        rows, levels = rows_of(hs, folder, name)
        raw, st = R.build(rows, levels, metric, M, efc, **kw)
        print(f"{name}: {st}")
        if name == "many_targets":
            assert st["max_incoming"] > 64, "no list received more ids than a wavefront has lanes within one batch"
        if name == "m32":
            assert st["full_lists"] == 65, "no full level-0 list of 64 ids took another id"
        assert st["present_hits"] == 0   # a build from nothing cannot reach the present-check: no old list names a new row
        _reading[name] = (rows, levels, raw, st)
    return _reading[name]
