"""The shapes at which the batched addPoint is held against tests/batch_build_restated.py, shared by
tests/test_batch_build_restated_cpu.py (the host twin) and tests/test_gpu_batch_build_restated.py (the device), and the premises of
the value-range families of tests/value_range.py as a BUILD meets them (on the rows' own distance table).  Integer-valued rows,
2000 at most: the reading's distances are exact and one call of it takes seconds."""
import numpy as np

import batch_build_restated as R
import value_range as vr
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
    """Two-dimensional rows on a side x side integer grid: n rows on side^2 points, so most rows have copies and most candidate
    pairs tie."""
    return np.random.default_rng(seed).integers(0, side, (n, 2)).astype(np.float32)


MANY_N, MANY_FROM = 2000, 1100


def many_targets_rows(levels, grow_div=0, batch_max=0):
    """The construction of test_a_batch_into_the_same_few_targets at 2000 rows: a spread-out prefix that ends where the first batch
    at or after row 1100 begins (more than 64 rows: 1100 / 16 = 68), then integer noise in [-2, 2] round row 7.  Every row of that
    batch finds row 7 nearest among the rows before it, so row 7's level-0 list takes the whole batch."""
    sched = R.schedule([int(x) for x in levels], grow_div=grow_div, batch_max=batch_max)
    begin, size = next((b, s) for b, s, _, _ in sched if b >= MANY_FROM)
    assert size > 64 and begin + size <= MANY_N
    spread = int_mixture(begin, 16, 6)
    noise = np.random.default_rng(5).integers(-2, 3, (MANY_N - begin, 16))
    return np.ascontiguousarray(np.concatenate([spread, spread[7] + noise]), np.float32), begin


# name -> (rows, metric, M, ef_construction, schedule and label keywords).  "many_targets" needs the levels: see rows_of.
CASES = {
    "default": (lambda: int_mixture(1500), L2, 8, 100, {}),
    "small_batches": (lambda: int_mixture(1200), L2, 4, 40, dict(batch_max=64, grow_div=1)),
    "both_caps": (lambda: int_mixture(700), L2, 31, 512, {}),            # kBgMaxM, kBgMaxEfc
    "efc_below_M": (lambda: int_mixture(800), L2, 8, 4, {}),             # the constructor raises ef_construction to M
    "default_ip": (lambda: int_mixture(1500), IP, 8, 100, {}),
    "small_batches_ip": (lambda: int_mixture(1200), IP, 4, 40, dict(batch_max=64, grow_div=1)),
    "both_caps_ip": (lambda: int_mixture(700), IP, 31, 512, {}),
    "efc_below_M_ip": (lambda: int_mixture(800), IP, 8, 4, {}),
    "ip_both_signs": (lambda: signed_rows(1500), IP, 8, 100, {}),
    "smallest_M": (lambda: int_mixture(600), L2, 2, 10, {}),
    "grow_div_4": (lambda: int_mixture(1000), L2, 8, 60, dict(grow_div=4)),
    "labels": (lambda: int_mixture(500), L2, 8, 40, dict(labels=(np.arange(500, dtype=np.uint64) * 7 + 3)[::-1].copy())),
    "n1": (lambda: int_mixture(1, 16, 3), L2, 4, 20, {}),
    "n2": (lambda: int_mixture(2, 16, 3), L2, 4, 20, {}),
    "n3": (lambda: int_mixture(3, 16, 3), L2, 4, 20, {}),
    "n9": (lambda: int_mixture(9, 16, 3), L2, 4, 20, {}),               # maxM0 + 1
    "n65": (lambda: int_mixture(65, 16, 3), L2, 4, 20, {}),
    "same_row": (lambda: np.tile(int_mixture(1, 16, 4), (300, 1)), L2, 4, 20, {}),
    "many_targets": (None, L2, 4, 40, {}),
    "grid": (grid_rows, L2, 6, 50, {}),
}
TIE_HEAVY = ("same_row", "grid", "many_targets")
GPU_CASES = ("default", "small_batches", "both_caps", "efc_below_M", "smallest_M", "ip_both_signs", "many_targets", "grid")


def read(p):
    with open(p, "rb") as f:
        return f.read()


def serial_levels(hs, folder, rows, metric, M, efc, labels=None):
    """The levels of the file hs.build_hnsw(threads=1) writes for these rows, M and seed: the compiled reference pins that builder."""
    p = str(folder / "serial.bin")
    hs.build_hnsw(rows, p, metric=metric, M=M, ef_construction=efc, branching_factor="4", seed=SEED, threads=1, labels=labels)
    return R.levels_of(read(p))


def rows_of(hs, folder, name):
    """(rows, levels) of a case; the rows are inside the reading's exact range."""
    make, metric, M, efc, kw = CASES[name]
    if name == "many_targets":
        rows, _ = many_targets_rows(serial_levels(hs, folder, int_mixture(MANY_N, 16, 6), metric, M, efc))   # (levels hang on no row)
    else:
        rows = make()
    rows = np.ascontiguousarray(rows, np.float32)
    assert len(rows) <= 2000 and R.exact_range(rows, metric) < R.EXACT
    return rows, serial_levels(hs, folder, rows, metric, M, efc, kw.get("labels"))


_reading = {}


def reading(hs, folder, name):
    """(rows, levels, the reading's file, its stats) of a case, computed once per process and never changed."""
    if name not in _reading:
        _, metric, M, efc, kw = CASES[name]
        rows, levels = rows_of(hs, folder, name)
        raw, st = R.build(rows, levels, metric, M, efc, **kw)
        print(f"{name}: {st}")
        if name in TIE_HEAVY:
            assert st["ties"] > 1000, f"{name}: the heaps compared equal keys {st['ties']} times"
        if name == "many_targets":
            assert st["max_incoming"] > 64, "no list received more ids than a wavefront has lanes within one batch"
        _reading[name] = (rows, levels, raw, st)
    return _reading[name]


def resume_cuts(levels, sched):
    """Prefix lengths for the continued build (4n): a batch boundary in the middle of the schedule; a row strictly inside a later
    batch; three rows before the last row that raises the top level, so that the add raises it."""
    begins = [b for b, _, _, _ in sched]
    boundary = begins[len(begins) // 2]
    b, s = next((b, s) for b, s, _, _ in sched if b > boundary and s >= 8)
    raiser = max(r for r in range(100, len(levels)) if levels[r] > max(levels[:r]))
    cuts = dict(boundary=boundary, inside=b + s // 2, raises=raiser - 3)
    assert cuts["boundary"] in begins and cuts["inside"] not in begins and max(levels[cuts["raises"]:]) > max(levels[:cuts["raises"]])
    return cuts


# ---- value-range families as a build meets them ------------------------------------------------------------------------------------
VR_N, VR_M, VR_EFC = 600, 8, 60


def vr_cases():
    """(family, metric, dim, exponent): the graph-kernel cases of value_range.py and l2_overflow at its own dim."""
    return vr.cases() + [("l2_overflow", L2, vr.OVERFLOW_DIM, vr.OVERFLOW_EXP)]


def vr_name(case):
    return vr.case_name(case)


def vr_rows(case, n=VR_N):
    """The family's rows through value_range's own base_draw and scaled (the rows rows_and_queries gives, n of them)."""
    _, _, d, s = case
    return vr.scaled(vr.base_draw(n, d, vr.SEEDS[0] + d), s)


_premise_met = set()


def vr_check_premise(oracle, case, rows):
    """The family's premise on the table of every distance a build of these rows can compute (Oracle.dist, as dist_table)."""
    family, metric, _, _ = case
    if (vr_name(case), len(rows)) in _premise_met:
        return
    t = vr.dist_table(oracle, metric, rows, rows)
    off = t[~np.eye(len(rows), dtype=bool)]
    what = vr_name(case)
    assert not np.isnan(t).any(), f"{what}: NaN"
    if family == "l2_overflow":
        inf = np.isposinf(t)
        assert inf.any() and not np.isneginf(t).any(), f"{what}: no +inf distance"
        assert (inf.sum(1) > 0).all() and ((~inf).sum(1) > vr.M).all(), f"{what}: a row without infinite, or with too few finite, distances"
        _premise_met.add((what, len(rows)))
        return
    assert np.isfinite(t).all(), f"{what}: a non-finite distance"
    if family == "large":
        assert (np.abs(t).max(1) > np.float32(2.0 ** 100)).all(), f"{what}: a row whose distances stay below 2^100"
    elif family == "l2_subnormal":
        assert (off >= 0).all() and (off[off != 0] < vr.SUBNORMAL).all() and (off != 0).any(), f"{what}: a nonzero distance is a normal float"
    elif family == "ip_ones":
        assert (t.view(np.uint32) == np.float32(1.0).view(np.uint32)).all(), f"{what}: a distance that is not exactly 1.0f"
    elif family == "ip_cross":
        both = ((t < 0).any(1) & (t > 0).any(1))
        assert 2 * both.sum() >= len(rows), f"{what}: fewer than half of the rows see both signs"
    _premise_met.add((what, len(rows)))
