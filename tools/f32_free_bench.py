#!/usr/bin/env python3
"""f32_free_bench.py -- what dropping the fp32 rows (hs_index_set_f32_resident(ix, 0)) does to the searches that used to read them,
on the bench's own workload: the cached 1M x 128 index and query seeds of bench.py, k = 10, ef = 70, u8 rows.  ONE loaded index in
ONE process, two states alternated B, C, B, C, ... for three rounds after both have been warmed:

  state B  narrow rows beside the resident fp32 rows: the filtered search runs hs::fast_kernel and the exact-order mode
           hs::strict_kernel, both on the fp32 rows -- the behaviour before fp32-free indexes existed, the yardstick;
  state C  fp32 rows dropped: the same calls run hs::fast_kernel_u8 / hs::strict_kernel_u8 on the u8 copy.

Per state and round, each the median of `--reps` host-timed calls on 10 000 queries (wall clock around the whole call, which is
how these host entry points are used; the copies of queries and results are the same in both states):
  (a) search_filtered with a one-third-off mask;
  (b) search_ids in the exact-order mode.
Every call's outputs are compared with state B's first answer, byte for byte.  The spread of state B's own rounds is the noise: a
state-C time inside it or better is "no loss", anything else is the loss it is.  device_bytes of states A (fp32 format), B and C
are on record.  Output: the log on stdout.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from bench import prepare_cached  # noqa: E402
from hsutil import headline_data, load_product  # noqa: E402

N, D, NQ, K = 1_000_000, 128, 10_000, 10


def log(*a):
    print(*a, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ef", type=int, default=70)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--index-dir", default="", help="index files of bench.py --index-dir instead of the user cache directory")
    args = ap.parse_args()
    import torch
    torch.cuda.init()   # (torch's bundled HIP runtime opens the device before the product's does, as in bench.py)
    hs = load_product()
    idir = args.index_dir or prepare_cached(N, D, 1, hs)[0]
    log(f"index: {os.path.basename(idir)}")
    ix = hs.Index(os.path.join(idir, "slim.bin"), hs.HS_KIND_SLIM, D, hs.HS_METRIC_L2)
    ix.set_ef(args.ef)
    q = headline_data(NQ, D, 456)
    allowed = (np.arange(N) % 3 != 0).astype(np.uint8)
    bytes_a = ix.info()["device_bytes"]
    ix.set_row_format(hs.HS_ROWS_U8)
    bytes_b = ix.info()["device_bytes"]

    def state(name):
        ix.set_f32_resident(name == "B")

    def filtered():
        return ix.search_filtered(q, K, allowed, want_stats=True)

    def exact():
        ix.set_exact_order(True)
        try:
            return ix.search_ids(q, K, want_dists=True, want_stats=True)
        finally:
            ix.set_exact_order(False)

    calls = (("filtered", filtered, "hs::fast_kernel"), ("exact order", exact, "hs::strict_kernel"))
    ref = {}
    t0 = time.perf_counter()
    state("C")
    t_drop = time.perf_counter() - t0
    bytes_c = ix.info()["device_bytes"]
    t0 = time.perf_counter()
    state("B")
    t_restore = time.perf_counter() - t0
    log(f"device_bytes: A (fp32 format) {bytes_a / 2**20:.1f} MiB, B (u8 beside fp32) {bytes_b / 2**20:.1f} MiB, C (u8 alone) {bytes_c / 2**20:.1f} MiB; "
        f"drop {t_drop * 1e3:.1f} ms, restore {t_restore * 1e3:.1f} ms")
    for st in ("B", "C"):   # warm both states, fix the reference answer, check the kernels
        state(st)
        for name, fn, kern in calls:
            r = fn()
            assert ix.last_kernel() == kern + ("_u8" if st == "C" else ""), (st, name, ix.last_kernel())
            if st == "B":
                ref[name] = r
            for key in ref[name]:
                assert ref[name][key] is None or ref[name][key].tobytes() == r[key].tobytes(), f"state {st}, {name}: {key} differs from state B's"
            log(f"state {st} {name}: kernel {ix.last_kernel()}, outputs == state B's")
    rows = {st: {name: [] for name, _, _ in calls} for st in ("B", "C")}
    for rnd in range(args.rounds):
        for st in ("B", "C"):
            state(st)
            for name, fn, _ in calls:
                ts = []
                for _ in range(args.reps):
                    t0 = time.perf_counter()
                    r = fn()
                    ts.append((time.perf_counter() - t0) * 1e3)
                    assert ref[name]["labels"].tobytes() == r["labels"].tobytes() and ref[name]["stats"].tobytes() == r["stats"].tobytes()
                rows[st][name].append(float(np.median(ts)))
                log(f"round {rnd} state {st} {name:>11}: {np.median(ts):.3f} ms per {NQ}-query call (median of {args.reps}, min {min(ts):.3f}), kernel {ix.last_kernel()}")
    log("\ncall | state B ms (rounds) | state C ms (rounds) | C vs B (medians) | spread of B's rounds")
    for name, _, _ in calls:
        b, c = rows["B"][name], rows["C"][name]
        spread = (max(b) - min(b)) / np.median(b) * 100
        delta = (np.median(c) / np.median(b) - 1) * 100
        verdict = "no loss" if delta <= spread else f"loss of {delta:.2f} %"
        log(f"{name:>11} | {np.median(b):.3f} ({', '.join(f'{x:.3f}' for x in b)}) | {np.median(c):.3f} ({', '.join(f'{x:.3f}' for x in c)}) | "
            f"{delta:+.2f} % | {spread:.2f} % -> {verdict}")
    log("RESULT " + json.dumps(dict(ef=args.ef, device_bytes=dict(A=bytes_a, B=bytes_b, C=bytes_c), ms=rows)))
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)
