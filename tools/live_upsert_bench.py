#!/usr/bin/env python3
"""live_upsert_bench.py -- upsert, replace_deleted and resizeIndex on a resident vanilla index (hs_index_upsert_points,
hs_index_resize) on the bench's rows: 1M x 128 (the cached data of bench.py when it is there, the same generator otherwise), the
vanilla graph built here with `--threads` threads (M = 16, efC = 200).  ONE process, wall-clock time around each call (every
call synchronises the device), `--rounds` alternated rounds; every timed call starts from a fresh load of the same file.

  (a) `--count` updates of existing labels in one call, and `--count` marks followed by `--count` replacements
      (addPoint(.., replace_deleted = true) of new labels) in one call, each against hs_index_add_points of `--count` new rows,
      serial (threads = 1, as an upsert is) -- the call the code before this change offers, which shares the fixed repack of the
      structure arrays: the ratio is what an update costs over an add.
  (b) hs_index_resize n -> 1.1 n against the only route the code before this change offers: hs_index_free + hs_index_load of
      the file with the larger max_elements.
Output: the log on stdout.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from bench import index_cache_dir  # noqa: E402
from hsutil import headline_data, load_product  # noqa: E402

D = 128


def log(*a):
    print(*a, flush=True)


def clock(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--count", type=int, default=1000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--index-dir", default="", help="index files of bench.py --index-dir instead of the user cache directory")
    args = ap.parse_args()
    import torch
    torch.cuda.init()   # (torch's bundled HIP runtime opens the device before the product's does, as in bench.py)
    hs = load_product()
    N, C = args.n, args.count
    idir = args.index_dir or index_cache_dir(N, D, 1)
    if os.path.exists(os.path.join(idir, "ready")) and os.path.exists(os.path.join(idir, "base.npy")):
        base = np.load(os.path.join(idir, "base.npy"))
    else:
        base = headline_data(N, D, 123)
    rng = np.random.default_rng(77)
    lo, hi = float(base.min()), float(base.max())
    pick = rng.permutation(N)[:C]
    new_rows = np.clip(base[rng.integers(0, N, C)] + rng.integers(-2, 3, (C, D)), lo, hi).astype(np.float32)
    new_labels = np.arange(N, N + C, dtype=np.uint64)
    cap = N + C + 8
    with tempfile.TemporaryDirectory() as tmp:
        full = os.path.join(tmp, "full.bin")
        t_build = clock(lambda: hs.build_hnsw(base, full, M=16, ef_construction=200, branching_factor="4", seed=100, threads=args.threads))
        log(f"graph: {N} rows built with {args.threads} threads in {t_build / 1e3:.1f} s")
        res = dict(add=[], update=[], mark=[], replace=[], resize=[], reload=[])
        for rnd in range(args.rounds):
            ix = hs.Index(full, hs.HS_KIND_HNSW, D, max_elements=cap)
            res["add"].append(clock(lambda: ix.add_points(new_rows, new_labels, threads=1)))
            del ix
            ix = hs.Index(full, hs.HS_KIND_HNSW, D, max_elements=cap)
            res["update"].append(clock(lambda: ix.upsert_points(new_rows, pick)))
            assert ix.info()["n"] == N and ix.get_row(int(pick[-1])).tobytes() == new_rows[-1].tobytes()
            del ix
            ix = hs.Index(full, hs.HS_KIND_HNSW, D, max_elements=cap)
            ix.set_replace_deleted(True)
            res["mark"].append(clock(lambda: ix.mark_deleted(pick)))
            res["replace"].append(clock(lambda: ix.upsert_points(new_rows, new_labels, True)))
            assert ix.info()["n"] == N and ix.deleted_count() == 0 and ix.info()["has_deleted"] == 0
            del ix
            log(f"round {rnd}: add {C} new rows (serial) {res['add'][-1]:.1f} ms | {C} updates {res['update'][-1]:.1f} ms | {C} marks {res['mark'][-1]:.2f} ms"
                f" + {C} replacements {res['replace'][-1]:.1f} ms")
            ix = hs.Index(full, hs.HS_KIND_HNSW, D, max_elements=N + 1)
            bytes0 = ix.info()["device_bytes"]
            res["resize"].append(clock(lambda: ix.resize(N + N // 10)))
            assert ix.capacity() == N + N // 10 and ix.info()["device_bytes"] == bytes0
            holder = {}

            def reload():
                holder["ix"] = None     # hs_index_free of the only reference
                holder["ix"] = hs.Index(full, hs.HS_KIND_HNSW, D, max_elements=N + N // 10)

            holder["ix"] = ix
            del ix
            res["reload"].append(clock(reload))
            del holder
            log(f"round {rnd}: hs_index_resize {N} -> {N + N // 10}: {res['resize'][-1]:.1f} ms | hs_index_free + hs_index_load with that max_elements: {res['reload'][-1]:.1f} ms")
        med = {k: float(np.median(v)) for k, v in res.items()}
        spread = {k: (max(v) - min(v)) / np.median(v) * 100 for k, v in res.items()}
        log(f"(a) {C} updates in one call {med['update']:.1f} ms (spread {spread['update']:.1f} %) = x{med['update'] / med['add']:.2f} of hs_index_add_points of {C} new rows, "
            f"serial, {med['add']:.1f} ms (spread {spread['add']:.1f} %)")
        log(f"(a) {C} marks {med['mark']:.2f} ms + {C} replacements in one call {med['replace']:.1f} ms (spread {spread['replace']:.1f} %) = x{med['replace'] / med['add']:.2f} of the same add")
        log(f"(b) hs_index_resize {med['resize']:.1f} ms (spread {spread['resize']:.1f} %) against free + load {med['reload']:.1f} ms (spread {spread['reload']:.1f} %): x{med['reload'] / med['resize']:.1f}")
        log("RESULT " + json.dumps(dict(n=N, count=C, threads=args.threads, **res)))
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)
