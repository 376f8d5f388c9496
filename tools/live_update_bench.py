#!/usr/bin/env python3
"""live_update_bench.py -- live updates of a resident vanilla index (hs_index_add_points, hs_index_mark_deleted) on the bench's
rows: the cached 1M x 128 data of bench.py, the vanilla graph built here with `--threads` threads (M = 16, efC = 200).  ONE
process, wall-clock time around each call (every call synchronises the device), `--rounds` alternated rounds.

  (a) the last `--add` rows added to the index of the others: in one call, and in 10 calls of a tenth each.  Baseline -- what the
      code before this change must do for the same resident result: hs_build_hnsw of all rows + hs_index_load, timed once.
  (b) `--add` marks in one call (and their removal).
  (c) a 10 000-query launch (hs_search_batch_dev, HS_MODE_PQ, the bench's ef) on the full index loaded WITH room against the same
      file loaded WITHOUT room, alternated; the first must lie inside the spread of the second's rounds.
  (d) the per-call fixed cost (host repack of the structure arrays + their upload): a call that adds ONE row.
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
from bench import prepare_cached  # noqa: E402
from hsutil import headline_data, load_product  # noqa: E402

D, NQ, K = 128, 10_000, 10


def log(*a):
    print(*a, flush=True)


def clock(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--add", type=int, default=1000)
    ap.add_argument("--ef", type=int, default=70)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--index-dir", default="", help="index files of bench.py --index-dir instead of the user cache directory")
    args = ap.parse_args()
    import torch
    torch.cuda.init()   # (torch's bundled HIP runtime opens the device before the product's does, as in bench.py)
    hs = load_product()
    dev = torch.device("cuda", 0)
    N, A = args.n, args.add
    if N == 1_000_000:
        idir = args.index_dir or prepare_cached(N, D, 1, hs)[0]
        base = np.load(os.path.join(idir, "base.npy"))
    else:
        base = headline_data(N, D, 123)
    q = headline_data(NQ, D, 456)
    n0 = N - A
    with tempfile.TemporaryDirectory() as tmp:
        part, full = os.path.join(tmp, "part.bin"), os.path.join(tmp, "full.bin")
        t_part = clock(lambda: hs.build_hnsw(base[:n0], part, M=16, ef_construction=200, branching_factor="4", seed=100, threads=args.threads))
        log(f"prefix graph: {n0} rows built with {args.threads} threads in {t_part / 1e3:.1f} s")
        # ---- baseline: full build + load, once -------------------------------------------------------------------------------
        t_build = clock(lambda: hs.build_hnsw(base, full, M=16, ef_construction=200, branching_factor="4", seed=100, threads=args.threads))
        holder = {}
        t_load = clock(lambda: holder.setdefault("ix", hs.Index(full, hs.HS_KIND_HNSW, D)))
        log(f"(a) baseline: hs_build_hnsw of {N} rows ({args.threads} threads) {t_build / 1e3:.1f} s + hs_index_load {t_load / 1e3:.1f} s = {(t_build + t_load) / 1e3:.1f} s")
        tight = holder.pop("ix")
        # ---- (a) adds, (d) fixed cost -----------------------------------------------------------------------------------------
        one, ten, fixed = [], [], []
        labels = np.arange(n0, N, dtype=np.uint64)
        for rnd in range(args.rounds):
            for how in ("one", "ten"):
                ix = hs.Index(part, hs.HS_KIND_HNSW, D, max_elements=N + 8)
                ix.seed_levels(100, n0)
                if how == "one":
                    ms = clock(lambda: ix.add_points(base[n0:], labels, threads=args.threads))
                    one.append(ms)
                    fixed.append(clock(lambda: ix.add_points(base[:1] + 1, [N + 1], threads=1)))
                else:
                    step = A // 10
                    per = [clock(lambda a=a: ix.add_points(base[a:a + step], np.arange(a, a + step), threads=args.threads)) for a in range(n0, N, step)]
                    ms = sum(per)
                    ten.append(ms)
                log(f"round {rnd} add {A} rows in {'one call' if how == 'one' else '10 calls'}: {ms:.1f} ms" + (f"; a call that adds one row: {fixed[-1]:.1f} ms" if how == "one" else f" ({', '.join(f'{x:.0f}' for x in per)})"))
                del ix
        log(f"(a) {A} rows in one call {np.median(one):.1f} ms; in 10 calls {np.median(ten):.1f} ms; baseline {(t_build + t_load):.0f} ms -> x{(t_build + t_load) / np.median(one):.0f} / x{(t_build + t_load) / np.median(ten):.0f}")
        log(f"(d) per-call fixed cost (repack of CSR / up_base / up_ptr / uptile from the host image + upload_small; one insertion included): {np.median(fixed):.1f} ms at n = {N}")
        # ---- (b) marks, (c) search with and without room ----------------------------------------------------------------------
        roomy = hs.Index(full, hs.HS_KIND_HNSW, D, max_elements=N + A)
        marks = np.arange(3, 3 + 7 * A, 7, dtype=np.uint64)
        mk, un = [], []
        for rnd in range(args.rounds):
            mk.append(clock(lambda: roomy.mark_deleted(marks)))
            un.append(clock(lambda: roomy.mark_deleted(marks, on=False)))
        log(f"(b) {A} marks in one call: {np.median(mk):.2f} ms ({', '.join(f'{x:.2f}' for x in mk)}; the first call builds the label map); removing them: {np.median(un):.2f} ms")
        dq = torch.from_numpy(q).to(dev)
        ol = torch.zeros((NQ, K), dtype=torch.int64, device=dev)
        od = torch.zeros((NQ, K), dtype=torch.float32, device=dev)
        oc = torch.zeros(NQ, dtype=torch.int32, device=dev)
        L = hs.lib()

        def launch(ix):
            hs._check(L.hs_search_batch_dev(ix._h, dq.data_ptr(), NQ, K, hs.HS_MODE_PQ, None, ol.data_ptr(), od.data_ptr(), oc.data_ptr(), None, None))

        def timed(ix):
            ts = []
            for _ in range(args.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                launch(ix)
                e1.record()
                e1.synchronize()
                ts.append(e0.elapsed_time(e1))
            ix.check()
            return float(np.median(ts))

        res = {}
        for ix in (tight, roomy):
            ix.set_ef(args.ef)
            launch(ix); torch.cuda.synchronize(); ix.check()
            res[id(ix)] = (ol.cpu().numpy().tobytes(), od.cpu().numpy().tobytes())
        assert res[id(tight)] == res[id(roomy)], "the index loaded with room answers differently"
        rows = dict(tight=[], roomy=[])
        for rnd in range(args.rounds):
            for name, ix in (("tight", tight), ("roomy", roomy)):
                rows[name].append(timed(ix))
                log(f"round {rnd} {name}: {rows[name][-1]:.3f} ms per {NQ}-query launch ({ix.last_kernel()}, ef {args.ef}, median of {args.reps})")
        t, r = rows["tight"], rows["roomy"]
        spread = (max(t) - min(t)) / np.median(t) * 100
        delta = (np.median(r) / np.median(t) - 1) * 100
        log(f"(c) loaded without room {np.median(t):.3f} ms | with room {np.median(r):.3f} ms | {delta:+.2f} % | spread of the former's rounds {spread:.2f} % -> "
            + ("inside the spread" if abs(delta) <= spread else "OUTSIDE the spread"))
        log("RESULT " + json.dumps(dict(n=N, add=A, threads=args.threads, baseline_ms=t_build + t_load, one_call_ms=one, ten_calls_ms=ten, fixed_ms=fixed,
                                        mark_ms=mk, unmark_ms=un, search_ms=rows)))
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)
