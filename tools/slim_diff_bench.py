#!/usr/bin/env python3
"""slim_diff_bench.py -- the patch server's step on two resident indexes (hs_slim_convert_diff + draining hs_slim_diff_next) on the
bench's rows: 1M x 128 (the cached data of bench.py when it is there, the same generator otherwise), the vanilla graph built here
with `--threads` threads (M = 16, efC = 200), its Slim index converted on the CPU.  ONE process, wall-clock time around each call
(every call synchronises the device), `--rounds` alternated rounds.

A round loads both indexes afresh, adds `--count` rows with hs_index_add_points (serial), then times
  (a) hs_slim_convert_diff + the genPatch drain (hs_slim_diff_next, `--limit` bytes per chunk, rows included), and once more with
      nothing added in between (the second conversion of a round: what the step costs when little has changed);
  (b) the only route the code before this change offers for the same Slim index on the device: hs_index_save of the vanilla index,
      hs_convert_slim_gpu file to file, hs_index_load of the result (which still leaves the diff of two files to the host).
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
    ap.add_argument("--limit", type=int, default=1 << 20)
    ap.add_argument("--index-dir", default="", help="index files of bench.py --index-dir instead of the user cache directory")
    args = ap.parse_args()
    import torch
    torch.cuda.init()   # (torch's bundled HIP runtime opens the device before the product's does, as in bench.py)
    hs = load_product()
    N, C = args.n, args.count
    idir = args.index_dir or index_cache_dir(N, D, 1)
    if os.path.exists(os.path.join(idir, "ready")) and os.path.exists(os.path.join(idir, "base.npy")):
        base = np.load(os.path.join(idir, "base.npy"))[:N]
    else:
        base = headline_data(N, D, 123)
    rng = np.random.default_rng(78)
    lo, hi = float(base.min()), float(base.max())
    new_rows = np.clip(base[rng.integers(0, N, C)] + rng.integers(-2, 3, (C, D)), lo, hi).astype(np.float32)
    new_labels = np.arange(N, N + C, dtype=np.uint64)
    cap = N + C + 8
    with tempfile.TemporaryDirectory() as tmp:
        full, slim = os.path.join(tmp, "full.bin"), os.path.join(tmp, "slim.bin")
        t_build = clock(lambda: hs.build_hnsw(base, full, M=16, ef_construction=200, branching_factor="4", seed=100, threads=args.threads))
        # the starting Slim index: one conversion from an empty one, so that the rounds measure what a batch changes
        t_conv = clock(lambda: hs.slim_convert_diff_files(None, full, slim, D, threads=args.threads).close())
        log(f"graph: {N} rows built with {args.threads} threads in {t_build / 1e3:.1f} s, first Slim conversion on the host {t_conv / 1e3:.1f} s")
        res = dict(diff=[], drain=[], diff_again=[], save=[], convert=[], load=[])
        first = {}
        for rnd in range(args.rounds):
            hx = hs.Index(full, hs.HS_KIND_HNSW, D, max_elements=cap)
            sx = hs.Index(slim, hs.HS_KIND_SLIM, D, max_elements=cap)
            hx.add_points(new_rows, new_labels, threads=1)
            holder = {}
            res["diff"].append(clock(lambda: holder.update(d=sx.convert_diff(hx, threads=args.threads))))
            d = holder["d"]
            sizes = []

            def drain():
                while True:
                    b, _, _, fin = d.next(args.limit, True, cap=2 * args.limit + (1 << 16))
                    sizes.append(len(b))
                    if fin:
                        return

            res["drain"].append(clock(drain))
            info = d.info()
            res["diff_again"].append(clock(lambda: holder.update(d2=sx.convert_diff(hx, threads=args.threads))))
            info2 = holder["d2"].info()
            if rnd == 0:
                first = dict(used_gpu=d.used_gpu, kernel_ms=d.kernel_ms, n_old=info["n_old"], n_new=info["n_new"], n_reprune=info["n_reprune"],
                             chunks=len(sizes), stream_bytes=int(sum(sizes)), again_kernel_ms=holder["d2"].kernel_ms,
                             again_n_old=info2["n_old"], again_n_new=info2["n_new"])
            assert d.used_gpu and info["n_new"] == C and info2["n_old"] == 0 and info2["n_new"] == 0
            saved, conv = os.path.join(tmp, "saved.bin"), os.path.join(tmp, "conv.bin")
            res["save"].append(clock(lambda: hx.save(saved)))
            res["convert"].append(clock(lambda: hs.convert_slim_gpu(saved, conv, D, threads=args.threads)))
            res["load"].append(clock(lambda: holder.update(w=hs.Index(conv, hs.HS_KIND_SLIM, D, max_elements=cap))))
            del holder, d, hx, sx
            log(f"round {rnd}: convert_diff {res['diff'][-1]:.1f} ms + drain {res['drain'][-1]:.1f} ms | again, nothing changed {res['diff_again'][-1]:.1f} ms"
                f" | save {res['save'][-1]:.1f} + convert_slim_gpu {res['convert'][-1]:.1f} + load {res['load'][-1]:.1f} ms")
        med = {k: float(np.median(v)) for k, v in res.items()}
        spread = {k: (max(v) - min(v)) / np.median(v) * 100 for k, v in res.items()}
        log(f"first round: {json.dumps(first)}")
        a, b = med["diff"] + med["drain"], med["save"] + med["convert"] + med["load"]
        log(f"(a) hs_slim_convert_diff {med['diff']:.1f} ms (spread {spread['diff']:.1f} %) + drain {med['drain']:.1f} ms (spread {spread['drain']:.1f} %) = {a:.1f} ms;"
            f" with nothing changed {med['diff_again']:.1f} ms (spread {spread['diff_again']:.1f} %)")
        log(f"(b) hs_index_save {med['save']:.1f} ms + hs_convert_slim_gpu {med['convert']:.1f} ms + hs_index_load {med['load']:.1f} ms = {b:.1f} ms"
            f" (spreads {spread['save']:.1f} / {spread['convert']:.1f} / {spread['load']:.1f} %): x{b / a:.2f} of (a)")
        log("RESULT " + json.dumps(dict(n=N, count=C, threads=args.threads, first=first, **res)))
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)
