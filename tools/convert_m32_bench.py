#!/usr/bin/env python3
"""convert_m32_bench.py -- the two Slim conversions at the reference's default graph shape: 1M x 128 rows (the cached data of
bench.py when it is there, the same generator otherwise), the vanilla graph built here by the host builder with `--threads` threads
(`--M` 32, `--efc` 128: maxM0 = 64, the device path's 64-slot stride; `--M 16 --efc 200` is the 32-slot stride).  ONE process,
wall-clock time around each call (every call synchronises the device), `--rounds` alternated rounds of

  (1) convertFromHNSW file to file: hs_convert_slim_gpu against hs_convert_slim(threads) -- load, convert, save in both;
  (2) the patch server's call after `--count` added rows: hs_slim_convert_diff on two resident indexes, loaded afresh and grown
      with hs_index_add_points in every round, against the same call on a pair whose device path is disabled.  The switch is one
      of the documented fall-backs: the vanilla index drops its fp32 rows (u8 row format), so the list passes and the diff run on
      the host and the changed rows are uploaded from the host image.

The host path of both is what the library ran for an M = 32 graph before the device path took capacities of 64.
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
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--M", type=int, default=32)
    ap.add_argument("--efc", type=int, default=128)
    ap.add_argument("--count", type=int, default=1000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--index-dir", default="", help="index files of bench.py --index-dir instead of the user cache directory")
    args = ap.parse_args()
    import torch
    torch.cuda.init()   # (torch's bundled HIP runtime opens the device before the product's does, as in bench.py)
    hs = load_product()
    N, C, T = args.n, args.count, args.threads
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
        full, slim, a, b = (os.path.join(tmp, x) for x in ("full.bin", "slim.bin", "host.slim", "gpu.slim"))
        t_build, _ = clock(lambda: hs.build_hnsw(base, full, M=args.M, ef_construction=args.efc, branching_factor="4", seed=100, threads=T))
        log(f"graph: {N} x {D} rows, M = {args.M}, ef_construction = {args.efc}, built with {T} host threads in {t_build / 1e3:.1f} s")
        # ---- (1) convertFromHNSW, file to file
        hs.convert_slim_gpu(full, b, D, threads=T)   # warm-up: code object load, first allocations
        res = dict(gpu=[], gpu_kernel=[], host=[])
        for rnd in range(args.rounds):
            t, (used, ms) = clock(lambda: hs.convert_slim_gpu(full, b, D, threads=T))
            assert used, "hs_convert_slim_gpu declined the graph"
            res["gpu"].append(t)
            res["gpu_kernel"].append(ms)
            res["host"].append(clock(lambda: hs.convert_slim(full, a, D, threads=T))[0])
            log(f"convert round {rnd}: hs_convert_slim_gpu {res['gpu'][-1]:.1f} ms (kernels {ms:.1f} ms) | hs_convert_slim({T} threads) {res['host'][-1]:.1f} ms")
        same = open(a, "rb").read() == open(b, "rb").read()
        assert same, "the two Slim files differ"
        # ---- (2) the patch server's call; the starting Slim index is one conversion from an empty one
        t_conv, _ = clock(lambda: hs.slim_convert_diff_files(None, full, slim, D, threads=T).close())
        log(f"first Slim conversion from an empty index, on the host: {t_conv / 1e3:.1f} s")
        res.update(diff_dev=[], diff_dev_kernel=[], diff_host=[])
        first, streams = {}, {}
        for rnd in range(args.rounds):
            for path in ("dev", "host"):
                hx = hs.Index(full, hs.HS_KIND_HNSW, D, max_elements=cap)
                sx = hs.Index(slim, hs.HS_KIND_SLIM, D, max_elements=cap)
                hx.add_points(new_rows, new_labels, threads=1)
                if path == "host":
                    hx.set_row_format(hs.HS_ROWS_U8)
                    hx.set_f32_resident(False)
                t, d = clock(lambda: sx.convert_diff(hx, threads=T))
                assert bool(d.used_gpu) == (path == "dev"), f"{path}: used_gpu = {d.used_gpu}"
                res["diff_" + path].append(t)
                if path == "dev":
                    res["diff_dev_kernel"].append(d.kernel_ms)
                if rnd == 0:
                    streams[path] = d.stream()
                    first[path] = d.info()
                d.close()
                del d, hx, sx
            log(f"diff round {rnd}: hs_slim_convert_diff on the device {res['diff_dev'][-1]:.1f} ms (kernels {res['diff_dev_kernel'][-1]:.1f} ms)"
                f" | device path disabled {res['diff_host'][-1]:.1f} ms")
        assert streams["dev"] == streams["host"] and first["dev"] == first["host"], "the two paths disagree"
        med = {k: float(np.median(v)) for k, v in res.items()}
        spread = {k: (max(v) - min(v)) / np.median(v) * 100 for k, v in res.items()}
        log(f"(1) hs_convert_slim_gpu {med['gpu']:.1f} ms (spread {spread['gpu']:.1f} %), of which kernels {med['gpu_kernel']:.1f} ms;"
            f" hs_convert_slim({T} threads) {med['host']:.1f} ms (spread {spread['host']:.1f} %): x{med['host'] / med['gpu']:.2f}; files byte-identical: {same}")
        log(f"(2) hs_slim_convert_diff after {C} added rows {json.dumps(first['dev'])}: device {med['diff_dev']:.1f} ms (spread {spread['diff_dev']:.1f} %),"
            f" of which kernel_ms {med['diff_dev_kernel']:.1f}; device path disabled {med['diff_host']:.1f} ms (spread {spread['diff_host']:.1f} %):"
            f" x{med['diff_host'] / med['diff_dev']:.2f}; streams byte-identical: True")
        log("RESULT " + json.dumps(dict(n=N, M=args.M, efc=args.efc, count=C, threads=T, first=first["dev"], **res)))
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)
