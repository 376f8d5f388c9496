#!/usr/bin/env python3
"""slimq_resident_bench.py -- "rows in, searchable SlimQ index out" with no file on the way (hs_slimq_index_from_rows)
against the file chain this repository had, and the load step alone against the parent commit's library, on the graph the
reference's strategy builds (M = 32, ef_construction = 128):
  cohere : the COHERE-like rows of tools/rq_build_bench.py, 1M x 768 unit vectors, inner product
  sift   : the bench's SIFT-like rows, 1M x 128, L2
16 centroids from a few Lloyd rounds on a sample; cluster ids are left to the calls (nearest centroid).

  pipeline <data>   ONE process, `--rounds` alternated rounds of
      (a) the chain: hs_build_rabitq_hnsw_batched -> file, hs_convert_hnsw_to_slimq -> file, hs_index_load, hs_slimq_set_dataset, each
          step timed,
      (b) hs_slimq_index_from_rows(with_dataset = 1), by its hs_slimq_pipeline_stats,
      and the three record arrays of the two indexes compared word for word in the first round.
  load <data> --parent-lib PATH   the SlimQ file written once, then `--rounds` alternated rounds of ONE process each that times
      hs_index_load of it: with the library at PATH (the parent commit's, built in a scratch directory; host tile assembly + upload)
      and with this tree's library (upload + tile kernels).  HS_LIB selects the library of a child.
  load-one FILE DIM METRIC   (the child of `load`) prints the seconds of one hs_index_load, after one warm-up load of a tiny index
Output: the log on stdout.
"""
import argparse
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from hsutil import headline_data, load_product  # noqa: E402
from rq_build_bench import EFC, M, cohere_like, log  # noqa: E402
from slimq_convert_bench import centroids_of, summary  # noqa: E402


def rows_of(hs, data, n):
    if data == "cohere":
        return cohere_like(n, 123), 768, hs.HS_METRIC_IP
    return headline_data(n, 128, 123), 128, hs.HS_METRIC_L2


def pipeline(hs, args):
    N, T = args.n, args.threads
    base, d, metric = rows_of(hs, args.data, N)
    cen = centroids_of(base)
    log(f"{args.data}: rows {N} x {d}, metric {metric}, M {M}, ef_construction {EFC}, 16 centroids, {T} host threads")
    t = {k: [] for k in ("chain", "build", "convert", "load", "dataset", "rows", "r_build", "r_convert", "r_resident", "r_tiles")}
    with tempfile.TemporaryDirectory(dir=args.tmp) as tmp:
        hp, qp = os.path.join(tmp, "hnsw.bin"), os.path.join(tmp, "slimq.bin")
        for rnd in range(args.rounds):
            t0 = time.perf_counter()
            hs.build_rabitq_hnsw_batched(base, hp, metric=metric, M=M, ef_construction=EFC, seed=100, device=0, threads=T)
            t1 = time.perf_counter()
            hs.convert_hnsw_to_slimq(hp, qp, d, cen, metric=metric, device=0, threads=T)
            t2 = time.perf_counter()
            b = hs.Index(qp, hs.HS_KIND_SLIMQ, d, metric=metric)
            t3 = time.perf_counter()
            b.slimq_set_dataset(base)
            t4 = time.perf_counter()
            for k, v in (("chain", t4 - t0), ("build", t1 - t0), ("convert", t2 - t1), ("load", t3 - t2), ("dataset", t4 - t3)):
                t[k].append(v)
            log(f"round {rnd}: (a) chain {t4 - t0:.2f} s = build to a file {t1 - t0:.2f} + convert to a file {t2 - t1:.2f} + hs_index_load {t3 - t2:.2f} "
                f"+ hs_slimq_set_dataset {t4 - t3:.2f}; graph file {os.path.getsize(hp)} bytes, SlimQ file {os.path.getsize(qp)} bytes")
            t0 = time.perf_counter()
            a, st = hs.slimq_index_from_rows(base, cen, metric=metric, M=M, ef_construction=EFC, seed=100, device=0, threads=T, with_dataset=True)
            t["rows"].append(time.perf_counter() - t0)
            t["r_build"].append(st["build"]["total_ms"] / 1e3); t["r_convert"].append(st["convert"]["total_ms"] / 1e3)
            t["r_resident"].append(st["resident_ms"] / 1e3); t["r_tiles"].append(st["tile_kernel_ms"])
            log(f"round {rnd}: (b) hs_slimq_index_from_rows {t['rows'][-1]:.2f} s: build {t['r_build'][-1]:.2f}, conversion and residency {t['r_convert'][-1]:.2f} "
                f"of which residency {t['r_resident'][-1]:.2f} (tile kernels {st['tile_kernel_ms']:.1f} ms)")
            if rnd == 0:
                same = a.info() == b.info()
                for which in (0, 1, 2):
                    x, y = a.debug_slimq_arrays(which), b.debug_slimq_arrays(which)
                    same = same and x[1:] == y[1:] and np.array_equal(x[0], y[0])
                    del x, y
                log(f"round 0: the two indexes' hs_info and three record arrays are {'identical' if same else 'DIFFERENT'}")
                if not same:
                    sys.exit(1)
            a.close(); b.close()
    ca = summary("(a) the file chain", t["chain"])
    for k, name in (("build", "hs_build_rabitq_hnsw_batched"), ("convert", "hs_convert_hnsw_to_slimq"), ("load", "hs_index_load"), ("dataset", "hs_slimq_set_dataset")):
        summary(f"    of which {name}", t[k])
    cb = summary("(b) hs_slimq_index_from_rows", t["rows"])
    summary("    of which the build", t["r_build"]); summary("    of which conversion and residency", t["r_convert"])
    summary("    of which residency (packing, uploads, tile kernels, dataset)", t["r_resident"]); summary("    tile kernels", t["r_tiles"], "ms")
    log(f"(a) / (b), medians: {ca / cb:.2f}x")


def load_ab(hs, args):
    N, T = args.n, args.threads
    base, d, metric = rows_of(hs, args.data, N)
    cen = centroids_of(base)
    here = hs.LIB_PATH
    log(f"{args.data}: rows {N} x {d}; parent library {args.parent_lib}, this library {here}")
    t = {"parent": [], "this": []}
    with tempfile.TemporaryDirectory(dir=args.tmp) as tmp:
        hp, qp = os.path.join(tmp, "hnsw.bin"), os.path.join(tmp, "slimq.bin")
        hs.build_rabitq_hnsw_batched(base, hp, metric=metric, M=M, ef_construction=EFC, seed=100, device=0, threads=T)
        hs.convert_hnsw_to_slimq(hp, qp, d, cen, metric=metric, device=0, threads=T)
        os.remove(hp)
        del base
        log(f"SlimQ file {os.path.getsize(qp)} bytes")
        for rnd in range(args.rounds):
            for name, lib in (("parent", args.parent_lib), ("this", here)):
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "load-one", qp, str(d), str(metric)], env=dict(os.environ, HS_LIB=lib),
                                     capture_output=True, text=True, timeout=1200)
                if out.returncode != 0:
                    log(f"round {rnd}: {name}: FAILED\n{out.stdout}{out.stderr}")
                    sys.exit(1)
                sec, dev_bytes = out.stdout.split()[-2:]
                t[name].append(float(sec))
                log(f"round {rnd}: hs_index_load with the {name} library {float(sec):.2f} s, device_bytes {dev_bytes}")
    p = summary("hs_index_load, parent library (host tile assembly + upload)", t["parent"])
    c = summary("hs_index_load, this library (upload + tile kernels)", t["this"])
    log(f"parent / this, medians: {p / c:.2f}x")


def load_one(hs, path, d, metric):
    import torch
    torch.cuda.init()
    hs.device_count()
    t0 = time.perf_counter()
    ix = hs.Index(path, hs.HS_KIND_SLIMQ, d, metric=metric)
    sec = time.perf_counter() - t0
    print(f"{sec:.4f} {ix.info()['device_bytes']}")
    ix.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["pipeline", "load", "load-one"])
    ap.add_argument("data")
    ap.add_argument("rest", nargs="*")
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--tmp", default=None, help="directory for the index files (default: the system's)")
    args = ap.parse_args()
    hs = load_product()
    if args.mode == "load-one":
        return load_one(hs, args.data, int(args.rest[0]), int(args.rest[1]))
    if args.data not in ("cohere", "sift"):
        ap.error("data: cohere or sift")
    import torch
    torch.cuda.init()   # (torch's bundled HIP runtime opens the device before the product's does, as in bench.py)
    if args.mode == "pipeline":
        return pipeline(hs, args)
    if not args.parent_lib or not os.path.exists(args.parent_lib):
        ap.error("load: --parent-lib, the parent commit's libhnsw_slim_amd.so")
    load_ab(hs, args)


if __name__ == "__main__":
    main()
