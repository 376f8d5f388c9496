#!/usr/bin/env python3
"""gpu_build_bench.py -- building the HNSW graph on the device (hs_build_hnsw_batched, csrc/build_gpu.hip) against the host
builders, on the bench's rows: 1M x 128 (the cached data of bench.py when it is there, the same generator otherwise), M = 16,
ef_construction = 200, as bench.py builds its index.  ONE process, wall-clock time around each call, `--rounds` alternated rounds of
  (a) hs_build_hnsw_batched on device 0 (upload, kernels, download and the file write included; its own kernel_ms beside it),
  (b) hs_build_hnsw with `--threads` threads (the timing-dependent parallel builder).
The serial builder's time is not measured here (ten minutes of one core): it is the figure in the log of the cached bench build.
Then recall@10 at ef `--ef` of the resident search (hs.Index of the vanilla file, search_pq) over the device-built graph, over the
last parallel-built graph and, with --serial-index, over a serial graph, against hs_index_exact_search on the same rows.
`--check-twin` builds the host twin (device = -1) of the same schedule once and compares the two files byte for byte.
`--schedules` runs (a) once per "grow_div:batch_max:scratch_ids" triple before the rounds, to choose the defaults from.
Output: the log on stdout.
"""
import argparse
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


def spread(name, xs, unit="s"):
    log(f"{name}: min {min(xs):.2f} median {sorted(xs)[len(xs) // 2]:.2f} max {max(xs):.2f} {unit} over {len(xs)} rounds ({', '.join(f'{x:.2f}' for x in xs)})")


def recall_of(hs, path, q, ef, k=10):
    ix = hs.Index(path, hs.HS_KIND_HNSW, D)
    ix.set_ef(ef)
    got = ix.search_pq(q, k)
    want = ix.exact_search(q, k)
    hits = sum(len(set(map(int, got["labels"][i][:got["cnt"][i]])) & set(map(int, want["labels"][i][:want["cnt"][i]]))) for i in range(len(q)))
    ix.close()
    return hits / (k * len(q))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--ef", type=int, default=70)
    ap.add_argument("--nq", type=int, default=10_000)
    ap.add_argument("--grow-div", type=int, default=0)
    ap.add_argument("--batch-max", type=int, default=0)
    ap.add_argument("--scratch-ids", type=int, default=0)
    ap.add_argument("--schedules", default="", help="comma-separated grow_div:batch_max:scratch_ids triples, each built once on the device")
    ap.add_argument("--no-host", action="store_true", help="skip (b)")
    ap.add_argument("--check-twin", action="store_true", help="also build the host twin and compare the two files byte for byte")
    ap.add_argument("--serial-index", default="", help="a serially built vanilla index of the same rows (recall only)")
    ap.add_argument("--index-dir", default="", help="index files of bench.py --index-dir instead of the user cache directory")
    args = ap.parse_args()
    import torch
    torch.cuda.init()   # (torch's bundled HIP runtime opens the device before the product's does, as in bench.py)
    hs = load_product()
    N = args.n
    idir = args.index_dir or index_cache_dir(N, D, 1)
    if os.path.exists(os.path.join(idir, "ready")) and os.path.exists(os.path.join(idir, "base.npy")):
        base = np.load(os.path.join(idir, "base.npy"))[:N]
    else:
        base = headline_data(N, D, 123)
    q = headline_data(args.nq, D, 456)
    log(f"rows: {N} x {D}, M 16, ef_construction 200; {args.nq} queries")
    with tempfile.TemporaryDirectory() as tmp:
        dev, par = os.path.join(tmp, "dev.bin"), os.path.join(tmp, "par.bin")

        def device_build(grow_div, batch_max, scratch_ids):
            t0 = time.perf_counter()
            st = hs.build_hnsw_batched(base, dev, M=16, ef_construction=200, branching_factor="4", seed=100, device=0, threads=args.threads,
                                       grow_div=grow_div, batch_max=batch_max, scratch_ids=scratch_ids)
            return time.perf_counter() - t0, st

        for triple in filter(None, args.schedules.split(",")):
            gd, bm, si = (int(x) for x in triple.split(":"))
            t, st = device_build(gd, bm, si)
            log(f"schedule grow_div {gd} batch_max {bm} scratch_ids {si}: {t:.2f} s wall, kernels {st['kernel_ms'] / 1e3:.2f} s, {st['batches']} batches, "
                f"{st['flagged_rows']} flagged rows, recall@10 ef {args.ef} {recall_of(hs, dev, q, args.ef):.4f}")
        t_dev, t_ker, t_par = [], [], []
        for rnd in range(args.rounds):
            t, st = device_build(args.grow_div, args.batch_max, args.scratch_ids)
            assert st["used_gpu"]
            t_dev.append(t); t_ker.append(st["kernel_ms"] / 1e3)
            log(f"round {rnd}: device build {t:.2f} s wall, kernels {st['kernel_ms'] / 1e3:.2f} s, {st['batches']} batches, {st['flagged_rows']} flagged rows")
            if not args.no_host:
                t0 = time.perf_counter()
                hs.build_hnsw(base, par, M=16, ef_construction=200, branching_factor="4", seed=100, threads=args.threads)
                t_par.append(time.perf_counter() - t0)
                log(f"round {rnd}: hs_build_hnsw with {args.threads} threads {t_par[-1]:.2f} s")
        if t_dev:
            spread("(a) device build, wall", t_dev)
            spread("(a) device build, kernels", t_ker)
            log(f"recall@10 at ef {args.ef}, device-built graph: {recall_of(hs, dev, q, args.ef):.4f}")
        if t_par:
            spread(f"(b) hs_build_hnsw, {args.threads} threads", t_par)
            log(f"recall@10 at ef {args.ef}, graph of the last parallel build: {recall_of(hs, par, q, args.ef):.4f}")
        if args.check_twin:
            t, st = device_build(args.grow_div, args.batch_max, args.scratch_ids)
            t0 = time.perf_counter()
            hs.build_hnsw_batched(base, par, M=16, ef_construction=200, branching_factor="4", seed=100, device=-1, threads=args.threads,
                                  grow_div=args.grow_div, batch_max=args.batch_max)
            same = open(dev, "rb").read() == open(par, "rb").read()
            log(f"host twin with {args.threads} threads {time.perf_counter() - t0:.2f} s; device file ({st['flagged_rows']} flagged rows) "
                f"{'equals' if same else 'DIFFERS FROM'} the twin's, {os.path.getsize(dev)} bytes")
            if not same:
                sys.exit(1)
        if args.serial_index:
            log(f"recall@10 at ef {args.ef}, serial graph {args.serial_index}: {recall_of(hs, args.serial_index, q, args.ef):.4f}")


if __name__ == "__main__":
    main()
