#!/usr/bin/env python3
"""rq_build_bench.py -- building HNSW-SlimQ's base graph (rabitqlib's builder) on the device (hs_build_rabitq_hnsw_batched, the rq
kernels of csrc/build_gpu.hip) against the host builders, at the reference strategy's M = 32, ef_construction = 128:
  cohere : the COHERE-like rows of tools/slimq_config.py, 1M x 768 unit vectors, inner product
  sift   : the bench's SIFT-like rows, 1M x 128, L2
ONE process, wall-clock time around each call, `--rounds` alternated rounds of
  (a) hs_build_rabitq_hnsw_batched on device 0 (upload, kernels, download and the file write included; its own kernel_ms beside it),
  (b) its host twin (device = -1) with `--threads` threads, in the first `--twin-rounds` rounds; the two files are compared,
  (c) hs_build_rabitq_hnsw with `--threads` threads (the timing-dependent parallel builder this repository had before).
Then recall@10 at ef `--ef`: the file loaded as a vanilla index (hs.Index, search_pq) against hs_index_exact_search on the same
rows, for the batched graph and for the last threaded graph.
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
from hsutil import headline_data, load_product, sift_like  # noqa: E402

M, EFC = 32, 128


def log(*a):
    print(*a, flush=True)


def spread(name, xs, unit="s"):
    log(f"{name}: min {min(xs):.2f} median {sorted(xs)[len(xs) // 2]:.2f} max {max(xs):.2f} {unit} over {len(xs)} rounds ({', '.join(f'{x:.2f}' for x in xs)})")


def cohere_like(m, seed, d=768):
    x = sift_like(m, d, seed, n_clusters=256, rank=24, sigma_sub=40.0, sigma_iso=1.5, integer=False, centre_lo=-40.0, centre_hi=40.0)
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def recall_of(hs, path, d, metric, q, ef, k=10):
    ix = hs.Index(path, hs.HS_KIND_HNSW, d, metric=metric)
    ix.set_ef(ef)
    got = ix.search_pq(q, k)
    want = ix.exact_search(q, k)
    hits = sum(len(set(map(int, got["labels"][i][:got["cnt"][i]])) & set(map(int, want["labels"][i][:want["cnt"][i]]))) for i in range(len(q)))
    ix.close()
    return hits / (k * len(q))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("data", choices=["cohere", "sift"])
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--twin-rounds", type=int, default=-1, help="rounds that also build the host twin (-1: all)")
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--ef", type=int, default=100)
    ap.add_argument("--nq", type=int, default=2000)
    ap.add_argument("--no-host", action="store_true", help="skip (c)")
    args = ap.parse_args()
    import torch
    torch.cuda.init()   # (torch's bundled HIP runtime opens the device before the product's does, as in bench.py)
    hs = load_product()
    N = args.n
    t0 = time.perf_counter()
    if args.data == "cohere":
        d, metric = 768, hs.HS_METRIC_IP
        base, q = cohere_like(N, 123), cohere_like(args.nq, 456)
    else:
        d, metric = 128, hs.HS_METRIC_L2
        base, q = headline_data(N, d, 123), headline_data(args.nq, d, 456)
    log(f"{args.data}: rows {N} x {d}, metric {metric}, M {M}, ef_construction {EFC}; {args.nq} queries; generated in {time.perf_counter() - t0:.0f} s")
    twin_rounds = args.rounds if args.twin_rounds < 0 else args.twin_rounds
    with tempfile.TemporaryDirectory() as tmp:
        dev, twin, par = (os.path.join(tmp, x) for x in ("dev.bin", "twin.bin", "par.bin"))
        t_dev, t_ker, t_twin, t_par = [], [], [], []
        for rnd in range(args.rounds):
            t0 = time.perf_counter()
            st = hs.build_rabitq_hnsw_batched(base, dev, metric=metric, M=M, ef_construction=EFC, seed=100, device=0, threads=args.threads)
            t_dev.append(time.perf_counter() - t0); t_ker.append(st["kernel_ms"] / 1e3)
            assert st["used_gpu"]
            log(f"round {rnd}: device build {t_dev[-1]:.2f} s wall, kernels {t_ker[-1]:.2f} s, {st['batches']} batches, {st['flagged_rows']} flagged rows")
            if rnd < twin_rounds:
                t0 = time.perf_counter()
                hs.build_rabitq_hnsw_batched(base, twin, metric=metric, M=M, ef_construction=EFC, seed=100, device=-1, threads=args.threads)
                t_twin.append(time.perf_counter() - t0)
                same = open(dev, "rb").read() == open(twin, "rb").read()
                log(f"round {rnd}: host twin with {args.threads} threads {t_twin[-1]:.2f} s; the device file {'equals' if same else 'DIFFERS FROM'} the twin's, "
                    f"{os.path.getsize(dev)} bytes")
                os.remove(twin)
                if not same:
                    sys.exit(1)
            if not args.no_host:
                t0 = time.perf_counter()
                hs.build_rabitq_hnsw(base, par, metric=metric, M=M, ef_construction=EFC, seed=100, threads=args.threads)
                t_par.append(time.perf_counter() - t0)
                log(f"round {rnd}: hs_build_rabitq_hnsw with {args.threads} threads {t_par[-1]:.2f} s")
        spread("(a) device build, wall", t_dev)
        spread("(a) device build, kernels", t_ker)
        if t_twin:
            spread(f"(b) host twin, {args.threads} threads", t_twin)
        if t_par:
            spread(f"(c) hs_build_rabitq_hnsw, {args.threads} threads", t_par)
            log(f"(c) / (a), medians: {sorted(t_par)[len(t_par) // 2] / sorted(t_dev)[len(t_dev) // 2]:.2f}x")
        log(f"recall@10 at ef {args.ef}, batched graph (device): {recall_of(hs, dev, d, metric, q, args.ef):.4f}")
        if t_par:
            log(f"recall@10 at ef {args.ef}, graph of the last threaded build: {recall_of(hs, par, d, metric, q, args.ef):.4f}")


if __name__ == "__main__":
    main()
