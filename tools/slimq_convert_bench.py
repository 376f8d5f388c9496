#!/usr/bin/env python3
"""slimq_convert_bench.py -- "base graph in, SlimQ index out": HierarchicalNSWSlimQ::convertFromHNSW on the device
(hs_convert_hnsw_to_slimq, csrc/convert_slimq.hip) against the host chain this repository had, on the graph the
reference's strategy builds (M = 32, ef_construction = 128):
  cohere : the COHERE-like rows of tools/rq_build_bench.py, 1M x 768 unit vectors, inner product
  sift   : the bench's SIFT-like rows, 1M x 128, L2
The base graph is built once on the device (hs_build_rabitq_hnsw_batched).  Then ONE process, wall-clock time around each call,
`--rounds` alternated rounds of
  (a) the two-step host chain: hs_convert_slimq_graph -> Slim file -> hs_convert_slimq, `--threads` threads (each step beside the sum),
  (b) hs_convert_hnsw_to_slimq with device = -1 and `--threads` threads (no intermediate file),
  (c) hs_convert_hnsw_to_slimq on device 0 (loading the graph file, uploads, kernels, downloads, host assembly and the file write
      included; the kernel time of each step beside it),
and the three SlimQ files compared byte for byte in every round.  16 centroids from a few Lloyd rounds on a sample; cluster ids
are left to the call (nearest centroid).
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
from hsutil import headline_data, load_product  # noqa: E402
from rq_build_bench import EFC, M, cohere_like, log  # noqa: E402


def summary(name, xs, unit="s"):
    med = sorted(xs)[len(xs) // 2]
    log(f"{name}: median {med:.2f} {unit} (min {min(xs):.2f}, max {max(xs):.2f}, spread {100 * (max(xs) - min(xs)) / med:.1f} %) over {len(xs)} rounds")
    return med


def centroids_of(base, k=16, sample=20_000, rounds=5):
    rng = np.random.default_rng(0)
    s = base[rng.choice(len(base), min(len(base), sample), replace=False)].astype(np.float32)
    cen = s[:k].copy()
    for _ in range(rounds):
        a = ((s * s).sum(1)[:, None] - 2.0 * s @ cen.T + (cen * cen).sum(1)[None, :]).argmin(1)
        for c in range(k):
            if np.any(a == c):
                cen[c] = s[a == c].mean(0)
    return np.ascontiguousarray(cen, np.float32)


def same_file(a, b, chunk=1 << 26):
    if os.path.getsize(a) != os.path.getsize(b):
        return False
    with open(a, "rb") as fa, open(b, "rb") as fb:
        while True:
            x, y = fa.read(chunk), fb.read(chunk)
            if x != y:
                return False
            if not x:
                return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("data", choices=["cohere", "sift"])
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--tmp", default=None, help="directory for the index files (default: the system's)")
    args = ap.parse_args()
    import torch
    torch.cuda.init()   # (torch's bundled HIP runtime opens the device before the product's does, as in bench.py)
    hs = load_product()
    N, T = args.n, args.threads
    t0 = time.perf_counter()
    if args.data == "cohere":
        d, metric = 768, hs.HS_METRIC_IP
        base = cohere_like(N, 123)
    else:
        d, metric = 128, hs.HS_METRIC_L2
        base = headline_data(N, d, 123)
    cen = centroids_of(base)
    log(f"{args.data}: rows {N} x {d}, metric {metric}, M {M}, ef_construction {EFC}, 16 centroids, {T} host threads; generated in {time.perf_counter() - t0:.0f} s")
    with tempfile.TemporaryDirectory(dir=args.tmp) as tmp:
        hp, sp, qa, qb, qc = (os.path.join(tmp, x) for x in ("hnsw.bin", "slim.bin", "chain.bin", "one_host.bin", "one_dev.bin"))
        t0 = time.perf_counter()
        st = hs.build_rabitq_hnsw_batched(base, hp, metric=metric, M=M, ef_construction=EFC, seed=100, device=0, threads=T)
        log(f"base graph: hs_build_rabitq_hnsw_batched on the device {time.perf_counter() - t0:.2f} s, {os.path.getsize(hp)} bytes, used_gpu {st['used_gpu']}")
        t = {k: [] for k in ("chain", "chain_graph", "chain_rec", "host", "host_graph", "host_rec", "dev", "dev_graph", "dev_rec", "dev_kg", "dev_kr")}
        for rnd in range(args.rounds):
            t0 = time.perf_counter()
            hs.convert_slimq_graph(hp, sp, d, metric=metric, threads=T)
            t1 = time.perf_counter()
            hs.convert_slimq(sp, metric, d, cen, qa, threads=T)
            t2 = time.perf_counter()
            t["chain"].append(t2 - t0); t["chain_graph"].append(t1 - t0); t["chain_rec"].append(t2 - t1)
            log(f"round {rnd}: (a) host chain {t2 - t0:.2f} s = hs_convert_slimq_graph {t1 - t0:.2f} s + hs_convert_slimq {t2 - t1:.2f} s; "
                f"Slim file {os.path.getsize(sp)} bytes")
            os.remove(sp)
            t0 = time.perf_counter()
            s = hs.convert_hnsw_to_slimq(hp, qb, d, cen, metric=metric, device=-1, threads=T)
            t["host"].append(time.perf_counter() - t0); t["host_graph"].append(s["graph_ms"] / 1e3); t["host_rec"].append(s["records_ms"] / 1e3)
            assert not s["graph_used_gpu"] and not s["records_used_gpu"]
            log(f"round {rnd}: (b) hs_convert_hnsw_to_slimq(device -1) {t['host'][-1]:.2f} s: graph passes {t['host_graph'][-1]:.2f} s, records {t['host_rec'][-1]:.2f} s")
            t0 = time.perf_counter()
            s = hs.convert_hnsw_to_slimq(hp, qc, d, cen, metric=metric, device=0, threads=T)
            t["dev"].append(time.perf_counter() - t0); t["dev_graph"].append(s["graph_ms"] / 1e3); t["dev_rec"].append(s["records_ms"] / 1e3)
            t["dev_kg"].append(s["graph_kernel_ms"]); t["dev_kr"].append(s["records_kernel_ms"])
            assert s["graph_used_gpu"] and s["records_used_gpu"], "hs_convert_hnsw_to_slimq declined the device"
            log(f"round {rnd}: (c) hs_convert_hnsw_to_slimq(device 0) {t['dev'][-1]:.2f} s: graph passes {t['dev_graph'][-1]:.2f} s (kernels {s['graph_kernel_ms']:.1f} ms), "
                f"records {t['dev_rec'][-1]:.2f} s (kernels {s['records_kernel_ms']:.1f} ms)")
            same = same_file(qa, qb) and same_file(qa, qc)
            log(f"round {rnd}: the three SlimQ files are {'byte-identical' if same else 'DIFFERENT'}, {os.path.getsize(qa)} bytes")
            if not same:
                sys.exit(1)
        a = summary(f"(a) host chain, {T} threads", t["chain"])
        summary("    of which hs_convert_slimq_graph", t["chain_graph"]); summary("    of which hs_convert_slimq", t["chain_rec"])
        b = summary(f"(b) one call on the host, {T} threads", t["host"])
        summary("    of which graph passes (file load included)", t["host_graph"]); summary("    of which records", t["host_rec"])
        c = summary("(c) one call on the device", t["dev"])
        summary("    of which graph passes (file load, upload, kernels, download, assembly)", t["dev_graph"])
        summary("    of which records (uploads, kernels, downloads)", t["dev_rec"])
        summary("    kernels of the graph passes", t["dev_kg"], "ms"); summary("    kernels of the records", t["dev_kr"], "ms")
        log(f"(a) / (b), medians: {a / b:.2f}x;  (a) / (c), medians: {a / c:.2f}x")


if __name__ == "__main__":
    main()
