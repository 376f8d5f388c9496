#!/usr/bin/env python3
"""live_batched_add_bench.py -- blocks of rows added to a resident vanilla index in the batched order on its device
(hs_index_add_points_batched) against the host calls for the same start state, hs_index_add_points with `--threads`
threads and with one, on the bench's rows (tests/hsutil.py::headline_data(1M, 128, 123), M = 16, efC = 200).

The resident index holds the first `--prefix` rows (built once on the device, hs_build_hnsw_batched, so the start state is the same
file for every call).  For each block size, `--rounds` alternated rounds in ONE process: a fresh load of the prefix file with room,
the generator seeded, wall clock around the one call under test (every call synchronises the device).  Reported beside the time:
the device time, batches, flagged rows, old lists downloaded and old nodes changed of the batched call, and recall@10 at `--ef` of
each result against hs_index_exact_search over the same index (once per method and block).  The serial host call is skipped for
blocks above `--serial-max` rows in all rounds but the first.
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
from hsutil import headline_data, load_product  # noqa: E402

D, NQ, K = 128, 2000, 10


def log(*a):
    print(*a, flush=True)


def clock(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


def recall(ix, q, ef):
    ix.set_ef(ef)
    got = ix.search_pq(q, K)
    want = ix.exact_search(q, K)
    hits = sum(len(set(got["labels"][i][:got["cnt"][i]].tolist()) & set(want["labels"][i].tolist())) for i in range(len(q)))
    return hits / (K * len(q))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--prefix", type=int, default=900_000)
    ap.add_argument("--blocks", default="1000,10000,100000")
    ap.add_argument("--ef", type=int, default=70)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--serial-max", type=int, default=10_000)
    args = ap.parse_args()
    hs = load_product()
    N, n0 = args.n, args.prefix
    blocks = [int(b) for b in args.blocks.split(",")]
    assert n0 + max(blocks) <= N
    base = headline_data(N, D, 123)
    q = headline_data(NQ, D, 456)
    result = dict(n=N, prefix=n0, threads=args.threads, ef=args.ef, blocks={})
    with tempfile.TemporaryDirectory() as tmp:
        part = os.path.join(tmp, "part.bin")
        ms, st = clock(lambda: hs.build_hnsw_batched(base[:n0], part, M=16, ef_construction=200, branching_factor="4", seed=100, device=0, threads=args.threads))
        log(f"prefix graph: {n0} rows, hs_build_hnsw_batched on the device, {ms / 1e3:.1f} s wall, {st['kernel_ms'] / 1e3:.2f} s device, {st['batches']} batches")

        def fresh(count):
            ix = hs.Index(part, hs.HS_KIND_HNSW, D, max_elements=n0 + count)
            ix.seed_levels(100, n0)
            return ix

        for count in blocks:
            rows, labels = base[n0:n0 + count], np.arange(n0, n0 + count, dtype=np.uint64)
            methods = {
                "batched": lambda ix: ix.add_points_batched(rows, labels, threads=args.threads),
                f"host{args.threads}": lambda ix: ix.add_points(rows, labels, threads=args.threads),
                "host1": lambda ix: ix.add_points(rows, labels, threads=1),
            }
            times = {m: [] for m in methods}
            extra, rec = {}, {}
            for rnd in range(args.rounds):
                for m, fn in methods.items():
                    if m == "host1" and count > args.serial_max and rnd > 0:
                        continue
                    ix = fresh(count)
                    ms, st = clock(lambda: fn(ix))
                    times[m].append(ms)
                    note = ""
                    if m == "batched":
                        changed, downloaded = ix.batched_add_changed()
                        extra = dict(used_gpu=st["used_gpu"], device_ms=st["kernel_ms"], batches=st["batches"], flagged_rows=st["flagged_rows"],
                                     lists_downloaded=int(downloaded), old_nodes_changed=int(len(changed)))
                        note = (f" (device {st['kernel_ms']:.1f} ms, {st['batches']} batches, {st['flagged_rows']} flagged rows, {downloaded} old lists "
                                f"downloaded, {len(changed)} old nodes changed, used_gpu {int(st['used_gpu'])})")
                    if m not in rec:
                        rec[m] = recall(ix, q, args.ef)
                        note += f"; recall@{K} at ef {args.ef} over {NQ} queries {rec[m]:.4f}"
                    log(f"block {count} round {rnd} {m}: {ms:.1f} ms{note}")
                    del ix
            med = {m: float(np.median(t)) for m, t in times.items()}
            hostN = f"host{args.threads}"
            verdict = "faster than" if med["batched"] < med[hostN] else "SLOWER than"
            log(f"block {count}: batched {med['batched']:.1f} ms | {args.threads} host threads {med[hostN]:.1f} ms | serial {med['host1']:.1f} ms "
                f"({len(times['host1'])} run(s)) -> the batched call is {verdict} the {args.threads}-thread host call (x{med[hostN] / med['batched']:.2f}), "
                f"x{med['host1'] / med['batched']:.1f} of the serial one")
            result["blocks"][count] = dict(ms=times, median_ms=med, recall=rec, **extra)
    log("RESULT " + json.dumps(result))
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)
