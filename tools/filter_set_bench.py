#!/usr/bin/env python3
"""filter_set_bench.py -- filter sets (hs_filter_set_*, hs_search_batch_filter_set) against hs_search_batch_filtered, the entry they
do not touch, on the bench's own workload: the cached 1M x 128 index and query seed of bench.py, k = 10, ef = 70.  ONE loaded index
in ONE process, old and new alternated old, new, old, new, ... for three rounds after both have been warmed; every figure is the
median of `--reps` host-timed calls (wall clock around the whole call: that is how these host entry points are used).

  (a) 10 000 queries under ONE 50 % filter: one hs_search_batch_filtered call (rebuilds deleted | !allowed on the host and uploads
      n bytes, every call) vs one hs_search_batch_filter_set call on a resident one-row set;
  (b) 10 000 queries under 16 DIFFERENT 50 % filters, 625 queries each: 16 hs_search_batch_filtered calls vs ONE set call;
  (c) 1000 single-query calls under one filter -- what the facade's searchKnn(q, k, isIdAllowed) issues per call with a cached
      functor: before, hs_search_batch_filtered with the cached allowed[] bytes; now, hs_search_batch_filter_set on the cached
      one-row set.  (The same C ABI calls hnswlib_amd.h makes, issued from this process; the Python call overhead is on both sides.)

Every new answer is compared with the old one, byte for byte.  The spread of the old entry's own rounds is the noise.
Output: the log on stdout.
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

N, D, NQ, K, NF = 1_000_000, 128, 10_000, 10, 16


def log(*a):
    print(*a, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ef", type=int, default=70)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--singles", type=int, default=1000)
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
    rng = np.random.default_rng(3)
    masks = (rng.random((NF, N)) < 0.5).astype(np.uint8)
    per = NQ // NF
    foq16 = np.repeat(np.arange(NF, dtype=np.uint32), per)
    zero = np.zeros(NQ, np.uint32)
    t0 = time.perf_counter()
    fs = hs.FilterSet.create(ix, NF)
    fs.write(0, masks)
    t_write = time.perf_counter() - t0
    info = fs.info()
    log(f"filter set: {NF} rows x {info['row_words']} words = {info['device_bytes'] / 2**20:.2f} MiB on the device; created and written from "
        f"{masks.nbytes / 2**20:.1f} MiB of host bytes in {t_write * 1e3:.1f} ms (once)")

    def a_old():
        return [ix.search_filtered(q, K, masks[0], want_stats=True)]

    def a_new():
        return [ix.search_filter_set(q, K, fs, zero, want_stats=True)]

    def b_old():
        return [ix.search_filtered(q[f * per:(f + 1) * per], K, masks[f], want_stats=True) for f in range(NF)]

    def b_new():
        r = ix.search_filter_set(q, K, fs, foq16, want_stats=True)
        return [{key: v[f * per:(f + 1) * per] for key, v in r.items()} for f in range(NF)]

    ns = args.singles
    one = np.zeros(1, np.uint32)

    def c_old():
        return [ix.search_filtered(q[i:i + 1], K, masks[0]) for i in range(ns)]

    def c_new():
        return [ix.search_filter_set(q[i:i + 1], K, fs, one) for i in range(ns)]

    cases = (("a: 10k queries, 1 filter", a_old, a_new, f"ms per {NQ}-query call"),
             ("b: 10k queries, 16 filters", b_old, b_new, f"ms per {NQ} queries (old: 16 calls, new: 1)"),
             (f"c: {ns} single-query calls", c_old, c_new, f"ms per {ns} calls"))

    def same(x, y, what):
        assert len(x) == len(y)
        for u, v in zip(x, y):
            for key in ("labels", "dists", "cnt"):
                assert np.ascontiguousarray(u[key]).tobytes() == np.ascontiguousarray(v[key]).tobytes(), f"{what}: {key} differs"
            if u.get("stats") is not None and v.get("stats") is not None:
                assert np.array_equal(u["stats"][:, :3], v["stats"][:, :3]), f"{what}: counters differ"

    for name, old, new, _ in cases:   # warm both, check the answers and the kernel
        ro = old()
        k_old = ix.last_kernel()
        rn = new()
        assert ix.last_kernel() == k_old, (name, k_old, ix.last_kernel())
        same(ro, rn, name)
        log(f"{name}: kernel {k_old} on both sides, outputs identical")
    rows = {name: dict(old=[], new=[]) for name, _, _, _ in cases}
    for rnd in range(args.rounds):
        for name, old, new, unit in cases:
            reps = args.reps if not name.startswith("c") else max(args.reps // 3, 1)
            for side, fn in (("old", old), ("new", new)):
                ts = []
                for _ in range(reps):
                    t0 = time.perf_counter()
                    fn()
                    ts.append((time.perf_counter() - t0) * 1e3)
                rows[name][side].append(float(np.median(ts)))
                log(f"round {rnd} {name} {side}: {np.median(ts):.3f} {unit} (median of {reps}, min {min(ts):.3f})")
    log("\ncase | hs_search_batch_filtered ms (rounds) | filter set ms (rounds) | old / new (medians) | spread of the old entry's rounds")
    for name, _, _, _ in cases:
        o, n = rows[name]["old"], rows[name]["new"]
        spread = (max(o) - min(o)) / np.median(o) * 100
        delta = (np.median(n) / np.median(o) - 1) * 100
        verdict = "not slower" if delta <= spread else f"slower by {delta:.2f} %"
        log(f"{name} | {np.median(o):.3f} ({', '.join(f'{x:.3f}' for x in o)}) | {np.median(n):.3f} ({', '.join(f'{x:.3f}' for x in n)}) | "
            f"{np.median(o) / np.median(n):.2f}x | {spread:.2f} % -> {verdict}")
    log("RESULT " + json.dumps(dict(ef=args.ef, ms=rows)))
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)
