#!/usr/bin/env python3
"""search_queue_bench.py -- the search queue (hs_queue_*) on the bench's own workload: the cached 1M x 128 index and query seeds
of bench.py, k = 10, ef = 70.  ONE loaded index in ONE process, the legs alternated for `--rounds` rounds after all have been
warmed; every figure is host wall clock around work that ends in a synchronisation, PCIe included (host queries in, host labels
out), and the spread of a leg's rounds is its noise.

  leg 1, small batches: 1250- and 2500-query host submissions.
      (a) today's path: hs_search_batch_async, page-locked buffers, 16 streams round-robin, as bench.py drives it;
      (b) the queue: 8 resp. 4 submissions per launch (flush after each group), slots = 2 and 4;
      (c) the ceiling: 10 000-query hs_search_batch_async batches, 16 streams.
      Reported: (b)/(a) and (b)/(c); the review's goal for (b)/(c) is >= 0.90.
  leg 2, single queries: 1, 8 and 64 client threads, one searchKnn per query through the facade (tools/search_queue_clients.cpp,
      compiled here when its binary is missing): SearchQueue<float>::searchKnn against the index's own searchKnn taken one at a
      time; q/s, p50 and p99 latency of a call.
  leg 3, host queries in place or staged: 1250- and 10 000-query submissions from page-locked, device-mapped buffers, gathered in
      place over the host link (the queue's choice for such buffers) against staging into the queue's slab (HS_QUEUE_IN_PLACE=0, read
      when a queue is created; pageable sources, as in leg 1, are always staged).

Every queue answer of the warm-up is compared with the direct one, byte for byte.  Output: the log on stdout.
"""
import argparse
import collections
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from bench import prepare_cached  # noqa: E402
from hsutil import headline_data, load_product  # noqa: E402

N, D, NQ, K, NB, S = 1_000_000, 128, 10_000, 10, 8, 16


def log(*a):
    print(*a, flush=True)


def clients_binary():
    out_dir = os.path.join(ROOT, "tools_out")
    exe = os.path.join(out_dir, "search_queue_clients")
    src = os.path.join(ROOT, "tools", "search_queue_clients.cpp")
    if not os.path.exists(exe) or os.path.getmtime(exe) < os.path.getmtime(src):
        os.makedirs(out_dir, exist_ok=True)
        lib_dir = os.path.join(ROOT, "hnsw-slim_amd")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-pthread", src, "-o", exe, "-L" + lib_dir, "-lhnsw_slim_amd", "-Wl,-rpath,$ORIGIN/../hnsw-slim_amd"])
    return exe


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ef", type=int, default=70)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batches", type=int, default=40, help="10 000-query equivalents per timed window")
    ap.add_argument("--calls", type=int, default=2000, help="leg 2: searchKnn calls per client thread (divided by the thread count above 8)")
    ap.add_argument("--legs", default="1,2,3", help="which legs to time; 1a / 1b / 1c name one part of leg 1 (for a run under a profiler)")
    ap.add_argument("--index-dir", default="", help="index files of bench.py --index-dir instead of the user cache directory")
    args = ap.parse_args()
    legs = set(args.legs.split(","))
    if "1" in legs:
        legs |= {"1a", "1b", "1c"}
    import torch
    torch.cuda.init()   # (torch's bundled HIP runtime opens the device before the product's does, as in bench.py)
    hs = load_product()
    assert hs.device_count() > 0, "no HIP device: this tool measures, it does not fall back"
    idir = args.index_dir or prepare_cached(N, D, 1, hs)[0]
    log(f"index: {os.path.basename(idir)}")
    spath = os.path.join(idir, "slim.bin")
    ix = hs.Index(spath, hs.HS_KIND_SLIM, D, hs.HS_METRIC_L2)
    ix.set_ef(args.ef)
    sets = [headline_data(NQ, D, 456 + b) for b in range(NB)]
    ref = [ix.search_ids(q, K)["labels"] for q in sets]
    log(f"ef {args.ef}, k {K}; kernel {ix.last_kernel()}; plan split at 10 000 queries: {hs.debug_search_plan(hs.debug_plan_input(ix, K, NQ))['split']}, "
        f"at 1250: {hs.debug_search_plan(hs.debug_plan_input(ix, K, 1250))['split']}")
    streams = [torch.cuda.Stream() for _ in range(S)]
    q_pin = [hs.PinnedArray((NQ, D), np.float32) for _ in range(NB)]
    for b in range(NB):
        q_pin[b].a[:] = sets[b]
    out_pin = [hs.PinnedArray((NQ, K), np.uint32) for _ in range(S)]

    def async_leg(bsz, check=False):
        """hs_search_batch_async: `args.batches` x 10 000 queries as bsz-query batches on 16 streams -> q/s"""
        per = NQ // bsz
        total = args.batches * per
        last = [None] * S
        t0 = time.perf_counter()
        for j in range(total):
            s = j % S
            if last[s] is not None:
                ix.check(streams[s].cuda_stream)   # the stream's staging buffers are free again once it has drained
                if check:
                    b, p = last[s]
                    assert np.array_equal(out_pin[s].a[:bsz], ref[b][p * bsz:(p + 1) * bsz])
            b, p = (j // per) % NB, j % per
            ix.search_ids_async(q_pin[b].a[p * bsz:(p + 1) * bsz], K, out_pin[s].a[:bsz], streams[s].cuda_stream)
            last[s] = (b, p)
        for s in range(S):
            if last[s] is not None:
                ix.check(streams[s].cuda_stream)
        return total * bsz / (time.perf_counter() - t0)

    def queue_leg(sq, bsz, source, check=False):
        """the queue: the same work as bsz-query host submissions, NQ // bsz per launch -> q/s"""
        per = NQ // bsz
        groups = collections.deque()
        depth = sq_slots[id(sq)]

        def reap():
            for (b, p), t in groups.popleft():
                r = sq.wait(t)
                if check:
                    assert np.array_equal(r["labels"], ref[b][p * bsz:(p + 1) * bsz])

        t0 = time.perf_counter()
        for g in range(args.batches):
            b = g % NB
            group = [((b, p), sq.submit(source[b][p * bsz:(p + 1) * bsz])) for p in range(per)]
            sq.flush()
            groups.append(group)
            if len(groups) >= depth:
                reap()
        while groups:
            reap()
        return args.batches * NQ / (time.perf_counter() - t0)

    sq_slots = {}

    def make_queue(slots, in_place=False):
        os.environ["HS_QUEUE_IN_PLACE"] = "1" if in_place else "0"
        sq = hs.SearchQueue(ix, K, hs.HS_MODE_SLIM_IDS, max_queries=NQ, slots=slots)
        os.environ.pop("HS_QUEUE_IN_PLACE")
        sq_slots[id(sq)] = slots
        return sq

    rows = collections.OrderedDict()

    def timed(name, fn, rnd):
        v = fn()
        rows.setdefault(name, []).append(v)
        log(f"round {rnd} {name}: {v / 1e6:.3f} M q/s")

    pageable = sets
    pinned = [p.a for p in q_pin]
    if legs & {"1a", "1b", "1c", "3"}:
        q2, q4 = make_queue(2), make_queue(4)
        q2_in = make_queue(2, in_place=True)
        log(f"queue device bytes: slots 2: {q2.info()['device_bytes'] / 2**20:.1f} MiB, slots 4: {q4.info()['device_bytes'] / 2**20:.1f} MiB")
        for bsz in (1250, 2500, NQ):   # warm every shape and check every answer
            async_leg(bsz, check=True)
            for sq in (q2, q4):
                queue_leg(sq, bsz, pageable, check=True)
            queue_leg(q2, bsz, pinned, check=True)
            queue_leg(q2_in, bsz, pinned, check=True)
        log("warm-up: every answer of every leg equals the direct search, byte for byte")
        for rnd in range(args.rounds):
            for bsz in (1250, 2500):
                if "1a" in legs:
                    timed(f"1a async {bsz} x16 streams", lambda: async_leg(bsz), rnd)
                if "1b" in legs:
                    timed(f"1b queue {bsz} x{NQ // bsz}/launch slots 2", lambda: queue_leg(q2, bsz, pageable), rnd)
                    timed(f"1b queue {bsz} x{NQ // bsz}/launch slots 4", lambda: queue_leg(q4, bsz, pageable), rnd)
            if "1c" in legs:
                timed("1c async 10000 x16 streams", lambda: async_leg(NQ), rnd)
            if "3" in legs:
                for bsz in (1250, NQ):
                    timed(f"3 queue {bsz} pinned source, staged", lambda: queue_leg(q2, bsz, pinned), rnd)
                    timed(f"3 queue {bsz} pinned source, in place", lambda: queue_leg(q2_in, bsz, pinned), rnd)
        for sq in (q2, q4, q2_in):
            sq.close()
        med = {k_: float(np.median(v)) for k_, v in rows.items()}
        log("\nleg | M q/s median (rounds) | spread of the rounds")
        for name, v in rows.items():
            log(f"{name} | {np.median(v) / 1e6:.3f} ({', '.join(f'{x / 1e6:.3f}' for x in v)}) | {(max(v) - min(v)) / np.median(v) * 100:.1f} %")
        if "1" in legs:
            c = med["1c async 10000 x16 streams"]
            for bsz in (1250, 2500):
                a = med[f"1a async {bsz} x16 streams"]
                for slots in (2, 4):
                    b = med[f"1b queue {bsz} x{NQ // bsz}/launch slots {slots}"]
                    log(f"{bsz}-query submissions, slots {slots}: (b)/(a) = {b / a:.3f}, (b)/(c) = {b / c:.3f} (goal >= 0.90: {'met' if b / c >= 0.9 else 'not met'}); "
                        f"(a)/(c) = {a / c:.3f}")
    if "2" in legs:
        exe = clients_binary()
        qf = os.path.join(ROOT, "tools_out", "search_queue_clients_q.f32")
        sets[0].tofile(qf)
        res = collections.OrderedDict()
        for rnd in range(args.rounds):
            for threads in (1, 8, 64):
                calls = max(args.calls * min(threads, 8) // threads, 100)
                for mode in ("plain", "queue"):
                    out = subprocess.run([exe, "slim", spath, str(D), qf, str(NQ), str(K), str(args.ef), str(threads), str(calls), mode],
                                         capture_output=True, text=True, timeout=600)
                    assert out.returncode == 0, out.stdout + out.stderr
                    r = json.loads(out.stdout.strip().splitlines()[-1])
                    res.setdefault((threads, mode), []).append(r)
                    log(f"round {rnd} leg 2 {threads} threads {mode}: {r['qps']:.0f} q/s, p50 {r['p50_us']:.0f} us, p99 {r['p99_us']:.0f} us, "
                        f"launches {r['launches']}, largest launch {r['largest_launch']}")
        log("\nthreads | entry | q/s median (rounds) | p50 us | p99 us | queue / plain")
        for threads in (1, 8, 64):
            base = np.median([r["qps"] for r in res[(threads, "plain")]])
            for mode in ("plain", "queue"):
                rs = res[(threads, mode)]
                qps = [r["qps"] for r in rs]
                log(f"{threads} | {mode} | {np.median(qps):.0f} ({', '.join(f'{x:.0f}' for x in qps)}) | {np.median([r['p50_us'] for r in rs]):.0f} | "
                    f"{np.median([r['p99_us'] for r in rs]):.0f} | {np.median(qps) / base:.2f}x")
        rows["leg2"] = {f"{t}_{m}": v for (t, m), v in res.items()}
    log("RESULT " + json.dumps(dict(ef=args.ef, rows=rows)))
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)
