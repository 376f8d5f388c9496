#!/usr/bin/env python3
"""flat_ab.py -- two builds of the library against each other on the bench's own workload (the cached 1M x 128 index and query
seeds of bench.py, k = 10, fp32 rows, hs::flat_kernel): library A (the baseline, e.g. built from the parent commit in a scratch
worktree) and library B (the build under test), alternated A, B, A, B, ... for --rounds rounds, EVERY round in a fresh child
process (HS_LIB selects the library), so that neither side inherits the other's clocks, caches or allocator state.

Per round and library:
  (a) HIP-event time of one 10 000-query search_ids_dev launch group on device-resident queries, median of 20;
  (b) q/s of --batches batches on --streams streams through hs_search_batch_async with page-locked buffers -- the way bench.py times
      `value` -- every batch's labels consumed and checked (checksum per batch, label by label for the last batch per stream);
  (c) a checksum of the labels of every query set: all rounds of both libraries must agree.
A gain counts only if the ranges do not overlap: the worst round of B better than the best round of A, in (a) and in (b).

--ef-list 32,128,256,512 --single-only : the regression guard over the other slot counts (S = 1, 2, 4, 8), (a) only; a shape
    counts as slower only beyond the spread of A's own rounds.
--bench-runs N : bench.py --gpus 1 (its default steps) N times per library, alternated; `value` per run.
--profile      : per library, each step a child process under its own time limit, the program after `--`:
    rocprofv3 --kernel-trace --stats on 5 launches, and -- in a run of its own, no tracing with it --
    rocprofv3 --pmc SQ_INSTS_SALU SQ_INSTS_VALU SQ_WAVES; reported per query and per distance evaluation.
A step that fails ends the sequence.  Output: the log on stdout, profiler CSV summaries under --out.
"""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N, D, NQ, K, NB = 1_000_000, 128, 10_000, 10, 8


def log(*a):
    print(*a, flush=True)


def open_index(ef):
    import torch
    torch.cuda.init()   # (torch's bundled HIP runtime opens the device before the product's does, as in bench.py)
    from bench import prepare_cached
    from hsutil import load_product
    hs = load_product()
    idir, _, _ = prepare_cached(N, D, 1, hs)
    ix = hs.Index(os.path.join(idir, "slim.bin"), hs.HS_KIND_SLIM, D, hs.HS_METRIC_L2)
    ix.set_ef(ef)
    return torch, hs, ix


def step_measure(args):
    from bench import checksum
    from hsutil import headline_data
    torch, hs, ix = open_index(args.ef)
    dev = torch.device("cuda", 0)
    S = args.streams
    qsets = [headline_data(NQ, D, 456 + b) for b in range(NB)]
    q_dev = [torch.from_numpy(q).to(dev) for q in qsets]
    lab = torch.empty((NQ, K), dtype=torch.int32, device=dev)
    ref = []
    for b in range(NB):   # (also the warm-up of the single-launch path)
        ix.search_ids_dev(q_dev[b], K, lab)
        ix.check()
        ref.append(np.sort(lab.cpu().numpy().view(np.uint32), axis=1))
    assert ix.last_kernel() == "hs::flat_kernel", ix.last_kernel()
    ref_sums = [checksum(r) for r in ref]
    ts = []
    for i in range(20):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ix.search_ids_dev(q_dev[i % NB], K, lab)
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    ix.check()
    res = dict(ef=args.ef, lib=hs.LIB_PATH, launch_ms=float(np.median(ts)), launch_min_ms=float(min(ts)), sums=[int(s) for s in ref_sums])
    if not args.single_only:
        streams = [torch.cuda.Stream(device=dev) for _ in range(S)]
        events = [torch.cuda.Event() for _ in range(S)]
        q_pin = [hs.PinnedArray((NQ, D), np.float32) for _ in range(NB)]
        for b in range(NB):
            q_pin[b].a[:] = qsets[b]
        out_pin = [hs.PinnedArray((NQ, K), np.uint32) for _ in range(S)]

        def pipelined(batches):
            last_on = [-1] * S

            def consume(s, full=False):
                if last_on[s] < 0:
                    return
                events[s].synchronize()
                if full:
                    assert np.array_equal(np.sort(out_pin[s].a, axis=1), ref[last_on[s]]), "labels differ from the single-launch path's"
                else:
                    assert checksum(out_pin[s].a) == ref_sums[last_on[s]], "labels differ from the single-launch path's"
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for j in range(batches):
                s = j % S
                consume(s)
                ix.search_ids_async(q_pin[j % NB].a, K, out_pin[s].a, streams[s].cuda_stream)
                events[s].record(streams[s])
                last_on[s] = j % NB
            for s in range(S):
                consume(s, full=True)
                ix.check(streams[s].cuda_stream)
            return batches * NQ / (time.perf_counter() - t0)
        pipelined(200)   # warm
        res["qps"] = pipelined(args.batches)
    log("RESULT " + json.dumps(res))


def step_short(args):
    """Five 10k launches on one stream: what the profiler runs look at; the traversal counters of one launch for the per-evaluation figures."""
    from hsutil import headline_data
    torch, hs, ix = open_index(args.ef)
    dev = torch.device("cuda", 0)
    q = torch.from_numpy(headline_data(NQ, D, 456)).to(dev)
    lab = torch.empty((NQ, K), dtype=torch.int32, device=dev)
    stats = torch.zeros((NQ, 4), dtype=torch.int32, device=dev)
    for _ in range(5):
        ix.search_ids_dev(q, K, lab, d_stats=stats)
    ix.check()
    st = stats.cpu().numpy().view(np.uint32)
    log("RESULT " + json.dumps(dict(launches=5, nq=NQ, kernel=ix.last_kernel(), n_dist=int(st[:, 0].sum()), n_hops=int(st[:, 1].sum()))))


def child(lib, argv, limit, prefix=()):
    """One step as a child process with its own time limit; returns (status, parsed RESULT line or None)."""
    cmd = ["timeout", "-k", "10", str(limit)] + list(prefix) + [sys.executable, os.path.abspath(__file__)] + argv
    p = subprocess.run(cmd, env=dict(os.environ, HS_LIB=lib), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    res = None
    for line in p.stdout.splitlines():
        if line.startswith("RESULT "):
            res = json.loads(line[7:])
    if p.returncode != 0 or res is None:
        log(p.stdout[-3000:])
    return p.returncode, res


def spread(v):
    return (max(v) - min(v)) / float(np.median(v)) * 100


def run_ab(args, ef, single_only):
    rows = {"A": [], "B": []}
    for rnd in range(args.rounds):
        for tag, lib in (("A", args.a), ("B", args.b)):
            argv = ["--step", "measure", "--ef", str(ef), "--batches", str(args.batches), "--streams", str(args.streams)] + (["--single-only"] if single_only else [])
            rc, r = child(lib, argv, 600)
            if rc != 0 or r is None:
                log(f"round {rnd} {tag}: step ended with status {rc}: nothing more is started")
                return None
            rows[tag].append(r)
            log(f"ef={ef} round {rnd} {tag}: single launch {r['launch_ms']:.4f} ms (min {r['launch_min_ms']:.4f})" +
                ("" if single_only else f", pipelined {r['qps'] / 1e6:.3f} M q/s over {args.batches} batches on {args.streams} streams, labels checked"))
    sums = {tuple(r["sums"]) for t in rows for r in rows[t]}
    la, lb = [r["launch_ms"] for r in rows["A"]], [r["launch_ms"] for r in rows["B"]]
    log(f"ef={ef}: label checksums of {NB} x {NQ} queries: " + ("identical in every round of both libraries" if len(sums) == 1 else "DIFFER between rounds / libraries"))
    log(f"ef={ef} single 10k launch, ms: A {', '.join(f'{x:.4f}' for x in la)} | B {', '.join(f'{x:.4f}' for x in lb)} | "
        f"median x{np.median(la) / np.median(lb):.4f}, spread A {spread(la):.2f} % B {spread(lb):.2f} %, "
        f"worst B {'<' if max(lb) < min(la) else '>='} best A: {'ranges do not overlap, B faster' if max(lb) < min(la) else 'no separated gain'}"
        f"{'; B SLOWER beyond the spread of A' if min(lb) > max(la) else ''}")
    ok = len(sums) == 1
    if not single_only:
        qa, qb = [r["qps"] for r in rows["A"]], [r["qps"] for r in rows["B"]]
        log(f"ef={ef} pipelined M q/s: A {', '.join(f'{x / 1e6:.3f}' for x in qa)} | B {', '.join(f'{x / 1e6:.3f}' for x in qb)} | "
            f"median x{np.median(qb) / np.median(qa):.4f}, spread A {spread(qa):.2f} % B {spread(qb):.2f} %, "
            f"worst B {'>' if min(qb) > max(qa) else '<='} best A: {'ranges do not overlap, B faster' if min(qb) > max(qa) else 'no separated gain'}")
    log("RESULT_AB " + json.dumps(dict(ef=ef, rows=rows)))
    return ok


def run_bench(args):
    vals = {"A": [], "B": []}
    for rnd in range(args.bench_runs):
        for tag, lib in (("A", args.a), ("B", args.b)):
            cmd = ["timeout", "-k", "10", "900", sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"]
            p = subprocess.run(cmd, env=dict(os.environ, HS_LIB=lib), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            val = None
            for line in p.stdout.splitlines():
                if line.startswith("{") and '"value"' in line:
                    val = json.loads(line)["value"]
            if p.returncode != 0 or val is None:
                log(p.stdout[-3000:])
                log(f"bench run {rnd} {tag} ended with status {p.returncode}: nothing more is started")
                return False
            vals[tag].append(val)
            log(f"bench.py --gpus 1, run {rnd} {tag}: value {val:.1f}")
    a, b = vals["A"], vals["B"]
    log(f"bench.py value: A {', '.join(f'{x:.1f}' for x in a)} | B {', '.join(f'{x:.1f}' for x in b)} | median x{np.median(b) / np.median(a):.4f}, "
        f"worst B {'>' if min(b) > max(a) else '<='} best A: {'ranges do not overlap, B faster' if min(b) > max(a) else 'no separated gain'}")
    return True


def run_profile(args):
    os.makedirs(args.out, exist_ok=True)
    for tag, lib in (("A", args.a), ("B", args.b)):
        tr, pm = os.path.join(args.out, f"trace_{tag}"), os.path.join(args.out, f"pmc_{tag}")
        short = ["--step", "short", "--ef", str(args.ef)]
        rc, r = child(lib, short, 300, prefix=["rocprofv3", "--kernel-trace", "--stats", "-d", tr, "--output-format", "csv", "--"])
        if rc != 0:
            log(f"{tag}: kernel-trace step ended with status {rc}: nothing more is started")
            return False
        hits = sorted(glob.glob(os.path.join(tr, "**", "*kernel_stats.csv"), recursive=True))
        if hits:
            dest = os.path.join(args.out, f"kernel_stats_{tag}.csv")
            shutil.copy(hits[0], dest)
            log(f"{tag} ({lib}) rocprofv3 --kernel-trace --stats, 5 launches of {NQ} queries at ef={args.ef}:")
            for line in open(dest).read().splitlines()[:8]:
                log("  " + line)
        rc, r = child(lib, short, 300, prefix=["rocprofv3", "--pmc", "SQ_INSTS_SALU", "SQ_INSTS_VALU", "SQ_WAVES", "-d", pm, "--output-format", "csv", "--"])
        if rc != 0 or r is None:
            log(f"{tag}: pmc step ended with status {rc}: nothing more is started")
            return False
        hits = sorted(glob.glob(os.path.join(pm, "**", "*counter_collection.csv"), recursive=True))
        tot, disp = {}, set()
        for row in [x for h in hits[:1] for x in csv.DictReader(open(h))]:
            if "flat_kernel" in row.get("Kernel_Name", ""):
                tot[row["Counter_Name"]] = tot.get(row["Counter_Name"], 0.0) + float(row.get("Counter_Value", 0) or 0)
                disp.add(row.get("Dispatch_Id", ""))
        nq_total, per_q_dist = r["launches"] * r["nq"], r["n_dist"] / r["nq"]
        if not tot:
            log(f"{tag}: (no counter output found)")
            continue
        salu, valu = tot.get("SQ_INSTS_SALU", 0) / nq_total, tot.get("SQ_INSTS_VALU", 0) / nq_total
        log(f"{tag} rocprofv3 --pmc SQ_INSTS_SALU SQ_INSTS_VALU SQ_WAVES ({len(disp)} hs::flat_kernel dispatches = {r['launches']} searches of {r['nq']} queries, "
            f"{int(tot.get('SQ_WAVES', 0))} waves): per query {salu:.0f} SALU + {valu:.0f} VALU; per distance evaluation ({per_q_dist:.0f} per query) "
            f"{salu / per_q_dist:.1f} SALU + {valu / per_q_dist:.1f} VALU")
    return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--a", help="library A: the baseline (path of a libhnsw_slim_amd.so)")
    ap.add_argument("--b", help="library B: the build under test")
    ap.add_argument("--step", choices=("ab", "measure", "short"), default="ab")
    ap.add_argument("--ef", type=int, default=70)
    ap.add_argument("--ef-list", default="", help="comma-separated ef values instead of --ef")
    ap.add_argument("--single-only", action="store_true")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batches", type=int, default=2000)
    ap.add_argument("--streams", type=int, default=16)
    ap.add_argument("--bench-runs", type=int, default=0)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--skip-ab", action="store_true", help="only --bench-runs / --profile")
    ap.add_argument("--out", default="tools_out/flat_ab")
    args = ap.parse_args()
    if args.step == "measure":
        return step_measure(args)
    if args.step == "short":
        return step_short(args)
    if not args.a or not args.b:
        ap.error("--a and --b are required")
    args.a, args.b = os.path.abspath(args.a), os.path.abspath(args.b)
    log(f"A = {args.a}\nB = {args.b}")
    if not args.skip_ab:
        for ef in ([int(x) for x in args.ef_list.split(",")] if args.ef_list else [args.ef]):
            if run_ab(args, ef, args.single_only) is None:
                return 1
    if args.bench_runs and not run_bench(args):
        return 1
    if args.profile and not run_profile(args):
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)
