#!/usr/bin/env python3
"""narrow_rows_bench.py -- what the u8 / fp16 row formats (hs_index_set_row_format) do to the flat kernel's speed on the bench's
own workload: the cached 1M x 128 index and query seeds of bench.py, k = 10, ef = 70, formats f32 / u8 / f16 on the SAME loaded
index in ONE process, alternated f32, u8, f16, f32, u8, f16, ... for three rounds after every format has been warmed.

Per format and round:
  (a) HIP-event time of one 10 000-query search_ids_dev launch group on device-resident queries, median of 20;
  (b) q/s of 2000 batches on 16 streams through hs_search_batch_async with page-locked buffers -- the way bench.py times `value`
      (every batch's labels consumed and checked before its output buffer is reused);
  (c) the labels of every query set equal to the f32 format's (checksum per batch, label by label for the last batch per stream).
The comparison is against the f32 format in the same process on the same index; the spread of its three rounds is the noise.

Default: runs the measurement and then, as child processes with a time limit each, the same short workload under
`rocprofv3 --kernel-trace --stats` and under `rocprofv3 --pmc FETCH_SIZE`, then `--pmc WRITE_SIZE` (counters in runs of their own,
and one counter per run: the pair in one pass is refused on gfx950, "exceeds the capabilities of the hardware to collect"); a step
that fails ends the sequence.  `--step measure|short` runs one step in this process (short: 5 launches per format, for the profiler).
Output: the log on stdout, CSV summaries of the two profiler runs under --out.
"""
import argparse
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
from bench import checksum, ground_truth, prepare_cached, recall_at_k  # noqa: E402
from hsutil import headline_data, load_product  # noqa: E402

N, D, NQ, K = 1_000_000, 128, 10_000, 10


def log(*a):
    print(*a, flush=True)


def load(hs, torch, ef):
    idir, t_build, _ = prepare_cached(N, D, 1, hs)
    log(f"index: {os.path.basename(idir)} " + (f"(built in {t_build:.0f} s)" if t_build else "(cached)"))
    ix = hs.Index(os.path.join(idir, "slim.bin"), hs.HS_KIND_SLIM, D, hs.HS_METRIC_L2)
    ix.set_ef(ef)
    return ix, idir


def step_measure(args):
    import torch
    torch.cuda.init()   # (torch's bundled HIP runtime opens the device before the product's does, as in bench.py)
    hs = load_product()
    dev = torch.device("cuda", 0)
    ix, idir = load(hs, torch, args.ef)
    fmts = [("f32", hs.HS_ROWS_F32), ("u8", hs.HS_ROWS_U8), ("f16", hs.HS_ROWS_F16)]
    NB, S = 8, args.streams
    qsets = [headline_data(NQ, D, 456 + b) for b in range(NB)]
    q_dev = [torch.from_numpy(q).to(dev) for q in qsets]
    streams = [torch.cuda.Stream(device=dev) for _ in range(S)]
    events = [torch.cuda.Event() for _ in range(S)]
    q_pin = [hs.PinnedArray((NQ, D), np.float32) for _ in range(NB)]
    for b in range(NB):
        q_pin[b].a[:] = qsets[b]
    out_pin = [hs.PinnedArray((NQ, K), np.uint32) for _ in range(S)]
    base_bytes = ix.info()["device_bytes"]

    # reference answers: the f32 format's labels of every query set (and its recall, so that the operating point is on record)
    ref, t_conv = [], {}
    lab = torch.empty((NQ, K), dtype=torch.int32, device=dev)
    for b in range(NB):
        ix.search_ids_dev(q_dev[b], K, lab)
        ix.check()
        ref.append(np.sort(lab.cpu().numpy().view(np.uint32), axis=1))
    assert ix.last_kernel() == "hs::flat_kernel"
    base_t = torch.from_numpy(np.load(os.path.join(idir, "base.npy"))).to(dev)
    gt = ground_truth(torch, base_t, q_dev[0], K, hs)
    del base_t
    log(f"ef={args.ef} k={K}: recall@10 {recall_at_k(ref[0], gt):.4f} on query set 0; index {base_bytes / 2**20:.0f} MiB on the device")
    ref_sums = [checksum(r) for r in ref]
    # warm every format (conversion time on record), labels of every query set against f32's
    for name, f in fmts:
        t0 = time.perf_counter()
        ix.set_row_format(f)
        t_conv[name] = time.perf_counter() - t0
        for b in range(NB):
            ix.search_ids_dev(q_dev[b], K, lab)
            ix.check()
            assert np.array_equal(np.sort(lab.cpu().numpy().view(np.uint32), axis=1), ref[b]), f"{name}: labels of query set {b} differ from f32's"
        log(f"{name}: set_row_format {t_conv[name] * 1e3:.1f} ms, device_bytes +{(ix.info()['device_bytes'] - base_bytes) / 2**20:.0f} MiB, "
            f"kernel {ix.last_kernel()}, labels of {NB} x {NQ} queries == f32's")

    def single_launch():
        ts = []
        for i in range(20):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ix.search_ids_dev(q_dev[i % NB], K, lab)
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        ix.check()
        return float(np.median(ts)), float(min(ts))

    def pipelined(batches):
        last_on = [-1] * S

        def consume(s, full=False):
            if last_on[s] < 0:
                return
            events[s].synchronize()
            if full:
                assert np.array_equal(np.sort(out_pin[s].a, axis=1), ref[last_on[s]]), "labels differ from the f32 format's"
            else:
                assert checksum(out_pin[s].a) == ref_sums[last_on[s]], "labels differ from the f32 format's"
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

    rows = {name: dict(launch_ms=[], launch_min_ms=[], qps=[]) for name, _ in fmts}
    for name, f in fmts:   # warm the pipelined path of every format too
        ix.set_row_format(f)
        pipelined(200)
    for rnd in range(args.rounds):
        for name, f in fmts:
            ix.set_row_format(f)
            med, mn = single_launch()
            qps = pipelined(args.batches)
            rows[name]["launch_ms"].append(med); rows[name]["launch_min_ms"].append(mn); rows[name]["qps"].append(qps)
            log(f"round {rnd} {name:>3}: single launch {med:.4f} ms (min {mn:.4f}), pipelined {qps / 1e6:.3f} M q/s over {args.batches} batches on {S} streams, "
                f"labels == f32's, kernel {ix.last_kernel()}")
    log("\nformat | single 10k launch, ms (median of 20; rounds) | pipelined M q/s (rounds) | vs f32 (median of rounds)")
    f32_l, f32_q = np.median(rows["f32"]["launch_ms"]), np.median(rows["f32"]["qps"])
    for name, _ in fmts:
        l, q = rows[name]["launch_ms"], rows[name]["qps"]
        log(f"{name:>6} | {np.median(l):.4f} ({', '.join(f'{x:.4f}' for x in l)}) | {np.median(q) / 1e6:.3f} ({', '.join(f'{x / 1e6:.3f}' for x in q)}) | "
            f"launch x{f32_l / np.median(l):.3f}, q/s x{np.median(q) / f32_q:.3f}")
    sl, sq = rows["f32"]["launch_ms"], rows["f32"]["qps"]
    log(f"noise (spread of the f32 rounds): launch {(max(sl) - min(sl)) / np.median(sl) * 100:.2f} %, q/s {(max(sq) - min(sq)) / np.median(sq) * 100:.2f} %")
    log("RESULT " + json.dumps(dict(ef=args.ef, rows=rows, set_row_format_s=t_conv)))


def step_short(args):
    """Five 10k launches per format on one stream: what the profiler runs look at."""
    import torch
    torch.cuda.init()   # (torch's bundled HIP runtime opens the device before the product's does, as in bench.py)
    hs = load_product()
    dev = torch.device("cuda", 0)
    ix, _ = load(hs, torch, args.ef)
    q = torch.from_numpy(headline_data(NQ, D, 456)).to(dev)
    lab = torch.empty((NQ, K), dtype=torch.int32, device=dev)
    for name, f in (("f32", hs.HS_ROWS_F32), ("u8", hs.HS_ROWS_U8), ("f16", hs.HS_ROWS_F16)):
        ix.set_row_format(f)
        for _ in range(5):
            ix.search_ids_dev(q, K, lab)
        ix.check()
        log(f"{name}: 5 launches, kernel {ix.last_kernel()}")


def summarize(d, pattern, dest):
    hits = sorted(glob.glob(os.path.join(d, "**", pattern), recursive=True))
    if hits:
        shutil.copy(hits[0], dest)
        log(f"{dest}:")
        for line in open(dest).read().splitlines()[:12]:
            log("  " + line)
    return bool(hits)


def pmc_summary(dirs, dest):
    """Mean FETCH_SIZE / WRITE_SIZE per launch of each flat kernel entry point out of the counter_collection CSVs."""
    import csv
    hits = [h for d in dirs for h in sorted(glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True))[:1]]
    if len(hits) != len(dirs):
        return False
    acc = {}
    for row in [r for h in hits for r in csv.DictReader(open(h))]:
        kern = row.get("Kernel_Name", "")
        if "flat_kernel" not in kern:
            continue
        name = "flat_kernel_u8" if "flat_kernel_u8" in kern else "flat_kernel_f16" if "flat_kernel_f16" in kern else "flat_kernel"
        key = (name, row.get("Counter_Name", ""))
        s = acc.setdefault(key, [0.0, set()])
        s[0] += float(row.get("Counter_Value", 0) or 0)
        s[1].add(row.get("Dispatch_Id", ""))
    with open(dest, "w") as f:
        f.write("kernel,counter,launches,mean_per_launch\n")
        for (name, ctr), (tot, ids) in sorted(acc.items()):
            f.write(f"{name},{ctr},{len(ids)},{tot / max(len(ids), 1):.1f}\n")
    log(f"{dest}:")
    for line in open(dest).read().splitlines():
        log("  " + line)
    return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=("all", "measure", "short"), default="all")
    ap.add_argument("--skip-measure", action="store_true", help="with --step all: only the profiler runs")
    ap.add_argument("--ef", type=int, default=70)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batches", type=int, default=2000)
    ap.add_argument("--streams", type=int, default=16)
    ap.add_argument("--out", default="tools_out/narrow_rows")
    args = ap.parse_args()
    if args.step == "measure":
        return step_measure(args)
    if args.step == "short":
        return step_short(args)
    os.makedirs(args.out, exist_ok=True)
    me = [sys.executable, os.path.abspath(__file__), "--ef", str(args.ef)]
    tr, pf, pw = (os.path.join(args.out, d) for d in ("trace", "pmc_fetch", "pmc_write"))
    steps = [
        (["timeout", "-k", "10", "900"] + me + ["--step", "measure", "--rounds", str(args.rounds), "--batches", str(args.batches), "--streams", str(args.streams)], None),
        (["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--stats", "-d", tr, "--output-format", "csv", "--"] + me + ["--step", "short"],
         lambda: summarize(tr, "*kernel_stats.csv", os.path.join(args.out, "kernel_stats.csv"))),
        (["timeout", "-k", "10", "300", "rocprofv3", "--pmc", "FETCH_SIZE", "-d", pf, "--output-format", "csv", "--"] + me + ["--step", "short"], None),
        (["timeout", "-k", "10", "300", "rocprofv3", "--pmc", "WRITE_SIZE", "-d", pw, "--output-format", "csv", "--"] + me + ["--step", "short"],
         lambda: pmc_summary([pf, pw], os.path.join(args.out, "pmc_stats.csv"))),
    ]
    for cmd, after in steps[1:] if args.skip_measure else steps:
        log("\n$ " + " ".join(os.path.relpath(c, ROOT) if c == os.path.abspath(__file__) else "python" if c == sys.executable else c for c in cmd))
        rc = subprocess.call(cmd)
        if rc != 0:
            log(f"step ended with status {rc}: nothing more is started")
            return rc
        if after and not after():
            log("(no profiler output found)")
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)
