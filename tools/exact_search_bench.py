#!/usr/bin/env python3
"""exact_search_bench.py -- the exact scan over a resident index (hs_index_exact_search_dev) on the bench's own workload: the
cached 1M x 128 index and query seed of bench.py, 10 000 queries, k = 10.  ONE loaded index in ONE process.

  1. unfiltered, fp32 rows, against hs_brute_force_dev on a second fp32 copy of the same rows: alternated old, new, old, new, ...
     for three rounds after both have been warmed, HIP-event time per call, median of `--reps`; outputs compared bit for bit.
     The spread of the old entry's own rounds is the noise, and the margin the new scan is held to.
  2. the same scan over the u8 copy of the rows (hs_index_set_row_format), same bits.
  3. filters that allow 50 % / 10 % / 1 % of the ids, eight different filters per selectivity: the scan with the queries grouped by
     filter (tiles of one filter: a tile skips what its filter excludes) and with the filters interleaved (every tile holds all
     eight), and recall@10 of hs_search_batch_filter_set at the bench's ef against the exact answer.
Output: the log on stdout.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from bench import prepare_cached  # noqa: E402
from hsutil import headline_data, load_product  # noqa: E402

N, D, NQ, K, PER = 1_000_000, 128, 10_000, 10, 8
SELECT = (0.5, 0.1, 0.01)


def log(*a):
    print(*a, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ef", type=int, default=70)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--index-dir", default="", help="index files of bench.py --index-dir instead of the user cache directory")
    args = ap.parse_args()
    import torch
    torch.cuda.init()   # (torch's bundled HIP runtime opens the device before the product's does, as in bench.py)
    hs = load_product()
    dev = torch.device("cuda", 0)
    idir = args.index_dir or prepare_cached(N, D, 1, hs)[0]
    log(f"index: {os.path.basename(idir)}")
    ix = hs.Index(os.path.join(idir, "slim.bin"), hs.HS_KIND_SLIM, D, hs.HS_METRIC_L2)
    ix.set_ef(args.ef)
    assert np.array_equal(ix.labels(), np.arange(N, dtype=np.uint64)), "the bench index labels its rows by index"
    q = headline_data(NQ, D, 456)
    dq = torch.from_numpy(q).to(dev)

    def outputs():
        return (torch.zeros((NQ, K), dtype=torch.int64, device=dev), torch.zeros((NQ, K), dtype=torch.float32, device=dev),
                torch.zeros(NQ, dtype=torch.int32, device=dev))

    def host(o):
        return dict(labels=o[0].cpu().numpy().view(np.uint64), dists=o[1].cpu().numpy(), cnt=o[2].cpu().numpy().view(np.uint32))

    def same(a, b, what):
        for key in ("labels", "dists", "cnt"):
            assert a[key].tobytes() == b[key].tobytes(), f"{what}: {key} differs"

    def timed(fn, reps):
        ts = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        ix.check()
        return float(np.median(ts)), float(min(ts))

    # ---- 1. unfiltered, fp32: the exhaustive scan over a second copy against the scan over the index's own rows -----------------
    base_t = torch.from_numpy(np.load(os.path.join(idir, "base.npy"))).to(dev)
    o_old, o_new = outputs(), outputs()
    old = lambda: hs.brute_force_dev(base_t, dq, K, o_old[0], o_old[1], d_counts=o_old[2])   # noqa: E731
    new = lambda: ix.exact_search_dev(dq, K, *o_new)                                         # noqa: E731
    old(); new(); ix.check()
    assert ix.last_kernel() == "hs::exact_scan_kernel"
    exact = host(o_new)
    same(host(o_old), exact, "fp32 scan against hs_brute_force_dev")
    log(f"unfiltered: outputs identical to hs_brute_force_dev's; second fp32 copy for the old entry: {base_t.numel() * 4 / 2**20:.0f} MiB, for the new one: none")
    rows = dict(old=[], new=[])
    for rnd in range(args.rounds):
        for side, fn in (("old", old), ("new", new)):
            med, mn = timed(fn, args.reps)
            rows[side].append(med)
            log(f"round {rnd} {side}: {med:.3f} ms per {NQ}-query call (median of {args.reps}, min {mn:.3f})")
    o, n = rows["old"], rows["new"]
    spread = (max(o) - min(o)) / np.median(o) * 100
    delta = (np.median(n) / np.median(o) - 1) * 100
    log(f"hs_brute_force_dev {np.median(o):.3f} ms ({', '.join(f'{x:.3f}' for x in o)}) | hs_index_exact_search_dev fp32 {np.median(n):.3f} ms "
        f"({', '.join(f'{x:.3f}' for x in n)}) | new / old {delta:+.2f} % | spread of the old entry's rounds {spread:.2f} % -> "
        + ("within the margin" if delta <= spread else "OUTSIDE the margin"))
    del base_t
    torch.cuda.empty_cache()

    # ---- 2. the u8 copy -----------------------------------------------------------------------------------------------------------
    ix.set_row_format(hs.HS_ROWS_U8)
    new(); ix.check()
    assert ix.last_kernel() == "hs::exact_scan_kernel_u8"
    same(exact, host(o_new), "u8 scan against the fp32 scan")
    u8_ms, u8_min = timed(new, args.reps)
    log(f"u8 rows: {u8_ms:.3f} ms per {NQ}-query call (median of {args.reps}, min {u8_min:.3f}), outputs identical to the fp32 scan's")
    ix.set_row_format(hs.HS_ROWS_F32)

    # ---- 3. filters -------------------------------------------------------------------------------------------------------------
    rng = np.random.default_rng(3)
    fs = hs.FilterSet.create(ix, len(SELECT) * PER)
    for s, p in enumerate(SELECT):
        fs.write(s * PER, (rng.random((PER, N)) < p).astype(np.uint8))
    filt = {}
    for s, p in enumerate(SELECT):
        inter = (s * PER + np.arange(NQ) % PER).astype(np.uint32)      # every tile of 8 holds all eight filters
        order = np.argsort(inter, kind="stable")                       # tiles of one filter
        dq_g, foq_g = torch.from_numpy(q[order]).to(dev), torch.from_numpy(inter[order].astype(np.int32)).to(dev)
        foq_i = torch.from_numpy(inter.astype(np.int32)).to(dev)
        og, oi = outputs(), outputs()
        grouped = lambda: ix.exact_search_dev(dq_g, K, *og, fs=fs, d_filter_of_query=foq_g)        # noqa: E731
        interleaved = lambda: ix.exact_search_dev(dq, K, *oi, fs=fs, d_filter_of_query=foq_i)      # noqa: E731
        grouped(); interleaved(); ix.check()
        eg, ei = host(og), host(oi)
        same(eg, {key: v[order] for key, v in ei.items()}, f"{p}: grouped against interleaved")
        g_ms, _ = timed(grouped, args.reps)
        i_ms, _ = timed(interleaved, args.reps)
        approx = ix.search_filter_set(q, K, fs, inter)
        hit = sum(len(np.intersect1d(approx["labels"][i, :approx["cnt"][i]], ei["labels"][i, :ei["cnt"][i]])) for i in range(NQ))
        recall = hit / max(int(ei["cnt"].sum()), 1)
        filt[str(p)] = dict(grouped_ms=g_ms, interleaved_ms=i_ms, recall=recall, kernel=ix.last_kernel())
        log(f"{p * 100:g} % allowed: exact scan {g_ms:.3f} ms grouped by filter, {i_ms:.3f} ms interleaved (per {NQ} queries, median of {args.reps}); "
            f"hs_search_batch_filter_set at ef = {args.ef} ({ix.last_kernel()}): recall@{K} {recall:.4f}")
    log("RESULT " + json.dumps(dict(ef=args.ef, unfiltered_ms=rows, u8_ms=u8_ms, filters=filt)))
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)
