#!/usr/bin/env python3
"""exact_screen_bench.py -- hs_index_exact_search_dev against hs_index_exact_search_screened_dev on the bench's rows and queries
(headline_data seeds 123 / 456: 1M x 128, 10 000 queries, k = 10).  ONE index in ONE process, both entries warmed, then alternated
old, new, old, new for three rounds; HIP-event time per call, median of `--reps`; outputs compared bit for bit before any timing.

  1. unfiltered over fp32 rows      2. unfiltered over the u8 copy      3. eight filters that allow 1 %, queries grouped by filter

With --q8 the comparison is instead hs_index_exact_search_screened_dev against hs_index_exact_search_q8_dev (byte queries, the integer
matrix cores: csrc/exact_screen_q8.hip) over the u8 copy of the same index, in the same process and the same alternation.  With --f16q
it is hs_index_exact_search_screened_dev against hs_index_exact_search_f16_dev (fp16 queries, the half-precision matrix cores:
csrc/exact_screen_f16q.hip) over the fp16 copy; the bench's integers 0 .. 255 are exact halves.  With --f8q it is
hs_index_exact_search_screened_dev against hs_index_exact_search_f8_dev (fp8 E4M3 queries, the fp8 matrix cores:
csrc/exact_screen_f8q.hip) over the fp8 copy of the bench's rows scaled by 1 / 8 and rounded to the nearest E4M3 value (0 .. 31.875 on a
grid of at most 2: both screens read the same rounded rows); always under the ring graph, since the cached index holds the unrounded rows.

The spread of the old entry's own rounds is the noise: a difference counts only where it lies outside it.  By default the index is the
bench's cached one; --ring puts the same rows under a ring graph instead (the exact entries read rows, labels and marks, never the
graph), which spares a fresh machine the HNSW build.  Output: the log on stdout.
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


def e4m3_of_bench(x):
    """(bytes, values): the bench's integers 0 .. 255, scaled by 1 / 8, as the nearest non-negative E4M3 byte and what it decodes to"""
    b = np.arange(0x7F)
    t = np.where(b >> 3 == 0, (b & 7) * 2.0 ** -9, (1 + (b & 7) / 8) * 2.0 ** ((b >> 3) - 7.0))
    lut = np.abs(np.arange(256)[:, None] / 8 - t[None, :]).argmin(1).astype(np.uint8)
    byt = lut[x.astype(np.int64)]
    return byt, t.astype(np.float32)[byt]


def log(*a):
    print(*a, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ring", action="store_true", help="the bench's rows under a ring graph: no HNSW build")
    ap.add_argument("--q8", action="store_true", help="the fp32 screen against the byte-query entry over u8 rows, nothing else")
    ap.add_argument("--f16q", action="store_true", help="the fp32 screen against the fp16-query entry over fp16 rows, nothing else")
    ap.add_argument("--f8q", action="store_true", help="the fp32 screen against the fp8-query entry over fp8 rows (ring graph), nothing else")
    ap.add_argument("--index-dir", default="", help="index files of bench.py --index-dir instead of the user cache directory")
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    hs = load_product()
    dev = torch.device("cuda", 0)
    if args.ring or args.f8q:
        ids = np.arange(N, dtype=np.uint32)
        base = headline_data(N, D, 123)
        ix = hs.Index.from_csr(hs.HS_KIND_SLIM, hs.HS_METRIC_L2, e4m3_of_bench(base)[1] if args.f8q else base, np.zeros(N, np.int32), np.arange(N + 1, dtype=np.uint64),
                               (ids + 1) % N, 0, 0)
        log("index: the bench's rows under a ring graph")
    else:
        idir = args.index_dir or prepare_cached(N, D, 1, hs)[0]
        ix = hs.Index(os.path.join(idir, "slim.bin"), hs.HS_KIND_SLIM, D, hs.HS_METRIC_L2)
        log(f"index: {os.path.basename(idir)}")
    q = headline_data(NQ, D, 456)

    def outputs():
        return (torch.zeros((NQ, K), dtype=torch.int64, device=dev), torch.zeros((NQ, K), dtype=torch.float32, device=dev),
                torch.zeros(NQ, dtype=torch.int32, device=dev))

    def timed(fn):
        ts = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        ix.check()
        return float(np.median(ts))

    result = {}

    def compare(name, dq, kernel, q8=None, f16=None, f8=None, **kw):
        o_old, o_new = outputs(), outputs()
        old = lambda: ix.exact_search_dev(dq, K, *o_old, **kw)            # noqa: E731
        new = lambda: ix.exact_search_screened_dev(dq, K, *o_new, **kw)   # noqa: E731
        if q8 is not None:   # the fp32 screen is the old side, the byte-query entry the new one
            old, new = new, lambda: ix.exact_search_q8_dev(q8, K, *o_old, **kw)   # noqa: E731
        if f16 is not None:   # likewise, the fp16-query entry the new side
            old, new = new, lambda: ix.exact_search_f16_dev(f16, K, *o_old, **kw)   # noqa: E731
        if f8 is not None:   # likewise, the fp8-query entry
            old, new = new, lambda: ix.exact_search_f8_dev(f8, K, *o_old, **kw)   # noqa: E731
        old(); new(); ix.check()
        assert ix.last_kernel() == kernel, ix.last_kernel()
        for a, b, what in zip(o_old, o_new, ("labels", "dists", "counts")):
            assert torch.equal(a, b), f"{name}: {what} differ"
        st = ix.exact_screen_stats()
        rows = dict(old=[], new=[])
        for rnd in range(args.rounds):
            for side, fn in (("old", old), ("new", new)):
                rows[side].append(timed(fn))
                log(f"{name} round {rnd} {side}: {rows[side][-1]:.3f} ms per {NQ}-query call (median of {args.reps})")
        o, n = rows["old"], rows["new"]
        spread = (max(o) - min(o)) / np.median(o) * 100
        spread_new = (max(n) - min(n)) / np.median(n) * 100
        delta = (np.median(n) / np.median(o) - 1) * 100
        so, sn = ("screened", "q8") if q8 is not None else ("screened", "f16q") if f16 is not None else ("screened", "f8q") if f8 is not None else ("scan", "screened")
        log(f"{name}: outputs identical | {so} {np.median(o):.3f} ms ({', '.join(f'{x:.3f}' for x in o)}, spread {spread:.2f} %) | {sn} "
            f"{np.median(n):.3f} ms ({', '.join(f'{x:.3f}' for x in n)}, spread {spread_new:.2f} %) | {sn} / {so} {delta:+.2f} % -> "
            + ("inside the spread: no difference shown" if abs(delta) <= max(spread, spread_new) else "outside the spread")
            + f" | fell_back {st['fell_back']}, reranked_rows {st['reranked_rows']} ({st['reranked_rows'] / max(st['screened'], 1):.2f} per screened query)")
        result[name] = {so + "_ms": o, sn + "_ms": n, **st}

    dq = torch.from_numpy(q).to(dev)
    if args.q8:
        ix.set_row_format(hs.HS_ROWS_U8)
        assert np.array_equal(q, q.astype(np.uint8)), "the bench's queries are bytes"
        compare("u8 rows, byte queries", dq, "hs::xq_screen_kernel_u8", q8=torch.from_numpy(q.astype(np.uint8)).to(dev))
        log("RESULT " + json.dumps(result))
        return 0
    if args.f16q:
        ix.set_row_format(hs.HS_ROWS_F16)
        assert np.array_equal(q, q.astype(np.float16).astype(np.float32)), "the bench's queries are exact halves"
        compare("fp16 rows, fp16 queries", dq, "hs::xh_screen_kernel", f16=torch.from_numpy(q.astype(np.float16)).to(dev))
        log("RESULT " + json.dumps(result))
        return 0
    if args.f8q:
        ix.set_row_format(hs.HS_ROWS_F8)
        qb, qv = e4m3_of_bench(q)
        compare("fp8 rows, fp8 queries", torch.from_numpy(qv).to(dev), "hs::xf_screen_kernel", f8=torch.from_numpy(qb).to(dev))
        log("RESULT " + json.dumps(result))
        return 0
    compare("fp32 rows", dq, "hs::xs_screen_kernel")
    rng = np.random.default_rng(3)
    fs = hs.FilterSet.create(ix, PER)
    fs.write(0, (rng.random((PER, N)) < 0.01).astype(np.uint8))
    foq = np.sort((np.arange(NQ) % PER).astype(np.int32), kind="stable")   # grouped by filter
    compare("1 % allowed, grouped by filter", dq, "hs::xs_screen_kernel", fs=fs, d_filter_of_query=torch.from_numpy(foq).to(dev))
    ix.set_row_format(hs.HS_ROWS_U8)
    compare("u8 rows", dq, "hs::xs_screen_kernel_u8")
    log("RESULT " + json.dumps(result))
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)
