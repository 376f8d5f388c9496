#!/usr/bin/env python3
"""narrow_build_bench.py -- the batched build on the device over u8 rows (hs_build_hnsw_batched_rows) against the same
build over fp32 rows (hs_build_hnsw_batched), on the bench's rows: 1M x 128 SIFT-like integers (the cached data of bench.py when it is
there, the same generator otherwise), M = 16, ef_construction = 200.  ONE process, `--rounds` alternated rounds of the two calls; per
call its own kernel_ms (device events, first kernel to last) and total_ms (the call, file write included), and beside them the time
of a pageable host-to-device copy of the bytes each call uploads (the same copy the call makes, timed here around a synchronise).
The difference of the kernel_ms medians is printed beside the spread of the fp32 rounds; the two files of the last round are compared.
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


def med(xs):
    return sorted(xs)[len(xs) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--index-dir", default="", help="index files of bench.py --index-dir instead of the user cache directory")
    args = ap.parse_args()
    import torch
    torch.cuda.init()   # (torch's bundled HIP runtime opens the device before the product's does, as in bench.py)
    hs = load_product()
    N = args.n
    idir = args.index_dir or index_cache_dir(N, D, 1)
    if os.path.exists(os.path.join(idir, "ready")) and os.path.exists(os.path.join(idir, "base.npy")):
        base = np.ascontiguousarray(np.load(os.path.join(idir, "base.npy"))[:N], np.float32)
    else:
        base = headline_data(N, D, 123)
    narrow = base.astype(np.uint8)
    assert np.array_equal(narrow.astype(np.float32), base), "the bench's rows are 8-bit integers"
    # the fp32 build reads the widened rows: the generator leaves a -0.0 here and there, which u8 does not carry (no distance depends
    # on it, but the file stores the rows)
    neg0 = int((np.signbit(base) & (base == 0)).sum())
    base = narrow.astype(np.float32)
    log(f"rows: {N} x {D}, M 16, ef_construction 200; fp32 {base.nbytes >> 20} MiB, u8 {narrow.nbytes >> 20} MiB; {neg0} values -0.0 read as +0.0")

    def upload_ms(x):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        d = torch.from_numpy(x).cuda()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        del d
        return ms

    kw = dict(M=16, ef_construction=200, branching_factor="4", seed=100, device=0)
    res = {"fp32": [], "u8": []}
    with tempfile.TemporaryDirectory() as tmp:
        paths = {"fp32": os.path.join(tmp, "f.bin"), "u8": os.path.join(tmp, "u.bin")}
        upload_ms(narrow)   # (warm-up of the copy path)
        for rnd in range(args.rounds):
            for name in ("fp32", "u8"):
                up = upload_ms(base if name == "fp32" else narrow)
                st = hs.build_hnsw_batched(base, paths[name], **kw) if name == "fp32" else hs.build_hnsw_batched_rows(narrow, paths[name], **kw)
                assert st["used_gpu"]
                res[name].append((st["kernel_ms"], st["total_ms"], up))
                log(f"round {rnd} {name}: kernel_ms {st['kernel_ms']:.1f} total_ms {st['total_ms']:.1f} upload_ms {up:.1f} "
                    f"({st['batches']} batches, {st['flagged_rows']} flagged rows)")
        same = open(paths["fp32"], "rb").read() == open(paths["u8"], "rb").read()
    for name, r in res.items():
        for j, what in enumerate(("kernel_ms", "total_ms", "upload_ms")):
            xs = [x[j] for x in r]
            log(f"{name} {what}: min {min(xs):.1f} median {med(xs):.1f} max {max(xs):.1f} over {len(xs)} rounds")
    kf, ku = [x[0] for x in res["fp32"]], [x[0] for x in res["u8"]]
    log(f"kernel_ms, u8 - fp32 (medians): {med(ku) - med(kf):+.1f} ms; spread of the fp32 rounds (max - min): {max(kf) - min(kf):.1f} ms")
    log(f"the two files of the last round {'are equal' if same else 'DIFFER'}")
    if not same:
        sys.exit(1)


if __name__ == "__main__":
    main()
