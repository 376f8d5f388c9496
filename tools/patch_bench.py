#!/usr/bin/env python3
"""patch_bench.py -- hs_index_patch on the (dim 128, n0 8000, delta 1500) patch of tests/test_gpu_patch.py.  `prepare DIR` writes the
two Slim files and the stream (CPU only); `time DIR REPS` loads old.slim with room and times one patch call (to_add = 1), REPS times
on a fresh index each after one uncounted call, with the library HS_LIB names (A/B runs share DIR), and prints the median, the
extremes, a digest of the patched index's answers and its device_bytes -> profiles/resident_write.log."""
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from hsutil import load_chal_encode, load_product, mixture  # noqa: E402

DIM, N0, DELTA = 128, 8000, 1500


def main():
    mode, d = sys.argv[1], sys.argv[2]
    hs, ce = load_product(), load_chal_encode()
    if mode == "prepare":
        os.makedirs(d, exist_ok=True)
        base = mixture(N0 + DELTA, DIM, 17, integer=True)
        raw = {}
        for tag, n in (("old", N0), ("new", N0 + DELTA)):
            hp, sp = os.path.join(d, f"{tag}.hnsw"), os.path.join(d, f"{tag}.slim")
            hs.build_hnsw(base[:n], hp, M=16, ef_construction=100, threads=1)
            hs.convert_slim(hp, sp, DIM, threads=1)
            raw[tag] = open(sp, "rb").read()
        patch, n_changed, n_added = ce.make_patch(raw["old"], raw["new"], DIM, to_add=True)
        open(os.path.join(d, "patch.bin"), "wb").write(patch)
        print(f"prepared: {n_changed} changed old nodes, {n_added} new nodes, {len(patch)} bytes", flush=True)
        return
    reps = int(sys.argv[3])
    patch = open(os.path.join(d, "patch.bin"), "rb").read()
    q = mixture(300, DIM, 18, integer=True)
    ms, answer = [], None
    for r in range(reps + 1):   # the first call (kernel load, first allocations) is not counted
        ix = hs.Index(os.path.join(d, "old.slim"), hs.HS_KIND_SLIM, DIM, max_elements=N0 + DELTA + 16)
        t0 = time.perf_counter()
        ix.patch(patch, to_add=True)
        t = (time.perf_counter() - t0) * 1e3
        if r:
            ms.append(t)
        ix.set_ef(48)
        got = ix.search_ids(q, 10, want_dists=True)
        key = (got["labels"].tobytes(), got["dists"].tobytes(), ix.info()["device_bytes"])
        assert answer is None or key == answer
        answer = key
        del ix
    print("RESULT " + json.dumps(dict(what="patch", lib=os.environ.get("HS_LIB", "tree"), reps=reps, median_ms=float(np.median(ms)), min_ms=min(ms), max_ms=max(ms),
                                      answer=hashlib.sha256(answer[0] + answer[1]).hexdigest()[:16], device_bytes=answer[2])), flush=True)


if __name__ == "__main__":
    main()
