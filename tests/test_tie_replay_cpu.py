"""Premise of tests/test_gpu_tie_replay.py, from the oracle alone (no device): on the doubled-rows graph of tests/tie_replay.py every
one of the 32 queries, at every (ef, k) of every leg, on both metrics and all three overloads, is a query whose k-subset hangs on
the layout of the reference's result heap.  A condition on the data, not a measurement: if a query fails it, the data changes
(tie_replay.SEED / LO / HI), no query is exempted."""
import numpy as np

import tie_replay as tr
from hsutil import Oracle, load_product


def test_every_query_ties_at_the_boundary(tmp_path):
    hs, oracle = load_product(), Oracle()
    files, base, q = tr.build_files(hs, str(tmp_path))
    assert base.shape == (512, 16) and q.shape == (32, 16)
    assert np.array_equal(base[0::2], base[1::2]) and len(np.unique(base, axis=0)) == 256
    assert all(k % 2 == 1 or ef == k for ef, k in tr.ALL_PAIRS)
    for f in files.values():
        for kind, path, call in tr.overloads(f):
            ox = oracle.load(path, kind, f["metric"], tr.D)
            for ef, k in tr.ALL_PAIRS:
                o = tr.reference(ox, q, ef, k, call)
                need = tr.through_replay(ox, q, ef, k, call, o)
                assert need.shape == (32,) and need.all(), f"{f['name']} {kind} {call} ef={ef} k={k}: queries {np.flatnonzero(~need).tolist()} do not tie"
                assert np.all(o["raw_sz"] >= k), f"{f['name']} {kind} {call} ef={ef} k={k}: a query has fewer than k results"
