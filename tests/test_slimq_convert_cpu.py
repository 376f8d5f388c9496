"""HierarchicalNSWSlimQ::convertFromHNSW in one call and the data-side quantiser alone, host paths:

  * hs_convert_hnsw_to_slimq(device=-1) writes the bytes of hs_convert_slimq_graph followed by hs_convert_slimq, without the file
    between them;
  * hs_debug_rq_quantize_rows(device=-1) against the compiled rabitqlib (tests/golden/rabitq_ref.npz: rotation and codes bit for bit,
    factors within the 1e-4 of the column magnitude of tests/test_rabitq_cpu.py) and, bit for bit, against a numpy-float32 reading of
    the reference's text (tests/slimq_convert_util.py);
  * the prune's closed form against prune_slimq (the host-only program slimq_prune_test);
  * the refusals of the new entries.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from hsutil import GOLDEN, ROOT, load_product
from slimq_convert_util import clustered_rows, quantize_rows_restated, same_bits_or_nan

G = np.load(os.path.join(GOLDEN, "rabitq_ref.npz"))


@pytest.fixture(scope="module")
def hs():
    return load_product()


def read(p):
    with open(p, "rb") as f:
        return f.read()


@pytest.fixture(scope="module")
def graphs(hs, tmp_path_factory):
    """One base graph per metric: n = 300, d = 64, M = 8, serial build."""
    out = {}
    for metric in (0, 1):
        base = clustered_rows(300, 64, 5 + metric, integer=False)
        p = str(tmp_path_factory.mktemp("g") / f"h{metric}.bin")
        hs.build_rabitq_hnsw(base, p, metric=metric, M=8, ef_construction=40, threads=1)
        out[metric] = (base, p)
    return out


@pytest.mark.parametrize("metric", (0, 1), ids=("l2", "ip"))
@pytest.mark.parametrize("with_ids", (False, True), ids=("nearest", "ids"))
@pytest.mark.parametrize("thr", (0, 1))
def test_one_call_writes_the_two_step_bytes(hs, graphs, tmp_path, metric, with_ids, thr):
    base, hp = graphs[metric]
    n, d = base.shape
    cen = np.ascontiguousarray(base[:5])
    ids = (np.arange(n) * 7 % 5).astype(np.uint32) if with_ids else None
    kw = dict(threshold_level=thr, top_degree_M0=12, low_degree_m0=5, top_degree_M=6, low_degree_m=3)
    sp, qp, one = (str(tmp_path / x) for x in ("s.bin", "q.bin", "one.bin"))
    hs.convert_slimq_graph(hp, sp, d, metric=metric, threads=2, **kw)
    hs.convert_slimq(sp, metric, d, cen, qp, cluster_ids=ids, flip_seed=3, threads=2)
    st = hs.convert_hnsw_to_slimq(hp, one, d, cen, metric=metric, cluster_ids=ids, flip_seed=3, device=-1, threads=2, **kw)
    assert read(one) == read(qp)
    assert st["graph_used_gpu"] == 0 and st["records_used_gpu"] == 0 and st["graph_kernel_ms"] == 0 and st["records_kernel_ms"] == 0
    assert st["total_ms"] >= st["graph_ms"] > 0 and st["total_ms"] >= st["records_ms"] > 0


@pytest.mark.parametrize("dim", (128, 96, 768))
def test_quantiser_matches_compiled_rabitqlib(hs, dim):
    p = f"d{dim}_"
    rot, cl, codes, fac = hs.debug_rq_quantize_rows(dim, int(G[p + "metric"]), G[p + "flip"], G[p + "x"], G[p + "cen"], device=-1)
    assert np.array_equal(rot.view(np.uint32), G[p + "rx"].view(np.uint32))
    assert np.array_equal(cl, np.zeros(len(cl), np.uint32))
    assert np.array_equal(codes, G[p + "codes"])
    scale = np.abs(G[p + "fac"]).max(axis=0, keepdims=True)
    assert np.all(np.abs(fac - G[p + "fac"]) <= 1e-4 * scale)


@pytest.mark.parametrize("metric", (0, 1), ids=("l2", "ip"))
@pytest.mark.parametrize("dim,ncl", ((64, 1), (100, 7), (192, 3)))
def test_quantiser_matches_numpy_reading_of_the_reference(hs, metric, dim, ncl):
    rng = np.random.default_rng(dim + metric)
    n = 40
    rows = clustered_rows(n, dim, dim, integer=False)
    cen = np.ascontiguousarray(rows[:ncl] + rng.normal(0, 0.1, (ncl, dim)).astype(np.float32))
    if ncl > 2:
        cen[2] = cen[1]          # duplicate centroids: the first wins
        rows[5] = cen[0]         # a row equal to its centroid: ip_resi == 0
    flips = rng.integers(0, 256, 4 * ((dim + 63) // 64 * 64) // 8, dtype=np.uint8)
    for ids in (None, (np.arange(n) % ncl).astype(np.uint32)):
        rot, cl, codes, fac = hs.debug_rq_quantize_rows(dim, metric, flips, rows, cen, cluster_ids=ids, device=-1)
        rx, rc = hs.rabitq_rotate(dim, flips, rows), hs.rabitq_rotate(dim, flips, cen)   # (pinned by tests/test_rabitq_cpu.py)
        assert np.array_equal(rot.view(np.uint32), rx.view(np.uint32))
        want_cl, want_codes, want_fac = quantize_rows_restated(rows, cen, rx, rc, metric, ids)
        assert np.array_equal(cl, want_cl)
        assert ids is not None or 2 not in cl
        assert np.array_equal(codes, want_codes)
        assert same_bits_or_nan(fac, want_fac)


def test_prune_closed_form_program():
    """csrc/slimq_prune_test.cpp: the chunked closed form of csrc/slimq_prune.hpp against prune_slimq, random and tie-heavy lists,
    Mlim 0 and 1 among the budgets."""
    exe = os.path.join(ROOT, "hnsw-slim_amd", "slimq_prune_test")
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "slimq_prune ok" in run.stdout, run.stdout + run.stderr


def test_refusals(hs, graphs, tmp_path):
    base, hp = graphs[0]
    n, d = base.shape
    cen = np.ascontiguousarray(base[:4])
    out, sp = str(tmp_path / "o.bin"), str(tmp_path / "s.bin")
    hs.convert_slimq_graph(hp, sp, d, threads=2)
    bad_ids = np.full(n, 4, np.uint32)

    def status(fn, *a, **k):
        with pytest.raises(hs.HsError) as e:
            fn(*a, **k)
        return e.value.status
    # metric, dim range, cluster ids, on each entry that takes them
    assert status(hs.convert_hnsw_to_slimq, hp, out, d, cen, metric=7) == hs.HS_ERR_INVALID
    assert status(hs.convert_slimq_graph_gpu, hp, out, d, metric=7, device=0) == hs.HS_ERR_INVALID
    assert status(hs.convert_slimq_gpu, sp, 7, d, cen, out, device=0) == hs.HS_ERR_INVALID
    assert status(hs.debug_rq_quantize_rows, d, 7, np.zeros(4 * d // 8, np.uint8), base, cen) == hs.HS_ERR_INVALID
    for bad_dim in (32, 4096):
        rows = np.zeros((2, bad_dim), np.float32)
        flips = np.zeros(4 * ((bad_dim + 63) // 64 * 64) // 8, np.uint8)
        assert status(hs.convert_hnsw_to_slimq, hp, out, bad_dim, rows) == hs.HS_ERR_UNSUPPORTED
        assert status(hs.convert_slimq_gpu, sp, 0, bad_dim, rows, out, device=0) == hs.HS_ERR_UNSUPPORTED
        assert status(hs.debug_rq_quantize_rows, bad_dim, 0, flips, rows, rows) == hs.HS_ERR_UNSUPPORTED
    assert status(hs.convert_hnsw_to_slimq, hp, out, d, cen, cluster_ids=bad_ids) == hs.HS_ERR_INVALID
    assert status(hs.debug_rq_quantize_rows, d, 0, np.zeros(4 * d // 8, np.uint8), base, cen, cluster_ids=bad_ids) == hs.HS_ERR_INVALID
    assert status(hs.convert_hnsw_to_slimq, hp, out, d, cen, device=-2) == hs.HS_ERR_INVALID
    # a device that does not exist
    assert status(hs.convert_hnsw_to_slimq, hp, out, d, cen, device=99) == hs.HS_ERR_DEVICE
    assert status(hs.convert_slimq_graph_gpu, hp, out, d, device=99) == hs.HS_ERR_DEVICE
    assert status(hs.convert_slimq_gpu, sp, 0, d, cen, out, device=99) == hs.HS_ERR_DEVICE
    assert status(hs.debug_rq_quantize_rows, d, 0, np.zeros(4 * d // 8, np.uint8), base, cen, device=99) == hs.HS_ERR_DEVICE
    # a file that is not there
    assert status(hs.convert_hnsw_to_slimq, str(tmp_path / "nope.bin"), out, d, cen) in (hs.HS_ERR_IO, hs.HS_ERR_CORRUPT)
    assert not os.path.exists(out)
    # null pointers, through the C ABI itself
    L = hs.lib()
    c, f = cen.ctypes.data, ctypes.c_float
    assert L.hs_convert_hnsw_to_slimq(None, 0, d, 0, f(.02), f(.02), 32, 8, 16, 4, c, 4, None, 1, -1, 1, out.encode(), None) == hs.HS_ERR_INVALID
    assert L.hs_convert_hnsw_to_slimq(hp.encode(), 0, d, 0, f(.02), f(.02), 32, 8, 16, 4, None, 4, None, 1, -1, 1, out.encode(), None) == hs.HS_ERR_INVALID
    assert L.hs_convert_hnsw_to_slimq(hp.encode(), 0, d, 0, f(.02), f(.02), 32, 8, 16, 4, c, 0, None, 1, -1, 1, out.encode(), None) == hs.HS_ERR_INVALID
    assert L.hs_convert_hnsw_to_slimq(hp.encode(), 0, d, 0, f(.02), f(.02), 32, 8, 16, 4, c, 4, None, 1, -1, 1, None, None) == hs.HS_ERR_INVALID
    assert L.hs_convert_slimq_graph_gpu(None, 0, d, 0, f(.02), f(.02), 32, 8, 16, 4, 0, 1, out.encode(), None, None) == hs.HS_ERR_INVALID
    assert L.hs_convert_slimq_gpu(sp.encode(), 0, d, None, 4, None, 1, 0, 1, out.encode(), None, None) == hs.HS_ERR_INVALID
    assert L.hs_convert_slimq_gpu(sp.encode(), 0, d, c, 4, None, 1, 0, 1, None, None, None) == hs.HS_ERR_INVALID
    assert L.hs_debug_rq_quantize_rows(d, 0, None, base.ctypes.data, n, c, 4, None, -1, None, None, None, None) == hs.HS_ERR_INVALID
