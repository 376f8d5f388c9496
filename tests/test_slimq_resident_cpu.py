"""A resident SlimQ index from rows or a graph, the parts that need no device:

  * hs_build_rabitq_hnsw_batched_mem + hs_graph_save write the file of hs_build_rabitq_hnsw_batched; hs_graph_load + hs_graph_save
    round-trip it;
  * hs_graph_convert_slimq(convert_device = -1) to a file writes the bytes of hs_convert_hnsw_to_slimq(device = -1);
  * its refusals: neither output, and a resident index without a device (nothing written);
  * the host statement of the three arrays (csrc/slimq_tiles.hpp through hs_debug_slimq_arrays_host) against an independent numpy
    reading of the file (tests/slimq_resident_util.py), on a converted graph and on hand-written files at every size where the tile
    assembly takes another path;
  * the stand-alone program slimq_tiles_test (AddressSanitizer / UBSan) on the same hand-made shapes.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from hsutil import ROOT, load_product
from slimq_convert_util import clustered_rows
from slimq_resident_util import HANDMADE, numpy_arrays, rec_words, write_slimq


@pytest.fixture(scope="module")
def hs():
    return load_product()


def read(p):
    with open(p, "rb") as f:
        return f.read()


BUILD = dict(M=8, ef_construction=40, seed=100)


@pytest.fixture(scope="module")
def base_graph(hs, tmp_path_factory):
    base = clustered_rows(300, 64, 5, integer=False)
    p = str(tmp_path_factory.mktemp("g") / "h.bin")
    hs.build_rabitq_hnsw_batched(base, p, device=-1, threads=2, **BUILD)
    return base, p


@pytest.mark.parametrize("batch_max", (1, 0), ids=("serial", "default"))
def test_mem_build_saves_the_file_builds_bytes(hs, tmp_path, batch_max):
    base = clustered_rows(300, 64, 5, integer=False)
    want, got = str(tmp_path / "w.bin"), str(tmp_path / "g.bin")
    st_file = hs.build_rabitq_hnsw_batched(base, want, device=-1, threads=2, batch_max=batch_max, **BUILD)
    with hs.build_rabitq_hnsw_batched_mem(base, device=-1, threads=2, batch_max=batch_max, **BUILD)[0] as g:
        g.save(got)
        assert g.info() == dict(n=300, dim=64, metric=0, M=8, ef_construction=40, maxlevel=g.info()["maxlevel"])
    assert read(got) == read(want)
    assert st_file["used_gpu"] is False and st_file["batches"] > 0


def test_graph_load_save_round_trips(hs, base_graph, tmp_path):
    base, hp = base_graph
    out = str(tmp_path / "again.bin")
    with hs.Graph.load(hp, 64) as g:
        assert g.info()["n"] == 300 and g.info()["dim"] == 64
        g.save(out)
    assert read(out) == read(hp)
    with pytest.raises(hs.HsError) as e:
        hs.Graph.load(str(tmp_path / "nope.bin"), 64)
    assert e.value.status in (hs.HS_ERR_IO, hs.HS_ERR_CORRUPT)
    with pytest.raises(hs.HsError):
        hs.Graph.load(hp, 96)


CONVERT = dict(top_degree_M0=12, low_degree_m0=5, top_degree_M=6, low_degree_m=3, flip_seed=3, threads=2)


@pytest.mark.parametrize("with_ids", (False, True), ids=("nearest", "ids"))
@pytest.mark.parametrize("metric,dim", ((0, 64), (1, 96)), ids=("l2_d64", "ip_d96"))
def test_graph_convert_writes_the_file_entrys_bytes(hs, tmp_path, metric, dim, with_ids):
    n = 400
    base = clustered_rows(n, dim, 11 + metric, integer=False)
    cen = np.ascontiguousarray(base[:4])
    ids = (np.arange(n) * 7 % 4).astype(np.uint32) if with_ids else None
    hp, want, got = (str(tmp_path / x) for x in ("h.bin", "w.bin", "g.bin"))
    hs.build_rabitq_hnsw_batched(base, hp, metric=metric, device=-1, threads=2, **BUILD)
    hs.convert_hnsw_to_slimq(hp, want, dim, cen, metric=metric, cluster_ids=ids, device=-1, **CONVERT)
    with hs.build_rabitq_hnsw_batched_mem(base, metric=metric, device=-1, threads=2, **BUILD)[0] as g:
        ix, st = hs.graph_convert_slimq(g, cen, out_path=got, cluster_ids=ids, convert_device=-1, **CONVERT)
    assert ix is None
    assert read(got) == read(want)
    assert st["graph_used_gpu"] == 0 and st["records_used_gpu"] == 0 and st["total_ms"] > 0


def test_refusals(hs, base_graph, tmp_path):
    base, hp = base_graph
    cen = np.ascontiguousarray(base[:4])
    out = str(tmp_path / "o.bin")
    with hs.Graph.load(hp, 64) as g:
        # neither a file nor an index
        with pytest.raises(hs.HsError) as e:
            hs.graph_convert_slimq(g, cen)
        assert e.value.status == hs.HS_ERR_INVALID
        # a resident index where no device is: refused before any work, the file of the same call is not written
        if hs.device_count() == 0:
            with pytest.raises(hs.HsError) as e:
                hs.graph_convert_slimq(g, cen, out_path=out, want_index=True)
            assert e.value.status == hs.HS_ERR_DEVICE
            with pytest.raises(hs.HsError) as e:
                hs.slimq_index_from_rows(base, cen, M=8, ef_construction=40, device=0)
            assert e.value.status == hs.HS_ERR_DEVICE
        with pytest.raises(hs.HsError) as e:
            hs.graph_convert_slimq(g, cen, out_path=out, want_index=True, index_device=99)
        assert e.value.status == hs.HS_ERR_DEVICE
        assert not os.path.exists(out)
        # the refusals of the calls being chained
        with pytest.raises(hs.HsError) as e:
            hs.graph_convert_slimq(g, cen, out_path=out, convert_device=-2)
        assert e.value.status == hs.HS_ERR_INVALID
        with pytest.raises(hs.HsError) as e:
            hs.graph_convert_slimq(g, cen, out_path=out, cluster_ids=np.full(300, 4, np.uint32))
        assert e.value.status == hs.HS_ERR_INVALID
        assert not os.path.exists(out)
    with pytest.raises(hs.HsError) as e:
        hs.slimq_index_from_rows(base, cen, M=8, device=-1)
    assert e.value.status == hs.HS_ERR_INVALID
    with pytest.raises(hs.HsError) as e:
        hs.slimq_index_from_rows(base[:, :32], cen[:, :32], M=8, device=99)
    assert e.value.status == hs.HS_ERR_DEVICE   # (the build's device check comes first, as in hs_build_rabitq_hnsw_batched)
    L = hs.lib()
    assert L.hs_graph_save(None, out.encode()) == hs.HS_ERR_INVALID
    assert L.hs_graph_info(None, None, None, None, None, None, None) == hs.HS_ERR_INVALID
    assert L.hs_slimq_index_save(None, out.encode()) == hs.HS_ERR_INVALID
    assert L.hs_debug_slimq_arrays(None, 0, None, 0, None, None, None) == hs.HS_ERR_INVALID
    L.hs_graph_free(None)


def check_host_arrays(hs, path, dim, metric=0):
    for fused in (True, False):
        want = numpy_arrays(path, fused)
        for which in (0, 1, 2):
            got, stride, rw = hs.debug_slimq_arrays_host(path, dim, which, metric=metric, fused=fused)
            w, ws, wrw = want[which]
            assert (stride, rw) == (ws, wrw), (which, fused)
            assert got.shape == w.shape and np.array_equal(got, w), (which, fused)
    return numpy_arrays(path, True)


def test_host_arrays_of_a_converted_graph(hs, base_graph, tmp_path):
    base, hp = base_graph
    qp = str(tmp_path / "q.bin")
    hs.convert_hnsw_to_slimq(hp, qp, 64, np.ascontiguousarray(base[:4]), device=-1, **CONVERT)
    arr = check_host_arrays(hs, qp, 64)
    assert arr[1][1] == 16 and arr[2][1] == 16 and arr[0][0].size == 300 * 8


@pytest.mark.parametrize("name", sorted(HANDMADE))
def test_host_arrays_of_handmade_files(hs, tmp_path, name):
    dim, lists, ep = HANDMADE[name]
    p = str(tmp_path / "q.bin")
    write_slimq(p, dim, lists, enterpoint=ep, ncl=2)
    arr = check_host_arrays(hs, p, dim)
    n, rw = len(lists), rec_words((dim + 63) // 64 * 64)
    assert rw == {64: 8, 128: 8, 192: 12}[dim]
    expect = {  # name -> (ftile stride, uptile stride)
        "single": (16, 0), "empty_level2": (16, 16), "deg16": (16, 0), "deg17": (32, 0), "hub64": (64, 0), "hub65": (0, 0),
        "upper65": (16, 0), "upper17_d192": (16, 32),
    }[name]
    assert (arr[1][1], arr[2][1]) == expect
    assert arr[1][0].size == n * expect[0] * rw
    if name == "empty_level2":
        ut = arr[2][0].reshape(-1, 16, rw + 4)
        assert ut.shape[0] == 6   # nodes 0 and 2: two lists and one unowned row each
        assert ut[0, 0, 3] == 1 and ut[0, 0, rw] == 0xFFFFFFFF and ut[0, 1, 3] == 2 and ut[0, 1, rw] == 3
        assert np.all(ut[2, :, 3] == 0xFFFFFFFF) and not ut[2][:, [0, 1, 2] + list(range(4, rw + 4))].any()


def test_host_arrays_capacity_and_bad_arguments(hs, tmp_path):
    dim, lists, ep = HANDMADE["deg16"]
    p = str(tmp_path / "q.bin")
    write_slimq(p, dim, lists, enterpoint=ep)
    L = hs.lib()
    words = ctypes.c_size_t()
    buf = np.zeros(4, np.uint32)
    assert L.hs_debug_slimq_arrays_host(p.encode(), 0, dim, 1, 1, buf.ctypes.data, 4, ctypes.byref(words), None, None) == hs.HS_ERR_CAPACITY
    assert words.value == 20 * 16 * 8
    assert L.hs_debug_slimq_arrays_host(p.encode(), 0, dim, 1, 3, None, 0, ctypes.byref(words), None, None) == hs.HS_ERR_INVALID
    assert L.hs_debug_slimq_arrays_host(None, 0, dim, 1, 0, None, 0, ctypes.byref(words), None, None) == hs.HS_ERR_INVALID
    assert L.hs_debug_slimq_arrays_host(p.encode(), 1, dim, 1, 0, None, 0, ctypes.byref(words), None, None) == hs.HS_ERR_CORRUPT


def test_tiles_program():
    """csrc/slimq_tiles_test.cpp: the host functions of csrc/slimq_tiles.hpp on the hand-made shapes, under AddressSanitizer / UBSan."""
    exe = os.path.join(ROOT, "hnsw-slim_amd", "slimq_tiles_test")
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "slimq_tiles ok" in run.stdout, run.stdout + run.stderr
