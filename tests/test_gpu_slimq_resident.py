"""A resident SlimQ index from rows or a graph, on the GPU.

  * the three record arrays as the tile kernels (csrc/slimq_tiles.hip) left them on the device, against the independent numpy reading
    of the file (tests/slimq_resident_util.py): hand-written files at every size where the assembly takes another path, one
    converted graph, with and without HS_SLIMQ_FUSED=0;
  * slimq_index_from_rows (no file) against the file chain build_rabitq_hnsw_batched -> convert_hnsw_to_slimq -> Index ->
    slimq_set_dataset: arrays, hs_info (device_bytes with it), answers, traversal counters and traces bit for bit, and the saved file;
  * graph_convert_slimq on the host against on the device; the refusals a SlimQ index keeps.
"""
import os
import subprocess

import numpy as np
import pytest

from hsutil import ROOT, load_product
from slimq_convert_util import clustered_rows
from slimq_resident_util import HANDMADE, numpy_arrays, write_slimq

pytestmark = pytest.mark.gpu

N, NQ = 3000, 200
BUILD = dict(M=16, ef_construction=64, seed=100)


@pytest.fixture(scope="module")
def hs():
    return load_product()


def read(p):
    with open(p, "rb") as f:
        return f.read()


def data(d, metric):
    x = clustered_rows(N + NQ, d, 31 + d + metric, integer=False, n_centres=8)
    return np.ascontiguousarray(x[:N]), np.ascontiguousarray(x[N:])


@pytest.fixture(scope="module")
def pairs(hs, tmp_path_factory):
    """(d, metric) -> dict(a = the index made from rows, b = the index loaded from the file chain's file, base, q, cen, qp, stats)"""
    tmp = tmp_path_factory.mktemp("resident")
    made = {}

    def get(d, metric):
        if (d, metric) not in made:
            base, q = data(d, metric)
            cen = np.ascontiguousarray(base[:8])
            hp, qp = str(tmp / f"h{d}_{metric}.bin"), str(tmp / f"q{d}_{metric}.bin")
            a, st = hs.slimq_index_from_rows(base, cen, metric=metric, device=0, threads=8, with_dataset=True, **BUILD)
            hs.build_rabitq_hnsw_batched(base, hp, metric=metric, device=0, threads=8, **BUILD)
            hs.convert_hnsw_to_slimq(hp, qp, d, cen, metric=metric, device=0, threads=8)
            b = hs.Index(qp, hs.HS_KIND_SLIMQ, d, metric=metric)
            b.slimq_set_dataset(base)
            made[(d, metric)] = dict(a=a, b=b, base=base, q=q, cen=cen, hp=hp, qp=qp, stats=st)
        return made[(d, metric)]
    return get


def assert_arrays_equal(x, y):
    for which in (0, 1, 2):
        gx, sx, rx = x.debug_slimq_arrays(which)
        gy, sy, ry = y.debug_slimq_arrays(which)
        assert (sx, rx) == (sy, ry), which
        assert gx.shape == gy.shape and np.array_equal(gx, gy), which


def assert_device_arrays(ix, path, fused):
    want = numpy_arrays(path, fused)
    for which in (0, 1, 2):
        got, stride, rw = ix.debug_slimq_arrays(which)
        w, ws, wrw = want[which]
        assert (stride, rw) == (ws, wrw), (which, fused)
        assert got.shape == w.shape and np.array_equal(got, w), (which, fused)


def assert_same_answers(a, b, q, efs, k=10, trace=True):
    b.slimq_set_tconst(a.slimq_tconst())
    for ef in efs:
        a.set_ef(ef)
        b.set_ef(ef)
        ga, gb = a.slimq_search(q, k, want_stats=True), b.slimq_search(q, k, want_stats=True)
        assert np.array_equal(ga["labels"], gb["labels"]), ef
        assert np.array_equal(ga["dists"].view(np.uint32), gb["dists"].view(np.uint32)), ef
        assert np.array_equal(ga["cnt"], gb["cnt"]) and np.array_equal(ga["stats"], gb["stats"]), ef
        if trace:
            ta, sa = a.slimq_trace(q[:32], k, 2048)
            tb, sb = b.slimq_trace(q[:32], k, 2048)
            assert np.array_equal(ta, tb) and np.array_equal(sa, sb), ef


@pytest.mark.parametrize("fused", (True, False), ids=("fused", "unfused"))
@pytest.mark.parametrize("name", sorted(HANDMADE))
def test_device_arrays_of_handmade_files(hs, tmp_path, monkeypatch, name, fused):
    dim, lists, ep = HANDMADE[name]
    p = str(tmp_path / "q.bin")
    write_slimq(p, dim, lists, enterpoint=ep, ncl=2)
    if not fused:
        monkeypatch.setenv("HS_SLIMQ_FUSED", "0")
    ix = hs.Index(p, hs.HS_KIND_SLIMQ, dim)
    assert_device_arrays(ix, p, fused)
    assert ix.info()["n"] == len(lists)
    ix.close()


@pytest.mark.parametrize("fused", (True, False), ids=("fused", "unfused"))
def test_device_arrays_of_a_converted_graph(hs, pairs, monkeypatch, fused):
    e = pairs(128, 0)
    if not fused:
        monkeypatch.setenv("HS_SLIMQ_FUSED", "0")
    ix = hs.Index(e["qp"], hs.HS_KIND_SLIMQ, 128)
    assert_device_arrays(ix, e["qp"], fused)
    if fused:
        assert ix.debug_slimq_arrays(1)[1] in (16, 32) and ix.debug_slimq_arrays(2)[0].size > 0
    ix.close()


@pytest.mark.parametrize("metric", (0, 1), ids=("l2", "ip"))
@pytest.mark.parametrize("d", (64, 96, 128))
def test_index_from_rows_is_the_index_of_the_file_chain(hs, pairs, tmp_path, d, metric):
    e = pairs(d, metric)
    a, b = e["a"], e["b"]
    assert_arrays_equal(a, b)
    assert a.info() == b.info()     # device_bytes among the fields
    assert a.info()["n"] == N and a.info()["kind"] == hs.HS_KIND_SLIMQ
    assert_same_answers(a, b, e["q"], (10, 64, 200))
    out = str(tmp_path / "saved.bin")
    a.save_slimq(out)
    assert read(out) == read(e["qp"])
    b.save_slimq(out)
    assert read(out) == read(e["qp"])
    st = e["stats"]
    assert st["build"]["used_gpu"] and st["convert"]["graph_used_gpu"] == 1 and st["convert"]["records_used_gpu"] == 1
    assert st["total_ms"] >= st["resident_ms"] >= st["tile_kernel_ms"] > 0


def test_split_launch_from_6144_queries(hs, pairs):
    e = pairs(64, 0)
    rng = np.random.default_rng(3)
    q = e["base"][rng.integers(0, N, 6200)] + rng.normal(0, 0.2, (6200, 64)).astype(np.float32)
    assert_same_answers(e["a"], e["b"], np.ascontiguousarray(q, np.float32), (48,), trace=False)


def test_convert_on_host_and_on_device_agree(hs, pairs, tmp_path):
    e = pairs(96, 1)
    fh, fd, sh, sd = (str(tmp_path / x) for x in ("fh.bin", "fd.bin", "sh.bin", "sd.bin"))
    with hs.Graph.load(e["hp"], 96, metric=1) as g:
        ih, sth = hs.graph_convert_slimq(g, e["cen"], out_path=fh, want_index=True, with_dataset=True, convert_device=-1, threads=8)
        idv, std = hs.graph_convert_slimq(g, e["cen"], out_path=fd, want_index=True, with_dataset=True, convert_device=0, threads=8)
    assert sth["graph_used_gpu"] == 0 and std["graph_used_gpu"] == 1 and std["records_used_gpu"] == 1
    assert read(fh) == read(fd) == read(e["qp"])
    assert_arrays_equal(ih, idv)
    assert_arrays_equal(ih, e["b"])
    assert ih.info() == idv.info() == e["b"].info()
    ih.save_slimq(sh)
    idv.save_slimq(sd)
    assert read(sh) == read(sd) == read(fh)
    assert_same_answers(ih, e["b"], e["q"], (64,), trace=False)   # the dataset came from the graph's own rows
    ih.close()
    idv.close()


def test_refusals_of_a_resident_slimq_index(hs, pairs):
    e = pairs(64, 0)
    with hs.Graph.load(e["hp"], 64) as g:
        ix, _ = hs.graph_convert_slimq(g, e["cen"], want_index=True, with_dataset=False, convert_device=0, threads=8)
    ix.set_ef(64)
    with pytest.raises(hs.HsError) as err:
        ix.slimq_search(e["q"], 10)
    assert err.value.status == hs.HS_ERR_INVALID and "hs_slimq_set_dataset() first" in str(err.value)
    ix.slimq_set_dataset(e["base"])
    assert_same_answers(ix, e["b"], e["q"], (64,), trace=False)
    assert ix.info() == e["b"].info()
    a = e["a"]
    with pytest.raises(hs.HsError) as err:
        a.add_points(e["base"][:2], np.array([N + 1, N + 2], np.uint64))
    assert err.value.status == hs.HS_ERR_UNSUPPORTED
    with pytest.raises(hs.HsError) as err:
        a.mark_deleted([0])
    assert err.value.status == hs.HS_ERR_UNSUPPORTED
    with pytest.raises(hs.HsError) as err:
        hs.SearchQueue(a, 10, hs.HS_MODE_PQ)
    assert err.value.status == hs.HS_ERR_INVALID
    ix.close()


def test_facade_builds_and_searches_without_a_file(tmp_path):
    """tests/facade_slimq_resident.cpp: construct -> convertFromHNSW -> setDataset -> searchKnn under setBuildOnDevice with no file
    created, the answers those of an index loaded from saveIndex's file."""
    exe = os.path.join(ROOT, "hnsw-slim_amd", "facade_slimq_resident")
    run = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True)
    assert run.returncode == 0 and "facade_slimq_resident ok" in run.stdout, run.stdout + run.stderr
