"""HierarchicalNSWSlimQ::convertFromHNSW on the GPU (csrc/convert_slimq.hip), device against host, byte for byte:

  * the graph passes (hs_convert_slimq_graph_gpu against hs_convert_slimq_graph) over the branches of the raw distance (rows below a
    packet, 1-3 packets, a remainder packet, a scalar tail, long rows), both list strides, continuous and tie-heavy rows, both
    metrics, tiny graphs, a hub whose union exceeds 64 ids, one beyond the on-chip buffers, M = 40 on the host path; one case against
    the plain-Python reading of tests/slim_restated.py directly;
  * the quantiser (hs_debug_rq_quantize_rows on the device against device = -1, and against the compiled rabitqlib's fixture);
  * whole files: hs_convert_slimq_gpu, hs_convert_hnsw_to_slimq(device = 0), the search on the result, the facade program.
"""
import os
import subprocess

import numpy as np
import pytest

from hsutil import GOLDEN, ROOT, load_chal_encode, load_product, mixture, write_vanilla_level0
from slim_restated import convert_graph_restated
from slimq_convert_util import clustered_rows, same_bits_or_nan

pytestmark = pytest.mark.gpu

G = np.load(os.path.join(GOLDEN, "rabitq_ref.npz"))
RESTATED = dict(threshold_level=0, top_degree_percent0=0.02, top_degree_percent=0.02, top_degree_M0=12, low_degree_m0=5, top_degree_M=6,
                low_degree_m=3)   # the parameter set of test_slimq_graph_conversion_matches_python_restatement
DEFAULTS = dict(threshold_level=0, top_degree_percent0=0.02, top_degree_percent=0.02, top_degree_M0=32, low_degree_m0=8, top_degree_M=16,
                low_degree_m=4)   # the reference's


@pytest.fixture(scope="module")
def hs():
    return load_product()


def read(p):
    with open(p, "rb") as f:
        return f.read()


def both_ways(hs, hp, d, metric, tmp_path, kw, tag=""):
    """The host's file and the device's; returns (host bytes, device bytes, used_gpu, host path)."""
    sp, gp = str(tmp_path / f"host{tag}.bin"), str(tmp_path / f"gpu{tag}.bin")
    hs.convert_slimq_graph(hp, sp, d, metric=metric, threads=4, **kw)
    used, ms = hs.convert_slimq_graph_gpu(hp, gp, d, metric=metric, device=0, threads=4, **kw)
    assert (ms > 0) == used
    return read(sp), read(gp), used, sp


def n_out_of_id_order(path, d):
    """Final level-0 lists that are not ascending by id: a list that went through the re-prune is in distance order."""
    s = load_chal_encode().parse_slim(read(path), d)
    return sum(list(map(int, l[0])) != sorted(map(int, l[0])) for l in s["lists"] if len(l))


# (name, n, d, M, metric, integer rows, threshold_level)
GRAPH_CASES = [
    ("d8_m8_l2", 700, 8, 8, 0, False, 0),
    ("d48_m8_ip", 700, 48, 8, 1, False, 0),
    ("d64_m8_l2_ties", 900, 64, 8, 0, True, 0),
    ("d80_m32_l2", 800, 80, 32, 0, False, 0),
    ("d100_m32_ip_ties", 800, 100, 32, 1, True, 0),
    ("d128_m32_l2_ties", 1200, 128, 32, 0, True, 0),
    ("d768_m32_ip", 700, 768, 32, 1, False, 0),
    ("d64_m32_l2_thr1", 1500, 64, 32, 0, False, 1),
    ("d100_m8_l2_n70", 70, 100, 8, 0, False, 0),
    ("d64_m32_ip_n70_ties", 70, 64, 32, 1, True, 0),
    ("d48_m8_l2_n2", 2, 48, 8, 0, False, 0),
    ("d80_m32_ip_n1", 1, 80, 32, 1, False, 0),
]


@pytest.mark.parametrize("case", GRAPH_CASES, ids=[c[0] for c in GRAPH_CASES])
def test_graph_passes_match_host(hs, tmp_path, case):
    name, n, d, M, metric, integer, thr = case
    base = clustered_rows(n, d, len(name) + n, integer)
    hp = str(tmp_path / "h.bin")
    hs.build_rabitq_hnsw(base, hp, metric=metric, M=M, ef_construction=40 if M == 8 else 128, threads=1)
    for tag, kw in (("a", RESTATED), ("b", DEFAULTS)):
        kw = dict(kw, threshold_level=thr)
        want, got, used, sp = both_ways(hs, hp, d, metric, tmp_path, kw, tag)
        assert used, "the device path declined the graph"
        assert got == want, (name, tag)
        if n >= 700:
            # (at M = 32 a level-0 list is re-pruned when its union exceeds 64 ids; the low budgets of the first set leave the
            #  8-dimensional graph without such a list)
            assert n_out_of_id_order(sp, d) > 0 or (d == 8 and tag == "a"), "premise: the re-prune ran on a level-0 list"
            # the loop-index quirk is live: Slim's own heuristic gives another graph from the same file
            vp = str(tmp_path / f"slim{tag}.bin")
            assert hs.convert_slim_gpu(hp, vp, d, metric=metric, device=0, threads=4, **kw)[0]
            assert read(vp) != got


def test_graph_passes_match_python_reading(hs, tmp_path):
    """Against tests/slim_restated.py directly, not through the host: integer rows, every distance exact."""
    rng = np.random.default_rng(77)
    n, d, M = 700, 64, 8
    centres = rng.integers(-60, 60, (12, d))
    base = (centres[rng.integers(0, 12, n)] + rng.integers(-25, 26, (n, d))).astype(np.float32)
    hp, gp = str(tmp_path / "h.bin"), str(tmp_path / "g.bin")
    hs.build_rabitq_hnsw(base, hp, M=M, ef_construction=40, threads=1)
    used, _ = hs.convert_slimq_graph_gpu(hp, gp, d, device=0, threads=2, **RESTATED)
    assert used
    ce = load_chal_encode()
    g, s = ce.parse_vanilla(read(hp)), ce.parse_slim(read(gp), d)
    kw = RESTATED
    want, unstable = convert_graph_restated(g, base, kw["threshold_level"], kw["top_degree_percent0"], kw["top_degree_percent"], kw["top_degree_M0"],
                                            kw["low_degree_m0"], kw["top_degree_M"], kw["low_degree_m"], prune="slimq")
    assert unstable == 0, "premise: no equal keys in a list of more than 16"
    for v in range(n):
        assert [[int(x) for x in l] for l in s["lists"][v]] == want[v], v
    assert sum(w[0] != sorted(w[0]) for w in want) > 0, "premise: the re-prune ran"


def hub_graph(n, d):
    """Node 0 in the middle, every other node on a sphere around it and listing node 0 and five nodes it is well away from: node 0 is
    the nearest entry of every list, and candidate 0 of a sorted list is always kept, so node 0 collects n - 1 reverse edges."""
    rng = np.random.default_rng(n)
    rows = rng.normal(0, 1, (n, d))
    rows[1:] *= 40.0 / np.linalg.norm(rows[1:], axis=1, keepdims=True)
    rows[0] = 0
    rows = rows.astype(np.float32)
    lists = [[1 + i for i in range(16)]]
    for v in range(1, n):
        cos = rows[1:].astype(np.float64) @ rows[v].astype(np.float64) / 1600.0
        far = 1 + np.nonzero(cos < 0.2)[0][:5]   # squared distance above 2 * 1600 * 0.8, node 0 at 1600
        assert len(far) == 5 and v not in far
        lists.append([0] + [int(u) for u in far])
    return rows, lists


def test_hub_union_above_64_ids(hs, tmp_path):
    n, d = 400, 20
    rows, lists = hub_graph(n, d)
    hp = str(tmp_path / "hub.bin")
    write_vanilla_level0(hp, rows, lists, 8)
    want, got, used, sp = both_ways(hs, hp, d, 0, tmp_path, DEFAULTS)
    assert used and got == want
    s = load_chal_encode().parse_slim(want, d)
    assert len(s["lists"][0][0]) == 16, "premise: node 0's union of 399 reverse edges was re-pruned to its capacity"


def test_union_beyond_the_buffers_takes_the_host(hs, tmp_path):
    n, d = 2300, 20   # 2299 reverse edges > 2048
    rows, lists = hub_graph(n, d)
    hp = str(tmp_path / "hub.bin")
    write_vanilla_level0(hp, rows, lists, 8)
    want, got, used, _ = both_ways(hs, hp, d, 0, tmp_path, DEFAULTS)
    assert not used and got == want


def test_m40_takes_the_host(hs, tmp_path):
    base = clustered_rows(300, 48, 3, False)
    hp = str(tmp_path / "h.bin")
    hs.build_rabitq_hnsw(base, hp, M=40, ef_construction=60, threads=4)
    want, got, used, _ = both_ways(hs, hp, 48, 0, tmp_path, DEFAULTS)
    assert not used and got == want


# ---- the quantiser -------------------------------------------------------------------------------------------------------------------
def quant_both(hs, d, metric, rows, cen, ids=None):
    flips = np.random.default_rng(d).integers(0, 256, 4 * ((d + 63) // 64 * 64) // 8, dtype=np.uint8)
    host = hs.debug_rq_quantize_rows(d, metric, flips, rows, cen, cluster_ids=ids, device=-1)
    dev = hs.debug_rq_quantize_rows(d, metric, flips, rows, cen, cluster_ids=ids, device=0)
    assert np.array_equal(dev[0].view(np.uint32), host[0].view(np.uint32)), "rotated rows"
    assert np.array_equal(dev[1], host[1]), "cluster ids"
    assert np.array_equal(dev[2], host[2]), "codes"
    assert same_bits_or_nan(dev[3], host[3]), "factors"
    return host


@pytest.mark.parametrize("metric", (0, 1), ids=("l2", "ip"))
@pytest.mark.parametrize("d", (64, 96, 100, 128, 768, 1000, 2000))
def test_quantiser_matches_host(hs, d, metric):
    rng = np.random.default_rng(d * 2 + metric)
    rows = clustered_rows(300, d, d, False, n_centres=20)
    for ncl in (1, 16, 70):
        cen = np.ascontiguousarray(rows[rng.choice(300, ncl, replace=False)] + rng.normal(0, 0.05, (ncl, d)).astype(np.float32))
        r = rows.copy()
        if ncl > 1:
            cen[ncl - 1] = cen[0]      # duplicate centroids, 69 rounds apart at ncl = 70: the first wins
            cen[1] = cen[0]
        r[7] = cen[0]                  # rows equal to their centroid: ip_resi == 0
        r[299] = cen[ncl // 2] if ncl != 2 else cen[0]
        host = quant_both(hs, d, metric, r, cen)
        assert ncl == 1 or (1 not in host[1] and ncl - 1 not in host[1])
        assert host[1][7] == 0 and not np.any(host[2][7]), "premise: row 7 sits on centroid 0, all residuals zero"
        if ncl > 1:
            assert len(set(host[1].tolist())) > 1
        quant_both(hs, d, metric, r, cen, ids=(np.arange(300) * 5 % ncl).astype(np.uint32))


@pytest.mark.parametrize("n", (1, 65))
def test_quantiser_row_counts(hs, n):
    rows = clustered_rows(n, 100, n, False)
    cen = clustered_rows(16, 100, 99, False)
    for metric in (0, 1):
        quant_both(hs, 100, metric, rows, cen)


@pytest.mark.parametrize("scale", (2.0 ** 20, 2.0 ** -20), ids=("x2^20", "x2^-20"))
def test_quantiser_scaled_rows(hs, scale):
    for d in (96, 128):
        rows = (clustered_rows(65, d, 4, False) * np.float32(scale)).astype(np.float32)
        cen = np.ascontiguousarray(rows[:16] * np.float32(1.01))
        for metric in (0, 1):
            quant_both(hs, d, metric, rows, cen)


@pytest.mark.parametrize("dim", (128, 96, 768))
def test_quantiser_matches_compiled_rabitqlib(hs, dim):
    p = f"d{dim}_"
    rot, cl, codes, fac = hs.debug_rq_quantize_rows(dim, int(G[p + "metric"]), G[p + "flip"], G[p + "x"], G[p + "cen"], device=0)
    assert np.array_equal(rot.view(np.uint32), G[p + "rx"].view(np.uint32))
    assert np.array_equal(codes, G[p + "codes"])


# ---- whole files ---------------------------------------------------------------------------------------------------------------------
FILE_CASES = [("d64_m8_l2", 700, 64, 8, 0, False, False), ("d100_m32_ip_ties", 800, 100, 32, 1, True, True),
              ("d128_m32_l2_ties", 900, 128, 32, 0, True, False)]


@pytest.mark.parametrize("case", FILE_CASES, ids=[c[0] for c in FILE_CASES])
def test_whole_files_and_search(hs, tmp_path, case):
    name, n, d, M, metric, integer, with_ids = case
    base = clustered_rows(n, d, n + d, integer)
    cen = np.ascontiguousarray(base[:9])
    ids = (np.arange(n) * 4 % 9).astype(np.uint32) if with_ids else None
    hp, sp, qp, q1, q2 = (str(tmp_path / x) for x in ("h.bin", "s.bin", "q.bin", "q_gpu.bin", "q_one.bin"))
    hs.build_rabitq_hnsw(base, hp, metric=metric, M=M, ef_construction=40 if M == 8 else 128, threads=1)
    hs.convert_slimq_graph(hp, sp, d, metric=metric, threads=4)
    hs.convert_slimq(sp, metric, d, cen, qp, cluster_ids=ids, flip_seed=5, threads=4)
    used, ms = hs.convert_slimq_gpu(sp, metric, d, cen, q1, cluster_ids=ids, flip_seed=5, device=0, threads=4)
    assert used and ms > 0 and read(q1) == read(qp)
    st = hs.convert_hnsw_to_slimq(hp, q2, d, cen, metric=metric, cluster_ids=ids, flip_seed=5, device=0, threads=4)
    assert st["graph_used_gpu"] == 1 and st["records_used_gpu"] == 1 and st["graph_kernel_ms"] > 0 and st["records_kernel_ms"] > 0
    assert read(q2) == read(qp)
    q = clustered_rows(30, d, 1, integer)
    res = []
    for p in (qp, q2):
        ix = hs.Index(p, hs.HS_KIND_SLIMQ, d, metric=metric)
        ix.slimq_set_dataset(base)
        ix.set_ef(48)
        res.append(ix.slimq_search(q, 10))
    assert np.array_equal(np.asarray(res[0]["labels"]), np.asarray(res[1]["labels"]))
    assert np.array_equal(np.asarray(res[0]["dists"]).view(np.uint32), np.asarray(res[1]["dists"]).view(np.uint32))


@pytest.mark.parametrize("metric", (0, 1), ids=("l2", "ip"))
def test_facade_slimq_convert(hs, tmp_path, metric):
    """tests/facade_slimq_convert.cpp: construct -> convertFromHNSW -> saveIndex, once with the two host calls and once after
    setBuildOnDevice; the program compares the two files, and the host's is the C ABI's."""
    exe = os.path.join(ROOT, "hnsw-slim_amd", "facade_slimq_convert")
    n, d, M, efc = 600, 64, 32, 128
    base = mixture(n, d, 21)
    cen = np.ascontiguousarray(base[:16])
    rf, cf, f_host, f_dev, hp, mine = (str(tmp_path / x) for x in ("rows.f32", "cen.f32", "host.bin", "dev.bin", "h.bin", "mine.bin"))
    base.tofile(rf); cen.tofile(cf)
    run = subprocess.run([exe, rf, str(n), str(d), str(M), str(efc), str(metric), "0", cf, "16", f_host, f_dev], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.split() == ["convert:", "1", "1", "1"], run.stdout
    hs.build_rabitq_hnsw(base, hp, metric=metric, M=M, ef_construction=efc, seed=100, threads=1)
    hs.convert_hnsw_to_slimq(hp, mine, d, cen, metric=metric, flip_seed=1, device=-1, threads=4)
    assert read(f_dev) == read(mine)
