"""convertFromHNSW on the GPU (hs_convert_slim_gpu, csrc/convert_gpu.hip) against the oracle's independent restatement
(oracle/hs_oracle_convert.hpp) and the CPU harness (hs_convert_slim, threads=1): the output FILE must be byte-identical to both --
every distance, every by-distance std::sort (libstdc++ tie order included), every pruning decision, the reverse-edge union and the
re-prune of over-full lists taken the same way."""
import os

import numpy as np
import pytest

from hsutil import GOLDEN, equal_key_star, load_chal_encode, load_product, mixture, write_vanilla_level0

pytestmark = pytest.mark.gpu
L2, IP = 0, 1


@pytest.fixture(scope="module")
def hs():
    m = load_product()
    assert m.device_count() > 0
    return m


def _same_file(hs, oracle, hp, dim, metric, tmp_path, expect_gpu=True, **kw):
    """GPU file == oracle file == CPU harness file.  expect_gpu: the shape is inside the device envelope, so the GPU entry must
    have run (a silent fall-back to the CPU conversion cannot pass); False: it must have declined.  Returns the oracle's stats."""
    a, b, o = str(tmp_path / "cpu.slim"), str(tmp_path / "gpu.slim"), str(tmp_path / "oracle.slim")
    st = oracle.convert_slim(hp, o, dim, metric=metric, **kw)
    hs.convert_slim(hp, a, dim, metric=metric, threads=1, **kw)
    used, ms = hs.convert_slim_gpu(hp, b, dim, metric=metric, **kw)
    assert used == expect_gpu, f"GPU entry used={used}, expected {expect_gpu}"
    want = open(o, "rb").read()
    assert open(b, "rb").read() == want, f"GPU file != oracle file {kw}"
    assert open(a, "rb").read() == want, f"CPU harness file != oracle file {kw}"
    return st


@pytest.mark.parametrize("name,metric,dim", [("l2_cont_d32", L2, 32), ("l2_int_d16", L2, 16), ("ip_d48", IP, 48), ("l2_cont_d20", L2, 20),
                                             ("l2_cont_d21", L2, 21), ("l2_cont_d10", L2, 10), ("ip_d20", IP, 20), ("ip_d21", IP, 21),
                                             ("ip_d10", IP, 10), ("l2_int_d16_del", L2, 16)])
def test_gpu_convert_is_byte_identical_on_golden_graphs(hs, oracle, tmp_path, name, metric, dim):
    hp = os.path.join(GOLDEN, f"{name}.hnsw.bin")
    _same_file(hs, oracle, hp, dim, metric, tmp_path)
    _same_file(hs, oracle, hp, dim, metric, tmp_path, threshold_level=1)
    _same_file(hs, oracle, hp, dim, metric, tmp_path, top_degree_M0=16, low_degree_m0=4, top_degree_M=8, low_degree_m=2, top_degree_percent=0.3)


@pytest.mark.parametrize("dim,metric,integer", [(128, L2, True), (96, L2, False), (64, IP, False), (100, L2, True)])
def test_gpu_convert_m16_graphs_with_ties(hs, oracle, tmp_path, dim, metric, integer):
    """M=16: maxM0 == 32, the top of the device envelope; level-0 lists of up to 32 ids (std::sort's introsort branch), tiny
    integer range => many equal distances; hubs whose reverse-edge union exceeds the capacity get re-pruned."""
    if integer:
        base = mixture(30000, dim, 5, lo=0, hi=6, sigma=1.5, integer=True, n_clusters=8)
    else:
        base = mixture(30000, dim, 6, lo=-1, hi=1, sigma=0.4, n_clusters=8)
    if metric == IP:
        base /= np.linalg.norm(base, axis=1, keepdims=True)
    hp = str(tmp_path / "h.bin")
    hs.build_hnsw(base.astype(np.float32), hp, metric=metric, M=16, ef_construction=100, threads=8)
    assert load_chal_encode().parse_vanilla(open(hp, "rb").read())["maxM0"] == 32
    st = _same_file(hs, oracle, hp, dim, metric, tmp_path)
    _same_file(hs, oracle, hp, dim, metric, tmp_path, low_degree_m0=24, top_degree_percent=0.1)
    _same_file(hs, oracle, hp, dim, metric, tmp_path, top_degree_M0=32, low_degree_m0=32, top_degree_M=32, low_degree_m=32)
    assert st["n_reprune"] > 0
    if integer:
        assert st["n_eqkey_over16"] > 0


def test_gpu_convert_declines_wide_graphs(hs, oracle, tmp_path):
    base = mixture(3000, 32, 7)
    hp = str(tmp_path / "h40.bin")
    hs.build_hnsw(base, hp, M=40, ef_construction=80, threads=8)     # maxM0 = 80 > 32: CPU path, same file
    _same_file(hs, oracle, hp, 32, L2, tmp_path, expect_gpu=False)


@pytest.mark.parametrize("spokes", (16, 17, 32))
def test_gpu_convert_equal_key_lists_at_the_rank_sort_boundary(hs, oracle, tmp_path, spokes):
    """A level-0 list of exactly 16 / 17 / 32 ids, all at one distance, pruned to 8: up to 16 entries the rank sort gives
    libstdc++'s order (insertion sort, stable), from 17 the ties take the std_sort emulation (convert_gpu.hip:96-119) and introsort's
    partition decides which 8 stay."""
    rows, lists = equal_key_star(spokes)
    hp = str(tmp_path / "star.bin")
    write_vanilla_level0(hp, rows, lists, M=16)
    st = _same_file(hs, oracle, hp, 16, L2, tmp_path, low_degree_m0=8)
    kept = [int(x) for x in load_chal_encode().parse_slim(open(str(tmp_path / "oracle.slim"), "rb").read(), 16)["lists"][0][0]]
    assert (kept == list(range(1, 9))) == (spokes <= 16), "premise: beyond 16 entries the tie order is not the list order"
    assert st["n_eqkey_over16"] == (spokes > 16)


@pytest.mark.parametrize("dim", (32, 20))
@pytest.mark.parametrize("metric", (L2, IP))
def test_gpu_convert_distance_paths(hs, oracle, tmp_path, dim, metric):
    """dim % 16 == 0: four lanes per row; otherwise the reference's SIMD4 / residual recipes on one lane per row."""
    base = mixture(4000, dim, 8 + dim, lo=-1, hi=1, sigma=0.5)
    if metric == IP:
        base /= np.linalg.norm(base, axis=1, keepdims=True)
    hp = str(tmp_path / "h.bin")
    hs.build_hnsw(base.astype(np.float32), hp, metric=metric, M=16, ef_construction=100, threads=8)
    _same_file(hs, oracle, hp, dim, metric, tmp_path)
    _same_file(hs, oracle, hp, dim, metric, tmp_path, threshold_level=1, top_degree_percent=0.2)


def test_gpu_convert_declines_a_union_beyond_its_buffer(hs, oracle, tmp_path):
    """One centre and 3000 points on a sphere around it (d=128: the points are more than a radius apart, the centre one radius away):
    every point keeps the centre, whose reverse-edge union outgrows kCvUnionCap (2048).  The device path must decline
    (needs_host) and the host conversion write the oracle's file."""
    rng = np.random.default_rng(9)
    pts = rng.standard_normal((3000, 128)).astype(np.float32)
    pts *= np.float32(10.0) / np.linalg.norm(pts, axis=1, keepdims=True).astype(np.float32)
    base = np.concatenate([np.zeros((1, 128), np.float32), pts])
    hp = str(tmp_path / "h.bin")
    hs.build_hnsw(base, hp, M=16, ef_construction=100, threads=8)
    st = _same_file(hs, oracle, hp, 128, L2, tmp_path, expect_gpu=False)
    assert st["max_union"] > 2048
