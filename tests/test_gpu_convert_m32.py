"""convertFromHNSW on the GPU (hs_convert_slim_gpu, csrc/convert_gpu.hip) for the reference's default graph, M = 32: maxM0 = 64,
maxM = 32, so the pruned and final lists hold up to 64 ids and the kernels run with 64 slots per task (ConvertInput::keep).  As
tests/test_gpu_convert.py: the oracle's file (oracle/hs_oracle_convert.hpp), the CPU harness's (hs_convert_slim, threads=1) and the
GPU entry's must be byte-identical, and the GPU entry must have run -- a fall-back to the host conversion cannot pass.  The
premises are about the oracle alone: they say that the graphs reach the lists of 33..64 ids, the std_sort emulation on them and
the re-prune to a limit of 64."""
import numpy as np
import pytest

from hsutil import equal_key_star, load_chal_encode, load_product, mixture, write_vanilla_level0

pytestmark = pytest.mark.gpu
L2, IP = 0, 1
DEFAULTS = dict()                                   # 32 / 8 / 16 / 4
WIDE = dict(top_degree_M0=64, low_degree_m0=48, top_degree_M=32, low_degree_m=24)


@pytest.fixture(scope="module")
def hs():
    m = load_product()
    assert m.device_count() > 0
    return m


def _same_file(hs, oracle, hp, dim, metric, tmp_path, **kw):
    """GPU file == oracle file == CPU harness file, and the GPU entry ran.  Returns (the oracle's stats, the oracle's file)."""
    a, b, o = str(tmp_path / "cpu.slim"), str(tmp_path / "gpu.slim"), str(tmp_path / "oracle.slim")
    st = oracle.convert_slim(hp, o, dim, metric=metric, **kw)
    hs.convert_slim(hp, a, dim, metric=metric, threads=1, **kw)
    used, ms = hs.convert_slim_gpu(hp, b, dim, metric=metric, **kw)
    assert used, f"GPU entry used={used}: the device path declined {kw}"
    want = open(o, "rb").read()
    assert open(b, "rb").read() == want, f"GPU file != oracle file {kw}"
    assert open(a, "rb").read() == want, f"CPU harness file != oracle file {kw}"
    return st, want


def _max_degree0(raw, dim):
    return max(len(l[0]) for l in load_chal_encode().parse_slim(raw, dim)["lists"])


def _rows(name):
    """(n and seed of the last two: the smallest of n in 6000, 9000, .. and then of the seeds from 8 / 9 up at which the oracle
    re-prunes a list for one of the three parameter sets; at n = 6000 it does for none of the seeds up to 19)"""
    if name == "l2_d32":
        return mixture(6000, 32, 7), L2
    if name == "ip_d48":
        base = mixture(9000, 48, 8, lo=-1, hi=1, sigma=0.5)
        return (base / np.linalg.norm(base, axis=1, keepdims=True)).astype(np.float32), IP
    return mixture(9000, 20, 15, lo=-1, hi=1, sigma=0.5), L2   # dim % 16 != 0: the one-lane-per-row distance path


@pytest.mark.parametrize("name", ("l2_d32", "ip_d48", "l2_d20"))
def test_gpu_convert_m32_mixture_graphs(hs, oracle, tmp_path, name):
    base, metric = _rows(name)
    dim = base.shape[1]
    hp = str(tmp_path / "h.bin")
    hs.build_hnsw(base, hp, metric=metric, M=32, ef_construction=100, threads=8)
    assert load_chal_encode().parse_vanilla(open(hp, "rb").read())["maxM0"] == 64
    reprunes = []
    for kw in (DEFAULTS, dict(threshold_level=1), dict(WIDE, top_degree_percent=0.2)):
        st, raw = _same_file(hs, oracle, hp, dim, metric, tmp_path, **kw)
        reprunes.append(st["n_reprune"])
    assert _max_degree0(raw, dim) > 32, "premise: the 64 / 48 / 32 / 24 set leaves level-0 lists above 32 ids"
    assert max(reprunes) > 0, "premise: some union outgrew its capacity and was pruned again"


def test_gpu_convert_m32_tie_heavy_rows(hs, oracle, tmp_path):
    """Integer rows in a tiny range: equal keys on lists of up to 64 ids (the std_sort emulation on one lane), hubs re-pruned to a
    limit of 64."""
    base = mixture(20000, 128, 5, lo=0, hi=6, sigma=1.5, integer=True, n_clusters=8)
    hp = str(tmp_path / "h.bin")
    hs.build_hnsw(base, hp, M=32, ef_construction=100, threads=8)
    assert load_chal_encode().parse_vanilla(open(hp, "rb").read())["maxM0"] == 64
    for kw in (DEFAULTS, WIDE):
        st, _ = _same_file(hs, oracle, hp, 128, L2, tmp_path, **kw)
        assert st["n_eqkey_over16"] > 0 and st["n_reprune"] > 0, f"premise {kw}: {st}"


@pytest.mark.parametrize("spokes", (33, 64))
def test_gpu_convert_m32_equal_key_stars(hs, oracle, tmp_path, spokes):
    """A level-0 list of 33 / 64 ids, all at one distance: pruned to 8, introsort's partition decides which stay; pruned to 40, more
    than 32 of an all-ties list are kept."""
    ce = load_chal_encode()
    rows, lists = equal_key_star(spokes, dim=32)
    hp = str(tmp_path / "star.bin")
    write_vanilla_level0(hp, rows, lists, M=32)
    st, raw = _same_file(hs, oracle, hp, 32, L2, tmp_path, low_degree_m0=8)
    kept = [int(x) for x in ce.parse_slim(raw, 32)["lists"][0][0]]
    assert len(kept) == 8 and kept != list(range(1, 9)), "premise: the tie order comes from introsort, not from the list order"
    assert st["n_eqkey_over16"] == 1
    st, raw = _same_file(hs, oracle, hp, 32, L2, tmp_path, low_degree_m0=40, top_degree_M0=64)
    assert len(ce.parse_slim(raw, 32)["lists"][0][0]) == min(spokes, 40)   # premise: more than 32 kept
