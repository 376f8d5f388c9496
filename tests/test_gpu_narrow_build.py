"""The batched build over u8 / fp16 rows on the GPU (hs_build_hnsw_batched_rows, csrc/build_gpu_u8.hip / build_gpu_f16.hip; DESIGN.md
4s): the file it writes against the fp32 device build and the host twin of the widened rows, byte for byte, at the smallest shapes
at which each path of the narrow reads can go wrong."""
import os

import numpy as np
import pytest

from hsutil import GOLDEN, load_product, mixture

pytestmark = pytest.mark.gpu
L2, IP = 0, 1
U8, F16 = np.uint8, np.float16


@pytest.fixture(scope="module")
def hs():
    m = load_product()
    assert m.device_count() > 0, "no HIP device"
    return m


def rows(dtype, n, dim, kind="mixture"):
    if kind == "ties":        # nearly every comparison is between equal keys: libstdc++'s heap mechanics decide
        return np.random.default_rng(3).integers(0, 3, (n, dim)).astype(dtype)
    if kind == "f16_edges":   # both signs, subnormals, +-0, the largest finite values
        v = np.array([0.0, -0.0, 6e-8, -6e-8, 6.1e-5, -3.05e-5, 1, -1, 0.5, -3.25, 1000, 65504, -65504], np.float16)
        return v[np.random.default_rng(4).integers(0, len(v), (n, dim))]
    x = mixture(n, dim, 11, integer=dtype is U8)
    return np.clip(x, 0, 255).astype(U8) if dtype is U8 else x.astype(F16)


# (dtype, metric, n, dim, M, efC, extra)
CASES = [(t, m, 600, d, 8, 40, {}) for t in (U8, F16) for m in (L2, IP) for d in (16, 128, 144)]        # one step, a round, a round and a part
CASES += [(t, m, 300, d, 8, 40, {}) for t in (U8, F16) for m in (L2, IP) for d in (1, 3, 23, 100)]       # the general recipes; rows at odd offsets
CASES += [
    (U8, L2, 500, 16, 8, 40, {"kind": "ties"}),
    (F16, IP, 300, 16, 8, 40, {"kind": "f16_edges"}),
    (U8, L2, 1500, 32, 8, 100, {"scratch_ids": 64, "flagged": True}),     # the re-run instantiation
    (F16, L2, 400, 16, 31, 512, {}),                                      # the link kernel's full-list re-prune at the envelope's edge
    (U8, IP, 600, 16, 8, 40, {"batch_max": 64, "grow_div": 1}),           # long segments of incoming ids
    (F16, L2, 300, 20, 8, 40, {"labels": True}),
] + [(U8, L2, n, 16, 4, 20, {}) for n in (1, 2, 3, 65)]


@pytest.mark.parametrize("dtype,metric,n,dim,M,efc,extra", CASES,
                         ids=["-".join([c[0].__name__, "ip" if c[1] else "l2", f"n{c[2]}", f"d{c[3]}", f"M{c[4]}"] + sorted(c[6])) for c in CASES])
def test_narrow_build_equals_fp32_build_and_twin(hs, tmp_path, dtype, metric, n, dim, M, efc, extra):
    extra = dict(extra)
    base = rows(dtype, n, dim, extra.pop("kind", "mixture"))
    flagged = extra.pop("flagged", False)
    kw = dict(metric=metric, M=M, ef_construction=efc, **extra)
    if kw.pop("labels", False):
        kw["labels"] = np.arange(n, dtype=np.uint64)[::-1] * 7 + 5
    a, b, c = (str(tmp_path / f) for f in ("a.bin", "b.bin", "c.bin"))
    st = hs.build_hnsw_batched_rows(base, a, device=0, **kw)
    wide = base.astype(np.float32)
    hs.build_hnsw_batched(wide, b, device=0, **kw)
    hs.build_hnsw_batched(wide, c, device=-1, threads=8, **{k: v for k, v in kw.items() if k != "scratch_ids"})
    assert st["used_gpu"] and (not flagged or st["flagged_rows"] > 0)
    got = open(a, "rb").read()
    assert got == open(b, "rb").read(), "the narrow device build differs from the fp32 device build"
    assert got == open(c, "rb").read(), "the narrow device build differs from the host twin"


def test_batch_1_over_u8_rows_equals_the_reference(hs, tmp_path):
    g = np.load(os.path.join(GOLDEN, "l2_int_d16.npz"))
    narrow = g["base"][:600].astype(U8)
    assert np.array_equal(narrow, g["base"][:600])
    # (the fixture's rows hold -0.0 here and there, which u8 cannot carry: the serial build reads the widened rows, whose file
    #  differs from the fixture's prefix build in those sign bits of the stored rows and in nothing else)
    ser, dev = str(tmp_path / "s.bin"), str(tmp_path / "d.bin")
    hs.build_hnsw(narrow.astype(np.float32), ser, M=int(g["M"]), ef_construction=int(g["efC"]), branching_factor="4", seed=100, threads=1)
    st = hs.build_hnsw_batched_rows(narrow, dev, M=int(g["M"]), ef_construction=int(g["efC"]), device=0, batch_max=1)
    assert st["used_gpu"] and st["batches"] == 600
    assert open(dev, "rb").read() == open(ser, "rb").read()


@pytest.mark.parametrize("dtype", (U8, F16))
def test_search_on_the_narrow_built_file(hs, tmp_path, dtype):
    base, q = rows(dtype, 2000, 32), rows(dtype, 20, 32)[::-1].astype(np.float32)
    a, b = str(tmp_path / "a.bin"), str(tmp_path / "b.bin")
    hs.build_hnsw_batched_rows(base, a, device=0)
    hs.build_hnsw_batched(base.astype(np.float32), b, device=0)
    nx = hs.Index.load_narrow(a, hs.HS_KIND_HNSW, 32, hs.HS_ROWS_U8 if dtype is U8 else hs.HS_ROWS_F16)
    fx = hs.Index(b, hs.HS_KIND_HNSW, 32)
    nx.set_ef(40); fx.set_ef(40)
    want, got = (x.search_pq(q, 10, want_stats=True) for x in (fx, nx))
    assert (want["cnt"] == 10).all()
    for key in want:   # labels in output order, distance bits, counts, all four stats columns
        assert want[key].dtype == got[key].dtype and want[key].tobytes() == got[key].tobytes(), key
