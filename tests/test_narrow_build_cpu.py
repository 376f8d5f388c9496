"""hs_build_hnsw_batched_rows without a device: the entry, the widening and the file assembly on the host twin against
hs_build_hnsw_batched of the widened rows; the refusals; the header's declaration as C."""
import os
import subprocess

import numpy as np
import pytest

from hsutil import ROOT, load_product, mixture


@pytest.fixture(scope="module")
def hs():
    return load_product()


@pytest.mark.parametrize("metric", (0, 1))
@pytest.mark.parametrize("dim", (16, 23))
@pytest.mark.parametrize("dtype", (np.uint8, np.float16))
def test_host_twin_over_narrow_rows_equals_the_widened_build(hs, tmp_path, dtype, dim, metric):
    x = mixture(400, dim, 5, integer=dtype is np.uint8)
    base = np.clip(x, 0, 255).astype(dtype) if dtype is np.uint8 else (x - 70).astype(dtype)
    labels = np.arange(400, dtype=np.uint64) * 3 + 1
    a, b = str(tmp_path / "a.bin"), str(tmp_path / "b.bin")
    kw = dict(metric=metric, M=8, ef_construction=40, device=-1, threads=4, labels=labels)
    st = hs.build_hnsw_batched_rows(base, a, **kw)
    want = hs.build_hnsw_batched(base.astype(np.float32), b, **kw)
    assert not st["used_gpu"] and st["batches"] == want["batches"]
    assert open(a, "rb").read() == open(b, "rb").read()


def test_refusals(hs, tmp_path):
    out = str(tmp_path / "x.bin")
    u8 = np.zeros((10, 16), np.uint8)
    for base, fmt in ((u8, hs.HS_ROWS_F32), (u8, 7), (np.zeros((10, 16), np.float32), None), (np.zeros((0, 16), np.uint8), None)):
        with pytest.raises(hs.HsError) as e:
            hs.build_hnsw_batched_rows(base, out, row_format=fmt)
        assert e.value.status == hs.HS_ERR_INVALID
    opts = hs.HsBatchBuildOpts(-1, 1, 0, 0, 0)
    assert hs.lib().hs_build_hnsw_batched_rows(None, hs.HS_ROWS_U8, None, 10, 16, 0, 8, 40, b"4", 100, opts, out.encode(), None) == hs.HS_ERR_INVALID
    for bad in (np.nan, np.inf, -np.inf):
        f16 = np.ones((10, 16), np.float16)
        f16[7, 3] = bad
        with pytest.raises(hs.HsError) as e:
            hs.build_hnsw_batched_rows(f16, out)
        assert e.value.status == hs.HS_ERR_UNSUPPORTED and "row 7 " in hs.last_error() and "component 3" in hs.last_error()
    assert not os.path.exists(out)


def test_header_declares_the_entry_as_c(tmp_path):
    hdr = os.path.join(ROOT, "include", "hnsw_slim_amd.h")
    assert "hs_build_hnsw_batched_rows(const void *base, int row_format" in open(hdr).read()
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", hdr])
