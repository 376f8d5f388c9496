"""Filter sets, host side (no device): hs_filter_pack / hs_filter_row_words against numpy.packbits(bitorder="little")."""
import numpy as np
import pytest

from hsutil import load_product


@pytest.fixture(scope="module")
def hs():
    return load_product()


@pytest.mark.parametrize("n", [1, 31, 32, 33, 127, 128, 2003])
def test_row_words(hs, n):
    """ceil(n / 32) words rounded up to a multiple of 4: every row starts 16-byte aligned."""
    rw = hs.filter_row_words(n)
    assert rw == (-(-n // 32) + 3) // 4 * 4
    assert rw % 4 == 0 and rw * 32 >= n and (rw - 4) * 32 < n


@pytest.mark.parametrize("nf", [1, 3])
@pytest.mark.parametrize("n", [1, 31, 32, 33, 127, 128, 2003])
def test_pack_vs_packbits(hs, n, nf):
    rng = np.random.default_rng(100 * n + nf)
    allowed = (rng.random((nf, n)) < 0.5).astype(np.uint8)
    allowed[0, n - 1] = 1                     # the last id of a row: the tail bit n % 32 - 1
    allowed *= rng.integers(1, 256, size=allowed.shape, dtype=np.uint8)   # any non-zero byte means "allowed"
    rw = hs.filter_row_words(n)
    words = hs.filter_pack(allowed)
    assert words.dtype == np.uint32 and words.shape == (nf, rw)          # row stride = hs_filter_row_words(n)
    want = np.zeros((nf, rw * 4), np.uint8)
    pb = np.packbits(allowed != 0, axis=1, bitorder="little")
    want[:, :pb.shape[1]] = pb
    assert np.array_equal(words.view(np.uint8), want)                    # little-endian words: byte b of a row = ids 8 b .. 8 b + 7
    # padding: bits n .. 32 rw of every row are zero (packbits pads a byte; the words beyond it are checked here too)
    bits = np.unpackbits(words.view(np.uint8), axis=1, bitorder="little")
    assert not bits[:, n:].any()
    assert np.array_equal(bits[:, :n], (allowed != 0).astype(np.uint8))


def test_pack_one_row_and_none_all(hs):
    """A 1-d mask is one filter; all-allowed and none-allowed rows."""
    n = 100
    assert hs.filter_pack(np.zeros(n, np.uint8)).shape == (1, 4)
    assert not hs.filter_pack(np.zeros(n, np.uint8)).any()
    w = hs.filter_pack(np.ones(n, np.uint8))[0]
    assert w.tolist() == [0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xF]
