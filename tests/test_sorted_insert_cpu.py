"""The flat kernel's rank-free sorted insert (csrc/sorted_insert.hpp), compiled for the host: csrc/sorted_insert_test.cpp replays
the lane-wise function over the 64 x S ranks of a wave against std::upper_bound + insert (equal keys stay in front) and against
the rank path the kernel used before, S in {1, 2, 3, 4, 6, 8}, full and padded sets, keys equal to existing keys and to the bound,
sequences of up to 8 insertions, every rank of keys and ids compared after every insertion."""
import os
import re
import subprocess

from hsutil import ROOT


def test_lanewise_insert_equals_upper_bound_insert():
    d = os.path.join(ROOT, "hnsw-slim_amd")
    subprocess.check_call(["make", "-C", d, "sorted_insert_test"])
    out = subprocess.run([os.path.join(d, "sorted_insert_test")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    m = re.search(r"sorted_insert ok: S in \{1,2,3,4,6,8\}, (\d+) rank comparisons", out.stdout)
    assert m and int(m.group(1)) > 1_000_000, out.stdout


def test_kernel_uses_the_tested_function():
    """The device code calls the function the host test drives, for every shape but the d = 960 ones (which keep the rank path)."""
    src = open(os.path.join(ROOT, "hnsw-slim_amd", "csrc", "flat_search.hip")).read()
    assert '#include "sorted_insert.hpp"' in src and "sorted_insert_lane<S>(tk, ti, upk, upi, kj, idj)" in src
    assert "constexpr bool kRankFree = D16 <= 8;" in src
