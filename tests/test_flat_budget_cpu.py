"""resource_usage.txt against the budget of the commit before the rank-free insert (tests/golden/flat_kernel_budget.txt, recorded
from a build of that commit with the same compiler): every hs::flat_kernel / flat_kernel_u8 / flat_kernel_f16 shape keeps at least
its waves/SIMD and at most its scratch bytes per lane.  The headline shape (L2, S = 2, d = 128): 5 waves, 12 bytes then."""
import os
import re
import subprocess

from hsutil import GOLDEN, ROOT

HEADLINE = "_ZN2hs11flat_kernelILi0ELi2ELi8EEEvNS_8DevIndexENS_10SearchArgsE"


def _built():
    path = os.path.join(ROOT, "hnsw-slim_amd", "resource_usage.txt")
    if not os.path.exists(path):
        subprocess.check_call(["make", "-C", os.path.dirname(path), "-B", "libhnsw_slim_amd.so"])
    kern = {}
    for m in re.finditer(r"Function Name: (\S+)\s+VGPRs: (\d+)\s+ScratchSize \[bytes/lane\]: (\d+)\s+Occupancy \[waves/SIMD\]: (\d+)", open(path).read()):
        kern[m.group(1)] = (int(m.group(4)), int(m.group(3)))
    return kern


def _budget():
    out = {}
    for line in open(os.path.join(GOLDEN, "flat_kernel_budget.txt")):
        if line.strip() and not line.startswith("#"):
            name, waves, scratch = line.split()
            out[name] = (int(waves), int(scratch))
    return out


def test_every_flat_shape_keeps_waves_and_scratch():
    kern, budget = _built(), _budget()
    assert len(budget) == 180 and budget[HEADLINE] == (5, 12)
    worse = []
    for name, (waves, scratch) in sorted(budget.items()):
        assert name in kern, f"{name} missing from resource_usage.txt"
        if kern[name][0] < waves or kern[name][1] > scratch:
            worse.append(f"{name}: {kern[name][0]} waves/SIMD, {kern[name][1]} B scratch (budget {waves} waves, {scratch} B)")
    assert not worse, "\n".join(worse)
    # no flat shape exists outside the budget either (a new shape needs a budget of its own)
    assert {n for n in kern if re.match(r"_ZN2hs\d+flat_kernel(_u8|_f16)?I", n)} == set(budget)
