"""The kernel a search runs is the one the launch plan names: hs_last_kernel after the search against
hs_debug_search_plan(hs_debug_plan_input(index, ...)) -- the plan made from the live index through the function every launch
uses -- over ef = k, the flat kernel's range and beyond it, crossed with the index states that move the choice.  The answers are
those of the same search in the reference's order (set_exact_order), and the oracle's where that is the state itself."""
import struct

import numpy as np
import pytest

from hsutil import Oracle, load_product, mixture
from test_gpu_parity import _pq_sorted

pytestmark = pytest.mark.gpu
N, D, NQ, K = 2000, 32, 64, 10
EFS = (10, 70, 600)
STATES = ("bare", "delete mark", "filter set", "exact order", "u8 rows", "u8 rows, fp32 dropped")


@pytest.fixture(scope="module")
def env(tmp_path_factory):
    hs = load_product()
    tmp = tmp_path_factory.mktemp("search_plan")
    x = mixture(N + NQ, D, seed=9, integer=True)
    hp, sp, dp, dsp = (str(tmp / name) for name in ("h.bin", "s.bin", "h_del.bin", "s_del.bin"))
    hs.build_hnsw(x[:N], hp, M=8, ef_construction=60, threads=4)
    hs.convert_slim(hp, sp, D, threads=4)
    # markDelete(7) on the saved vanilla index (hnswalg.h:917-930: bit 0 of byte 2 of the node's level-0 record), then converted
    raw = bytearray(open(hp, "rb").read())
    offset_level0, = struct.unpack_from("<Q", raw, 0)
    size_per_element, = struct.unpack_from("<Q", raw, 24)
    raw[96 + offset_level0 + 7 * size_per_element + 2] |= 1
    open(dp, "wb").write(raw)
    hs.convert_slim(dp, dsp, D, threads=4)
    return hs, Oracle(), sp, dsp, np.ascontiguousarray(x[N:])


def same_answers(a, b, what):
    assert np.array_equal(a["cnt"], b["cnt"]), what
    assert _pq_sorted(a["dists"], a["labels"], a["cnt"]) == _pq_sorted(b["dists"], b["labels"], b["cnt"]), what


@pytest.mark.parametrize("state", STATES)
def test_last_kernel_is_the_planned_one(env, state):
    hs, oracle, sp, dsp, q = env
    path = dsp if state == "delete mark" else sp
    ix = hs.Index(path, hs.HS_KIND_SLIM, D)
    assert ix.info()["has_deleted"] == (1 if state == "delete mark" else 0)
    fs = None
    if state == "filter set":
        allowed = (np.arange(N) % 3 != 0).astype(np.uint8)
        fs = hs.FilterSet.create(ix, 1)
        fs.write(0, allowed)
    if state.startswith("u8 rows"):
        ix.set_row_format(hs.HS_ROWS_U8)
        ix.set_f32_resident(state == "u8 rows")
    foq = np.zeros(NQ, np.uint32)

    def search():
        return ix.search_filter_set(q, K, fs, foq) if fs else ix.search_pq(q, K)

    seen = set()
    for ef in EFS:
        ix.set_ef(ef)
        ix.set_exact_order(state == "exact order")
        got = search()
        kernel = ix.last_kernel()
        plan = hs.debug_search_plan(hs.debug_plan_input(ix, K, NQ, has_filter=fs is not None))
        assert kernel == plan["name"], (state, ef, plan)
        seen.add(kernel)
        if state == "exact order":
            ox = oracle.load(path, "slim", 0, D)
            ox.set_ef(ef)
            want = ox.search_pq(q, K)
        else:
            ix.set_exact_order(True)
            want = search()
            assert ix.last_kernel().startswith("hs::strict_kernel")
        same_answers(got, want, (state, ef))
    # the states do move the choice: what each is expected to reach over the three ef
    assert seen == {"bare": {"hs::flat_kernel", "hs::strict_kernel"}, "delete mark": {"hs::fast_kernel", "hs::strict_kernel"},
                    "filter set": {"hs::fast_kernel", "hs::strict_kernel"}, "exact order": {"hs::strict_kernel"},
                    "u8 rows": {"hs::flat_kernel_u8", "hs::strict_kernel"},
                    "u8 rows, fp32 dropped": {"hs::flat_kernel_u8", "hs::strict_kernel_u8"}}[state], seen
