"""The launch plan of a search batch (csrc/search_plan.cpp) through hs_debug_search_plan: which kernel serves pass 0 for every
combination of index state, call and diagnostic knob, the invariants every plan keeps, and the numbers of the bench shapes
pinned to recorded values.  Host only: no device is needed to make a plan."""
import json
import os

import pytest
from hsutil import load_product

hs = load_product()
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F32, F16, U8 = hs.HS_ROWS_F32, hs.HS_ROWS_F16, hs.HS_ROWS_U8
OVERFLOW, HAZARD = 1 << 2, 1 << 3   # 1 << ST_OVERFLOW, 1 << ST_HAZARD (csrc/engine.hpp)


def plan(**kw):
    """The plan of the base case -- a bare Slim index, threshold_level 0, tiles present, n = 1 000 000, dim 128, fp32 rows
    resident, ef 70, k 10, 10 000 queries, no knob set -- with the given members / knobs changed."""
    return hs.debug_search_plan(hs.plan_input(**kw))


FREE_U8 = dict(row_fmt=U8, f32_resident=0)
FREE_F16 = dict(row_fmt=F16, f32_resident=0)
# (members and knobs changed from the base case, kernel, further members of the plan)
CASES = [
    # bare index
    (dict(ef=70), "hs::flat_kernel", dict(split=1, rerun_select_mask=OVERFLOW | HAZARD)),
    (dict(nq=6143), "hs::flat_kernel", dict(split=0)),
    (dict(nq=6144), "hs::flat_kernel", dict(split=1)),
    (dict(ef=10, k=10), "hs::flat_kernel", {}),
    (dict(ef=200, k=200), "hs::strict_kernel", {}),   # the ef == k fast shape exists to 128 only, and flat requires `fast`
    (dict(ef=600), "hs::strict_kernel", dict(split=0, rerun_select_mask=OVERFLOW)),
    # what excludes the flat kernel
    (dict(dim=100), "hs::fast_kernel", {}),
    (dict(k=100, ef=128), "hs::fast_kernel", {}),
    (dict(has_uptile=0, maxlevel=3), "hs::fast_kernel", {}),
    (dict(has_deleted=1, ef=70), "hs::fast_kernel", {}),
    (dict(has_filter=1, ef=70), "hs::fast_kernel", {}),
    (dict(has_filter=1, ef=10, k=10), "hs::strict_kernel", {}),
    (dict(has_deleted=1, ef=10, k=10), "hs::strict_kernel", {}),
    # what forces the strict kernel
    (dict(threshold_level=1), "hs::strict_kernel", {}),
    (dict(has_tile0=0), "hs::strict_kernel", {}),
    (dict(exact_order=1), "hs::strict_kernel", {}),
    (dict(want_raw=1), "hs::strict_kernel", {}),
    # row formats and residency
    (dict(row_fmt=U8), "hs::flat_kernel_u8", dict(rows=U8, rerun_rows=F32)),
    (dict(row_fmt=U8, has_deleted=1), "hs::fast_kernel", dict(rows=F32, rerun_rows=F32)),
    (dict(FREE_U8), "hs::flat_kernel_u8", dict(rows=U8, rerun_rows=U8)),
    (dict(FREE_U8, has_deleted=1), "hs::fast_kernel_u8", dict(rows=U8, rerun_rows=U8)),
    (dict(FREE_U8, ef=600), "hs::strict_kernel_u8", dict(rows=U8, rerun_rows=U8)),
    (dict(FREE_F16), "hs::flat_kernel_f16", dict(rows=F16, rerun_rows=F16)),
    (dict(FREE_F16, has_deleted=1), "hs::fast_kernel_f16", dict(rows=F16, rerun_rows=F16)),
    (dict(FREE_F16, ef=600), "hs::strict_kernel_f16", dict(rows=F16, rerun_rows=F16)),
    # knobs
    (dict(kernel="fast"), "hs::fast_kernel", {}),
    (dict(kernel="lean", ef=70), "hs::lean_kernel", dict(hash_fill_shift=3)),
    (dict(kernel="lean", ef=32), "hs::fast_kernel", {}),
    (dict(FREE_U8, kernel="lean"), "hs::fast_kernel_u8", {}),
    (dict(lean_min_ef=100000), "hs::fast_kernel", {}),
    (dict(order=0, nq=10_000), "hs::flat_kernel", dict(split=0)),
    (dict(order=1, nq=300), "hs::flat_kernel", dict(split=1)),
    (dict(order=2), "hs::flat_kernel", dict(split=1, skip_order=0)),
    (dict(order=2, kernel="fast"), "hs::fast_kernel", dict(split=1, skip_order=1)),
    (dict(vis16=0, kernel="fast"), "hs::fast_kernel", dict(vis_bits=0)),
    (dict(vis16=0, has_deleted=1), "hs::fast_kernel", dict(vis_bits=0)),
]
FAMILY = {"flat": hs.HS_PLAN_FLAT, "lean": hs.HS_PLAN_LEAN, "fast": hs.HS_PLAN_FAST, "strict": hs.HS_PLAN_STRICT}


@pytest.mark.parametrize("case", CASES, ids=[",".join(f"{k}={v}" for k, v in c[0].items()) for c in CASES])
def test_kernel_choice_and_plan_invariants(case):
    change, name, want = case
    p = plan(**change)
    assert p["name"] == name, p
    assert p["family"] == FAMILY[name.split("::")[1].split("_")[0]], p
    for member, v in want.items():
        assert p[member] == v, (member, p)
    # what every plan keeps
    assert 0 < p["lds_bytes"] <= 160 * 1024, p
    assert p["cand_cap"] % 2 == 0 and p["rerun_cand_cap"] % 2 == 0, p
    if p["vis_bits"] == 0:   # the 32-bit form of the visited set
        assert p["hash_slots"] % 64 == 0, p
    assert p["rerun_hash_slots"] % 64 == 0, p
    assert p["ef"] == max(change.get("ef", 70), change.get("k", 10))
    # tier-2 scratch per query: visited set, candidate heap (8 B entries), insertion log (8 B entries), hop counts (bytes), the
    # flat kernel's parking area -- in words (csrc/search_plan.hpp)
    assert p["spill_stride"] == 8192 + 2 * 4096 + 2 * p["log_cap"] + p["hop_cap"] // 4 + 2048, p
    if not p["split"]:
        assert not p["skip_order"]
    if p["family"] == hs.HS_PLAN_FLAT:
        assert p["fl_ok"] and p["hash_slots"] == 4 * p["fl_nb"] and p["vis_bits"] == p["fl_bits"], p
    if p["family"] == hs.HS_PLAN_STRICT:
        assert not p["split"] and p["rerun_select_mask"] == OVERFLOW, p
    else:
        assert p["rerun_select_mask"] == OVERFLOW | HAZARD, p


def test_a_knob_changes_nothing_it_does_not_name():
    """HS_ORDER=2 drops the order launch of the fast family only; the flat kernel keeps it."""
    for kw in (dict(), dict(kernel="fast"), dict(has_deleted=1)):
        a, b = plan(**kw), plan(order=2, **kw)
        for member in a:
            if member not in ("split", "skip_order"):
                assert a[member] == b[member], (kw, member)
        assert b["split"] == 1 and b["skip_order"] == (b["family"] == hs.HS_PLAN_FAST)


def test_plan_refusals():
    with pytest.raises(hs.HsError) as e:
        plan(ef=(1 << 20) + 1)
    assert e.value.status == hs.HS_ERR_INVALID and "ef too large" in str(e.value)
    with pytest.raises(hs.HsError) as e:
        plan(dim=100_000)
    assert e.value.status == hs.HS_ERR_CAPACITY


GRID = [(n, ef, nq) for n in (50_000, 1_000_000, 100_000_000) for ef in (32, 70, 128, 256, 512) for nq in (300, 1250, 10_000)]


def test_bench_shapes_keep_their_recorded_plans():
    """Every member of the plan, for the base case over index size x ef x launch size, equals what was recorded while the plan
    agreed, launch by launch and argument by argument, with the launch decisions it replaced (golden/search_plan_values.json)."""
    gold = json.load(open(os.path.join(GOLDEN, "search_plan_values.json")))["plans"]
    assert [(g["n"], g["ef"], g["nq"]) for g in gold] == GRID
    for g in gold:
        assert plan(n=g["n"], ef=g["ef"], nq=g["nq"]) == g["plan"], (g["n"], g["ef"], g["nq"])


def test_flat_plan_is_the_earlier_hook_s():
    """The flat kernel's visited-set plan equals what hs_debug_flat_plan -- the hook this one replaced, which planned for a
    stand-in index of dim 128 -- returned over the same grid (golden/flat_plan_parent.json)."""
    gold = json.load(open(os.path.join(GOLDEN, "flat_plan_parent.json")))["plans"]
    assert [(g["n"], g["ef"], g["nq"]) for g in gold] == GRID
    for g in gold:
        p = plan(n=g["n"], ef=g["ef"], nq=g["nq"])
        got = dict(nb=p["fl_nb"], mul=p["fl_mul"], sh=p["fl_sh"], bits=p["fl_bits"], ok=p["fl_ok"])
        assert got == {k: g[k] for k in got}, (g, p)
