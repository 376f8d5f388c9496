"""The launch plan of a search batch (csrc/search_plan.cpp) through hs_debug_search_plan: which kernel serves pass 0 for every
combination of index state, call and diagnostic knob, the invariants every plan keeps, and the numbers of the bench shapes
pinned to recorded values; and the fast kernel's shape table (hs_debug_fast_shape) against the documented compiled dims and the
instantiations the build holds.  Host only: no device is needed to make a plan."""
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


# ---- the fast kernel's shape table (csrc/search_plan.cpp fast_shape, hs_debug_fast_shape) --------------------------------------------
L2, IP = 0, 1
# DESIGN.md 4a / the comments of fast_shape: dim -> d16 of every distance pass compiled for a bare index, and for one with delete
# marks or under a filter set
COMPILED = {(L2, True): {64: 4, 96: 6, 128: 8, 256: 16, 512: 32, 768: 48, 960: 60, 1024: 64, 100: -25},
            (IP, True): {512: 32, 768: 48, 1024: 64, 1536: 96, 100: -25},
            (L2, False): {128: 8},
            (IP, False): {}}
# ef classes of the slots per lane, at both ends of each; k = ef where the plan admits the fast kernel with it (bare, ef <= 128)
EF_SLOTS = [(1, 1), (64, 1), (65, 2), (128, 2), (129, 4), (256, 4), (257, 8), (512, 8)]


def fast_shape(metric, dim, ef, k, bare=True):
    return hs.debug_fast_shape(metric, dim, ef, k, bare)


def fast_shapes_reachable():
    """Every (metric, slots, d16, wb, bare) fast_shape returns over dims 4..1600 for a call the plan hands to the fast kernel:
    ef > k, or ef == k <= 128 on a bare index (beam_search.hip fast_supported)."""
    out = set()
    for metric in (L2, IP):
        for bare in (True, False):
            for dim in range(4, 1601):
                for ef, _ in EF_SLOTS:
                    for k in ([ef - 1] if ef > 1 else []) + ([ef] if bare and ef <= 128 else []):
                        s = fast_shape(metric, dim, ef, k, bare)
                        out.add((metric, s["slots"], s["d16"], s["wb"], int(bare)))
    return out


def test_fast_shape_compiled_dims_are_the_documented_ones():
    for (metric, bare), table in COMPILED.items():
        got = {}
        for dim in range(4, 1601):
            d16 = fast_shape(metric, dim, 100, 10, bare)["d16"]
            if d16 not in (0, -1):
                got[dim] = d16
                assert (d16 > 0 and 16 * d16 == dim) or (d16 < -1 and dim % 16 != 0 and -4 * d16 == dim), (metric, bare, dim, d16)
            else:
                assert d16 == (0 if dim % 16 == 0 else -1), (metric, bare, dim, d16)
        assert got == table, (metric, bare)
    # the distance pass is a property of (metric, dim, bare) alone
    for metric, dim in ((L2, 128), (L2, 100), (IP, 768), (L2, 160), (IP, 77)):
        for bare in (True, False):
            assert len({fast_shape(metric, dim, ef, k, bare)["d16"] for ef, _ in EF_SLOTS for k in (1, ef)}) == 1


def test_fast_shape_slots_and_boundary_watch_follow_ef_and_k():
    for metric, dim in ((L2, 128), (L2, 100), (L2, 160), (L2, 33), (IP, 768), (IP, 384)):
        for bare in (True, False):
            for ef in range(1, 513):
                want = 1 if ef <= 64 else 2 if ef <= 128 else 4 if ef <= 256 else 8
                for k in {1, max(ef - 1, 1), ef}:
                    s = fast_shape(metric, dim, ef, k, bare)
                    assert s["slots"] == want and s["wb"] == int(bare and k == ef), (metric, dim, bare, ef, k, s)
            # the search runs with max(ef, k)
            assert fast_shape(metric, dim, 10, 100, bare) == fast_shape(metric, dim, 100, 100, bare)
    for bad in (dict(metric=2), dict(dim=0), dict(ef=513), dict(k=600)):
        kw = dict(dict(metric=L2, dim=128, ef=100, k=10), **bad)
        with pytest.raises(hs.HsError) as e:
            fast_shape(kw["metric"], kw["dim"], kw["ef"], kw["k"])
        assert e.value.status == hs.HS_ERR_INVALID


def test_fast_shape_table_is_the_set_of_instantiations_built():
    """The launchers of beam_search.hip dispatch on fast_shape and instantiate one kernel per `case`; the compiler's resource
    report lists every instantiation of the build.  The two sets are equal: a case added to or dropped from a launcher without the
    table changing (or the reverse) shows as a kernel nobody can launch, or as a shape the launcher refuses."""
    import re

    from test_f32_free_cpu import _report
    built, filt = set(), set()
    num = lambda s: -int(s[1:]) if s.startswith("n") else int(s)
    for name in _report():
        m = re.fullmatch(r"_ZN2hs11fast_kernelILi(\d)ELi(\d)ELi(n?\d+)ELb(\d)ELb(\d)EEEvNS_8DevIndexENS_10SearchArgsE(NS_10FilterArgsE)?", name)
        if m:
            shape = (int(m.group(1)), int(m.group(2)), num(m.group(3)), int(m.group(4)), int(m.group(5)))
            (filt if m.group(6) else built).add(shape)
    want = fast_shapes_reachable()
    assert built == want, (sorted(built - want), sorted(want - built))
    assert filt == {s for s in want if not s[4]}, "the filter-set overloads: every !bare shape and nothing else"
    assert len(built) == 128 and len(filt) == 20
