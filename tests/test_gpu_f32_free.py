"""fp32-free indexes on the device (hs_index_set_f32_resident, hs_index_load_narrow): an index that holds its rows in u8 or fp16
ONLY.  Every case runs one call three times on one index -- fp32 format (state A), narrow rows beside the fp32 rows (state B),
narrow rows alone (state C) -- and asserts A == B == C byte for byte (labels in output order, distance bits, counts, all four stats
columns), C against the oracle, and the kernel that served C: the narrow twin of whichever of flat / fast / strict the index
would have run (hs::flat_kernel_u8, hs::fast_kernel_f16, hs::strict_kernel_u8, ...; csrc/beam_search_u8.hip, beam_search_f16.hip).
All data is exactly representable: small-integer or SIFT-like rows for u8, float16-rounded rows for fp16."""
import os
import subprocess
import sys

import numpy as np
import pytest

from hsutil import ROOT, headline_data, load_chal_encode, load_product, mixture
from test_gpu_narrow_rows import K, L2, IP, N, D, _int_rows, bench_index, hs, same_as_oracle, same_bytes, small_int_index  # noqa: F401
from test_gpu_narrow_rows import oracle_answer as _oracle_answer
from test_gpu_parity import _pq_sorted

pytestmark = pytest.mark.gpu


def oracle_answer(ox, q, ef, key):
    """test_gpu_narrow_rows.oracle_answer under keys of this module's own.  `bench_index` is a module-scoped fixture, so this module
    and that one each build a graph (with 16 threads: not the same graph twice), while the answers are cached in ONE dict over there
    by (key, ef): under its keys one module would be handed the answers of the other's graph."""
    return _oracle_answer(ox, q, ef, ("f32_free",) + tuple(key))


def suffix(hs, fmt):
    return {hs.HS_ROWS_U8: "_u8", hs.HS_ROWS_F16: "_f16"}[fmt]


def three_states(hs, ix, fmt, run, what, kernel):
    """run() in states A, B and C of ix: identical outputs; `kernel` ("hs::flat_kernel" | "hs::fast_kernel" | "hs::strict_kernel")
    served A, its narrow twin C (B: the flat kernel reads narrow, the others fp32).  Leaves ix in state C; returns C's result."""
    ix.set_f32_resident(True)
    ix.set_row_format(hs.HS_ROWS_F32)
    assert ix.row_format() == hs.HS_ROWS_F32 and ix.f32_resident()
    a = run()
    assert ix.last_kernel() == kernel, f"{what}: state A ran {ix.last_kernel()}"
    ix.set_row_format(fmt)
    b = run()
    assert ix.last_kernel() == (kernel + suffix(hs, fmt) if kernel == "hs::flat_kernel" else kernel), f"{what}: state B ran {ix.last_kernel()}"
    ix.set_f32_resident(False)
    assert ix.row_format() == fmt and not ix.f32_resident()
    c = run()
    assert ix.last_kernel() == kernel + suffix(hs, fmt), f"{what}: state C ran {ix.last_kernel()}"
    same_bytes(a, b, what + " (B)")
    same_bytes(a, c, what + " (C)")
    return c


def formats(hs):
    return (hs.HS_ROWS_U8, hs.HS_ROWS_F16)


def ids(ix, q, k=K):
    return lambda: ix.search_ids(q, k, want_dists=True, want_stats=True)


# ---- 1. bare search: the flat twin ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq", (6143, 10_000))
def test_bench_shape_host_entry(hs, bench_index, nq):
    """50k x 128 headline_data, nq below and above the descent / order / level-0 split."""
    ix, ox, _ = bench_index
    q = headline_data(nq, D, 456)
    for ef in (64, 70, 129, 512):
        ix.set_ef(ef)
        want = oracle_answer(ox, q, ef, ("host", nq))
        for fmt in formats(hs):
            what = f"nq={nq} ef={ef} fmt={fmt}"
            r = three_states(hs, ix, fmt, ids(ix, q), what, "hs::flat_kernel")
            same_as_oracle(want, r["labels"], r["dists"], r["stats"], what)
    ix.set_f32_resident(True)
    ix.set_row_format(hs.HS_ROWS_F32)


def test_bench_shape_device_entry_two_streams(hs, bench_index):
    """search_ids_dev on torch device tensors, two 10 000-query batches in flight on two non-default streams, states A and C."""
    import torch
    ix, ox, _ = bench_index
    dev = torch.device("cuda", 0)
    qs = [headline_data(10_000, D, 456 + b) for b in range(2)]
    q_dev = [torch.from_numpy(q).to(dev) for q in qs]
    streams = [torch.cuda.Stream(device=dev) for _ in range(2)]
    torch.cuda.synchronize()
    ix.set_ef(70)
    res = {}
    for fmt in (hs.HS_ROWS_F32, hs.HS_ROWS_U8, hs.HS_ROWS_F16):
        ix.set_f32_resident(True)
        ix.set_row_format(fmt)
        if fmt != hs.HS_ROWS_F32:
            ix.set_f32_resident(False)
        outs = []
        for b in range(2):
            lab = torch.full((10_000, K), -1, dtype=torch.int32, device=dev)
            dst = torch.full((10_000, K), float("nan"), dtype=torch.float32, device=dev)
            cnt = torch.zeros((10_000,), dtype=torch.int32, device=dev)
            sts = torch.zeros((10_000, 4), dtype=torch.int32, device=dev)
            streams[b].wait_stream(torch.cuda.current_stream())
            ix.search_ids_dev(q_dev[b], K, lab, dst, cnt, sts, streams[b].cuda_stream)
            outs.append((lab, dst, cnt, sts))
        for b in range(2):
            ix.check(streams[b].cuda_stream)
        assert ix.last_kernel() == "hs::flat_kernel" + ("" if fmt == hs.HS_ROWS_F32 else suffix(hs, fmt))
        assert ix.f32_resident() == (fmt == hs.HS_ROWS_F32)
        res[fmt] = [tuple(t.cpu().numpy() for t in outs[b]) for b in range(2)]
    for fmt in formats(hs):
        for b in range(2):
            for x, y in zip(res[hs.HS_ROWS_F32][b], res[fmt][b]):
                assert x.tobytes() == y.tobytes(), f"device entry, batch {b}, fmt={fmt}: differs from the fp32-format run"
            lab, dst, cnt, sts = res[fmt][b]
            assert np.all(cnt == K)
            same_as_oracle(oracle_answer(ox, qs[b], 70, ("dev", b)), lab, dst, sts, f"device entry, batch {b}, fmt={fmt}")
    ix.set_f32_resident(True)
    ix.set_row_format(hs.HS_ROWS_F32)


@pytest.mark.parametrize("metric", (L2, IP))
@pytest.mark.parametrize("d", (16, 64, 96, 320, 960))
def test_tie_heavy_integer_rows(hs, oracle, tmp_path, d, metric):
    n = 6000 if d <= 128 else 2500
    base, q = _int_rows(n, d, 31 + d), _int_rows(64, d, 77 + d)
    hp, sp = str(tmp_path / "h.bin"), str(tmp_path / "s.bin")
    hs.build_hnsw(base, hp, metric=metric, M=12, ef_construction=80, threads=8)
    hs.convert_slim(hp, sp, d, metric=metric, threads=8)
    ix, ox = hs.Index(sp, hs.HS_KIND_SLIM, d, metric=metric), oracle.load(sp, "slim", metric, d)
    for ef, k in ((40, 10), (129, 10), (192, 64), (512, 64)):
        ix.set_ef(ef); ox.set_ef(ef)
        o, oi = ox.search_pq(q, k, threads=8), ox.search_ids(q, k, threads=8)
        for fmt in formats(hs):
            cfg = f"d={d} metric={metric} ef={ef} k={k} fmt={fmt}"
            g = three_states(hs, ix, fmt, lambda: ix.search_pq(q, k, want_stats=True), cfg, "hs::flat_kernel")
            assert np.array_equal(g["cnt"], o["cnt"]), cfg
            assert _pq_sorted(g["dists"], g["labels"], g["cnt"]) == _pq_sorted(o["dists"], o["labels"], o["cnt"]), cfg
            r = three_states(hs, ix, fmt, ids(ix, q, k), cfg + " ids", "hs::flat_kernel")
            assert np.array_equal(np.sort(r["labels"], 1), np.sort(oi["labels"], 1)), cfg
            assert np.array_equal(r["stats"][:, :3], oi["counters"][:, :3]), cfg


# ---- 2. the strict twin ---------------------------------------------------------------------------------------------------------
def _deleted_index(hs, s, deleted):
    return hs.Index.from_arrays(hs.HS_KIND_SLIM, hs.HS_METRIC_L2, s["rows"], s["level"], s["lists"], s["enterpoint"], s["maxlevel"],
                                labels=s["labels"], deleted=deleted)


@pytest.mark.parametrize("fmt_name", ("HS_ROWS_U8", "HS_ROWS_F16"))
def test_strict_twin(hs, oracle, small_int_index, tmp_path, fmt_name):
    sp, s, base, q = small_int_index
    fmt = getattr(hs, fmt_name)
    ix, ox = hs.Index(sp, hs.HS_KIND_SLIM, 64), oracle.load(sp, "slim", L2, 64)
    ix.set_ef(64); ox.set_ef(64)
    # exact-order mode: the reference's array order
    ix.set_exact_order(True)
    r = three_states(hs, ix, fmt, ids(ix, q), "exact order", "hs::strict_kernel")
    ix.set_exact_order(False)
    o = ox.search_ids(q, K)
    assert np.array_equal(r["labels"], o["labels"]) and np.array_equal(r["stats"][:, :3], o["counters"][:, :3])

    def raw_valid():   # (the arrays beyond raw_sz[i] entries are not written)
        r = ix.search_raw(q, K)
        keep = np.arange(r["raw_d"].shape[1])[None, :] < r["raw_sz"][:, None]
        return dict(raw_d=np.where(keep, r["raw_d"], np.float32(0)), raw_i=np.where(keep, r["raw_i"], np.uint32(0)), raw_sz=r["raw_sz"], stats=r["stats"])
    r = three_states(hs, ix, fmt, raw_valid, "search_raw", "hs::strict_kernel")
    assert np.array_equal(r["raw_sz"], o["raw_sz"])
    # ef beyond the fast and flat kernels
    ix.set_ef(600); ox.set_ef(600)
    r = three_states(hs, ix, fmt, ids(ix, q), "ef = 600", "hs::strict_kernel")
    o = ox.search_ids(q, K)
    assert np.array_equal(np.sort(r["labels"], 1), np.sort(o["labels"], 1)) and np.array_equal(r["stats"][:, :3], o["counters"][:, :3])
    # threshold_level = 1: the upper beam of searchBaseLayer
    hp, tp = str(tmp_path / "h.bin"), str(tmp_path / "t1.bin")
    hs.build_hnsw(base, hp, M=16, ef_construction=100, threads=8)
    hs.convert_slim(hp, tp, 64, threshold_level=1, threads=8)
    tx, to = hs.Index(tp, hs.HS_KIND_SLIM, 64), oracle.load(tp, "slim", L2, 64)
    assert tx.info()["threshold_level"] == 1
    for ef in (16, 64):
        tx.set_ef(ef); to.set_ef(ef)
        r = three_states(hs, tx, fmt, ids(tx, q), f"threshold_level = 1, ef={ef}", "hs::strict_kernel")
        o = to.search_ids(q, K)
        assert np.array_equal(np.sort(r["labels"], 1), np.sort(o["labels"], 1)) and np.array_equal(r["stats"][:, :3], o["counters"][:, :3])
    # k = ef on an index with delete marks (the fast kernel's boundary watch is compiled for bare indexes only)
    deleted = (np.arange(3000) % 5 == 0).astype(np.uint8)
    dx = _deleted_index(hs, s, deleted)
    dx.set_ef(40); ox.set_ef(40)
    r = three_states(hs, dx, fmt, lambda: dx.search_pq(q, 40, want_stats=True), "k = ef, delete marks", "hs::strict_kernel")
    ox.set_filter(1 - deleted)
    o = ox.search_pq(q, 40)
    ox.set_filter(None)
    assert np.array_equal(r["cnt"], o["cnt"]) and _pq_sorted(r["dists"], r["labels"], r["cnt"]) == _pq_sorted(o["dists"], o["labels"], o["cnt"])


# ---- 3. the fast twin -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt_name", ("HS_ROWS_U8", "HS_ROWS_F16"))
def test_fast_twin(hs, oracle, small_int_index, fmt_name):
    """The !bare shapes at S = 1, 2, 4, 8 (ef 48, 100, 200, 400) through a filter and through delete marks; the bare shapes where
    the flat kernel does not serve a bare index without any environment knob: k > 64 -- ef = 100, 200, 400 (S = 2, 4, 8) and
    ef == k = 100 (the boundary-watching S = 2 shape).  The bare S = 1 shapes (ef <= 64 < k is impossible) are reached only with
    HS_KERNEL=fast: test_forced_fast_kernel_in_a_child_process."""
    sp, s, base, q = small_int_index
    fmt = getattr(hs, fmt_name)
    ix, ox = hs.Index(sp, hs.HS_KIND_SLIM, 64), oracle.load(sp, "slim", L2, 64)
    allowed = (np.arange(3000) % 3 != 0).astype(np.uint8)
    deleted = (np.arange(3000) % 4 == 1).astype(np.uint8)
    dx = _deleted_index(hs, s, deleted)
    for ef in (48, 100, 200, 400):
        ix.set_ef(ef); ox.set_ef(ef); dx.set_ef(ef)
        r = three_states(hs, ix, fmt, lambda: ix.search_filtered(q, K, allowed, want_stats=True), f"filtered ef={ef}", "hs::fast_kernel")
        ox.set_filter(allowed)
        o = ox.search_pq(q, K)
        assert np.array_equal(r["cnt"], o["cnt"]) and _pq_sorted(r["dists"], r["labels"], r["cnt"]) == _pq_sorted(o["dists"], o["labels"], o["cnt"]), ef
        r = three_states(hs, dx, fmt, lambda: dx.search_pq(q, K, want_stats=True), f"delete marks ef={ef}", "hs::fast_kernel")
        ox.set_filter(1 - deleted)
        o = ox.search_pq(q, K)
        ox.set_filter(None)
        assert np.array_equal(r["cnt"], o["cnt"]) and _pq_sorted(r["dists"], r["labels"], r["cnt"]) == _pq_sorted(o["dists"], o["labels"], o["cnt"]), ef
    for ef, k in ((100, 65), (200, 65), (400, 65), (100, 100), (128, 128)):
        ix.set_ef(ef); ox.set_ef(ef)
        r = three_states(hs, ix, fmt, lambda: ix.search_pq(q, k, want_stats=True), f"bare ef={ef} k={k}", "hs::fast_kernel")
        o = ox.search_pq(q, k)
        assert np.array_equal(r["cnt"], o["cnt"]) and _pq_sorted(r["dists"], r["labels"], r["cnt"]) == _pq_sorted(o["dists"], o["labels"], o["cnt"]), (ef, k)
        r = three_states(hs, ix, fmt, ids(ix, q, k), f"bare ids ef={ef} k={k}", "hs::fast_kernel")
        o = ox.search_ids(q, k)
        assert np.array_equal(np.sort(r["labels"], 1), np.sort(o["labels"], 1)) and np.array_equal(r["stats"][:, :3], o["counters"][:, :3]), (ef, k)


_FORCED_FAST = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from hsutil import load_product
hs = load_product()
sp, qf, out = sys.argv[2], sys.argv[3], sys.argv[4]
q = np.fromfile(qf, np.float32).reshape(-1, 64)
ix = hs.Index(sp, hs.HS_KIND_SLIM, 64)
res = {}
for state in ("A", "C8", "C16"):
    ix.set_f32_resident(True)
    ix.set_row_format({"A": hs.HS_ROWS_F32, "C8": hs.HS_ROWS_U8, "C16": hs.HS_ROWS_F16}[state])
    if state != "A":
        ix.set_f32_resident(False)
    for ef, k in ((48, 10), (64, 64), (100, 10), (100, 100), (200, 10), (400, 10)):
        ix.set_ef(ef)
        r = ix.search_ids(q, k, want_dists=True, want_stats=True)
        want = {"A": "hs::fast_kernel", "C8": "hs::fast_kernel_u8", "C16": "hs::fast_kernel_f16"}[state]
        assert ix.last_kernel() == want, (state, ef, k, ix.last_kernel())
        for key in ("labels", "dists", "stats"):
            res[f"{state}_{ef}_{k}_{key}"] = r[key]
np.savez(out, **res)
"""


def test_forced_fast_kernel_in_a_child_process(hs, oracle, small_int_index, tmp_path):
    """HS_KERNEL=fast (read once per process, hence the child): every bare shape of the fast kernel, S = 1, 2, 4, 8 and the two
    ef == k shapes, in states A and C of both formats -- equal bytes, and C equal to the oracle."""
    sp, _, _, q = small_int_index
    qf, out = str(tmp_path / "q.f32"), str(tmp_path / "res.npz")
    q.tofile(qf)
    env = dict(os.environ, HS_KERNEL="fast")
    subprocess.run([sys.executable, "-c", _FORCED_FAST, os.path.join(ROOT, "tests"), sp, qf, out], env=env, check=True, timeout=600)
    res = np.load(out)
    ox = oracle.load(sp, "slim", L2, 64)
    for ef, k in ((48, 10), (64, 64), (100, 10), (100, 100), (200, 10), (400, 10)):
        ox.set_ef(ef)
        o = ox.search_ids(q, k)
        for state in ("C8", "C16"):
            for key in ("labels", "dists", "stats"):
                a, c = res[f"A_{ef}_{k}_{key}"], res[f"{state}_{ef}_{k}_{key}"]
                assert a.dtype == c.dtype and a.tobytes() == c.tobytes(), (state, ef, k, key)
            assert np.array_equal(np.sort(res[f"{state}_{ef}_{k}_labels"], 1), np.sort(o["labels"], 1)), (state, ef, k)
            assert np.array_equal(res[f"{state}_{ef}_{k}_stats"][:, :3], o["counters"][:, :3]), (state, ef, k)


@pytest.mark.parametrize("fmt_name", ("HS_ROWS_U8", "HS_ROWS_F16"))
def test_inner_product_strict_and_fast_twins(hs, oracle, tmp_path, fmt_name):
    """The inner-product strict and fast twins (every other case of sections 2 and 3 is L2) at the smallest shape that reaches them:
    d = 16, 200 tie-heavy integer rows, 20 queries, k = 3, ef = 10.  Strict: the exact-order mode, the reference's array order.
    Fast: under a filter (the !bare S = 1 shape), and bare at ef == k = 65 -- the boundary-watching shape, where the flat kernel
    does not serve a bare index (k > 64; ef == k = 10 would need HS_KERNEL=fast, read once per process)."""
    n, d = 200, 16
    fmt = getattr(hs, fmt_name)
    base, q = _int_rows(n, d, 5), _int_rows(20, d, 6)
    hp, sp = str(tmp_path / "h.bin"), str(tmp_path / "s.bin")
    hs.build_hnsw(base, hp, metric=IP, M=8, ef_construction=60, threads=4)
    hs.convert_slim(hp, sp, d, metric=IP, threads=4)
    ix, ox = hs.Index(sp, hs.HS_KIND_SLIM, d, metric=IP), oracle.load(sp, "slim", IP, d)
    ix.set_ef(10); ox.set_ef(10)
    ix.set_exact_order(True)
    r = three_states(hs, ix, fmt, ids(ix, q, 3), "IP exact order", "hs::strict_kernel")
    ix.set_exact_order(False)
    o = ox.search_ids(q, 3)
    assert np.array_equal(r["labels"], o["labels"]) and np.array_equal(r["stats"][:, :3], o["counters"][:, :3])
    allowed = (np.arange(n) % 3 != 0).astype(np.uint8)
    r = three_states(hs, ix, fmt, lambda: ix.search_filtered(q, 3, allowed, want_stats=True), "IP filtered", "hs::fast_kernel")
    ox.set_filter(allowed)
    o = ox.search_pq(q, 3)
    ox.set_filter(None)
    assert np.array_equal(r["cnt"], o["cnt"]) and _pq_sorted(r["dists"], r["labels"], r["cnt"]) == _pq_sorted(o["dists"], o["labels"], o["cnt"])
    ix.set_ef(65); ox.set_ef(65)
    r = three_states(hs, ix, fmt, lambda: ix.search_pq(q, 65, want_stats=True), "IP bare ef = k = 65", "hs::fast_kernel")
    o = ox.search_pq(q, 65)
    assert np.all(o["cnt"] == 65)   # every query reaches k nodes: searchKnn(q, k, tableint*) below is defined
    assert np.array_equal(r["cnt"], o["cnt"]) and _pq_sorted(r["dists"], r["labels"], r["cnt"]) == _pq_sorted(o["dists"], o["labels"], o["cnt"])
    r = three_states(hs, ix, fmt, ids(ix, q, 65), "IP bare ids ef = k = 65", "hs::fast_kernel")
    o = ox.search_ids(q, 65)
    assert np.array_equal(np.sort(r["labels"], 1), np.sort(o["labels"], 1)) and np.array_equal(r["stats"][:, :3], o["counters"][:, :3])


# ---- 4. the re-run pass ---------------------------------------------------------------------------------------------------------
RERUN_SEED = 31


@pytest.mark.parametrize("fmt_name", ("HS_ROWS_U8", "HS_ROWS_F16"))
def test_rerun_pass_reads_the_narrow_rows(hs, oracle, tmp_path, fmt_name):
    """The recipe of tests/test_gpu_parity.py::test_fallback_pass_is_exact on integer rows (mixture(6000, 32, RERUN_SEED,
    integer=True)): with cand_cap = 80 and hash_slots = 256 queries overflow the first pass and are answered by the re-run pass
    (stats column 3 == 2), which on an fp32-free index launches hs::strict_kernel_u8 / _f16.  The precondition is asserted on
    state A -- the fp32 kernels, not the code under test: at least one query takes the re-run in the exact-order mode (as in
    the original recipe; the fast kernel spills to its tier-2 region first, its count is only required to be equal across
    states).  Seed: RERUN_SEED = 31, the seed of the original recipe.  Observed on an MI355X in state A (the test prints it,
    `pytest -rP`): 128 of 128 queries answered by pass 2 in the exact-order mode, 0 of 128 in the default mode (the fast kernel's
    tier-2 spill absorbs the overflow), the same for both formats.  If the data ever gives none in the exact-order mode the test
    fails there rather than passing vacuously."""
    fmt = getattr(hs, fmt_name)
    base, q = mixture(6000, 32, RERUN_SEED, integer=True), mixture(128, 32, RERUN_SEED + 1, integer=True)
    hp, sp = str(tmp_path / "h.bin"), str(tmp_path / "s.bin")
    hs.build_hnsw(base, hp, M=8, ef_construction=100, threads=8)
    hs.convert_slim(hp, sp, 32, threads=8)
    ix, ox = hs.Index(sp, hs.HS_KIND_SLIM, 32), oracle.load(sp, "slim", L2, 32)
    ix.set_ef(64); ox.set_ef(64)
    want = ox.search_ids(q, 10)
    ix.set_capacity(cand_cap=80, hash_slots=256)
    for exact in (True, False):
        ix.set_exact_order(exact)
        ix.set_f32_resident(True)
        ix.set_row_format(hs.HS_ROWS_F32)
        a = ix.search_ids(q, 10, want_dists=True, want_stats=True)
        n_rerun, kernel_a = int((a["stats"][:, 3] == 2).sum()), ix.last_kernel()
        assert kernel_a == "hs::strict_kernel" if exact else kernel_a in ("hs::flat_kernel", "hs::fast_kernel")
        print(f"re-run pass, exact={exact}: {n_rerun} of {len(q)} queries answered by pass 2 in state A")
        if exact:
            assert n_rerun > 0, "state A: no query took the re-run pass -- the data does not exercise it"
        ix.set_row_format(fmt)
        ix.set_f32_resident(False)
        c = ix.search_ids(q, 10, want_dists=True, want_stats=True)
        assert ix.last_kernel() == kernel_a + suffix(hs, fmt)
        same_bytes(a, c, f"re-run pass, exact={exact}")
        assert np.array_equal(np.sort(c["labels"], 1), np.sort(want["labels"], 1))
        if exact:
            assert np.array_equal(c["labels"], want["labels"])
    ix.set_capacity(0, 0)


# ---- 5. accounting and state changes --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra_rows", (0, 500))
def test_accounting_state_changes_and_refusals(hs, small_int_index, extra_rows):
    sp, _, _, q = small_int_index
    n, d = 3000, 64
    cap = n + extra_rows
    ix = hs.Index(sp, hs.HS_KIND_SLIM, d, max_elements=cap if extra_rows else 0)
    ix.set_ef(100)
    bytes_a = ix.info()["device_bytes"]
    first = ix.search_ids(q, K, want_dists=True, want_stats=True)
    assert ix.last_kernel() == "hs::flat_kernel" and ix.f32_resident()
    # drop on an fp32-format index: refused, nothing changes
    with pytest.raises(hs.HsError) as e:
        ix.set_f32_resident(False)
    assert e.value.status == hs.HS_ERR_INVALID
    assert ix.f32_resident() and ix.row_format() == hs.HS_ROWS_F32 and ix.info()["device_bytes"] == bytes_a
    same_bytes(first, ix.search_ids(q, K, want_dists=True, want_stats=True), "after the refused drop")
    for fmt, width in ((hs.HS_ROWS_U8, 1), (hs.HS_ROWS_F16, 2)):
        ix.set_row_format(fmt)
        assert ix.info()["device_bytes"] == bytes_a + cap * d * width
        for rnd in range(2):   # drop -> restore -> drop
            ix.set_f32_resident(False)
            ix.set_f32_resident(False)   # idempotent
            assert not ix.f32_resident() and ix.info()["device_bytes"] == bytes_a - cap * d * 4 + cap * d * width
            same_bytes(first, ix.search_ids(q, K, want_dists=True, want_stats=True), f"fmt={fmt} dropped, round {rnd}")
            assert ix.last_kernel() == "hs::flat_kernel" + suffix(hs, fmt)
            ix.set_exact_order(True)
            strict_c = ix.search_ids(q, K, want_dists=True, want_stats=True)
            assert ix.last_kernel() == "hs::strict_kernel" + suffix(hs, fmt)
            # any other format while dropped: refused, everything as it was
            for other in (hs.HS_ROWS_F32, hs.HS_ROWS_U8, hs.HS_ROWS_F16):
                if other == fmt:
                    ix.set_row_format(other)   # (the format it has: a no-op)
                    continue
                with pytest.raises(hs.HsError) as e:
                    ix.set_row_format(other)
                assert e.value.status == hs.HS_ERR_INVALID and "restore the fp32 rows first" in str(e.value)
                assert ix.row_format() == fmt and not ix.f32_resident()
                assert ix.info()["device_bytes"] == bytes_a - cap * d * 4 + cap * d * width
            same_bytes(strict_c, ix.search_ids(q, K, want_dists=True, want_stats=True), "after the refused format changes")
            ix.set_f32_resident(True)
            ix.set_f32_resident(True)
            assert ix.f32_resident() and ix.info()["device_bytes"] == bytes_a + cap * d * width
            same_bytes(strict_c, ix.search_ids(q, K, want_dists=True, want_stats=True), "restored, exact order")
            assert ix.last_kernel() == "hs::strict_kernel"   # the fp32 kernel names are back
            ix.set_exact_order(False)
            allowed = (np.arange(n) % 3 != 0).astype(np.uint8)
            ix.search_filtered(q, K, allowed)
            assert ix.last_kernel() == "hs::fast_kernel"
            same_bytes(first, ix.search_ids(q, K, want_dists=True, want_stats=True), "restored")
            assert ix.last_kernel() == "hs::flat_kernel" + suffix(hs, fmt)
        ix.set_row_format(hs.HS_ROWS_F32)
        assert ix.info()["device_bytes"] == bytes_a
    same_bytes(first, ix.search_ids(q, K, want_dists=True, want_stats=True), "back in fp32 format")
    assert ix.last_kernel() == "hs::flat_kernel"


# ---- 6. patch -------------------------------------------------------------------------------------------------------------------
def _patch_files(hs, ce, tmp_path, rows_by_tag, dim, M):
    files = {}
    for tag, rows in rows_by_tag.items():
        hp, sp = str(tmp_path / f"{tag}.hnsw"), str(tmp_path / f"{tag}.slim")
        hs.build_hnsw(rows, hp, M=M, ef_construction=100, threads=1)   # serial: the first insertions are the same in all
        hs.convert_slim(hp, sp, dim, threads=1)
        files[tag] = open(sp, "rb").read()
    return files


def _patched_equals_whole(hs, oracle, tmp_path, ix, fx, want_file, dim, q, efs, fmt):
    ref = hs.Index(want_file, hs.HS_KIND_SLIM, dim)
    ox = oracle.load(want_file, "slim", 0, dim)
    for ef in efs:
        for x in (ix, fx, ref, ox):
            x.set_ef(ef)
        for exact in (False, True):
            for x in (ix, fx, ref):
                x.set_exact_order(exact)
            c, f, b = (x.search_ids(q, 10, want_dists=True, want_stats=True) for x in (ix, fx, ref))
            assert ix.last_kernel() == ("hs::strict_kernel" if exact else "hs::flat_kernel") + suffix(hs, fmt)
            same_bytes(f, c, f"patched fp32-free index vs the same patch on an fp32 index, ef={ef} exact={exact}")
            same_bytes(b, c, f"patched fp32-free index vs the index loaded whole, ef={ef} exact={exact}")
            o = ox.search_ids(q, 10)
            assert np.array_equal(np.sort(c["labels"], 1), np.sort(o["labels"], 1)) and np.array_equal(c["stats"][:, :3], o["counters"][:, :3])
            if exact:
                assert np.array_equal(c["labels"], o["labels"])


def test_patch_per_row_on_an_f32_free_index(hs, oracle, tmp_path):
    """The d = 128 integer case of tests/test_gpu_patch.py on a state-C index (per-row path: the tile stride stays); a patch whose
    new rows hold 300.0 is refused and the index answers as before."""
    ce = load_chal_encode()
    dim, n0, delta = 128, 8000, 1500
    base = mixture(n0 + delta, dim, 17, integer=True)
    bad = base.copy()
    bad[n0 + 700, 5] = np.float32(300.0)
    files = _patch_files(hs, ce, tmp_path, {"old": base[:n0], "new": base, "bad": bad}, dim, 16)
    patch, n_changed, n_added = ce.make_patch(files["old"], files["new"], dim, to_add=True)
    bad_patch, _, bad_added = ce.make_patch(files["old"], files["bad"], dim, to_add=True)
    assert n_added == delta and bad_added == delta and n_changed > 0
    want_file = str(tmp_path / "expect.slim")
    open(want_file, "wb").write(ce.with_entry_of(files["new"], files["old"]))
    q = mixture(300, dim, 18, integer=True)
    cap = n0 + delta + 16
    ix = hs.Index(str(tmp_path / "old.slim"), hs.HS_KIND_SLIM, dim, max_elements=cap)
    fx = hs.Index(str(tmp_path / "old.slim"), hs.HS_KIND_SLIM, dim, max_elements=cap)
    ix.set_row_format(hs.HS_ROWS_U8)
    ix.set_f32_resident(False)
    ix.set_ef(48)
    before = ix.search_ids(q, 10, want_dists=True, want_stats=True)
    bytes_before, stride_before = ix.info()["device_bytes"], ix.info()["max_degree0"]
    with pytest.raises(hs.HsError) as e:
        ix.patch(bad_patch, to_add=True)
    assert e.value.status == hs.HS_ERR_UNSUPPORTED and str(n0 + 700) in str(e.value), str(e.value)
    assert ix.info()["n"] == n0 and ix.row_format() == hs.HS_ROWS_U8 and not ix.f32_resident() and ix.info()["device_bytes"] == bytes_before
    same_bytes(before, ix.search_ids(q, 10, want_dists=True, want_stats=True), "after the refused patch")
    ix.patch(patch, to_add=True)
    fx.patch(patch, to_add=True)
    assert ix.info()["n"] == n0 + delta and not ix.f32_resident() and ix.row_format() == hs.HS_ROWS_U8
    assert (ix.info()["max_degree0"] + 15) // 16 == (stride_before + 15) // 16, "this case is meant to keep the tile stride"
    assert ix.info()["device_bytes"] == fx.info()["device_bytes"] - cap * dim * 4 + cap * dim
    _patched_equals_whole(hs, oracle, tmp_path, ix, fx, want_file, dim, q, (10, 48, 100), hs.HS_ROWS_U8)
    ix.set_ef(48); ix.set_exact_order(False)
    assert not np.array_equal(ix.search_ids(q, 10)["labels"], before["labels"]), "the patch changed nothing?"


def test_patch_that_re_tiles_an_f32_free_index(hs, oracle, tmp_path):
    """An index of 12 nodes (level-0 lists of at most 11 ids: tile stride 16) grown to 4000: the lists outgrow the stride, the
    patch takes the whole-upload path, which on an fp32-free index rebuilds the fp16 copy from the host image."""
    ce = load_chal_encode()
    dim, n0, delta = 64, 12, 3988
    base = np.ascontiguousarray(mixture(n0 + delta, dim, 23, integer=True))
    files = _patch_files(hs, ce, tmp_path, {"old": base[:n0], "new": base}, dim, 16)
    patch, n_changed, n_added = ce.make_patch(files["old"], files["new"], dim, to_add=True)
    assert n_added == delta
    want_file = str(tmp_path / "expect.slim")
    open(want_file, "wb").write(ce.with_entry_of(files["new"], files["old"]))
    q = mixture(200, dim, 24, integer=True)
    cap = n0 + delta
    ix = hs.Index(str(tmp_path / "old.slim"), hs.HS_KIND_SLIM, dim, max_elements=cap)
    fx = hs.Index(str(tmp_path / "old.slim"), hs.HS_KIND_SLIM, dim, max_elements=cap)
    ix.set_row_format(hs.HS_ROWS_F16)
    ix.set_f32_resident(False)
    assert ix.info()["max_degree0"] <= 16
    ix.patch(patch, to_add=True)
    fx.patch(patch, to_add=True)
    assert ix.info()["max_degree0"] > 16, "the patch was meant to outgrow the tile stride"
    assert ix.info()["n"] == cap and not ix.f32_resident() and ix.row_format() == hs.HS_ROWS_F16
    assert ix.info()["device_bytes"] == fx.info()["device_bytes"] - cap * dim * 4 + cap * dim * 2
    _patched_equals_whole(hs, oracle, tmp_path, ix, fx, want_file, dim, q, (10, 48), hs.HS_ROWS_F16)


# ---- 7. load_narrow -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_elements", (0, 3500))
def test_load_narrow_equals_load_set_drop(hs, oracle, small_int_index, tmp_path, max_elements):
    sp, s, base, q = small_int_index
    ox = oracle.load(sp, "slim", L2, 64)
    allowed = (np.arange(3000) % 3 != 0).astype(np.uint8)
    for fmt in formats(hs):
        nx = hs.Index.load_narrow(sp, hs.HS_KIND_SLIM, 64, fmt, max_elements=max_elements)
        ix = hs.Index(sp, hs.HS_KIND_SLIM, 64, max_elements=max_elements)
        ix.set_row_format(fmt)
        ix.set_f32_resident(False)
        assert nx.row_format() == fmt and not nx.f32_resident()
        assert nx.info() == ix.info()
        for ef in (48, 600):
            nx.set_ef(ef); ix.set_ef(ef); ox.set_ef(ef)
            a, b = (x.search_ids(q, K, want_dists=True, want_stats=True) for x in (nx, ix))
            same_bytes(b, a, f"load_narrow fmt={fmt} ef={ef}")
            assert nx.last_kernel() == ix.last_kernel() == ("hs::flat_kernel" if ef == 48 else "hs::strict_kernel") + suffix(hs, fmt)
            o = ox.search_ids(q, K)
            assert np.array_equal(np.sort(a["labels"], 1), np.sort(o["labels"], 1)) and np.array_equal(a["stats"][:, :3], o["counters"][:, :3])
        nx.set_ef(48); ix.set_ef(48)
        a, b = (x.search_filtered(q, K, allowed, want_stats=True) for x in (nx, ix))
        same_bytes(b, a, "load_narrow, filtered")
        assert nx.last_kernel() == "hs::fast_kernel" + suffix(hs, fmt)
        # and back to an ordinary index
        nx.set_f32_resident(True)
        nx.set_row_format(hs.HS_ROWS_F32)
        plain = hs.Index(sp, hs.HS_KIND_SLIM, 64, max_elements=max_elements)
        plain.set_ef(48)
        assert nx.info() == plain.info()
        same_bytes(plain.search_ids(q, K, want_dists=True, want_stats=True), nx.search_ids(q, K, want_dists=True, want_stats=True), "restored after load_narrow")
        assert nx.last_kernel() == "hs::flat_kernel"


def test_load_narrow_refusals(hs, small_int_index, tmp_path):
    from test_gpu_slimq import build
    sp, s, base, q = small_int_index
    rows = base.copy()
    bad_row = 1234
    rows[bad_row, 17] = np.float32(255.5)
    rows[2500, 3] = np.float32(-1.0)
    hp, bp = str(tmp_path / "h.bin"), str(tmp_path / "bad.bin")
    hs.build_hnsw(rows, hp, M=16, ef_construction=100, threads=8)
    hs.convert_slim(hp, bp, 64, threads=8)
    with pytest.raises(hs.HsError) as e:
        hs.Index.load_narrow(bp, hs.HS_KIND_SLIM, 64, hs.HS_ROWS_U8)
    assert e.value.status == hs.HS_ERR_UNSUPPORTED and str(bad_row) in str(e.value), str(e.value)
    ok = hs.Index.load_narrow(bp, hs.HS_KIND_SLIM, 64, hs.HS_ROWS_F16)   # 255.5 and -1 are fp16 values
    assert ok.row_format() == hs.HS_ROWS_F16 and not ok.f32_resident()
    for fmt, status in ((hs.HS_ROWS_F32, hs.HS_ERR_INVALID), (9, hs.HS_ERR_INVALID)):
        with pytest.raises(hs.HsError) as e:
            hs.Index.load_narrow(sp, hs.HS_KIND_SLIM, 64, fmt)
        assert e.value.status == status
    b20 = mixture(2000, 20, 3, integer=True)
    h20, s20 = str(tmp_path / "h20.bin"), str(tmp_path / "s20.bin")
    hs.build_hnsw(b20, h20, M=16, ef_construction=100, threads=8)
    hs.convert_slim(h20, s20, 20, threads=8)
    with pytest.raises(hs.HsError) as e:
        hs.Index.load_narrow(s20, hs.HS_KIND_SLIM, 20, hs.HS_ROWS_U8)
    assert e.value.status == hs.HS_ERR_UNSUPPORTED
    qp = build(hs, tmp_path, "q", mixture(3000, 128, 1, integer=True), L2, 8)
    with pytest.raises(hs.HsError) as e:
        hs.Index.load_narrow(qp, hs.HS_KIND_SLIMQ, 128, hs.HS_ROWS_U8)
    assert e.value.status == hs.HS_ERR_UNSUPPORTED


# ---- 8. sharded, facade ---------------------------------------------------------------------------------------------------------
def test_sharded_loopback_with_f32_free_replicas(hs, small_int_index):
    sp, _, _, q = small_int_index
    reps = [hs.Index.load_narrow(sp, hs.HS_KIND_SLIM, 64, hs.HS_ROWS_U8), hs.Index(sp, hs.HS_KIND_SLIM, 64)]
    reps[1].set_row_format(hs.HS_ROWS_U8)
    reps[1].set_f32_resident(False)
    single = hs.Index(sp, hs.HS_KIND_SLIM, 64)
    comm = hs.Comm([0, 0])
    for exact, kernel in ((False, "hs::flat_kernel"), (True, "hs::strict_kernel")):
        for x in reps + [single]:
            x.set_ef(48)
            x.set_exact_order(exact)
        want = single.search_ids(q, K, want_dists=True)
        got = comm.search_ids(reps, q, K, want_dists=True)
        assert all(r.last_kernel() == kernel + "_u8" for r in reps) and single.last_kernel() == kernel
        assert np.array_equal(got["labels"], want["labels"]) and got["dists"].tobytes() == want["dists"].tobytes()
        assert np.array_equal(got["cnt"], want["cnt"])
    comm.close()


def test_cpp_facade_with_an_f32_free_index(hs, oracle, tmp_path):
    exe = os.path.join(ROOT, "hnsw-slim_amd", "facade_f32_free")
    assert os.path.exists(exe)
    n, d, nq, k, ef = 3000, 64, 100, 10, 80
    base, q = mixture(n, d, 1, integer=True), mixture(nq, d, 2, integer=True)
    bf, qf, out = (str(tmp_path / f) for f in ("b.f32", "q.f32", "o.bin"))
    base.tofile(bf); q.tofile(qf)
    subprocess.check_call([exe, bf, str(n), str(d), qf, str(nq), str(k), str(ef), out])
    raw = np.fromfile(out, np.uint32)
    assert raw[:8].tolist() == [0, 1, 1, 0, 0, 1, 1, 1], raw[:8]
    slim_labels, slim_exact, hnsw_labels = (raw[8 + i * nq * k:8 + (i + 1) * nq * k].reshape(nq, k) for i in range(3))
    hp, sp = str(tmp_path / "h.bin"), str(tmp_path / "s.bin")
    hs.build_hnsw(base, hp, M=16, ef_construction=100, branching_factor="4", seed=100, threads=1)   # what the facade built
    hs.convert_slim(hp, sp, d)
    ox, ov = oracle.load(sp, "slim", L2, d), oracle.load(hp, "hnsw", L2, d)
    ox.set_ef(ef); ov.set_ef(ef)
    want = ox.search_ids(q, k)["labels"]
    assert np.array_equal(np.sort(slim_labels, 1), np.sort(want, 1))
    assert np.array_equal(slim_exact, want)
    w = ov.search_pq(q, k)
    assert np.all(w["cnt"] == k)
    assert np.array_equal(np.sort(hnsw_labels, 1), np.sort(w["labels"].astype(np.uint32), 1))
