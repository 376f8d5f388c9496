"""The search queue (hs_queue_*, SearchQueue): small submissions from many callers coalesced into one search launch.

Every comparison is bit for bit against the direct entry (search_ids / search_pq / search_filter_set) on the same index and ef:
labels, distances, counts, the padding of unused slots and all four stats columns.  Indexes are the small ones of
test_gpu_filter_sets.py (mixture, build_hnsw M = 8, convert_slim): 600 - 3000 rows, one per kernel the plan can choose."""
import os
import subprocess
import threading

import numpy as np
import pytest

from hsutil import ROOT, load_product, mixture

pytestmark = pytest.mark.gpu
L2, IP, K = 0, 1, 10
EFS = (10, 64, 200)
NQ = 330
# 37 submissions of 1, 1, 2, 3, 5, 8, 13, 21, 1, 1, ... rows: 228 in all
SIZES = [(1, 1, 2, 3, 5, 8, 13, 21)[i % 8] for i in range(37)]
TOTAL = sum(SIZES)
#        name          n     d    integer metric
SHAPES = {"d16": (2003, 16, False, L2), "d128": (3001, 128, True, L2), "d20": (2003, 20, False, L2), "d21ip": (2003, 21, False, IP),
          "d10": (1000, 10, False, L2), "d960": (600, 960, False, L2)}
# index name -> (shape, kind, what is done to it after the load)
INDEXES = {"slim_d16": ("d16", "slim", None), "slim_d128_int_flat": ("d128", "slim", None), "hnsw_d20_pq": ("d20", "hnsw", None),
           "hnsw_d21_ip": ("d21ip", "hnsw", None), "hnsw_d16_marked": ("d16", "hnsw", "marks"), "slim_d128_u8_only": ("d128", "slim", "u8"),
           "slim_d960": ("d960", "slim", None)}


@pytest.fixture(scope="module")
def hs():
    return load_product()


@pytest.fixture(scope="module")
def files(hs, tmp_path_factory):
    """shape name -> (vanilla file, Slim file, the NQ queries); built once."""
    tmp = tmp_path_factory.mktemp("search_queue")
    out = {}
    for name, (n, d, integer, metric) in SHAPES.items():
        x = mixture(n + NQ, d, seed=9, integer=integer)
        hp, sp = str(tmp / f"h_{name}.bin"), str(tmp / f"s_{name}.bin")
        hs.build_hnsw(x[:n], hp, metric=metric, M=8, ef_construction=60, threads=4)
        hs.convert_slim(hp, sp, d, metric=metric, threads=4)
        q = np.ascontiguousarray(x[n:])
        q.setflags(write=False)
        out[name] = (hp, sp, q)
    return out


def open_index(hs, files, name):
    """-> (index, the queue mode that fits it, queries)"""
    shape, kind, extra = INDEXES[name]
    n, d, _, metric = SHAPES[shape]
    hp, sp, q = files[shape]
    if kind == "hnsw":
        ix, mode = hs.Index(hp, hs.HS_KIND_HNSW, d, metric=metric), hs.HS_MODE_PQ
    else:
        ix, mode = hs.Index(sp, hs.HS_KIND_SLIM, d, metric=metric), hs.HS_MODE_SLIM_IDS
    if extra == "marks":
        ix.mark_deleted(np.arange(0, n, 7, dtype=np.uint64))
        assert ix.info()["has_deleted"] == 1
    if extra == "u8":
        ix.set_row_format(hs.HS_ROWS_U8)
        ix.set_f32_resident(False)
        assert not ix.f32_resident()
    return ix, mode, q


def direct(hs, ix, mode, q, k=K):
    if mode == hs.HS_MODE_SLIM_IDS:
        return ix.search_ids(q, k, want_dists=True, want_stats=True)
    return ix.search_pq(q, k, want_stats=True)


def same(got, want, what, rows=slice(None)):
    """every array `got` holds, against the same rows of `want`, as bytes"""
    for key in ("labels", "dists", "cnt", "stats"):
        if got.get(key) is None:
            continue
        assert np.ascontiguousarray(got[key]).tobytes() == np.ascontiguousarray(want[key][rows]).tobytes(), f"{what}: {key}"


def segments(sizes):
    at = 0
    for m in sizes:
        yield slice(at, at + m)
        at += m


def concat(results):
    return {key: np.concatenate([r[key] for r in results]) for key in ("labels", "dists", "cnt", "stats")}


def dev_submit(hs, sq, dq, stream=0, want_dists=True, want_stats=True, foq=None):
    """a device submission with fresh output tensors (filled with a pattern no answer has)"""
    import torch
    nq, k, dev, ids = dq.shape[0], sq.k, dq.device, sq.mode == hs.HS_MODE_SLIM_IDS
    lab = torch.full((nq, k), 7, dtype=torch.int32 if ids else torch.int64, device=dev)
    dist = torch.full((nq, k), -1.0, dtype=torch.float32, device=dev) if (want_dists or not ids) else None
    cnt = torch.full((nq,), 77, dtype=torch.int32, device=dev)
    stats = torch.full((nq, 4), 77, dtype=torch.int32, device=dev) if want_stats else None
    return sq.submit_dev(dq, lab, dist, cnt, stats, d_filter_of_query=foq, stream=stream)


def dev_result(hs, sq, t):
    ids = sq.mode == hs.HS_MODE_SLIM_IDS
    host = lambda x, dt: None if x is None else x.cpu().numpy().view(dt)
    return dict(labels=host(t.labels, np.uint32 if ids else np.uint64), dists=host(t.dists, np.float32), cnt=host(t.cnt, np.uint32),
                stats=host(t.stats, np.uint32))


# ---- 1. one launch, same bits -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(INDEXES))
def test_one_launch_same_bits(hs, files, name):
    ix, mode, q = open_index(hs, files, name)
    bytes_before = ix.info()["device_bytes"]
    sq = hs.SearchQueue(ix, K, mode, max_queries=1024, slots=2)
    assert ix.info()["device_bytes"] == bytes_before and sq.info()["device_bytes"] > 0
    for i, ef in enumerate(EFS):
        ix.set_ef(ef)
        want = direct(hs, ix, mode, q[:TOTAL])
        kernel = ix.last_kernel()
        tickets = [sq.submit(q[s], want_dists=True, want_stats=True) for s in segments(SIZES)]
        info = sq.info()
        assert info["pending"] == TOTAL and info["launches"] == i and info["in_flight"] == 0
        first = sq.wait(tickets[0])
        info = sq.info()
        assert info["launches"] == i + 1 and info["largest_launch"] == TOTAL and info["pending"] == 0 and info["in_flight"] == 0
        assert info["submitted"] == (i + 1) * TOTAL
        assert ix.last_kernel() == kernel
        results = [first] + [sq.wait(t) for t in tickets[1:]]
        same(concat(results), want, f"{name} ef={ef}: the concatenation against one direct call")
        for r, s in zip(results, segments(SIZES)):
            same(r, direct(hs, ix, mode, q[s]), f"{name} ef={ef}: rows {s.start}..{s.stop} against their own direct call")
        with pytest.raises(hs.HsError) as e:   # a ticket is waited once
            sq.wait(tickets[3])
        assert e.value.status == hs.HS_ERR_INVALID
    sq.close()


# ---- 2. the case the feature exists for ---------------------------------------------------------------------------------------
def test_large_coalesced_launch_takes_the_large_batch_plan(hs, files):
    """8 x 800 rows: each direct call is planned as a small launch, the coalesced one as descent / order / level-0 search.
    What this can observe: the plan is a pure function of nq (read here for 6400 and for 800), the queue reports ONE launch of 6400
    rows, and the backend hands that launch to search_dev whole -- so the launch group was planned for nq = 6400.  The plan's name is
    the kernel family only and is the same for both shapes: nothing read back from the device says which shape ran."""
    ix, mode, _ = open_index(hs, files, "slim_d128_int_flat")
    n, d = SHAPES["d128"][:2]
    q = mixture(6400, d, seed=21, integer=True)
    ix.set_ef(64)
    big = hs.debug_search_plan(hs.debug_plan_input(ix, K, 6400))
    small = hs.debug_search_plan(hs.debug_plan_input(ix, K, 800))
    assert big["split"] == 1 and small["split"] == 0, "the coalesced launch must be planned differently from its segments"
    sq = hs.SearchQueue(ix, K, mode, max_queries=8192, slots=2)
    tickets = [sq.submit(q[s], want_dists=True, want_stats=True) for s in segments([800] * 8)]
    results = [sq.wait(t) for t in tickets]
    info = sq.info()
    assert info["launches"] == 1 and info["largest_launch"] == 6400   # ... so the launch group was planned for nq = 6400: `big`
    assert ix.last_kernel() == big["name"]
    same(concat(results), direct(hs, ix, mode, q), "6400 rows against one direct call")
    for r, s in zip(results, segments([800] * 8)):
        same(r, direct(hs, ix, mode, q[s]), f"rows {s.start}.. against their own (unsplit) direct call")
    sq.close()


# ---- 3. segment shapes --------------------------------------------------------------------------------------------------------
def test_300_single_row_device_submissions_and_65_segments(hs, files):
    """300 segments: the row prefix is searched in global memory (more than the 256 the kernels keep in LDS); 65: in LDS."""
    import torch
    ix, mode, q = open_index(hs, files, "slim_d16")
    ix.set_ef(64)
    dev = torch.device("cuda:0")
    dq = torch.from_numpy(q.copy()).to(dev)
    sq = hs.SearchQueue(ix, K, mode, max_queries=512, slots=2)
    tickets = [dev_submit(hs, sq, dq[i:i + 1]) for i in range(300)]
    sq.wait(tickets[150])
    assert sq.info()["launches"] == 1 and sq.info()["largest_launch"] == 300
    for t in tickets[:150] + tickets[151:]:
        sq.wait(t)
    want = direct(hs, ix, mode, q[:300])
    same(concat([dev_result(hs, sq, t) for t in tickets]), want, "300 single-row device submissions")
    sizes = [1 + i % 5 for i in range(65)]   # 65 segments, 195 rows, host
    tickets = [sq.submit(q[s], want_dists=True, want_stats=True) for s in segments(sizes)]
    results = [sq.wait(t) for t in tickets]
    assert sq.info()["launches"] == 2 and sq.info()["largest_launch"] == 300
    same(concat(results), direct(hs, ix, mode, q[:sum(sizes)]), "65 host segments")
    sq.close()


@pytest.mark.parametrize("name", ["hnsw_d10", "hnsw_d21_ip", "slim_d16"])
def test_device_sources_off_the_16_byte_boundary(hs, files, name):
    """A torch slice that starts 4 bytes past a 16-byte boundary: d = 10 and d = 21 rows never take the 16-byte path, d = 16 rows
    would by their length and must not by their address."""
    import torch
    if name == "hnsw_d10":
        hp, _, q = files["d10"]
        ix, mode = hs.Index(hp, hs.HS_KIND_HNSW, 10), hs.HS_MODE_PQ
    else:
        ix, mode, q = open_index(hs, files, name)
    ix.set_ef(64)
    d, nq = q.shape[1], 40
    dev = torch.device("cuda:0")
    flat = torch.zeros(nq * d + 1, dtype=torch.float32, device=dev)
    flat[1:] = torch.from_numpy(q[:nq].copy()).to(dev).reshape(-1)
    dq = flat[1:].view(nq, d)
    assert dq.data_ptr() % 16 == 4 and dq.is_contiguous()
    sq = hs.SearchQueue(ix, K, mode, max_queries=64, slots=1)
    a, b = dev_submit(hs, sq, dq[:13]), dev_submit(hs, sq, dq[13:])   # the second starts at 4 + 13 * d * 4 bytes
    sq.wait(a), sq.wait(b)
    assert sq.info()["launches"] == 1
    same(concat([dev_result(hs, sq, a), dev_result(hs, sq, b)]), direct(hs, ix, mode, q[:nq]), name)
    sq.close()


def test_host_and_device_mixed_and_outputs_partly_absent(hs, files):
    import torch
    ix, mode, q = open_index(hs, files, "slim_d16")
    assert mode == hs.HS_MODE_SLIM_IDS
    ix.set_ef(64)
    dev = torch.device("cuda:0")
    dq = torch.from_numpy(q.copy()).to(dev)
    sq = hs.SearchQueue(ix, K, mode, max_queries=256, slots=2)
    cuts = [slice(0, 7), slice(7, 8), slice(8, 40), slice(40, 41), slice(41, 90), slice(90, 100)]
    t = [sq.submit(q[cuts[0]], want_dists=False, want_stats=False),          # labels and counts only
         dev_submit(hs, sq, dq[cuts[1]], want_dists=False, want_stats=True),
         sq.submit(q[cuts[2]], want_dists=True, want_stats=False),
         dev_submit(hs, sq, dq[cuts[3]], want_dists=True, want_stats=False),
         sq.submit(q[cuts[4]], want_dists=False, want_stats=True),
         dev_submit(hs, sq, dq[cuts[5]], want_dists=True, want_stats=True)]
    for x in t:
        sq.wait(x)
    assert sq.info()["launches"] == 1 and sq.info()["largest_launch"] == 100
    want = direct(hs, ix, mode, q[:100])
    for x, s in zip(t, cuts):
        r = dev_result(hs, sq, x) if x.device else x.result()
        assert r["labels"] is not None and r["cnt"] is not None
        same(r, want, f"rows {s.start}..{s.stop}", rows=s)
    assert t[0].dists is None and t[0].stats is None and t[1].dists is None and t[3].stats is None
    # a launch in which nobody asked for distances or stats
    u = [sq.submit(q[s], want_dists=False, want_stats=False) for s in (slice(0, 3), slice(3, 9))]
    for x, s in zip(u, (slice(0, 3), slice(3, 9))):
        same(sq.wait(x), want, "labels only", rows=s)
    sq.close()


def test_pageable_rows_are_copied_at_submit_and_page_locked_rows_serve_in_place(hs, files):
    ix, mode, q = open_index(hs, files, "slim_d128_int_flat")
    ix.set_ef(64)
    want = direct(hs, ix, mode, q[:60])
    sq = hs.SearchQueue(ix, K, mode, max_queries=64, slots=1)
    mine = q[:20].copy()                               # pageable: free again when submit returns
    a = sq.submit(mine, want_dists=True, want_stats=True)
    mine[:] = 0
    pin = hs.PinnedArray((40, q.shape[1]), np.float32)   # page-locked and device-mapped: gathered where it lies
    assert pin.device_view() is not None
    pin.a[:] = q[20:60]
    b = sq.submit(pin.a[:15], want_dists=True, want_stats=True)
    c = sq.submit(pin.a[15:], want_dists=True, want_stats=True)   # a source that starts inside the allocation
    same(concat([sq.wait(t) for t in (a, b, c)]), want, "pageable and page-locked sources in one launch")
    assert sq.info()["launches"] == 1
    sq.close()


def test_k_1_k_above_the_index_size_and_an_empty_index(hs, files, tmp_path):
    ix, mode, q = open_index(hs, files, "slim_d16")
    ix.set_ef(64)
    sq = hs.SearchQueue(ix, 1, mode, max_queries=64, slots=1)   # k = 1: a result row is narrower than the four stats columns
    t = [sq.submit(q[s], want_dists=True, want_stats=True) for s in segments([1, 2, 30])]
    same(concat([sq.wait(x) for x in t]), direct(hs, ix, mode, q[:33], k=1), "k = 1")
    sq.close()
    # five rows, k = 10: counts below k, the padding is scattered too
    x = mixture(5 + 20, 16, seed=3)
    hp, sp = str(tmp_path / "h5.bin"), str(tmp_path / "s5.bin")
    hs.build_hnsw(x[:5], hp, M=8, ef_construction=60)
    hs.convert_slim(hp, sp, 16)
    for ix5, mode5 in ((hs.Index(hp, hs.HS_KIND_HNSW, 16), hs.HS_MODE_PQ), (hs.Index(sp, hs.HS_KIND_SLIM, 16), hs.HS_MODE_SLIM_IDS)):
        ix5.set_ef(64)
        sq = hs.SearchQueue(ix5, K, mode5, max_queries=64, slots=1)
        t = [sq.submit(x[5:][s], want_dists=True, want_stats=True) for s in segments([3, 1, 16])]
        got, want = concat([sq.wait(y) for y in t]), direct(hs, ix5, mode5, x[5:])
        assert (want["cnt"] == 5).all() and np.isinf(want["dists"][:, 5:]).all()
        same(got, want, "five rows, k = 10")
        sq.close()
    # an index without elements: count 0 and padding for every query, no search kernel
    empty = np.zeros((0, 16), np.float32)
    for kind, mode0 in ((hs.HS_KIND_HNSW, hs.HS_MODE_PQ), (hs.HS_KIND_SLIM, hs.HS_MODE_SLIM_IDS)):
        ix0 = hs.Index.from_arrays(kind, hs.HS_METRIC_L2, empty, [], [], 0, 0)
        sq = hs.SearchQueue(ix0, K, mode0, max_queries=64, slots=1)
        t = [sq.submit(x[5:][s], want_dists=True, want_stats=True) for s in segments([2, 5])]
        got, want = concat([sq.wait(y) for y in t]), direct(hs, ix0, mode0, x[5:12])
        assert (want["cnt"] == 0).all()
        same(got, want, "empty index")
        sq.close()


# ---- 4. auto-flush and slots --------------------------------------------------------------------------------------------------
def test_auto_flush_at_max_queries_and_one_slot_in_order(hs, files):
    ix, mode, q = open_index(hs, files, "hnsw_d20_pq")
    ix.set_ef(64)
    want = direct(hs, ix, mode, q)
    sq = hs.SearchQueue(ix, K, mode, max_queries=64, slots=2)
    sizes = [30, 30, 10, 54, 1, 64, 5]   # launches: 60 | 10 + 54 = 64 | 1 then 64 would be 65: 1 | 64 | 5 left pending
    tickets, seen = [], []
    for s in segments(sizes):
        tickets.append(sq.submit(q[s], want_stats=True))
        i = sq.info()
        seen.append((i["launches"], i["pending"]))
    assert seen == [(0, 30), (0, 60), (1, 10), (1, 64), (2, 1), (3, 64), (4, 5)]
    with pytest.raises(hs.HsError) as e:   # more than max_queries in one submission: refused, nothing changes
        sq.submit(q[:65])
    assert e.value.status == hs.HS_ERR_INVALID and sq.info()["pending"] == 5 and sq.info()["submitted"] == sum(sizes)
    zero = sq.submit(q[:0])                # nothing to search: complete at once, launches nothing
    assert sq.wait(zero)["labels"].shape == (0, K) and sq.info()["launches"] == 4
    results = [sq.wait(t) for t in reversed(tickets)][::-1]
    assert sq.info()["launches"] == 5 and sq.info()["largest_launch"] == 64 and sq.info()["in_flight"] == 0
    same(concat(results), want, "auto-flushed launches", rows=slice(0, sum(sizes)))
    sq.close()
    one = hs.SearchQueue(ix, K, mode, max_queries=64, slots=1)   # one slot: the second and third flush complete the launch before
    tickets = []
    for s in segments([3, 4, 5]):
        tickets.append(one.submit(q[s], want_stats=True))
        one.flush()
        assert one.info()["in_flight"] == 1 and one.info()["launches"] == len(tickets)
    one.drain()
    assert one.info()["in_flight"] == 0
    same(concat([t.result() for t in tickets]), want, "slots = 1", rows=slice(0, 12))
    with pytest.raises(hs.HsError):        # drain released every ticket
        one.wait(tickets[0])
    one.close()


# ---- 5. filter set ------------------------------------------------------------------------------------------------------------
def test_filter_set_segments_and_a_filter_index_outside_the_set(hs, files):
    ix, _, q = open_index(hs, files, "hnsw_d20_pq")
    n = SHAPES["d20"][0]
    ix.set_ef(64)
    rng = np.random.default_rng(4)
    filt = np.stack([np.ones(n, bool), rng.random(n) < 0.5, rng.random(n) < 0.1]).astype(np.uint8)
    fs = hs.FilterSet.create(ix, 3)
    fs.write(0, filt)
    foq = (np.arange(NQ) % 3).astype(np.uint32)
    want = ix.search_filter_set(q[:60], K, fs, foq[:60], want_stats=True)
    sq = hs.SearchQueue(ix, K, hs.HS_MODE_PQ, max_queries=128, slots=2, fs=fs)
    cuts = list(segments([1, 9, 20, 30]))
    tickets = [sq.submit(q[s], filter_of_query=foq[s], want_stats=True) for s in cuts]
    same(concat([sq.wait(t) for t in tickets]), want, "segments under different filters")
    assert sq.info()["launches"] == 1
    # one query of one segment names filter 3 of a set of 3: every ticket of that launch reports it, that query has count 0 and
    # padding, the others their answers; the next launch is clean
    bad = foq[:20].copy()
    bad[14] = 3
    tickets = [sq.submit(q[s], filter_of_query=bad[s], want_stats=True) for s in (slice(0, 10), slice(10, 20))]
    for t in tickets:
        with pytest.raises(hs.HsError) as e:
            sq.wait(t)
        assert e.value.status == hs.HS_ERR_INVALID
    got = concat([t.result() for t in tickets])
    assert got["cnt"][14] == 0 and (got["labels"][14] == np.uint64(0xFFFFFFFFFFFFFFFF)).all() and np.isinf(got["dists"][14]).all()
    keep = np.arange(20) != 14
    for key in ("labels", "dists", "cnt"):
        assert got[key][keep].tobytes() == want[key][:20][keep].tobytes(), key
    clean = sq.submit(q[:20], filter_of_query=foq[:20], want_stats=True)
    same(sq.wait(clean), want, "the launch after the reported one", rows=slice(0, 20))
    sq.close()


# ---- 6. device stream ordering ------------------------------------------------------------------------------------------------
def test_device_stream_ordering_without_a_host_synchronisation(hs, files):
    """The queries are produced by torch work on a side stream right before submit_dev(stream=...), the results are read by torch
    on that stream after join_stream: no host synchronisation between the two."""
    import torch
    ix, mode, q = open_index(hs, files, "slim_d128_int_flat")
    ix.set_ef(64)
    want = direct(hs, ix, mode, q[:200])
    dev = torch.device("cuda:0")
    half = torch.from_numpy((q[:200] / 2).copy()).to(dev)   # (integer rows: halving and doubling are exact)
    torch.cuda.synchronize()
    st = torch.cuda.Stream(device=dev)
    sq = hs.SearchQueue(ix, K, mode, max_queries=256, slots=2)
    with torch.cuda.stream(st):
        big = torch.zeros((4096, 4096), device=dev)
        for _ in range(20):
            big = torch.cos(big) + 1.0                       # keeps the stream busy ahead of the producer
        dq = half * 2.0 + big[0, 0] * 0.0                    # the queries exist only once `st` gets here
        t = dev_submit(hs, sq, dq, stream=st.cuda_stream)
        sq.join_stream(t, st.cuda_stream)                    # flushes; `st` now waits for the launch, the host does not
        lab, dist, cnt, stats = t.labels.clone(), t.dists.clone(), t.cnt.clone(), t.stats.clone()
    st.synchronize()
    got = dict(labels=lab.cpu().numpy().view(np.uint32), dists=dist.cpu().numpy(), cnt=cnt.cpu().numpy().view(np.uint32),
               stats=stats.cpu().numpy().view(np.uint32))
    same(got, want, "results read on the caller's stream")
    sq.wait(t)                                               # the ticket is still the caller's to release
    sq.close()


# ---- 7. threads ---------------------------------------------------------------------------------------------------------------
def test_sixteen_threads_of_single_queries(hs, files):
    ix, mode, q = open_index(hs, files, "slim_d16")
    ix.set_ef(64)
    want = direct(hs, ix, mode, q[:320])
    sq = hs.SearchQueue(ix, K, mode, max_queries=64, slots=2)
    got, errors = [None] * 320, []

    def client(t):
        try:
            for i in range(t * 20, t * 20 + 20):
                got[i] = sq.wait(sq.submit(q[i:i + 1], want_dists=True, want_stats=True))
        except Exception as e:   # noqa: BLE001 -- reported below
            errors.append(repr(e))

    threads = [threading.Thread(target=client, args=(t,), daemon=True) for t in range(16)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(timeout=120)
    assert not any(th.is_alive() for th in threads), "a client thread is still waiting"
    assert not errors, errors
    same(concat(got), want, "16 threads x 20 single queries")
    info = sq.info()
    assert info["submitted"] == 320 and 1 <= info["launches"] <= 320 and info["pending"] == 0 and info["in_flight"] == 0
    sq.close()


# ---- 8. refusals --------------------------------------------------------------------------------------------------------------
def test_refusals(hs, files, tmp_path):
    def refused(call, status=None):
        with pytest.raises(hs.HsError) as e:
            call()
        assert e.value.status == (hs.HS_ERR_INVALID if status is None else status)

    ix, mode, q = open_index(hs, files, "slim_d16")
    hx, _, _ = open_index(hs, files, "hnsw_d20_pq")
    before = direct(hs, ix, mode, q[:20])
    refused(lambda: hs.SearchQueue(hx, K, hs.HS_MODE_SLIM_IDS))              # searchKnn(q, k, tableint*) is the Slim index's
    refused(lambda: hs.SearchQueue(ix, 0, mode))                             # k == 0
    refused(lambda: hs.SearchQueue(ix, K, 2))                                # no such mode
    for mq, slots in ((0, 2), (32769, 2), (64, 0), (64, 17)):
        refused(lambda: hs.SearchQueue(ix, K, mode, max_queries=mq, slots=slots))
    hp, sp, _ = files["d128"]
    qp = str(tmp_path / "q.bin")
    hs.convert_slimq(sp, 0, 128, mixture(8, 128, seed=1, integer=True), qp, threads=4)
    qx = hs.Index(qp, hs.HS_KIND_SLIMQ, 128)
    refused(lambda: hs.SearchQueue(qx, K, hs.HS_MODE_PQ))                    # a SlimQ index
    fs = hs.FilterSet.create(hx, 2)
    other = hs.Index(files["d10"][0], hs.HS_KIND_HNSW, 10)
    refused(lambda: hs.SearchQueue(other, K, hs.HS_MODE_PQ, fs=fs))          # a set of another index size (2003 ids against 1000)
    sfs = hs.FilterSet.create(ix, 2)
    refused(lambda: hs.SearchQueue(ix, K, hs.HS_MODE_SLIM_IDS, fs=sfs))      # a filter set answers in HS_MODE_PQ only
    fq = hs.SearchQueue(hx, K, hs.HS_MODE_PQ, fs=fs)
    refused(lambda: fq.submit(files["d20"][2][:4]))                          # ... and wants a filter per query
    assert fq.info()["submitted"] == 0
    fq.close()
    sq = hs.SearchQueue(ix, K, mode, max_queries=32, slots=1)
    refused(lambda: sq.submit(q[:33]))
    refused(lambda: sq.wait(hs.QueueTicket(12345)))                          # an unknown ticket
    refused(lambda: sq.join_stream(hs.QueueTicket(12345)))
    L = hs.lib()
    import ctypes
    t = ctypes.c_uint64(0)
    qq = np.ascontiguousarray(q[:2])
    assert L.hs_queue_submit(sq._h, qq.ctypes.data, 2, None, None, None, None, None, None, ctypes.byref(t)) == hs.HS_ERR_INVALID   # labels32 required
    assert sq.info()["submitted"] == 0 and sq.info()["launches"] == 0
    t1 = sq.submit(q[:20], want_dists=True, want_stats=True)
    same(sq.wait(t1), before, "after the refusals")
    refused(lambda: sq.wait(t1))                                             # a second wait
    sq.close()
    sq.close()


def test_python_queue_keeps_dropped_tickets_alive(hs, files):
    """The numpy arrays of a host submission are the ticket's; the queue holds their addresses until the launch is done, so it holds
    the ticket too: a caller may drop it and drain."""
    import gc
    ix, mode, q = open_index(hs, files, "slim_d16")
    ix.set_ef(64)
    sq = hs.SearchQueue(ix, K, mode, max_queries=64, slots=1)
    for s in segments([5, 7]):
        sq.submit(q[s], want_dists=True, want_stats=True)   # tickets dropped at once
    gc.collect()
    assert len(sq._out) == 2
    sq.drain()
    assert not sq._out
    kept = sq.submit(q[:3])
    sq.submit(q[3:6])
    same(sq.wait(kept), direct(hs, ix, mode, q[:3]), "after the drain", rows=slice(None))
    assert len(sq._out) == 1
    sq.close()
    assert not sq._out


# ---- 9. facade ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["hnsw", "slim"])
def test_facade_queue(hs, files, tmp_path, kind):
    """hnswlib::SearchQueue<float> through hnswlib_amd.h: submit / wait of 1-, 2- and 3-row batches in one launch, then 8 threads
    calling its searchKnn(q, k) one query at a time."""
    exe = os.path.join(ROOT, "hnsw-slim_amd", "facade_queue")
    assert os.path.exists(exe), "facade_queue is built by `make -C hnsw-slim_amd all`"
    hp, sp, q = files["d16"]
    d, nq, ef, threads = 16, 120, 64, 8
    qf, out = str(tmp_path / "q.f32"), str(tmp_path / "out.bin")
    q[:nq].tofile(qf)
    subprocess.check_call([exe, kind, hp if kind == "hnsw" else sp, str(d), qf, str(nq), str(K), str(ef), str(threads), out], timeout=300)
    ix = hs.Index(hp, hs.HS_KIND_HNSW, d) if kind == "hnsw" else hs.Index(sp, hs.HS_KIND_SLIM, d)
    ix.set_ef(ef)
    want = ix.search_pq(q[:nq], K)
    buf, nA = open(out, "rb").read(), nq // 2
    launches, largest = np.frombuffer(buf, np.uint64, 2, 0)
    assert launches == 1 and largest == nA
    off = 16
    labels = np.frombuffer(buf, np.uint64, nA * K, off).reshape(nA, K); off += nA * K * 8
    dists = np.frombuffer(buf, np.float32, nA * K, off).reshape(nA, K); off += nA * K * 4
    cnt = np.frombuffer(buf, np.uint32, nA, off); off += nA * 4
    same(dict(labels=labels, dists=dists, cnt=cnt), want, "submit / wait", rows=slice(0, nA))
    for i in range(nA, nq):
        c = int(np.frombuffer(buf, np.uint32, 1, off)[0]); off += 4
        rec = np.frombuffer(buf, np.dtype([("d", "<f4"), ("l", "<u8")]), c, off); off += 12 * c
        assert c == int(want["cnt"][i]), i
        got = sorted(zip(rec["d"].view(np.uint32).tolist(), rec["l"].tolist()))
        assert got == sorted(zip(want["dists"][i, :c].view(np.uint32).tolist(), want["labels"][i, :c].tolist())), i
        assert list(rec["d"]) == sorted(rec["d"], reverse=True), i   # a priority_queue pops the farthest first
    assert off == len(buf)
