"""The search shape bench.py times, against the oracle: d=128 with the compiled-in flat kernel (flat_kernel<L2, 1 | 2 | 3, 8>,
flat_search.hip:989-994), batches on both sides of kOrderMinQueries (search_plan.hpp: from 6144 queries a launch runs as descent /
order / level-0 search), the device entry search_ids_dev on non-default streams with two batches in flight.

The index is the bench's: headline_data(50 000, 128, 123), M=16, efC=200, branching factor 4, seed 100, Slim defaults.  For every
shape: the kernel that ran is the flat one, the label sets equal searchKnn(q, k, tableint*)'s, the counters equal, and the sorted
fp32 distances are bit-identical to the oracle's.  The distances are taken from the oracle's priority-queue overload with its
enter-point pre-mark switched off: the id-array overload under test does not tag the enter point before the descent
(hnswalg_slim.h:2036-2038, oracle/hs_oracle.hpp slim_search_core), the (q, k) overload does (:1919), and with the tag the two
overloads may search differently for a query whose result contains the enter point.
"""
import numpy as np
import pytest

from hsutil import headline_data, load_product

pytestmark = pytest.mark.gpu
N, D, K = 50_000, 128, 10
NQS = (6143, 6144, 10_000)
EFS = (64, 65, 70, 128, 129)


@pytest.fixture(scope="module")
def hs():
    m = load_product()
    assert m.device_count() > 0, "no HIP device visible"
    return m


@pytest.fixture(scope="module")
def bench_index(hs, oracle, tmp_path_factory):
    """(device index, oracle index, base rows) of the bench's workload at 50 000 rows, built once."""
    d = tmp_path_factory.mktemp("bench_shape")
    base = headline_data(N, D, 123)
    hp, sp = str(d / "hnsw.bin"), str(d / "slim.bin")
    hs.build_hnsw(base, hp, M=16, ef_construction=200, branching_factor="4", seed=100, threads=16)
    hs.convert_slim(hp, sp, D, threads=16)
    return hs.Index(sp, hs.HS_KIND_SLIM, D, hs.HS_METRIC_L2), oracle.load(sp, "slim", 0, D), base


_want_cache = {}


def oracle_answer(ox, q, ef, key):
    """Sorted labels, counters and sorted distances of the oracle for queries q at ef (cached by key)."""
    if (key, ef) not in _want_cache:
        ox.set_ef(ef)
        ids = ox.search_ids(q, K, threads=16)
        ox.set_mark_ep(0)
        try:
            pq = ox.search_pq(q, K, threads=16)
        finally:
            ox.set_mark_ep(-1)
        assert np.all(pq["cnt"] == K)
        _want_cache[(key, ef)] = dict(labels=np.sort(ids["labels"], axis=1), counters=ids["counters"][:, :3],
                                      dists=np.sort(pq["dists"], axis=1))
    return _want_cache[(key, ef)]


def check(ix, want, labels, dists, stats, what):
    assert ix.last_kernel() == "hs::flat_kernel", what
    assert np.array_equal(np.sort(labels.astype(np.uint32), axis=1), want["labels"]), f"{what}: label sets differ"
    assert np.array_equal(stats[:, :3].astype(np.uint32), want["counters"]), f"{what}: counters differ"
    assert np.sort(dists, axis=1).view(np.uint32).tobytes() == want["dists"].view(np.uint32).tobytes(), f"{what}: distances differ"


@pytest.mark.parametrize("nq", NQS)
def test_bench_shape_host_entry_matches_oracle(hs, bench_index, nq):
    ix, ox, _ = bench_index
    q = headline_data(nq, D, 456)
    for ef in EFS:
        ix.set_ef(ef)
        r = ix.search_ids(q, K, want_dists=True, want_stats=True)
        check(ix, oracle_answer(ox, q, ef, ("host", nq)), r["labels"], r["dists"], r["stats"], f"nq={nq} ef={ef}")
        replays = int((r["stats"][:, 3] == 1).sum())
        print(f"nq={nq} ef={ef}: {replays} queries took the tie re-run")
        # measured on an MI355X: 1 or 2 queries at every shape here; a count of zero means the tie path went unexercised
        assert replays > 0, f"nq={nq} ef={ef}: no query took the tie re-run"


def test_bench_shape_device_entry_two_streams_matches_oracle(hs, bench_index):
    """What the bench times: search_ids_dev on torch device tensors, two 10 000-query batches (the bench's query seeds 456 and 457)
    in flight at once on two non-default streams."""
    import torch
    ix, ox, _ = bench_index
    dev = torch.device("cuda", 0)
    qs = [headline_data(10_000, D, 456 + b) for b in range(2)]
    q_dev = [torch.from_numpy(q).to(dev) for q in qs]
    streams = [torch.cuda.Stream(device=dev) for _ in range(2)]
    torch.cuda.synchronize()
    for ef in EFS:
        ix.set_ef(ef)
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
        for b in range(2):
            lab, dst, cnt, sts = (t.cpu().numpy() for t in outs[b])
            assert np.all(cnt == K)
            check(ix, oracle_answer(ox, qs[b], ef, ("dev", b)), lab, dst, sts, f"device entry, batch {b}, ef={ef}")


@pytest.mark.parametrize("case", ("one_query_6200_times", "6200_base_rows"))
def test_bench_shape_degenerate_order_inputs(hs, bench_index, case):
    """6200 queries (above kOrderMinQueries): all one query, so every entry key of order_kernel is equal (its hi == lo path,
    beam_search.hip:1221); or exact base rows, each at distance 0 from its own node."""
    ix, ox, base = bench_index
    if case == "one_query_6200_times":
        q = np.ascontiguousarray(np.repeat(headline_data(1, D, 456), 6200, axis=0))
    else:
        q = np.ascontiguousarray(base[np.random.default_rng(11).choice(N, 6200, replace=False)])
    for ef in (64, 70, 129):
        ix.set_ef(ef)
        r = ix.search_ids(q, K, want_dists=True, want_stats=True)
        check(ix, oracle_answer(ox, q, ef, case), r["labels"], r["dists"], r["stats"], f"{case} ef={ef}")
