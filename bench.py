#!/usr/bin/env python3
"""bench.py -- QPS @ recall@10 >= 0.95 of the batched HNSW-Slim search on SIFT-1M-like data (BASELINE.json configs[1]).

Metric: queries / wall second of the batched search call INCLUDING the H2D copy of the queries and the D2H
copy of the labels, index upload excluded -- the clock runs around the whole query loop as in the reference's
HnswSlimStrategy::solve (include/strategy/hnsw_slim_strategy.h:107-118).

One "step" = a block of `--batches-per-step` (100) batches of 10 000 queries.  Every batch is a DISTINCT pre-generated
query set in page-locked host memory (8 sets, rotated); a batch is: H2D of its queries, the search
(HierarchicalNSWSlim::searchKnn(q,k,tableint*) for every query), D2H of its labels.  Batches are issued round-robin on
`--streams` HIP streams through the C ABI's asynchronous host-pointer entry (hs_search_batch_async), so copies and
kernels of consecutive batches overlap as in a serving loop; 20 steps = 2000 batches (about 2 s) inside the timed region.
Every batch's labels are CONSUMED before its output buffer is reused: the host waits on the batch's event and compares a
checksum of the labels that came back with the reference answers of that query set (the last batch of every stream is
compared label by label), and hs_search_check's counters are sticky, so a capacity failure in any batch is reported.
Workload: SIFT-1M-like d=128 L2, M=16 efC=200, Slim defaults, k=10; ef_search = the smallest value of the sweep whose
recall@10 >= 0.95 on this data (the points evaluated are reported in `config.sweep`; with `--full`, all of them, timed).

Multi-GPU (torchrun, one rank per GPU): the index is replicated; `--scaling strong` (the default for N > 1): ONE 10k batch is
split into contiguous shards over the ranks (BASELINE.json configs[3]) and the per-rank top-k labels are joined by one RCCL
all-gather per batch -- this is `value`; the weak figure (every rank searches its own 10k batches) is measured right after on a
shorter region and reported as a side field (`--full`).  Only rank 0 computes ground truth and chooses ef; the ranks share its choice.

A plain run does only what `value` needs: load the index, ground truth, ef ascending until recall@10 >= 0.95, the reference
answers of the query sets, warm-up, the timed steps, the result line.  `--full` adds what takes runs of its own: the whole ef
sweep with per-point launch timing, the weak-scaling side figure, the single-launch / device-resident / synchronous-entry side
figures with the single-launch roofline, and the CPU baseline (unless `--no-cpu-baseline`).

Data + index: built once into the user's cache directory (`$XDG_CACHE_HOME` or `~/.cache`, under hnsw-slim-amd/bench/) --
`__graft_entry__.build()` does it through `--prepare-only` -- and loaded from there; `--index-dir` uses (or fills) a directory
of your choice instead.  The data and the queries are seeded, and the graph is built by the serial addPoint loop (the
reference's own build order; about ten minutes of one core at 1M), so every build of the index is the same file and every run
computes the same labels.  (`--build-threads N` builds faster, but a parallel build's graph depends on thread timing.)

`--dump-outputs DIR` writes, after the timed steps, the labels the timed path returned for each query set in its last step as
DIR/labels_qset<b>.npy (float64, [queries, k]; at most 64 MiB in all, else a fixed row sample plus <name>_rows.npy).

Prints ONE JSON line (rank 0).  See DESIGN.md "Measurement" for the roofline accounting.
"""
import argparse
import hashlib
import inspect
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hsutil  # noqa: E402
from hsutil import headline_data, load_product  # noqa: E402

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak (MI355X_MICROARCH.md); ~6300 GB/s measured achievable
DATA_DESC = ("synthetic: tests/hsutil.py::headline_data (4096-component mixture of rank-12 Gaussians + sigma=4 isotropic noise, "
             "rounded to integers in [0,255]; builder-calibrated -- SURVEY.md 8d's isotropic mixture is un-indexable by HNSW-Slim at 1M, "
             "profiles/r01_calib_isotropic_vs_lowrank.log); base seed 123, query batch b of rank r seed 456+100r+b")


DUMP_LIMIT_BYTES = 64 << 20
T0 = time.perf_counter()   # (near) process start: the setup-time marks in the log


def log(*a):
    print("[bench]", *a, file=sys.stderr, flush=True)


def default_threads():
    """CPU threads for the Slim conversion (deterministic at any thread count): OMP_NUM_THREADS where the job is given a CPU
    budget, else the usable cores (at most 64)."""
    env = os.environ.get("OMP_NUM_THREADS", "")
    if env.isdigit() and int(env) > 0:
        return int(env)
    return min(len(os.sched_getaffinity(0)) or 8, 64)


def graph_tag(build_threads):
    """The serial build (1 thread, the default) is the reference's addPoint loop and the same graph on every run; a parallel
    build inserts in whatever order its threads reach the points, so its graph -- and the labels searched on it -- vary."""
    return "serial" if build_threads == 1 else f"threads{build_threads}"


def index_cache_dir(n, d, build_threads=1):
    """Default home of the bench's data + index, keyed by the shape, the build mode and the code that makes them (generator,
    builder)."""
    h = hashlib.sha256()
    with open(os.path.join(ROOT, "hnsw-slim_amd", "csrc", "host_graph.hpp"), "rb") as f:
        h.update(f.read())
    for fn in (hsutil._lowrank_clusters, hsutil.sift_like, hsutil.headline_data):
        h.update(inspect.getsource(fn).encode())
    root = os.environ.get("XDG_CACHE_HOME") or os.path.join(os.path.expanduser("~"), ".cache")
    return os.path.join(root, "hnsw-slim-amd", "bench", f"sift-like_n{n}_d{d}_M16_efc200_{graph_tag(build_threads)}_{h.hexdigest()[:12]}")


def prepare_index(idir, n, d, build_threads, hs, keep_hnsw=True):
    """base.npy, slim.bin (and hnsw.bin if keep_hnsw) of the workload in idir; the `ready` marker is written last.
    Returns (build seconds, convert seconds): zeros when idir was already complete."""
    hpath, spath, bpath, ready = (os.path.join(idir, f) for f in ("hnsw.bin", "slim.bin", "base.npy", "ready"))
    if os.path.exists(spath) and os.path.exists(bpath) and os.path.exists(ready):
        return 0.0, 0.0
    os.makedirs(idir, exist_ok=True)
    t0 = time.time()
    base = headline_data(n, d, 123)
    log(f"generated base {base.shape} in {time.time() - t0:.1f}s; building HNSW M=16 efC=200 with {build_threads} thread(s)")
    t0 = time.time()
    hs.build_hnsw(base, hpath, M=16, ef_construction=200, branching_factor="4", seed=100, threads=build_threads)
    t_build = time.time() - t0
    t0 = time.time()
    hs.convert_slim(hpath, spath, d, threads=default_threads())
    t_conv = time.time() - t0
    np.save(bpath, base)
    if not keep_hnsw:
        os.remove(hpath)
    with open(ready, "w") as f:
        f.write("ok")
    log(f"build {t_build:.1f}s, convertFromHNSW {t_conv:.1f}s")
    return t_build, t_conv


def prepare_cached(n, d, build_threads, hs):
    """prepare_index into index_cache_dir(n, d), staged in a sibling directory and renamed into place when complete, so an
    interrupted build never leaves a directory that looks ready.  Returns (directory, build s, convert s)."""
    idir = index_cache_dir(n, d, build_threads)
    if os.path.exists(os.path.join(idir, "ready")):
        return idir, 0.0, 0.0
    stage = f"{idir}.part{os.getpid()}"
    shutil.rmtree(stage, ignore_errors=True)
    t_build, t_conv = prepare_index(stage, n, d, build_threads, hs, keep_hnsw=False)
    if os.path.isdir(idir) and not os.path.exists(os.path.join(idir, "ready")):
        shutil.rmtree(idir, ignore_errors=True)
    try:
        os.rename(stage, idir)
    except OSError:
        if not os.path.exists(os.path.join(idir, "ready")):
            raise
        shutil.rmtree(stage, ignore_errors=True)   # another process completed it first
    return idir, t_build, t_conv


def dump_outputs(outdir, arrays, limit=DUMP_LIMIT_BYTES):
    """Write every array as outdir/<name>.npy in float64 (labels are integers far below 2**53: exact).  If that would exceed
    `limit` bytes in all, the same fraction of each array's rows is kept -- a sorted sample drawn with seed 0, so identical
    from run to run -- and outdir/<name>_rows.npy holds the row numbers kept.  Returns the names written."""
    os.makedirs(outdir, exist_ok=True)
    arrays = {k: np.asarray(v) for k, v in arrays.items()}
    full_bytes = sum(a.size for a in arrays.values()) * 8
    frac = 1.0
    if full_bytes > limit:   # sampled: every kept row also costs its row number
        frac = limit / sum(a.shape[0] * (a.size // max(a.shape[0], 1) + 1) * 8 for a in arrays.values())
    written = []
    for name, a in arrays.items():
        if frac < 1.0:
            keep = max(1, int(a.shape[0] * frac))
            rows = np.sort(np.random.default_rng(0).choice(a.shape[0], keep, replace=False))
            np.save(os.path.join(outdir, f"{name}_rows.npy"), rows.astype(np.float64))
            written.append(f"{name}_rows")
            a = a[rows]
        np.save(os.path.join(outdir, f"{name}.npy"), a.astype(np.float64))
        written.append(name)
    return written


def ground_truth(torch, base_t, q_t, k, hs):
    """Exact L2 k-NN: the product's exhaustive-scan kernel (BruteforceSearch semantics, exact recipe distances)."""
    lab = torch.empty((q_t.shape[0], k), dtype=torch.int64, device=q_t.device)
    dd = torch.empty((q_t.shape[0], k), dtype=torch.float32, device=q_t.device)
    hs.brute_force_dev(base_t, q_t, k, lab, dd)
    return lab.cpu().numpy()


def recall_at_k(labels, gt):
    hits = 0
    for i in range(labels.shape[0]):
        hits += len(set(labels[i].tolist()) & set(gt[i].tolist()))
    return hits / gt.size


def checksum(labels):
    """Order-independent fingerprint of a [nq, k] label block: (sum, xor) -- two batches with the same per-query label SETS agree."""
    v = np.ascontiguousarray(labels).ravel().astype(np.uint64)
    return int(v.sum()), int(np.bitwise_xor.reduce(v))


def hip_queue_hint(nq, world, scaling):
    """Many SMALL launches in flight (a strong split's per-rank shards: 10 000 / 8 = 1250 queries) are held back by the HIP
    runtime's default of 4 hardware queues, onto which the 16 streams are multiplexed: measured on one MI355X with 1250-query
    batches, 16 in flight, PCIe-inclusive: 5.65 M q/s with 4 queues, 8.36 M with 8, 9.77 M with 16 (profiles/r03_small_batch_queues.log);
    10k-query batches prefer the default (13.8 vs 13.0 M q/s).  The variable is read when the HIP runtime initialises, so it is
    set here, before torch is imported, and only when the caller has not set it.  One process per GPU gets 8 (RCCL brings queues
    of its own, and a device whose hardware queues are oversubscribed time-slices them: two rank processes REHEARSING on one GPU
    with 16 queues each fell to 9 k q/s -- which is why the one-device rehearsal is left alone); a single process gets 16."""
    strong = scaling == "strong" or (scaling == "auto" and world > 1)
    per_rank = nq // world if strong else nq
    if per_rank <= 2500 and os.environ.get("HS_BENCH_ONE_DEVICE") != "1":
        os.environ.setdefault("GPU_MAX_HW_QUEUES", "16" if world == 1 else "8")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--base-size", dest="n", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--batch", dest="nq", type=int, default=10_000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--ef", type=int, default=0, help="fixed ef_search (0 = smallest sweep value with recall>=0.95)")
    ap.add_argument("--build-threads", type=int, default=1, help="threads of the HNSW build: 1 (default) = the serial addPoint loop, the "
                                                                 "same graph on every run; more are faster, but the graph then varies")
    ap.add_argument("--index-dir", default="", help="reuse/build index files here instead of the user cache directory")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cand-cap", type=int, default=0)
    ap.add_argument("--hash-slots", type=int, default=0)
    ap.add_argument("--streams", type=int, default=16, help="HIP streams the batches are issued on round-robin (batches in flight); 1 = strictly serial")
    ap.add_argument("--batches-per-step", type=int, default=100)
    ap.add_argument("--query-sets", type=int, default=8, help="distinct pre-generated query batches rotated through")
    ap.add_argument("--scaling", choices=("auto", "weak", "strong"), default="auto", help="auto: strong (one batch split over the ranks) when --gpus > 1")
    ap.add_argument("--full", action="store_true", help="also the whole ef sweep with launch timing, the side figures, the single-launch "
                                                        "roofline, the weak-scaling side figure and the CPU baseline")
    ap.add_argument("--dump-outputs", metavar="DIR", default="", help="write the labels of the last timed step here (.npy, float64)")
    ap.add_argument("--prepare-only", action="store_true", help="build the data + index (default cache or --index-dir) and exit; no GPU")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    threads = max(1, args.build_threads)
    if args.prepare_only:
        hs = load_product()
        if args.index_dir:
            idir = args.index_dir
            prepare_index(idir, args.n, args.dim, threads, hs)
        else:
            idir, _, _ = prepare_cached(args.n, args.dim, threads, hs)
        log(f"data + index ready in {idir}")
        return
    hip_queue_hint(args.nq, int(os.environ.get("WORLD_SIZE", "1")), args.scaling)

    import torch
    import torch.distributed as dist

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    # rehearsal knobs (1-GPU box): HS_BENCH_ONE_DEVICE=1 maps every rank to cuda:0, HS_BENCH_BACKEND=gloo
    # replaces RCCL (which refuses two ranks on one device); the driver's multi-GPU run uses neither.
    if os.environ.get("HS_BENCH_ONE_DEVICE") == "1":
        local_rank = 0
    backend = os.environ.get("HS_BENCH_BACKEND", "nccl")
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if world > 1:
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(backend)
    assert world == args.gpus, f"--gpus {args.gpus} but WORLD_SIZE={world}"

    hs = load_product()
    import importlib.util
    _sp = importlib.util.spec_from_file_location('hs_sharded', os.path.join(ROOT, 'hnsw-slim_amd', 'sharded.py'))
    sharded = importlib.util.module_from_spec(_sp)
    _sp.loader.exec_module(sharded)
    N, D, NQ, K = args.n, args.dim, args.nq, args.k
    BPS, NB, S = max(1, args.batches_per_step), max(1, args.query_sets), max(1, args.streams)
    strong = world > 1 and args.scaling in ("auto", "strong")
    full_run = args.full

    # ---- data + index: rank 0 builds once (normally already done: the cache) and publishes a marker file; the other ranks
    #      generate their query sets meanwhile and wait on the file system, not inside a collective ---------------------
    tmp = None
    idir = args.index_dir or index_cache_dir(N, D, threads)
    t_build = t_conv = 0.0
    if rank == 0:
        if args.index_dir:
            t_build, t_conv = prepare_index(idir, N, D, threads, hs)
        else:
            try:
                idir, t_build, t_conv = prepare_cached(N, D, threads, hs)
            except OSError as e:
                if world > 1:
                    raise
                log(f"index cache not usable ({e}); building in a temporary directory")
                tmp = tempfile.TemporaryDirectory()
                idir = tmp.name
                t_build, t_conv = prepare_index(idir, N, D, threads, hs, keep_hnsw=False)
    spath, bpath, ready = (os.path.join(idir, f) for f in ("slim.bin", "base.npy", "ready"))
    # query sets: the same global batches on every rank (strong: each rank takes its shard of a batch; weak: each rank searches them whole)
    query_sets = [headline_data(NQ, D, 456 + b) for b in range(NB)]
    while not os.path.exists(ready):
        time.sleep(0.5)
    base = np.load(bpath, mmap_mode="r")
    log(f"data + index ready ({time.perf_counter() - T0:.1f}s since start)")

    ix = hs.Index(spath, hs.HS_KIND_SLIM, D, hs.HS_METRIC_L2, device=local_rank)
    info = ix.info()
    if args.cand_cap or args.hash_slots:
        ix.set_capacity(args.cand_cap, args.hash_slots)
    q_sets_t = [torch.from_numpy(q).to(dev) for q in query_sets]
    q_t = q_sets_t[0]
    d_labels = torch.empty((NQ, K), dtype=torch.int32, device=dev)
    d_counts = torch.empty((NQ,), dtype=torch.int32, device=dev)
    d_stats = torch.empty((NQ, 4), dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def run(ef, q=None, stats=False):
        ix.set_ef(ef)
        ix.search_ids_dev(q_t if q is None else q, K, d_labels, None, d_counts, d_stats if stats else None, stream)
        ix.check(stream)

    # ---- rank 0 only: ground truth, the ef sweep on query set 0 (device-resident, one launch at a time), the operating point:
    #      the smallest sweep ef whose recall@10 >= 0.95 over ALL the query sets of the timed region.  A plain run stops the
    #      sweep at the first ef that passes on set 0 (the one a whole sweep would choose too); --full times every point -----
    sweep, chosen, recall, recalls = {}, 0, 0.0, []
    efs = [args.ef] if args.ef else [32, 48, 64, 68, 70, 72, 80, 96, 128, 192, 256, 384, 512]
    if rank == 0:
        base_t = torch.from_numpy(np.ascontiguousarray(base)).to(dev)
        gts = [ground_truth(torch, base_t, q, K, hs) for q in q_sets_t]
        del base_t
        torch.cuda.empty_cache()
        for ef in efs:
            run(ef, stats=True)
            torch.cuda.synchronize()
            lab = d_labels.cpu().numpy().astype(np.uint32)
            st = d_stats.cpu().numpy().astype(np.int64)
            rec = recall_at_k(lab, gts[0])
            bytes_q = st[:, 0] * 4 * D + st[:, 2] * 4 + st[:, 1] * 8
            point = dict(recall=round(rec, 4))
            if full_run:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                run(ef)
                e0.record()
                for _ in range(3):
                    run(ef)
                e1.record()
                torch.cuda.synchronize()
                ms = e0.elapsed_time(e1) / 3
                point["single_launch_qps"] = round(NQ / ms * 1e3)
            point.update(n_dist=round(float(st[:, 0].mean()), 1), n_hops=round(float(st[:, 1].mean()), 1),
                         bytes_per_query=round(float(bytes_q.mean())), fallback=int((st[:, 3] != 0).sum()))
            if full_run:
                point["alg_GBs"] = round(float(bytes_q.sum()) / ms / 1e6, 1)
            point["kernel"] = ix.last_kernel()
            sweep[ef] = point
            log(f"ef={ef}: {sweep[ef]}")
            if not chosen and rec >= 0.95:
                chosen = ef
                if not args.ef and (not full_run or os.environ.get("HS_BENCH_FULL_SWEEP", "1") == "0"):
                    break
        chosen = chosen or efs[-1]
        while True:
            recalls = []
            for b in range(NB):
                run(chosen, q_sets_t[b])
                torch.cuda.synchronize()
                recalls.append(recall_at_k(d_labels.cpu().numpy().astype(np.uint32), gts[b]))
            recall = float(np.mean(recalls))
            later = [e for e in efs if e > chosen]
            if recall >= 0.95 or args.ef or not later:
                break
            log(f"ef={chosen}: recall@10 {recall:.4f} over the {NB} query sets < 0.95 -> next sweep point")
            chosen = later[0]
    if world > 1:  # every rank times rank 0's operating point
        c = torch.tensor([chosen], device=dev)
        dist.broadcast(c, src=0)
        chosen = int(c.item())
    # reference answers (this rank's own device) + algorithmic bytes of every query set at the operating point
    ix.set_ef(chosen)
    ref_labels, ref_sums, alg_bytes = [], [], []
    for b in range(NB):
        run(chosen, q_sets_t[b], stats=True)
        torch.cuda.synchronize()
        st = d_stats.cpu().numpy().astype(np.int64)
        alg_bytes.append(float((st[:, 0] * 4 * D + st[:, 2] * 4 + st[:, 1] * 8).sum()))
        lab = d_labels.cpu().numpy().astype(np.uint32)
        ref_labels.append(np.sort(lab, axis=1))
        ref_sums.append(checksum(lab))
    kernel_name = ix.last_kernel()
    alg_bytes_launch = float(np.mean(alg_bytes))

    # ---- the timed region(s) ------------------------------------------------------------------------------------------
    streams = [torch.cuda.Stream(device=dev) for _ in range(S)]
    events = [torch.cuda.Event() for _ in range(S)]

    def timed(strong_mode, steps, warmup):
        """One timed region; returns (elapsed seconds, batches).  Every batch is consumed: before a stream's output buffer is
        reused the host waits for that stream's previous batch and checks the checksum of its labels."""
        lo, hi = sharded.shard_range(NQ, rank, world) if strong_mode else (0, NQ)
        rows = hi - lo
        last_on = [-1] * S
        if world == 1:
            # product path: page-locked host buffers in, page-locked host buffers out, hs_search_batch_async on the stream
            q_pin = [hs.PinnedArray((NQ, D), np.float32) for _ in range(NB)]
            for b in range(NB):
                q_pin[b].a[:] = query_sets[b]
            out_pin = [hs.PinnedArray((NQ, K), np.uint32) for _ in range(S)]
            out_np = [o.a for o in out_pin]

            def issue(j, s):
                ix.search_ids_async(q_pin[j % NB].a, K, out_np[s], streams[s].cuda_stream)

            def mine(s):
                return out_np[s], last_on[s], slice(0, NQ)
        else:
            # one rank per GPU: H2D, hs_search_batch_dev, RCCL all-gather of the labels, D2H of the gathered [tot x K]
            q_pin = [torch.from_numpy(query_sets[b][lo:hi].copy()).pin_memory() for b in range(NB)]
            q_dev = [torch.empty((rows, D), dtype=torch.float32, device=dev) for _ in range(S)]
            # small shards (up to 2 MiB of queries, as hs_search_batch_async does it): no staging copy -- the kernels read each
            # query once from a device-mapped page-locked buffer (hs_host_alloc), see profiles/r03_small_batch_queues.log
            q_map = None
            if 0 < rows * D * 4 <= (2 << 20) and os.environ.get("HS_ZERO_COPY", "1") != "0":
                q_hold = [hs.PinnedArray((rows, D), np.float32) for _ in range(NB)]
                for b in range(NB):
                    q_hold[b].a[:] = query_sets[b][lo:hi]
                q_map = [h.device_view() for h in q_hold]
                if any(v is None for v in q_map):
                    q_map = None
            lab_dev = [torch.empty((rows, K), dtype=torch.int32, device=dev) for _ in range(S)]
            cnt_dev = [torch.empty((max(rows, 1),), dtype=torch.int32, device=dev) for _ in range(S)]
            tot = NQ if strong_mode else world * NQ
            out_pin = [torch.empty((tot, K), dtype=torch.int32).pin_memory() for _ in range(S)]
            out_np = [o.numpy().view(np.uint32) for o in out_pin]

            def issue(j, s):
                with torch.cuda.stream(streams[s]):
                    if q_map is None:
                        q_dev[s].copy_(q_pin[j % NB], non_blocking=True)
                    if rows:
                        ix.search_ids_dev(q_dev[s] if q_map is None else q_map[j % NB], K, lab_dev[s], None, cnt_dev[s], None, streams[s].cuda_stream)
                    full = sharded.all_gather_rows(lab_dev[s], tot, world, rank)  # RCCL over xGMI: every rank holds all top-k
                    out_pin[s].copy_(full, non_blocking=True)

            def mine(s):   # strong: the whole gathered batch; weak: this rank's block of the gathered [world x NQ] rows
                return out_np[s], last_on[s], (slice(0, NQ) if strong_mode else slice(rank * NQ, (rank + 1) * NQ))

        def consume(s, full=False):
            if last_on[s] < 0:
                return
            events[s].synchronize()
            got, b, sl = mine(s)
            if full:
                assert np.array_equal(np.sort(got[sl], axis=1), ref_labels[b]), "timed path returned different labels"
            else:
                assert checksum(got[sl]) == ref_sums[b], "timed path returned different labels"

        def batch(j):
            s = j % S
            consume(s)
            issue(j, s)
            events[s].record(streams[s])
            last_on[s] = j % NB

        def finish(ended=None):
            for s_, st_ in enumerate(streams):
                consume(s_, full=True)
                if ended is not None and last_on[s_] >= 0:
                    ended.append((s_, last_on[s_]))
                last_on[s_] = -1
                ix.check(st_.cuda_stream)  # synchronises the stream; the counters are sticky: any batch's capacity failure shows here

        torch.cuda.synchronize()
        for j in range(warmup * BPS):
            batch(j)
        finish()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()
        ended = []
        t0 = time.perf_counter()
        for j in range(steps * BPS):
            batch(j)
        finish(ended)
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        el = time.perf_counter() - t0
        if world > 1:
            t = torch.tensor([el], device=dev, dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            el = float(t.item())
        finals = {}
        for s_, b in ended:   # each stream's last batch of the last step: the labels the timed path handed back
            got, _, sl = mine(s_)
            finals[b] = got[sl].copy()
        return el, steps * BPS, rows, finals

    elapsed, n_batches, rows, final_labels = timed(strong, args.steps, args.warmup)
    log(f"timed region done ({time.perf_counter() - T0:.1f}s since start)")
    total_queries = (NQ if strong else world * NQ) * n_batches
    qps = total_queries / elapsed
    dumped = None
    if rank == 0 and args.dump_outputs:
        dumped = dump_outputs(args.dump_outputs, {f"labels_qset{b}": final_labels[b] for b in sorted(final_labels)})
    weak_side = None
    if strong and full_run:   # the weak figure beside it: every rank searches whole 10k batches (a quarter of the steps)
        w_el, w_nb, _, _ = timed(False, max(args.steps // 4, 1), max(args.warmup // 4, 1))
        weak_side = round(world * NQ * w_nb / w_el, 1)

    # ---- side figures (never `value`, --full only): one launch alone on the GPU, device-resident pipelined rate ------
    kern_ms = dev_resident_qps = sync_host_qps = None
    if full_run:
        def finish_all():
            for st_ in streams:
                ix.check(st_.cuda_stream)

        ke0, ke1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        kern_ms = []
        for i in range(max(min(args.steps, 40), 10)):
            qq = q_sets_t[i % NB]
            ke0.record()
            ix.search_ids_dev(qq, K, d_labels, None, d_counts, None, stream)
            ke1.record()
            torch.cuda.synchronize()
            kern_ms.append(ke0.elapsed_time(ke1))
        ix.check(stream)
        kern_ms = float(np.mean(kern_ms))
        outs = [(torch.empty((NQ, K), dtype=torch.int32, device=dev), torch.empty((NQ,), dtype=torch.int32, device=dev)) for _ in range(S)]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for j in range(16 * S):
            ix.search_ids_dev(q_sets_t[j % NB], K, outs[j % S][0], None, outs[j % S][1], None, streams[j % S].cuda_stream)
        finish_all()
        dev_resident_qps = 16 * S * NQ / (time.perf_counter() - t0)
        if rank == 0 and world == 1:   # the synchronous host-pointer entry on pageable memory
            ix.search_ids(query_sets[0], K)
            t0 = time.perf_counter()
            for i in range(5):
                ix.search_ids(query_sets[i % NB], K)
            sync_host_qps = round(5 * NQ / (time.perf_counter() - t0), 1)

    # ---- CPU baseline (--full): the oracle (port) on this box's host cores, rank 0, N=1 only --------------------------
    cpu = None
    if rank == 0 and world == 1 and full_run and not args.no_cpu_baseline:
        from hsutil import Oracle
        threads_all = min(len(os.sched_getaffinity(0)) or 1, 64)
        model, phys = "unknown", set()
        try:
            core = pkg = None
            for line in open("/proc/cpuinfo"):
                if line.startswith("model name") and model == "unknown":
                    model = line.split(":", 1)[1].strip()
                elif line.startswith("physical id"):
                    pkg = line.split(":", 1)[1].strip()
                elif line.startswith("core id"):
                    core = line.split(":", 1)[1].strip()
                elif not line.strip():
                    if core is not None:
                        phys.add((pkg, core))
                    core = pkg = None
        except OSError:
            pass

        def cpu_run(variant, budget_s):
            ox = Oracle(variant).load(spath, "slim", 0, D)
            ox.set_ef(chosen)
            ns = min(NQ, 2000)
            t0 = time.perf_counter()
            ox.search_ids(query_sets[0][:ns], K, threads=1, raw=False)
            t1 = time.perf_counter() - t0
            reps, tN, same = 0, 0.0, True
            while tN < budget_s and reps < 4 * NB:
                t0 = time.perf_counter()
                rN = ox.search_ids(query_sets[reps % NB], K, threads=threads_all, raw=False)
                tN += time.perf_counter() - t0
                same = same and bool(np.array_equal(np.sort(rN["labels"], axis=1), ref_labels[reps % NB]))
                reps += 1
            return reps * NQ / tN, ns / t1, reps, same

        q_par, q_ser, reps, same = cpu_run("", 10.0)
        of_par, of_ser, of_reps, of_same = cpu_run("_ofast", 6.0)
        cpu = dict(value=round(q_par, 1), unit="queries/s", cores=threads_all, kind="port",
                   sample=f"{reps} batches of {NQ} queries (the bench's query sets), OpenMP dynamic over {threads_all} threads, ef={chosen}; "
                          f"serial (as shipped, 1 core) on the first 2000 queries: {q_ser:.0f} queries/s",
                   serial_qps=round(q_ser, 1), gpu_label_sets_identical=same,
                   cpu_model=model, physical_cores_visible=len(phys) or None, hardware_threads_used=threads_all,
                   compiler="g++ (oracle/Makefile, built in the build container)", flags="-O3 -march=native -ffp-contract=off -fno-fast-math -fopenmp (the pinned parity flags)",
                   ofast={"flags": "-Ofast -flto -march=native -fopenmp (/root/reference/CMakeLists.txt:14)", "value": round(of_par, 1), "serial_qps": round(of_ser, 1),
                          "batches": of_reps, "label_sets_identical_to_gpu": of_same})

    def rnd(x, nd):   # side figures a plain run does not measure stay null
        return None if x is None else round(x, nd)

    if rank == 0:
        # HBM traffic (PMC) cannot be collected from inside this process; the committed profile of this same workload is quoted
        traffic, tsrc = None, None
        for name in ("r03_traffic.json", "r02_traffic.json", "r02_traffic_ef70.json"):   # (the operating point is 68 or 70 depending on the graph the box built)
            tpath = os.path.join(ROOT, "profiles", name)
            if os.path.exists(tpath) and N == 1_000_000 and NQ == 10_000 and D == 128:
                tj = json.load(open(tpath))
                if chosen == tj.get("ef") and tj.get("kernel", "hs::lean_kernel") == kernel_name:
                    traffic, tsrc = tj["hbm_bytes_per_launch"], "profiles/" + name
                    break
        kname = kernel_name   # the kernel the library chose for this shape (hs_last_kernel)
        step_ms = elapsed / args.steps * 1e3
        batch_ms = elapsed / n_batches * 1e3
        achieved_single = alg_bytes_launch / (kern_ms * 1e-3) / 1e9 if full_run else None   # one launch alone on the GPU
        eff = alg_bytes_launch * (1 if strong else world) / (batch_ms * 1e-3) / 1e9
        out = {
            "metric": "QPS @ recall@10>=0.95 (SIFT-1M d=128, k=10)", "value": round(qps, 1), "unit": "queries/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(step_ms, 4),
            "higher_is_better": True, "scaling": "strong" if strong else "weak", "vs_baseline": None, "dtype": "f32", "data": DATA_DESC,
            "config": {"workload": f"SIFT-1M-like d={D} L2, N={N}, batch={NQ} queries" + ("" if strong else "/GPU") +
                                   f", HNSW-Slim M=16 efC=200 (Slim defaults), k={K}, ef_search={chosen}",
                       "step": f"1 step = {BPS} batches; each batch = H2D of {rows if strong else NQ} queries (one of {NB} distinct page-locked sets, rotated) + search + "
                               + ("RCCL all-gather of the labels + " if world > 1 else "") + "D2H of the labels; every batch's labels are checked (checksum) before its buffer is reused",
                       "batches_timed": n_batches, "ms_per_batch": round(batch_ms, 4), "timed_seconds": round(elapsed, 3),
                       "pipelining": f"batches issued round-robin on {S} HIP streams (up to {S} in flight)",
                       "hip_hw_queues": os.environ.get("GPU_MAX_HW_QUEUES", "runtime default (4)"),
                       "entry": "hs_search_batch_async (host pointers)" if world == 1 else "hs_search_batch_dev + torch.distributed all_gather_into_tensor" + (" (queries read in place from mapped page-locked memory)" if (strong and 0 < rows * D * 4 <= (2 << 20)) else ""),
                       "ef_search": chosen, "recall_at_10": round(recall, 4), "recall_per_query_set": [round(r, 4) for r in recalls],
                       "sweep": sweep, "index": info, "build_s": round(t_build, 1), "convert_s": round(t_conv, 1), "build_threads": threads,
                       "device_resident_pipelined_qps": rnd(dev_resident_qps, 1), "single_launch_qps": rnd(kern_ms and NQ / kern_ms * 1e3, 1),
                       "sync_host_pointer_api_qps_pageable": sync_host_qps,
                       "weak_scaling_qps_side_figure": weak_side},
            # achieved/frac: algorithmic bytes of one 10k-query launch / the HIP-event duration of that launch alone on the GPU
            # (what a rocprofv3 kernel-trace of the search kernel's dispatches adds up to, profiles/r03_kernel_stats_1stream.csv);
            # timed_region_*: the same bytes / the effective per-batch time of the timed region (S batches in flight, PCIe included).
            "roofline": {"bound": "hbm", "achieved": rnd(achieved_single, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": rnd(achieved_single and achieved_single / HBM_PEAK_GBS, 4), "traffic": traffic, "traffic_source": tsrc,
                         "kernel": kname, "launch_ms": rnd(kern_ms, 4),
                         "launch": None if not full_run else f"one 10k-query pass = {kname[4:]} (upper-level descent) + order_kernel (start order) + {kname[4:]} "
                                   f"(level-0 search) + the (normally empty) re-run scan; launch_ms spans them, a rocprofv3 kernel trace shows two "
                                   f"{kname[4:]} dispatches per pass whose durations add up to it",
                         "timed_region_achieved": round(eff, 1), "timed_region_frac": round(eff / HBM_PEAK_GBS, 4),
                         "launches_in_flight": S, "algorithmic_bytes_per_launch": alg_bytes_launch},
            "cpu_baseline": cpu, "full": full_run, "outputs_dumped": dumped,
        }
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.destroy_process_group()
    if tmp is not None:
        tmp.cleanup()


if __name__ == "__main__":
    main()
