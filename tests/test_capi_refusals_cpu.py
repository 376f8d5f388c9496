"""What the C ABI answers to a bad call, pinned: (status, hs_last_error()) of a fixed list of calls against
tests/golden/capi_refusals.json.  Every call is refused before a device is asked for anything, or names a device that no machine has
(1 << 20), so the table is the same with and without a GPU.  Where an entry checks several things, a call with two faults at once
pins the order in which it reports them.

Run as a script, `python tests/test_capi_refusals_cpu.py --record` writes the table from the library in use (HS_LIB selects another
build of it); the committed table was recorded once from the commit before the one that introduced csrc/capi_guard.hpp."""
import ctypes
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hostile_graphs as hg  # noqa: E402
from hsutil import GOLDEN, ROOT, load_product, mixture, vanilla_bytes  # noqa: E402

TABLE = os.path.join(GOLDEN, "capi_refusals.json")
NODEV = 1 << 20   # a device index that no machine has
HUGE = 1 << 40


def _ptr(a):
    return a.ctypes.data


def make_cases(hs, tmp):
    """[(name, call)]: call() returns the status of one refused C-ABI call.  Paths under `tmp` never reach the table."""
    L = hs.lib()
    BO, BS = hs.HsBatchBuildOpts, hs.HsBatchBuildStats
    out = ctypes.c_void_p()
    po = ctypes.byref(out)
    u64 = ctypes.c_uint64()
    pu64 = ctypes.byref(u64)
    szv = ctypes.c_size_t()
    psz = ctypes.byref(szv)
    f = np.zeros(64 * 16, np.float32)
    w = np.zeros(4096, np.uint32)
    l64 = np.zeros(64, np.uint64)
    by = np.zeros(4096, np.uint8)
    F, W, L64, BY = _ptr(f), _ptr(w), _ptr(l64), _ptr(by)
    missing = os.path.join(tmp, "no_such_dir", "missing.bin").encode()
    o = os.path.join(tmp, "out.bin").encode()

    # a tiny vanilla file built on the host (labels 0..7), the same with room, one with a delete mark, one of dim 64
    rows8 = mixture(8, 4, 3)
    tiny = os.path.join(tmp, "tiny.hnsw")
    hs.build_hnsw(rows8, tiny, M=4, ef_construction=20, threads=1)
    tiny = tiny.encode()
    marked = os.path.join(tmp, "marked.hnsw")
    with open(marked, "wb") as fh:
        fh.write(vanilla_bytes(rows8, [[(i + 1) % 8] for i in range(8)], 4, marks=[1] + [0] * 7))
    marked = marked.encode()
    rows64 = mixture(8, 64, 4)
    tiny64 = os.path.join(tmp, "tiny64.hnsw")
    hs.build_hnsw(rows64, tiny64, M=4, ef_construction=20, threads=1)
    tiny64 = tiny64.encode()
    # one of the refused files of tests/hostile_graphs.py
    good_raw = open(os.path.join(GOLDEN, "handmade_levels.hnsw.bin"), "rb").read()
    _, bad_raw, _ = hg.mutations("hnsw", good_raw, hg.DIM)[0]
    hostile = os.path.join(tmp, "hostile.hnsw")
    with open(hostile, "wb") as fh:
        fh.write(bad_raw)
    hostile = hostile.encode()
    good = os.path.join(GOLDEN, "handmade_levels.hnsw.bin").encode()

    new_rows = mixture(2, 4, 9)
    NR = _ptr(new_rows)

    def labels(*v):
        a = np.array(v, np.uint64)
        keep.append(a)
        return _ptr(a)

    keep = [f, w, l64, by, rows8, rows64, new_rows]

    def opts(device=-1, threads=1, grow_div=0, batch_max=0, scratch_ids=0):
        return ctypes.byref(BO(device, threads, grow_div, batch_max, scratch_ids))

    def params(centroids=F, num_cluster=1):
        p = hs.HsSlimqParams(0, 0.02, 0.02, 32, 8, 16, 8, centroids, num_cluster, None, 1)
        keep.append(p)
        return ctypes.byref(p)

    c = []

    def add(name, fn):
        assert name not in [n for n, _ in c], name
        c.append((name, fn))

    # ---- capi_index ------------------------------------------------------------------------------------------------------------
    add("index_load:null", lambda: L.hs_index_load(None, 0, 0, 4, 0, 0, po))
    add("index_load:bad_metric+dim0", lambda: L.hs_index_load(missing, 0, 7, 0, 0, 0, po))
    add("index_load:dim0+missing", lambda: L.hs_index_load(missing, 0, 0, 0, 0, 0, po))
    add("index_load:bad_kind+missing", lambda: L.hs_index_load(missing, 9, 0, 4, 0, 0, po))
    add("index_load:missing", lambda: L.hs_index_load(missing, 0, 0, 4, 0, 0, po))
    add("index_load:missing_slim", lambda: L.hs_index_load(missing, 1, 0, 4, 0, 0, po))
    add("index_load:missing_slimq", lambda: L.hs_index_load(missing, 2, 0, 64, 0, 0, po))
    add("index_load:hostile+nodev", lambda: L.hs_index_load(hostile, 0, 0, hg.DIM, 0, NODEV, po))
    add("index_load:nodev", lambda: L.hs_index_load(good, 0, 0, hg.DIM, 0, NODEV, po))
    add("index_load:nodev_room", lambda: L.hs_index_load(tiny, 0, 0, 4, 64, NODEV, po))
    add("index_load_mem:null", lambda: L.hs_index_load_mem(None, 0, 0, 0, 4, 0, 0, po))
    add("index_load_mem:hostile", lambda: L.hs_index_load_mem(bad_raw, len(bad_raw), 0, 0, hg.DIM, 0, NODEV, po))
    add("index_load_mem:truncated", lambda: L.hs_index_load_mem(good_raw, 40, 0, 0, hg.DIM, 0, NODEV, po))
    add("index_load_mem:nodev", lambda: L.hs_index_load_mem(good_raw, len(good_raw), 0, 0, hg.DIM, 0, NODEV, po))
    add("index_load_narrow:null", lambda: L.hs_index_load_narrow(None, 0, 0, 16, 0, 0, 2, po))
    add("index_load_narrow:bad_format+slimq", lambda: L.hs_index_load_narrow(missing, 2, 0, 20, 0, 0, 0, po))
    add("index_load_narrow:slimq+dim20", lambda: L.hs_index_load_narrow(missing, 2, 0, 20, 0, 0, 2, po))
    add("index_load_narrow:dim20+bad_metric", lambda: L.hs_index_load_narrow(missing, 0, 7, 20, 0, 0, 2, po))
    add("index_load_narrow:bad_metric+missing", lambda: L.hs_index_load_narrow(missing, 0, 7, 16, 0, 0, 2, po))
    add("index_load_narrow:missing", lambda: L.hs_index_load_narrow(missing, 0, 0, 16, 0, 0, 1, po))
    add("index_load_narrow:nodev", lambda: L.hs_index_load_narrow(good, 0, 0, 16, 0, NODEV, 1, po))
    add("index_patch:null", lambda: L.hs_index_patch(None, None, 0, 0))
    lv = np.zeros(2, np.int32)
    lp = np.array([0, 1, 2], np.uint64)
    li = np.array([1, 0], np.uint32)
    keep.extend([lv, lp, li])

    def arrays(kind=0, metric=0, n=2, dim=4, ep=0, maxlevel=0, device=NODEV, outp=po, levels=lv, ids=li):
        return L.hs_index_from_host_arrays(kind, metric, n, dim, F, None, None, _ptr(levels), _ptr(lp), _ptr(ids), ep, maxlevel, 0, device, outp)

    add("from_host_arrays:null_out+bad_kind", lambda: arrays(kind=9, outp=None))
    add("from_host_arrays:bad_kind+bad_metric", lambda: arrays(kind=9, metric=7))
    add("from_host_arrays:bad_metric+dim0", lambda: arrays(metric=7, dim=0))
    add("from_host_arrays:dim0+ep", lambda: arrays(dim=0, ep=5))
    add("from_host_arrays:ep+level", lambda: arrays(ep=5, maxlevel=-1))
    add("from_host_arrays:level", lambda: arrays(levels=np.array([0, 3], np.int32)))
    add("from_host_arrays:id", lambda: arrays(ids=np.array([1, 7], np.uint32)))
    add("from_host_arrays:nodev", lambda: arrays())
    add("set_ef:null", lambda: L.hs_set_ef(None, 10))
    add("set_capacity:null", lambda: L.hs_set_capacity(None, 0, 0))
    add("set_exact_order:null", lambda: L.hs_set_exact_order(None, 1))
    add("index_info:null", lambda: L.hs_index_info(None, None))
    add("set_row_format:null", lambda: L.hs_index_set_row_format(None, 9))
    add("set_f32_resident:null", lambda: L.hs_index_set_f32_resident(None, 0))
    add("rows_representable:null+bad_format", lambda: L.hs_rows_representable(F, 2, 16, 9, None))
    add("rows_representable:bad_format", lambda: L.hs_rows_representable(F, 2, 16, 9, pu64))
    add("rows_to_narrow:null+bad_format", lambda: L.hs_rows_to_narrow(F, 2, 16, 0, None, pu64))
    add("rows_to_narrow:bad_format+dim20", lambda: L.hs_rows_to_narrow(F, 2, 20, 0, BY, pu64))
    add("rows_to_narrow:dim20", lambda: L.hs_rows_to_narrow(F, 2, 20, 2, BY, pu64))
    add("labels:null", lambda: L.hs_labels(None, None))

    # ---- capi_build ------------------------------------------------------------------------------------------------------------
    add("build_hnsw:null", lambda: L.hs_build_hnsw(None, 8, 4, 0, 4, 20, b"4", 100, 1, o))
    add("build_hnsw:n0", lambda: L.hs_build_hnsw(F, 0, 4, 0, 4, 20, b"4", 100, 1, o))
    add("build_hnsw_labeled:null", lambda: L.hs_build_hnsw_labeled(F, None, 8, 4, 0, 4, 20, None, 100, 1, o))
    add("build_hnsw:missing_dir", lambda: L.hs_build_hnsw(_ptr(rows8), 8, 4, 0, 4, 20, b"4", 100, 1, missing))

    def batched(base=F, n=8, dim=4, metric=0, M=4, bf=b"4", op=None, path=o):
        return L.hs_build_hnsw_batched(base, None, n, dim, metric, M, 20, bf, 100, opts() if op is None else op, path, None)

    add("build_hnsw_batched:null+bad_metric", lambda: batched(base=None, metric=7))
    add("build_hnsw_batched:bad_metric+dim0", lambda: batched(metric=7, dim=0))
    add("build_hnsw_batched:dim0+M0", lambda: batched(dim=0, M=0))
    add("build_hnsw_batched:M0+null_opts", lambda: L.hs_build_hnsw_batched(F, None, 8, 4, 0, 0, 20, b"4", 100, None, o, None))
    add("build_hnsw_batched:too_many+null_opts", lambda: L.hs_build_hnsw_batched(F, None, HUGE, 4, 0, 4, 20, b"4", 100, None, o, None))
    add("build_hnsw_batched:null_opts", lambda: L.hs_build_hnsw_batched(F, None, 8, 4, 0, 4, 20, b"4", 100, None, o, None))
    add("build_hnsw_batched:device-2+scratch", lambda: batched(op=opts(device=-2, scratch_ids=100)))
    add("build_hnsw_batched:scratch+nodev", lambda: batched(op=opts(device=NODEV, scratch_ids=100)))
    add("build_hnsw_batched:scratch32", lambda: batched(op=opts(scratch_ids=32)))
    add("build_hnsw_batched:grow_div+nodev", lambda: batched(op=opts(device=NODEV, grow_div=1 << 33)))
    add("build_hnsw_batched:batch_max", lambda: batched(op=opts(batch_max=1 << 33)))
    add("build_hnsw_batched:nodev", lambda: batched(op=opts(device=NODEV)))
    add("build_hnsw_batched:missing_dir", lambda: batched(base=_ptr(rows8), path=missing))
    add("build_schedule:null", lambda: L.hs_build_schedule(8, 4, None, 100, 0, 0, 0, None, None, None, psz))
    add("build_schedule:M0", lambda: L.hs_build_schedule(8, 0, b"4", 100, 0, 0, 0, None, None, None, psz))

    def resume(path=tiny, metric=0, dim=4, max_el=16, rows=NR, labs=None, count=1, outp=o):
        return L.hs_hnsw_resume(path, metric, dim, max_el, rows, labels(100) if labs is None else labs, count, 100, 8, 1, outp)

    def resume_b(path=tiny, metric=0, dim=4, max_el=16, rows=NR, labs=None, count=1, op=None, outp=o, null_opts=False):
        return L.hs_hnsw_resume_batched(path, metric, dim, max_el, rows, labels(100) if labs is None else labs, count, 100, 8,
                                        None if null_opts else (opts() if op is None else op), outp, None)

    for tag, fn in (("resume", resume), ("resume_batched", resume_b)):
        add(f"{tag}:null_labels+bad_metric", lambda fn=fn: fn(metric=7, labs=0))
        add(f"{tag}:null_path", lambda fn=fn: fn(path=None))
        add(f"{tag}:bad_metric+dim0", lambda fn=fn: fn(metric=7, dim=0))
        add(f"{tag}:dim0+missing", lambda fn=fn: fn(dim=0, path=missing))
        add(f"{tag}:missing", lambda fn=fn: fn(path=missing))
        add(f"{tag}:hostile", lambda fn=fn: fn(path=hostile, dim=hg.DIM))
        add(f"{tag}:capacity+label_exists", lambda fn=fn: fn(max_el=8, labs=labels(3)))
        add(f"{tag}:capacity", lambda fn=fn: fn(max_el=8))
        add(f"{tag}:label_exists", lambda fn=fn: fn(labs=labels(3)))
        add(f"{tag}:label_exists_row1", lambda fn=fn: fn(labs=labels(100, 5), count=2))
        add(f"{tag}:label_twice", lambda fn=fn: fn(labs=labels(100, 100), count=2))
        add(f"{tag}:label_twice_then_exists", lambda fn=fn: fn(labs=labels(100, 100, 3), count=3, rows=_ptr(mixture(3, 4, 1))))
        add(f"{tag}:missing_out_dir", lambda fn=fn: fn(outp=missing))
    add("resume_batched:bad_metric+null_opts", lambda: resume_b(metric=7, null_opts=True))
    add("resume_batched:dim0+null_opts", lambda: resume_b(dim=0, null_opts=True))
    add("resume_batched:null_opts+missing", lambda: resume_b(path=missing, null_opts=True))
    add("resume_batched:device-2+missing", lambda: resume_b(path=missing, op=opts(device=-2)))
    add("resume_batched:scratch+missing", lambda: resume_b(path=missing, op=opts(scratch_ids=65)))
    add("resume_batched:label_exists+marks", lambda: resume_b(path=marked, labs=labels(3)))
    add("resume_batched:marks", lambda: resume_b(path=marked))

    def slim(fn, path=missing, outp=o, metric=0, dim=4):
        return fn(path, metric, dim, 0, 0.02, 0.02, 32, 8, 16, 8, 1, outp)

    def slim_gpu(fn, path=missing, outp=o, metric=0, dim=4, device=NODEV):
        return fn(path, metric, dim, 0, 0.02, 0.02, 32, 8, 16, 8, device, 1, outp, None, None)

    for tag, fn in (("convert_slim", L.hs_convert_slim), ("convert_slimq_graph", L.hs_convert_slimq_graph)):
        add(f"{tag}:null", lambda fn=fn: slim(fn, path=None))
        add(f"{tag}:null_out", lambda fn=fn: slim(fn, outp=None))
        add(f"{tag}:missing", lambda fn=fn: slim(fn))
        add(f"{tag}:hostile", lambda fn=fn: slim(fn, path=hostile, dim=hg.DIM))
        add(f"{tag}:missing_out_dir", lambda fn=fn: slim(fn, path=tiny, outp=missing))
    add("convert_slim_gpu:null+nodev", lambda: slim_gpu(L.hs_convert_slim_gpu, path=None))
    add("convert_slim_gpu:nodev+missing", lambda: slim_gpu(L.hs_convert_slim_gpu))
    add("convert_slimq_graph_gpu:null+bad_metric", lambda: slim_gpu(L.hs_convert_slimq_graph_gpu, path=None, metric=7))
    add("convert_slimq_graph_gpu:bad_metric+device-1", lambda: slim_gpu(L.hs_convert_slimq_graph_gpu, metric=7, device=-1))
    add("convert_slimq_graph_gpu:device-1+missing", lambda: slim_gpu(L.hs_convert_slimq_graph_gpu, device=-1))
    add("convert_slimq_graph_gpu:nodev+missing", lambda: slim_gpu(L.hs_convert_slimq_graph_gpu))

    add("build_rabitq_hnsw:null", lambda: L.hs_build_rabitq_hnsw(None, 8, 4, 0, 4, 20, 100, 1, o))
    add("build_rabitq_hnsw:dim0+bad_metric", lambda: L.hs_build_rabitq_hnsw(F, 8, 0, 7, 4, 20, 100, 1, o))
    add("build_rabitq_hnsw:bad_metric+M1", lambda: L.hs_build_rabitq_hnsw(F, 8, 4, 7, 1, 20, 100, 1, o))
    add("build_rabitq_hnsw:M1", lambda: L.hs_build_rabitq_hnsw(F, 8, 4, 0, 1, 20, 100, 1, o))

    def rq_b(base=F, n=8, dim=4, metric=0, M=4, op=None, path=o, null_opts=False):
        return L.hs_build_rabitq_hnsw_batched(base, n, dim, metric, M, 20, 100, None if null_opts else (opts() if op is None else op), path, None)

    def rq_mem(base=F, n=8, dim=4, metric=0, M=4, op=None, outp=po, null_opts=False):
        return L.hs_build_rabitq_hnsw_batched_mem(base, n, dim, metric, M, 20, 100, None if null_opts else (opts() if op is None else op), outp, None)

    add("build_rabitq_hnsw_batched:null_path+null_base", lambda: rq_b(base=None, path=None))
    add("build_rabitq_hnsw_batched_mem:null_out+bad_metric", lambda: rq_mem(outp=None, metric=7))
    for tag, fn in (("build_rabitq_hnsw_batched", rq_b), ("build_rabitq_hnsw_batched_mem", rq_mem)):
        add(f"{tag}:null_base+bad_metric", lambda fn=fn: fn(base=None, metric=7))
        add(f"{tag}:bad_metric+M1", lambda fn=fn: fn(metric=7, M=1))
        add(f"{tag}:M1+too_many", lambda fn=fn: fn(M=1, n=HUGE))
        add(f"{tag}:too_many+null_opts", lambda fn=fn: fn(n=HUGE, null_opts=True))
        add(f"{tag}:null_opts", lambda fn=fn: fn(null_opts=True))
        add(f"{tag}:device-2", lambda fn=fn: fn(op=opts(device=-2)))
        add(f"{tag}:scratch+nodev", lambda fn=fn: fn(op=opts(device=NODEV, scratch_ids=3)))
        add(f"{tag}:nodev", lambda fn=fn: fn(op=opts(device=NODEV)))
    add("debug_rq_raw_dist:null+bad_metric", lambda: L.hs_debug_rq_raw_dist(None, F, 1, 4, 7, -2, F))
    add("debug_rq_raw_dist:bad_metric+device-2", lambda: L.hs_debug_rq_raw_dist(F, F, 1, 4, 7, -2, F))
    add("debug_rq_raw_dist:device-2", lambda: L.hs_debug_rq_raw_dist(F, F, 1, 4, 0, -2, F))
    add("debug_rq_raw_dist:dim9000+nodev", lambda: L.hs_debug_rq_raw_dist(F, F, 1, 9000, 0, NODEV, F))
    add("debug_rq_raw_dist:nodev", lambda: L.hs_debug_rq_raw_dist(F, F, 1, 4, 0, NODEV, F))

    def bf_dev(base=F, n=8, dim=4, metric=0, nq=1, k=1):
        return L.hs_brute_force_dev(base, None, n, dim, metric, F, nq, k, L64, F, None, None)

    add("brute_force_dev:null+bad_metric", lambda: bf_dev(base=None, metric=7))
    add("brute_force_dev:bad_metric+dim0", lambda: bf_dev(metric=7, dim=0))
    add("brute_force_dev:dim0+k0", lambda: bf_dev(dim=0, k=0))
    add("brute_force_dev:dim5000+k0", lambda: bf_dev(dim=5000, k=0))
    add("brute_force_dev:k65+too_many", lambda: bf_dev(k=65, n=HUGE))
    add("brute_force_dev:too_many", lambda: bf_dev(n=HUGE))
    add("brute_force:null+nodev", lambda: L.hs_brute_force(None, 8, 4, 0, None, F, 1, 1, NODEV, L64, F, None))
    add("brute_force:nodev+bad_metric", lambda: L.hs_brute_force(F, 8, 4, 7, None, F, 1, 1, NODEV, L64, F, None))
    add("exact_search:null", lambda: L.hs_index_exact_search(None, None, F, 1, 1, None, L64, F, None))
    add("exact_search_dev:null", lambda: L.hs_index_exact_search_dev(None, None, F, 1, 1, None, L64, F, None, None))

    def slimq(path=missing, metric=0, dim=64, cent=F, ncl=1, outp=o):
        return L.hs_convert_slimq(path, metric, dim, cent, ncl, None, 1, 1, outp)

    add("convert_slimq:null_centroids+dim32", lambda: slimq(cent=None, dim=32))
    add("convert_slimq:ncl0", lambda: slimq(ncl=0))
    add("convert_slimq:dim32+missing", lambda: slimq(dim=32))
    add("convert_slimq:dim4096", lambda: slimq(dim=4096))
    add("convert_slimq:missing", lambda: slimq())

    # ---- capi_update -----------------------------------------------------------------------------------------------------------
    add("seed_levels:null", lambda: L.hs_index_seed_levels(None, 1, 1))
    add("add_points:null", lambda: L.hs_index_add_points(None, None, None, 0, 1))
    add("add_points_batched:null", lambda: L.hs_index_add_points_batched(None, None, None, 0, None, None))
    add("debug_batched_add_changed:null", lambda: L.hs_debug_batched_add_changed(None, None, 0, None, None))
    add("mark_deleted:null", lambda: L.hs_index_mark_deleted(None, None, 0, 1))
    add("index_save:null", lambda: L.hs_index_save(None, o))
    add("get_row:null", lambda: L.hs_index_get_row(None, 0, F))
    add("set_replace_deleted:null", lambda: L.hs_index_set_replace_deleted(None, 1))
    add("upsert_points:null", lambda: L.hs_index_upsert_points(None, None, None, None, 0))
    add("resize:null", lambda: L.hs_index_resize(None, 10))

    def replay(path=tiny, metric=0, dim=4, max_el=16, ops=(), rows=NR, outp=o, allow=0):
        a = np.array(ops, np.uint64).reshape(-1)
        keep.append(a)
        return L.hs_hnsw_replay(path, metric, dim, max_el, allow, _ptr(a) if len(a) else None, len(a) // 4, rows, outp)

    add("replay:null_ops+bad_metric", lambda: L.hs_hnsw_replay(tiny, 7, 4, 16, 0, None, 1, NR, o))
    add("replay:bad_metric+dim0", lambda: replay(metric=7, dim=0))
    add("replay:dim0+missing", lambda: replay(dim=0, path=missing))
    add("replay:missing", lambda: replay(path=missing))
    add("replay:bad_kind", lambda: replay(ops=[(99, 0, 0, 0)]))
    ADD, MARK, UNMARK, RESIZE = hs.HS_OP_ADD, hs.HS_OP_MARK, hs.HS_OP_UNMARK, hs.HS_OP_RESIZE
    add("replay:add_without_rows", lambda: replay(ops=[(ADD, 100, 0, 0)], rows=None))
    add("replay:label_not_found", lambda: replay(ops=[(MARK, 999, 0, 0)]))
    add("replay:label_not_found_unmark", lambda: replay(ops=[(UNMARK, 999, 0, 0)]))
    add("replay:capacity", lambda: replay(max_el=8, ops=[(ADD, 100, 0, 0)]))
    add("replay:replace_disabled", lambda: replay(ops=[(ADD, 100, 1, 0)]))
    add("replay:mark_twice", lambda: replay(ops=[(MARK, 3, 0, 0), (MARK, 3, 0, 0)]))
    add("replay:unmark_unmarked", lambda: replay(ops=[(UNMARK, 3, 0, 0)]))
    add("replay:resize_below_count", lambda: replay(ops=[(RESIZE, 2, 0, 0)]))

    # ---- capi_convert_slimq -------------------------------------------------------------------------------------------------------
    def slimq_gpu(path=missing, metric=0, dim=64, cent=F, ncl=1, device=NODEV, outp=o):
        return L.hs_convert_slimq_gpu(path, metric, dim, cent, ncl, None, 1, device, 1, outp, None, None)

    add("convert_slimq_gpu:null_path+null_centroids", lambda: slimq_gpu(path=None, cent=None))
    add("convert_slimq_gpu:null_centroids+dim32", lambda: slimq_gpu(cent=None, dim=32))
    add("convert_slimq_gpu:dim32+too_many_clusters", lambda: slimq_gpu(dim=32, ncl=HUGE))
    add("convert_slimq_gpu:too_many_clusters+bad_metric", lambda: slimq_gpu(ncl=HUGE, metric=7))
    add("convert_slimq_gpu:bad_metric+device-1", lambda: slimq_gpu(metric=7, device=-1))
    add("convert_slimq_gpu:device-1", lambda: slimq_gpu(device=-1))
    add("convert_slimq_gpu:nodev+missing", lambda: slimq_gpu())

    def to_slimq(path=missing, metric=0, dim=64, cent=F, ncl=1, device=-1, outp=o):
        return L.hs_convert_hnsw_to_slimq(path, metric, dim, 0, 0.02, 0.02, 32, 8, 16, 8, cent, ncl, None, 1, device, 1, outp, None)

    add("convert_hnsw_to_slimq:null_path+dim32", lambda: to_slimq(path=None, dim=32))
    add("convert_hnsw_to_slimq:dim32+device-2", lambda: to_slimq(dim=32, device=-2))
    add("convert_hnsw_to_slimq:bad_metric+device-2", lambda: to_slimq(metric=7, device=-2))
    add("convert_hnsw_to_slimq:device-2+missing", lambda: to_slimq(device=-2))
    add("convert_hnsw_to_slimq:nodev+missing", lambda: to_slimq(device=NODEV))
    add("convert_hnsw_to_slimq:missing", lambda: to_slimq())
    add("convert_hnsw_to_slimq:hostile", lambda: to_slimq(path=hostile, dim=64))

    def quant(flips=BY, dim=64, metric=0, n=1, cent=F, ncl=1, cids=None, device=-1):
        return L.hs_debug_rq_quantize_rows(dim, metric, flips, F, n, cent, ncl, cids, device, F, W, L64, F)

    add("debug_rq_quantize_rows:null_flips+dim32", lambda: quant(flips=None, dim=32))
    add("debug_rq_quantize_rows:dim32+device-2", lambda: quant(dim=32, device=-2))
    add("debug_rq_quantize_rows:device-2+too_many", lambda: quant(device=-2, n=HUGE))
    add("debug_rq_quantize_rows:too_many+nodev", lambda: quant(n=HUGE, device=NODEV))
    cid = np.array([5], np.uint32)
    keep.append(cid)
    add("debug_rq_quantize_rows:cluster_id+nodev", lambda: quant(cids=_ptr(cid), device=NODEV))
    add("debug_rq_quantize_rows:nodev", lambda: quant(device=NODEV))

    # ---- capi_diff -------------------------------------------------------------------------------------------------------------
    add("slim_convert_diff:null", lambda: L.hs_slim_convert_diff(None, None, 0.02, 0.02, 32, 8, 16, 8, 1, po, None, None))
    add("slim_diff_info:null", lambda: L.hs_slim_diff_info(None, None, None, None, None))
    add("slim_diff_ids:null", lambda: L.hs_slim_diff_ids(None, None, None))
    add("slim_diff_stream:null", lambda: L.hs_slim_diff_stream(None, None, None, 0, psz))
    add("slim_diff_next:null", lambda: L.hs_slim_diff_next(None, None, 10, 0, None, 0, psz, None, None, None))
    add("slim_index_save:null", lambda: L.hs_slim_index_save(None, o))

    def diff_files(old=None, path=missing, metric=0, dim=4, out_slim=o, stream=None, outp=None):
        return L.hs_slim_convert_diff_files(old, path, metric, dim, 0, 0.02, 0.02, 32, 8, 16, 8, 1, out_slim, stream, outp)

    add("slim_convert_diff_files:null+bad_metric", lambda: diff_files(path=None, metric=7))
    add("slim_convert_diff_files:bad_metric+dim0", lambda: diff_files(metric=7, dim=0))
    add("slim_convert_diff_files:dim0+missing", lambda: diff_files(dim=0))
    add("slim_convert_diff_files:missing", lambda: diff_files())
    add("slim_convert_diff_files:missing_old", lambda: diff_files(old=missing, path=tiny))
    add("slim_convert_diff_files:missing_stream_dir", lambda: diff_files(path=tiny, stream=missing))
    diff = ctypes.c_void_p()

    def diff_handle():
        if not diff.value:
            assert diff_files(path=tiny, outp=ctypes.byref(diff)) == hs.HS_OK, L.hs_last_error()
        return diff

    add("slim_diff_stream:owning_diff_with_index", lambda: L.hs_slim_diff_stream(diff_handle(), ctypes.c_void_p(1), BY, 4096, psz))
    add("slim_diff_stream:buffer_too_small", lambda: L.hs_slim_diff_stream(diff_handle(), None, BY, 0, psz))
    add("slim_diff_next:owning_diff_with_index", lambda: L.hs_slim_diff_next(diff_handle(), ctypes.c_void_p(1), 10, 1, BY, 4096, psz, None, None, None))
    add("slim_diff_next:buffer_too_small", lambda: L.hs_slim_diff_next(diff_handle(), None, 10, 1, BY, 8, psz, None, None, None))

    # ---- capi_filter, capi_queue, capi_search -----------------------------------------------------------------------------------------
    add("filter_pack:null", lambda: L.hs_filter_pack(None, 4, 1, W))
    add("filter_set_create:null_out", lambda: L.hs_filter_set_create(None, 1, None))
    add("filter_set_create:null_index+nf0", lambda: L.hs_filter_set_create(None, 0, po))
    add("filter_set_write:null", lambda: L.hs_filter_set_write(None, 0, 1, BY))
    add("filter_set_write_bits:null", lambda: L.hs_filter_set_write_bits(None, 0, 1, W))
    add("filter_set_write_dev:null", lambda: L.hs_filter_set_write_dev(None, 0, 1, BY, None))
    add("filter_set_read:null", lambda: L.hs_filter_set_read(None, 0, BY))
    add("filter_set_info:null", lambda: L.hs_filter_set_info(None, None, None, None, None))
    add("search_batch_filter_set:null", lambda: L.hs_search_batch_filter_set(None, None, F, 1, 1, W, L64, F, W, None))
    add("search_batch_filter_set_dev:null", lambda: L.hs_search_batch_filter_set_dev(None, None, F, 1, 1, W, L64, F, W, None, None))
    add("queue_create:null_out", lambda: L.hs_queue_create(None, 0, 9, 0, 0, None, None))
    add("queue_create:null_index+k0", lambda: L.hs_queue_create(None, 0, 9, 0, 0, None, po))
    add("queue_submit:null", lambda: L.hs_queue_submit(None, F, 1, None, None, L64, F, W, None, pu64))
    add("queue_submit_dev:null", lambda: L.hs_queue_submit_dev(None, F, 1, None, None, L64, F, W, None, None, pu64))
    add("queue_flush:null", lambda: L.hs_queue_flush(None))
    add("queue_wait:null", lambda: L.hs_queue_wait(None, 1))
    add("queue_join_stream:null", lambda: L.hs_queue_join_stream(None, 1, None))
    add("queue_drain:null", lambda: L.hs_queue_drain(None))
    add("queue_info:null", lambda: L.hs_queue_info(None, None))
    add("search_batch:ids_without_labels32", lambda: L.hs_search_batch(None, F, 1, 1, 0, None, L64, F, W, None))
    add("search_batch:pq_without_outputs", lambda: L.hs_search_batch(None, F, 1, 1, 1, W, None, None, None, None))
    add("search_batch:null_index", lambda: L.hs_search_batch(None, F, 1, 1, 1, None, L64, F, W, None))
    add("search_batch_dev:pq_without_outputs", lambda: L.hs_search_batch_dev(None, F, 1, 1, 1, W, None, None, None, None, None))
    add("search_batch_dev:null_index+nq", lambda: L.hs_search_batch_dev(None, F, HUGE, 1, 1, None, L64, F, W, None, None))
    add("search_batch_async:ids_without_labels32", lambda: L.hs_search_batch_async(None, F, 1, 1, 0, None, L64, F, W, None, None))
    add("search_batch_async:bad_mode+null_index", lambda: L.hs_search_batch_async(None, F, 1, 1, 5, None, None, None, None, None, None))
    add("search_batch_async:null_index+k0", lambda: L.hs_search_batch_async(None, F, 1, 0, 1, None, L64, F, W, None, None))
    add("search_batch_filtered:null", lambda: L.hs_search_batch_filtered(None, F, 1, 1, BY, None, None, None, None))
    add("search_batch_raw:no_raw_outputs", lambda: L.hs_search_batch_raw(None, F, 1, 1, 1, None, None, None, None))
    add("search_batch_raw:null_index", lambda: L.hs_search_batch_raw(None, F, 1, 1, 1, F, W, W, None))
    add("search_check:null", lambda: L.hs_search_check(None, None))
    add("debug_search_plan:null", lambda: L.hs_debug_search_plan(None, None))
    add("debug_plan_input:null", lambda: L.hs_debug_plan_input(None, 1, 1, 0, 0, None))
    fsh = hs.HsFastShape()
    add("debug_fast_shape:null_out+bad_metric", lambda: L.hs_debug_fast_shape(7, 0, 10, 10, 1, None))
    add("debug_fast_shape:bad_metric+dim0", lambda: L.hs_debug_fast_shape(7, 0, 10, 10, 1, ctypes.byref(fsh)))
    add("debug_fast_shape:dim0", lambda: L.hs_debug_fast_shape(0, 0, 10, 10, 1, ctypes.byref(fsh)))
    add("debug_fast_shape:ef513", lambda: L.hs_debug_fast_shape(0, 16, 513, 10, 1, ctypes.byref(fsh)))
    add("debug_heap_ops:null+lds3", lambda: L.hs_debug_heap_ops(None, 0, 1, 3, W, W, W))
    add("debug_heap_ops:lds3", lambda: L.hs_debug_heap_ops(W, 0, 1, 3, W, W, W))

    # ---- capi_slimq, capi_slimq_resident ------------------------------------------------------------------------------------------
    add("slimq_set_dataset:null", lambda: L.hs_slimq_set_dataset(None, F, 1, 64))
    add("slimq_set_tconst:null", lambda: L.hs_slimq_set_tconst(None, 1.0))
    add("slimq_search_batch:null", lambda: L.hs_slimq_search_batch(None, F, 1, 1, L64, F, W, None))
    add("slimq_search_batch_dev:null", lambda: L.hs_slimq_search_batch_dev(None, F, 1, 1, L64, F, W, None, None))
    add("slimq_trace:null", lambda: L.hs_slimq_trace(None, F, 1, 1, W, 16, None))
    add("slimq_prepare_debug:null", lambda: L.hs_slimq_prepare_debug(None, F, 1, F))
    add("rabitq_rotate:null+dim0", lambda: L.hs_rabitq_rotate(0, None, F, 1, F))
    add("rabitq_rotate:dim32", lambda: L.hs_rabitq_rotate(32, BY, F, 1, F))
    add("rabitq_rotate:dim4096", lambda: L.hs_rabitq_rotate(4096, BY, F, 0, F))
    add("rabitq_quantize_data:null", lambda: L.hs_rabitq_quantize_data(64, 0, None, 1, F, L64, F))
    add("rabitq_quantize_data:padded65", lambda: L.hs_rabitq_quantize_data(65, 0, F, 1, F, L64, F))
    add("rabitq_prepare_query:null", lambda: L.hs_rabitq_prepare_query(64, 1.0, None, 1, F, L64))
    add("rabitq_prepare_query:padded65", lambda: L.hs_rabitq_prepare_query(65, 1.0, F, 1, F, L64))
    add("rabitq_estimate:null", lambda: L.hs_rabitq_estimate(64, None, F, 1, F, L64, F, F, 1, F))
    add("graph_load:null+bad_metric", lambda: L.hs_graph_load(None, 7, 4, po))
    add("graph_load:bad_metric+dim0", lambda: L.hs_graph_load(missing, 7, 0, po))
    add("graph_load:dim0+missing", lambda: L.hs_graph_load(missing, 0, 0, po))
    add("graph_load:missing", lambda: L.hs_graph_load(missing, 0, 4, po))
    add("graph_load:hostile", lambda: L.hs_graph_load(hostile, 0, hg.DIM, po))
    graphs = {}

    def graph(dim):
        if dim not in graphs:
            g = ctypes.c_void_p()
            assert L.hs_graph_load(tiny if dim == 4 else tiny64, 0, dim, ctypes.byref(g)) == hs.HS_OK, L.hs_last_error()
            graphs[dim] = g
        return graphs[dim]

    add("graph_save:null", lambda: L.hs_graph_save(None, o))
    add("graph_save:null_path", lambda: L.hs_graph_save(graph(4), None))
    add("graph_save:missing_dir", lambda: L.hs_graph_save(graph(4), missing))
    add("graph_info:null", lambda: L.hs_graph_info(None, None, None, None, None, None, None))

    def gconv(g=None, p=None, cdev=-1, path=o, idev=0, outp=None, dim=64, null_p=False):
        return L.hs_graph_convert_slimq(graph(dim) if g is None else g, None if null_p else (params() if p is None else p), cdev, 1, path, idev, 0, outp, None)

    add("graph_convert_slimq:null_graph", lambda: gconv(g=ctypes.c_void_p()))
    add("graph_convert_slimq:null_params+no_output", lambda: gconv(null_p=True, path=None))
    add("graph_convert_slimq:no_output+null_centroids", lambda: gconv(p=params(centroids=None), path=None))
    add("graph_convert_slimq:null_centroids+dim4", lambda: gconv(p=params(centroids=None), dim=4))
    add("graph_convert_slimq:dim4+device-2", lambda: gconv(dim=4, cdev=-2))
    add("graph_convert_slimq:too_many_clusters", lambda: gconv(p=params(num_cluster=HUGE)))
    add("graph_convert_slimq:device-2+index_device-1", lambda: gconv(cdev=-2, idev=-1, outp=po))
    add("graph_convert_slimq:nodev+index_device-1", lambda: gconv(cdev=NODEV, idev=-1, outp=po))
    add("graph_convert_slimq:index_device-1", lambda: gconv(idev=-1, outp=po))
    add("graph_convert_slimq:index_nodev", lambda: gconv(idev=NODEV, outp=po))
    add("graph_convert_slimq:missing_dir", lambda: gconv(path=missing))

    def from_rows(base=F, dim=64, metric=0, M=4, op=None, p=None, outp=po, null_p=False):
        return L.hs_slimq_index_from_rows(base, 8, dim, metric, M, 20, 100, opts(device=NODEV) if op is None else op, None if null_p else (params() if p is None else p),
                                          1, 0, outp, None)

    add("slimq_index_from_rows:null_out+bad_metric", lambda: from_rows(outp=None, metric=7))
    add("slimq_index_from_rows:null_params+bad_metric", lambda: from_rows(null_p=True, metric=7))
    add("slimq_index_from_rows:bad_metric+M1", lambda: from_rows(metric=7, M=1))
    add("slimq_index_from_rows:nodev+dim32", lambda: from_rows(dim=32))
    add("slimq_index_from_rows:device-1+dim32", lambda: from_rows(dim=32, op=opts(device=-1)))
    add("slimq_index_from_rows:device-2+dim32", lambda: from_rows(dim=32, op=opts(device=-2)))
    add("slimq_index_save:null", lambda: L.hs_slimq_index_save(None, o))
    add("debug_slimq_arrays:null", lambda: L.hs_debug_slimq_arrays(None, 0, None, 0, psz, None, None))
    add("debug_slimq_arrays_host:null", lambda: L.hs_debug_slimq_arrays_host(None, 0, 64, 1, 0, None, 0, psz, None, None))
    add("debug_slimq_arrays_host:which3+missing", lambda: L.hs_debug_slimq_arrays_host(missing, 0, 64, 1, 3, None, 0, psz, None, None))
    add("debug_slimq_arrays_host:missing", lambda: L.hs_debug_slimq_arrays_host(missing, 0, 64, 1, 0, None, 0, psz, None, None))

    # ---- capi_comm -------------------------------------------------------------------------------------------------------------
    add("comm_init:null_out", lambda: L.hs_comm_init(1, None, None))
    add("comm_init:n0", lambda: L.hs_comm_init(0, None, po))
    add("comm_init:n65", lambda: L.hs_comm_init(65, None, po))
    add("comm_check:null", lambda: L.hs_comm_check(None, None, 0))
    add("search_batch_sharded:null", lambda: L.hs_search_batch_sharded(None, None, F, 1, 1, 1, None, L64, F, W))
    add("search_batch_sharded_async:null", lambda: L.hs_search_batch_sharded_async(None, None, F, 1, 1, 1, None, L64, F, W, 0))
    add("comm_results_dev:null", lambda: L.hs_comm_results_dev(None, 0, None, None, None, None))

    def cleanup():
        if diff.value:
            L.hs_slim_diff_free(diff)
        for g in graphs.values():
            L.hs_graph_free(g)

    return c, cleanup, keep


def run_cases(hs):
    """{name: [status, text]} of every case, in the order of the list."""
    L = hs.lib()
    got = {}
    with tempfile.TemporaryDirectory() as tmp:
        cases, cleanup, keep = make_cases(hs, tmp)
        for name, call in cases:
            status = call()
            text = L.hs_last_error().decode()
            assert tmp not in text, (name, text)   # the table holds nothing of this machine
            got[name] = [int(status), text]
        cleanup()
        del keep
    return got


@pytest.fixture(scope="module")
def hs():
    return load_product()


@pytest.fixture(scope="module")
def got(hs):
    return run_cases(hs)


def test_every_refusal_is_the_recorded_one(hs, got):
    want = json.load(open(TABLE))
    assert list(got) == list(want), sorted(set(got) ^ set(want))
    wrong = {n: (got[n], want[n]) for n in want if got[n] != want[n]}
    assert not wrong, wrong
    assert all(s != hs.HS_OK for s, _ in got.values())


def test_file_and_batched_resume_report_labels_alike(hs, got):
    for case in ("label_exists", "label_exists_row1", "label_twice", "label_twice_then_exists", "capacity", "capacity+label_exists"):
        assert got["resume:" + case] == got["resume_batched:" + case], case
    assert got["resume:label_exists"] == [hs.HS_ERR_UNSUPPORTED, "label 3 (row 0) already exists: updatePoint is not supported"]
    assert got["resume:label_twice"] == [hs.HS_ERR_INVALID, "label 100 appears twice in the call (rows 0 and 1)"]


def test_io_and_corrupt_mapping(hs, got):
    assert got["index_load:missing"] == [hs.HS_ERR_IO, "Cannot open file"]
    assert got["index_load:hostile+nodev"][0] == hs.HS_ERR_CORRUPT and "corrupted" in got["index_load:hostile+nodev"][1]
    assert got["index_load:nodev"] == [hs.HS_ERR_DEVICE, "no HIP device (this library has no CPU search path)"]
    assert got["build_hnsw_batched:nodev"] == [hs.HS_ERR_DEVICE, "no HIP device"]


def test_guard_program():
    """csrc/capi_guard_test.cpp under AddressSanitizer / UBSan, as its own binary: what a throwing body comes out as (std::bad_alloc with
    the default and an entry's own text, the loaders' texts, anything else, a thrown int), a returned status passed through with the
    error text untouched, and the scope guard on return, on throw and dismissed."""
    d = os.path.join(ROOT, "hnsw-slim_amd")
    subprocess.check_call(["make", "-C", d, "capi_guard_test"])
    run = subprocess.run([os.path.join(d, "capi_guard_test")], capture_output=True, text=True)
    assert run.returncode == 0 and "capi_guard ok" in run.stdout, run.stdout + run.stderr


if __name__ == "__main__":
    assert sys.argv[1:] == ["--record"], "usage: test_capi_refusals_cpu.py --record"
    table = run_cases(load_product())
    with open(TABLE, "w") as fh:
        json.dump(table, fh, indent=1)
        fh.write("\n")
    print(f"{len(table)} refusals recorded in {TABLE}")
