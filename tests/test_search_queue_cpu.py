"""The search queue (hs_queue_*) without a GPU: the new symbols are declared, exported and bound; the host core of the queue
(csrc/search_queue.hpp: segment table, auto-flush, tickets, slots, completion rules) runs against a fake CPU backend as two
stand-alone sanitizer builds (make search_queue_test), never inside Python; and the refusals that need no device."""
import ctypes
import os
import re
import subprocess

import pytest

from hsutil import ROOT, load_product

QUEUE_SYMBOLS = ["hs_queue_create", "hs_queue_free", "hs_queue_submit", "hs_queue_submit_dev", "hs_queue_flush", "hs_queue_wait",
                 "hs_queue_join_stream", "hs_queue_drain", "hs_queue_info"]
LIBDIR = os.path.join(ROOT, "hnsw-slim_amd")
CASES = "search_queue ok: 14 cases"


@pytest.fixture(scope="module")
def hs():
    m = load_product()
    m.build_library()
    return m


def test_queue_symbols_declared_exported_and_bound(hs):
    hdr = open(os.path.join(ROOT, "include", "hnsw_slim_amd.h")).read()
    declared = set(re.findall(r"\b(hs_[a-z_0-9]+)\s*\(", hdr))
    L = hs.lib()
    for name in QUEUE_SYMBOLS:
        assert name in declared, f"{name} is not declared in include/hnsw_slim_amd.h"
        assert hasattr(L, name), f"{name} is not exported"
        assert name in hs.EXPORTS
    assert "struct hs_queue_info {" in hdr and "typedef struct hs_queue hs_queue;" in hdr
    for name in ("SearchQueue", "QueueTicket", "HsQueueInfo"):
        assert hasattr(hs, name)
    assert [f for f, _ in hs.HsQueueInfo._fields_] == ["submitted", "launches", "pending", "in_flight", "largest_launch", "device_bytes"]
    for method in ("submit", "submit_dev", "flush", "wait", "join_stream", "drain", "info", "close"):
        assert callable(getattr(hs.SearchQueue, method))


def test_null_arguments_are_refused_without_a_device(hs):
    L = hs.lib()
    h, t = ctypes.c_void_p(), ctypes.c_uint64(0)
    assert L.hs_queue_create(None, 10, hs.HS_MODE_PQ, 64, 2, None, ctypes.byref(h)) == hs.HS_ERR_INVALID and not h
    assert L.hs_queue_create(None, 10, hs.HS_MODE_PQ, 64, 2, None, None) == hs.HS_ERR_INVALID
    assert L.hs_queue_submit(None, None, 0, None, None, None, None, None, None, ctypes.byref(t)) == hs.HS_ERR_INVALID
    for call in (L.hs_queue_flush, L.hs_queue_drain):
        assert call(None) == hs.HS_ERR_INVALID
    assert L.hs_queue_wait(None, 1) == hs.HS_ERR_INVALID
    assert L.hs_queue_join_stream(None, 1, None) == hs.HS_ERR_INVALID
    assert L.hs_queue_info(None, None) == hs.HS_ERR_INVALID
    L.hs_queue_free(None)   # as free(NULL)


@pytest.fixture(scope="module")
def programs():
    subprocess.check_call(["make", "-C", LIBDIR, "search_queue_test"])
    return os.path.join(LIBDIR, "search_queue_test"), os.path.join(LIBDIR, "search_queue_test_tsan")


def test_host_core_under_address_and_ub_sanitizers(programs):
    """1, 2, 64, 65 and 300 segments, segments of one row, auto-flush at / below / above max_queries, the oversize refusal, nq == 0,
    slots exhausted, a launch that fails to enqueue, a launch whose check reports, double wait, unknown ticket, drain with
    unwaited tickets, 8 threads x 200 submit + wait, 12 threads of submit + wait against a thread that drains."""
    out = subprocess.run([programs[0]], capture_output=True, text=True)
    assert out.returncode == 0 and CASES in out.stdout, out.stdout + out.stderr


def test_host_core_under_thread_sanitizer(programs):
    out = subprocess.run([programs[1]], capture_output=True, text=True)
    if out.returncode != 0 and "unexpected memory mapping" in out.stdout + out.stderr:
        pytest.skip("ThreadSanitizer's runtime refuses to start on this machine: " + (out.stdout + out.stderr).strip().splitlines()[0])
    assert out.returncode == 0 and CASES in out.stdout, out.stdout + out.stderr
