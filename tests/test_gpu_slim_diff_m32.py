"""convertFromHNSWWithDiff / genPatch on two resident indexes (hs_slim_convert_diff, csrc/convert_diff.hip + capi_diff.cpp) for the
reference's default graph, M = 32: capacities of 64 / 32, so the list passes and the diff kernel run with 64 slots per task.
The pattern of tests/test_gpu_slim_diff.py: one round on the resident pair against the host twin hs_slim_convert_diff_files on the
files of the same state, byte for byte, and -- on integer-valued rows, the only ones tests/slim_diff_restated.py reads -- against
that independent Python reading.  The list passes must have run on the device: a fall-back to the host conversion cannot pass.

Two parameter sets: the defaults (32 / 8 / 16 / 4; the capacity of 64 alone selects the wide stride, the final lists stay short) and
64 / 48 / 32 / 24, whose changed nodes end with level-0 lists above 32 ids and whose longest list outgrows the tile stride the Slim
index was loaded with, so the write path re-tiles the resident index."""
import struct

import numpy as np
import pytest

from hsutil import load_chal_encode, load_product, mixture
from slim_diff_restated import SlimState, convert_with_diff, full_stream

pytestmark = pytest.mark.gpu
L2 = 0
DIM, N0, ADD, CAP = 32, 2800, 200, 3000
SETS = {"defaults": dict(), "wide": dict(top_degree_M0=64, low_degree_m0=48, top_degree_M=32, low_degree_m=24)}
LIMIT = 4000   # genPatch's byte limit per chunk: dozens of chunks


@pytest.fixture(scope="module")
def hs():
    m = load_product()
    m.build_library()
    assert m.device_count() > 0
    return m


def _bits(ix, q, exact):
    ix.set_ef(64)
    ix.set_exact_order(exact)
    r = ix.search_ids(q, 10, want_dists=True, want_stats=True)
    kernel = ix.last_kernel()
    ix.set_exact_order(False)
    return (r["labels"].tobytes(), r["dists"].tobytes(), r["cnt"].tobytes(), r["stats"][:, :3].tobytes()), kernel


def _drain(d, limit):
    chunks = []
    for _ in range(100000):
        b, ow, nw, fin = d.next(limit, True)
        chunks.append(b)
        if fin:
            return chunks
    raise AssertionError("genPatch never finished")


def _tile_stride(raw):
    deg = max(len(l[0]) for l in load_chal_encode().parse_slim(raw, DIM)["lists"])
    return max(16, (deg + 15) // 16 * 16)


@pytest.fixture(scope="module", params=[(s, i) for i in (False, True) for s in SETS], ids=lambda p: f"{p[0]}_{'int' if p[1] else 'float'}")
def served(request, hs, tmp_path_factory):
    """One round of the server: the resident pair, 200 rows added, the conversion, and what it handed out (a diff object serves
    until the next conversion of its index, so everything is read from it here)."""
    name, integer = request.param
    kw = SETS[name]
    tmp = tmp_path_factory.mktemp(f"m32_{name}_{int(integer)}")
    base = mixture(CAP, DIM, 11, integer=integer)
    hp, sp, now, saved = (str(tmp / x) for x in ("h.bin", "old.slim", "now.hnsw", "server.slim"))
    hs.build_hnsw(base[:N0], hp, M=32, ef_construction=80, threads=1)
    hs.convert_slim(hp, sp, DIM, **kw)
    sx = hs.Index(sp, hs.HS_KIND_SLIM, DIM, max_elements=CAP)
    hx = hs.Index(hp, hs.HS_KIND_HNSW, DIM, max_elements=CAP)
    hx.seed_levels(100, N0)
    hx.add_points(base[N0:], np.arange(N0, N0 + ADD), threads=1)
    hx.save(now)
    d = sx.convert_diff(hx, **kw)
    sx.save_slim(saved)
    old_ids, new_ids = d.ids()
    return dict(hs=hs, name=name, integer=integer, kw=kw, tmp=tmp, base=base, sp=sp, now=now, saved=saved, sx=sx, hx=hx, used_gpu=d.used_gpu,
                info=d.info(), old_ids=old_ids.tolist(), new_ids=new_ids.tolist(), stream=d.stream(), chunks=_drain(d, LIMIT))


def test_list_passes_ran_on_the_device_and_equal_the_host_twin(served):
    s, hs = served, served["hs"]
    assert s["used_gpu"], "the list passes did not run on the GPU"
    ref = str(s["tmp"] / "files.slim")
    f = hs.slim_convert_diff_files(s["sp"], s["now"], ref, DIM, threads=4, **s["kw"])
    wo, wn = f.ids()
    assert s["old_ids"] == wo.tolist() and s["new_ids"] == wn.tolist(), "changed lists"
    assert s["info"] == f.info()
    assert s["stream"] == f.stream(), "stream"
    assert s["chunks"] == _drain(f, LIMIT), "chunked drain"
    new_raw = open(s["saved"], "rb").read()
    assert new_raw == open(ref, "rb").read(), "saved Slim image"
    # the premises
    assert s["info"]["n_old"] > 0 and s["new_ids"] == list(range(N0, N0 + ADD))
    lists = load_chal_encode().parse_slim(new_raw, DIM)["lists"]
    longest = max(len(lists[i][0]) for i in s["old_ids"] + s["new_ids"])
    old_stride, new_stride = _tile_stride(open(s["sp"], "rb").read()), _tile_stride(new_raw)
    if s["name"] == "wide":
        assert longest > 32, "premise: a changed node's final level-0 list holds more than 32 ids"
        assert s["info"]["n_reprune"] > 0, "premise: a union above the capacity of 64 was pruned again"
        assert old_stride < new_stride == 64, "premise: the conversion outgrew the resident tile stride (the re-tile step ran)"
    else:
        assert old_stride == new_stride, "premise: the changed nodes were written in place"
    if s["integer"]:   # the independent reading (tests/slim_diff_restated.py reads integer-valued rows only)
        kw = s["kw"]
        state = SlimState.from_file(open(s["sp"], "rb").read(), DIM)
        g = load_chal_encode().parse_vanilla(open(s["now"], "rb").read())
        old_ids, new_ids, stats = convert_with_diff(state, g, 0.02, 0.02, kw.get("top_degree_M0", 32), kw.get("low_degree_m0", 8),
                                                    kw.get("top_degree_M", 16), kw.get("low_degree_m", 4))
        assert stats["tied"] == 0, "the restatement does not model the heap order among equal distances: choose another seed"
        assert (s["old_ids"], s["new_ids"]) == (old_ids, new_ids), "changed lists (restatement)"
        assert s["info"]["n_reprune"] == stats["reprune"]
        assert new_raw == state.file_bytes(), "saved Slim image (restatement)"
        assert s["stream"] == full_stream(state, old_ids, new_ids), "stream (restatement)"


def test_resident_slim_index_answers_as_a_fresh_load(served):
    s, hs = served, served["hs"]
    q = mixture(64, DIM, 12, integer=s["integer"])
    whole = hs.Index(s["saved"], hs.HS_KIND_SLIM, DIM)
    got, kernel = _bits(s["sx"], q, False)
    assert kernel == "hs::flat_kernel", kernel
    assert got == _bits(whole, q, False)[0], "flat kernel, k=10, ef=64"
    got, kernel = _bits(s["sx"], q, True)
    assert kernel.startswith("hs::strict_kernel"), kernel
    assert got == _bits(whole, q, True)[0], "exact order"
    assert s["sx"].info()["n"] == N0 + ADD


def test_genpatch_chunks_bring_a_client_to_the_servers_file(served):
    s, hs = served, served["hs"]
    old_raw, new_raw = open(s["sp"], "rb").read(), open(s["saved"], "rb").read()
    # premise: the 200 rows moved neither the enter point nor the top level, which the stream does not carry
    assert struct.unpack_from("<iiI", old_raw, 48) == struct.unpack_from("<iiI", new_raw, 48)
    assert len(s["chunks"]) >= 3
    client = hs.Index(s["sp"], hs.HS_KIND_SLIM, DIM, max_elements=CAP)
    for c in s["chunks"]:
        client.patch(c, to_add=True)
    out = str(s["tmp"] / "client.slim")
    client.save_slim(out)
    assert open(out, "rb").read() == new_raw, "the client's saved file"


def test_a_second_call_with_nothing_changed(served):
    s = served
    d = s["sx"].convert_diff(s["hx"], **s["kw"])
    assert d.used_gpu, "the list passes did not run on the GPU"
    assert d.info()["n_old"] == 0 and d.info()["n_new"] == 0 and d.stream() == struct.pack("<3Q", N0 + ADD, 0, 0)
    assert [x.tolist() for x in d.ids()] == [[], []]
