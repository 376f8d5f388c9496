"""Helpers of the resident-SlimQ tests (test_slimq_resident_cpu.py, test_gpu_slimq_resident.py).

numpy_arrays is an independent reading of the three arrays a resident HNSW-SlimQ index searches -- rec, ftile, uptile -- written from
the file format (header, elements, CHAL blobs) and the stride rules of DESIGN.md 4q, not from csrc/slimq_tiles.hpp: it
parses the file with struct / numpy and places every word.  write_slimq writes such a file byte by byte from Python lists, and
HANDMADE are the small graphs both test files share.  The hand-made search cases (slimq_handmade.py) write their files with
write_slimq too, and the plain-Python reading of the search (slimq_search_restated.py) runs over parse_slimq's fields."""
import struct

import numpy as np

NONE = 0xFFFFFFFF


def rec_words(padded):
    return (4 + 2 * (padded // 64) + 3) & ~3


def write_slimq(path, dim, lists, metric=0, enterpoint=0, ncl=1, seed=0, threshold_level=0, factors=None, cluster=None, code=None):
    """lists[i] = the neighbour lists of node i, level 0 first (one list per level 0..level(i)); an empty lists[i] (or one whose
    lists are all empty) is written as a node without a blob, with its level kept.  lists[i] may also be (level, []) for a node of
    that level without a blob.  Records are random but reproducible; factors (n x 3 f32: f_add, f_rescale, f_error), cluster (n u32)
    and code (n x padded/64 u64) replace the random ones where given, which changes none of the other bytes.  Returns the dict numpy
    reading should find."""
    n = len(lists)
    padded = (dim + 63) // 64 * 64
    sbin, sex = padded // 8 + 12, padded * 3 // 8 + 8
    spe = 28 + sbin + sex
    rng = np.random.default_rng(seed + 17 * dim + n)
    levels, nodes = [], []
    for l in lists:
        if isinstance(l, tuple):
            levels.append(l[0]); nodes.append([])
        else:
            levels.append(max(len(l) - 1, 0)); nodes.append([list(x) for x in l])
    maxlevel = max(levels) if n else 0
    hdr = struct.pack("<6Q", n, spe, 8, 4, 28, 16) + struct.pack("<iiI", maxlevel, threshold_level, enterpoint)
    hdr += struct.pack("<4Q", 16, 32, 16, 100) + b"\0" + struct.pack("<3Q", ncl, dim, padded)
    hdr += struct.pack("<3Q", 24, 28, 28 + sbin) + struct.pack("<3Q", sbin, sex, 3) + bytes([metric])
    cent = rng.normal(0, 1, (ncl, padded)).astype(np.float32)
    flips = rng.integers(0, 256, 4 * padded // 8, dtype=np.uint8)
    rnd_cluster = rng.integers(0, ncl, n).astype(np.uint32)
    rnd_code = rng.integers(0, 1 << 63, (n, padded // 64), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, (n, padded // 64)).astype(np.uint64)
    rnd_factors = rng.normal(0, 3, (n, 3)).astype(np.float32)
    cluster = rnd_cluster if cluster is None else np.ascontiguousarray(cluster, np.uint32)
    code = rnd_code if code is None else np.ascontiguousarray(code, np.uint64)
    factors = rnd_factors if factors is None else np.ascontiguousarray(factors, np.float32)
    assert cluster.shape == (n,) and code.shape == (n, padded // 64) and factors.shape == (n, 3)
    labels = (np.arange(n, dtype=np.uint64) * np.uint64(3) + np.uint64(1000))
    body, blobs = [], []
    for i in range(n):
        total = sum(len(x) for x in nodes[i])
        el = bytearray(spe)
        struct.pack_into("<iIQ", el, 0, levels[i], total, int(labels[i]))
        struct.pack_into("<I", el, 24, int(cluster[i]))
        el[28:28 + padded // 8] = code[i].tobytes()
        el[28 + padded // 8:28 + padded // 8 + 12] = factors[i].tobytes()
        body.append(bytes(el))
        if total == 0:
            blobs.append(struct.pack("<I", 0))
            continue
        offs, run = [], 0
        for x in nodes[i][:-1]:
            run += len(x)
            offs.append(run)
        blob = struct.pack(f"<{len(offs)}H", *offs) + b"".join(struct.pack(f"<{len(x)}I", *x) for x in nodes[i])
        assert len(blob) == 2 * levels[i] + 4 * total
        blobs.append(struct.pack("<I", len(blob)) + blob)
    with open(path, "wb") as f:
        f.write(b"".join([hdr, cent.tobytes(), flips.tobytes()] + body + blobs))
    return dict(n=n, dim=dim, padded=padded, levels=levels)


def parse_slimq(path):
    """The file as SURVEY.md 8b lays it out -> dict(n, padded, level, cluster, code (n x padded/64 u64), factors (n x 3 f32),
    lists[i][l] = ids of level l, or [] for a node without a blob)."""
    b = open(path, "rb").read()
    n, spe, _, _, _, _ = struct.unpack_from("<6Q", b, 0)
    o = 48 + 12 + 32 + 1
    ncl, dim, padded = struct.unpack_from("<3Q", b, o)
    o += 24 + 24
    sbin, sex, _ = struct.unpack_from("<3Q", b, o)
    o += 24 + 1
    assert spe == 28 + sbin + sex and sbin == padded // 8 + 12
    o += ncl * padded * 4 + 4 * padded // 8
    level, total = np.zeros(n, np.int64), np.zeros(n, np.int64)
    cluster = np.zeros(n, np.uint32)
    code = np.zeros((n, padded // 64), np.uint64)
    factors = np.zeros((n, 3), np.float32)
    for i in range(n):
        e = b[o + i * spe:o + (i + 1) * spe]
        level[i], total[i] = struct.unpack_from("<iI", e, 0)
        cluster[i] = struct.unpack_from("<I", e, 24)[0]
        code[i] = np.frombuffer(e[28:28 + padded // 8], np.uint64)
        factors[i] = np.frombuffer(e[28 + padded // 8:28 + padded // 8 + 12], np.float32)
    o += n * spe
    lists = []
    for i in range(n):
        sz = struct.unpack_from("<I", b, o)[0]
        o += 4
        if sz == 0 or total[i] == 0:
            lists.append([])
            continue
        L, T = int(level[i]), int(total[i])
        offs = list(struct.unpack_from(f"<{L}H", b, o))
        ids = np.frombuffer(b[o + 2 * L:o + 2 * L + 4 * T], np.uint32)
        bounds = [0] + offs + [T]
        lists.append([ids[bounds[l]:bounds[l + 1]] for l in range(L + 1)])
        o += sz
    assert o == len(b)
    return dict(n=n, padded=padded, level=level, cluster=cluster, code=code, factors=factors, lists=lists)


def stride_of(longest):
    """a tile's slots: the longest list rounded up to 16, at least 16; no tile beyond 64"""
    return 0 if longest > 64 else max(16, (longest + 15) // 16 * 16)


def numpy_arrays(path, fused=True):
    """-> {0: (rec words, 1, rw), 1: (ftile words, stride, rw), 2: (uptile words, up_stride, rw + 4)}; an absent array is
    (empty, 0, 0)."""
    q = parse_slimq(path)
    n, padded = q["n"], q["padded"]
    rw = rec_words(padded)
    rec = np.zeros((n, rw), np.uint32)
    rec[:, 0] = q["factors"][:, 0].view(np.uint32)
    rec[:, 1] = q["factors"][:, 1].view(np.uint32)
    rec[:, 2] = q["cluster"]
    rec[:, 3] = q["factors"][:, 2].view(np.uint32)
    rec[:, 4:4 + 2 * (padded // 64)] = np.ascontiguousarray(q["code"]).view(np.uint32).reshape(n, -1)
    none = (np.zeros(0, np.uint32), 0, 0)
    out = {0: (rec.reshape(-1).copy(), 1, rw), 1: none, 2: none}
    if not fused:
        return out
    lists = q["lists"]
    # upper slots: a node with a blob and level L > 0 owns L + 1 consecutive rows (its L lists, then one nobody owns), in id order
    up_base = np.full(n, NONE, np.uint32)
    rows = []   # per row: the ids of its list, or None for an unowned row
    for i in range(n):
        if len(lists[i]) > 1:
            up_base[i] = len(rows)
            rows += [lists[i][l] for l in range(1, len(lists[i]))] + [None]
    stride = stride_of(max([len(l[0]) for l in lists if len(l)], default=0))
    if stride:
        ft = np.zeros((n, stride, rw), np.uint32)
        ft[:, :, 3] = NONE
        for i in range(n):
            if len(lists[i]):
                for j, nb in enumerate(lists[i][0]):
                    ft[i, j] = rec[nb]
                    ft[i, j, 3] = nb
        out[1] = (ft.reshape(-1), stride, rw)
    if rows:
        ups = stride_of(max(len(r) for r in rows if r is not None))
        if ups:
            ut = np.zeros((len(rows), ups, rw + 4), np.uint32)
            ut[:, :, 3] = NONE
            for t, r in enumerate(rows):
                for j, nb in enumerate(r if r is not None else []):
                    ut[t, j, :rw] = rec[nb]
                    ut[t, j, 3] = nb
                    ut[t, j, rw] = up_base[nb]
            out[2] = (ut.reshape(-1), ups, rw + 4)
    return out


def ring(n, deg):
    return [[[(i + 1 + j) % n for j in range(deg)]] for i in range(n)]


def handmade():
    """name -> (dim, lists, enterpoint): the shapes at which the tile assembly takes another path."""
    cases = {}
    cases["single"] = (64, [(0, [])], 0)
    # node 1: level 2 without a blob (up_base NONE) listed by nodes 0 and 2 on levels 0..2
    cases["empty_level2"] = (64, [[[1, 2], [1, 2], [1]], (2, []), [[0, 1], [1, 0], [1]], [[0, 1, 2]]], 0)
    cases["deg16"] = (128, ring(20, 16), 0)
    cases["deg17"] = (128, ring(20, 17), 0)
    cases["hub64"] = (64, [[list(range(1, 65))]] + [[[0]] for _ in range(64)], 0)
    cases["hub65"] = (64, [[list(range(1, 66))]] + [[[0]] for _ in range(65)], 0)
    up = [[[1], list(range(1, 66))]] + [[[0], [0]] for _ in range(65)]
    cases["upper65"] = (64, up, 0)
    up17 = [[[1, 2], list(range(1, 18)), [1]]] + [[[0], [0], [0]]] + [[[0], [0]] for _ in range(16)] + [[[0, 1]] for _ in range(3)]
    cases["upper17_d192"] = (192, up17, 0)
    return cases


HANDMADE = handmade()
