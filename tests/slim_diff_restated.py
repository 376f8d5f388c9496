"""Plain-Python reading of HierarchicalNSWSlim::convertFromHNSWWithDiff (hnswalg_slim.h:1110-1424) and genPatch (:1427-1476), with
hnsw->getNeighborsByHeuristic2 (hnswalg.h:481-523), for tests/test_slim_diff_cpu.py.  Written from the reference, not from the
product's host code.

Integer-valued L2 rows only: every distance is an exact int64.  Where the reference is undefined or timing-dependent this reading
takes the product's documented decisions: a re-pruned list holds the entries the heuristic kept (the reference
pops `limit` entries whatever was kept), the changed lists are ascending, elements beyond the previous count start empty.
It does not model libstdc++'s heap order among equal distances: `tied` counts the re-pruned lists whose kept entries hold two equal
distances, and the caller asserts that it is 0.
"""
import struct

import numpy as np

from slim_restated import degree_histogram, hub_threshold, hub_top_n

SLIM_HDR = "<6Q2iI4Q?"


class SlimState:
    """The Slim object between calls: per element the 24 head bytes ([i32 level][u32 total][u64 label][8 pointer bytes]) and the
    row, the neighbour blob (b"" = null pointer), label_lookup_, and what the constructor / loadIndex fixed."""

    def __init__(self, dim, threshold_level, maxM, maxM0, M, efC):
        self.dim, self.threshold_level, self.maxM, self.maxM0, self.M, self.efC = dim, threshold_level, maxM, maxM0, M, efC
        self.count, self.maxlevel, self.enterpoint, self.has_deleted = 0, 0, 0, False
        self.heads, self.rows, self.blobs, self.lookup = [], [], [], {}

    @classmethod
    def from_file(cls, raw, dim):
        """loadIndex (:753-815) + buildLabelLookup (:216-220)."""
        h = struct.unpack_from(SLIM_HDR, raw, 0)
        n, spe = h[0], h[1]
        assert spe == 24 + 4 * dim
        s = cls(dim, h[7], h[9], h[10], h[11], h[12])
        s.count, s.maxlevel, s.enterpoint, s.has_deleted = n, h[6], h[8], h[13]
        pos = struct.calcsize(SLIM_HDR)
        for i in range(n):
            s.heads.append(bytearray(raw[pos:pos + 24]))
            s.rows.append(bytes(raw[pos + 24:pos + spe]))
            pos += spe
        for i in range(n):
            (sz,) = struct.unpack_from("<I", raw, pos)
            pos += 4
            level, total = struct.unpack_from("<iI", s.heads[i], 0)
            if sz == 0 or total == 0:
                s.blobs.append(b"")
            else:
                s.blobs.append(bytes(raw[pos:pos + sz]))
                pos += sz
        assert pos == len(raw)
        for i in range(n):
            s.lookup[struct.unpack_from("<Q", s.heads[i], 8)[0]] = i
        return s

    def level(self, i):
        return struct.unpack_from("<i", self.heads[i], 0)[0]

    def total(self, i):
        return struct.unpack_from("<I", self.heads[i], 4)[0]

    def file_bytes(self):
        """saveIndex (:717-751)."""
        out = [struct.pack(SLIM_HDR, self.count, 24 + 4 * self.dim, 8, 4, 24, 16, self.maxlevel, self.threshold_level, self.enterpoint,
                           self.maxM, self.maxM0, self.M, self.efC, self.has_deleted)]
        for i in range(self.count):
            out.append(bytes(self.heads[i]) + self.rows[i])
        for i in range(self.count):
            sz = 2 * self.level(i) + 4 * self.total(i)
            out.append(struct.pack("<I", sz))
            if sz and self.total(i):
                out.append(self.blobs[i])
        return b"".join(out)

    def record(self, v, is_new, with_row):
        """One record of the stream (:1390-1402, 1406-1422) / of genPatch (:1433-1466)."""
        sz = 2 * self.level(v) + 4 * self.total(v)
        out = struct.pack("<I", v) + bytes(self.heads[v][:16 if is_new else 8]) + struct.pack("<I", sz)
        if sz:
            out += self.blobs[v]
        if is_new and with_row:
            out += self.rows[v]
        return out


def heuristic2(cands, M, dmat):
    """getNeighborsByHeuristic2 (hnswalg.h:481-523) on [(distance, id)]: None when the list passes unchanged (size < M), else the
    kept entries in the order they were kept.  queue_closest pops (-distance, id) pairs largest first: ascending distance, and
    among equal distances the LARGER id first."""
    if len(cands) < M:
        return None
    kept = []
    for d, u in sorted(cands, key=lambda t: (t[0], -t[1])):
        if len(kept) >= M:
            break
        if all(dmat[k, u] >= d for _, k in kept):   # dropped when a kept neighbour is strictly closer to it than the node
            kept.append((d, u))
    return kept


def convert_with_diff(s, g, pct0, pct, top_M0, low_m0, top_M, low_m):
    """convertFromHNSWWithDiff of SlimState `s` from the parsed vanilla file `g` (chal_encode.parse_vanilla).  Returns
    (changed old ids, new ids, dict(reprune=lists re-pruned, tied=re-pruned lists with two kept entries at one distance))."""
    n, lists, rows = g["count"], g["lists"], g["rows"]
    r64 = rows.astype(np.int64)
    assert np.array_equal(r64.astype(np.float32), rows), "integer-valued rows only"
    sq = (r64 * r64).sum(1)
    dmat = sq[:, None] + sq[None, :] - 2 * (r64 @ r64.T)
    prev_count = s.count
    s.count, s.has_deleted, s.maxlevel, s.enterpoint = n, bool(np.any(g["marks"])), g["maxlevel"], g["enterpoint"]
    for i in range(n):   # label_lookup_.merge: keys the Slim index holds keep their id
        s.lookup.setdefault(int(g["labels"][i]), i)
    while len(s.heads) < n:   # the realloc'd slots: empty here
        s.heads.append(bytearray(24))
        s.rows.append(b"")
        s.blobs.append(b"")
    hist, level_cnts = degree_histogram(g)
    thr = [hub_threshold(hist[l], hub_top_n(level_cnts[l], pct0 if l == 0 else pct)) for l in range(g["maxlevel"] + 1)]
    nn = [[None] * len(lists[v]) for v in range(n)]
    for v in range(n):   # :1189-1232
        for l, ids in enumerate(lists[v]):
            size = len(ids)
            M0 = (top_M0 if size > thr[l] else low_m0) if l == 0 else (top_M if size > thr[l] else low_m)
            cands = [(int(dmat[v, int(u)]), int(u)) for u in ids]
            kept = heuristic2(cands, M0, dmat)
            nn[v][l] = set(u for _, u in (cands if kept is None else kept))
    rev = [[set() for _ in lists[v]] for v in range(n)]
    for v in range(n):   # :1234-1241
        for l in range(len(lists[v])):
            for u in nn[v][l]:
                rev[u][l].add(v)
    stats = dict(reprune=0, tied=0)
    old_ids, new_ids = [], []
    for i in range(n):   # :1243-1379
        prev_blob = s.blobs[i]
        L = len(lists[i]) - 1
        neighbours, offsets = [], []
        for l in range(L + 1):
            ids = sorted(nn[i][l] | rev[i][l])
            limit = s.maxM0 if l == 0 else s.maxM
            if len(ids) > limit:   # :1279-1303
                kept = heuristic2([(int(dmat[i, u]), u) for u in ids], limit, dmat)
                stats["reprune"] += 1
                if len({d for d, _ in kept}) != len(kept):
                    stats["tied"] += 1
                ids = [u for _, u in reversed(kept)]   # pop order of a max-heap on distance: farthest first
            if l != s.threshold_level:   # :1317-1330
                ids = [u for u in ids if len(lists[u]) - 1 == l]
            neighbours += ids
            offsets.append(len(neighbours))
        total = len(neighbours)
        label = int(g["labels"][i])
        s.heads[i][0:8] = struct.pack("<iI", L, total)
        s.heads[i][8:16] = struct.pack("<Q", label)
        s.rows[i] = np.ascontiguousarray(rows[i], np.float32).tobytes()
        if total == 0:   # :1340-1343: pointer null, in neither list
            s.blobs[i] = b""
            continue
        blob = struct.pack(f"<{L}H", *offsets[:L]) + struct.pack(f"<{total}I", *neighbours)
        s.blobs[i] = blob
        if s.lookup[label] != i:   # :1360-1378
            new_ids.append(i)
        elif prev_blob == b"" or prev_blob != blob:
            (new_ids if i >= prev_count else old_ids).append(i)
    return old_ids, new_ids, stats


def full_stream(s, old_ids, new_ids):
    """What the std::ostream overload writes (:1384-1422)."""
    return (struct.pack("<3Q", s.count, len(old_ids), len(new_ids)) + b"".join(s.record(v, False, False) for v in old_ids) +
            b"".join(s.record(v, True, False) for v in new_ids))


def gen_patch(s, old_ids, new_ids, cursors, limit, to_add):
    """genPatch (:1427-1476) from cursors = [ind_old_, ind_new_] (advanced in place).  Returns (record bytes, old_written,
    new_written, finished).  The record that reaches `limit` is written and its cursor is not advanced: `return` skips the loop
    increment."""
    out, written, ow, nw = [], 0, 0, 0
    while cursors[0] < len(old_ids):
        ow += 1
        v = old_ids[cursors[0]]
        out.append(s.record(v, False, False))
        written += 2 * s.level(v) + 4 * s.total(v) + 4 + 8 + 4
        if written >= limit:
            return b"".join(out), ow, nw, False
        cursors[0] += 1
    while cursors[1] < len(new_ids):
        nw += 1
        v = new_ids[cursors[1]]
        out.append(s.record(v, True, to_add))
        written += 2 * s.level(v) + 4 * s.total(v) + 4 + 16 + 4 + 4 * s.dim   # the row counts whether or not it is written (:1468-1469)
        if written >= limit:
            return b"".join(out), ow, nw, False
        cursors[1] += 1
    return b"".join(out), ow, nw, True


def patch_from_stream(s, stream, to_add):
    """patchFromStream (:2292-2335) on SlimState `s` (the client's copy)."""
    count, n_old, n_new = struct.unpack_from("<3Q", stream, 0)
    pos = 24
    s.count = count
    while len(s.heads) < count:
        s.heads.append(bytearray(24))
        s.rows.append(b"")
        s.blobs.append(b"")
    for k in range(n_old + n_new):
        (v,) = struct.unpack_from("<I", stream, pos)
        pos += 4
        head = 8 if k < n_old else 16
        s.heads[v][:head] = stream[pos:pos + head]
        pos += head
        if k >= n_old:
            s.lookup[struct.unpack_from("<Q", s.heads[v], 8)[0]] = v
        (sz,) = struct.unpack_from("<I", stream, pos)
        pos += 4
        s.blobs[v] = bytes(stream[pos:pos + sz])
        pos += sz
        if to_add and k >= n_old:
            s.rows[v] = bytes(stream[pos:pos + 4 * s.dim])
            pos += 4 * s.dim
    assert pos == len(stream)
