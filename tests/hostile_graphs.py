"""Hostile graphs: an independent reading of what a graph must satisfy before a search kernel may index with it, and a catalogue
of small files, arrays and patch streams that each break exactly one item of it.

`violations(parsed)` is written from the kernels' index expressions (beam_search.hip descend / strict_beam, flat_search.hip,
lean_search.hip, slimq_search.hip) and from the host code that packs a graph for them, not from csrc/index_check.hpp: it is the
reference the product's accept / refuse verdict is compared with.  It reads what oracle/chal_encode.py's parse_vanilla / parse_slim /
parse_slimq return (None = the file's own arithmetic -- sizes, offsets of the header, its length -- does not hold, ARITH).

  level      a node's level is negative (a CHAL blob has 2 * level offset bytes; the packer loops l = 1 .. level); in a vanilla file
             also above maxlevel (convertFromHNSW's per-level histograms have maxlevel + 1 rows).  A Slim / SlimQ node may be taller
             than maxlevel: a patch adds nodes and keeps maxlevel.
  enterpoint enterpoint >= n: vec[enterpoint * dim], up_base[enterpoint].
  maxlevel   maxlevel < 0 with n > 0.
  ep_level   level(enterpoint) < maxlevel: the descent's first read is up_ptr[up_base[ep] + maxlevel - 1].
  threshold  threshold_level < 0: the descent runs while lvl > threshold_level, so down to up_ptr[b + 0 - 1] and below.
  count      a list does not fit its storage: a vanilla count word above maxM0 / maxM; CHAL offsets that decrease or exceed total.
  id         a neighbour id >= n: vec[id * dim], tile0[id * stride], up_base[id], the visited set.
  owner      a level-l list (l >= 1) names a node of level < l: the descent moves there and reads up_ptr[up_base[id] + l - 1 .. + l],
             the next owner's words or, for the last owner, the words past the end of up_ptr.  In the image a patch stream leaves
             (unlisted_ok) a named node without any list passes: a diff arrives in chunks, an early chunk names new nodes whose
             records come later, and until then they have no blob, so up_base NONE, which every descent tests before a slot.
  cluster    SlimQ: a cluster id >= num_cluster (g_add[cluster] in the estimate).
An empty graph (n == 0) violates nothing."""
import struct

import numpy as np

from hsutil import load_chal_encode

ARITH = "arithmetic"
VAN_HDR, SLIM_HDR_LEN, SLIMQ_EXT_LEN = 96, 93, 73
FF = 0xFFFFFFFF


def read(kind, raw, dim):
    """parse_vanilla / parse_slim / parse_slimq of `raw`; None when the file's own arithmetic does not hold."""
    ce = load_chal_encode()
    try:
        raw = bytes(raw)
        if kind == "hnsw":
            g = ce.parse_vanilla(raw)
            return g if g["dim"] == dim else None
        return ce.parse_slim(raw, dim) if kind == "slim" else ce.parse_slimq(raw)
    except (AssertionError, struct.error, ValueError, OverflowError, MemoryError):
        return None


def _chal_lists(L, T, off, ids):
    """[(fits, ids)] for levels 0 .. L of a CHAL blob with offsets `off` (L of them) and `ids` (T of them)."""
    out = []
    for lvl in range(L + 1):
        s = 0 if lvl == 0 else int(off[lvl - 1])
        e = T if lvl == L else int(off[lvl])
        fits = s <= e <= T
        out.append((fits, ids[s:e] if fits else ids[:0]))
    return out


def _normal(p):
    """(n, enterpoint, maxlevel, threshold_level, levels, nodes, strict): nodes[i] = None (no lists) or [(fits, ids)] per level."""
    if "blobs" in p:      # parse_slimq
        h = p["hdr"]
        levels = [int(x) for x in p["level"]]
        nodes = []
        for i, blob in enumerate(p["blobs"]):
            L, T = levels[i], int(p["total"][i])
            nodes.append(None if not blob else _chal_lists(L, T, np.frombuffer(blob, np.uint16, L), np.frombuffer(blob, np.uint32, T, 2 * L)))
        return h[0], h[8], h[6], h[7], levels, nodes, False
    if "level" in p:      # parse_slim
        levels = [int(x) for x in p["level"]]
        nodes = []
        for i, off in enumerate(p["offsets"]):
            if off is None:
                nodes.append(None)
                continue
            T = int(p["total"][i])
            bounds = [0] + [int(x) for x in off] + [T]
            fits = all(a <= b for a, b in zip(bounds, bounds[1:])) and bounds[-2] <= T
            nodes.append([(fits, ids) for ids in p["lists"][i]])
        return p["count"], p["enterpoint"], p["maxlevel"], p["threshold_level"], levels, nodes, False
    levels = [len(x) - 1 for x in p["lists"]]   # parse_vanilla
    nodes = [[(c <= (p["maxM"] if l else p["maxM0"]), ids) for l, (c, ids) in enumerate(zip(p["counts"][i], p["lists"][i]))]
             for i in range(p["count"])]
    return p["count"], p["enterpoint"], p["maxlevel"], 0, levels, nodes, True


def violations(parsed, strict=None, unlisted_ok=False):
    """The items (names above, sorted, each once) that `parsed` violates; [] = every kernel may index with it."""
    if parsed is None:
        return [ARITH]
    n, ep, maxlevel, thr, levels, nodes, is_vanilla = _normal(parsed)
    strict = is_vanilla if strict is None else strict
    if n == 0:
        return []
    out = set()
    if any(l < 0 for l in levels) or (strict and maxlevel >= 0 and any(l > maxlevel for l in levels)):
        out.add("level")
    if ep >= n:
        out.add("enterpoint")
    if maxlevel < 0:
        out.add("maxlevel")
    elif ep < n and levels[ep] < maxlevel:
        out.add("ep_level")
    if thr < 0:
        out.add("threshold")
    for i in range(n):
        if nodes[i] is None or levels[i] < 0:
            continue
        for l, (fits, ids) in enumerate(nodes[i]):
            if not fits:
                out.add("count")
                continue
            for x in ids:
                x = int(x)
                if x >= n:
                    out.add("id")
                elif l > 0 and levels[x] < l and not (unlisted_ok and nodes[x] is None):
                    out.add("owner")
    if "blobs" in parsed and any(int(c) >= parsed["ext"][0] for c in parsed["cluster"]):
        out.add("cluster")
    return sorted(out)


# ---- where the words of a (valid) file lie ------------------------------------------------------------------------------------
def locate(kind, raw, dim):
    """Byte offsets into a VALID file: dict(n, ep, maxlevel, threshold (CHAL), levels[i], level_word[i] (CHAL) / size_word[i] (vanilla),
    count_word[(i, l)] and cap[(i, l)] (vanilla), off_slot[(i, l)] (CHAL: the u16 end of level l < level(i)), total[i] (CHAL),
    ids[(i, l)] = (offset of the first id, count), cluster_word[i] (SlimQ))."""
    raw = bytes(raw)
    w = dict(levels=[], level_word={}, size_word={}, count_word={}, cap={}, off_slot={}, total={}, ids={}, cluster_word={})
    if kind == "hnsw":
        (_, _, n, spe, _, _, maxlevel, ep, maxM, maxM0) = struct.unpack_from("<6QiI2Q", raw, 0)
        w.update(n=n, ep=52, maxlevel=48, threshold=None, ep_value=ep, maxlevel_value=maxlevel)
        pos = VAN_HDR + n * spe
        per = 4 + 4 * maxM
        for i in range(n):
            e = VAN_HDR + i * spe
            w["count_word"][(i, 0)], w["cap"][(i, 0)] = e, maxM0
            w["ids"][(i, 0)] = (e + 4, struct.unpack_from("<H", raw, e)[0])
            (sz,) = struct.unpack_from("<I", raw, pos)
            w["size_word"][i] = pos
            pos += 4
            w["levels"].append(sz // per)
            for l in range(1, sz // per + 1):
                b = pos + (l - 1) * per
                w["count_word"][(i, l)], w["cap"][(i, l)] = b, maxM
                w["ids"][(i, l)] = (b + 4, struct.unpack_from("<H", raw, b)[0])
            pos += sz
        return w
    n, spe = struct.unpack_from("<2Q", raw, 0)
    maxlevel, thr, ep = struct.unpack_from("<2iI", raw, 48)
    w.update(n=n, ep=56, maxlevel=48, threshold=52, ep_value=ep, maxlevel_value=maxlevel)
    el0 = SLIM_HDR_LEN
    if kind == "slimq":
        ncl, _, padded = struct.unpack_from("<3Q", raw, SLIM_HDR_LEN)
        el0 = SLIM_HDR_LEN + SLIMQ_EXT_LEN + ncl * padded * 4 + 4 * padded // 8
        w["ncl"] = ncl
    pos = el0 + n * spe
    for i in range(n):
        e = el0 + i * spe
        L, T = struct.unpack_from("<iI", raw, e)
        w["levels"].append(L)
        w["level_word"][i], w["total"][i] = e, T
        if kind == "slimq":
            w["cluster_word"][i] = e + 24
        (sz,) = struct.unpack_from("<I", raw, pos)
        pos += 4
        if sz == 0 or T == 0:
            continue
        off = list(struct.unpack_from(f"<{L}H", raw, pos))
        bounds = [0] + off + [T]
        for l in range(L + 1):
            if l < L:
                w["off_slot"][(i, l)] = pos + 2 * l
            w["ids"][(i, l)] = (pos + 2 * L + 4 * bounds[l], bounds[l + 1] - bounds[l])
        pos += sz
    return w


def put(raw, at, value, fmt="<I"):
    b = bytearray(raw)
    struct.pack_into(fmt, b, at, value)
    return bytes(b)


def word(raw, at, fmt="<I"):
    return struct.unpack_from(fmt, raw, at)[0]


def mutations(kind, raw, dim):
    """Single-field edits of the valid file `raw`, each with the one violation it must produce: [(name, bytes, violation)]."""
    w = locate(kind, raw, dim)
    n, lv = w["n"], w["levels"]
    out = []

    def add(name, at, value, item, fmt="<I"):
        out.append((name, put(raw, at, value, fmt), item))

    for tag, v in (("n", n), ("ff", FF)):
        add(f"ep_{tag}", w["ep"], v, "enterpoint")
    lists0 = [(k, v) for k, v in sorted(w["ids"].items()) if k[1] == 0 and v[1] > 0]
    lists_up = [(k, v) for k, v in sorted(w["ids"].items()) if k[1] > 0 and v[1] > 0]
    for where, ls in (("l0", lists0), ("up", lists_up)):
        if not ls:
            continue
        (_, (at, cnt)) = ls[len(ls) // 2]
        for tag, v in (("n", n), ("ff", FF)):
            add(f"id_{tag}_{where}", at + 4 * (cnt - 1), v, "id")
    if kind == "hnsw":
        for where, keys in (("l0", [k for k in sorted(w["count_word"]) if k[1] == 0]), ("up", [k for k in sorted(w["count_word"]) if k[1] > 0])):
            if keys:
                k = keys[len(keys) // 2]
                add(f"count_cap1_{where}", w["count_word"][k], w["cap"][k] + 1, "count", "<H")
                add(f"count_ffff_{where}", w["count_word"][k], 0xFFFF, "count", "<H")
        owners = [i for i in range(n) if lv[i] > 0]
        if owners:   # the level word of a vanilla node is its size word: -1 breaks the file's arithmetic
            add("level_neg", w["size_word"][owners[0]], FF, ARITH)
        if w["maxlevel_value"] >= 1:   # a vanilla file's levels end at maxlevel (legal in a Slim file: near_misses)
            add("maxlevel_below_tallest", w["maxlevel"], w["maxlevel_value"] - 1, "level", "<i")
    else:
        add("threshold_neg", w["threshold"], -1, "threshold", "<i")
        with_lists = [i for i in range(n) if (i, 0) in w["ids"]]
        bare = [i for i in range(n) if (i, 0) not in w["ids"]]
        if with_lists:   # its size word no longer matches 2 * level + 4 * total
            add("level_neg", w["level_word"][with_lists[0]], -1, ARITH, "<i")
        if bare:
            add("level_neg_bare", w["level_word"][bare[0]], -1, "level", "<i")
        slots = sorted(w["off_slot"])
        if slots:
            i, l = slots[len(slots) // 2]
            add("offset_above_total", w["off_slot"][(i, l)], w["total"][i] + 1, "count", "<H")
        for i in range(n):   # a decreasing pair: the end of level 0 above the end of level 1
            if lv[i] >= 2 and (i, 0) in w["off_slot"]:
                o1 = word(raw, w["off_slot"][(i, 1)], "<H")
                if o1 + 1 <= w["total"][i]:
                    add("offsets_decrease", w["off_slot"][(i, 0)], o1 + 1, "count", "<H")
                    break
        if kind == "slimq":
            add("cluster_ncl", w["cluster_word"][n // 2], w["ncl"], "cluster")
    if n:
        add("maxlevel_above_ep", w["maxlevel"], lv[w["ep_value"]] + 1, "ep_level", "<i")
        add("maxlevel_neg", w["maxlevel"], -1, "maxlevel", "<i")
    owners = [i for i in range(n) if lv[i] > 0 and (i, lv[i]) in w["ids"]]
    flat = [i for i in range(n) if lv[i] == 0]
    if owners and flat:   # the last owner's top list names a level-0 node: past the end of up_ptr
        i = owners[-1]
        at, cnt = w["ids"][(i, lv[i])]
        if cnt:
            add("last_owner_names_level0", at, flat[len(flat) // 2], "owner")
    ones = [i for i in range(n) if lv[i] == 1]
    mids = [k for k in sorted(w["ids"]) if k[1] == 2 and w["ids"][k][1] > 0 and k[0] != (owners[-1] if owners else -1)]
    if ones and mids:   # a level-2 list in the middle of the file names a level-1 node: its successor's slots
        at, cnt = w["ids"][mids[len(mids) // 2]]
        add("level2_names_level1", at + 4 * (cnt - 1), ones[len(ones) // 2], "owner")
    return out


def near_misses(kind, raw, dim):
    """Edits that look like the mutations and are legal: [(name, bytes)]."""
    w = locate(kind, raw, dim)
    n, lv = w["n"], w["levels"]
    out = []
    lists0 = [(k, v) for k, v in sorted(w["ids"].items()) if k[1] == 0 and v[1] > 1]
    lists_up = [(k, v) for k, v in sorted(w["ids"].items()) if k[1] > 0 and v[1] > 0]
    if lists0:
        (_, (at, cnt)) = lists0[len(lists0) // 2]
        out.append(("id_other_valid_l0", put(raw, at, n - 1)))
        out.append(("duplicate_id", put(raw, at + 4, word(raw, at))))
    if lists_up:
        ((i, l), (at, cnt)) = lists_up[len(lists_up) // 2]
        tall = [j for j in range(n) if lv[j] >= l]
        out.append(("id_other_valid_up", put(raw, at, tall[-1])))
    if kind == "hnsw":
        keys = [k for k in sorted(w["count_word"]) if w["ids"][k][1] > 0]
        k = keys[len(keys) // 2]
        out.append(("count_minus_one", put(raw, w["count_word"][k], w["ids"][k][1] - 1, "<H")))
        # up to capacity: the slots behind the count hold zeros (id 0) or ids the list held before, as the reference leaves them
        k0 = [k for k in sorted(w["count_word"]) if k[1] == 0][n // 2]
        out.append(("count_at_capacity", put(raw, w["count_word"][k0], w["cap"][k0], "<H")))
    elif w["maxlevel_value"] >= 1:   # a node (the enter point among them) taller than maxlevel: what a patched index looks like
        out.append(("taller_than_maxlevel", put(raw, w["maxlevel"], w["maxlevel_value"] - 1, "<i")))
    return out


# ---- the same families as arrays (hs_index_from_host_arrays) --------------------------------------------------------------------
def arrays_of(parsed_vanilla):
    """dict(vectors, levels, list_ptr, list_ids, enterpoint, maxlevel, threshold_level) of a parsed vanilla file."""
    g = parsed_vanilla
    flat = [np.asarray(l, np.uint32) for node in g["lists"] for l in node]
    ptr = np.zeros(len(flat) + 1, np.uint64)
    ptr[1:] = np.cumsum([len(x) for x in flat])
    return dict(vectors=g["rows"].copy(), levels=np.array([len(x) - 1 for x in g["lists"]], np.int32), list_ptr=ptr,
                list_ids=np.concatenate(flat).astype(np.uint32), enterpoint=g["enterpoint"], maxlevel=g["maxlevel"], threshold_level=0)


def arrays_violations(a):
    """violations() of the arrays, read as the vanilla reading reads a file (levels end at maxlevel)."""
    n = len(a["levels"])
    lists, counts, t = [], [], 0
    for i in range(n):
        node, cn = [], []
        for _ in range(max(int(a["levels"][i]), 0) + 1):
            s, e = int(a["list_ptr"][t]), int(a["list_ptr"][t + 1])
            node.append(a["list_ids"][s:e] if s <= e else a["list_ids"][:0])
            cn.append(0 if s <= e else 1 << 30)   # a decreasing list_ptr: a list that does not fit
            t += 1
        lists.append(node)
        counts.append(cn)
    out = set(violations(dict(count=n, enterpoint=a["enterpoint"], maxlevel=a["maxlevel"], maxM=1 << 20, maxM0=1 << 20, lists=lists, counts=counts)))
    if any(int(l) < 0 for l in a["levels"]):
        out.add("level")
    if a["threshold_level"] < 0:
        out.add("threshold")
    return sorted(out)


def array_cases(a):
    """([(name, arrays, violation)], [(name, arrays)]): hostile edits of valid arrays `a`, and near misses."""
    n, lv, ptr = len(a["levels"]), a["levels"], a["list_ptr"]
    first = np.concatenate([[0], np.cumsum(lv.astype(np.int64) + 1)])[:n]
    bad, ok = [], []

    def edit(**kw):
        b = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in a.items()}
        for k, v in kw.items():
            if isinstance(v, tuple):
                b[k][v[0]] = v[1]
            else:
                b[k] = v
        return b

    owners = [i for i in range(n) if lv[i] > 0 and ptr[first[i] + lv[i] + 1] > ptr[first[i] + lv[i]]]
    flat = [i for i in range(n) if lv[i] == 0]
    l0 = int(ptr[first[n // 2]])            # first id of a level-0 list
    up = int(ptr[first[owners[0]] + 1])     # first id of a level-1 list
    bad += [("ep_n", edit(enterpoint=n), "enterpoint"), ("ep_ff", edit(enterpoint=FF), "enterpoint"),
            ("id_n_l0", edit(list_ids=(l0, n)), "id"), ("id_ff_l0", edit(list_ids=(l0, FF)), "id"),
            ("id_n_up", edit(list_ids=(up, n)), "id"), ("id_ff_up", edit(list_ids=(up, FF)), "id"),
            ("maxlevel_above_ep", edit(maxlevel=int(lv[a["enterpoint"]]) + 1), "ep_level"),
            ("threshold_neg", edit(threshold_level=-1), "threshold"),
            ("list_ptr_decreases", edit(list_ptr=(int(first[n // 2]) + 1, int(ptr[first[n // 2]]) - 1)), "count"),
            ("last_owner_names_level0", edit(list_ids=(int(ptr[first[owners[-1]] + lv[owners[-1]]]), flat[0])), "owner")]
    twos = [i for i in owners[:-1] if lv[i] >= 2 and ptr[first[i] + 3] > ptr[first[i] + 2]]
    ones = [i for i in range(n) if lv[i] == 1]
    if twos and ones:
        bad.append(("level2_names_level1", edit(list_ids=(int(ptr[first[twos[0]] + 2]), ones[0])), "owner"))
    tall = [i for i in range(n) if lv[i] >= 1]
    ok += [("id_other_valid_l0", edit(list_ids=(l0, n - 1))), ("id_other_valid_up", edit(list_ids=(up, tall[-1]))),
           ("duplicate_id", edit(list_ids=(l0 + 1, int(a["list_ids"][l0]))))]
    return bad, ok


# ---- patch streams --------------------------------------------------------------------------------------------------------------
def patch_records(stream, dim, to_add=True):
    """[(offset of the record, id, level, total, offset of its blob, is_new)] of a well-framed genPatch stream, and its header."""
    new_count, n_old, n_new = struct.unpack_from("<3Q", stream, 0)
    pos, recs = 24, []
    for r in range(n_old + n_new):
        is_new = r >= n_old
        rid, level, total = struct.unpack_from("<IiI", stream, pos)
        head = 16 if is_new else 8
        (nsz,) = struct.unpack_from("<I", stream, pos + 4 + head)
        blob = pos + 4 + head + 4
        recs.append((pos, rid, level, total, blob, is_new))
        pos = blob + nsz + (4 * dim if (is_new and to_add) else 0)
    assert pos == len(stream)
    return (new_count, n_old, n_new), recs


def patched(parsed_old, stream, dim, to_add=True):
    """What parse_slim would return for the image after `stream` is applied to `parsed_old` (the fields violations() reads)."""
    (new_count, _, _), recs = patch_records(stream, dim, to_add)
    n0 = parsed_old["count"]
    level = [int(x) for x in parsed_old["level"]] + [0] * (new_count - n0)
    total = [int(x) for x in parsed_old["total"]] + [0] * (new_count - n0)
    offsets = list(parsed_old["offsets"]) + [None] * (new_count - n0)
    lists = list(parsed_old["lists"]) + [[np.zeros(0, np.uint32)]] * (new_count - n0)
    for (_, rid, L, T, blob, _) in recs:
        if rid >= new_count:
            return None
        level[rid], total[rid] = L, T
        (nsz,) = struct.unpack_from("<I", stream, blob - 4)
        if nsz == 0 or T == 0:
            offsets[rid], lists[rid] = None, [np.zeros(0, np.uint32) for _ in range(L + 1)]
            continue
        off = np.frombuffer(stream, np.uint16, L, blob).astype(np.int64)
        ids = np.frombuffer(stream, np.uint32, T, blob + 2 * L)
        bounds = [0] + list(off) + [T]
        offsets[rid], lists[rid] = off, [ids[bounds[l]:bounds[l + 1]].copy() for l in range(L + 1)]
    return dict(count=new_count, enterpoint=parsed_old["enterpoint"], maxlevel=parsed_old["maxlevel"], threshold_level=parsed_old["threshold_level"],
                level=np.array(level, np.int32), total=np.array(total, np.uint32), offsets=offsets, lists=lists)


def hostile_patches(parsed_old, stream, dim):
    """Well-framed edits of one record of a valid stream (to_add): [(name, bytes, violation)]."""
    (new_count, n_old, _), recs = patch_records(stream, dim)
    after = patched(parsed_old, stream, dim)
    lv = [int(x) for x in after["level"]]
    out = []
    with0 = [r for r in recs if r[3] > 0]
    (pos, rid, L, T, blob, _) = with0[len(with0) // 2]
    out.append(("blob_id_new_count", put(stream, blob + 2 * L, new_count), "id"))
    multi = [r for r in recs if r[2] >= 1 and r[3] > 0]
    (pos, rid, L, T, blob, _) = multi[0]
    out.append(("offset_above_total", put(stream, blob, T + 1, "<H"), "count"))
    flat = [i for i in range(new_count) if lv[i] == 0 and int(after["total"][i]) > 0]   # level-0 nodes that do have a list
    for (pos, rid, L, T, blob, _) in multi:   # a level-1 slice with an id in it
        o0 = struct.unpack_from("<H", stream, blob)[0]
        e1 = T if L == 1 else struct.unpack_from("<H", stream, blob + 2)[0]
        if e1 > o0:
            out.append(("upper_list_names_shorter", put(stream, blob + 2 * L + 4 * o0, flat[len(flat) // 2]), "owner"))
            break
    out.append(("record_id_new_count", put(stream, recs[len(recs) // 2][0], new_count), ARITH))
    return out


# ---- the base files and the product's verdict ---------------------------------------------------------------------------------
BASES = ("handmade_levels", "handmade_star64", "l2_int_d16")   # multi-level and tiny; a list at capacity; built by the reference
DIM = 16
SLIMQ_DIM = 64   # the smallest dim a SlimQ index takes


def base_files(hs, tmp):
    """{(kind, name): (bytes, dim)}: the three vanilla files, their Slim files through hs.convert_slim and through the verbatim
    re-encoding, and the SlimQ twin of handmade_levels (its lists over 64-dim records, through write_slimq)."""
    import os
    from hsutil import GOLDEN
    from slimq_resident_util import write_slimq
    ce = load_chal_encode()
    out = {}
    for name in BASES:
        path = os.path.join(GOLDEN, name + ".hnsw.bin")
        raw = open(path, "rb").read()
        out[("hnsw", name)] = (raw, DIM)
        out[("slim", name + "_verbatim")] = (ce.vanilla_to_slim_verbatim(raw), DIM)
        sp = os.path.join(str(tmp), name + ".slim")
        hs.convert_slim(path, sp, DIM, threads=1)
        out[("slim", name + "_converted")] = (open(sp, "rb").read(), DIM)
    g = ce.parse_vanilla(out[("hnsw", "handmade_levels")][0])
    qp = os.path.join(str(tmp), "levels.slimq")
    write_slimq(qp, SLIMQ_DIM, [[list(map(int, l)) for l in node] for node in g["lists"]], enterpoint=g["enterpoint"], ncl=2)
    out[("slimq", "handmade_levels_twin")] = (ce.write_slimq(ce.parse_slimq(open(qp, "rb").read())), SLIMQ_DIM)
    return out


def product_status(hs, kind, raw, dim, path=None, **kw):
    """(status, text) of loading `raw` as `kind`: through hs_index_load_mem, or hs_index_load when a path to write it to is given."""
    k = {"hnsw": hs.HS_KIND_HNSW, "slim": hs.HS_KIND_SLIM, "slimq": hs.HS_KIND_SLIMQ}[kind]
    src = raw
    if path is not None:
        with open(path, "wb") as f:
            f.write(raw)
        src = str(path)
    try:
        ix = hs.Index(src, k, dim, **kw)
    except hs.HsError as e:
        return e.status, str(e)
    return hs.HS_OK, ix


def accepted(hs, status):
    return status in (hs.HS_OK, hs.HS_ERR_DEVICE)   # without a device a good input gets as far as the device test


def patch_pair(hs, tmp, dim=DIM, n0=300, delta=40, M=8):
    """(old Slim file, new Slim file, the genPatch stream from the one to the other) of a small pair: the first n0 rows, then all."""
    import os
    from hsutil import mixture
    base = mixture(n0 + delta, dim, 17)
    files = {}
    for tag, n in (("old", n0), ("new", n0 + delta)):
        hp, sp = os.path.join(str(tmp), f"{tag}.hnsw"), os.path.join(str(tmp), f"{tag}.slim")
        hs.build_hnsw(base[:n], hp, M=M, ef_construction=100, threads=1)   # serial: the first n0 insertions are the same in both
        hs.convert_slim(hp, sp, dim, threads=1)
        files[tag] = open(sp, "rb").read()
    patch, n_changed, n_added = load_chal_encode().make_patch(files["old"], files["new"], dim, to_add=True)
    assert n_added == delta and n_changed > 0
    return files["old"], files["new"], patch
