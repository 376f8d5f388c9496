"""Hand-made SlimQ files for the search kernel: the cases test_slimq_handmade_cpu.py and test_gpu_slimq_handmade.py share.

Three families, all written by write_slimq (labels 3 i + 1000, so an id handed out as a label shows):
  layout   random records, ncl = 2: the eight HANDMADE graphs of slimq_resident_util and graphs whose lists are wider than a tile
           (64 ids) on level 0, on the upper levels, on both or on neither -- every pairing of {fused, CSR} level 0 with {fused, CSR}
           upper levels.  `strides` = (level-0 tile stride, upper tile stride) the index must report; 0 = that array is absent.
  steered  ncl = 1, f_rescale = 0, f_add small integers: a node's estimate is f_add + g_add bit for bit, g_add the same for every
           node of a query, so ties and minima of the estimates stand where f_add puts them.  Rows and queries are small integers, so
           the exact distances tie as well.
  hash     2000 nodes without lists but for one chain over ids that share eight home slots of a 128-slot expanded-node set.
"""
import functools

import numpy as np

from slimq_resident_util import HANDMADE

EFK_ALL = ((1, 1), (2, 1), (63, 10), (64, 63), (65, 64), (128, 65), (129, 10), (256, 100), (257, 10), (512, 10), (513, 10), (1024, 10))
NQ = 32


class Case:
    def __init__(self, name, family, dim, lists, enterpoint=0, metric=0, ncl=2, f_add=None, int_rows=False, runs=((48, 10), (8, 3)),
                 strides=None, hash_slots=0, seed=0):
        self.name, self.family, self.dim, self.lists, self.enterpoint, self.metric, self.ncl = name, family, dim, lists, enterpoint, metric, ncl
        self.runs, self.strides, self.hash_slots = tuple(runs), strides, hash_slots
        self.n = n = len(lists)
        self.padded = (dim + 63) // 64 * 64
        self.t_const = 3.0 * float(np.sqrt(self.padded))   # any positive number serves; both sides are handed this one
        rng = np.random.default_rng(1000 + seed + 31 * n + dim)
        if int_rows:
            self.rows = rng.integers(0, 4, (n, dim)).astype(np.float32)
            self.queries = rng.integers(0, 4, (NQ, dim)).astype(np.float32)
        else:
            self.rows = rng.normal(0, 1, (n, dim)).astype(np.float32)
            self.queries = rng.normal(0, 1, (NQ, dim)).astype(np.float32)
        self.factors = None
        if f_add is not None:
            self.factors = np.zeros((n, 3), np.float32)
            self.factors[:, 0] = np.asarray(f_add, np.float32)

    def write(self, path):
        from slimq_resident_util import write_slimq
        write_slimq(path, self.dim, self.lists, metric=self.metric, enterpoint=self.enterpoint, ncl=self.ncl, factors=self.factors)

    def many_queries(self, nq):
        """the queries of the ordered two-launch pass (from 6144 queries on)"""
        return np.random.default_rng(77 + self.n).normal(0, 1, (nq, self.dim)).astype(np.float32)


def pick(rng, pool, m, me):
    """m distinct ids of pool, not me"""
    pool = [x for x in pool if x != me]
    return [int(x) for x in rng.choice(pool, size=min(m, len(pool)), replace=False)]


def leveled(seed, n, level_of, deg0, wide0=lambda i: 0, deg_up=lambda i, l: 6):
    """lists of a graph whose node i has level level_of(i): level-0 lists of deg0 random ids (wide0(i) ids where that is not 0), the
    level-l list of node i names deg_up(i, l) nodes of level >= l (an upper list may only name nodes that own that level)."""
    rng = np.random.default_rng(seed)
    lv = [level_of(i) for i in range(n)]
    lists = []
    for i in range(n):
        ls = [pick(rng, range(n), wide0(i) or deg0, i)]
        for l in range(1, lv[i] + 1):
            ls.append(pick(rng, [j for j in range(n) if lv[j] >= l], deg_up(i, l), i))
        lists.append(ls)
    return lists


def layout_cases():
    out = []
    expect = dict(single=(16, 0), empty_level2=(16, 16), deg16=(16, 0), deg17=(32, 0), hub64=(64, 0), hub65=(0, 0), upper65=(16, 0),
                  upper17_d192=(16, 32))
    for name in sorted(HANDMADE):
        dim, lists, ep = HANDMADE[name]
        out.append(Case(name, "layout", dim, lists, ep, strides=expect[name]))
    rng = np.random.default_rng(5)
    hubs = [[[(i + 1 + j) % 260 for j in range(5)]] for i in range(260)]
    for h, m in enumerate((64, 65, 128, 129, 200)):
        hubs[h] = [pick(rng, range(260), m, h)]
    out.append(Case("hubs", "layout", 64, hubs, strides=(0, 0)))
    every7 = lambda i: 200 if i % 7 == 0 else 0
    out.append(Case("wide0", "layout", 64, leveled(11, 300, lambda i: 0, 8, every7), strides=(0, 0)))
    lv3 = lambda i: 2 if i < 6 else 1 if i < 40 else 0
    out.append(Case("wide0_up", "layout", 64, leveled(12, 300, lv3, 8, every7, lambda i, l: 5 if l == 2 else 16 if i % 3 == 0 else 7),
                    strides=(0, 16)))
    lv1 = lambda i: 1 if i < 140 else 0
    out.append(Case("wide_up", "layout", 64, leveled(13, 300, lv1, 16, deg_up=lambda i, l: 130 if i == 0 else 9), strides=(16, 0)))
    # both wide: every level-2 node owns a level-1 list of 130 ids, so the descent scans one wherever level 2 leaves it
    lvb = lambda i: 2 if i < 5 else 1 if i < 140 else 0
    both = lambda i, l: 4 if l == 2 else 130 if i < 5 else 9
    for dim, metric in ((64, 0), (128, 0), (100, 0), (320, 1), (768, 1)):
        name = "wide_both" if dim == 64 else f"wide_both_d{dim}_{'ip' if metric else 'l2'}"
        out.append(Case(name, "layout", dim, leveled(14, 300, lvb, 8, every7, both), metric=metric, strides=(0, 0)))
    return out


def steered_cases():
    out = []
    # descent: the entry (node 0, f_add 50) owns a level-1 list of the ids 1..130 in order; everyone else sits at 20 but the minima
    for name, minima in (("descent_ties_63", (63,)), ("descent_ties_64", (64,)), ("descent_ties_129", (129,)), ("descent_ties_9_69", (9, 69))):
        n = 150
        lists = [[[(i + 1 + j) % n for j in range(4)]] + ([[0]] if 1 <= i <= 130 else []) for i in range(n)]
        lists[0] = [lists[0][0], list(range(1, 131))]
        f = np.full(n, 20.0)
        f[0] = 50.0
        for idx in minima:
            f[1 + idx] = 5.0   # list index idx holds id idx + 1
        c = Case(name, "steered", 64, lists, ncl=1, f_add=f, int_rows=True, runs=((48, 10),), strides=(16, 0))
        c.first_pop = 1 + minima[0]
        out.append(c)
    for name, values in (("all_equal", (7,)), ("four_values", (3, 5, 7, 9))):
        rng = np.random.default_rng(21)
        n = 1100
        lists = [[pick(rng, range(n), 70 if i % 50 == 0 else 12, i)] for i in range(n)]
        out.append(Case(name, "steered", 64, lists, ncl=1, f_add=rng.choice(values, n), int_rows=True, runs=EFK_ALL, strides=(0, 0)))
    # duplicates: node 0 names id 40 at list indexes 3 and 67 of 70; node 1 names 2 twice, 3 three times and itself
    n = 90
    lists = [[[(i + 1) % n, (i + 5) % n]] for i in range(n)]
    first = list(range(1, 71))
    first[3] = first[67] = 40
    lists[0] = [first]
    lists[1] = [[2, 2, 3, 1, 3, 3, 50]]
    lists[2] = [[2, 60, 60, 4]]
    f = np.random.default_rng(22).integers(1, 12, n)
    out.append(Case("duplicates", "steered", 64, lists, ncl=1, f_add=f, int_rows=True, runs=((128, 10), (8, 5)), strides=(0, 0)))
    # n < k: nodes 0..3 reachable from the entry (3 has no lists), 4 and 5 are not
    lists = [[[1, 2]], [[2, 3]], [[0, 3]], (0, []), [[0]], [[4]]]
    out.append(Case("n_lt_k", "steered", 64, lists, ncl=1, f_add=[4, 2, 6, 3, 1, 1], int_rows=True, runs=((1, 10), (16, 10)), strides=(16, 0)))
    return out


HASH_SLOTS = 128


def home_slot(i, slots=HASH_SLOTS):
    """The home slot of id i in the kernel's expanded-node set, restated from csrc/slimq_search.hip (hash_of): this premise knows the
    kernel's hash on purpose -- the collisions have to be arranged for the table the kernel really keeps."""
    return ((i * 2654435761) & 0xFFFFFFFF) >> 7 & (slots - 1)


def probe_lengths(expanded, slots=HASH_SLOTS):
    """Linear probing of the ids in expansion order -> (longest run of occupied slots walked before the free one, whether a walk
    passed the table's end)."""
    tab, longest, wrapped = [None] * slots, 0, False
    for i in expanded:
        h, steps = home_slot(i, slots), 0
        while tab[(h + steps) % slots] is not None:
            steps += 1
        wrapped |= h + steps >= slots
        longest = max(longest, steps)
        tab[(h + steps) % slots] = i
    return longest, wrapped


def hash_cases():
    out = []
    n = 2000
    crowd = [i for i in range(n) if home_slot(i) >= 120]
    assert len(crowd) >= 110
    for m in (90, 110):
        chain = crowd[:m]
        lists = [(0, []) for _ in range(n)]
        for j, i in enumerate(chain):
            lists[i] = [[chain[(j + 1) % m]]]
        c = Case(f"hash{m}", "hash", 64, lists, enterpoint=chain[0], runs=((128, 10),), strides=(16, 0), hash_slots=HASH_SLOTS)
        c.chain = chain
        out.append(c)
    return out


@functools.lru_cache(maxsize=1)
def cases():
    return {c.name: c for c in layout_cases() + steered_cases() + hash_cases()}


NAMES = sorted(cases())
