"""Shared by test_live_sequences_cpu.py and test_gpu_live_sequences.py: the random update sequences of
tests/golden/updates_seq_<name>.npz (tests/golden/make_golden_updates.py: seeded legal operation lists run through the compiled
reference, the SHA-256 of its saved file after every operation, its search results at the checkpoints, its own account of every
operation) and their start graphs."""
import hashlib
import importlib.util
import os

import numpy as np

from hsutil import GOLDEN

ADD, MARK, UNMARK, RESIZE = 0, 1, 2, 3
GOLDEN_START = {"G1": "l2_int_d16", "G1off": "l2_int_d16", "G2": "l2_cont_d32", "G3": "l2_int_d16_del", "G4": "l2_cont_d32_del"}
NAMES = ["G1", "G1off", "G2", "G3", "G4", "W32", "W128", "W320", "W960", "T"]
DIMS = {"G1": 16, "G1off": 16, "G2": 32, "G3": 16, "G4": 32, "W32": 32, "W128": 128, "W320": 320, "W960": 960, "T": 32}
INTEGER = [n for n in NAMES if n not in ("G2", "G4")]     # rows the u8 / fp16 formats hold exactly


def generator():
    """tests/golden/make_golden_updates.py as a module: its coverage() and needed() are what picked the fixtures' seeds."""
    spec = importlib.util.spec_from_file_location("make_golden_updates", os.path.join(GOLDEN, "make_golden_updates.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def sha(data):
    return hashlib.sha256(data).digest()


def file_sha(path):
    with open(path, "rb") as f:
        return sha(f.read())


class Sequence:
    def __init__(self, name):
        f = np.load(os.path.join(GOLDEN, f"updates_seq_{name}.npz"))
        self.name, self.f, self.dim = name, f, DIMS[name]
        self.ops = f["ops"]
        self.rows = np.ascontiguousarray(f["rows"], np.float32)       # (the W / T fixtures store uint8)
        self.cap, self.allow = int(f["max_elements"]), bool(f["allow"])
        self.checkpoints = [int(c) for c in f["checkpoints"]]
        self.k, self.efs = int(f["k"]), [int(e) for e in f["efs"]]
        if name in GOLDEN_START:
            self.queries = np.ascontiguousarray(np.load(os.path.join(GOLDEN, GOLDEN_START[name].replace("_del", "") + ".npz"))["queries"], np.float32)
        else:
            self.queries = np.ascontiguousarray(f["queries"], np.float32)
        for a in (self.ops, self.rows, self.queries):
            a.setflags(write=False)

    def digest(self, c):
        """The reference's digest after the first c operations."""
        return (self.f["digest"][c - 1] if c else self.f["start_digest"]).tobytes()

    def reference(self, c, ef):
        return {key: self.f[f"cp{c}_ef{ef}_{key}"] for key in ("dists", "labels", "cnt", "calls")}


_seqs, _starts = {}, {}


def sequence(name):
    if name not in _seqs:
        _seqs[name] = Sequence(name)
    return _seqs[name]


def start_file(hs, name, tmp_path_factory):
    """The start graph's file, with the fixture's digest: a golden file, or built here as the reference built it."""
    if name not in _starts:
        s = sequence(name)
        if name in GOLDEN_START:
            path = os.path.join(GOLDEN, GOLDEN_START[name] + ".hnsw.bin")
        else:
            path = str(tmp_path_factory.mktemp(f"seq_{name}") / "start.bin")
            hs.build_hnsw(np.ascontiguousarray(s.f["base"], np.float32), path, M=int(s.f["M"]), ef_construction=int(s.f["efC"]),
                          branching_factor="4", seed=100, threads=1)
        assert file_sha(path) == s.digest(0), f"{name}: the start graph is not the reference's"
        _starts[name] = path
    return _starts[name]


def pq_sorted(d, l, c):
    return [sorted(zip(d[i, :int(c[i])].view(np.uint32).tolist(), l[i, :int(c[i])].tolist())) for i in range(len(c))]
