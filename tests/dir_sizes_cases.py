"""Inputs of the directory-size call (numpy only, no GPU): rows of a location
as (materialized_path, name, is_dir, size) turned into the call's columns, and
the shapes tests/test_gpu_dir_sizes.py runs.  Keys here are BLAKE2b-64 of the
path strings (any injective 64-bit key does: the call only compares keys);
the end-to-end test uses the product's own keys."""
from __future__ import annotations

import hashlib

import numpy as np

MISS = 0xFFFFFFFF
U = 0xFFFFFFFFFFFFFFFF
F = 0xFFFFFFFF


def key_of(path: str) -> int:
    return int.from_bytes(hashlib.blake2b(path.encode(), digest_size=8).digest(), "little")


def columns(rows, key=key_of):
    """rows: [(materialized_path, name, is_dir, size)] in id order ->
    (dirkey, selfkey, flags, size) as uint64 / uint8 arrays."""
    dirkey = np.array([key(mp) for mp, _, _, _ in rows], np.uint64)
    selfkey = np.array([key(mp + nm + "/") if d else 0 for mp, nm, d, _ in rows], np.uint64)
    flags = np.array([1 if d else 0 for _, _, d, _ in rows], np.uint8)
    size = np.array([0 if d else s for _, _, d, s in rows], np.uint64)
    return dirkey, selfkey, flags, size


def chain(depth=70):
    """One file at the bottom of `depth` nested directories."""
    rows, mp = [], "/"
    for k in range(depth):
        rows.append((mp, "d%d" % k, True, 0))
        mp += "d%d/" % k
    rows.append((mp, "leaf.bin", False, 12345))
    return rows


def star(files=5000):
    """One directory holding `files` files of size 2^33 + i."""
    return [("/", "hub", True, 0)] + [("/hub/", "f%d" % i, False, (1 << 33) + i)
                                      for i in range(files)]


def star_alternating(files=3000):
    """`files` files alternating between two directories."""
    rows = [("/", "a", True, 0), ("/", "b", True, 0)]
    return rows + [("/" + "ab"[i & 1] + "/", "f%d" % i, False, 1000 + i) for i in range(files)]


def bushy(seed=5):
    """300 directories x 3 files under 20 directories under 2, ids shuffled:
    children before parents, siblings scattered."""
    rng = np.random.default_rng(seed)
    rows = [("/", "t0", True, 0), ("/", "t1", True, 0)]
    for m in range(20):
        top = "/t%d/" % (m % 2)
        rows.append((top, "m%d" % m, True, 0))
        for l in range(15):
            mid = top + "m%d/" % m
            rows.append((mid, "l%d" % l, True, 0))
            for f in range(3):
                rows.append((mid + "l%d/" % l, "f%d.dat" % f, False,
                             int(rng.integers(1, 1 << 40))))
    order = rng.permutation(len(rows))
    return [rows[i] for i in order]


def empty_directories():
    rows = [("/", "e%d" % i, True, 0) for i in range(40)]
    return rows + [("/e%d/" % i, "inner", True, 0) for i in range(0, 40, 3)]


# ---- the malformed inputs, with the answer written out by hand -----------------------
KA, KS, KX, KY, KZ, KQ, KROOT = 11, 22, 33, 44, 55, 66, 77


def malformed():
    """(dirkey, selfkey, flags, size), (parent, total, files, counts).
    row  0 dir  A            top level, owns the key KA
         1 dir  A'           the same self key: has no children
         2 file in A         10 bytes
         3 dir  S            its own parent
         4 file in S         5 bytes
         5 dir  X            child of Y   } a two-cycle
         6 dir  Y            child of X   }
         7 dir  Z            hangs below X: resolved, the cycle absorbs it
         8 file in Z         7 bytes
         9 file              its directory row is absent, 100 bytes
        10 file in Y         3 bytes"""
    dirkey = np.array([KROOT, KROOT, KA, KS, KS, KY, KX, KX, KZ, KQ, KY], np.uint64)
    selfkey = np.array([KA, KA, 0, KS, 0, KX, KY, KZ, 0, 0, 0], np.uint64)
    flags = np.array([1, 1, 0, 1, 0, 1, 1, 1, 0, 0, 0], np.uint8)
    size = np.array([0, 0, 10, 0, 5, 0, 0, 0, 7, 100, 3], np.uint64)
    parent = np.array([MISS, MISS, 0, 3, 3, 6, 5, 5, 7, MISS, 6], np.uint32)
    total = np.array([10, 0, 10, U, 5, U, U, 7, 7, 100, 3], np.uint64)
    files = np.array([1, 0, 0, F, 0, F, F, 1, 0, 0, 0], np.uint32)
    counts = np.array([6, 3, 3, 110], np.uint64)
    return (dirkey, selfkey, flags, size), (parent, total, files, counts)


# ---- self keys that share table slots -------------------------------------------------
def chosen_self_keys(kind, n_keys, specials, seed=0):
    """Directory rows whose self keys are a scenario of tests/hash_keys.py (one
    home slot at the table's end, or clusters that straddle it; with `specials`
    the keys 0 and ~0 too), in a table of 2 x (directory rows) slots rounded up
    to a power of two.  Every second directory is a child of the directory
    before it; every directory holds two files; further files name the
    scenario's absent keys, so their walks run through the clusters and find
    nothing.  Returns the columns and the scenario."""
    from tests import hash_keys as H
    sc = H.table_scenario(kind, n_keys, specials, False, H.cap_join, seed)
    rng = np.random.default_rng([seed, n_keys, 9])
    keys = sc.keys
    nd = keys.size
    root = H.keys_at(sc.cap, sc.cap // 2 + 7, 1, rng)[0]
    assert root not in set(keys.tolist()) and H.cap_join(nd) == sc.cap
    dirkey, selfkey, flags, size = [], [], [], []
    for k in range(nd):
        dirkey.append(int(keys[k - 1]) if k & 1 else int(root))
        selfkey.append(int(keys[k]))
        flags.append(1)
        size.append(0)
    for k in rng.permutation(nd).tolist():
        for f in range(2):
            dirkey.append(int(keys[k]))
            selfkey.append(0)
            flags.append(0)
            size.append(1 + 3 * k + f)
    for a in sc.absent.tolist():
        dirkey.append(a)
        selfkey.append(0)
        flags.append(0)
        size.append(1 << 20)
    cols = (np.array(dirkey, np.uint64), np.array(selfkey, np.uint64), np.array(flags, np.uint8),
            np.array(size, np.uint64))
    return cols, sc
