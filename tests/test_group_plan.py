"""CPU: the plan of a grouping call (csrc/dedup.hip group_layout) -- bucket
bits, partition path, record size, coarse rounds and the workspace arrays --
read through sdgpu_group_plan (csrc/internal.hpp), which touches no device.

Checked against a model written here from the rules dedup.hip states
(kBucketRows rows per bucket, 12 bits staged, two-level above, runs while a
second-pass block's run list holds them), for the production choice and for
the test-only overrides SDGPU_GROUP_BITS / SDGPU_GROUP_HIST.  The overrides
are read once per process, so every forced plan is computed by a child.
"""
import ctypes
import json
import os
import re
import subprocess
import sys

import pytest

from spacedrive_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spacedrive_amd", "csrc")

DIRECT, STAGED12, RUNS, HIST = 0, 1, 2, 3
ARRAYS = ["hist", "tiles", "rec", "hist1", "rec1", "gkey", "gmin", "fine", "fE", "ftot", "fbase",
          "ovf", "run_s", "run_l", "segtot", "lcnt", "xst", "xcnt"]
HEAD = 7
WORDS = HEAD + 2 * len(ARRAYS)

# the row counts on either side of a change of path (tests/test_gpu_dedup.py)
PATH_EDGES = [3073 * 2**11 - 1, 3073 * 2**11, 3073 * 2**12 - 1, 3073 * 2**12]
GRID_N = ([1, 255, 256, 257] +
          [3073 * 2**k + d for k in (1, 10, 11, 12, 14) for d in (-1, 1)] +
          [2**28 - 1, 2**28 + 1, 2**31])


def _const(header, name):
    text = open(os.path.join(CSRC, header)).read()
    m = re.search(r"constexpr\s+\w+\s+" + name + r"\s*=\s*(\d+)", text)
    assert m, (header, name)
    return int(m.group(1))


K_PART_BLOCKS = _const("part_device.hpp", "kPartBlocks")
K_RUN_MAX_BINS = _const("bucket_part_device.hpp", "kRunMaxBins")
K_MAX_RUNS = _const("bucket_part_device.hpp", "kMaxRuns")
K_MAX_BITS = _const("bucket_part_device.hpp", "kMaxBucketBits")
K_STAGE_BITS = _const("bucket_part_device.hpp", "kStageBits")
K_STAGE2_BITS = _const("bucket_part_device.hpp", "kStage2Bits")
K_STAGE2_BLOCKS = _const("bucket_part_device.hpp", "kStage2Blocks")
K_PART_THREADS = _const("part_device.hpp", "kPartThreads")
K_BUCKET_ROWS = 3072  # dedup.hip kBucketRows (a uint64_t constant with a comment)


def _decode(words):
    p = dict(zip(("bits", "cbits", "rec12", "rounds", "path", "total", "ws_bytes"), words[:HEAD]))
    p["arrays"] = {a: (words[HEAD + 2 * i], words[HEAD + 1 + 2 * i]) for i, a in enumerate(ARRAYS)}
    return p


def plan(n, bits_rows=0, implicit=False, with_sink=False):
    lib = _native.load()
    f = lib.sdgpu_group_plan
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int, ctypes.c_int,
                  ctypes.POINTER(ctypes.c_uint64), ctypes.c_uint32]
    out = (ctypes.c_uint64 * WORDS)()
    assert f(n, bits_rows, int(implicit), int(with_sink), out, WORDS) == WORDS
    return _decode(list(out))


# ---- the model ----------------------------------------------------------------

def model_bits(n, bits_rows=0):
    rows = bits_rows if bits_rows and bits_rows < n else n
    bits = 1
    while bits < K_MAX_BITS and (rows >> bits) > K_BUCKET_ROWS:
        bits += 1
    return bits


def model(n, implicit, bits, hist=False):
    """(cbits, rec12, rounds, path) that follow from the bucket bits."""
    cbits = bits - K_STAGE2_BITS if bits > K_STAGE_BITS else 0
    rec12 = implicit and bits >= K_STAGE_BITS
    tile = -(-n // K_PART_BLOCKS) if cbits else 0
    per_round = (8 if rec12 else 4) * K_PART_THREADS  # k_part_private: priv_round
    rounds = -(-tile // per_round)
    if bits < K_STAGE_BITS:
        path = DIRECT
    elif not cbits:
        path = STAGED12
    elif (K_PART_BLOCKS // K_STAGE2_BLOCKS) * rounds <= K_MAX_RUNS and not hist:
        path = RUNS
    else:
        path = HIST
    return cbits, rec12, rounds, path


def check_layout(p, n, where):
    """Aligned, pairwise disjoint, inside total, total within what a caller
    allocates, and a run table for the rounds the kernels are given."""
    spans = sorted((off, size, a) for a, (off, size) in p["arrays"].items() if size)
    for off, size, a in spans:
        assert off % 256 == 0, (where, a, off)
        assert off + size <= p["total"], (where, a)
    for (o0, s0, a0), (o1, _, a1) in zip(spans, spans[1:]):
        assert o0 + s0 <= o1, (where, a0, a1)
    for a, (off, size) in p["arrays"].items():
        assert off % 256 == 0 and off <= p["total"], (where, a)
    assert p["total"] <= p["ws_bytes"], (where, p["total"], p["ws_bytes"])
    # every array the two passes index by row, bucket or block holds its rows
    assert p["arrays"]["rec"][1] >= 16 * n, where
    nf = 1 << p["bits"]
    for a in ("fine", "fE"):
        assert p["arrays"][a][1] >= 4 * nf * K_PART_BLOCKS, (where, a)
    assert p["arrays"]["ftot"][1] >= 4 * nf and p["arrays"]["fbase"][1] >= 4 * (nf + 1), where
    assert p["arrays"]["lcnt"][1] >= 4 * (nf + 1), where
    if p["cbits"]:
        assert p["arrays"]["rec1"][1] >= 16 * n, where
        assert p["arrays"]["hist1"][1] >= 4 * ((K_PART_BLOCKS << p["cbits"]) + 1), where
        assert p["rounds"] >= 1, where
    need = 4 * K_PART_BLOCKS * p["rounds"] * K_RUN_MAX_BINS
    for a in ("run_s", "run_l"):
        assert p["arrays"][a][1] >= need, (where, a, p["arrays"][a][1], need)
    assert p["arrays"]["segtot"][1] >= 4 * K_RUN_MAX_BINS, where


def grid():
    for n in GRID_N:
        for implicit in (False, True):
            for with_sink in (False, True):
                for bits_rows in (0, n // 3, n):
                    yield n, bits_rows, implicit, with_sink


# ---- nothing forced -----------------------------------------------------------

def test_plan_rejects_bad_arguments():
    lib = _native.load()
    plan(1)  # sets the prototype
    out = (ctypes.c_uint64 * WORDS)()
    assert lib.sdgpu_group_plan(0, 0, 0, 0, out, WORDS) == -22
    assert lib.sdgpu_group_plan(1, 0, 0, 0, None, WORDS) == -22
    assert lib.sdgpu_group_plan(1, 0, 0, 0, out, WORDS - 1) == -22


def test_plan_is_not_part_of_the_c_abi():
    assert "sdgpu_group_plan" not in _native.declared_symbols()


def test_paths_at_the_path_edges():
    want = [(11, DIRECT), (12, STAGED12), (12, STAGED12), (13, RUNS)]
    for n, (bits, path) in zip(PATH_EDGES, want):
        for implicit in (False, True):
            p = plan(n, implicit=implicit)
            assert (p["bits"], p["path"]) == (bits, path), (n, implicit, p)
            assert p["cbits"] == (4 if bits == 13 else 0)


def test_histogram_path_begins_where_the_run_list_ends():
    # 16-byte records: 4096-row rounds, 2 coarse blocks per second-pass block
    assert plan(2**28)["path"] == RUNS and plan(2**28)["rounds"] == 256
    assert plan(2**28 + 1)["path"] == HIST
    # 12-byte records: 8192-row rounds
    assert plan(2**29, implicit=True)["path"] == RUNS
    assert plan(2**29, implicit=True)["rounds"] == 256
    assert plan(2**29 + 1, implicit=True)["path"] == HIST
    assert plan(2**28 + 1, implicit=True)["path"] == RUNS


def test_rec12_only_from_12_bits_with_implicit_ranks():
    for n in GRID_N + PATH_EDGES:
        for implicit in (False, True):
            p = plan(n, implicit=implicit)
            assert p["rec12"] == int(implicit and p["bits"] >= 12), (n, implicit, p)


def test_bits_rows_lowers_the_bits_and_never_raises_them():
    for n in GRID_N + PATH_EDGES:
        full = plan(n)["bits"]
        assert full == model_bits(n)
        for br in (1, n // 1000, n // 3, n - 1, n, n + 1, 4 * n):
            if br <= 0:
                continue
            got = plan(n, bits_rows=br)["bits"]
            assert got == model_bits(n, br) and got <= full, (n, br, got, full)
    assert plan(3073 * 2**12, bits_rows=3073 * 2**11)["path"] == STAGED12
    assert plan(3073 * 2**12, bits_rows=1000)["path"] == DIRECT


def test_layout_over_the_grid():
    for n, bits_rows, implicit, with_sink in grid():
        where = (n, bits_rows, implicit, with_sink)
        p = plan(n, bits_rows, implicit, with_sink)
        assert p["bits"] == model_bits(n, bits_rows), where
        assert (p["cbits"], p["rec12"], p["rounds"], p["path"]) == \
            tuple(int(x) for x in model(n, implicit, p["bits"])), (where, p)
        check_layout(p, n, where)
        assert bool(p["arrays"]["xst"][1]) == with_sink and bool(p["arrays"]["xcnt"][1]) == with_sink


# ---- the overrides (static reads: one child per setting) ------------------------

_CHILD = r'''
import ctypes, json, sys
lib = ctypes.CDLL(sys.argv[1])
f = lib.sdgpu_group_plan
f.restype = ctypes.c_int
f.argtypes = [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int, ctypes.c_int,
              ctypes.POINTER(ctypes.c_uint64), ctypes.c_uint32]
W = int(sys.argv[2])
res = []
for case in json.loads(sys.argv[3]):
    out = (ctypes.c_uint64 * W)()
    assert f(*case, out, W) == W
    res.append(list(out))
print(json.dumps(res))
'''


def child_plans(env_extra):
    cases = [[n, br, int(i), int(s)] for n, br, i, s in grid()]
    env = {k: v for k, v in os.environ.items() if not k.startswith("SDGPU_GROUP_")}
    env.update(env_extra)
    r = subprocess.run([sys.executable, "-c", _CHILD, _native.LIB_PATH, str(WORDS),
                        json.dumps(cases)], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    return [(tuple(c), _decode(w)) for c, w in zip(cases, json.loads(r.stdout))]


@pytest.mark.parametrize("bits", [1, 11, 12, 13, 14, 15])
@pytest.mark.parametrize("hist", [False, True])
def test_forced_bits_and_histogram(bits, hist):
    env = {"SDGPU_GROUP_BITS": str(bits)}
    if hist:
        env["SDGPU_GROUP_HIST"] = "1"
    for (n, bits_rows, implicit, with_sink), p in child_plans(env):
        where = (bits, hist, n, bits_rows, implicit, with_sink)
        assert p["bits"] == bits, where
        assert (p["cbits"], p["rec12"], p["rounds"], p["path"]) == \
            tuple(int(x) for x in model(n, implicit, bits, hist)), (where, p)
        if bits > 12 and hist:
            assert p["path"] == HIST, where
        check_layout(p, n, where)


def test_histogram_flag_alone_changes_two_level_calls_only():
    for (n, bits_rows, implicit, with_sink), p in child_plans({"SDGPU_GROUP_HIST": "1"}):
        bits = model_bits(n, bits_rows)
        assert p["bits"] == bits
        assert p["path"] == model(n, implicit, bits, True)[3]
        assert (p["path"] == HIST) == (bits > 12)
        check_layout(p, n, (n, bits_rows, implicit, with_sink))


@pytest.mark.parametrize("env", [{"SDGPU_GROUP_BITS": "0"}, {"SDGPU_GROUP_BITS": "16"},
                                 {"SDGPU_GROUP_BITS": "-3"}, {"SDGPU_GROUP_BITS": "abc"},
                                 {"SDGPU_GROUP_BITS": "13x"}, {"SDGPU_GROUP_BITS": ""},
                                 {"SDGPU_GROUP_HIST": "0"}, {"SDGPU_GROUP_HIST": "2"},
                                 {"SDGPU_GROUP_HIST": "11"}])
def test_out_of_range_overrides_are_ignored(env):
    for (n, bits_rows, implicit, with_sink), p in child_plans(env):
        q = plan(n, bits_rows, implicit, with_sink)  # this process: nothing forced
        assert p == q, (env, n, bits_rows, implicit, with_sink)
