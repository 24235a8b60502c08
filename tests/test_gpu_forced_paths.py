"""GPU: every partition path of the grouping at small row counts -- the
two-level histogram path for the first time.

csrc/dedup.hip group_layout picks the path (direct, 12-bit staged, two-level
over runs, two-level over a histogram) from the row count alone, so a test
reaches a path only by being big enough: 12.6 M rows for the run path, more
than 2^28 for the histogram one.  The structural edges of those paths -- tiles
shorter than a round, blocks with an empty tile, segments that receive nothing
or everything, a bucket past the LDS table, fine counters wrapping, the first
call on a workspace nobody wrote -- need 1..300 000 rows.  The test-only
overrides SDGPU_GROUP_BITS / SDGPU_GROUP_HIST (dedup.hip forced_plan) choose
the bucket bits and the two-level variant of a process; each configuration
runs in one fresh child on a poisoned workspace (SDGPU_POISON_WS, as
tests/test_gpu_poison.py), proves from the plan and from the kernel timer's
names that the forced path is the one that ran, and compares every result
bit-exactly with the oracle (file_identifier/mod.rs:136-333).
"""
import json
import os
import subprocess
import sys
import time

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_CHILD = r'''
import ctypes, json, sys, time
T0 = time.time()
sys.path.insert(0, sys.argv[1])
BITS, HIST, LARGE = int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4])
import numpy as np
import torch
from oracle import oracle as O
from spacedrive_amd import dedup
from spacedrive_amd._native import Context

ctx = Context(0)
ops = dedup.HipOps(ctx)
CB = BITS - 9 if BITS > 12 else 0            # coarse digit bits (kStage2Bits = 9)
ALL_ONES = np.uint64(2**64 - 1)
res = {"plan": [], "sig": {}, "counts": {}}
bad = res["counts"]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- the forced plan is what group_layout reports -----------------------------
gp = ctx.lib.sdgpu_group_plan
gp.restype = ctypes.c_int
gp.argtypes = [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int, ctypes.c_int,
               ctypes.POINTER(ctypes.c_uint64), ctypes.c_uint32]
for n in (1, 257, 70_001, 300_000, 17_000_000):
    for implicit in (0, 1):
        for bits_rows in (0, n // 3):
            w = (ctypes.c_uint64 * 43)()
            assert gp(n, bits_rows, implicit, 0, w, 43) == 43
            res["plan"].append([int(w[0]), int(w[4]), int(w[2])])  # bits, path, rec12


def mixed(rng, n):
    """80 % distinct keys, the all-ones key among them, 1 % keyless rows."""
    pool = rng.integers(0, 2**64 - 1, max(1, int(n * 0.8)), dtype=np.uint64, endpoint=True)
    pool[0] = ALL_ONES
    key = pool[rng.integers(0, pool.size, n)]
    has = (rng.random(n) > 0.01).astype(np.uint8)
    key[n // 2], has[n // 2] = ALL_ONES, 1
    return key, has


_seg0 = {}


def seg0_keys(rng, n):
    """Keys whose rows all fall in coarse segment 0: the top CB digit bits
    (the hash bits below the shard byte) are zero; at 12 bits, the top 4."""
    cb = CB or 4
    if cb not in _seg0:
        k = rng.integers(0, 2**64 - 1, 1 << 22, dtype=np.uint64, endpoint=True)
        _seg0[cb] = np.unique(k[(dedup.shard_of(k, 8 + cb) & ((1 << cb) - 1)) == 0])
    pool = _seg0[cb][:max(1, int(n * 0.8))]
    return pool[rng.integers(0, pool.size, n)], np.ones(n, np.uint8)


def rep_implicit(name, key, has, chunks=(100,)):
    """12-byte records from 12 bits on: rows without a rank array."""
    dk, dh = dev(key.view(np.int64)), dev(has)
    for ch in chunks:
        got = ops.group_rows(dk, dh, None, ch, 0).cpu().numpy().view(np.uint32)
        bad[f"{name}_implicit_c{ch}"] = int(np.count_nonzero(got != O.group_reps(key, has, ch)))


def rep_explicit(name, key, has, rng, chunks=(100,), permute=True):
    """16-byte records: a rank array, permuted; the oracle sees rank order."""
    n = key.size
    rank = rng.permutation(n).astype(np.uint32) if permute else np.arange(n, dtype=np.uint32)
    order = np.argsort(rank)
    dk, dh, dr = dev(key.view(np.int64)), dev(has), dev(rank.view(np.int32))
    for ch in chunks:
        got = ops.group_rows(dk, dh, dr, ch, 0).cpu().numpy().view(np.uint32)
        ref = O.group_reps(key[order], has[order], ch)  # positions in rank order = ranks
        bad[f"{name}_explicit_c{ch}"] = int(np.count_nonzero(got[order] != ref))


def ref_lists(key, has, first_rank, chunk):
    """The oracle's write set of rows with ranks first_rank + i: the chunk rule
    runs on global ranks, so the oracle sees first_rank keyless rows in front."""
    k = np.concatenate([np.zeros(first_rank, np.uint64), key])
    h = np.concatenate([np.zeros(first_rank, np.uint8), has])
    c, lr, lo = O.link_batch(O.group_reps(k, h, chunk), None, None, 0)
    return c[c >= first_rank], lr, lo


def same_lists(who, obj, ref):
    got = dedup.split_link_lists(who, obj)
    return int(not all(np.array_equal(g, r) for g, r in zip(got, ref)))


def fused(name, key, has, first_rank=0, chunk=100):
    """The fused write set: implicit ranks, its own keyless sink, no trim."""
    who, obj, cnt = dedup.group_link_device(dev(key.view(np.int64)), dev(has), None, None,
                                            first_rank, chunk, ctx=ctx, trim=False)
    torch.cuda.synchronize()
    c, l, e = (int(x) for x in cnt.cpu().tolist())
    ref = ref_lists(key, has, first_rank, chunk)
    ok = (c, l, e) == (ref[0].size, ref[1].size, ref[0].size + ref[1].size)
    bad[f"{name}_fused_b{first_rank}_c{chunk}"] = int(not ok) or same_lists(
        who[:e].cpu().numpy(), obj[:e].cpu().numpy(), ref)


def fused_explicit(name, key, has, rng, chunk=100):
    """The fused write set over a permuted rank array: 16-byte records."""
    rank = rng.permutation(key.size).astype(np.uint32)
    order = np.argsort(rank)
    who, obj, cnt = dedup.group_link_device(dev(key.view(np.int64)), dev(has), None,
                                            dev(rank.view(np.int32)), 0, chunk, ctx=ctx,
                                            trim=False)
    torch.cuda.synchronize()
    c, l, e = (int(x) for x in cnt.cpu().tolist())
    ref = O.link_batch(O.group_reps(key[order], has[order], chunk), None, None, 0)  # rank space
    ok = (c, l, e) == (ref[0].size, ref[1].size, ref[0].size + ref[1].size)
    bad[f"{name}_fused_explicit_c{chunk}"] = int(not ok) or same_lists(
        who[:e].cpu().numpy(), obj[:e].cpu().numpy(), ref)


def all_forms(name, key, has, rng):
    rep_implicit(name, key, has, chunks=(100, 1, 7))
    rep_explicit(name, key, has, rng, chunks=(100, 7))
    fused(name, key, has)
    fused(name, key, has, first_rank=1037, chunk=7)
    fused_explicit(name, key, has, rng)


# ---- the path that ran: the first call of the process, timed -------------------
rng = np.random.default_rng(1000 * BITS + HIST)
key, has = mixed(rng, 70_001)
dk, dh = dev(key.view(np.int64)), dev(has)
ctx.set_timing(True)
got = ops.group_rows(dk, dh, None, 100, 0)
torch.cuda.synchronize()
res["sig"]["implicit"] = sorted(ctx.kernel_times())
ctx.set_timing(True)  # resets the timer
rank = np.arange(70_001, dtype=np.uint32)
got16 = ops.group_rows(dk, dh, dev(rank.view(np.int32)), 100, 0)
torch.cuda.synchronize()
res["sig"]["explicit"] = sorted(ctx.kernel_times())
ctx.set_timing(False)
ref = O.group_reps(key, has, 100)
bad["first_call_implicit"] = int(np.count_nonzero(got.cpu().numpy().view(np.uint32) != ref))
bad["first_call_explicit"] = int(np.count_nonzero(got16.cpu().numpy().view(np.uint32) != ref))

# ---- every form's FIRST call on a workspace nobody wrote ---------------------------
# (a workspace is poisoned when it is allocated: a context of its own per form,
# or the earlier forms' values would still lie in it)
main_ctx, main_ops = ctx, ops
for n in (257, 70_001):
    key, has = mixed(rng, n)
    for form in (lambda: rep_explicit(f"fresh_{n}", key, has, rng),
                 lambda: fused(f"fresh_{n}", key, has),
                 lambda: fused(f"fresh_{n}", key, has, first_rank=1037, chunk=7)):
        ctx = Context(0)
        ops = dedup.HipOps(ctx)
        form()
        torch.cuda.synchronize()
        ctx.close()
ctx, ops = main_ctx, main_ops

# ---- row counts x keys x forms ---------------------------------------------------
for n in (1, 255, 256, 257, 4097, 70_001, 300_000):
    key, has = mixed(rng, n)
    all_forms(f"mixed_{n}", key, has, rng)
    # one key on every row: one segment takes everything, the bucket is global
    key = np.full(n, rng.integers(1, 2**63, dtype=np.uint64), np.uint64)
    all_forms(f"same_{n}", key, np.ones(n, np.uint8), rng)
    # no keyed row at all
    all_forms(f"keyless_{n}", key, np.zeros(n, np.uint8), rng)
    # every row in coarse segment 0
    key, has = seg0_keys(rng, n)
    all_forms(f"seg0_{n}", key, has, rng)

n = 300_000
base_key, base_has = mixed(rng, n)
hot = np.uint64(0x1234_5678_9ABC_DEF1)


def repeats(m):
    """One key on rows 0..m-1: m rows of one final bucket in the first
    1172-row tile (8-bit fine counters of the 12-byte coarse pass wrap at 256)."""
    k, h = base_key.copy(), base_has.copy()
    k[:m], h[:m] = hot, 1
    return k, h


for tag, m in (("a", 300), ("b", 0), ("c", 255), ("d", 256), ("e", 300)):
    # 300 wraps; 0 must find the flag reset; 255 / 256: at the wrap; 300 again
    k, h = repeats(m)
    rep_implicit(f"repeat{m}{tag}", k, h)
    rep_explicit(f"repeat{m}{tag}", k, h, rng)
    fused(f"repeat{m}{tag}", k, h)
# one key on 20 000 random rows: a global-table bucket among ~9-row buckets
k, h = base_key.copy(), base_has.copy()
at = rng.choice(n, 20_000, replace=False)
k[at], h[at] = hot, 1
all_forms("hot20000", k, h, rng)

# ---- two batches through an Object index ----------------------------------------
for n in (257, 70_001):
    key, has = mixed(rng, n)
    ref = O.group_reps(key, has, 100)
    rank = np.arange(n, dtype=np.uint32)
    dk, dh, dr = dev(key.view(np.int64)), dev(has), dev(rank.view(np.int32))
    idx = dedup.ObjectIndex(ctx)
    parts = [dedup.group_rows_indexed(dk[a:b], dh[a:b], dr[a:b], idx, 100).cpu().numpy()
             for a, b in ((0, n // 3), (n // 3, n))]
    bad[f"index_{n}"] = int(np.count_nonzero(np.concatenate(parts).view(np.uint32) != ref))
    idx.close()

# ---- the padded exchange through a one-rank communicator -------------------------
# (RecIn / RecRankIn inputs, the moved keyless sink, the bits_rows hint)
for n in (257, 70_001, 300_000):
    key, has = mixed(rng, n)
    ref = O.group_reps(key, has, 100)
    rank = np.arange(n, dtype=np.uint32)
    dk, dh, dr = dev(key.view(np.int64)), dev(has), dev(rank.view(np.int32))
    comm = dedup.Comm.init_rank(ctx, 1, 0, dedup.Comm.unique_id())
    comm.set_exchange(dedup.EXCHANGE_PADDED, n)
    got = dedup.group_sharded(dk, dh, dr, comm, None, 100).cpu().numpy().view(np.uint32)
    bad[f"padded_rep_{n}"] = int(np.count_nonzero(got != ref))
    idx = dedup.ObjectIndex(ctx)
    parts = [dedup.group_sharded(dk[a:b], dh[a:b], dr[a:b], comm, idx, 100).cpu().numpy()
             for a, b in ((0, n // 2), (n // 2, n))]
    bad[f"padded_index_{n}"] = int(np.count_nonzero(np.concatenate(parts).view(np.uint32) != ref))
    who, obj, (c, l) = dedup.group_link_sharded(dk, dh, None, dr, comm, 100)
    bad[f"padded_write_set_{n}"] = same_lists(who.cpu().numpy(), obj.cpu().numpy(),
                                              O.link_batch(ref, None, None, 0))
    idx.close()
    comm.close()

# ---- 16-bit fine counters of the histogram path's coarse pass --------------------
if LARGE:
    # a tile is n / 256 rows and k_part_scatter_runs counts in 16 bits whatever
    # the record size: 66 000 rows of one key in the first 66 407-row tile wrap
    # a counter, so k_fine_recount rebuilds the counts from the records
    n = 17_000_000
    key = rng.integers(0, 2**64 - 1, n, dtype=np.uint64, endpoint=True)
    key[:66_000] = hot
    has = np.ones(n, np.uint8)
    ref = O.group_reps(key, has, 100)
    dk, dh = dev(key.view(np.int64)), dev(has)
    dr = torch.arange(n, dtype=torch.int32, device="cuda")
    for call in (1, 2):
        got = ops.group_rows(dk, dh, dr, 100, 0).cpu().numpy().view(np.uint32)
        bad[f"large_recount_call{call}"] = int(np.count_nonzero(got != ref))

res["secs"] = round(time.time() - T0, 2)
print(json.dumps(res), flush=True)
'''

# kernel timer names (dedup.hip KScope) of one rep call, per path
_SIGNATURE = {
    "staged12": {"bucket_hist", "bucket_scatter", "bucket_group"},
    "runs": {"bucket_scatter1", "bucket_fine_scan", "bucket_scatter", "bucket_group"},
    "hist": {"bucket_hist", "bucket_scatter1", "bucket_fine_scan", "bucket_scatter",
             "bucket_group"},
}

CONFIGS = [(12, 0, 0), (13, 0, 0), (15, 0, 0), (13, 1, 1), (15, 1, 0), (14, 1, 0)]


@pytest.mark.parametrize("bits,hist,large", CONFIGS,
                         ids=[f"bits{b}" + ("_hist" if h else "") for b, h, _ in CONFIGS])
def test_forced_path_vs_oracle(bits, hist, large):
    env = dict(os.environ, SDGPU_POISON_WS="1", SDGPU_GROUP_BITS=str(bits))
    env.pop("SDGPU_GROUP_HIST", None)
    if hist:
        env["SDGPU_GROUP_HIST"] = "1"
    t0 = time.time()
    p = subprocess.run([sys.executable, "-c", _CHILD, ROOT, str(bits), str(hist), str(large)],
                       capture_output=True, text=True, timeout=400 if large else 240, env=env)
    wall = time.time() - t0
    assert p.returncode == 0, p.stderr[-3000:]
    res = json.loads(p.stdout.strip().splitlines()[-1])
    kind = "staged12" if bits == 12 else ("hist" if hist else "runs")
    print(f"\nforced bits={bits} hist={hist}: signature {res['sig']}, child {res['secs']} s, "
          f"wall {wall:.1f} s, {len(res['counts'])} cases")
    # the forced plan: bits and path for every call, 12-byte records iff implicit
    path = {"staged12": 1, "runs": 2, "hist": 3}[kind]
    assert res["plan"] and all(pl[:2] == [bits, path] for pl in res["plan"]), res["plan"]
    # the path that ran, for both record sizes: not vacuous
    for form in ("implicit", "explicit"):
        ran = {k for k in res["sig"][form] if k.startswith("bucket_")}
        assert ran == _SIGNATURE[kind], (form, res["sig"])
    wrong = {k: v for k, v in res["counts"].items() if v != 0}
    assert len(res["counts"]) > 200 and not wrong, wrong
    if large:
        assert {"large_recount_call1", "large_recount_call2"} <= set(res["counts"])
