"""GPU: the grouping on keys with CHOSEN hashes (tests/hash_keys.py), under the
default plan and forced bucket bits 6, 12, 13 and 15 (one fresh child each, as
tests/test_gpu_forced_paths.py: SDGPU_GROUP_BITS, SDGPU_POISON_WS), through the
rep API (implicit and permuted explicit ranks), the fused write set and the
link batch, every result against oracle.group_reps / link_batch:

* one-bit families: 65 keys whose hashes differ from a base in exactly one
  bit must stay 65 groups -- the packed word's key field (kb, lowm), the 12-
  and 16-byte records;
* 512 keys that share bucket, first LDS slot and probe step, at the last slot
  with the largest step and at slot 0 with step 1: chains of 512, next_slot's
  wrap, the 16-bit offset wrap; with 10 rows each the bucket takes the global
  table, where the 512 keys share one home slot;
* the key whose HASH is ~0 (bucket records carry the hash, so this key, not
  the key ~0, reaches K5's `k == kEmpty` / special_min branch), alone, with
  the key ~0, past the LDS capacity, with and without keyless rows;
* digits 0 and 2^bits - 1;
* owner boundaries of the exchange (shard bytes 84..86, 127 | 128, 170 | 171,
  255) through peer contexts on one GPU, world 2 and 3.

Why the probe loops end on these inputs: the LDS tables hold at most 4608 of
6144 and 4093 of 8192 slots, the double-hashing steps are coprime with 6144
(1 + 6 k) and odd for 8192, so a sequence visits every slot and meets an empty
one; the global table has 2m < tsize <= 4m slots for m records with a masked
step of 1, and its second loop looks for a key the first loop stored."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from oracle import oracle as O
from tests import hash_keys as HK

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_CHILD = r'''
import ctypes, json, sys, time
T0 = time.time()
sys.path.insert(0, sys.argv[1])
BITS = int(sys.argv[2])
import numpy as np
import torch
from oracle import oracle as O
from spacedrive_amd import dedup
from spacedrive_amd._native import Context
from tests import hash_keys as HK

ctx = Context(0)
ops = dedup.HipOps(ctx)
M64 = HK.M64
KS = np.uint64(HK.KEY_HASH_ALL_ONES)       # the key whose hash is ~0
res = {"plan": [], "counts": {}, "rows": {}}
bad = res["counts"]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


gp = ctx.lib.sdgpu_group_plan
gp.restype = ctypes.c_int
gp.argtypes = [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int, ctypes.c_int,
               ctypes.POINTER(ctypes.c_uint64), ctypes.c_uint32]
for n in (1500, 70_000):
    w = (ctypes.c_uint64 * 43)()
    assert gp(n, 0, 1, 0, w, 43) == 43
    res["plan"].append([n, int(w[0])])


def rep_implicit(name, key, has, chunks):
    dk, dh = dev(key.view(np.int64)), dev(has)
    out = {}
    for ch in chunks:
        t = ops.group_rows(dk, dh, None, ch, 0)
        got = t.cpu().numpy().view(np.uint32)
        ref = O.group_reps(key, has, ch)
        bad[f"{name}_implicit_c{ch}"] = int(np.count_nonzero(got != ref))
        # the link batch over the device's rep
        c, lr, lo = (x.cpu().numpy().view(np.uint32)
                     for x in dedup.link_batch_device(t, None, dh, 0, ctx=ctx))
        rc, rlr, rlo = O.link_batch(ref, None, has, 0)
        bad[f"{name}_linkbatch_c{ch}"] = int(not (np.array_equal(c, rc) and np.array_equal(lr, rlr)
                                                  and np.array_equal(lo, rlo)))
        out[ch] = got
    return out


def rep_explicit(name, key, has, rng, ch=100):
    n = key.size
    rank = rng.permutation(n).astype(np.uint32)
    order = np.argsort(rank)
    got = ops.group_rows(dev(key.view(np.int64)), dev(has), dev(rank.view(np.int32)), ch,
                         0).cpu().numpy().view(np.uint32)
    ref = O.group_reps(key[order], has[order], ch)
    bad[f"{name}_explicit_c{ch}"] = int(np.count_nonzero(got[order] != ref))


def ref_lists(key, has, first_rank, chunk):
    k = np.concatenate([np.zeros(first_rank, np.uint64), key])
    h = np.concatenate([np.zeros(first_rank, np.uint8), has])
    c, lr, lo = O.link_batch(O.group_reps(k, h, chunk), None, None, 0)
    return c[c >= first_rank], lr, lo


def same_lists(who, obj, ref):
    got = dedup.split_link_lists(who, obj)
    return int(not all(np.array_equal(g, r) for g, r in zip(got, ref)))


def fused(name, key, has, first_rank=0, chunk=100):
    who, obj, cnt = dedup.group_link_device(dev(key.view(np.int64)), dev(has), None, None,
                                            first_rank, chunk, ctx=ctx, trim=False)
    torch.cuda.synchronize()
    c, l, e = (int(x) for x in cnt.cpu().tolist())
    ref = ref_lists(key, has, first_rank, chunk)
    ok = (c, l, e) == (ref[0].size, ref[1].size, ref[0].size + ref[1].size)
    bad[f"{name}_fused_b{first_rank}_c{chunk}"] = int(not ok) or same_lists(
        who[:e].cpu().numpy(), obj[:e].cpu().numpy(), ref)


def fused_explicit(name, key, has, rng, chunk=100):
    rank = rng.permutation(key.size).astype(np.uint32)
    order = np.argsort(rank)
    who, obj, cnt = dedup.group_link_device(dev(key.view(np.int64)), dev(has), None,
                                            dev(rank.view(np.int32)), 0, chunk, ctx=ctx,
                                            trim=False)
    torch.cuda.synchronize()
    c, l, e = (int(x) for x in cnt.cpu().tolist())
    ref = O.link_batch(O.group_reps(key[order], has[order], chunk), None, None, 0)
    ok = (c, l, e) == (ref[0].size, ref[1].size, ref[0].size + ref[1].size)
    bad[f"{name}_fused_explicit_c{chunk}"] = int(not ok) or same_lists(
        who[:e].cpu().numpy(), obj[:e].cpu().numpy(), ref)


def all_forms(name, key, has, rng, groups_of=None):
    """groups_of: keys that must be exactly that many groups.  With chunks of
    one row every later row of a key links to its first, so the distinct reps
    over those keys' rows count the groups the kernel formed."""
    assert key.size < 70_000
    res["rows"][name] = int(key.size)
    got = rep_implicit(name, key, has, (100, 1))
    if groups_of is not None:
        rows = np.isin(key, groups_of) & (has != 0)
        bad[f"{name}_groups"] = int(np.unique(got[1][rows]).size != np.unique(key[rows]).size)
    rep_explicit(name, key, has, rng)
    fused(name, key, has)
    fused(name, key, has, first_rank=1037, chunk=7)
    fused_explicit(name, key, has, rng)


rng = np.random.default_rng(100 + BITS)
ones = lambda n: np.ones(n, np.uint8)  # noqa: E731

# ---- one-bit families ---------------------------------------------------------------
for tag, base in (("rand", int(rng.integers(1, M64 - 1, dtype=np.uint64))), ("zero", 0),
                  ("ones", M64)):
    fam = HK.one_bit_family(base)
    key = HK.spread_rows(fam, 3, rng, rng.integers(1, M64 - 1, 5000, dtype=np.uint64))
    all_forms(f"onebit_{tag}", key, ones(key.size), rng, groups_of=fam)
# the three families in one call
fams = np.unique(np.concatenate([HK.one_bit_family(b) for b in (0, M64, 0x0123456789ABCDEF)]))
key = HK.spread_rows(fams, 3, rng, rng.integers(1, M64 - 1, 5000, dtype=np.uint64))
all_forms("onebit_all", key, ones(key.size), rng, groups_of=fams)

# ---- one slot, one step ---------------------------------------------------------------
for tag, lo32 in (("last", HK.LO32_LAST), ("first", HK.LO32_FIRST)):
    fam = HK.slot_step_family(lo32)
    key = HK.spread_rows(fam, 2, rng)                      # 1024 rows of one bucket: LDS
    all_forms(f"oneslot_{tag}_x2", key, ones(key.size), rng, groups_of=fam)
    key = HK.spread_rows(fam, 10, rng)                     # 5120 rows: the global table
    assert np.isin(key, fam).sum() == 5120
    all_forms(f"oneslot_{tag}_x10", key, ones(key.size), rng, groups_of=fam)
# both families and random rows around them
fam = np.concatenate([HK.slot_step_family(HK.LO32_LAST), HK.slot_step_family(HK.LO32_FIRST)])
key = HK.spread_rows(fam, 4, rng, rng.integers(1, M64 - 1, 20_000, dtype=np.uint64))
all_forms("oneslot_both_x4", key, ones(key.size), rng, groups_of=fam)

# ---- the key whose hash is ~0 ---------------------------------------------------------
two = np.array([KS, M64], np.uint64)
for keyless in (0, 1):
    def has_of(n):
        return (rng.random(n) > 0.1).astype(np.uint8) if keyless else ones(n)
    sfx = "_keyless" if keyless else ""
    key = np.full(700, KS, np.uint64)
    all_forms("hash_ones_alone" + sfx, key, has_of(700), rng, groups_of=two[:1])
    key = np.concatenate([two[rng.integers(0, 2, 1400)],
                          rng.integers(1, M64 - 1, 200, dtype=np.uint64)])
    key = rng.permutation(key)
    all_forms("hash_ones_with_key_ones" + sfx, key, has_of(key.size), rng, groups_of=two)
    key = rng.permutation(np.concatenate([np.repeat(two, 5000),
                                          rng.integers(1, M64 - 1, 500, dtype=np.uint64)]))
    all_forms("hash_ones_5000" + sfx, key, has_of(key.size), rng, groups_of=two)
    # in one bucket with other keys of the highest digit
    hi = HK.keys_with_hash(300, rng, digit=(1 << 15) - 1, digit_bits=15)
    key = HK.spread_rows(np.concatenate([hi, two[:1]]), 3, rng)
    all_forms("hash_ones_in_bucket" + sfx, key, has_of(key.size), rng)

# ---- digit edges ----------------------------------------------------------------------
eb = BITS if BITS else 5
edge = np.concatenate([HK.digit_edge_keys(eb, 200, rng), two[:1], np.array([0], np.uint64)])
assert set(HK.digit_of(edge, eb).tolist()) == {0, (1 << eb) - 1}
key = HK.spread_rows(edge, 3, rng, rng.integers(1, M64 - 1, 3000, dtype=np.uint64))
all_forms("digit_edges", key, ones(key.size), rng, groups_of=edge)
edge15 = HK.digit_edge_keys(15, 300, rng)
key = HK.spread_rows(edge15, 3, rng)
all_forms("digit_edges_only", key, ones(key.size), rng, groups_of=edge15)

res["secs"] = round(time.time() - T0, 2)
print(json.dumps(res), flush=True)
'''

CONFIGS = [0, 6, 12, 13, 15]


@pytest.mark.parametrize("bits", CONFIGS, ids=["default"] + [f"bits{b}" for b in CONFIGS[1:]])
def test_chosen_hashes_vs_oracle(bits):
    env = dict(os.environ, SDGPU_POISON_WS="1")
    env.pop("SDGPU_GROUP_HIST", None)
    env.pop("SDGPU_GROUP_BITS", None)
    if bits:
        env["SDGPU_GROUP_BITS"] = str(bits)
    t0 = time.time()
    p = subprocess.run([sys.executable, "-c", _CHILD, ROOT, str(bits)], capture_output=True,
                       text=True, timeout=240, env=env)
    wall = time.time() - t0
    assert p.returncode == 0, p.stderr[-3000:]
    res = json.loads(p.stdout.strip().splitlines()[-1])
    print(f"\nchosen hashes bits={bits}: child {res['secs']} s, wall {wall:.1f} s, "
          f"{len(res['counts'])} cases, plan {res['plan']}")
    # the plan that ran: the forced bits, or what the row count gives (1 and 5)
    want = [[1500, bits or 1], [70_000, bits or 5]]
    assert res["plan"] == want, res["plan"]
    assert max(res["rows"].values()) < 70_000
    wrong = {k: v for k, v in res["counts"].items() if v != 0}
    assert len(res["counts"]) > 150 and not wrong, wrong
    for name in ("onebit_ones", "oneslot_last_x2", "oneslot_first_x10", "hash_ones_5000_keyless",
                 "digit_edges"):
        assert f"{name}_groups" in res["counts"] or name.startswith("hash_ones_in"), name
        assert f"{name}_fused_explicit_c100" in res["counts"] and f"{name}_linkbatch_c1" in res["counts"]


# ---- owner boundaries of the exchange ------------------------------------------------
@pytest.fixture(scope="module")
def ctxs():
    from spacedrive_amd._native import Context
    cs = [Context(0) for _ in range(3)]
    yield cs
    for c in cs:
        c.close()


@pytest.mark.parametrize("mode", ["counted", "padded"])
@pytest.mark.parametrize("world", [2, 3])
def test_owner_boundaries(ctxs, world, mode):
    """Keys on both sides of every boundary of ((h >> 56) * world) >> 8: grouped
    sharded against the oracle, and each rank's share -- the keys its Object
    index holds afterwards, the rows its write set lists -- against
    dedup.shard_of."""
    import torch
    from spacedrive_amd import dedup
    rng = np.random.default_rng(world)
    pool = np.concatenate([HK.owner_boundary_keys(300, rng),
                           rng.integers(1, HK.M64 - 1, 1000, dtype=np.uint64),
                           np.array([0, HK.M64, HK.KEY_HASH_ALL_ONES], np.uint64)])
    total = 12_000
    k = pool[rng.integers(0, pool.size, total)]
    h = (rng.random(total) > 0.02).astype(np.uint8)
    owner = (dedup.shard_of(k) * world) >> 8
    edge = dedup.shard_of(k)
    for s in HK.OWNER_SHARDS:
        assert ((edge == s) & (h == 1)).sum() > 100
    comms = dedup.Comm.init_all(ctxs[:world])
    ex = dedup.EXCHANGE_COUNTED if mode == "counted" else dedup.EXCHANGE_PADDED
    keys, hass, vals, ranks, spans = [], [], [], [], []
    for r in range(world):
        a, b = total * r // world, total * (r + 1) // world
        spans.append((a, b))
        keys.append(torch.from_numpy(k[a:b].view(np.int64)).cuda())
        hass.append(torch.from_numpy(h[a:b]).cuda())
        vals.append(torch.from_numpy(np.ones(b - a, np.uint8)).cuda())
        ranks.append(torch.arange(a, b, dtype=torch.int64).to(torch.int32).cuda())
    for cm in comms:
        cm.set_exchange(ex, max(x.numel() for x in keys))
    ref = O.group_reps(k, h, 100)
    idxs = [dedup.ObjectIndex(c, 256) for c in ctxs[:world]]
    before = [cm.stats() for cm in comms]
    reps = dedup.group_sharded_all(keys, hass, ranks, comms, idxs, 100)
    torch.cuda.synchronize()
    for (a, b), rp in zip(spans, reps):
        np.testing.assert_array_equal(rp.cpu().numpy().view(np.uint32), ref[a:b])
    keyed = h == 1
    asked = torch.from_numpy(np.unique(k).view(np.int64)).cuda()
    uowner = (dedup.shard_of(np.unique(k)) * world) >> 8
    in_use = np.isin(np.unique(k), k[keyed])
    for r in range(world):
        # the rows this rank received, and the keys it keeps: its shards', no others
        got_rows = comms[r].stats()["rows_received"] - before[r]["rows_received"]
        if mode == "counted":
            assert got_rows == int((keyed & (owner == r)).sum())
        held = idxs[r].lookup(asked).cpu().numpy().view(np.uint32) != 0xFFFFFFFF
        np.testing.assert_array_equal(held, in_use & (uowner == r))
    # the write set: rank r lists the keyed rows it owns and its own keyless rows
    parts = dedup.group_link_sharded_all(keys, hass, vals, ranks, comms, 100)
    rc, rlr, rlo = O.link_batch(ref, None, None, 0)
    w = np.concatenate([p[0].cpu().numpy() for p in parts])
    o = np.concatenate([p[1].cpu().numpy() for p in parts])
    c, lr, lo = dedup.split_link_lists(w, o)
    np.testing.assert_array_equal(c, rc)
    np.testing.assert_array_equal(lr, rlr)
    np.testing.assert_array_equal(lo, rlo)
    for r, (a, b) in enumerate(spans):
        rows = parts[r][0].cpu().numpy().view(np.uint32) & np.uint32(0x7FFFFFFF)
        mine = np.flatnonzero((keyed & (owner == r)) | (~keyed & (np.arange(total) >= a)
                                                        & (np.arange(total) < b)))
        np.testing.assert_array_equal(np.sort(rows), mine)
    for ix in idxs:
        ix.close()
    for cm in comms:
        cm.close()
