"""GPU: the Object index as a library-lifetime structure -- lookup, removal by
key and by Object id, revival, export, stats, bounded capacity under churn,
and groupings after removals equal to the oracle's (a removed Object is one the
reference's library-wide find_many, file_identifier/mod.rs:168-185, no longer
returns).  The model is a Python dict {key: value}; every key pool holds
2**64-1, the table's empty-slot value."""
import os

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

EXISTING = 0x80000000
MISS = 0xFFFFFFFF
SPECIAL = np.uint64(2**64 - 1)


def _rows(seed, n, distinct, keyless=0.01):
    rng = np.random.default_rng(seed)
    pool = rng.integers(0, 2**64 - 1, distinct, dtype=np.uint64, endpoint=True)
    pool[0] = SPECIAL  # the table's empty-slot value is a legal key
    key = pool[rng.integers(0, pool.size, n)]
    has = (rng.random(n) > keyless).astype(np.uint8)
    return key, has


def _pool(seed, n):
    """n distinct keys, the first one 2**64-1."""
    rng = np.random.default_rng(seed)
    pool = np.unique(rng.integers(0, 2**64 - 2, 2 * n, dtype=np.uint64))
    pool = rng.permutation(pool)[:n].copy()
    pool[0] = SPECIAL
    assert np.unique(pool).size == n
    return pool


def _dk(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64).copy()).cuda()


def _dv(a, dtype=np.uint32):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype).view(np.int32).copy()).cuda()


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


class Model:
    """{key: value}; a key keeps the value of the lowest slot encoding
    (value ^ EXISTING): registered Objects before ranks, lowest first."""

    def __init__(self):
        self.d = {}

    def put(self, keys, values):
        for k, v in zip(np.asarray(keys, np.uint64).tolist(), np.asarray(values).tolist()):
            v = int(v) & 0xFFFFFFFF
            if k not in self.d or (v ^ EXISTING) < (self.d[k] ^ EXISTING):
                self.d[k] = v

    def register(self, keys, handles):
        self.put(keys, np.asarray(handles, np.uint32) | np.uint32(EXISTING))

    def remove(self, keys):
        n = 0
        for k in set(np.asarray(keys, np.uint64).tolist()):
            n += self.d.pop(k, None) is not None
        return n

    def remove_handles(self, handles):
        hs = {int(h) | EXISTING for h in handles if h >= 0}
        gone = [k for k, v in self.d.items() if v in hs]
        for k in gone:
            del self.d[k]
        return gone

    def lookup(self, keys):
        return np.array([self.d.get(k, MISS) for k in np.asarray(keys, np.uint64).tolist()],
                        np.uint32)


def _register(idx, model, keys, handles, **kw):
    idx.add_objects(_dk(keys), _dv(handles), **kw)
    if model is not None:
        model.register(keys, handles)


def _assert_lookup(idx, model, keys):
    got = _u32(idx.lookup(_dk(keys)))
    np.testing.assert_array_equal(got, model.lookup(keys))


def test_lookup_equals_model(ctx):
    """400 registered keys (50 of them twice, under different handles) and 200
    absent ones: EXISTING | min handle, or MISS; host form == device form."""
    from spacedrive_amd import _native, dedup
    assert _native.INDEX_MISS == MISS
    pool = _pool(1, 600)
    keys, absent = pool[:400], pool[400:]
    rng = np.random.default_rng(2)
    h1 = rng.permutation(400).astype(np.uint32) + 10
    idx, m = dedup.ObjectIndex(ctx, 256), Model()
    _register(idx, m, keys, h1)
    _register(idx, m, keys[:50], rng.permutation(50).astype(np.uint32) + 5)   # some lower
    _register(idx, m, keys[25:75][:25], np.arange(25, dtype=np.uint32) + 1000)  # some higher
    ask = rng.permutation(np.concatenate([keys, absent]))
    want = m.lookup(ask)
    assert np.count_nonzero(want == MISS) == 200
    assert np.all((want[want != MISS] & EXISTING) != 0)
    dev = _u32(idx.lookup(_dk(ask)))
    np.testing.assert_array_equal(dev, want)
    host = idx.lookup(ask)
    assert host.dtype == np.uint32
    np.testing.assert_array_equal(host, want)
    assert idx.lookup(int(SPECIAL)) == m.d[int(SPECIAL)]       # the separately stored key
    assert idx.lookup(int(absent[3])) == MISS
    assert idx.count() == 400 and idx.stats()[:2] == (400, 400)
    assert idx.stats()[2] >= 1024
    idx.close()


def test_remove_inside_probe_chains_and_revive(ctx):
    """500 keys in a 1024-slot table sit in multi-slot probe chains; removing a
    random half must not cut a chain for the others.  Then 100 removed keys
    come back under HIGHER handles: the stale minimum must not survive."""
    from spacedrive_amd import dedup
    pool = _pool(3, 500)
    rng = np.random.default_rng(4)
    handles = rng.permutation(500).astype(np.uint32) + 100
    idx, m = dedup.ObjectIndex(ctx, 256), Model()
    _register(idx, m, pool, handles)
    assert idx.stats() == (500, 500, 1024)
    sel = rng.permutation(500)
    gone, kept = pool[sel[:250]], pool[sel[250:]]
    if SPECIAL not in gone:   # the special key goes through removal and revival too
        gone[0], kept[np.flatnonzero(kept == SPECIAL)[0]] = SPECIAL, gone[0]
    assert idx.remove(_dk(gone)) == 250 == m.remove(gone)
    got = _u32(idx.lookup(_dk(pool)))
    np.testing.assert_array_equal(got, m.lookup(pool))
    assert np.all(_u32(idx.lookup(_dk(gone))) == MISS)
    assert np.all(_u32(idx.lookup(_dk(kept))) != MISS)
    assert idx.count() == 250
    st = idx.stats()
    assert st[0] == 250 and st[1] == 500
    assert idx.remove(_dk(gone)) == 0                      # already removed
    assert idx.remove(_dk(np.repeat(kept[7], 5))) == 1     # one key listed 5 times
    m.remove(kept[7:8])
    assert idx.count() == 249
    # revive 100 of the first removal under higher handles than before
    back = gone[:100]
    old = {int(k): int(h) for k, h in zip(pool, handles)}
    new_h = np.array([old[int(k)] + 5000 for k in back], np.uint32)
    _register(idx, m, back[:10], new_h[:10])               # fits: revived in place
    assert idx.stats() == (259, 500, 1024)
    _register(idx, m, back[10:], new_h[10:])               # (may rebuild the table)
    got = _u32(idx.lookup(_dk(back)))
    np.testing.assert_array_equal(got, new_h | np.uint32(EXISTING))
    _assert_lookup(idx, m, pool)
    assert idx.count() == 349 == idx.stats()[0]
    idx.close()


def test_count_after_revive_is_350(ctx):
    """The issue's figures exactly: 500 registered, 250 removed, 100 revived."""
    from spacedrive_amd import dedup
    pool = _pool(5, 500)
    idx = dedup.ObjectIndex(ctx, 256)
    _register(idx, None, pool, np.arange(500, dtype=np.uint32) + 1)
    assert idx.remove(_dk(pool[:250])) == 250
    assert idx.count() == 250
    _register(idx, None, pool[:100], np.arange(100, dtype=np.uint32) + 9000)
    assert idx.count() == 350 == idx.stats()[0]
    got = _u32(idx.lookup(_dk(pool[:100])))
    np.testing.assert_array_equal(got, (np.arange(100, dtype=np.uint32) + 9000) | np.uint32(EXISTING))
    idx.close()


def test_conditional_removal(ctx):
    """remove(key, value): the wrong value removes nothing, the right one removes."""
    from spacedrive_amd import dedup
    pool = _pool(6, 300)
    handles = np.arange(300, dtype=np.uint32) + 40
    idx, m = dedup.ObjectIndex(ctx, 256), Model()
    _register(idx, m, pool, handles)
    stored = m.lookup(pool[:60])
    wrong = stored.copy()
    wrong[:30] += 1                                    # another Object took the key over
    wrong[30:] = stored[30:] & np.uint32(0x7FFFFFFF)   # the handle read as a rank
    assert idx.remove(_dk(pool[:60]), _dv(wrong)) == 0
    assert idx.count() == 300
    _assert_lookup(idx, m, pool)
    mixed = stored.copy()
    mixed[::2] = wrong[::2]                             # every other one stale
    assert idx.remove(_dk(pool[:60]), _dv(mixed)) == 30
    m.remove(pool[:60][1::2])
    _assert_lookup(idx, m, pool)
    assert idx.count() == 270
    idx.close()


def _scenario(ctx):
    """An index with both value kinds and removed slots: 300 registered Objects,
    a dedup_batch of 2,000 rows (rank entries), 120 handles removed."""
    from spacedrive_amd import dedup
    pool = _pool(7, 900)
    ek = pool[:300]
    eh = np.arange(300, dtype=np.uint32) * 3 + 10_000
    idx, m = dedup.ObjectIndex(ctx, 256), Model()
    _register(idx, m, ek, eh)
    rng = np.random.default_rng(8)
    bkeys = np.concatenate([pool[300:800], ek[:40]])    # 500 new keys + 40 owned ones
    key = bkeys[rng.integers(0, bkeys.size, 2000)]
    key[5] = pool[300]
    has = (rng.random(2000) > 0.02).astype(np.uint8)
    rep = dedup.dedup_batch(key, has, 0, idx, 100, ctx)
    r = np.arange(2000, dtype=np.uint32)
    created = (rep == r) & (has == 1)
    m.put(key[created], r[created])                     # the index keeps the lowest rank
    ranks_before = {k: v for k, v in m.d.items() if not v & EXISTING}
    assert len(ranks_before) > 300
    return idx, m, pool, ek, eh, ranks_before


def test_remove_by_handle(ctx):
    """remove_objects with 120 handles -- some absent from the table, one equal
    to a stored RANK: exactly the matching existing-handle entries go."""
    idx, m, pool, ek, eh, ranks_before = _scenario(ctx)
    _assert_lookup(idx, m, pool)
    a_rank = sorted(ranks_before.values())[len(ranks_before) // 2]
    handles = np.concatenate([eh[50:150],                       # 100 present
                              eh[:19] + 1,                      # 19 absent (between handles)
                              [a_rank]]).astype(np.int32)       # a stored rank's number
    assert handles.size == 120 and a_rank not in set(eh.tolist())
    before = idx.count()
    removed = idx.remove_objects(_dv(handles, np.int32), 20_000)
    gone = m.remove_handles(handles.tolist())
    assert removed == len(gone) == 100
    _assert_lookup(idx, m, pool)
    assert idx.count() == before - 100
    # no rank entry was touched
    for k, v in ranks_before.items():
        assert m.d[k] == v
    got = idx.lookup(np.array(list(ranks_before), np.uint64))
    np.testing.assert_array_equal(got, np.array(list(ranks_before.values()), np.uint32))
    # ids past max_handle and negative ids match nothing
    assert idx.remove_objects(_dv(np.array([-1, -7, int(eh[200])], np.int32), np.int32),
                              int(eh[200]) - 1) == 0
    assert idx.remove_objects(_dv(np.array([-1, int(eh[200])], np.int32), np.int32),
                              int(eh[200])) == 1
    idx.close()


def test_orphan_remover_feeds_the_index(ctx):
    """consumers.orphan_objects' device result goes straight into
    remove_objects: exactly the orphans' keys miss afterwards."""
    import torch
    from spacedrive_amd import consumers, dedup
    pool = _pool(9, 700)
    obj_ids = (np.arange(700, dtype=np.int32) * 2 + 3)          # Object i owns pool[i]
    rng = np.random.default_rng(10)
    idx, m = dedup.ObjectIndex(ctx, 256), Model()
    _register(idx, m, pool, obj_ids.astype(np.uint32))
    referenced = rng.random(700) > 0.3
    if referenced[0]:
        referenced[0] = False                                   # the key ~0's Object is an orphan
    fp = np.concatenate([obj_ids[referenced], obj_ids[referenced][:50],
                         np.full(30, -1, np.int32)])            # NULL object_ids
    fp = rng.permutation(fp).astype(np.int32)
    want = O.orphan_objects(obj_ids, fp)
    max_id = int(obj_ids.max())
    out, cnt, removed = consumers.remove_orphans_from_index(
        idx, torch.from_numpy(obj_ids).cuda(), torch.from_numpy(fp).cuda(), max_id)
    n = int(cnt.item())
    np.testing.assert_array_equal(out[:n].cpu().numpy(), want)
    assert removed == want.size == int((~referenced).sum())
    gone = m.remove_handles(want.tolist())
    assert len(gone) == want.size
    got = _u32(idx.lookup(_dk(pool)))
    np.testing.assert_array_equal(got == MISS, ~referenced)
    np.testing.assert_array_equal(got, m.lookup(pool))
    assert idx.count() == int(referenced.sum())
    idx.close()


def test_export_equals_model(ctx):
    """After registrations, a grouping, removals and a revival: the export is
    the model as a set -- the key ~0 and both value kinds included; a short
    buffer gets the full count and nothing past cap."""
    import torch
    idx, m, pool, ek, eh, ranks_before = _scenario(ctx)
    idx.remove_objects(_dv(eh[50:150].astype(np.int32), np.int32), 20_000)
    m.remove_handles(eh[50:150].tolist())
    some_ranks = np.array(list(ranks_before)[:60], np.uint64)
    assert idx.remove(_dk(some_ranks)) == 60 == m.remove(some_ranks)
    _register(idx, m, ek[60:80], np.arange(20, dtype=np.uint32) + 30_000)   # revived
    if int(SPECIAL) not in m.d:
        _register(idx, m, [SPECIAL], np.array([77], np.uint32))
    k, v = idx.export()
    got = dict(zip(k.cpu().numpy().view(np.uint64).tolist(), _u32(v).tolist()))
    assert k.numel() == len(got) == len(m.d) == idx.count()
    assert got == m.d
    assert int(SPECIAL) in got
    kinds = np.array(list(got.values()), np.uint32) & np.uint32(EXISTING)
    assert np.any(kinds != 0) and np.any(kinds == 0)
    # default cap too small: export() retries once with the reported count
    k2, v2 = idx.export(cap=10)
    assert dict(zip(k2.cpu().numpy().view(np.uint64).tolist(), _u32(v2).tolist())) == m.d
    # a short buffer: full count, nothing past cap (guard words intact)
    cap, guard = 100, 64
    dkey = torch.full((cap + guard,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    dval = torch.full((cap + guard,), 0x5B5B5B5B, dtype=torch.int32, device="cuda")
    dcnt = torch.zeros(1 + guard, dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    rc = ctx.lib.sdgpu_index_export_device(idx.h, dkey.data_ptr(), dval.data_ptr(), cap,
                                           dcnt.data_ptr(), s)
    assert rc == 0
    torch.cuda.synchronize()
    assert int(dcnt[0].item()) == len(m.d) > cap
    assert torch.all(dcnt[1:] == 0)
    assert torch.all(dkey[cap:] == 0x5A5A5A5A5A5A5A5A) and torch.all(dval[cap:] == 0x5B5B5B5B)
    part = dict(zip(dkey[:cap].cpu().numpy().view(np.uint64).tolist(), _u32(dval[:cap]).tolist()))
    assert len(part) == cap and all(m.d[kk] == vv for kk, vv in part.items())
    # cap 0 with NULL arrays: just the count
    rc = ctx.lib.sdgpu_index_export_device(idx.h, None, None, 0, dcnt.data_ptr(), s)
    assert rc == 0 and int(dcnt[0].item()) == len(m.d)
    idx.close()


# ---- groupings after a removal against the oracle --------------------------------

N, NA, NB = 60_000, 30_000, 45_000


def _run_rows(seed):
    """_rows(seed, 60_000, 20_000) with the key ~0 on a keyed row of every batch."""
    key, has = _rows(seed, N, 20_000)
    for i in (10, NA + 5, NB + 5):
        key[i], has[i] = SPECIAL, 1
    return key, has


def _removed_set(key, has, seed, count, among=None):
    """`count` distinct keys of keyed rows of batch A, the key ~0 among them."""
    rng = np.random.default_rng(seed)
    cand = np.unique(key[:NA][has[:NA] == 1]) if among is None else among
    cand = cand[cand != SPECIAL]
    R = rng.choice(cand, count - 1, replace=False)
    return np.concatenate([R, [SPECIAL]])


def _has_without(key, has, R):
    """has with the A-rows whose key is in R turned keyless: for the rows after
    A, a removed Object is one the library-wide lookup no longer returns."""
    has2 = has.copy()
    has2[:NA][np.isin(key[:NA], R)] = 0
    return has2


def test_grouping_after_removal_matches_oracle(ctx):
    """Batch A through the index, 3,000 of its keys removed, two more batches:
    a removed key's first later row creates again, the chunk rule applies from
    there, and the last batch links to creators of the one before (revival
    through the creators' insert)."""
    from spacedrive_amd import dedup
    key, has = _run_rows(21)
    idx = dedup.ObjectIndex(ctx, 1000)
    repA = dedup.dedup_batch(key[:NA], has[:NA], 0, idx, 100, ctx)
    np.testing.assert_array_equal(repA, O.group_reps(key, has, 100)[:NA])
    R = _removed_set(key, has, 22, 3000)
    assert idx.remove(_dk(R)) == 3000
    repB = dedup.dedup_batch(key[NA:NB], has[NA:NB], NA, idx, 100, ctx)
    repC = dedup.dedup_batch(key[NB:], has[NB:], NB, idx, 100, ctx)
    want = O.group_reps(key, _has_without(key, has, R), 100)[NA:]
    got = np.concatenate([repB, repC])
    np.testing.assert_array_equal(got, want)
    # the removal mattered, and C linked to Objects re-created in B
    assert np.any(want != O.group_reps(key, has, 100)[NA:])
    inR = np.isin(key[NB:], R) & (has[NB:] == 1)
    assert np.count_nonzero(inR & (repC >= NA) & (repC < NB)) > 100
    # a removed key that no later row carries stays out of the index
    later = np.unique(key[NA:][has[NA:] == 1])
    assert idx.count() == np.unique(key[has == 1]).size - np.setdiff1d(R, later).size
    idx.close()


def test_grouping_after_removal_with_registered_objects(ctx):
    """Registered Objects, some of their keys removed (all (key, handle) pairs
    of a removed key drop out of the expectation)."""
    from spacedrive_amd import dedup
    key, has = _run_rows(23)
    rng = np.random.default_rng(24)
    ek = np.concatenate([rng.choice(key, 4000), rng.integers(0, 2**63, 1000, dtype=np.uint64),
                         [SPECIAL]])
    ek = np.concatenate([ek, ek[:500]])                 # keys owned by two Objects
    eh = rng.permutation(ek.size).astype(np.uint32) + 17
    idx = dedup.ObjectIndex(ctx, 1000)
    idx.add_objects(_dk(ek), _dv(eh))
    repA = dedup.dedup_batch(key[:NA], has[:NA], 0, idx, 100, ctx)
    np.testing.assert_array_equal(repA, O.group_reps_existing(key, has, 100, ek, eh)[:NA])
    # removed: registered keys (in A or not) and keys only A's creators hold
    uek = np.unique(ek)
    R = np.concatenate([_removed_set(key, has, 25, 1500, among=uek),
                        _removed_set(key, has, 26, 1501)[:-1]])
    R = np.unique(R)
    removed = idx.remove(_dk(R))
    present = np.union1d(uek, np.unique(key[:NA][has[:NA] == 1]))
    assert removed == np.intersect1d(R, present).size
    repB = dedup.dedup_batch(key[NA:NB], has[NA:NB], NA, idx, 100, ctx)
    repC = dedup.dedup_batch(key[NB:], has[NB:], NB, idx, 100, ctx)
    keep = ~np.isin(ek, R)
    want = O.group_reps_existing(key, _has_without(key, has, R), 100, ek[keep], eh[keep])[NA:]
    np.testing.assert_array_equal(np.concatenate([repB, repC]), want)
    assert np.count_nonzero(want & np.uint32(EXISTING)) > 1000
    idx.close()


def test_fused_grouping_after_removal(ctx):
    """The same through group_link(..., index=idx): the write sets of the later
    batches equal the oracle's as sets."""
    from spacedrive_amd import dedup
    key, has = _run_rows(27)
    rng = np.random.default_rng(28)
    ek = np.concatenate([rng.choice(key, 3000), [SPECIAL]])
    eh = rng.permutation(ek.size).astype(np.uint32) + 9
    idx = dedup.ObjectIndex(ctx, 1000)
    idx.add_objects(_dk(ek), _dv(eh))

    def run(a, b):
        import torch
        who, obj, (c, l) = dedup.group_link_device(_dk(key[a:b]), torch.from_numpy(has[a:b]).cuda(),
                                                   None, None, a, 100, ctx=ctx, index=idx)
        return who.cpu().numpy(), obj.cpu().numpy(), c, l

    wA, oA, cA, lA = run(0, NA)
    refA = O.group_reps_existing(key, has, 100, ek, eh)[:NA]
    rcA, rlrA, rloA = O.link_batch(refA, None, None, 0)
    fcA, flrA, floA = dedup.split_link_lists(wA, oA)
    np.testing.assert_array_equal(fcA, rcA)
    np.testing.assert_array_equal(flrA, rlrA)
    np.testing.assert_array_equal(floA, rloA)
    R = np.unique(np.concatenate([_removed_set(key, has, 29, 2000),
                                  _removed_set(key, has, 30, 800, among=np.unique(ek))]))
    assert idx.remove(_dk(R)) == R.size
    wB, oB, cB, lB = run(NA, NB)
    wC, oC, cC, lC = run(NB, N)
    keep = ~np.isin(ek, R)
    ref = O.group_reps_existing(key, _has_without(key, has, R), 100, ek[keep], eh[keep])[NA:]
    rc, rlr, rlo = O.link_batch(ref, None, None, NA)
    fc, flr, flo = dedup.split_link_lists(np.concatenate([wB, wC]), np.concatenate([oB, oC]))
    assert (cB + cC, lB + lC) == (rc.size, rlr.size)
    np.testing.assert_array_equal(fc, rc)
    np.testing.assert_array_equal(flr, rlr)
    np.testing.assert_array_equal(flo, rlo)
    idx.close()


def test_bounded_churn(ctx):
    """30 rounds of register 900 / look up / remove 900 in an index made for
    1,000 keys: the rehash drops removed slots, so capacity stops growing
    (without that the table doubles every other round)."""
    from spacedrive_amd import dedup
    idx = dedup.ObjectIndex(ctx, 1000)
    rng = np.random.default_rng(31)
    cap_after_2 = None

    def one_round(rnd):
        keys = np.unique(rng.integers(0, 2**64 - 2, 1000, dtype=np.uint64))[:899]
        keys = np.concatenate([keys, [SPECIAL]])
        assert keys.size == 900
        h = (rng.permutation(900) + 1 + 1000 * rnd).astype(np.uint32)
        dk = _dk(keys)
        idx.add_objects(dk, _dv(h))
        got = _u32(idx.lookup(dk))
        np.testing.assert_array_equal(got, h | np.uint32(EXISTING))
        return dk

    for rnd in range(30):
        dk = one_round(rnd)
        assert idx.count() == 900
        assert idx.remove(dk) == 900
        if rnd == 1:
            cap_after_2 = idx.stats()[2]
    live, used, cap = idx.stats()
    assert cap <= cap_after_2, (cap, cap_after_2)
    assert live == 0 == idx.count()
    assert used <= cap // 2 + 1
    one_round(30)                         # still answered exactly
    assert idx.count() == 900
    idx.close()


def test_sharded_shares(ctx):
    """Two shares of one list (add_objects world=2) on one GPU, the same removal
    list given to both: the per-key union of their lookups is the model, and
    each share misses every key of the other."""
    from spacedrive_amd import dedup
    pool = _pool(33, 800)
    handles = np.arange(800, dtype=np.uint32) + 50
    owner = (dedup.shard_of(pool) * 2) >> 8
    assert 300 < int((owner == 0).sum()) < 500
    m = Model()
    m.register(pool[:600], handles[:600])
    shares = [dedup.ObjectIndex(ctx, 256) for _ in range(2)]
    for r, sh in enumerate(shares):
        _register(sh, None, pool[:600], handles[:600], world=2, rank=r)
        assert sh.count() == int((owner[:600] == r).sum())
    gone = np.concatenate([pool[100:300], pool[600:650]])       # some absent everywhere
    total = sum(sh.remove(_dk(gone)) for sh in shares)
    assert total == 200 == m.remove(gone)
    got = [_u32(sh.lookup(_dk(pool))) for sh in shares]
    for r in range(2):
        assert np.all(got[r][owner != r] == MISS)               # the other share's keys
    assert not np.any((got[0] != MISS) & (got[1] != MISS))
    union = np.where(got[0] != MISS, got[0], got[1])
    np.testing.assert_array_equal(union, m.lookup(pool))
    for sh in shares:
        sh.close()


# ---- a caller-owned index across two identifier jobs ------------------------------

def _small_library(root, n=2400, seed=41):
    """Location 1: n small files under /a/ and /b/, about a quarter of them
    duplicates of earlier content (so /b/ shares cas_ids with /a/)."""
    from spacedrive_amd.file_identifier import FilePaths
    rng = np.random.default_rng(seed)
    t = FilePaths()
    loc = os.path.join(root, "loc1")
    for d in ("a", "b"):
        os.makedirs(os.path.join(loc, d), exist_ok=True)
        t.add(1, "/", d, is_dir=True)
    contents = []
    for i in range(n):
        if contents and rng.random() < 0.25:
            data = contents[rng.integers(0, len(contents))]
        else:
            data = O.synth_file_bytes(50_000 + i, 0, int(rng.integers(0, 3000)))
            contents.append(data)
        d = "a" if rng.random() < 0.5 else "b"
        name = f"f{i:05d}.bin"
        with open(os.path.join(loc, d, name), "wb") as f:
            f.write(data)
        t.add(1, f"/{d}/", name)
    return t, loc


def test_caller_owned_index_across_two_jobs(ctx, tmp_path):
    """One index through two jobs, Objects deleted in between and taken out
    with remove_objects: the second job links as a job that loads a fresh
    index from the table."""
    import copy
    import torch
    from spacedrive_amd import dedup
    from spacedrive_amd.file_identifier import FileIdentifierJob
    t, loc = _small_library(str(tmp_path))
    idx = dedup.ObjectIndex(ctx, 4096)
    j1 = FileIdentifierJob(t, 1, loc, sub_path="a", chunks_per_step=3, ctx=ctx, index=idx).init()
    j1.run()
    j1.close()
    assert idx.h is not None                       # the job did not close the caller's index
    ek, eh = t.existing_objects()
    assert idx.count() == np.unique(ek).size > 500
    k, v = idx.export()
    assert torch.all((v.view(torch.int32) < 0))    # every entry names an Object id, none a rank
    # the library deletes the Objects of 60 cas_ids (all Objects of each key:
    # the index keeps one Object per key, include/sdgpu.h); their rows are orphans again
    rng = np.random.default_rng(42)
    dead_keys = set(rng.choice(np.unique(ek), 60, replace=False).tolist())
    dead_objs = sorted({int(h) for kk, h in zip(ek.tolist(), eh.tolist()) if kk in dead_keys})
    dead = set(dead_objs)
    for i, o in enumerate(t.object_id):
        if o in dead:
            t.object_id[i] = None
    removed = idx.remove_objects(torch.tensor(dead_objs, dtype=torch.int32).cuda(),
                                 t.next_object_id)
    assert removed == 60
    assert idx.count() == np.unique(t.existing_objects()[0]).size
    # second job over the whole location: /b/ and the rows orphaned above
    fresh = copy.deepcopy(t)
    j2 = FileIdentifierJob(t, 1, loc, chunks_per_step=4, ctx=ctx, index=idx).init()
    m2 = j2.run()
    j2.close()
    jf = FileIdentifierJob(fresh, 1, loc, chunks_per_step=4, ctx=ctx).init()
    mf = jf.run()
    jf.close()
    assert t.object_id == fresh.object_id and t.cas_id == fresh.cas_id
    assert (m2.total_objects_created, m2.total_objects_linked) == \
        (mf.total_objects_created, mf.total_objects_linked)
    assert m2.total_objects_linked > 300
    assert idx.h is not None
    assert idx.count() == np.unique(t.existing_objects()[0]).size
    idx.close()
