"""GPU: the four open-addressing tables (Object index, thumbnail table with its
filter, the indexer's row table and directory set, the sync op log) on keys
with CHOSEN hashes (tests/hash_keys.py): probe chains that wrap through slot 0,
chains as long as half the table, the keys 0 and ~0 next to a cluster that
ends at the last slot, absent keys that walk the whole wrapped cluster, copies
of every key so that CAS losers and finders mix in one chain -- and the op
log at 2^16 and 2^24 slots, where the key ~0's slot number alone needs one
more sort pass.

Random keys reach none of this: 1024 of them in 2048 slots give a longest
displacement of about 13.  The premises of every scenario are asserted from the
model in tests/test_hash_keys.py (CPU) on the same builders; the expected
results come from the existing oracles, which know nothing about slots.

Why the walks end: every table has a power-of-two capacity with load <= 1/2
(asserted here through stats() where the table has them, by the capacity rule
otherwise), every step is (h + 1) & (cap - 1), so a walk stays inside the table
and meets an empty slot."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import hash_keys as HK
from tests import sync_oracle as SO
from tests.test_gpu_index_lifecycle import EXISTING, MISS, Model, _dk, _dv, _register, _u32
from tests.test_gpu_indexer_diff import check as indexer_check
from tests.test_gpu_indexer_diff import is_dir_of, meta_of
from tests.test_gpu_stale_thumbnails import check as stale_check
from tests.test_gpu_stale_thumbnails import dev, even_dirs
from tests.test_gpu_sync_ingest import Log
from tests.test_gpu_thumbnailer import check as work_check
from tests.test_gpu_thumbnailer import expected as work_expected

pytestmark = pytest.mark.gpu

M64 = HK.M64
CASES = pytest.mark.parametrize("case", HK.TABLE_CASES, ids=HK.case_id)


def _scenario(case, cap_of):
    sc = HK.table_scenario(*case, cap_of)
    HK.check_table_scenario(sc)          # the premise, from the model: not assumed
    return sc


def _asked(sc, rng):
    """Every present and absent key, two to three times, shuffled."""
    both = np.concatenate([sc.keys, sc.absent])
    return rng.permutation(np.repeat(both, rng.integers(2, 4, both.size)))


# ---- Object index ------------------------------------------------------------------
@CASES
def test_object_index(ctx, case):
    from spacedrive_amd import dedup
    sc = _scenario(case, HK.cap_first_call)
    rng = np.random.default_rng(len(sc.name))
    idx, m = dedup.ObjectIndex(ctx, 256), Model()
    assert idx.stats() == (0, 0, 1024)
    handles = rng.permutation(sc.rows.size).astype(np.uint32) + 10
    _register(idx, m, sc.rows, handles)                  # copies: the lowest handle stays
    n = sc.keys.size
    assert idx.stats() == (n, n, sc.cap) and idx.count() == n
    ask = _asked(sc, rng)
    want = m.lookup(ask)
    assert np.count_nonzero(want == MISS) == np.isin(ask, sc.absent).sum() > 0
    np.testing.assert_array_equal(_u32(idx.lookup(_dk(ask))), want)
    np.testing.assert_array_equal(idx.lookup(ask), want)             # host form
    # every second key of the wrapped chain goes (the key ~0 too): no chain is cut
    chain = sc.homes[sc.cap - 1]
    gone = chain[::2]
    if sc.specials:
        gone = np.concatenate([gone, np.array([M64], np.uint64)])
    listed = rng.permutation(np.repeat(gone, 2))
    assert idx.remove(_dk(listed)) == gone.size == m.remove(gone)
    np.testing.assert_array_equal(_u32(idx.lookup(_dk(ask))), m.lookup(ask))
    assert np.all(_u32(idx.lookup(_dk(gone))) == MISS)
    assert np.all(_u32(idx.lookup(_dk(chain[1::2]))) != MISS)
    assert idx.stats() == (n - gone.size, n, sc.cap)
    k, v = idx.export()
    assert dict(zip(k.cpu().numpy().view(np.uint64).tolist(), _u32(v).tolist())) == m.d
    # revival under higher handles (in place while the table has room, else a rebuild)
    back = gone[: max(1, gone.size // 2)]
    _register(idx, m, back, np.arange(back.size, dtype=np.uint32) + 50_000)
    np.testing.assert_array_equal(_u32(idx.lookup(_dk(back))),
                                  (np.arange(back.size, dtype=np.uint32) + 50_000) | np.uint32(EXISTING))
    np.testing.assert_array_equal(_u32(idx.lookup(_dk(ask))), m.lookup(ask))
    assert idx.count() == len(m.d) == idx.stats()[0]
    # growth: the rehash re-places the wrapped cluster
    cap_before = idx.stats()[2]
    more = np.concatenate([HK.keys_at(2 * cap_before, 2 * cap_before - 1, 300, rng),
                           rng.integers(1, M64 - 1, 2 * cap_before, dtype=np.uint64)])
    _register(idx, m, more, np.arange(more.size, dtype=np.uint32) + 100_000)
    assert idx.stats()[2] > cap_before and idx.stats()[0] == len(m.d)
    ask = np.concatenate([ask, more[::3]])
    np.testing.assert_array_equal(_u32(idx.lookup(_dk(ask))), m.lookup(ask))
    k, v = idx.export()
    assert dict(zip(k.cpu().numpy().view(np.uint64).tolist(), _u32(v).tolist())) == m.d
    # a grouping over rows that carry those keys
    ek = np.array(list(m.d), np.uint64)
    eh = np.array(list(m.d.values()), np.uint32)
    assert np.all(eh & np.uint32(EXISTING))
    pool = np.concatenate([sc.keys, sc.absent, more[:200]])
    key = pool[rng.integers(0, pool.size, 4000)]
    has = (rng.random(4000) > 0.02).astype(np.uint8)
    import torch
    rep = dedup.group_rows_indexed(_dk(key), torch.from_numpy(has).cuda(),
                                   torch.arange(4000, dtype=torch.int32, device="cuda"), idx, 100)
    np.testing.assert_array_equal(_u32(rep), O.group_reps_existing(key, has, 100, ek, eh))
    idx.close()


# ---- thumbnail table ---------------------------------------------------------------
def _exists(ctx, thumbs, col, has):
    from spacedrive_amd import thumbnailer as T
    return T.thumbnail_exists(dev(thumbs), dev(col), None if has is None else dev(has),
                              ctx=ctx).cpu().numpy()


@CASES
def test_thumbnail_table(ctx, case):
    sc = _scenario(case, HK.cap_join)
    rng = np.random.default_rng(len(sc.name) + 1)
    thumbs = sc.rows
    # the library owns every second thumbnail key; absent keys walk the cluster
    owned = sc.keys[::2]
    col = np.concatenate([np.repeat(owned, 2), np.repeat(sc.absent, 2), sc.keys[1::2][:20]])
    has = np.ones(col.size, np.uint8)
    has[-20:] = 0                                        # keyless rows own nothing
    order = rng.permutation(col.size)
    col, has = col[order], has[order]
    stale, _ = stale_check(ctx, thumbs, even_dirs(thumbs.size, 7), [(col, has)])
    assert stale.size == np.isin(thumbs, sc.keys[1::2]).sum()
    stale_check(ctx, thumbs, even_dirs(thumbs.size, 3), [(col, None), (sc.absent, None)])
    # the work list and thumbnail_exists over a column of present and absent keys
    ask = _asked(sc, rng)
    ahas = (rng.random(ask.size) > 0.05).astype(np.uint8)
    elig = (rng.random(ask.size) > 0.1).astype(np.uint8)
    _, _, stats, present = work_check(ctx, thumbs, ask, ahas, elig)
    np.testing.assert_array_equal(present, (np.isin(ask, sc.keys) & (ahas == 1)).astype(np.uint8))
    assert stats[0] == present.sum() > 0
    work_check(ctx, thumbs, ask)
    np.testing.assert_array_equal(_exists(ctx, thumbs, ask, ahas), present)
    np.testing.assert_array_equal(_exists(ctx, thumbs, ask, None),
                                  work_expected(thumbs, ask)[3])


@pytest.mark.parametrize("cap", [1024, 2048])
def test_thumbnail_filter(ctx, cap):
    """One home slot, eight filter bits: present keys on four of them; absent
    keys on a set bit pass the filter and walk the whole chain, absent keys on a
    clear bit stop at the filter.  A wrong bit index would show as a present
    key reported missing."""
    fs = HK.filter_scenario(cap)
    HK.check_filter_scenario(fs)
    rng = np.random.default_rng(cap)
    thumbs = fs.present if cap == 1024 else np.concatenate(
        [fs.present, HK.keys_at(cap, cap // 2, 520 - fs.present.size, rng)])   # > 512: 2048 slots
    assert HK.cap_join(thumbs.size) == cap
    for absent in (fs.absent_walk, fs.absent_stop, np.concatenate([fs.absent_walk, fs.absent_stop])):
        col = rng.permutation(np.concatenate([fs.present, absent, absent[:10], fs.present[:30]]))
        _, _, stats, present = work_check(ctx, thumbs, col)
        np.testing.assert_array_equal(present, np.isin(col, fs.present).astype(np.uint8))
        assert stats[0] == fs.present.size + 30 and stats[1] == col.size
        assert stats[3] == absent.size                   # one work row per absent key
        np.testing.assert_array_equal(_exists(ctx, thumbs, col, None), present)
        # the sweep: the library owns the absent keys and every third present one
        lib = rng.permutation(np.concatenate([absent, fs.present[::3]]))
        stale, _ = stale_check(ctx, thumbs, even_dirs(thumbs.size, 5), [(lib, None)])
        assert stale.size == thumbs.size - fs.present[::3].size


# ---- indexer ------------------------------------------------------------------------
@CASES
def test_indexer_diff(ctx, case):
    kind, n, sp, cp = case
    sc = _scenario(case, HK.cap_join)
    # the walked directories are a table of their own: scenario (a) there too
    dsc = _scenario(("one_home", 64 if n <= 100 else 300, sp, cp), HK.cap_join)
    rng = np.random.default_rng(len(sc.name) + 2)
    r_key = sc.rows.copy()
    n_r = r_key.size
    r_flags = is_dir_of(r_key)
    r_meta = meta_of(r_key)
    # copies of a key differ in inode, so the state tells which row was matched
    _, first = np.unique(r_key, return_index=True)
    later = np.ones(n_r, bool)
    later[first] = False
    r_meta[later, 0] += np.uint64(1) + np.flatnonzero(later).astype(np.uint64)
    # rows lie in walked directories and in directories that only share their chain
    dirs = np.concatenate([dsc.keys, dsc.absent])
    r_dirkey = dirs[rng.integers(0, dirs.size, n_r)]
    wd_key = dsc.rows
    # on disk: every second present key (the others' rows go where their directory
    # was walked), every absent key (new), copies of both
    w_key = np.concatenate([sc.keys[::2], sc.keys[::4], sc.absent, sc.absent[::2]])
    w_key = rng.permutation(w_key)
    w_flags = is_dir_of(w_key) | ((rng.random(w_key.size) < 0.05).astype(np.uint8) << 1)
    w_meta = meta_of(w_key)
    cols = (w_key, w_flags, w_meta, wd_key, r_key, r_dirkey, r_flags, r_meta)
    create, update, remove, match, state, counts = indexer_check(ctx, cols)
    # match is the LOWEST row of the key, whoever won the slot
    low = {}
    for j, k in enumerate(r_key.tolist()):
        low.setdefault(k, j)
    hit = np.isin(w_key, sc.keys)
    assert [low[k] for k in w_key[hit].tolist()] == match[hit].tolist()
    assert (match[~hit] == 0xFFFFFFFF).all() and update.size == 0
    assert create.size == (~hit).sum() + int(counts[3])
    # no row of a directory that merely shares a chain with a walked one
    assert remove.size > 0 and np.isin(r_dirkey[remove], dsc.keys).all()
    assert not np.isin(r_dirkey[remove], dsc.absent).any()


# ---- op log -----------------------------------------------------------------------
@CASES
def test_oplog(ctx, case):
    sc = _scenario(case, HK.cap_first_call)
    rng = np.random.default_rng(len(sc.name) + 3)
    key = sc.rows
    n = key.size
    ts = rng.integers(-6, 7, n)
    inst = rng.integers(0, 4, n)
    tag = key ^ np.uint64(0x5555)
    every = np.concatenate([sc.keys, sc.absent])
    # ingest, committed
    a = Log(ctx, capacity_hint=1)
    assert a.dev.stats() == (0, 1024)
    _, _, _, counts = a.ingest(key, tag, ts, inst, [0, 3, 0, 9])
    assert counts[2] == sc.keys.size and a.dev.stats() == (sc.keys.size, sc.cap)
    a.check_latest(every)
    # ingest without commit, then add: the same log
    b = Log(ctx, capacity_hint=1)
    apply, applied, _, _ = b.ingest(key, tag, ts, commit=False)
    assert b.dev.stats() == (sc.keys.size, sc.cap)
    b.check_latest(every)
    got, want = b.add(key[applied], tag[applied], ts[applied])
    assert got == want == 0 and a.model == b.model
    b.check_latest(every)
    # add alone; then tags that disagree with the stored ones, counted exactly
    c = Log(ctx, capacity_hint=1)
    got, want = c.add(key, tag, ts)
    assert got == want == 0 and c.dev.stats() == (sc.keys.size, sc.cap)
    c.check_latest(every)
    # (the ops at the scenario's capacity: a page that fits the reserved room)
    room = sc.cap // 2 - sc.keys.size
    if room >= 8:
        again = sc.keys[rng.integers(0, sc.keys.size, room)]
        bad = again ^ np.uint64(0x5555)
        bad[::3] ^= np.uint64(1 << 40)
        got, want = c.add(again, bad, np.zeros(room, np.int64))
        assert got == want == len(range(0, room, 3))
        assert c.dev.stats() == (sc.keys.size, sc.cap)
        _, _, _, counts = a.ingest(again, bad, rng.integers(-9, 9, room), tags_agree=False)
        assert counts[3] == want and a.dev.stats() == (sc.keys.size, sc.cap)
    # a page with the absent keys (they walk the wrapped cluster and enter behind
    # it) and more: growth from a table whose cluster wraps
    more = np.concatenate([sc.absent, rng.integers(1, M64 - 1, sc.cap, dtype=np.uint64), sc.keys])
    more = rng.permutation(more)
    a.ingest(more, more ^ np.uint64(0x5555), rng.integers(-9, 9, more.size),
             rng.integers(0, 4, more.size), [0] * 4)
    stored, cap = a.dev.stats()
    assert cap > sc.cap and stored == len(a.model)
    a.check_latest(np.concatenate([every, more]))
    got, want = a.add(sc.keys, sc.keys ^ np.uint64(0x5555), np.zeros(sc.keys.size, np.int64))
    assert got == want == 0                              # the tags survived the rehash


@pytest.mark.parametrize("hint,cap", [(32768, 1 << 16), (8_388_608, 1 << 24)],
                         ids=["cap_2_16", "cap_2_24"])
def test_oplog_power_of_256_capacity(ctx, hint, cap):
    """At cap = 2^16 / 2^24 the slot numbers 0 .. cap - 1 fit 2 / 3 sort passes
    and the key ~0's slot number, cap, alone needs the next one: without it the
    key ~0's ops would sort among the ops of slot 0."""
    log = Log(ctx, capacity_hint=hint)
    assert log.dev.stats() == (0, cap)
    key, ts, homes, chosen = HK.oplog_page(cap)
    rng = np.random.default_rng(cap)
    inst = rng.integers(0, 5, key.size)
    apply, applied, winners, counts = log.ingest(key, None, ts, inst, [0, 0, 7, 0, 1])
    assert counts[1] == counts[2] == np.unique(key).size
    assert log.dev.stats() == (np.unique(key).size, cap)
    # the key ~0's ops against the oracle once more, by themselves: its first op
    # applies, a later one below the running maximum does not
    sp = np.flatnonzero(key == np.uint64(M64))
    run = np.maximum.accumulate(ts[sp])
    assert apply[sp].tolist() == (ts[sp] >= run).astype(int).tolist() and apply[sp[0]] == 1
    # a second page over the same keys, not committed, then committed
    ts2 = rng.integers(-6, 7, key.size)
    log.ingest(key, None, ts2, commit=False)
    log.ingest(key[::-1].copy(), None, ts2, inst, [0] * 5)
    assert log.dev.stats() == (np.unique(key).size, cap)
    log.check_latest(np.concatenate([chosen, np.array([0, M64, 12345], np.uint64)]))
    log.dev.close()
