"""GPU: flag patterns at the seams of the shared 4096-position tile compaction
(csrc/compact_device.hpp), through every single-GPU feature that lists with
it: orphan Objects, stale thumbnails, the indexer diff's three lists, the sync
ingest's two, and the link batch's two.

The feature tests cover sizes with random contents.  Here the listed positions
are chosen: none, all, only the last, only 4095 (the last of tile 0), only 4096
(the first of tile 1), and every 65th, which makes the ballot of every wave
and row step a different one.  n: 1, one wave, one tile, one tile and one
position, two tiles and one position.  A pattern that needs a position past n
has no case.  Lists, their lengths and the per-list counts are compared
exactly with the oracles the feature tests use (plain numpy for orphans and
the link batch), and the list under test with the chosen positions themselves.
Every call goes through the helpers of its feature's own test file."""
import numpy as np
import pytest

from tests import test_gpu_indexer_diff as GI
from tests import test_gpu_stale_thumbnails as GT
from tests import test_gpu_sync_ingest as GS

pytestmark = pytest.mark.gpu

SIZES = (1, 64, 4096, 4097, 8193)
PATTERNS = {
    "none": lambda n: [],
    "all": lambda n: range(n),
    "last": lambda n: [n - 1],
    "only4095": lambda n: [4095],
    "only4096": lambda n: [4096],
    "every65th": lambda n: range(0, n, 65),
}
CASES = [pytest.param(n, name, id=f"{n}-{name}") for n in SIZES for name, f in PATTERNS.items()
         if all(p < n for p in f(n))]


def mask_of(n, name):
    m = np.zeros(n, bool)
    m[list(PATTERNS[name](n))] = True
    return m


def distinct_keys(seed, count):
    """Distinct odd keys below 2^63: none is 0 or ~0."""
    rng = np.random.default_rng(seed)
    keys = np.unique(rng.integers(1, 2**62, count + count // 8 + 16, dtype=np.uint64) * np.uint64(2)
                     + np.uint64(1))
    assert keys.size >= count
    return rng.permutation(keys)[:count]


@pytest.mark.parametrize("n,name", CASES)
def test_orphan_objects(ctx, n, name):
    import torch
    from spacedrive_amd import consumers
    m = mask_of(n, name)
    objs = (np.arange(n, dtype=np.int32) * 3 + 7)       # ids are not positions
    fp = np.concatenate([objs[~m], np.full(5, -1, np.int32), objs[~m][::2]]).astype(np.int32)
    want = objs[m]
    d_obj, d_fp = torch.from_numpy(objs).cuda(), torch.from_numpy(fp).cuda()
    got = consumers.orphan_objects(d_obj, d_fp, int(objs.max()), ctx)
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    out, cnt = consumers.orphan_objects(d_obj, d_fp, int(objs.max()), ctx, trim=False)
    assert int(cnt.item()) == want.size
    np.testing.assert_array_equal(out[:want.size].cpu().numpy(), want)


@pytest.mark.parametrize("n,name", CASES)
def test_stale_thumbnails(ctx, n, name):
    m = mask_of(n, name)
    keys = distinct_keys(n, n + 40)
    thumbs, foreign = keys[:n], keys[n:]
    owned = np.concatenate([thumbs[~m][::-1], foreign, thumbs[~m][:7]])
    stale, start = GT.check(ctx, thumbs, GT.even_dirs(n, 3), [(owned, None)])
    np.testing.assert_array_equal(stale, np.flatnonzero(m))
    assert start[-1] == m.sum()


@pytest.mark.parametrize("which", ["create", "update", "remove"])
@pytest.mark.parametrize("n,name", CASES)
def test_indexer_diff(ctx, n, name, which):
    """The chosen positions on one of the three lists; the other two hold a few
    entries as well, so the list's tiles do not start the one scan."""
    m = mask_of(n, name)
    keys = distinct_keys(n + 1, 2 * n + 20)
    dirs = np.array([11, 13], np.uint64)
    other = ~m & (np.arange(n) % 7 == 1)                 # on the other walked-entry list
    if which == "remove":
        # n rows in a walked directory: the chosen ones have no entry; a few
        # entries changed, a few new
        r_key = keys[:n]
        w_key = np.concatenate([r_key[~m], keys[n:n + 9]])
        changed = np.concatenate([other[~m], np.zeros(9, bool)])
        r_dirkey = np.full(n, dirs[0], np.uint64)
    else:
        # n entries: the chosen ones new (create) or changed (update), the
        # `other` ones the opposite; ten rows of a walked directory have no entry
        new = m if which == "create" else other
        changed = other if which == "create" else m
        w_key = keys[:n]
        r_key = np.concatenate([keys[n:n + 10], w_key[~new]])
        r_dirkey = np.concatenate([np.full(10, dirs[0], np.uint64),
                                   np.full(r_key.size - 10, dirs[1], np.uint64)])
    w_meta, r_meta = GI.meta_of(w_key), GI.meta_of(r_key)
    w_meta[changed, 0] += np.uint64(1)                   # another inode
    cols = (w_key, np.zeros(w_key.size, np.uint8), w_meta, dirs[:1], r_key, r_dirkey,
            np.zeros(r_key.size, np.uint8), r_meta)
    got = dict(zip(GI.NAMES, GI.check(ctx, cols)))
    np.testing.assert_array_equal(got[which], np.flatnonzero(m))
    assert got["counts"][GI.NAMES.index(which)] == m.sum()
    assert all(got["counts"][i] == got[GI.NAMES[i]].size for i in range(3))


@pytest.mark.parametrize("lists", ["applied_and_winner", "winner_of_chains"])
@pytest.mark.parametrize("n,name", CASES)
def test_sync_ingest(ctx, n, name, lists):
    """applied_and_winner: one key per op, logged at 10; the chosen ops come
    with 20, the others with 5: both lists are the chosen positions.
    winner_of_chains: every op up to the last chosen one shares the key of the
    next chosen position, timestamps ascending: all of them apply, the chosen
    ones win; the ops behind are old."""
    m = mask_of(n, name)
    chosen = np.flatnonzero(m)
    keys = distinct_keys(n + 2, n)
    log = GS.Log(ctx)
    if lists == "applied_and_winner":
        bad, want_bad = log.add(keys, keys, np.full(n, 10))
        assert bad == want_bad == 0
        key, ts = keys, np.where(m, 20, 5)
        want_applied = chosen
    else:
        chained = np.arange(n) <= (chosen[-1] if chosen.size else -1)
        if (~chained).any():
            old = keys[~chained]
            bad, want_bad = log.add(old, old, np.full(old.size, 10))
            assert bad == want_bad == 0
        key = keys.copy()
        key[chained] = keys[chosen[np.searchsorted(chosen, np.flatnonzero(chained))]]
        ts = np.where(chained, np.arange(n), 5)
        want_applied = np.flatnonzero(chained)
    _, applied, winners, counts = log.ingest(key, None, ts)
    np.testing.assert_array_equal(applied, want_applied)
    np.testing.assert_array_equal(winners, chosen)
    assert counts[0] == want_applied.size and counts[1] == chosen.size


@pytest.mark.parametrize("which", ["create", "link"])
@pytest.mark.parametrize("n,name", CASES)
def test_link_batch(ctx, n, name, which):
    """The chosen rows create (rep = own rank) and the others connect, or the
    other way round; every eleventh of the others is not valid and is in
    neither list."""
    import torch
    from spacedrive_amd import dedup
    m = mask_of(n, name)
    first_rank = 5
    rank = np.arange(n, dtype=np.uint32) + np.uint32(first_rank)
    creates = m if which == "create" else ~m
    rep = np.where(creates, rank, rank + np.uint32(1)).astype(np.uint32)
    valid = (m | (np.arange(n) % 11 != 3)).astype(np.uint8)
    want_c = rank[creates & (valid != 0)]
    links = ~creates & (valid != 0)
    d_rep = torch.from_numpy(rep.view(np.int32)).cuda()
    d_valid = torch.from_numpy(valid).cuda()
    c, lr, lo = dedup.link_batch_device(d_rep, None, d_valid, first_rank, ctx=ctx)
    np.testing.assert_array_equal(c.cpu().numpy().view(np.uint32), want_c)
    np.testing.assert_array_equal(lr.cpu().numpy().view(np.uint32), rank[links])
    np.testing.assert_array_equal(lo.cpu().numpy().view(np.uint32), rep[links])
    chosen = rank[m]
    got = (c if which == "create" else lr).cpu().numpy().view(np.uint32)
    np.testing.assert_array_equal(got, chosen)
    c2, lr2, lo2, cnt = dedup.link_batch_device(d_rep, None, d_valid, first_rank, ctx=ctx,
                                                trim=False)
    assert cnt.cpu().numpy().view(np.uint32).tolist() == [want_c.size, int(links.sum())]
    np.testing.assert_array_equal(c2[:want_c.size].cpu().numpy().view(np.uint32), want_c)
    np.testing.assert_array_equal(lr2[:int(links.sum())].cpu().numpy().view(np.uint32), rank[links])
