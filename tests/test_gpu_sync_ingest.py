"""GPU: sdgpu_sync_ingest_device, sdgpu_oplog_add_device and
sdgpu_oplog_latest_device against tests/sync_oracle.py.  Every output of every
case is compared exactly with ingest_keys -- apply, the two lists, the counts,
the clocks and `latest` of every touched key afterwards -- and the two list
buffers, filled with a sentinel beforehand, must be untouched past their
lengths.

The sort and the segmented scan work in tiles of TILE = 2048 ops, the list
compaction in tiles of 4096.  The sort takes one pass per 8 bits of a slot
number 0 .. capacity: 2 passes up to 2^15 slots (capacity_hint 1 gives 1024),
3 up to 2^23 (capacity_hint 100 000 gives 2^18), 4 beyond (capacity_hint
9 000 000 gives 2^25)."""
import ctypes

import numpy as np
import pytest

from tests import sync_oracle as SO

pytestmark = pytest.mark.gpu

TILE = 2048
POISON32 = 0xA5A5A5A5
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
ALL_ONES = (1 << 64) - 1


def _dev(a, dtype=None):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a.copy()).cuda()


class Log:
    """A device log and the oracle's model of it, kept side by side."""

    def __init__(self, ctx, capacity_hint=1):
        from spacedrive_amd.sync import OpLog
        self.dev = OpLog(capacity_hint, ctx)
        self.ctx = ctx
        self.model = {}

    def add(self, key, tag, ts):
        key, tag, ts = (np.asarray(key, dtype=np.uint64), np.asarray(tag, dtype=np.uint64),
                        np.asarray(ts, dtype=np.int64))
        got = self.dev.add(_dev(key), _dev(tag), _dev(ts))
        want, self.model = SO.add_keys(key, tag, ts, self.model)
        return got, want

    def check_latest(self, keys):
        keys = np.unique(np.asarray(keys, dtype=np.uint64))
        ts, found = self.dev.latest(_dev(keys))
        want_ts, want_found = SO.latest_keys(keys, self.model)
        assert np.array_equal(found.cpu().numpy(), want_found)
        assert np.array_equal(ts.cpu().numpy(), want_ts)

    def ingest(self, key, tag, ts, instance=None, clock=None, commit=True, tags_agree=True):
        """One page through the C entry point with sentinel-filled buffers; every
        output against ingest_keys.  Returns (apply, applied, winners, counts)."""
        import torch
        key = np.asarray(key, dtype=np.uint64)
        tag = key if tag is None else np.asarray(tag, dtype=np.uint64)
        ts = np.asarray(ts, dtype=np.int64)
        n = key.size
        want = SO.ingest_keys(key, tag, ts, instance, clock, self.model, commit)
        w_apply, w_applied, w_winners, w_counts, w_clock, self.model = want
        dk, dt, dts = _dev(key), _dev(tag), _dev(ts)
        d_apply = torch.full((n + 1,), 0xA5, dtype=torch.uint8, device="cuda")
        d_applied = torch.full((n + 1,), POISON32 - (1 << 32), dtype=torch.int32, device="cuda")
        d_winner = d_applied.clone()
        d_counts = torch.full((4,), POISON32 - (1 << 32), dtype=torch.int32, device="cuda")
        # one entry more than n: an empty page still has a pointer to give
        d_inst = None if instance is None else _dev(np.append(np.asarray(instance, dtype=np.uint32),
                                                              np.uint32(0)))
        d_clock = None if clock is None else _dev(np.asarray(clock, dtype=np.uint64))
        p = lambda t: t.data_ptr() if t is not None and t.numel() else None  # noqa: E731
        rc = self.ctx.lib.sdgpu_sync_ingest_device(
            self.dev.h, p(dk), p(dt), p(dts), None if d_inst is None else d_inst.data_ptr(), n,
            None if d_clock is None else d_clock.data_ptr(), 0 if clock is None else len(clock),
            0 if commit else 1, d_apply.data_ptr(), d_applied.data_ptr(), d_winner.data_ptr(),
            d_counts.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc
        counts = d_counts.cpu().numpy().view(np.uint32)
        apply = d_apply.cpu().numpy()
        applied = d_applied.cpu().numpy().view(np.uint32)
        winners = d_winner.cpu().numpy().view(np.uint32)
        if tags_agree:
            assert w_counts[3] == 0
            assert np.array_equal(counts, w_counts), (counts, w_counts)
        else:
            assert np.array_equal(counts[:3], w_counts[:3]) and counts[3] > 0 and w_counts[3] > 0
        assert np.array_equal(apply[:n], w_apply) and apply[n] == 0xA5
        assert np.array_equal(applied[:counts[0]], w_applied)
        assert np.array_equal(winners[:counts[1]], w_winners)
        # nothing is written past the two lengths
        assert (applied[counts[0]:] == POISON32).all() and (winners[counts[1]:] == POISON32).all()
        if clock is not None:
            assert d_clock.cpu().numpy().view(np.uint64).tolist() == w_clock
        self.check_latest(key)
        return apply[:n], applied[:counts[0]], winners[:counts[1]], counts


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 1,
                               3 * TILE + 1, 4095, 4096, 4097, 8193])   # 4096: the lists' tile
def test_sizes_few_keys_many_ties(ctx, n):
    rng = np.random.default_rng(n)
    log = Log(ctx)
    key = rng.integers(0, max(n // 3, 1) + 1, n).astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    ts = rng.integers(-3, 4, n)
    inst = rng.integers(0, 5, n)
    log.ingest(key, None, ts, inst, [0, 7, 0, ALL_ONES - 1, 3])
    # the same page re-delivered: ops at their key's maximum apply again
    _, applied, _, _ = log.ingest(key, None, ts, inst, [0] * 5)
    assert n == 0 or applied.size > 0


def test_all_keys_distinct_and_every_key_twice(ctx):
    rng = np.random.default_rng(2)
    n = 3 * TILE + 77
    key = rng.permutation(n).astype(np.uint64) + np.uint64(1 << 40)
    log = Log(ctx)
    apply, _, winners, counts = log.ingest(key, None, rng.integers(-9, 9, n))
    assert apply.all() and counts[1] == n and counts[2] == n
    twice = np.concatenate([key, key])[rng.permutation(2 * n)]
    log = Log(ctx)
    _, _, winners, counts = log.ingest(twice, None, rng.integers(-2, 3, 2 * n))
    assert counts[1] == n and counts[2] == n


@pytest.mark.parametrize("order", ["ascending", "descending", "constant", "random5"])
def test_one_key_for_all_ops(ctx, order):
    """One segment over ten tiles of the scan."""
    n = 20_000
    rng = np.random.default_rng(5)
    ts = {"ascending": np.arange(n) - 7, "descending": -np.arange(n), "constant": np.full(n, 42),
          "random5": rng.integers(0, 5, n)}[order]
    log = Log(ctx)
    apply, applied, winners, counts = log.ingest(np.full(n, 0xABCDEF, dtype=np.uint64), None, ts,
                                                 rng.integers(0, 3, n), [0, 0, 0])
    assert counts[1] == 1 and counts[2] == 1
    assert counts[0] == {"ascending": n, "descending": 1, "constant": n}.get(order, counts[0])
    # a second page below, at and above the logged maximum
    top = int(ts.max())
    log.ingest(np.full(3, 0xABCDEF, dtype=np.uint64), None, [top - 1, top, top + 1])


def test_hot_keys_among_singletons(ctx):
    rng = np.random.default_rng(6)
    single = rng.permutation(50_000).astype(np.uint64) + np.uint64(1000)
    hot = rng.integers(0, 10, 30_000).astype(np.uint64)
    key = np.concatenate([single, hot])[rng.permutation(80_000)]
    log = Log(ctx, capacity_hint=100_000)            # 2^18 slots: three sort passes
    assert log.dev.stats() == (0, 1 << 18)
    _, _, _, counts = log.ingest(key, None, rng.integers(-50, 50, key.size),
                                 rng.integers(0, 2000, key.size), [0] * 1500)   # clocks past LDS
    assert counts[1] == 50_010 and log.dev.stats() == (50_010, 1 << 18)


def test_special_keys_and_extreme_timestamps(ctx):
    """Keys 0 and ~0 on both sides; timestamps at the ends of int64; t equal to
    the logged maximum."""
    vals = [I64_MIN, -1, 0, 1, I64_MAX]
    log = Log(ctx)
    pre = np.array([0, ALL_ONES, 5, 5, 6, 7], dtype=np.uint64)
    got, want = log.add(pre, pre, [3, -1, I64_MIN, 0, I64_MAX, I64_MIN])
    assert got == want == 0
    log.check_latest([0, ALL_ONES, 5, 6, 7, 8])
    assert log.dev.stats()[0] == 5
    rng = np.random.default_rng(8)
    keys = np.array([0, ALL_ONES, 5, 6, 7, 8, 9], dtype=np.uint64)
    key = keys[rng.integers(0, keys.size, 700)]
    ts = np.array(vals, dtype=np.int64)[rng.integers(0, 5, 700)]
    # the clock takes the unsigned order: -1 is the largest NTP64
    apply, _, _, counts = log.ingest(key, None, ts, rng.integers(0, 4, 700), [0, 1 << 63, 5])
    assert counts[2] == 2 and log.dev.stats()[0] == 7
    # equal to the logged maximum applies, one below does not
    apply, _, _, _ = log.ingest(np.array([0, 0, ALL_ONES, ALL_ONES], dtype=np.uint64), None,
                                [I64_MAX, I64_MAX - 1, I64_MAX, I64_MAX - 1])
    assert apply.tolist() == [1, 0, 1, 0]
    # a key that only ever saw INT64_MIN: applied, and still without a timestamp
    log2 = Log(ctx)
    apply, _, _, _ = log2.ingest(np.array([0, ALL_ONES, 3], dtype=np.uint64), None, [I64_MIN] * 3)
    assert apply.all()
    ts, found = log2.dev.latest(_dev(np.array([0, ALL_ONES, 3], dtype=np.uint64)))
    assert not found.any() and (ts == I64_MIN).all()


def test_signed_apply_unsigned_clock(ctx):
    """The pinned case: t = 2^63 (stored as INT64_MIN) is older than t = 1 for
    the op log, newer for the clock."""
    log = Log(ctx)
    apply, _, winners, _ = log.ingest(np.array([4, 4], dtype=np.uint64), None, [1, I64_MIN],
                                      [0, 0], [0])
    assert apply.tolist() == [1, 0] and winners.tolist() == [0]


def test_clocks(ctx):
    rng = np.random.default_rng(9)
    n = 5000
    key = rng.integers(0, 100, n).astype(np.uint64)
    ts = rng.integers(-1000, 1000, n)
    log = Log(ctx)
    log.ingest(key, None, ts, rng.integers(0, 9, n), [0, 5, 1 << 62])     # indices past the end
    log.ingest(key, None, ts)                                             # both NULL
    import torch
    one = torch.zeros(4, dtype=torch.int64, device="cuda")
    with pytest.raises(OSError):                                          # exactly one of the two
        from spacedrive_amd._native import check
        check(ctx.lib.sdgpu_sync_ingest_device(log.dev.h, one.data_ptr(), one.data_ptr(),
                                               one.data_ptr(), one.data_ptr(), 4, None, 0, 0,
                                               one.data_ptr(), one.data_ptr(), one.data_ptr(),
                                               one.data_ptr(), None))


def test_preloaded_log_and_three_pages(ctx):
    rng = np.random.default_rng(10)
    pool = rng.integers(0, 1 << 63, 3000).astype(np.uint64)
    log = Log(ctx)
    rows = pool[rng.integers(0, 2000, 9000)]                 # duplicates in any order
    got, want = log.add(rows, rows, rng.integers(-100, 100, rows.size))
    assert got == want == 0
    log.check_latest(pool)
    for page in range(3):
        key = pool[rng.integers(0, 3000, 2500)]
        log.ingest(key, None, rng.integers(-120, 120, key.size), rng.integers(0, 3, key.size),
                   [0, 0, 0])
    log.check_latest(pool)


def test_pages_of_1000_equal_one_page(ctx):
    rng = np.random.default_rng(11)
    key = rng.integers(0, 400, 5000).astype(np.uint64)
    ts = rng.integers(-30, 30, 5000)
    whole, paged = Log(ctx), Log(ctx)
    apply, _, _, _ = whole.ingest(key, None, ts)
    parts = [paged.ingest(key[a:a + 1000], None, ts[a:a + 1000])[0] for a in range(0, 5000, 1000)]
    assert np.array_equal(np.concatenate(parts), apply) and whole.model == paged.model


def test_no_commit_then_add(ctx):
    rng = np.random.default_rng(12)
    key = rng.integers(0, 300, 4000).astype(np.uint64)
    ts = rng.integers(-40, 40, 4000)
    pre = np.arange(0, 300, 2, dtype=np.uint64)
    a, b = Log(ctx), Log(ctx)
    for log in (a, b):
        log.add(pre, pre, rng.integers(-10, 10, pre.size) * 0 + 3)
    before = {k: list(v) for k, v in a.model.items()}
    apply, applied, _, _ = a.ingest(key, None, ts, commit=False)
    # `latest` is unchanged (ingest checked it against the model); the model
    # only gained keys without a timestamp
    assert {k: v for k, v in a.model.items() if v[0] is not None} == before
    got, want = a.add(key[applied], key[applied], ts[applied])
    assert got == want == 0
    apply_b, _, _, _ = b.ingest(key, None, ts, commit=True)
    assert np.array_equal(apply, apply_b) and a.model == b.model
    a.check_latest(np.arange(300))
    b.check_latest(np.arange(300))


def test_growth_from_the_smallest_table(ctx):
    rng = np.random.default_rng(13)
    key = rng.permutation(200_000).astype(np.uint64) * np.uint64(0x100000001B3) + np.uint64(17)
    tag = key ^ np.uint64(0x5555)
    ts = rng.integers(I64_MIN, I64_MAX, key.size)
    log = Log(ctx, capacity_hint=1)
    assert log.dev.stats() == (0, 1024)                      # two sort passes
    for a in range(0, 200_000, 50_000):
        log.ingest(key[a:a + 50_000], tag[a:a + 50_000], ts[a:a + 50_000])
    stored, cap = log.dev.stats()
    assert stored == 200_000 and cap >= 400_000
    log.check_latest(key)                                    # timestamps survived the rehashes
    got, want = log.add(key[::7], tag[::7], ts[::7])          # and so did the tags
    assert got == want == 0
    got, want = log.add(key[:100], key[:100], ts[:100])
    assert got == want == 100


def test_widest_slot_numbers(ctx):
    """capacity_hint 9 000 000: 2^25 slots, 26-bit slot numbers, four sort passes."""
    rng = np.random.default_rng(14)
    log = Log(ctx, capacity_hint=9_000_000)
    assert log.dev.stats() == (0, 1 << 25)
    key = rng.integers(0, 1 << 63, 3000).astype(np.uint64)
    key = np.concatenate([key, [0, ALL_ONES]]).astype(np.uint64)[rng.integers(0, 3002, 3 * TILE + 5)]
    log.ingest(key, None, rng.integers(-5, 5, key.size))
    log.ingest(key, None, rng.integers(-6, 6, key.size), rng.integers(0, 2, key.size), [0, 0])


def test_tags(ctx):
    log = Log(ctx)
    key = np.array([11, 12, 11, 13], dtype=np.uint64)
    # two tuples with one key in one page
    _, _, _, counts = log.ingest(key, [1, 2, 9, 3], [0, 0, 0, 0], tags_agree=False)
    # and across pages (the stored tag of 12 is 2, of 13 is 3)
    _, _, _, counts = log.ingest(np.array([12, 13], dtype=np.uint64), [2, 4], [1, 1],
                                 tags_agree=False)
    assert counts[3] == 1
    log2 = Log(ctx)
    log2.add([21, 22], [1, 2], [0, 0])
    got, want = log2.add([21, 22, 22], [1, 3, 2], [5, 5, 5])
    assert got == want == 1
    _, _, _, counts = log2.ingest(np.array([21, 22], dtype=np.uint64), [1, 2], [9, 9])
    assert counts[3] == 0


def test_wrapper_and_host_variant(ctx):
    from spacedrive_amd import sync as S
    rng = np.random.default_rng(15)
    n = 2 * TILE + 9
    key = rng.integers(0, 500, n).astype(np.uint64)
    ts = rng.integers(-20, 20, n)
    inst = rng.integers(0, 4, n)
    want = SO.ingest_keys(key, key, ts, inst, [0, 0, 9])
    log = S.OpLog(0, ctx)
    import torch
    clock = torch.tensor([0, 0, 9], dtype=torch.int64, device="cuda")
    apply, applied, winner, counts = log.ingest(_dev(key), _dev(key), _dev(ts),
                                                _dev(inst.astype(np.uint32)), clock)
    assert np.array_equal(apply.cpu().numpy(), want[0])
    assert np.array_equal(applied.cpu().numpy().view(np.uint32), want[1])
    assert np.array_equal(winner.cpu().numpy().view(np.uint32), want[2])
    assert counts.tolist() == want[3].tolist()
    assert [c & ALL_ONES for c in clock.tolist()] == want[4]      # the NTP64 bits
    host_log = S.OpLog(0, ctx)
    hclock = np.array([0, 0, 9], dtype=np.uint64)
    apply, applied, winner, counts = S.ingest_host(host_log, key, key, ts, inst, hclock)
    assert np.array_equal(apply, want[0]) and np.array_equal(applied, want[1])
    assert np.array_equal(winner, want[2]) and np.array_equal(counts, want[3])
    assert hclock.tolist() == want[4]
    lts, found = host_log.latest(_dev(np.arange(500, dtype=np.uint64)))
    wts, wfound = SO.latest_keys(np.arange(500, dtype=np.uint64), want[5])
    assert np.array_equal(lts.cpu().numpy(), wts) and np.array_equal(found.cpu().numpy(), wfound)
    host_log.clear()
    assert host_log.stats()[0] == 0
    assert not host_log.latest(_dev(np.arange(500, dtype=np.uint64)))[1].any()
    counts = (ctypes.c_uint32 * 4)(7, 7, 7, 7)
    assert ctx.lib.sdgpu_sync_ingest(host_log.h, None, None, None, None, 0, None, 0, 0, None,
                                     None, None, ctypes.cast(counts, ctypes.c_void_p)) == 0
    assert not any(counts)
