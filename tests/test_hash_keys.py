"""CPU: tests/hash_keys.py -- the inverse of row_hash, the key constructors, and
the premise of every scenario the GPU tests build from them (a walk crosses the
end of the table, a chain is as long as the keys placed at its home, present
and absent keys share home slot and filter bit, two hashes differ in exactly
one bit).  The GPU tests call the same builders, so a scenario cannot lose its
edge unnoticed."""
import numpy as np
import pytest

from oracle import oracle as O
from spacedrive_amd import dedup
from tests import hash_keys as HK

M64 = HK.M64


def test_unmix_inverts_mix():
    rng = np.random.default_rng(1)
    h = rng.integers(0, M64, 100_000, dtype=np.uint64, endpoint=True)
    edge = np.array([0, M64] + [1 << b for b in range(64)] + [M64 ^ (1 << b) for b in range(64)],
                    np.uint64)
    for v in (h, edge):
        assert np.array_equal(O.mix64(HK.unmix64(v)), v)
        assert np.array_equal(HK.unmix64(O.mix64(v)), v)
        assert np.array_equal(HK.mix64(v), O.mix64(v))


def test_constants():
    assert int(O.mix64(np.array([0], np.uint64))[0]) == 0
    assert int(HK.unmix64(M64)[0]) == HK.KEY_HASH_ALL_ONES == 0xCF9A04AFFA6BADC0
    assert int(O.mix64(np.array([M64], np.uint64))[0]) == HK.HASH_OF_ALL_ONES == 0xB4D055FCF2CBBD7B
    k = np.array([HK.KEY_HASH_ALL_ONES], np.uint64)
    # the last slot, shard 255, highest digit, last LDS slot, largest step
    assert int(O.mix64(k)[0]) == M64
    assert int(dedup.shard_of(k)[0]) == 255 and int(HK.digit_of(k, 15)[0]) == (1 << 15) - 1
    assert int(HK.lds_slot(M64)[0]) == 6143 and int(HK.lds_step(M64)[0]) == 6139
    assert int(HK.pk_slot(M64)[0]) == 8191 and int(HK.pk_step(M64)[0]) == 8191
    assert int(HK.lds_slot(0)[0]) == 0 and int(HK.lds_step(0)[0]) == 1
    assert int(HK.pk_slot(0)[0]) == 0 and int(HK.pk_step(0)[0]) == 1


@pytest.mark.parametrize("cap,slot", [(1024, 1023), (1024, 0), (2048, 1023), (1 << 16, 255),
                                      (1 << 24, (1 << 24) - 1)])
def test_keys_at(cap, slot):
    rng = np.random.default_rng(cap + slot)
    k = HK.keys_at(cap, slot, 700, rng)
    assert k.dtype == np.uint64 and np.unique(k).size == 700
    assert np.all(O.mix64(k) & np.uint64(cap - 1) == np.uint64(slot))
    assert not np.isin(k, np.array([0, M64], np.uint64)).any()
    assert np.unique(O.mix64(k) >> np.uint64(40)).size > 600      # the other bits are random
    again = HK.keys_at(cap, slot, 700, np.random.default_rng(cap + slot))
    assert np.array_equal(k, again)                               # reproducible


def test_keys_with_hash_fields():
    rng = np.random.default_rng(3)
    k = HK.keys_with_hash(300, rng, shard=85)
    assert np.unique(k).size == 300 and np.all(dedup.shard_of(k) == 85)
    assert np.unique(HK.digit_of(k, 12)).size > 200
    k = HK.keys_with_hash(300, rng, digit=(1 << 13) - 1, digit_bits=13)
    assert np.unique(k).size == 300 and np.all(HK.digit_of(k, 13) == (1 << 13) - 1)
    assert np.all(HK.digit_of(k, 4) == 15) and np.unique(dedup.shard_of(k)).size > 100
    k = HK.keys_with_hash(300, rng, lo32=0xDEADBEEF)
    assert np.all(O.mix64(k) & np.uint64(0xFFFFFFFF) == np.uint64(0xDEADBEEF))


@pytest.mark.parametrize("lo32", [HK.LO32_LAST, HK.LO32_FIRST, 0x80001234])
def test_slot_step_family(lo32):
    """512 keys: one bucket under every plan, one first slot, one step -- in the
    6144-slot table and in the packed 8192-slot one."""
    k = HK.slot_step_family(lo32)
    h = O.mix64(k)
    assert k.size == 512 and np.unique(k).size == 512
    for bits in (1, 5, 6, 12, 13, 14, 15):
        assert np.unique(HK.digit_of(k, bits)).size == 1
    assert np.unique(dedup.shard_of(k)).size == 1
    assert np.unique(HK.lds_slot(h)).size == 1 and np.unique(HK.lds_step(h)).size == 1
    assert np.unique(HK.pk_slot(h)).size == 1 and np.unique(HK.pk_step(h)).size == 1
    # exactly the 9 bits 32..40 vary, and take every value
    assert np.unique((h >> np.uint64(32)) & np.uint64(511)).size == 512
    assert np.unique(h & np.uint64(~(511 << 32) & M64)).size == 1
    if lo32 == HK.LO32_LAST:
        assert int(HK.lds_slot(h)[0]) == 6143 and int(HK.lds_step(h)[0]) == 6139
        assert int(HK.pk_slot(h)[0]) == 8191 and int(HK.pk_step(h)[0]) == 8191
    if lo32 == HK.LO32_FIRST:
        assert int(HK.lds_slot(h)[0]) == 0 and int(HK.lds_step(h)[0]) == 1
        assert int(HK.pk_slot(h)[0]) == 0 and int(HK.pk_step(h)[0]) == 1
    # the steps visit every slot: coprime with 6144, odd for 8192
    assert np.gcd(int(HK.lds_step(h)[0]), 6144) == 1 and int(HK.pk_step(h)[0]) % 2 == 1
    # in the global table (a power of two of at most 2^32 slots) one home slot
    assert np.unique(h & np.uint64(0xFFFFFFFF)).size == 1


@pytest.mark.parametrize("base", [0, M64, 0x9E3779B97F4A7C15])
def test_one_bit_family(base):
    k = HK.one_bit_family(base)
    h = O.mix64(k)
    assert k.size == 65 and np.unique(k).size == 65 and int(h[0]) == base
    diff = h[1:] ^ h[0]
    assert sorted(int(d).bit_length() - 1 for d in diff) == list(range(64))
    assert all(bin(int(d)).count("1") == 1 for d in diff)          # exactly one differing bit
    if base == M64:
        assert int(k[0]) == HK.KEY_HASH_ALL_ONES


@pytest.mark.parametrize("cap_of", [HK.cap_join, HK.cap_first_call], ids=["join", "first_call"])
@pytest.mark.parametrize("case", HK.TABLE_CASES, ids=HK.case_id)
def test_table_scenarios(case, cap_of):
    kind, n, sp, cp = case
    sc = HK.table_scenario(kind, n, sp, cp, cap_of)
    assert sc.cap == cap_of(sc.rows.size) and sc.cap >= 1024
    p = HK.check_table_scenario(sc)
    if kind == "one_home" and not sp:
        assert p.longest == n - 1 and p.crossed == n - 1
    if kind == "straddle":
        # the keys homed at 0..2 are pushed forward by the wrapped cluster (which
        # key ends where depends on the order; the taken slots do not): one
        # run of taken slots from cap - 3 across the end
        for s in (0, 1, 2):
            at = p.slot[np.isin(sc.keys, sc.homes[s])]
            assert at.size == 8 and (at > s).sum() >= 7
        taken = [i for i, k in enumerate(p.table) if k is not None]
        run = sc.ordinary.size + (1 if sp else 0)
        assert sorted(taken) == sorted((sc.cap - 3 + j) % sc.cap for j in range(run))
    if sp:
        assert M64 in sc.keys.tolist() and 0 in sc.keys.tolist()
    if cp:
        _, cnt = np.unique(sc.rows, return_counts=True)
        assert cnt.min() >= 2 and cnt.max() <= 5
    if not cp and n <= 512:
        assert sc.cap == 1024                                     # the smallest table there is
    # random placement, for comparison, reaches none of this (the issue's figures)
    rnd = HK.place(np.random.default_rng(7).integers(1, M64, 1024, dtype=np.uint64), 2048)
    assert rnd.longest < 40


def test_same_scenario_every_time():
    a = HK.table_scenario("straddle", 200, True, True, HK.cap_join)
    b = HK.table_scenario("straddle", 200, True, True, HK.cap_join)
    assert np.array_equal(a.rows, b.rows) and np.array_equal(a.absent, b.absent)


@pytest.mark.parametrize("cap", [1024, 2048])
def test_filter_scenario(cap):
    fs = HK.filter_scenario(cap)
    HK.check_filter_scenario(fs)
    assert fs.home == cap - 1
    # a key's filter bit is its home slot plus cap times the three bits above it
    hb = HK.filter_bit(fs.present, cap)
    assert set((hb - fs.home) // cap) == set(HK.SET_BITS)


@pytest.mark.parametrize("cap", [1 << 16, 1 << 24])
def test_oplog_page_needs_the_extra_pass(cap):
    """Slot numbers are 0 .. cap: at a power-of-256 capacity the key ~0's slot
    alone has a bit in the next digit."""
    key, ts, homes, chosen = HK.oplog_page(cap)
    assert key.size < 5000 and key.size == ts.size
    assert (key == np.uint64(M64)).sum() >= 18
    sp_ts = ts[key == np.uint64(M64)]
    assert np.unique(sp_ts).size < sp_ts.size and (np.diff(sp_ts) < 0).any()   # ties, disorder
    passes = lambda top: (int(top).bit_length() + 7) // 8  # noqa: E731
    assert passes(cap) == passes(cap - 1) + 1
    for other in (1 << 10, 1 << 18, 1 << 25):
        assert passes(other) == passes(other - 1)
    home = (O.mix64(chosen) & np.uint64(cap - 1)).tolist()
    assert {0, 255, 256, 65535 & (cap - 1), cap - 1} <= set(home)
    assert 0 in key.tolist()


def test_spread_rows():
    rng = np.random.default_rng(5)
    keys = HK.one_bit_family(0x1234)
    extra = rng.integers(1, M64, 5000, dtype=np.uint64)
    rows = HK.spread_rows(keys, 3, rng, extra)
    assert rows.size < 70_000
    for k in keys.tolist():
        at = np.flatnonzero(rows == np.uint64(k))
        assert at.size == 3 and np.unique(at // 100).size == 3
    assert np.isin(extra, rows).all()


@pytest.mark.parametrize("bits", [5, 6, 12, 13, 15])
def test_digit_edges(bits):
    k = HK.digit_edge_keys(bits, 200, np.random.default_rng(bits))
    d = HK.digit_of(k, bits)
    assert np.unique(k).size == 400
    assert (d[:200] == 0).all() and (d[200:] == (1 << bits) - 1).all()
    if bits > 12:            # two-level: the coarse (top bits - 9) and the fine (low 9) digit
        cb = bits - 9
        assert (d[200:] >> 9 == (1 << cb) - 1).all() and (d[200:] & 511 == 511).all()


def test_owner_boundaries():
    k = HK.owner_boundary_keys(300, np.random.default_rng(9))
    s = dedup.shard_of(k)
    assert np.unique(k).size == k.size == 300 * len(HK.OWNER_SHARDS)
    assert sorted(set(s.tolist())) == list(HK.OWNER_SHARDS)
    own = {w: dict(zip(s.tolist(), ((s * w) >> 8).tolist())) for w in (2, 3)}
    assert own[2][127] == 0 and own[2][128] == 1
    assert (own[3][85], own[3][86], own[3][170], own[3][171]) == (0, 1, 1, 2)
    assert own[3][84] == 0 and own[3][255] == 2 and own[2][255] == 1
