"""Keys with chosen hashes (numpy only, no GPU).

Every table and digit of the grouping and join paths is addressed by
row_hash(key), the splitmix64 finaliser of csrc/rows_device.hpp.  It is a
bijection, so a test can choose the hash -- a home slot, a shard byte, a bucket
digit, an LDS slot and step -- and derive the key:

    unmix64(h)          the key whose hash is h
    keys_at             keys that share a home slot of a power-of-two table
    keys_with_hash      keys whose hashes agree on named fields (low word,
                        shard byte, the digit bits below it)
    one_bit_family      a key and the 64 keys one hash bit away from it
    place               a plain model of linear probing: used ONLY to prove
                        that a scenario reaches what it claims (a walk crosses
                        the end, a chain has the promised length), never as the
                        expected result of a kernel
    table_scenario ...  the scenarios of tests/test_gpu_hash_placement.py and
                        tests/test_gpu_group_chosen_hashes.py; the CPU tests
                        (tests/test_hash_keys.py) assert their premises on the
                        same builders
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

M64 = (1 << 64) - 1
ALL_ONES = np.uint64(M64)
KEY_HASH_ALL_ONES = 0xCF9A04AFFA6BADC0     # unmix64(~0): its bucket records read "empty"
HASH_OF_ALL_ONES = 0xB4D055FCF2CBBD7B      # mix64(~0): an ordinary hash


def _u64(x):
    return np.atleast_1d(np.asarray(x, dtype=np.uint64)).copy()


def mix64(k):
    """row_hash: the splitmix64 finaliser, vectorised over uint64."""
    z = _u64(k)
    with np.errstate(over="ignore"):
        z ^= z >> np.uint64(30)
        z *= np.uint64(0xBF58476D1CE4E5B9)
        z ^= z >> np.uint64(27)
        z *= np.uint64(0x94D049BB133111EB)
        z ^= z >> np.uint64(31)
    return z


def unmix64(h):
    """The inverse of mix64, vectorised over uint64: each xor-shift is undone by
    repeating it (x ^= x >> s is inverted by x ^= (x >> s) ^ (x >> 2s) while
    3s >= 64), each multiplication by the constant's inverse mod 2^64."""
    z = _u64(h)
    with np.errstate(over="ignore"):
        z ^= (z >> np.uint64(31)) ^ (z >> np.uint64(62))
        z *= np.uint64(0x319642B2D24D8EC3)
        z ^= (z >> np.uint64(27)) ^ (z >> np.uint64(54))
        z *= np.uint64(0x96DE1B173F119089)
        z ^= (z >> np.uint64(30)) ^ (z >> np.uint64(60))
    return z


def _distinct_hashes(fixed_mask: int, fixed_value: int, count: int, rng) -> np.ndarray:
    """`count` distinct hashes h with h & fixed_mask == fixed_value; the free
    bits random but reproducible (all of them, in order, when count is the
    whole space).  The hashes of the keys 0 and ~0 are never drawn."""
    free = [b for b in range(64) if not (fixed_mask >> b) & 1]
    space = 1 << len(free)
    assert 0 < count <= space, (count, space)
    if len(free) <= 20:                      # enumerate the space
        idx = np.arange(space, dtype=np.uint64)
        if count < space:
            idx = np.sort(rng.choice(space, count, replace=False)).astype(np.uint64)
        h = np.full(idx.size, fixed_value, np.uint64)
        for j, b in enumerate(free):
            h |= ((idx >> np.uint64(j)) & np.uint64(1)) << np.uint64(b)
    else:
        h = np.zeros(0, np.uint64)
        while h.size < count:
            draw = rng.integers(0, M64, 2 * count + 16, dtype=np.uint64, endpoint=True)
            draw = (draw & np.uint64(~fixed_mask & M64)) | np.uint64(fixed_value)
            draw = draw[(draw != np.uint64(0)) & (draw != np.uint64(HASH_OF_ALL_ONES))]
            _, first = np.unique(np.concatenate([h, draw]), return_index=True)
            h = np.concatenate([h, draw])[np.sort(first)]
        h = h[:count]
    assert np.unique(h).size == count
    return h


def keys_at(cap: int, slot: int, count: int, rng) -> np.ndarray:
    """`count` distinct keys whose home slot in a table of `cap` slots (a power
    of two) is `slot`: mix64(key) & (cap - 1) == slot.  None is 0 or ~0."""
    assert cap & (cap - 1) == 0 and 0 <= slot < cap
    return unmix64(_distinct_hashes(cap - 1, slot, count, rng))


def keys_with_hash(count: int, rng, lo32=None, shard=None, digit=None, digit_bits: int = 0):
    """`count` distinct keys whose hashes agree on the named fields and differ
    elsewhere: lo32 = hash bits 0..31 (the LDS slot and step of the group
    tables), shard = bits 56..63 (the owner's byte), digit = the digit_bits
    bits below the shard byte (the bucket digit of every plan of at most
    digit_bits bits).  With lo32, shard and a 15-bit digit fixed, 9 bits
    (32..40) stay free: count = 512 returns the whole family."""
    mask = value = 0
    if lo32 is not None:
        mask |= 0xFFFFFFFF
        value |= int(lo32) & 0xFFFFFFFF
    if shard is not None:
        mask |= 0xFF << 56
        value |= (int(shard) & 0xFF) << 56
    if digit_bits:
        assert digit is not None and 0 <= digit < (1 << digit_bits)
        mask |= ((1 << digit_bits) - 1) << (56 - digit_bits)
        value |= int(digit) << (56 - digit_bits)
    return unmix64(_distinct_hashes(mask, value, count, rng))


def one_bit_family(base_hash: int) -> np.ndarray:
    """65 keys: the key whose hash is base_hash, then for b = 0..63 the key
    whose hash differs from it in bit b alone."""
    h = np.full(65, int(base_hash) & M64, np.uint64)
    h[1:] ^= np.uint64(1) << np.arange(64, dtype=np.uint64)
    return unmix64(h)


def shard_byte(keys):
    return (mix64(keys) >> np.uint64(56)).astype(np.int64)


def digit_of(keys, bits: int):
    """The `bits` hash bits below the shard byte (part_device.hpp digit_of, skip 8)."""
    return ((mix64(keys) << np.uint64(8)) >> np.uint64(64 - bits)).astype(np.int64)


# ---- the group tables' slot and step (group_device.hpp) ---------------------------
LDS_SLOTS, PK_SLOTS = 6144, 8192


def lds_slot(h):
    return ((_u64(h) & np.uint64(0xFFFFFFFF)) * np.uint64(LDS_SLOTS)) >> np.uint64(32)


def lds_step(h):
    return np.uint64(1) + np.uint64(6) * (_u64(h) & np.uint64(1023))


def pk_slot(h):
    """group_packed_regs' sa / 8: the top 13 bits of h lo."""
    return (_u64(h) & np.uint64(0xFFFFFFFF)) >> np.uint64(19)


def pk_step(h):
    """group_packed_regs' sst / 8: odd, from the low 13 bits of h lo (bit 0 forced)."""
    return ((_u64(h) << np.uint64(1)) | np.uint64(1)) & np.uint64(PK_SLOTS - 1)


# ---- the model of linear probing ----------------------------------------------------
@dataclass
class Placement:
    cap: int
    table: list                  # slot -> key or None
    slot: np.ndarray             # final slot of each key given (cap: the key ~0's own slot)
    longest: int                 # longest displacement from a home slot
    crossed: int                 # insert walks that went from slot cap - 1 to slot 0
    special: bool = False        # the key ~0 was entered

    def probe(self, keys):
        """(found, steps, crossed) per key for a read walk: the slots looked at
        after the home slot until the key or an empty slot, and whether the
        walk went from slot cap - 1 to slot 0."""
        keys = _u64(keys)
        home = (mix64(keys) & np.uint64(self.cap - 1)).tolist()
        found, steps, crossed = [], [], []
        for k, h in zip(keys.tolist(), home):
            if k == M64:
                found.append(self.special), steps.append(0), crossed.append(False)
                continue
            n, x = 0, False
            while self.table[h] is not None and self.table[h] != k:
                x = x or h == self.cap - 1
                h = (h + 1) & (self.cap - 1)
                n += 1
                assert n < self.cap, "a full table: no walk ends"
            found.append(self.table[h] == k), steps.append(n), crossed.append(x)
        return np.array(found), np.array(steps), np.array(crossed)


def place(keys, cap: int) -> Placement:
    """Linear probing of `keys` (copies allowed) into `cap` slots in the order
    given; the key ~0 takes the slot one past the table, as every table here
    does it.  Which slots end up taken does not depend on the order."""
    keys = _u64(keys)
    assert cap & (cap - 1) == 0
    table = [None] * cap
    home = (mix64(keys) & np.uint64(cap - 1)).tolist()
    slot = np.zeros(keys.size, np.int64)
    longest = crossed = 0
    special = False
    for i, (k, h) in enumerate(zip(keys.tolist(), home)):
        if k == M64:
            slot[i], special = cap, True
            continue
        n, x = 0, False
        while table[h] is not None and table[h] != k:
            x = x or h == cap - 1
            h = (h + 1) & (cap - 1)
            n += 1
            assert n < cap, "a full table: no walk ends"
        table[h] = k
        slot[i] = h
        longest = max(longest, n)
        crossed += int(x)
    return Placement(cap, table, slot, longest, crossed, special)


# ---- capacities the host code chooses ---------------------------------------------
def pow2_at_least(x: int, floor: int = 1024) -> int:
    p = floor
    while p < x:
        p <<= 1
    return p


def cap_join(rows: int) -> int:
    """The thumbnail table, the indexer's row table and directory set: a power
    of two >= 2 x rows (copies counted), at least 1024."""
    return pow2_at_least(2 * rows)


def cap_first_call(rows: int, created: int = 1024) -> int:
    """The Object index and the op log after ONE call of `rows` rows on an empty
    table of `created` slots: unchanged while rows <= created / 2, else the
    power of two >= 4 x rows (shard.cpp index_reserve / oplog_reserve)."""
    return created if rows <= created // 2 else pow2_at_least(4 * rows)


# ---- scenarios of the open-addressing tables ---------------------------------------
@dataclass
class Scenario:
    name: str
    cap: int
    keys: np.ndarray             # distinct keys of the table side (0 / ~0 included when `specials`)
    rows: np.ndarray             # the table side as given to the kernel: keys, or shuffled copies
    absent: np.ndarray           # distinct keys that are not in the table
    specials: bool
    homes: dict = field(default_factory=dict)   # home slot -> ordinary keys placed there

    @property
    def ordinary(self):
        return self.keys[(self.keys != np.uint64(0)) & (self.keys != ALL_ONES)]


def _copies(keys, counts, rng):
    return rng.permutation(np.repeat(keys, counts))


def table_scenario(kind: str, n_keys: int, specials: bool, copies: bool, cap_of, seed: int = 0):
    """One scenario of the four tables.

    kind "one_home": n_keys ordinary keys homed at slot cap - 1, so the chain
        wraps through slot 0 and is n_keys slots long.
    kind "straddle": clusters homed at cap - 3 .. cap - 1 (n_keys in all, a
        tenth each at cap - 3 and cap - 2) plus 8 keys at each of the slots
        0..2, which the wrapped cluster pushes forward.
    specials: the keys 0 (home 0) and ~0 (its own slot) are present as well.
    copies: every key is listed 2..5 times, shuffled.
    cap_of(rows): the capacity the host code gives a table built from `rows`
        rows -- the keys are derived for that capacity.
    absent keys: homed at cap - 1 (they walk the whole wrapped cluster), at
        cap - 2, at slots 0, 1 and in the middle of the wrapped run, and a few
        whose home is free."""
    rng = np.random.default_rng([seed, n_keys, int(specials), int(copies),
                                 {"one_home": 1, "straddle": 2}[kind]])
    if kind == "one_home":
        per_home = {-1: n_keys}
    else:
        a = max(1, n_keys // 10)
        per_home = {-3: a, -2: a, -1: n_keys - 2 * a, 0: 8, 1: 8, 2: 8}
    total = sum(per_home.values()) + (2 if specials else 0)
    counts = rng.integers(2, 6, total) if copies else np.ones(total, np.int64)
    cap = cap_of(int(counts.sum()))
    homes = {h % cap: keys_at(cap, h % cap, c, rng) for h, c in per_home.items()}
    keys = np.concatenate(list(homes.values()))
    if specials:
        keys = np.concatenate([keys, np.array([0, M64], np.uint64)])
    keys = rng.permutation(keys)
    rows = _copies(keys, counts, rng) if copies else keys
    run = sum(per_home.values())              # the run of taken slots from the first cluster on
    inside = [cap - 1, cap - 2, 0, 1, (cap - 1 + run // 2) % cap]
    absent = [keys_at(cap, s, 12, rng) for s in inside]
    absent.append(keys_at(cap, cap // 2, 4, rng))          # home free: no walk
    absent = np.concatenate(absent)
    absent = absent[~np.isin(absent, keys)]
    name = f"{kind}_{n_keys}" + ("_sp" if specials else "") + ("_copies" if copies else "")
    return Scenario(name, cap, keys, rows, rng.permutation(absent), specials, homes)


def check_table_scenario(sc: Scenario) -> Placement:
    """The premises of a table scenario, from the model: load <= 1/2; at least
    one insert walk crosses the end; in "one_home" the longest displacement is
    exactly (keys at that home) - 1, i.e. the chain is as long as the keys
    placed there; every absent key homed in the cluster walks to an empty slot,
    those homed at cap - 1 across the end and past every key of the chain."""
    cap = sc.cap
    p = place(sc.keys, cap)
    assert np.unique(sc.keys).size == sc.keys.size
    assert set(sc.rows.tolist()) == set(sc.keys.tolist())
    assert sc.ordinary.size * 2 <= cap
    again = place(sc.rows, cap)               # copies find their key: the same slots taken
    assert [s is None for s in again.table] == [s is None for s in p.table]
    assert p.special == sc.specials and (0 in sc.keys.tolist()) == sc.specials
    assert p.crossed >= 1
    last = sc.homes[cap - 1]
    assert np.all(mix64(last) & np.uint64(cap - 1) == np.uint64(cap - 1))
    if sc.name.startswith("one_home"):
        assert p.longest >= last.size - 1
        assert p.crossed >= last.size - 1
        if not sc.specials:
            assert p.longest == last.size - 1 and p.crossed == last.size - 1
    found, steps, crossed = p.probe(sc.absent)
    assert not found.any()
    at_end = mix64(sc.absent) & np.uint64(cap - 1) == np.uint64(cap - 1)
    assert at_end.sum() >= 8 and crossed[at_end].all() and (steps[at_end] >= last.size).all()
    assert (steps > 0).sum() >= 40 and (steps == 0).sum() >= 1
    # every present key is found again, the wrapped ones across the end
    f2, _, c2 = p.probe(sc.keys)
    assert f2.all() and c2.sum() >= 1
    return p


TABLE_CASES = [  # (kind, keys, specials, copies): (a)-(e) of the placement tests
    ("one_home", 64, False, False), ("one_home", 300, False, False), ("one_home", 512, False, False),
    ("one_home", 64, True, False), ("one_home", 300, True, False), ("one_home", 510, True, False),
    ("straddle", 200, False, False), ("straddle", 200, True, False),
    ("one_home", 64, False, True), ("one_home", 100, True, True), ("one_home", 300, True, True),
    ("one_home", 512, False, True), ("straddle", 100, True, True), ("straddle", 200, False, True),
    ("one_home", 1024, False, False),   # 2048 slots at load exactly 1/2 (join tables)
    ("one_home", 1000, True, False),
]


def case_id(case) -> str:
    kind, n, sp, cp = case
    return f"{kind}_{n}" + ("_sp" if sp else "") + ("_copies" if cp else "")


# ---- the thumbnail filter -------------------------------------------------------
@dataclass
class FilterScenario:
    cap: int
    home: int
    present: np.ndarray          # thumbnail keys: one home slot, filter bits SET_BITS
    absent_walk: np.ndarray      # absent, same home slot, a filter bit that is set: the walk runs
    absent_stop: np.ndarray      # absent, same home slot, a clear filter bit: stops at the filter


SET_BITS = (0, 2, 5, 7)          # values of hash bits 10..12 the present keys cover (cap 1024)


def filter_bit(keys, cap: int):
    return (mix64(keys) & np.uint64(8 * cap - 1)).astype(np.int64)


def filter_scenario(cap: int = 1024, home: int | None = None, seed: int = 0) -> FilterScenario:
    """Keys of one home slot of the thumbnail table; the filter bit of a key is
    row_hash & (8 cap - 1) = home + cap * (the three hash bits above the
    slot's), so one home slot has 8 filter bits."""
    rng = np.random.default_rng([seed, cap, 77])
    home = cap - 1 if home is None else home
    lg = cap.bit_length() - 1

    def at(bit3, count):
        return unmix64(_distinct_hashes(8 * cap - 1, home | (bit3 << lg), count, rng))

    present = np.concatenate([at(b, 30) for b in SET_BITS])
    walk = np.concatenate([at(b, 25) for b in SET_BITS])
    stop = np.concatenate([at(b, 25) for b in range(8) if b not in SET_BITS])
    walk = walk[~np.isin(walk, present)]
    return FilterScenario(cap, home, rng.permutation(present), rng.permutation(walk),
                          rng.permutation(stop))


def check_filter_scenario(fs: FilterScenario):
    cap = fs.cap
    m = np.uint64(cap - 1)
    for part in (fs.present, fs.absent_walk, fs.absent_stop):
        assert np.all(mix64(part) & m == np.uint64(fs.home)) and np.unique(part).size == part.size
    set_bits = set(filter_bit(fs.present, cap).tolist())
    assert len(set_bits) == len(SET_BITS)                       # present keys differ in filter bit
    assert set(filter_bit(fs.absent_walk, cap).tolist()) == set_bits
    assert not set(filter_bit(fs.absent_stop, cap).tolist()) & set_bits
    assert fs.absent_walk.size >= 50 and fs.absent_stop.size >= 50
    assert not np.isin(fs.absent_walk, fs.present).any()
    p = place(fs.present, cap)
    assert p.longest == fs.present.size - 1                     # one chain of all of them
    _, steps, _ = p.probe(fs.absent_walk)
    assert (steps == fs.present.size).all()                     # the walk really runs, to the end
    return p


# ---- the op log at a power-of-256 capacity -------------------------------------------
def oplog_page(cap: int, n_random: int = 400, seed: int = 0):
    """(key, ts) of one page of fewer than 5000 ops for a log of `cap` slots:
    the key ~0 (slot number cap: the one slot that needs the extra sort pass at
    cap = 2^16 and 2^24) several times with ties and out-of-order timestamps,
    keys homed at slots 0, 255, 256, 65535 and cap - 1 (with the key 0), and a
    few hundred random keys; every key two to four times."""
    rng = np.random.default_rng([seed, cap])
    homes = sorted({0, 255, 256, 65535 & (cap - 1), cap - 1})
    chosen = np.concatenate([keys_at(cap, s, 6, rng) for s in homes] + [np.array([0], np.uint64)])
    rand = rng.integers(1, M64 - 1, n_random, dtype=np.uint64)
    keys = np.concatenate([chosen, rand, np.full(9, M64, np.uint64)])
    key = rng.permutation(np.repeat(keys, rng.integers(2, 5, keys.size)))
    ts = rng.integers(-4, 5, key.size)        # few values: ties, and later ops below earlier ones
    assert key.size < 5000
    return key, ts, homes, chosen


# ---- scenarios of the grouping --------------------------------------------------------
def spread_rows(keys, per_key: int, rng, extra=None, chunk: int = 100):
    """Rows with `per_key` copies of every key, the copies of one key in
    different `chunk`-row chunks, `extra` (more keys, one row each) mixed in;
    the few positions left over hold random keys of one row each."""
    keys = _u64(keys)
    extra = np.zeros(0, np.uint64) if extra is None else _u64(extra)
    n = keys.size * per_key + extra.size
    block = -(-n // per_key)
    block = -(-block // chunk) * chunk + chunk        # copies at least a chunk apart
    out = np.zeros(block * per_key, np.uint64)
    used = np.zeros(block * per_key, bool)
    pos = rng.permutation(block)[:keys.size]
    for c in range(per_key):
        out[c * block + pos] = keys
        used[c * block + pos] = True
    free = rng.permutation(np.flatnonzero(~used))
    out[free[:extra.size]] = extra
    rest = free[extra.size:]          # positions left over: one-row filler keys
    out[rest] = rng.integers(1, M64 - 1, rest.size, dtype=np.uint64)
    return out


def slot_step_family(lo32: int, digit15: int = 0x5A5A, shard: int = 0x3C):
    """The 512 keys that share bucket (under every plan up to 15 bits), shard
    byte, LDS slot and probe step: hash bits 32..40 enumerate them."""
    return keys_with_hash(512, None, lo32=lo32, shard=shard, digit=digit15, digit_bits=15)


LO32_LAST = 0xFFFFFFFF        # lds_slot 6143, lds_step 6139; packed slot 8191, step 8191
LO32_FIRST = 0x00000000       # slot 0, step 1 in both tables


def digit_edge_keys(bits: int, count: int, rng):
    """Keys whose `bits`-bit digit is 0 and 2^bits - 1 (count of each): on the
    two-level paths both the coarse and the fine digit sit at their extremes."""
    lo = keys_with_hash(count, rng, digit=0, digit_bits=bits)
    hi = keys_with_hash(count, rng, digit=(1 << bits) - 1, digit_bits=bits)
    return np.concatenate([lo, hi])


OWNER_SHARDS = (84, 85, 86, 127, 128, 170, 171, 255)


def owner_boundary_keys(per_shard: int, rng):
    """Keys on both sides of every owner boundary of world 2 (127 | 128) and
    world 3 (85 | 86, 170 | 171), and at the last shard byte."""
    return np.concatenate([keys_with_hash(per_shard, rng, shard=s) for s in OWNER_SHARDS])
