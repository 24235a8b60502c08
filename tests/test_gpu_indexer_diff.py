"""GPU: the indexer's rescan diff (sdgpu_indexer_diff_device) equals the
restatement of walk.rs:309-381,624-636 and of the header's contract in
tests/indexer_oracle.py: create, update, remove, match, state and counts,
exactly."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import indexer_oracle as IO

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = np.uint64(0xFFFFFFFFFFFFFFFF)
NAMES = ("create", "update", "remove", "match", "state", "counts")
T0, MS = IO.T0, IO.MS

_POOL = {}


def pool():
    """Built once: 700 000 distinct path keys (none 0 or ~0) and 2 000 distinct
    directory keys."""
    if not _POOL:
        rng = np.random.default_rng(2025)
        keys = np.unique(rng.integers(1, 2**63, 720_000, dtype=np.uint64) * np.uint64(2)
                         + np.uint64(1))
        _POOL["keys"] = rng.permutation(keys)[:700_000]
        _POOL["dirs"] = np.unique(rng.integers(1, 2**63, 2100, dtype=np.uint64))[:2000]
        assert _POOL["keys"].size == 700_000 and _POOL["dirs"].size == 2000
    return _POOL


def meta_of(keys):
    """inode, device, modified_at derived from the key, so that both sides of a
    pair agree until one is changed."""
    m = np.empty((keys.size, 3), np.uint64)
    m[:, 0] = (keys >> np.uint64(20)) & np.uint64(0xFFFFF)
    m[:, 1] = 1
    m[:, 2] = np.uint64(T0) + (keys & np.uint64(0xFFFF))
    return m


def is_dir_of(keys):
    return ((keys >> np.uint64(7)) % np.uint64(10) == 0).astype(np.uint8)


def columns(seed, n_r, n_w, n_wd, rows_from=0):
    """A rescan in numbers: four fifths of the walked entries have a row, the
    rest are new; of the pairs a few per cent each differ in kind, inode,
    device or time (both sides of the 1 ms test, and rows newer than the disk);
    a twentieth of the rows have no metadata, a twentieth of the entries are
    ancestors; the walked directories are drawn, with copies, from three
    quarters of the 2 000 the rows lie in."""
    p, rng = pool(), np.random.default_rng(seed)
    r_key = p["keys"][rows_from:rows_from + n_r].copy()
    r_dirkey = p["dirs"][rng.integers(0, 2000, n_r)]
    r_flags = is_dir_of(r_key) | ((rng.random(n_r) < 0.05).astype(np.uint8) << 1)
    r_meta = meta_of(r_key)
    have = min(n_r, n_w * 4 // 5)
    w_key = rng.permutation(np.concatenate([
        rng.permutation(r_key)[:have], p["keys"][600_000:600_000 + n_w - have]]))
    w_flags = is_dir_of(w_key) ^ (rng.random(n_w) < 0.03).astype(np.uint8)
    w_flags |= (rng.random(n_w) < 0.05).astype(np.uint8) << 1
    w_meta = meta_of(w_key)
    w_meta[:, 0] += (rng.random(n_w) < 0.03).astype(np.uint64)
    w_meta[:, 1] += (rng.random(n_w) < 0.03).astype(np.uint64)
    delta = rng.choice(np.array([0, MS, MS + 1, -MS - 1, -3600 * 1000 * MS, 5000 * MS], np.int64),
                       n_w, p=[0.85, 0.03, 0.03, 0.03, 0.03, 0.03])
    w_meta[:, 2] = (w_meta[:, 2].view(np.int64) + delta).view(np.uint64)
    wd_key = p["dirs"][rng.integers(0, 1500, n_wd)]
    return w_key, w_flags, w_meta, wd_key, r_key, r_dirkey, r_flags, r_meta


def expected(cols):
    w_key, w_flags, w_meta, wd_key, r_key, r_dirkey, r_flags, r_meta = cols
    lst = lambda a: None if a is None else a.tolist()  # noqa: E731
    signed = lambda m: np.ascontiguousarray(m).view(np.int64).reshape(-1, 3).tolist()  # noqa: E731
    out = IO.diff_keys(lst(w_key), lst(w_flags), signed(w_meta), lst(wd_key), lst(r_key),
                       lst(r_dirkey), lst(r_flags), signed(r_meta))
    return tuple(np.array(o, np.int64) for o in out)


def dev(a):
    import torch
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(a).cuda()


def as_i64(t):
    a = t.cpu().numpy()
    if a.dtype == np.int32:
        a = a.view(np.uint32)
    return a.astype(np.int64)


def run(ctx, cols, trim=True):
    from spacedrive_amd import indexer as X
    return tuple(as_i64(t) for t in X.diff(*[dev(c) for c in cols], ctx=ctx, trim=trim))


def mismatches(got, want):
    """Per output whether it differs from the oracle's (0 = equal); untrimmed
    lists are compared up to their length."""
    bad = []
    for g, e in zip(got, want):
        bad.append(int(not np.array_equal(g[:e.size], e)))
    return bad


def check(ctx, cols):
    got, want = run(ctx, cols), expected(cols)
    for g, e, name in zip(got, want, NAMES):
        np.testing.assert_array_equal(g, e, err_msg=name)
    return got


# the build's 256-row step, the probe's 512, the row pass's 1024, the 4096-position
# compaction tile, and 512 / 513 rows: the last in 1024 slots, the first in 2048
SIZES = [0, 1, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 4095, 4096, 4097]


@pytest.mark.parametrize("n_w", SIZES)
@pytest.mark.parametrize("n_r", SIZES)
def test_sizes(ctx, n_r, n_w):
    n_wd = (0, 1, 1000)[(SIZES.index(n_r) + SIZES.index(n_w)) % 3]
    create, update, remove, match, state, counts = check(ctx, columns(n_r * 7 + n_w, n_r, n_w, n_wd))
    if n_wd == 0:
        assert remove.size == 0
    if n_r == 0:
        assert (state == IO.CREATE).all() and (match == IO.MISS).all()
    if n_r >= 4095 and n_w >= 4095 and n_wd == 1000:
        assert create.size and update.size and remove.size and counts[3]


@pytest.mark.parametrize("n_wd", [0, 1, 512, 513, 1000])
def test_walked_directory_counts(ctx, n_wd):
    remove = check(ctx, columns(n_wd, 4097, 1025, n_wd))[2]
    assert remove.size == 0 if n_wd == 0 else remove.size > 0 or n_wd == 1


def test_300k(ctx):
    create, update, remove, match, state, counts = check(ctx, columns(3, 300_000, 300_000, 1000))
    assert set(np.unique(state)) == {0, 1, 2, 3}
    assert min(create.size, update.size, remove.size, int(counts[3])) > 1000
    assert remove.size < 200_000 and (match != IO.MISS).sum() == 240_000


def test_table_walks(ctx):
    """1024 rows in 2048 slots, load exactly 1/2: several hundred of the keys
    share their home slot with another, so both the build's and the probe's
    walks go past the first slot.  Then absent keys whose home slot is taken:
    they walk to an empty slot."""
    from oracle import oracle as O
    p = pool()
    cols = list(columns(17, 1024, 0, 1000))
    r_key = cols[4]
    home = O.mix64(r_key) & np.uint64(2047)
    _, inv, cnt = np.unique(home, return_inverse=True, return_counts=True)
    shared = int((cnt[inv] > 1).sum())
    assert shared >= 300
    absent = p["keys"][100_000:160_000]
    taken = absent[np.isin(O.mix64(absent) & np.uint64(2047), home)][:10_000]
    assert taken.size == 10_000
    rng = np.random.default_rng(18)
    w_key = rng.permutation(np.concatenate([r_key, taken]))
    cols[0], cols[1], cols[2] = w_key, is_dir_of(w_key), meta_of(w_key)
    create, update, remove, match, state, counts = check(ctx, tuple(cols))
    assert create.size == 10_000 and (match != IO.MISS).sum() == 1024
    assert remove.size == 0 and update.size == 0


@pytest.mark.parametrize("where", ["both", "walked_only", "rows_only", "rows_ancestor"])
def test_keys_zero_and_all_ones(ctx, where):
    """0 and ~0 are ordinary keys on every side, also as directory keys."""
    cols = list(columns(23, 3000, 3000, 100))
    w_key, w_flags, w_meta, wd_key, r_key, r_dirkey, r_flags, r_meta = cols
    special = np.array([0, ALL], np.uint64)
    if where != "walked_only":
        r_key[[5, 2999]] = special
        r_flags[[5, 2999]] = 0
        r_meta[[5, 2999]] = meta_of(special)
        r_dirkey[[5, 2999]] = special[::-1]
        r_dirkey[[100, 101]] = special
        wd_key[[3, 4]] = special
        # rows 100 and 101 lie in the directories 0 and ~0 and are not on disk
        gone = np.isin(w_key, r_key[[100, 101]])
        w_key[gone] = pool()["keys"][690_000:690_000 + int(gone.sum())]
    if where != "rows_only":
        w_key[[7, 2998]] = special
        w_meta[[7, 2998]] = meta_of(special)
        w_meta[7, 0] += 1
        w_flags[[7, 2998]] = 2 if where == "rows_ancestor" else 0
    create, update, remove, match, state, _ = check(ctx, tuple(cols))
    if where == "both":
        assert match[7] == 5 and match[2998] == 2999 and state[7] == 2 and state[2998] == 1
        assert 5 not in remove and 2999 not in remove and 100 in remove and 101 in remove
    elif where == "walked_only":
        assert match[7] == IO.MISS == match[2998] and 7 in create and 2998 in create
    else:
        assert {5, 2999, 100, 101} <= set(remove.tolist())


@pytest.mark.parametrize("name", sorted(IO.CASES))
def test_hand_cases(ctx, name):
    walk, rows, create, update, remove = IO.CASES[name]
    cols, names = IO.to_columns(walk, rows)
    arrays = tuple(np.array(c, np.uint8) if i in (1, 6)
                   else np.array(c, np.int64).reshape(-1, 3).view(np.uint64) if i in (2, 7)
                   else np.array(c, np.uint64) for i, c in enumerate(cols))
    got = check(ctx, arrays)
    assert IO.tuples_from_keys([g.tolist() for g in got], names, rows) == (create, update, remove)


def test_null_flags(ctx):
    cols = list(columns(29, 5000, 5000, 500))
    for null in ((1,), (6,), (1, 6)):
        c = list(cols)
        for i in null:
            c[i] = None
        got = check(ctx, tuple(c))
        assert (got[5][3] == 0) == (null == (1, 6))


def test_duplicated_keys(ctx):
    """A caller error under the schema, but defined: the rows of one key are
    spared or removed together, the lowest answers, every walked copy gets its
    own answer."""
    rng = np.random.default_rng(31)
    w_key, w_flags, w_meta, wd_key, r_key, r_dirkey, r_flags, r_meta = columns(31, 6000, 6000, 800)
    r_key = r_key[rng.integers(0, 2000, 6000)]        # about three rows per key
    w_key[:3000] = r_key[rng.integers(0, 6000, 3000)]  # walked copies, with their own metadata
    wd_key = np.concatenate([wd_key, wd_key, wd_key[:5]])
    cols = (w_key, w_flags, w_meta, wd_key, r_key, r_dirkey, r_flags, r_meta)
    create, update, remove, match, state, _ = check(ctx, cols)
    hit = match != IO.MISS
    first = {}
    for j, k in enumerate(r_key.tolist()):
        first.setdefault(k, j)
    assert all(first[k] == j for k, j in zip(w_key[hit].tolist(), match[hit].tolist()))
    assert remove.size > 50 and np.unique(w_key).size < 5000


def test_one_directory_everything_removed_nothing_changed(ctx):
    p = pool()
    w_key, w_flags, w_meta, wd_key, r_key, r_dirkey, r_flags, r_meta = columns(37, 9000, 9000, 10)
    one = np.full(9000, p["dirs"][1999], np.uint64)
    # all rows in one directory, which was walked
    got = check(ctx, (w_key, w_flags, w_meta, p["dirs"][1990:2000], r_key, one, r_flags, r_meta))
    assert 0 < got[2].size < 9000
    # ... and which was not
    got = check(ctx, (w_key, w_flags, w_meta, p["dirs"][:1999], r_key, one, r_flags, r_meta))
    assert got[2].size == 0
    # every row removed: all directories walked, nothing of them on disk
    none = p["keys"][650_000:659_000]
    got = check(ctx, (none, None, meta_of(none), p["dirs"], r_key, r_dirkey, r_flags, r_meta))
    np.testing.assert_array_equal(got[2], np.arange(9000))
    assert got[0].size == 9000
    got = check(ctx, (none[:0], None, meta_of(none[:0]), p["dirs"], r_key, r_dirkey, r_flags, r_meta))
    np.testing.assert_array_equal(got[2], np.arange(9000))
    # nothing changed: the disk is the index
    got = check(ctx, (r_key, r_flags & 1, r_meta, p["dirs"], r_key, r_dirkey, r_flags, r_meta))
    assert got[5].tolist() == [0, 0, 0, 0] and (got[4] == IO.UNCHANGED).all()
    np.testing.assert_array_equal(got[3], np.arange(9000))


def raw_call(ctx, cols, fill=0xA5):
    """The device call on output buffers pre-filled with `fill`; the untrimmed
    outputs as numpy arrays."""
    import torch
    d = [dev(c) for c in cols]
    n_w, n_wd, n_r = cols[0].size, cols[3].size, cols[4].size
    full = lambda n, dt: torch.full((max(n, 1) * dt,), fill, dtype=torch.uint8, device="cuda")  # noqa: E731
    create, update, remove, match = full(n_w, 4), full(n_w, 4), full(n_r, 4), full(n_w, 4)
    state, counts = full(n_w, 1), full(4, 4)
    ptr = lambda t: None if t is None or t.numel() == 0 else t.data_ptr()  # noqa: E731
    rc = ctx.lib.sdgpu_indexer_diff_device(
        ctx.h, ptr(d[0]), ptr(d[1]), ptr(d[2]), n_w, ptr(d[3]), n_wd, ptr(d[4]), ptr(d[5]),
        ptr(d[6]), ptr(d[7]), n_r, match.data_ptr(), state.data_ptr(), create.data_ptr(),
        update.data_ptr(), remove.data_ptr(), counts.data_ptr(),
        torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    u32 = lambda t: t.cpu().numpy().view(np.uint32).astype(np.int64)  # noqa: E731
    return (u32(create), u32(update), u32(remove), u32(match)[:n_w],
            state.cpu().numpy().astype(np.int64)[:n_w], u32(counts))


def untouched_past_lengths(got, want, fill32=0xA5A5A5A5):
    return all((g[e.size:] == fill32).all() for g, e in zip(got[:3], want[:3]))


@pytest.mark.parametrize("n_r,n_w", [(5000, 4097), (1, 1), (4096, 0), (0, 513)])
def test_nothing_written_past_the_lengths(ctx, n_r, n_w):
    cols = columns(41, n_r, n_w, 700)
    got, want = raw_call(ctx, cols), expected(cols)
    assert mismatches(got, want) == [0] * 6
    assert untouched_past_lengths(got, want)
    assert sum(g.size - e.size for g, e in zip(got[:3], want[:3])) > 0


def test_host_twin_equals_device_call(ctx):
    from spacedrive_amd import indexer as X
    for n_r, n_w, n_wd in ((7000, 6000, 900), (0, 300, 5), (300, 0, 5), (0, 0, 4)):
        cols = columns(43 + n_r, n_r, n_w, n_wd)
        want = expected(cols)
        got = X.diff_host(*cols, ctx=ctx)
        for g, e, name in zip(got, want, NAMES):
            np.testing.assert_array_equal(g.astype(np.int64), e, err_msg=name)
        for g, e in zip(run(ctx, cols), got):
            np.testing.assert_array_equal(g, e.astype(np.int64))
    cols = list(columns(44, 2000, 2000, 100))
    cols[1] = cols[6] = None
    for g, e in zip(X.diff_host(*cols, ctx=ctx), expected(tuple(cols))):
        np.testing.assert_array_equal(g.astype(np.int64), e)


def test_trim_false(ctx):
    cols = columns(47, 6000, 5000, 600)
    got, want = run(ctx, cols, trim=False), expected(cols)
    assert got[0].size == 5000 == got[1].size and got[2].size == 6000
    assert mismatches(got, want) == [0] * 6


def run_reuse(ctx, poisoned=False):
    """Calls of different sizes through one context, larger and smaller ones in
    turn and other tables' keys in between: mismatches per call."""
    bad = []
    for seed, n_r, n_w, n_wd, at in ((51, 9000, 9000, 1000, 0), (52, 700, 300, 10, 20_000),
                                     (53, 20_000, 5000, 300, 5000), (54, 600, 9000, 0, 0),
                                     (55, 0, 100, 7, 0), (56, 4097, 0, 1000, 40_000)):
        cols = columns(seed, n_r, n_w, n_wd, rows_from=at)
        want = expected(cols)
        got = raw_call(ctx, cols) if poisoned else run(ctx, cols)
        bad.append(mismatches(got, want)
                   + ([int(not untouched_past_lengths(got, want))] if poisoned else []))
    return bad


def test_two_calls_through_one_context(ctx):
    assert run_reuse(ctx) == [[0] * 6] * 6


_CHILD = r'''
import json, sys
sys.path.insert(0, sys.argv[1])
from spacedrive_amd._native import Context
from tests import test_gpu_indexer_diff as G
ctx = Context(0)
ctx.set_timing(True)
out = G.run_reuse(ctx, poisoned=True)
ctx.sync()
print(json.dumps({"bad": out, "kernels": sorted(ctx.kernel_times())}), flush=True)
'''


def test_first_calls_on_poisoned_workspace():
    """The same in one fresh child whose workspaces start as 0xA5 bytes
    (SDGPU_POISON_WS=1) and whose outputs are pre-filled with 0xA5: no region
    of the workspace is read before the call wrote it."""
    env = dict(os.environ, SDGPU_POISON_WS="1")
    p = subprocess.run([sys.executable, "-c", _CHILD, ROOT], capture_output=True, text=True,
                       timeout=240, env=env)
    assert p.returncode == 0, p.stderr[-3000:]
    out = json.loads(p.stdout.strip().splitlines()[-1])
    assert out["bad"] == [[0] * 7] * 6
    assert "poisoned" in p.stderr and "link_ws" in p.stderr
    assert {"idx_build", "idx_probe", "idx_rows", "idx_count", "idx_scan",
            "idx_write"} <= set(out["kernels"])


def test_path_and_dir_keys_are_blake3(ctx):
    """path_keys / dir_keys against BLAKE3 of the same bytes: an empty name,
    messages of 63 / 64 / 65 bytes, a 4 000-byte path, names that are not
    ASCII."""
    from oracle import oracle as O
    from spacedrive_amd import indexer as X
    fit = lambda n: "/" + "d" * (n - 4 - 2 - 4) + "/"  # noqa: E731  "P" salt mp NUL "n" NUL "ext"
    tuples = [("/", "", ""), ("/", "a", "txt"), (fit(63), "n", "ext"), (fit(64), "n", "ext"),
              (fit(65), "n", "ext"), ("/" + "p" * 3998 + "/", "long", "bin"),
              ("/früh/", "日本語のファイル", "tärgz"), ("/a/", "b", ""), ("/a/b/", "", "")]
    for salt in (0, 1, 255):
        msgs = [b"P" + bytes([salt]) + m.encode() + b"\0" + n.encode() + b"\0" + e.encode()
                for m, n, e in tuples]
        assert [len(m) for m in msgs[2:5]] == [63, 64, 65] and len(msgs[5]) > 4000
        want = [int.from_bytes(O.blake3(m)[:8], "little") for m in msgs]
        got = X.path_keys(*zip(*tuples), salt=salt, ctx=ctx)
        assert got.dtype == np.uint64 and got.tolist() == want
        dirs = [t[0] for t in tuples] + ["/" + "q" * 60, "/" + "q" * 61, "/" + "q" * 62]
        dmsgs = [b"D" + bytes([salt]) + d.encode() for d in dirs]
        assert [len(m) for m in dmsgs[-3:]] == [63, 64, 65]
        want = [int.from_bytes(O.blake3(m)[:8], "little") for m in dmsgs]
        assert X.dir_keys(dirs, salt=salt, ctx=ctx).tolist() == want
    assert X.path_keys([], [], []).size == 0
    # the separators keep (mp, name, ext) apart: "a" + "b.c" is not "a.b" + "c"
    k = X.path_keys(["/", "/", "/"], ["a", "a.b", "a"], ["b.c", "c", ""], ctx=ctx)
    assert np.unique(k).size == 3
    assert X.path_keys(["/"], ["a"], [""], salt=1, ctx=ctx)[0] != k[2]
