"""GPU: the stale-thumbnail anti-join (sdgpu_stale_thumbnails_device) and the
sweep built on it equal the restatement of thumbnail_remover.rs:236-367 in
tests/thumb_oracle.py: the stale positions, their per-directory offsets, and
the tree a sweep leaves behind."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from tests import thumb_oracle as TO

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = np.uint64(0xFFFFFFFFFFFFFFFF)


def dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).cuda()


def expected(thumbs, dir_start, columns):
    ids = TO.hex_of_keys(thumbs)
    dirs = [ids[a:b] for a, b in zip(dir_start[:-1], dir_start[1:])]
    libs = [TO.library_cas_ids(k, h) for k, h in columns]
    stale, start = TO.stale_positions(dirs, libs)
    return np.array(stale, dtype=np.int64), np.array(start, dtype=np.int64)


def run(ctx, thumbs, dir_start, columns, trim=True):
    from spacedrive_amd import thumbnail_remover as T
    cols = [(dev(k), None if h is None else dev(h)) for k, h in columns]
    stale, start = T.stale_thumbnails(dev(thumbs), dev(np.asarray(dir_start, np.uint32)), cols,
                                      ctx, trim=trim)
    return stale.cpu().numpy().astype(np.int64), start.cpu().numpy().astype(np.int64)


def check(ctx, thumbs, dir_start, columns):
    stale, start = run(ctx, thumbs, dir_start, columns)
    e_stale, e_start = expected(thumbs, dir_start, columns)
    np.testing.assert_array_equal(start, e_start)
    np.testing.assert_array_equal(stale, e_stale)
    return stale, start


def even_dirs(n, n_dirs):
    return (np.arange(n_dirs + 1, dtype=np.int64) * n // n_dirs).astype(np.uint32)


_POOL = {}


def pool():
    """Built once: 100 003 distinct thumbnail keys (none 0 or ~0) and three
    columns over them: a large one (has_key NULL) holding the even thumbnails,
    an empty one, and a small one holding every fifth.  A tenth of the small
    column's rows have has_key == 0 and carry the keys of odd thumbnails, most
    of which nothing else owns: those must not count."""
    if not _POOL:
        rng = np.random.default_rng(2024)
        keys = np.unique(rng.integers(1, 2**63, 110_000, dtype=np.uint64))
        keys = rng.permutation(keys)[:100_003]
        foreign = rng.integers(1, 2**63, 200_000, dtype=np.uint64) | np.uint64(1 << 63)
        big = rng.permutation(np.concatenate([keys[::2], foreign, keys[::2][:50_000]]))[:300_000]
        small = np.concatenate([keys[::5], foreign[:3000]])
        has = np.ones(small.size, np.uint8)
        dead = np.arange(0, small.size, 10)
        has[dead] = 0
        small = small.copy()
        small[dead] = keys[1::2][:dead.size]          # keys of thumbnails nobody else owns
        _POOL.update(keys=keys, foreign=foreign,
                     columns=[(small, has), (np.zeros(0, np.uint64), np.zeros(0, np.uint8)),
                              (big, None)])
    return _POOL


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 512, 4095, 4096, 4097, 100_003])
def test_thumbnail_counts(ctx, n):
    """Powers of two put the table at exactly its highest load."""
    p = pool()
    check(ctx, p["keys"][:n], even_dirs(n, 7), p["columns"])


@pytest.mark.parametrize("rows", [0, 1, 1023, 1024, 1025, 300_000])
def test_column_rows(ctx, rows):
    p = pool()
    rng = np.random.default_rng(rows)
    thumbs = p["keys"][:4097]
    col = rng.choice(np.concatenate([thumbs[:3000], p["foreign"][:3000]]), rows)
    has = (rng.random(rows) > 0.1).astype(np.uint8)
    check(ctx, thumbs, even_dirs(4097, 5), [(col, has)])
    check(ctx, thumbs, even_dirs(4097, 5), [(col, None)])


@pytest.mark.parametrize("n_cols", [0, 1, 3])
def test_column_layouts(ctx, n_cols):
    p = pool()
    thumbs = p["keys"][:10_000]
    cols = {0: [], 1: [p["columns"][0]], 3: p["columns"]}[n_cols]
    stale, start = check(ctx, thumbs, even_dirs(10_000, 256), cols)
    if n_cols == 0:
        np.testing.assert_array_equal(stale, np.arange(10_000))
    if n_cols == 1:   # has_key == 0 rows carry thumbnail keys: none of those is owned
        small, has = cols[0]
        dead = set(small[has == 0].tolist()) - set(small[has == 1].tolist())
        pos = {int(k): i for i, k in enumerate(thumbs.tolist())}
        hit = [pos[k] for k in dead if k in pos]
        assert hit and set(hit) <= set(stale.tolist())


@pytest.mark.parametrize("special", [0, int(ALL)])
@pytest.mark.parametrize("case", ["owned", "not_owned", "column_only"])
def test_special_keys(ctx, special, case):
    """Key 0 and key ~0 (the table's empty marker: it has a slot of its own)."""
    p = pool()
    sp = np.uint64(special)
    thumbs = p["keys"][:300].copy()
    col = np.concatenate([p["keys"][:300:3], p["foreign"][:100]])
    has = np.ones(col.size, np.uint8)
    if case != "column_only":
        thumbs[17] = sp
        thumbs[250] = sp          # the same key in two directories: one answer
    if case == "not_owned":
        col[5], has[5] = sp, 0    # a keyless row holding it does not own it
    else:
        col[5] = sp
    stale, _ = check(ctx, thumbs, even_dirs(300, 4), [(col, has)])
    if case == "owned":
        assert 17 not in stale and 250 not in stale
    if case == "not_owned":
        assert 17 in stale and 250 in stale


@pytest.mark.parametrize("pattern", ["all_owned", "none_owned", "non_indexed_only"])
def test_hit_patterns(ctx, pattern):
    p = pool()
    n = 5000
    thumbs = p["keys"][:n]
    lib = (p["foreign"][:4000], np.ones(4000, np.uint8))
    cols = {"all_owned": [(np.concatenate([thumbs, p["foreign"][:100]]), None)],
            "none_owned": [lib],
            # the non-indexed set is one more column with has_key == NULL
            "non_indexed_only": [lib, (thumbs[::3].copy(), None)]}[pattern]
    stale, start = check(ctx, thumbs, even_dirs(n, 256), cols)
    if pattern == "all_owned":
        assert stale.size == 0 and not start.any()
    if pattern == "none_owned":
        np.testing.assert_array_equal(stale, np.arange(n))
        np.testing.assert_array_equal(start, even_dirs(n, 256))
    if pattern == "non_indexed_only":
        np.testing.assert_array_equal(stale, np.flatnonzero(np.arange(n) % 3 != 0))


@pytest.mark.parametrize("n_dirs", [1, 256, 1000])
def test_directories(ctx, n_dirs):
    """Empty directories at the front, in the middle and at the end; a boundary
    exactly at 4096 (the compaction's tile) and one at 4097; the one-thumbnail
    directory [4096, 4097) wholly stale next to one wholly owned."""
    p = pool()
    n = 10_000
    thumbs = p["keys"][:n]
    if n_dirs == 1:
        start = np.array([0, n], np.uint32)
    else:
        rng = np.random.default_rng(n_dirs)
        fixed = [0, 0, 0, 2000, 2000, 2000, 4096, 4097, 4200, n, n, n]
        cuts = rng.choice(np.arange(1, n), n_dirs + 1 - len(fixed), replace=False)
        start = np.sort(np.concatenate([fixed, cuts])).astype(np.uint32)
    assert start.size == n_dirs + 1
    owned = np.random.default_rng(7).random(n) < 0.5
    owned[4096] = False
    owned[4097:4200] = True
    col = np.concatenate([thumbs[owned], p["foreign"][:500]])
    stale, s = check(ctx, thumbs, start, [(col, None)])
    if n_dirs > 1:
        d = int(np.flatnonzero(start == 4096)[-1])
        assert start[d + 1] == 4097 and s[d + 1] - s[d] == 1          # emptied
        last = int(np.flatnonzero(start == 4097)[-1])
        e = int(np.flatnonzero(start > 4097)[0])
        assert s[e] == s[last]                                          # [4097, next cut) all owned
        assert s[0] == s[2] == 0 and s[-1] == s[-3] == stale.size


def reuse_shapes():
    p = pool()
    large = (p["keys"], even_dirs(100_003, 256), p["columns"])
    # the small shape's keys are thumbnails of the large one that were hit there
    small = (p["keys"][:130:2].copy(), even_dirs(65, 3), [(p["foreign"][:10], None)])
    return [large, small, large]


def run_reuse(ctx):
    """Large, small, large again on one context: per call, the number of
    positions that differ from the restatement (0 = equal)."""
    bad = []
    shapes = reuse_shapes()
    want = [expected(*sh) for sh in shapes[:2]]
    for (thumbs, start, cols), (e_stale, e_s) in zip(shapes, want + want[:1]):
        stale, s = run(ctx, thumbs, start, cols)
        bad.append(int(stale.size != e_stale.size or not np.array_equal(stale, e_stale)
                       or not np.array_equal(s, e_s)))
    return bad


def test_workspace_reuse(ctx):
    """Old table contents must not leak into a later call."""
    assert run_reuse(ctx) == [0, 0, 0]
    thumbs, start, cols = reuse_shapes()[1]
    stale, _ = run(ctx, thumbs, start, cols)
    np.testing.assert_array_equal(stale, np.arange(65))     # nothing owns them here


_CHILD = r'''
import json, sys
sys.path.insert(0, sys.argv[1])
from spacedrive_amd._native import Context
from tests import test_gpu_stale_thumbnails as G
print(json.dumps(G.run_reuse(Context(0))), flush=True)
'''


def test_first_calls_on_poisoned_workspace():
    """The same in a fresh process whose new workspaces start as 0xA5 bytes."""
    env = dict(os.environ, SDGPU_POISON_WS="1")
    p = subprocess.run([sys.executable, "-c", _CHILD, ROOT], capture_output=True, text=True,
                       timeout=240, env=env)
    assert p.returncode == 0, p.stderr[-3000:]
    assert json.loads(p.stdout.strip().splitlines()[-1]) == [0, 0, 0]


def test_host_variant_equals_the_device_variant(ctx):
    from spacedrive_amd import thumbnail_remover as T
    p = pool()
    thumbs, start = p["keys"][:4097], even_dirs(4097, 100)
    stale, s = run(ctx, thumbs, start, p["columns"])
    h_stale, h_s = T.stale_thumbnails_host(thumbs, start, p["columns"], ctx)
    np.testing.assert_array_equal(h_stale.astype(np.int64), stale)
    np.testing.assert_array_equal(h_s.astype(np.int64), s)
    e_stale, e_s = expected(thumbs, start, p["columns"])
    np.testing.assert_array_equal(h_stale.astype(np.int64), e_stale)
    # inconsistent offsets are refused where they can be read
    with pytest.raises(OSError):
        T.stale_thumbnails_host(thumbs, np.array([0, 5000, 4097], np.uint32), p["columns"], ctx)
    # no thumbnails at all
    z, zs = T.stale_thumbnails_host(thumbs[:0], np.zeros(4, np.uint32), p["columns"], ctx)
    assert z.size == 0 and not zs.any()


def test_untrimmed_equals_trimmed(ctx):
    p = pool()
    thumbs, start = p["keys"][:4097], even_dirs(4097, 100)
    stale, s = run(ctx, thumbs, start, p["columns"])
    full, s2 = run(ctx, thumbs, start, p["columns"], trim=False)
    assert full.size == 4097
    np.testing.assert_array_equal(s2, s)
    np.testing.assert_array_equal(full[:s[-1]], stale)


# ---- the sweep ---------------------------------------------------------------------

def make_cache(root, seed=5):
    """About 2 000 thumbnails over about 40 shard directories, with every
    oddity of the scan.  Returns (lib_a, lib_b, non_indexed): two libraries'
    (keys, has_key) columns, the second sharing keys with the first, and the
    non-indexed cas_ids."""
    rng = np.random.default_rng(seed)
    keys = np.unique(rng.integers(1, 2**63, 2100, dtype=np.uint64))[:2000]
    keys = rng.permutation(keys)
    ids = TO.hex_of_keys(keys)
    os.makedirs(root)
    with open(os.path.join(root, "version.txt"), "w") as f:
        f.write("1")
    shard = rng.integers(0, 40, keys.size)
    for c, d in zip(ids, shard):
        name = "%02x" % d       # the directory a thumbnail is found in need not be c[:2]
        os.makedirs(os.path.join(root, name), exist_ok=True)
        with open(os.path.join(root, name, c + ".webp"), "wb") as f:
            f.write(b"w")
    os.makedirs(os.path.join(root, "empty"))
    odd = os.path.join(root, "%02x" % shard[0])  # holds ids[0], which library a owns
    for n in (".webp", "X.WEBP", "a.b.webp", "not-a-cas-id.webp", "AABBCCDDEEFF0011.webp",
              "BBBBCCDDEEFF0011.webp", ids[5] + ".webp"):   # a second copy of ids[5], elsewhere
        with open(os.path.join(odd, n), "wb") as f:
            f.write(b"w")
    outside = root + "_outside"
    os.makedirs(outside)
    with open(os.path.join(outside, "ffffffffffffffff.webp"), "wb") as f:
        f.write(b"w")
    os.symlink(outside, os.path.join(root, "ln"))
    a = np.concatenate([keys[:900], rng.integers(1, 2**63, 500, dtype=np.uint64)])
    has_a = np.ones(a.size, np.uint8)
    has_a[1:900:9] = 0                             # rows without a cas_id: their bytes own nothing
    has_a[0] = 1
    b = np.concatenate([keys[700:1300], rng.integers(1, 2**63, 300, dtype=np.uint64)])
    non_indexed = set(ids[1300:1500]) | {"BBBBCCDDEEFF0011", "a.b", "0000000000000000"}
    return (a, has_a), (b, None), non_indexed


def test_process_clean_up_end_to_end(ctx, tmp_path):
    from spacedrive_amd import thumbnail_remover as T
    root, copy = str(tmp_path / "thumbs"), str(tmp_path / "copy")
    lib_a, lib_b, non_indexed = make_cache(root)
    shutil.copytree(root, copy, symlinks=True)
    libs = [(dev(k), None if h is None else dev(h)) for k, h in (lib_a, lib_b)]
    sets = [TO.library_cas_ids(k, h) for k, h in (lib_a, lib_b)]
    dry = T.process_clean_up(root, libs, non_indexed, ctx, dry_run=True)
    assert TO.listing(root) == TO.listing(copy)
    rep = T.process_clean_up(root, libs, non_indexed, ctx)
    files, dirs = TO.process_clean_up(copy, sets, non_indexed)
    assert TO.listing(root) == TO.listing(copy)
    rel = lambda paths, base: sorted(os.path.relpath(x, base) for x in paths)  # noqa: E731
    assert rel(rep["removed_files"], root) == rel(files, copy)
    assert rel(rep["removed_dirs"], root) == rel(dirs, copy)
    assert rel(dry["removed_files"], root) == rel(files, copy)
    assert rel(dry["removed_dirs"], root) == rel(dirs, copy)
    assert 400 < len(files) < 1000 and "empty" in rel(dirs, copy)
    again = T.process_clean_up(root, libs, non_indexed, ctx)
    assert again == {"removed_files": [], "removed_dirs": []}
    assert os.path.exists(os.path.join(root + "_outside", "ffffffffffffffff.webp"))


def test_thumbnail_remover_run(ctx, tmp_path):
    from spacedrive_amd import thumbnail_remover as T
    root = str(tmp_path / "thumbs")
    lib_a, lib_b, non_indexed = make_cache(root, seed=6)
    before = TO.listing(root)
    actor = T.ThumbnailRemover(root, ctx)
    for c in non_indexed:
        actor.new_non_indexed_thumbnail(c)
    assert actor.run() is None and TO.listing(root) == before     # no library loaded (:176)
    actor.add_library("a", (dev(lib_a[0]), dev(lib_a[1])))
    actor.add_library("b", (dev(lib_b[0]), None))
    actor.run()
    kept = TO.listing(root)
    sets = [TO.library_cas_ids(*lib_a), TO.library_cas_ids(*lib_b)]
    only_a = (sets[0] - sets[1]) - non_indexed
    mine = [p for p in kept if os.path.basename(p)[:-5].decode() in only_a]
    assert len(mine) > 300
    assert actor.run() == {"removed_files": [], "removed_dirs": []}
    actor.remove_library("a")                                     # the only owner leaves
    rep = actor.run()
    assert sorted(os.path.basename(f)[:-5] for f in rep["removed_files"]) == \
        sorted(os.path.basename(p)[:-5].decode() for p in mine)
    left = TO.listing(root)
    assert not set(left) & set(mine)
    actor.remove_library("b")
    assert actor.run() is None and TO.listing(root) == left
