"""GPU: spacedrive_amd.indexer.rescan + apply on a real directory tree equal the
restatement of walk.rs:309-381,624-636 in tests/indexer_oracle.py applied to
the same listings and rows, through additions, a touch, a rename over a file,
deletions, a file replaced by a directory and a rule that drops a sub-tree."""
import os
import shutil

import numpy as np
import pytest

from tests import indexer_oracle as IO

pytestmark = pytest.mark.gpu


def make_tree(root):
    """10 directories of 25 files, three of them with a sub-directory of 10:
    293 entries."""
    for d in range(10):
        os.makedirs(os.path.join(root, "d%d" % d))
        for f in range(25):
            name = ("f%02d.txt", "g%02d.tar.gz", ".h%02d", "plain%02d", "ü%02d.jpg")[f % 5] % f
            with open(os.path.join(root, "d%d" % d, name), "wb") as fh:
                fh.write(b"%d/%d" % (d, f))
    for d in (1, 4, 7):
        os.makedirs(os.path.join(root, "d%d" % d, "sub"))
        for f in range(10):
            with open(os.path.join(root, "d%d" % d, "sub", "s%d.bin" % f), "wb") as fh:
                fh.write(b"s")
    return 10 + 250 + 3 + 30


def oracle_walk(walk):
    """The product's Walk as the oracle's listings: every walked directory with
    its buffer (the test's rules push no ancestors)."""
    buffers = {cp: [] for cp in walk.dirs}
    for e in walk.entries:
        assert not e.ancestor
        buffers[e.materialized_path].append((e.materialized_path, e.name, e.extension, e.is_dir,
                                             e.inode, e.device, e.modified_at))
    return [(cp, buffers[cp]) for cp in walk.dirs]


def listing_of(root, accept):
    """The accepted paths by os.walk, independently of the product's scan."""
    out = set()
    for base, dirs, files in os.walk(root):
        rel = os.path.relpath(base, root)
        rel = "" if rel == "." else rel.replace(os.sep, "/")
        dirs[:] = [d for d in dirs if accept((rel + "/" + d).lstrip("/"), True)]
        out |= {((rel + "/" + d).lstrip("/"), True) for d in dirs}
        out |= {((rel + "/" + f).lstrip("/"), False) for f in files
                if accept((rel + "/" + f).lstrip("/"), False)}
    return out


def step(X, index, root, accept):
    """One rescan + apply on both sides; the rescan, compared on the way."""
    rows = index.rows()
    by_id = {r[0]: r for r in rows}
    res = X.rescan(index, root, accept)
    w = res.walk
    paths = {((e.materialized_path + e.name + ("." + e.extension if e.extension else ""))[1:],
              e.is_dir) for e in w.entries}
    assert paths == listing_of(root, accept)
    ow = oracle_walk(w)
    want = IO.diff_tuples(ow, rows)
    four = lambda i: (w.entries[i].materialized_path, w.entries[i].name,  # noqa: E731
                      w.entries[i].extension, w.entries[i].is_dir)
    assert sorted(map(four, res.create)) == sorted(want[0])
    assert sorted((res.match[i], four(i)) for i in res.update) == sorted(want[1])
    assert sorted(res.remove) == want[2]
    assert res.kind_changed == sum(1 for s in res.state if s == X.KIND_CHANGED)
    cleared = X.apply(index, res)
    want_rows, want_cleared = IO.apply_tuples(rows, ow, want, max(by_id, default=0) + 1)
    assert sorted(r[1:] for r in index.rows()) == sorted(r[1:] for r in want_rows)
    assert sorted(cleared) == sorted(want_cleared)
    assert len(set(index.tuples())) == len(index)
    return res


def change_tree(root, replace_file_by_directory):
    """Files added, a file touched, one replaced via rename, one backdated,
    files and a directory deleted and, if asked for, a file replaced by a
    directory; the directories whose listing changed get an mtime well past
    1 ms."""
    j = os.path.join
    changed_dirs = {d: os.stat(j(root, d)) for d in ("d0", "d2", "d3", "d5")}
    for name in ("new1.txt", "new2", ".new3"):                      # files added
        open(j(root, "d0", name), "wb").close()
    os.makedirs(j(root, "d0", "fresh", "deeper"))
    open(j(root, "d0", "fresh", "deeper", "n.txt"), "wb").close()
    touched = j(root, "d2", "f00.txt")                               # a new mtime
    st = os.stat(touched)
    os.utime(touched, ns=(st.st_atime_ns, st.st_mtime_ns + 5_000_000_000))
    old = os.stat(j(root, "d2", "f05.txt"))                          # replaced via rename
    with open(j(root, "d2", "tmp"), "wb") as fh:
        fh.write(b"other")
    os.utime(j(root, "d2", "tmp"), ns=(old.st_atime_ns, old.st_mtime_ns))
    os.replace(j(root, "d2", "tmp"), j(root, "d2", "f05.txt"))
    assert os.stat(j(root, "d2", "f05.txt")).st_ino != old.st_ino
    backdated = j(root, "d2", "f10.txt")                             # older on disk: left alone
    st = os.stat(backdated)
    os.utime(backdated, ns=(st.st_atime_ns, st.st_mtime_ns - 3_600_000_000_000))
    os.remove(j(root, "d3", "f00.txt"))                              # files and a directory deleted
    os.remove(j(root, "d3", ".h02"))
    shutil.rmtree(j(root, "d4"))
    if replace_file_by_directory:
        os.remove(j(root, "d5", "plain03"))
        os.makedirs(j(root, "d5", "plain03"))
        open(j(root, "d5", "plain03", "inside.txt"), "wb").close()
    for d, st in changed_dirs.items():          # their listings changed: a new mtime, well past 1 ms
        os.utime(j(root, d), ns=(st.st_atime_ns, st.st_mtime_ns + 10_000_000_000))


def rules(rel, is_dir):
    """Drops the sub-tree d7."""
    return rel != "d7" and not rel.startswith("d7/")


def test_rescan_follows_the_tree(ctx, tmp_path):
    from spacedrive_amd import indexer as X
    root = str(tmp_path / "loc")
    n = make_tree(root)
    everything = lambda rel, is_dir: True  # noqa: E731
    index = X.LocationIndex()
    first = step(X, index, root, everything)
    assert len(first.create) == n == len(index) and not first.update and not first.remove
    again = step(X, index, root, everything)
    assert (again.create, again.update, again.remove) == ([], [], [])
    assert set(again.state) == {X.UNCHANGED} and None not in again.match

    change_tree(root, replace_file_by_directory=True)

    second = step(X, index, root, rules)
    by_name = {(e.materialized_path, e.name, e.extension): s
               for e, s in zip(second.walk.entries, second.state)}
    assert by_name[("/d2/", "f00", "txt")] == X.UPDATE == by_name[("/d2/", "f05", "txt")]
    assert by_name[("/d2/", "f10", "txt")] == X.UNCHANGED
    assert by_name[("/d5/", "plain03", "")] == X.KIND_CHANGED and second.kind_changed == 1
    assert len(second.create) == 3 + 3 + 1 + 1 and len(second.update) == 2 + 4
    # d3's two files, d4 itself (its 36 descendants lie in directories that were
    # not walked, and stay), d7 itself (dropped by the rules, its rows stay too)
    assert len(second.remove) == 2 + 1 + 1
    tuples = set(index.tuples())
    assert ("/d4/", "f00", "txt") in tuples and ("/d7/sub/", "s0", "bin") in tuples
    assert ("/", "d4", "") not in tuples and ("/", "d7", "") not in tuples
    # the row of the replaced file is still a file: the reference's behaviour
    i = index.tuples().index(("/d5/", "plain03", ""))
    assert index.is_dir[i] is False

    # Another rescan reports nothing new.  What the reference reports on every
    # rescan -- the directory that replaced a file, created again and skipped as
    # a duplicate -- is reported here too, as state 3, and changes nothing.
    before = index.rows()
    third = step(X, index, root, rules)
    assert (third.update, third.remove) == ([], []) and index.rows() == before
    assert [third.state[i] for i in third.create] == [X.KIND_CHANGED] and third.kind_changed == 1
    # The caller repairs what state 3 exposes: the stale row goes, the entry is
    # created, and then a rescan reports nothing at all.
    index.remove([third.match[third.create[0]]])
    fourth = step(X, index, root, rules)
    assert len(fourth.create) == 1 and fourth.kind_changed == 0
    fifth = step(X, index, root, rules)
    assert (fifth.create, fifth.update, fifth.remove, fifth.kind_changed) == ([], [], [], 0)
    assert fifth.salt == 0


def test_second_rescan_after_changes_reports_nothing(ctx, tmp_path):
    """The same changes without the file replaced by a directory (the one case
    the reference itself reports again on every rescan): after rescan + apply a
    second rescan reports nothing at all."""
    from spacedrive_amd import indexer as X
    root = str(tmp_path / "loc")
    n = make_tree(root)
    index = X.LocationIndex()
    assert len(step(X, index, root, lambda rel, is_dir: True).create) == n
    change_tree(root, replace_file_by_directory=False)
    changed = step(X, index, root, rules)
    assert (len(changed.create), len(changed.update), len(changed.remove)) == (6, 2 + 4, 4)
    assert changed.kind_changed == 0
    before = index.rows()
    second = step(X, index, root, rules)
    assert (second.create, second.update, second.remove, second.kind_changed) == ([], [], [], 0)
    assert set(second.state) == {X.UNCHANGED} and None not in second.match
    assert index.rows() == before and second.salt == 0


def test_salt_is_a_byte(ctx, tmp_path, monkeypatch):
    """A collision at salt 255 is followed by salt 0."""
    from spacedrive_amd import indexer as X
    root = str(tmp_path / "loc")
    os.makedirs(root)
    for name in ("x", "y"):
        open(os.path.join(root, name), "wb").close()
    real = X.path_keys

    def colliding(mps, names, exts, salt=0, ctx=None):
        keys = real(mps, names, exts, salt, ctx)
        if salt == 255 and keys.size == 2:
            keys[1] = keys[0]
        return keys

    monkeypatch.setattr(X, "path_keys", colliding)
    res = X.rescan(X.LocationIndex(), root, salt=255)
    assert res.salt == 0 and len(res.create) == 2
    with pytest.raises(ValueError):
        X.path_message("/", "a", "", salt=256)


def test_forced_collision_takes_the_resalt_path(ctx, tmp_path, monkeypatch):
    from spacedrive_amd import indexer as X
    root = str(tmp_path / "loc")
    os.makedirs(os.path.join(root, "a"))
    for name in ("x.txt", "y.txt", "z.txt"):
        open(os.path.join(root, "a", name), "wb").close()
    real, calls = X.path_keys, []

    def colliding(mps, names, exts, salt=0, ctx=None):
        keys = real(mps, names, exts, salt, ctx)
        t = list(zip(mps, names, exts))
        calls.append(salt)
        if salt == 0 and ("/a/", "x", "txt") in t and ("/a/", "y", "txt") in t:
            keys[t.index(("/a/", "y", "txt"))] = keys[t.index(("/a/", "x", "txt"))]
        return keys

    everything = lambda rel, is_dir: True  # noqa: E731
    monkeypatch.setattr(X, "path_keys", colliding)
    index = X.LocationIndex()
    first = step(X, index, root, everything)        # two walked paths share a key at salt 0
    assert first.salt == 1 and len(first.create) == 4 and 0 in calls and 1 in calls
    os.remove(os.path.join(root, "a", "y.txt"))
    second = step(X, index, root, everything)       # the rows share it now, the walk does not
    assert second.salt == 1 and len(second.remove) == 1 and not second.create

    # a new file whose key equals an existing row's at salt 0: unique on each
    # side, and the pair check finds the strings differ
    def crossing(mps, names, exts, salt=0, ctx=None):
        keys = real(mps, names, exts, salt, ctx)
        t = list(zip(mps, names, exts))
        if salt == 0 and ("/a/", "w", "txt") in t:
            keys[t.index(("/a/", "w", "txt"))] = real(["/a/"], ["z"], ["txt"], 0, ctx)[0]
        return keys

    os.rename(os.path.join(root, "a", "z.txt"), os.path.join(root, "a", "w.txt"))
    monkeypatch.setattr(X, "path_keys", crossing)
    third = step(X, index, root, everything)
    assert third.salt == 1 and len(third.create) == 1 and len(third.remove) == 1
    assert ("/a/", "w", "txt") in index.tuples() and ("/a/", "z", "txt") not in index.tuples()

    # a collision under every salt: three attempts, then the error
    def hopeless(mps, names, exts, salt=0, ctx=None):
        keys = real(mps, names, exts, salt, ctx)
        keys[:] = keys[:1] if keys.size else keys
        return keys

    monkeypatch.setattr(X, "path_keys", hopeless)
    with pytest.raises(X.KeyCollision):
        X.rescan(index, root, everything)
    assert np.unique(hopeless(["/", "/"], ["a", "b"], ["", ""])).size == 1
