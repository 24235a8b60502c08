"""CPU: dir_sizes.sizes_oracle is pinned to SQLite itself -- the reference's
store, asked the only way it can be asked (one prefix scan per directory) -- and
to hand-written answers for the malformed inputs."""
import sqlite3

import numpy as np

from spacedrive_amd.dir_sizes import MISS, sizes_oracle
from tests import dir_sizes_cases as C


def small_tree():
    """41 rows, depth 4; names with the LIKE wildcards % and _ and non-ASCII
    ones, so a prefix that was matched as a pattern would show."""
    rows = [("/", "100%", True, 0), ("/", "100_", True, 0), ("/", "1000", True, 0),
            ("/", "Übung", True, 0), ("/", "top.txt", False, 17), ("/", "empty", True, 0)]
    rows += [("/100%/", "a_b", True, 0), ("/100%/", "a%b", True, 0), ("/100%/", "axb", True, 0),
             ("/100%/", "f.bin", False, 1 << 35)]
    rows += [("/100%/a_b/", "x%d" % i, False, 100 + i) for i in range(4)]
    rows += [("/100%/a%b/", "y%d" % i, False, 1000 + i) for i in range(3)]
    rows += [("/100%/axb/", "z", False, 9), ("/100%/axb/", "日本", True, 0)]
    rows += [("/100%/axb/日本/", "深い", True, 0), ("/100%/axb/日本/", "файл", False, 4096)]
    rows += [("/100%/axb/日本/深い/", "k%d" % i, False, (1 << 32) + i) for i in range(5)]
    rows += [("/100_/", "p%d" % i, False, 7 * i) for i in range(9)]
    rows += [("/1000/", "q", False, 1), ("/1000/", "sub", True, 0), ("/1000/sub/", "r", False, 2)]
    rows += [("/Übung/", "é", False, 33), ("/Übung/", "ü_%", True, 0),
             ("/Übung/ü_%/", "s", False, 44)]
    return rows


def test_oracle_equals_sqlite_prefix_sums():
    rows = small_tree()
    assert len(rows) == 41 and max(mp.count("/") for mp, _, _, _ in rows) == 5
    db = sqlite3.connect(":memory:")
    db.execute("CREATE TABLE file_path (id INTEGER PRIMARY KEY, materialized_path TEXT, "
               "name TEXT, is_dir INTEGER, size INTEGER)")
    db.executemany("INSERT INTO file_path (materialized_path, name, is_dir, size) "
                   "VALUES (?, ?, ?, ?)", [(mp, nm, int(d), s) for mp, nm, d, s in rows])
    parent, total, files, counts = sizes_oracle(*C.columns(rows))
    q = ("SELECT COALESCE(SUM(size),0), COUNT(*) FROM file_path WHERE is_dir = 0 AND "
         "substr(materialized_path, 1, length(?)) = ?")
    dirs = 0
    for i, (mp, nm, d, s) in enumerate(rows):
        if d:
            prefix = mp + nm + "/"
            assert db.execute(q, (prefix, prefix)).fetchone() == (int(total[i]), int(files[i])), \
                prefix
            dirs += 1
        else:
            assert (int(total[i]), int(files[i])) == (s, 0)
        # the parent is the directory row whose children path is the row's own path
        want = [j for j, (m2, n2, d2, _) in enumerate(rows) if d2 and m2 + n2 + "/" == mp]
        assert parent[i] == (want[0] if want else MISS)
    top = [i for i, r in enumerate(rows) if r[0] == "/"]
    everything = db.execute("SELECT SUM(size) FROM file_path WHERE is_dir = 0").fetchone()[0]
    assert counts.tolist() == [dirs, dirs, len(top), everything]
    assert int(total[5]) == 0 and int(files[5]) == 0          # the empty directory


def test_oracle_does_not_depend_on_row_order():
    rows = small_tree()
    rng = np.random.default_rng(3)
    order = rng.permutation(len(rows)).tolist()
    _, total, files, counts = sizes_oracle(*C.columns(rows))
    _, t2, f2, c2 = sizes_oracle(*C.columns([rows[i] for i in order]))
    assert np.array_equal(t2, total[order]) and np.array_equal(f2, files[order])
    assert np.array_equal(c2, counts)


def test_malformed_inputs_against_hand_written_values():
    cols, want = C.malformed()
    got = sizes_oracle(*cols)
    for g, w, name in zip(got, want, ("parent", "total", "files", "counts")):
        assert g.dtype == w.dtype and g.tolist() == w.tolist(), name


def test_sums_wrap_modulo_two_to_the_64():
    rows = [("/", "d", True, 0), ("/d/", "a", False, (1 << 64) - 1), ("/d/", "b", False, 3),
            ("/", "c", False, (1 << 64) - 2)]
    parent, total, files, counts = sizes_oracle(*C.columns(rows))
    assert total.tolist() == [2, (1 << 64) - 1, 3, (1 << 64) - 2] and files[0] == 2
    assert counts.tolist() == [1, 1, 2, 0]


def test_no_directories_and_nothing():
    k = np.array([5, 5, 6], np.uint64)
    parent, total, files, counts = sizes_oracle(k, None, None, np.array([1, 2, 3], np.uint64))
    assert parent.tolist() == [MISS] * 3 and total.tolist() == [1, 2, 3]
    assert files.tolist() == [0, 0, 0] and counts.tolist() == [0, 0, 3, 6]
    e = np.zeros(0, np.uint64)
    parent, total, files, counts = sizes_oracle(e, e, np.zeros(0, np.uint8), e)
    assert parent.size == total.size == files.size == 0 and counts.tolist() == [0, 0, 0, 0]
