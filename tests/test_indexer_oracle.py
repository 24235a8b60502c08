"""CPU: the indexer oracle (tests/indexer_oracle.py) against hand-written cases
that pin each rule of walk.rs:309-381,624-636 and indexer/mod.rs:305-388, and
its two restatements -- on string tuples and on integer keys -- against each
other."""
import random

import pytest

from tests import indexer_oracle as IO


@pytest.mark.parametrize("name", sorted(IO.CASES))
def test_hand_case(name):
    walk, rows, create, update, remove = IO.CASES[name]
    assert IO.diff_tuples(walk, rows) == (create, update, remove)
    cols, names = IO.to_columns(walk, rows)
    got = IO.diff_keys(*cols)
    assert IO.tuples_from_keys(got, names, rows) == (create, update, remove)
    assert got[5] == [len(create), len(update), len(remove),
                      1 if name == "file_replaced_by_directory" else 0]


def test_cases_cover_the_rules():
    assert len(IO.CASES) == 11
    states = set()
    for walk, rows, *_ in IO.CASES.values():
        states |= set(IO.diff_keys(*IO.to_columns(walk, rows)[0])[4])
    assert states == {IO.UNCHANGED, IO.UPDATE, IO.KIND_CHANGED}   # CREATE: the random trees
    cols, _ = IO.to_columns(*IO.CASES["ancestor_only_entry"][:2])
    assert sorted(cols[1]) == [0, 3]          # the file, and the directory as ANCESTOR
    assert IO.CASES["no_metadata_row"][1][0][5] is None


def test_the_time_test_is_one_sided_and_strict():
    e = IO._f("/", "a", "txt")
    for delta, want in ((IO.MS, 0), (IO.MS + 1, 1), (-IO.MS - 1, 0), (-3600 * 1000 * IO.MS, 0),
                        (0, 0), (1, 0)):
        walk = [("/", [e[:6] + (IO.T0 + delta,)])]
        assert len(IO.diff_tuples(walk, [IO._row(1, e)])[1]) == want, delta


def _random_tree(rng):
    """A walk and rows over a small name space: most things collide on purpose."""
    dirs = ["/"] + ["/d%d/" % i for i in range(3)] + ["/d0/e/"]
    names = ["a", "b", "c", "d0", "e"]
    meta = lambda: (rng.choice([1, 2]), rng.choice([1, 2]),  # noqa: E731
                    IO.T0 + rng.choice([0, IO.MS, IO.MS + 1, -5 * IO.MS]))
    seen, rows = set(), []
    for _ in range(rng.randrange(0, 14)):
        t = (rng.choice(dirs), rng.choice(names), rng.choice(["", "txt"]))
        if t in seen:
            continue
        seen.add(t)
        m = meta()
        if rng.random() < 0.2:
            m = (None,) + m[1:]
        rows.append((len(rows) + 1,) + t + (rng.random() < 0.3,) + m)
    walk, listed = [], set()
    for cp in rng.sample(dirs, rng.randrange(0, len(dirs) + 1)):
        buffer = []
        for _ in range(rng.randrange(0, 5)):
            t = (cp, rng.choice(names), rng.choice(["", "txt"]))
            if t in listed:
                continue
            listed.add(t)
            buffer.append(t + (rng.random() < 0.3,) + meta())
        walk.append((cp, buffer))
    # an ancestor pushed from a deeper directory, when its own listing did not have it
    if walk and ("/", "d0", "") not in listed and rng.random() < 0.5:
        walk[-1][1].append(("/", "d0", "", True) + meta())
    return walk, rows


def test_both_restatements_agree_on_random_trees():
    rng = random.Random(5)
    seen_states, removed, ancestors = set(), 0, 0
    for _ in range(600):
        walk, rows = _random_tree(rng)
        cols, names = IO.to_columns(walk, rows)
        got = IO.diff_keys(*cols)
        want = IO.diff_tuples(walk, rows)
        assert IO.tuples_from_keys(got, names, rows) == want
        seen_states |= set(got[4])
        removed += len(got[2])
        ancestors += sum(1 for f in cols[1] if f & 2)
    assert seen_states == {0, 1, 2, 3} and removed > 100 and ancestors > 20


def test_apply_skips_duplicates_and_clears_updated_ids():
    walk, rows, *_ = IO.CASES["file_replaced_by_directory"]
    after, cleared = IO.apply_tuples(rows, walk, IO.diff_tuples(walk, rows), 2)
    assert after == rows and cleared == []            # the old row stays, nothing is added
    walk, rows, *_ = IO.CASES["inode_only"]
    after, cleared = IO.apply_tuples(rows, walk, IO.diff_tuples(walk, rows), 2)
    assert cleared == [1] and after[0][5] == 10 and rows[0][5] == 11


def test_oracle_imports_nothing_from_the_product():
    text = open(IO.__file__).read()
    assert "import" not in text.split('"""', 2)[2]
