"""CPU: the search oracle (tests/search_oracle.py) pinned to SQLite itself, the
engine the reference's Prisma client runs search.paths on (core/src/api/
search.rs:393-562).  file_path, object and tag_on_object are built in memory
from random columns with NULLs; the reference's query is written as SQL -- a
LEFT JOIN for the Object terms and orders, EXISTS for the tags, ORDER BY is_dir
DESC, field, id, LIMIT / OFFSET, and the cursor's OR / AND arms of :463-475
verbatim, the descending `id <` included.  The `, id ASC` term added where the
reference has none (OrderOnly, Offset) is the stated deviation: one of the
orders SQLite may return."""
import sqlite3

import numpy as np

from tests import search_oracle as SO


def _val(x, null):
    return None if x == null else int(x)


def build_db(r, o):
    db = sqlite3.connect(":memory:")
    db.execute("CREATE TABLE file_path (id INTEGER PRIMARY KEY, location_id INTEGER, ext INTEGER,"
               " dir_key INTEGER, is_dir INTEGER, date_created INTEGER, object_id INTEGER,"
               " eligible INTEGER, okey INTEGER)")
    db.execute("CREATE TABLE object (id INTEGER PRIMARY KEY, kind INTEGER, favorite INTEGER,"
               " hidden INTEGER, date_accessed INTEGER, okey INTEGER)")
    db.execute("CREATE TABLE tag_on_object (object_id INTEGER, tag_id INTEGER)")
    dk = r.dir_key.view(np.int64)
    m = o.m if o is not None else 0
    rows = []
    for i in range(r.n):
        ob = int(r.object[i])
        rows.append((i + 1, _val(r.location[i], -1), _val(r.ext[i], 0xFFFF), int(dk[i]),
                     int(r.flags[i] & 1), _val(r.date_created[i], SO.NULL),
                     ob + 1 if 0 <= ob < m else None, int(r.eligible[i]),
                     None if r.order_key is None else _val(r.order_key[i], SO.NULL)))
    db.executemany("INSERT INTO file_path VALUES (?,?,?,?,?,?,?,?,?)", rows)
    objs = []
    for j in range(m):
        f = int(o.flags[j])
        # hidden: true, or one of the two values that are "not true"
        hidden = 1 if f & 4 else (None if j % 2 else 0)
        objs.append((j + 1, _val(o.kind[j], -1), None if f & 2 else f & 1, hidden,
                     _val(o.date_accessed[j], SO.NULL), _val(o.order_key[j], SO.NULL)))
    db.executemany("INSERT INTO object VALUES (?,?,?,?,?,?)", objs)
    if m:
        db.executemany("INSERT INTO tag_on_object VALUES (?,?)",
                       [(int(a) + 1, int(b)) for a, b in zip(o.tag_obj, o.tag_tag)])
    return db


def sql_page(db, r, q):
    """(page, counts) the way the reference asks SQLite for them."""
    use, fl = q.use, q.flags
    where, args = ["fp.eligible <> 0"], []

    def term(sql, *a):
        where.append(sql)
        args.extend(a)

    if use & SO.USE_LOCATION:
        term("fp.location_id = ?", q.location)
    if use & SO.USE_EXTENSION:
        term("fp.ext = ?", q.ext)
    if use & SO.USE_CREATED_FROM:
        term("fp.date_created >= ?", q.created_from)
    if use & SO.USE_CREATED_TO:
        term("fp.date_created <= ?", q.created_to)
    if use & SO.USE_DIR:
        term("fp.dir_key = ?", int(np.uint64(q.dir_key).view(np.int64)))
    if (use & SO.OBJECT_TERMS) or (fl & SO.NEEDS_OBJECT):
        term("o.id IS NOT NULL")                                   # object::is(params)
    if use & SO.USE_HIDDEN_EXCLUDE:
        term("(o.hidden IS NULL OR o.hidden <> 1)")                # search.rs:276-279
    if use & SO.USE_FAVORITE:
        term("o.favorite = ?", q.favorite)
    if use & SO.USE_KIND:
        kinds = [k for k in range(32) if (q.kind_mask >> k) & 1]
        term("o.kind IN (%s)" % ",".join(map(str, kinds)))
    if use & SO.USE_TAGS:
        term("EXISTS (SELECT 1 FROM tag_on_object t WHERE t.object_id = o.id AND t.tag_id IN (%s))"
             % ",".join(map(str, q.tags)))
    if use & SO.USE_ACCESSED_EQ:
        if q.accessed_eq == SO.NULL:
            term("o.date_accessed IS NULL")
        else:
            term("o.date_accessed = ?", q.accessed_eq)
    if use & SO.USE_ACCESSED_NE:
        if q.accessed_ne == SO.NULL:
            term("NOT (o.date_accessed IS NULL)")
        else:
            term("NOT (o.date_accessed = ?)", q.accessed_ne)
    src = "FROM file_path fp LEFT JOIN object o ON o.id = fp.object_id WHERE "
    filt = " AND ".join(where)
    matching = db.execute("SELECT COUNT(*), COALESCE(SUM(fp.is_dir = 1), 0) " + src + filt,
                          args).fetchone()
    key = "o.okey" if fl & SO.ORDER_BY_OBJECT else ("fp.okey" if r.order_key is not None else None)
    desc = bool(fl & SO.DESC)
    cand, cargs = [filt], list(args)
    if fl & SO.FILES_ONLY:
        cand.append("fp.is_dir <> 1")                              # :453-455
    if fl & SO.CURSOR:
        # the caller's cursor_row back into the cursor's id (ids are 1..n)
        cid = q.cursor_row + 1 if desc else q.cursor_row
        if key is None:
            cand.append("fp.id > ?")                               # :483-485, no direction
            cargs.append(q.cursor_row)
        elif fl & SO.CURSOR_STRICT:
            cand.append(f"{key} {'<' if desc else '>'} ?")         # :497-515
            cargs.append(q.cursor_key)
        else:                                                      # :463-475
            cand.append(f"({key} {'<' if desc else '>'} ? OR "
                        f"({key} = ? AND fp.id {'<' if desc else '>'} ?))")
            cargs += [q.cursor_key, q.cursor_key, cid]
    csql = " AND ".join(cand)
    n_cand = db.execute("SELECT COUNT(*) " + src + csql, cargs).fetchone()[0]
    order = []
    if fl & SO.GROUP_DIRS:
        order.append("fp.is_dir DESC")                             # :429-431
    if key is not None:
        order.append(f"{key} {'DESC' if desc else 'ASC'}")
    order.append("fp.id ASC")                                      # :526-527; the deviation
    page = [x[0] - 1 for x in db.execute(
        "SELECT fp.id " + src + csql + " ORDER BY " + ", ".join(order) + " LIMIT ? OFFSET ?",
        cargs + [q.take, q.offset])]
    return np.array(page, np.uint32), np.array([matching[0], n_cand, len(page), matching[1]],
                                               np.uint32)


def test_sqlite_is_the_engine_assumed():
    assert sqlite3.sqlite_version_info >= (3, 30)
    db = sqlite3.connect(":memory:")
    # NULLs sort first ascending and last descending; a comparison with NULL is not true
    db.execute("CREATE TABLE t (v INTEGER)")
    db.executemany("INSERT INTO t VALUES (?)", [(2,), (None,), (1,)])
    assert [x[0] for x in db.execute("SELECT v FROM t ORDER BY v ASC")] == [None, 1, 2]
    assert [x[0] for x in db.execute("SELECT v FROM t ORDER BY v DESC")] == [2, 1, None]
    assert db.execute("SELECT COUNT(*) FROM t WHERE NOT (v = 1)").fetchone()[0] == 1


def test_oracle_equals_sqlite_over_seeded_queries():
    seen_use = seen_flags = 0
    pages = 0
    for seed in range(400):
        r, o, q = SO.random_case(seed, max_n=300, max_m=60)
        if q.cursor_key == SO.NULL:
            continue
        db = build_db(r, o)
        want_page, want_counts = sql_page(db, r, q)
        page, counts = SO.search_page(r, o, q)
        np.testing.assert_array_equal(counts, want_counts, err_msg=f"seed {seed}")
        np.testing.assert_array_equal(page, want_page, err_msg=f"seed {seed}")
        seen_use |= q.use
        seen_flags |= q.flags
        pages += len(page) > 0
        db.close()
    assert seen_use == (1 << 11) - 1 and seen_flags == (1 << 7) - 1
    assert pages >= 150


def test_each_term_and_direction_against_sqlite():
    rng = np.random.default_rng(77)
    r, o = SO.random_table(rng, 400, 80, 200)
    db = build_db(r, o)
    ops = dict(location=2, ext=1, created_from=102, created_to=107, dir_key=(1 << 64) - 1,
               favorite=0, kind_mask=0xF0F0F0, tags=(3, 9, 17), accessed_eq=SO.NULL,
               accessed_ne=52)
    n = 0
    for bit in range(11):
        for fl in (0, SO.DESC, SO.GROUP_DIRS, SO.GROUP_DIRS | SO.DESC | SO.FILES_ONLY,
                   SO.ORDER_BY_OBJECT, SO.ORDER_BY_OBJECT | SO.DESC,
                   SO.CURSOR, SO.CURSOR | SO.DESC, SO.CURSOR | SO.CURSOR_STRICT | SO.ORDER_BY_OBJECT):
            q = SO.query(use=1 << bit, flags=fl, cursor_key=1, cursor_row=200, take=100,
                         offset=0 if fl & SO.CURSOR else 3, **ops)
            want_page, want_counts = sql_page(db, r, q)
            page, counts = SO.search_page(r, o, q)
            np.testing.assert_array_equal(counts, want_counts)
            np.testing.assert_array_equal(page, want_page)
            n += 1
    assert n == 99
