"""Plain numpy restatement of the explorer's search page (include/sdgpu.h,
"explorer: one search page"): filter, candidates, cursor predicate, order,
page and counts.  The product code never imports this; tests/test_search_
oracle.py pins it to SQLite itself.

Rows / objects are any objects with the header's field names as attributes
(numpy arrays or None); the query has the header's operand names."""
from types import SimpleNamespace

import numpy as np

NULL = -(1 << 62)
(USE_LOCATION, USE_EXTENSION, USE_CREATED_FROM, USE_CREATED_TO, USE_DIR, USE_FAVORITE,
 USE_HIDDEN_EXCLUDE, USE_KIND, USE_TAGS, USE_ACCESSED_EQ, USE_ACCESSED_NE) = (1 << b for b in range(11))
DESC, GROUP_DIRS, FILES_ONLY, CURSOR, CURSOR_STRICT, ORDER_BY_OBJECT, NEEDS_OBJECT = (
    1 << b for b in range(7))
OBJECT_TERMS = (USE_FAVORITE | USE_HIDDEN_EXCLUDE | USE_KIND | USE_TAGS | USE_ACCESSED_EQ
                | USE_ACCESSED_NE)


def rows(n, **cols):
    base = dict(n=n, location=None, ext=None, dir_key=None, flags=None, date_created=None,
                object=None, eligible=None, order_key=None)
    base.update(cols)
    return SimpleNamespace(**base)


def objects(m, **cols):
    base = dict(m=m, kind=None, flags=None, date_accessed=None, order_key=None,
                tag_obj=np.zeros(0, np.int32), tag_tag=np.zeros(0, np.int32))
    base.update(cols)
    base["n_pairs"] = len(base["tag_obj"])
    return SimpleNamespace(**base)


def query(**kw):
    base = dict(use=0, flags=0, location=0, ext=0, favorite=0, dir_key=0, created_from=0,
                created_to=0, kind_mask=0, tags=(), accessed_eq=0, accessed_ne=0, cursor_key=0,
                cursor_row=0, offset=0, take=0)
    base.update(kw)
    return SimpleNamespace(**base)


def search_page(r, o, q):
    """(page: uint32 row indices, counts: uint32[4])."""
    n = r.n
    counts = np.zeros(4, np.uint32)
    if n == 0:
        return np.zeros(0, np.uint32), counts
    idx = np.arange(n, dtype=np.int64)
    match = np.ones(n, bool) if r.eligible is None else np.asarray(r.eligible) != 0
    is_dir = np.zeros(n, bool) if r.flags is None else (np.asarray(r.flags) & 1) != 0
    use, fl = q.use, q.flags
    if use & USE_LOCATION:
        match &= (r.location != -1) & (r.location == q.location)
    if use & USE_EXTENSION:
        match &= (r.ext != 0xFFFF) & (r.ext == q.ext)
    if use & USE_CREATED_FROM:
        match &= (r.date_created != NULL) & (r.date_created >= q.created_from)
    if use & USE_CREATED_TO:
        match &= (r.date_created != NULL) & (r.date_created <= q.created_to)
    if use & USE_DIR:
        match &= r.dir_key == np.uint64(q.dir_key)
    has_obj = np.zeros(n, bool)
    ob = np.zeros(n, np.int64)
    if r.object is not None:
        ob = np.asarray(r.object).astype(np.int64)
        has_obj = ob >= 0
        if o is not None:
            has_obj &= ob < o.m
        ob = np.where(has_obj, ob, 0)
    if (use & OBJECT_TERMS) or (fl & NEEDS_OBJECT):
        match &= has_obj

    def gather(col):
        return np.asarray(col)[ob] if o.m else np.zeros(n, np.asarray(col).dtype)

    if use & USE_HIDDEN_EXCLUDE:
        match &= (gather(o.flags) & 4) == 0
    if use & USE_FAVORITE:
        f = gather(o.flags)
        match &= ((f & 1) != 0) if q.favorite else ((f & 3) == 0)
    if use & USE_KIND:
        k = gather(o.kind).astype(np.int64)
        ok = (k >= 0) & (k < 32)
        match &= ok & (((q.kind_mask >> np.where(ok, k, 0)) & 1) != 0)
    if use & USE_TAGS:
        mark = np.zeros(max(o.m, 1), bool)
        hit = np.isin(np.asarray(o.tag_tag), np.asarray(list(q.tags), np.int64))
        to = np.asarray(o.tag_obj)[hit]
        mark[to[(to >= 0) & (to < o.m)]] = True
        match &= mark[ob]
    if use & USE_ACCESSED_EQ:
        match &= gather(o.date_accessed) == q.accessed_eq     # the sentinel: IS NULL
    if use & USE_ACCESSED_NE:
        d = gather(o.date_accessed)
        match &= (d != NULL) if q.accessed_ne == NULL else ((d != NULL) & (d != q.accessed_ne))
    # the order key
    if fl & ORDER_BY_OBJECT:
        v = np.where(has_obj, gather(o.order_key), NULL)
        has_key = True
    elif r.order_key is not None:
        v = np.asarray(r.order_key).astype(np.int64)
        has_key = True
    else:
        v = np.full(n, NULL, np.int64)
        has_key = False
    cand = match.copy()
    if fl & FILES_ONLY:
        cand &= ~is_dir
    if fl & CURSOR:
        if not has_key:
            cand &= idx >= q.cursor_row
        else:
            c = q.cursor_key
            tie = (v == c) if not fl & CURSOR_STRICT else np.zeros(n, bool)
            if fl & DESC:
                ok = (v < c) | (tie & (idx < q.cursor_row))
            else:
                ok = (v > c) | (tie & (idx >= q.cursor_row))
            cand &= (v != NULL) & ok
    # order: directories first under GROUP_DIRS, the key (NULL lowest), the row
    group = (~is_dir).astype(np.int64) if fl & GROUP_DIRS else np.zeros(n, np.int64)
    primary = -v if fl & DESC else v               # NULL = -2^62 is below every value
    order = np.lexsort((idx, primary, group))
    order = order[cand[order]]
    counts[0] = match.sum()
    counts[1] = cand.sum()
    counts[3] = (match & is_dir).sum()
    page = order[q.offset:q.offset + q.take].astype(np.uint32)
    counts[2] = len(page)
    return page, counts


# ---- seeded random tables and queries (the GPU and the SQLite tests share them) ----

def random_table(rng, n, m, n_pairs, key_values=None):
    """Columns with NULLs and many ties.  Returns (rows, objects) of numpy arrays."""
    def nullable(vals, size, p_null, null, dtype):
        a = rng.choice(np.asarray(vals, dtype=dtype), size=size)
        a[rng.random(size) < p_null] = null
        return a

    kv = list(range(-4, 5)) + [(1 << 62) - 1, -(1 << 62) + 1] if key_values is None else key_values
    r = rows(
        n,
        location=nullable([1, 2, 3], n, 0.1, -1, np.int32),
        ext=nullable([0, 1, 2, 3], n, 0.1, 0xFFFF, np.uint16),
        dir_key=rng.choice(np.array([0, 7, 0xFFFFFFFFFFFFFFFF, 1 << 63], np.uint64), size=n),
        flags=(rng.random(n) < 0.3).astype(np.uint8),
        date_created=nullable(range(100, 110), n, 0.1, NULL, np.int64),
        object=rng.integers(-1, max(m, 1), size=n).astype(np.int32) if m else np.full(n, -1, np.int32),
        eligible=(rng.random(n) < 0.9).astype(np.uint8),
        order_key=nullable(kv, n, 0.15, NULL, np.int64))
    o = objects(
        m,
        kind=nullable(range(0, 24), m, 0.1, -1, np.int32),
        flags=rng.integers(0, 8, size=m).astype(np.uint8) & np.uint8(7),
        date_accessed=nullable(range(50, 54), m, 0.3, NULL, np.int64),
        order_key=nullable(kv, m, 0.15, NULL, np.int64),
        tag_obj=rng.integers(0, max(m, 1), size=n_pairs).astype(np.int32),
        tag_tag=rng.integers(1, 40, size=n_pairs).astype(np.int32))
    # favorite cannot be true and NULL at once
    o.flags = np.where(o.flags & 2, o.flags & ~np.uint8(1), o.flags).astype(np.uint8)
    return r, o


def random_query(rng, r, o, force_use=0, force_flags=0):
    use = force_use
    for b in range(11):
        if rng.random() < 0.2:
            use |= 1 << b
    if use & USE_ACCESSED_EQ and use & USE_ACCESSED_NE and rng.random() < 0.5:
        use &= ~USE_ACCESSED_EQ
    fl = force_flags
    for bit in (DESC, GROUP_DIRS, NEEDS_OBJECT, ORDER_BY_OBJECT):
        if rng.random() < 0.4:
            fl |= bit
    if rng.random() < 0.2:
        fl |= FILES_ONLY
    offset = 0
    if rng.random() < 0.5 or fl & (CURSOR | CURSOR_STRICT):
        fl |= CURSOR
        if rng.random() < 0.3:
            fl |= CURSOR_STRICT
    elif rng.random() < 0.7:
        offset = int(rng.integers(0, max(r.n // 2, 1) + 1))
    n_tags = int(rng.choice([0, 1, 3, 32]))
    pick = lambda vals: int(rng.choice(np.asarray(vals, dtype=np.int64)))  # noqa: E731
    null_or = lambda vals: NULL if rng.random() < 0.3 else pick(vals)  # noqa: E731
    return query(
        use=use, flags=fl, location=pick([1, 2, 3, -1]), ext=pick([0, 1, 2, 3, 0xFFFF]),
        favorite=pick([0, 1]), dir_key=int(rng.choice(np.array([0, 7, 0xFFFFFFFFFFFFFFFF, 1 << 63],
                                                               np.uint64))),
        created_from=pick(range(99, 111)), created_to=pick(range(99, 111)),
        kind_mask=int(rng.integers(0, 1 << 24)), tags=tuple(int(t) for t in rng.integers(1, 60, size=n_tags)),
        accessed_eq=null_or(range(50, 54)), accessed_ne=null_or(range(50, 54)),
        cursor_key=pick(list(range(-4, 5)) + [(1 << 62) - 1, -(1 << 62) + 1]),
        cursor_row=int(rng.integers(0, r.n + 1)), offset=offset,
        take=pick([0, 1, 5, 100, 256]))


def random_case(seed, max_n=3000, max_m=500):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, max_n + 1))
    m = int(rng.integers(0, max_m + 1))
    r, o = random_table(rng, n, m, int(rng.integers(0, 3 * m + 1)) if m else 0)
    if rng.random() < 0.15:
        r.order_key = None
    q = random_query(rng, r, o)
    return r, o, q
