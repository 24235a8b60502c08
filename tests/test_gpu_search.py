"""GPU: the explorer's search page (sdgpu_search_page_device, search.hip) against
the numpy restatement of include/sdgpu.h (tests/search_oracle.py, itself pinned
to SQLite by tests/test_search_oracle.py).  In every case d_page and d_counts
are pre-filled with 0xA5 and the page must stay untouched past counts[2].  The
shapes sit where the kernels can go wrong: tile and wave boundaries of the
compaction, the final-sort bound SELECT_FINAL_RECORDS and one past it, buckets
far larger than the page at the page's boundary, keys that differ only in the
first or only in the last digits, the extremes of the value range and NULLs."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests import search_oracle as SO  # noqa: E402
from spacedrive_amd import explorer as E  # noqa: E402

S = E.SELECT_FINAL_RECORDS
POISON = np.uint32(0xA5A5A5A5)
BIG = 4 * S + 1


def _dev(a):
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        a = a.view(np.int16)
    elif a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(a).cuda()


def to_device(r, o):
    rows = E.Rows(r.n, *(_dev(getattr(r, c)) for c in E.ROW_COLUMNS))
    objs = None if o is None else E.Objects(o.m, *(_dev(getattr(o, c)) for c in E.OBJECT_COLUMNS))
    return rows, objs


def as_query(q):
    return E.Query(**{k: getattr(q, k) for k in E.Query.__dataclass_fields__})


def run_device(r, o, q, ctx=None, dev=None):
    rows, objs = dev if dev is not None else to_device(r, o)
    page = torch.full((E.MAX_TAKE,), int(POISON.view(np.int32)), dtype=torch.int32, device="cuda")
    counts = torch.full((4,), int(POISON.view(np.int32)), dtype=torch.int32, device="cuda")
    E.search_page(rows, objs, as_query(q), ctx=ctx, page=page, counts=counts)
    torch.cuda.synchronize()
    return page.cpu().numpy().view(np.uint32), counts.cpu().numpy().view(np.uint32)


def check(r, o, q, ctx=None, dev=None):
    want_page, want_counts = SO.search_page(r, o, q)
    page, counts = run_device(r, o, q, ctx, dev)
    np.testing.assert_array_equal(counts, want_counts)
    P = int(counts[2])
    np.testing.assert_array_equal(page[:P], want_page)
    assert (page[P:] == POISON).all(), "written past the page"
    return page[:P], counts


def plain_rows(n, key=None, flags=None, eligible=None):
    return SO.rows(n, order_key=key, flags=flags, eligible=eligible)


# ---- compaction boundaries -----------------------------------------------------------

@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1025])
def test_compaction_boundaries(n):
    rng = np.random.default_rng(n)
    key = rng.integers(-3, 4, size=n).astype(np.int64)
    one = lambda i: np.eye(1, n, i, dtype=np.uint8)[0]  # noqa: E731
    for eligible in (None, np.zeros(n, np.uint8), one(0), one(n - 1),
                     (rng.random(n) < 0.5).astype(np.uint8)):
        for take in (0, 1, 100, 256):
            p, c = check(plain_rows(n, key, eligible=eligible), None, SO.query(take=take))
            if eligible is None:
                assert c[0] == c[1] == n and c[2] == min(take, n)


# ---- selection ---------------------------------------------------------------------

def _selection_cases():
    rng = np.random.default_rng(11)
    n = BIG
    equal = np.full(n, 5, np.int64)
    two = np.where(rng.random(n) < 0.5, -7, 9).astype(np.int64)
    n_low = int((two == -7).sum())
    top = ((rng.integers(0, 1024, size=n) - 512) << 52).astype(np.int64)
    low = rng.integers(0, 256, size=n).astype(np.int64)
    ext = rng.choice(np.array([(1 << 62) - 1, -(1 << 62) + 1, 0, SO.NULL], np.int64), size=n)
    nulls = np.where(rng.random(n) < 0.5, SO.NULL, rng.integers(-2, 3, size=n)).astype(np.int64)
    cases = []
    for desc in (0, SO.DESC):
        d = "desc" if desc else "asc"
        cases += [
            (f"equal-mid-{d}", equal, dict(flags=desc, offset=2 * S + 7, take=100)),
            (f"equal-0-{d}", equal, dict(flags=desc, offset=0, take=256)),
            (f"equal-end-{d}", equal, dict(flags=desc, offset=n - 3, take=100)),
            (f"two-boundary-{d}", two, dict(flags=desc, take=100,
                                             offset=(n - n_low if desc else n_low) - 50)),
            (f"two-0-{d}", two, dict(flags=desc, offset=0, take=100)),
            (f"top-digit-{d}", top, dict(flags=desc, offset=0, take=100)),
            (f"top-digit-off-{d}", top, dict(flags=desc, offset=n // 2, take=256)),
            (f"low-digit-{d}", low, dict(flags=desc, offset=0, take=100)),
            (f"low-digit-off-{d}", low, dict(flags=desc, offset=n // 3, take=100)),
            (f"extremes-{d}", ext, dict(flags=desc, offset=0, take=256)),
            (f"extremes-off-{d}", ext, dict(flags=desc, offset=n // 4 - 10, take=100)),
            (f"nulls-{d}", nulls, dict(flags=desc, offset=0, take=100)),
            (f"nulls-off-{d}", nulls, dict(flags=desc, offset=n // 2 - 20, take=100)),
        ]
    return cases


_SELECTION = _selection_cases()


@pytest.mark.parametrize("name,key,kw", _SELECTION, ids=[c[0] for c in _SELECTION])
def test_selection(name, key, kw):
    p, c = check(plain_rows(len(key), key), None, SO.query(**kw))
    assert c[1] == len(key) and c[2] == min(kw["take"], len(key) - kw["offset"])


@pytest.mark.parametrize("take", [0, 1, 100, 256])
def test_take_and_offsets_around_the_end(take):
    rng = np.random.default_rng(take)
    n = S + 500
    key = rng.integers(-50, 50, size=n).astype(np.int64)
    eligible = (rng.random(n) < 0.97).astype(np.uint8)
    cand = int(eligible.sum())
    assert cand > S
    for offset in (0, cand - 1, cand, cand + 1, cand + 1000, cand - take // 2, cand - take):
        if offset < 0:
            continue
        check(plain_rows(n, key, eligible=eligible), None, SO.query(take=take, offset=offset))


@pytest.mark.parametrize("cand,n", [(c, n) for n in (S, S + 1, BIG)
                                    for c in (1, S - 1, S, S + 1, S + 2) if c <= n])
def test_final_sort_bound(cand, n):
    """Candidates <= S take the direct path (from the host when n <= S, from the
    first pass's state otherwise); S + 1 is the first count a pass runs for."""
    rng = np.random.default_rng(cand * 7 + n)
    key = rng.integers(-(1 << 40), 1 << 40, size=n).astype(np.int64)
    eligible = np.zeros(n, np.uint8)
    eligible[rng.choice(n, size=cand, replace=False)] = 1
    for q in (SO.query(take=100), SO.query(take=256, offset=cand // 2),
              SO.query(take=100, flags=SO.DESC, offset=max(cand - 60, 0))):
        check(plain_rows(n, key, eligible=eligible), None, q)


# ---- cursor -------------------------------------------------------------------------

@pytest.mark.parametrize("desc", [0, SO.DESC])
@pytest.mark.parametrize("strict", [0, SO.CURSOR_STRICT])
def test_cursor_inside_a_run_of_equal_keys(desc, strict):
    n = 1000
    key = np.repeat(np.arange(10, dtype=np.int64), 100)
    key[::7] = SO.NULL                        # present and never returned
    rng = np.random.default_rng(3)
    rng.shuffle(key)
    rows = plain_rows(n, key)
    for cursor_row in (0, 1, 499, 500, 999, 1000):
        q = SO.query(flags=SO.CURSOR | desc | strict, cursor_key=4, cursor_row=cursor_row, take=100)
        p, c = check(rows, None, q)
        assert (key[p] != SO.NULL).all()
    # a NULL cursor key compares with nothing the way SQL does not: every non-NULL
    # key is above the sentinel ascending, none is below it descending
    check(rows, None, SO.query(flags=SO.CURSOR | desc | strict, cursor_key=SO.NULL, take=100))


def test_cursor_without_an_order_key():
    n = 700
    rows = plain_rows(n, None, flags=(np.arange(n) % 3 == 0).astype(np.uint8))
    for cursor_row in (0, 1, 350, 699, 700):
        for fl in (0, SO.GROUP_DIRS, SO.GROUP_DIRS | SO.FILES_ONLY):
            check(rows, None, SO.query(flags=SO.CURSOR | fl, cursor_row=cursor_row, take=100))


@pytest.mark.parametrize("desc", [0, SO.DESC])
def test_order_by_object_with_rows_that_have_none(desc):
    rng = np.random.default_rng(5)
    r, o = SO.random_table(rng, 2000, 300, 0)
    for fl in (0, SO.CURSOR | SO.CURSOR_STRICT, SO.CURSOR, SO.NEEDS_OBJECT):
        q = SO.query(flags=SO.ORDER_BY_OBJECT | desc | fl, cursor_key=1, cursor_row=900, take=100)
        p, c = check(r, o, q)
        if fl & SO.CURSOR:
            assert (r.object[p] >= 0).all()


def test_order_by_object_with_no_objects_at_all():
    """m == 0: every order key is NULL, so a cursor reaches no row, and without one
    the rows come in id order; the Object columns may then be NULL pointers."""
    n = 300
    r = SO.rows(n, object=np.full(n, -1, np.int32), flags=(np.arange(n) % 4 == 0).astype(np.uint8))
    o = SO.objects(0, order_key=np.zeros(0, np.int64))
    for fl in (SO.CURSOR, SO.CURSOR | SO.DESC, SO.CURSOR | SO.CURSOR_STRICT):
        p, c = check(r, o, SO.query(flags=SO.ORDER_BY_OBJECT | fl, cursor_row=10, take=100))
        assert c[0] == n and c[1] == 0 and c[2] == 0
    p, c = check(r, o, SO.query(flags=SO.ORDER_BY_OBJECT | SO.GROUP_DIRS, take=100))
    assert c[1] == n and len(p) == 100


# ---- grouping -----------------------------------------------------------------------

@pytest.mark.parametrize("desc", [0, SO.DESC])
def test_group_dirs_straddling_the_boundary(desc):
    rng = np.random.default_rng(8)
    n = S + 300
    flags = (rng.random(n) < 0.5).astype(np.uint8)
    key = rng.integers(-20, 20, size=n).astype(np.int64)
    dirs = int(flags.sum())
    rows = plain_rows(n, key, flags=flags)
    p, c = check(rows, None, SO.query(flags=SO.GROUP_DIRS | desc, offset=dirs - 40, take=100))
    assert flags[p[:40]].all() and not flags[p[40:]].any() and c[3] == dirs
    check(rows, None, SO.query(flags=SO.GROUP_DIRS | desc, take=100))
    p, c = check(rows, None, SO.query(flags=SO.GROUP_DIRS | SO.FILES_ONLY | desc, take=100))
    assert not flags[p].any() and c[0] == n and c[1] == n - dirs and c[3] == dirs
    small = plain_rows(90, key[:90], flags=flags[:90])
    check(small, None, SO.query(flags=SO.GROUP_DIRS | desc, take=100))


# ---- filter -------------------------------------------------------------------------

@pytest.fixture(scope="module")
def table():
    rng = np.random.default_rng(21)
    r, o = SO.random_table(rng, 2500, 400, 900)
    # duplicate pairs
    o.tag_obj = np.concatenate([o.tag_obj, o.tag_obj[:200]])
    o.tag_tag = np.concatenate([o.tag_tag, o.tag_tag[:200]])
    o.n_pairs = len(o.tag_obj)
    return r, o, to_device(r, o)


OPERANDS = dict(location=2, ext=1, created_from=102, created_to=107, dir_key=(1 << 64) - 1,
                favorite=1, kind_mask=(1 << 5) | (1 << 7) | (1 << 23), tags=(3, 9, 17),
                accessed_eq=51, accessed_ne=52)


@pytest.mark.parametrize("bit", range(11))
def test_each_term_alone(table, bit):
    r, o, dev = table
    p, c = check(r, o, SO.query(use=1 << bit, take=256, **OPERANDS), dev=dev)
    assert 0 < c[0] < r.n


def test_all_terms_together_and_variants(table):
    r, o, dev = table
    allbits = (1 << 11) - 1
    check(r, o, SO.query(use=allbits & ~SO.USE_ACCESSED_NE, take=256, **OPERANDS), dev=dev)
    check(r, o, SO.query(use=allbits & ~SO.USE_ACCESSED_EQ, take=256, **OPERANDS), dev=dev)
    loose = SO.USE_HIDDEN_EXCLUDE | SO.USE_KIND | SO.USE_TAGS | SO.USE_CREATED_FROM
    p, c = check(r, o, SO.query(use=loose, take=256, **OPERANDS), dev=dev)
    assert c[0] > 0
    for v in (SO.NULL, 50):
        kw = dict(OPERANDS, accessed_eq=v, accessed_ne=v)
        check(r, o, SO.query(use=SO.USE_ACCESSED_EQ, take=256, **kw), dev=dev)
        check(r, o, SO.query(use=SO.USE_ACCESSED_NE, take=256, **kw), dev=dev)


def test_rows_without_an_object(table):
    r, o, dev = table
    none = int((r.object < 0).sum())
    assert none > 0
    p, c = check(r, o, SO.query(take=0, flags=SO.NEEDS_OBJECT), dev=dev)
    assert c[0] == int(r.eligible.astype(bool)[r.object >= 0].sum())
    p, c = check(r, o, SO.query(take=0), dev=dev)
    assert c[0] == int(r.eligible.sum())
    # NEEDS_OBJECT needs no Object columns
    check(r, None, SO.query(take=100, flags=SO.NEEDS_OBJECT))


def test_favorite_false_against_null(table):
    r, o, dev = table
    assert ((o.flags & 3) == 2).any()
    p, c = check(r, o, SO.query(use=SO.USE_FAVORITE, favorite=0, take=256), dev=dev)
    assert ((o.flags[r.object[p]] & 3) == 0).all() and c[0] > 0


def test_tags(table):
    r, o, dev = table
    check(r, o, SO.query(use=SO.USE_TAGS, tags=(1000, 1001), take=100), dev=dev)      # absent
    p, c = check(r, o, SO.query(use=SO.USE_TAGS, tags=tuple(range(1, 33)), take=100), dev=dev)
    assert c[0] > 0
    check(r, o, SO.query(use=SO.USE_TAGS, tags=(), take=100), dev=dev)
    bare = SO.objects(o.m, kind=o.kind, flags=o.flags, date_accessed=o.date_accessed,
                      order_key=o.order_key)
    p, c = check(r, bare, SO.query(use=SO.USE_TAGS, tags=(3,), take=100))             # no pairs
    assert c[0] == 0


# ---- random ---------------------------------------------------------------------------

@pytest.mark.parametrize("chunk", range(4))
def test_random_queries(chunk):
    for seed in range(chunk * 50, chunk * 50 + 50):
        r, o, q = SO.random_case(seed)
        check(r, o, q)


# ---- plumbing -------------------------------------------------------------------------

def test_caller_stream_and_back_to_back_calls():
    from spacedrive_amd._native import Context
    rng = np.random.default_rng(31)
    big_r, big_o = SO.random_table(rng, BIG, 300, 500)
    small_r, small_o = SO.random_table(rng, S + 40, 100, 50)
    with Context(0) as ctx:
        stream = torch.cuda.Stream()      # non-blocking with respect to the null stream
        d_big, d_small = to_device(big_r, big_o), to_device(small_r, small_o)
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            q1 = SO.query(use=SO.USE_TAGS, tags=(2, 3, 4), flags=SO.GROUP_DIRS, offset=700, take=100)
            q2 = SO.query(use=SO.USE_KIND, kind_mask=0xFFF, flags=SO.DESC, take=256)
            check(big_r, big_o, q1, ctx=ctx, dev=d_big)
            check(small_r, small_o, q2, ctx=ctx, dev=d_small)     # fewer rows, same workspace
            check(big_r, big_o, q2, ctx=ctx, dev=d_big)
            check(small_r, small_o, q1, ctx=ctx, dev=d_small)


def test_host_entry_point_equals_the_device_one():
    for seed in (1000, 1001, 1002, 1003, 1004, 1005):
        r, o, q = SO.random_case(seed)
        rows = E.Rows(r.n, *(getattr(r, c) for c in E.ROW_COLUMNS))
        objs = E.Objects(o.m, *(getattr(o, c) for c in E.OBJECT_COLUMNS))
        page, counts = E.search_page_host(rows, objs, as_query(q))
        d_page, d_counts = check(r, o, q)
        np.testing.assert_array_equal(counts, d_counts)
        np.testing.assert_array_equal(page, d_page)
    rng = np.random.default_rng(9)
    key = rng.integers(-9, 9, size=BIG).astype(np.int64)
    page, counts = E.search_page_host(E.Rows(BIG, order_key=key), None,
                                      E.Query(offset=BIG // 2, take=100))
    want, wc = SO.search_page(plain_rows(BIG, key), None, SO.query(offset=BIG // 2, take=100))
    np.testing.assert_array_equal(page, want)
    np.testing.assert_array_equal(counts, wc)


def test_paths_end_to_end(tmp_path):
    from spacedrive_amd.file_identifier import FilePaths
    t = FilePaths()
    t.add(1, "/", "docs", True)
    t.add(1, "/", "pics", True)
    names = ["b.jpg", "a.jpg", "C.png", "notes.txt", "a.JPG", "zz"]
    for nm in names:
        t.add(1, "/pics/", nm)
    t.add(1, "/pics/", "sub", True)
    t.add(1, "/docs/", "a.jpg")
    t.add(2, "/pics/", "other.jpg")
    for i in range(len(t)):
        if not t.is_dir[i]:
            t.cas_id[i] = "%016x" % (0xA100000000000000 + i)
            t.object_id[i] = i + 1
    attrs = E.ObjectAttrs(kind={i + 1: (5 if t.name[i].lower().endswith(("jpg", "png")) else 3)
                                for i in range(len(t)) if not t.is_dir[i]},
                          hidden={4: True}, favorite={3: True, 5: False},
                          date_accessed={3: 1000, 4: 2000}, tags=[(3, 7), (3, 7), (5, 8)])
    created = [100 + i for i in range(len(t))]
    cols = E.SearchColumns(t, attrs, date_created=created)
    by_name = {"orderOnly": {"field": "name", "value": "Asc"}}
    folder = {"locationId": 1, "path": "pics"}
    # a folder view: the directory first, then the names in BINARY order; rows
    # of directories have no Object, and the default hidden: Exclude is only
    # switched on with an `object` filter (search.rs:178-182)
    got = E.paths(cols, 100, by_name, folder)
    assert [t.name[x["row"]] for x in got] == ["sub", "C.png", "a.JPG", "a.jpg", "b.jpg",
                                               "notes.txt", "zz"]
    assert E.paths_count(cols, folder) == 7
    # hidden: Exclude through an (empty) object filter drops the directory and the hidden row
    got = E.paths(cols, 100, by_name, dict(folder, object={}))
    assert [t.name[x["row"]] for x in got] == ["C.png", "a.JPG", "b.jpg", "notes.txt", "zz"]
    # the cursor: after "a.jpg" (id 4), files only
    cur = {"cursor": {"id": 4, "cursor": {"isDir": False, "variant": {
        "name": {"order": "Asc", "data": "a.jpg"}}}}}
    got = E.paths(cols, 2, cur, folder)
    assert [t.name[x["row"]] for x in got] == ["b.jpg", "notes.txt"]
    # category, extension, search, tags, take.min(100), MaybeNot
    photos = E.paths(cols, 255, by_name, {"locationId": 1, "object": {"category": "Photos"}})
    assert [t.name[x["row"]] for x in photos] == ["C.png", "a.JPG", "a.jpg", "b.jpg"]
    assert E.paths(cols, 10, None, {"object": {"category": "Trash"}}) == []
    assert E.paths_count(cols, {"extension": "jpg"}) == 4
    assert E.paths_count(cols, {"extension": "nope"}) == 0
    assert E.paths_count(cols, {"search": "A.J"}) == 3
    assert E.paths_count(cols, {"search": ""}) == len(t)
    assert E.paths_count(cols, {"object": {"tags": [7], "hidden": "include"}}) == 1
    assert E.paths_count(cols, {"object": {"dateAccessed": {"not": None}, "hidden": "include"}}) == 2
    assert E.paths_count(cols, {"object": {"dateAccessed": None, "hidden": "include"}}) == 6
    assert E.paths_count(cols, {"createdAt": {"from": 103, "to": 105}}) == 3
    with pytest.raises(LookupError, match="Directory not found"):
        E.paths(cols, 10, None, {"locationId": 1, "path": "missing"})
    # has_local_thumbnail from the existing presence call
    thumbs = np.array([int.from_bytes(bytes.fromhex(t.cas_id[3]), "little"), 12345], np.uint64)
    got = E.paths(cols, 100, by_name, folder, thumb_keys=_dev(thumbs))
    assert [x["has_local_thumbnail"] for x in got] == [False, False, False, True, False, False,
                                                       False]
    assert got[0]["thumbnail_key"] is None and got[3]["thumbnail_key"] == [t.cas_id[3]]
    # search.objects over the Object columns as rows
    assert E.objects_count(cols, {"hidden": "include"}) == 8
    assert E.objects_count(cols) == 7
    by_kind = {"orderOnly": {"field": "kind", "value": "Desc"}}
    got = E.objects(cols, 3, by_kind, {"favorite": True})
    assert got == [3]
    got = E.objects(cols, 100, by_kind, None)
    kinds = [attrs.kind[x] for x in got]
    assert kinds == sorted(kinds, reverse=True) and len(got) == 7
    # a cursor through search.objects: Object ids are not row index + 1 (3, 4, 5, 6,
    # 7, 8, 10, 11 here, 4 hidden), so cursor_row comes from the ids themselves
    cur = lambda cid, variant: {"cursor": {"id": cid, "cursor": variant}}  # noqa: E731
    assert E.objects(cols, 100, cur(6, "none"), None) == [7, 8, 10, 11]
    assert E.objects(cols, 100, cur(9, "none"), None) == [10, 11]          # an id no Object has
    asc = {"kind": {"order": "Asc", "data": 3}}
    assert E.objects(cols, 100, cur(6, asc), None) == [8, 3, 5, 7, 10, 11]
    desc = {"kind": {"order": "Desc", "data": 5}}
    assert E.objects(cols, 100, cur(7, desc), None) == [3, 5, 6, 8]
