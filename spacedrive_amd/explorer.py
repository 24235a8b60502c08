"""The explorer's search page (core/src/api/search.rs:393-562 search.paths,
:563-582 pathsCount, :583-708 search.objects) from the columns the jobs already
keep on the device: one call filters, orders, applies the cursor or the offset
and takes the page (sdgpu_search_page_device, include/sdgpu.h).

* ``search_page`` / ``search_page_host`` -- the two entry points on tensors /
  numpy arrays.
* ``SearchColumns`` -- the columns and the extension dictionary of a FilePaths
  table plus Object attributes.
* ``paths`` / ``paths_count`` -- the reference's FilePathSearchArgs translated
  into a query; ``objects`` / ``objects_count`` the same over the Object columns
  as rows.
* ``name_contains`` -- the `search` terms as the call's eligible column.

Deviations: where the reference gives no final id order
(OrderOnly, Offset) ties go by ascending id, one of the orders SQLite may
return; search.objects orders ties by pub_id (search.rs:657-658), here by id.
"""
from __future__ import annotations

import bisect
import ctypes
from dataclasses import dataclass, field

from ._native import check, default_context

NULL = -(1 << 62)               # SDGPU_SEARCH_NULL
MAX_TAKE = 256                  # SDGPU_SEARCH_MAX_TAKE
SELECT_FINAL_RECORDS = 3840     # SDGPU_SEARCH_SELECT_FINAL
REFERENCE_MAX_TAKE = 100        # search.rs:27 MAX_TAKE

(USE_LOCATION, USE_EXTENSION, USE_CREATED_FROM, USE_CREATED_TO, USE_DIR, USE_FAVORITE,
 USE_HIDDEN_EXCLUDE, USE_KIND, USE_TAGS, USE_ACCESSED_EQ, USE_ACCESSED_NE) = (
    1 << b for b in range(11))
DESC, GROUP_DIRS, FILES_ONLY, CURSOR, CURSOR_STRICT, ORDER_BY_OBJECT, NEEDS_OBJECT = (
    1 << b for b in range(7))

_vp, _u64 = ctypes.c_void_p, ctypes.c_uint64


class _Rows(ctypes.Structure):          # sdgpu_search_rows_t
    _fields_ = [("n", _u64), ("location", _vp), ("ext", _vp), ("dir_key", _vp), ("flags", _vp),
                ("date_created", _vp), ("object", _vp), ("eligible", _vp), ("order_key", _vp)]


class _Objects(ctypes.Structure):       # sdgpu_search_objects_t
    _fields_ = [("m", _u64), ("kind", _vp), ("flags", _vp), ("date_accessed", _vp),
                ("order_key", _vp), ("tag_obj", _vp), ("tag_tag", _vp), ("n_pairs", _u64)]


class _Query(ctypes.Structure):         # sdgpu_search_query_t
    _fields_ = [("use", ctypes.c_uint32), ("flags", ctypes.c_uint32),
                ("location", ctypes.c_int32), ("ext", ctypes.c_uint16),
                ("favorite", ctypes.c_uint16), ("dir_key", ctypes.c_uint64),
                ("created_from", ctypes.c_int64), ("created_to", ctypes.c_int64),
                ("kind_mask", ctypes.c_uint32), ("n_tags", ctypes.c_uint32),
                ("tags", ctypes.c_int32 * 32), ("accessed_eq", ctypes.c_int64),
                ("accessed_ne", ctypes.c_int64), ("cursor_key", ctypes.c_int64),
                ("cursor_row", ctypes.c_int64), ("offset", ctypes.c_int64),
                ("take", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


ROW_COLUMNS = ("location", "ext", "dir_key", "flags", "date_created", "object", "eligible",
               "order_key")
OBJECT_COLUMNS = ("kind", "flags", "date_accessed", "order_key", "tag_obj", "tag_tag")


@dataclass
class Rows:
    """One table's file_path rows in ascending id order: the header's columns
    (torch tensors for search_page, numpy arrays for search_page_host; None = a
    column the query does not use)."""
    n: int
    location: object = None      # int32, -1 = NULL
    ext: object = None           # uint16 (torch: int16 bits), 0xFFFF = NULL
    dir_key: object = None       # uint64 (torch: int64 bits)
    flags: object = None         # uint8, bit 0 is_dir
    date_created: object = None  # int64
    object: object = None        # int32, -1 = no Object
    eligible: object = None      # uint8
    order_key: object = None     # int64


@dataclass
class Objects:
    m: int
    kind: object = None           # int32, -1 = NULL
    flags: object = None          # uint8: 1 favorite, 2 favorite NULL, 4 hidden
    date_accessed: object = None  # int64
    order_key: object = None      # int64
    tag_obj: object = None        # int32 [n_pairs]
    tag_tag: object = None

    @property
    def n_pairs(self) -> int:
        return 0 if self.tag_obj is None else len(self.tag_obj)


@dataclass
class Query:
    use: int = 0
    flags: int = 0
    location: int = 0
    ext: int = 0
    favorite: int = 0
    dir_key: int = 0
    created_from: int = 0
    created_to: int = 0
    kind_mask: int = 0
    tags: tuple = ()
    accessed_eq: int = 0
    accessed_ne: int = 0
    cursor_key: int = 0
    cursor_row: int = 0
    offset: int = 0
    take: int = 0

    def c_struct(self) -> _Query:
        q = _Query(self.use, self.flags, self.location, self.ext, self.favorite, self.dir_key,
                   self.created_from, self.created_to, self.kind_mask, len(self.tags))
        if len(self.tags) <= 32:
            for i, t in enumerate(self.tags):
                q.tags[i] = t
        q.accessed_eq, q.accessed_ne = self.accessed_eq, self.accessed_ne
        q.cursor_key, q.cursor_row = self.cursor_key, self.cursor_row
        q.offset, q.take = self.offset, self.take
        return q


def _structs(rows, objects, addr):
    r = _Rows(rows.n, *(addr(getattr(rows, c)) for c in ROW_COLUMNS))
    o = None
    if objects is not None:
        o = _Objects(objects.m, *(addr(getattr(objects, c)) for c in OBJECT_COLUMNS),
                     objects.n_pairs)
    return r, o


def search_page(rows: Rows, objects: Objects | None, query: Query, ctx=None, page=None,
                counts=None):
    """sdgpu_search_page_device on device tensors: (page int32 [MAX_TAKE],
    counts int32 [4]) on the current stream, no synchronisation.  page[0 ..
    counts[2]) are the row indices of the page; counts = matching rows,
    candidates, page length, directories among the matching rows."""
    import torch
    some = next((t for t in (getattr(rows, c) for c in ROW_COLUMNS) if t is not None), None)
    dev = some.device if some is not None else torch.device("cuda", torch.cuda.current_device())
    ctx = ctx or default_context(dev.index)
    if page is None:
        page = torch.empty(MAX_TAKE, dtype=torch.int32, device=dev)
    if counts is None:
        counts = torch.empty(4, dtype=torch.int32, device=dev)
    r, o = _structs(rows, objects, lambda t: None if t is None or t.numel() == 0 else t.data_ptr())
    q = query.c_struct()
    s = torch.cuda.current_stream(dev).cuda_stream
    check(ctx.lib.sdgpu_search_page_device(
        ctx.h, ctypes.addressof(r), ctypes.addressof(o) if o is not None else None,
        ctypes.addressof(q), page.data_ptr(), counts.data_ptr(), s), "sdgpu_search_page_device")
    return page, counts


def search_page_host(rows: Rows, objects: Objects | None, query: Query, ctx=None):
    """sdgpu_search_page on numpy arrays: (page uint32 trimmed to counts[2],
    counts uint32 [4])."""
    import numpy as np
    ctx = ctx or default_context()
    keep = []

    def addr(a):
        if a is None or len(a) == 0:
            return None
        a = np.ascontiguousarray(a)
        keep.append(a)
        return a.ctypes.data

    r, o = _structs(rows, objects, addr)
    q = query.c_struct()
    page = np.empty(MAX_TAKE, dtype=np.uint32)
    counts = np.empty(4, dtype=np.uint32)
    check(ctx.lib.sdgpu_search_page(
        ctx.h, ctypes.addressof(r), ctypes.addressof(o) if o is not None else None,
        ctypes.addressof(q), page.ctypes.data, counts.ctypes.data), "sdgpu_search_page")
    return page[:int(counts[2])], counts


# ---- the reference's arguments ----------------------------------------------------

# library/cat.rs:46-60 to_object_kind; every other category but Recents and
# Favorites maps to object::id::equals(-1) (:74): nothing.
CATEGORY_KIND = {"Photos": 5, "Videos": 7, "Music": 6, "Books": 22, "Encrypted": 11,
                 "Databases": 21, "Archives": 8, "Applications": 9}
CATEGORY_NONE = ("Albums", "Movies", "Documents", "Downloads", "Projects", "Games", "Contacts",
                 "Trash")
CATEGORIES = ("Recents", "Favorites") + tuple(CATEGORY_KIND) + CATEGORY_NONE


def category_terms(name: str):
    """Category::to_where_param (cat.rs:62-75) as query terms: a dict of Query
    fields to merge, or None for the categories that match no Object."""
    if name == "Recents":
        return {"use": USE_ACCESSED_NE, "accessed_ne": NULL}    # not date_accessed = NULL
    if name == "Favorites":
        return {"use": USE_FAVORITE, "favorite": 1}
    if name in CATEGORY_KIND:
        return {"use": USE_KIND, "kind_mask": 1 << CATEGORY_KIND[name]}
    if name in CATEGORY_NONE:
        return None
    raise ValueError(f"unknown category {name!r}")


def maybe_not_terms(value):
    """MaybeNot<Option<date>> of ObjectFilterArgs.date_accessed (search.rs:94-108,
    :311-312): `v` -> equals v, `{"not": v}` -> not equals v; None is SQL NULL."""
    if isinstance(value, dict) and set(value) == {"not"}:
        v = value["not"]
        return {"use": USE_ACCESSED_NE, "accessed_ne": NULL if v is None else int(v)}
    return {"use": USE_ACCESSED_EQ, "accessed_eq": NULL if value is None else int(value)}


def name_contains(table, terms):
    """The `search` argument (search.rs:165-169: split on ' ', every piece a
    name::contains) as an eligible column, built on the host: an ASCII-case-
    insensitive substring match per term, as SQLite's LIKE; every term, the empty
    one an empty search yields included, needs a non-NULL name."""
    import numpy as np
    if isinstance(terms, str):
        terms = terms.split(" ")
    low = [_ascii_lower(t) for t in terms]
    out = np.zeros(len(table), dtype=np.uint8)
    for i, name in enumerate(table.name):
        if name is None:
            continue
        nm = _ascii_lower(name)
        out[i] = all(t in nm for t in low)
    return out


_LOWER = {c: c + 32 for c in range(65, 91)}


def _ascii_lower(s: str) -> str:
    return s.translate(_LOWER)


def _split_extension(name: str, is_dir: bool):
    i = name.rfind(".")
    return "" if is_dir or i <= 0 else name[i + 1:]


@dataclass
class ObjectAttrs:
    """What the explorer filters and orders Objects by (schema.prisma Object):
    dicts keyed by Object id; a missing id is NULL."""
    kind: dict = field(default_factory=dict)
    favorite: dict = field(default_factory=dict)
    hidden: dict = field(default_factory=dict)
    date_accessed: dict = field(default_factory=dict)
    tags: list = field(default_factory=list)    # (object id, tag id) pairs


class SearchColumns:
    """The call's columns for a FilePaths table: numpy on the host, tensors on
    the device (``rows()`` / ``objects()``), the extension dictionary (``ext_id``)
    and the order columns (``order_column``).  Dates and sizes are optional
    per-row sequences (None = NULL); for directory rows size_in_bytes can take
    the totals of dir_sizes.location_sizes.  dir_key is the indexer's key of the row's
    materialized_path (indexer.dir_keys, computed on the device)."""

    def __init__(self, table, attrs: ObjectAttrs | None = None, date_created=None,
                 date_modified=None, date_indexed=None, size_in_bytes=None, salt: int = 0,
                 ctx=None):
        import numpy as np
        import torch
        from . import indexer
        self.table, self.salt, self.ctx = table, salt, ctx
        n = len(table)
        attrs = attrs or ObjectAttrs(kind=dict(getattr(table, "object_kind", {})))
        self.attrs = attrs
        self.location = np.array([-1 if x is None else x for x in table.location_id], np.int32)
        exts = [_split_extension(nm, d) for nm, d in zip(table.name, table.is_dir)]
        self.ext_names = sorted(set(exts))
        self._ext_id = {e: i for i, e in enumerate(self.ext_names)}
        self.ext = np.array([self._ext_id[e] for e in exts], np.uint16)
        paths = sorted(set(table.materialized_path))
        pk = dict(zip(paths, indexer.dir_keys(paths, salt, ctx).tolist())) if paths else {}
        self.dir_key = np.array([pk[p] for p in table.materialized_path], np.uint64)
        self.flags = np.array([1 if d else 0 for d in table.is_dir], np.uint8)
        self.object_ids = sorted({o for o in table.object_id if o is not None})
        oidx = {o: i for i, o in enumerate(self.object_ids)}
        self.object = np.array([-1 if o is None else oidx[o] for o in table.object_id], np.int32)

        def col(values):
            if values is None:
                return np.full(n, NULL, np.int64)
            return np.array([NULL if v is None else v for v in values], np.int64)

        self.order = {"dateCreated": col(date_created), "dateModified": col(date_modified),
                      "dateIndexed": col(date_indexed), "sizeInBytes": col(size_in_bytes)}
        # a rank of the name under BINARY collation: 2 r + 1, so that a cursor
        # string that is no row's name falls between two ranks
        self.names = sorted({nm.encode() for nm in table.name if nm is not None})
        nr = {nm: 2 * i + 1 for i, nm in enumerate(self.names)}
        self.order["name"] = np.array([NULL if nm is None else nr[nm.encode()]
                                       for nm in table.name], np.int64)
        ids = self.object_ids
        self.o_kind = np.array([attrs.kind.get(o, -1) if attrs.kind.get(o) is not None else -1
                                for o in ids], np.int32)
        fav, hid = attrs.favorite, attrs.hidden
        self.o_flags = np.array([(1 if fav.get(o) else 0) | (2 if fav.get(o) is None else 0)
                                 | (4 if hid.get(o) else 0) for o in ids], np.uint8)
        self.o_date_accessed = np.array([NULL if attrs.date_accessed.get(o) is None
                                         else attrs.date_accessed[o] for o in ids], np.int64)
        pairs = [(oidx[o], t) for o, t in attrs.tags if o in oidx]
        self.tag_obj = np.array([p[0] for p in pairs], np.int32)
        self.tag_tag = np.array([p[1] for p in pairs], np.int32)
        self.o_order = {"kind": np.where(self.o_kind < 0, NULL, self.o_kind).astype(np.int64),
                        "dateAccessed": self.o_date_accessed}
        dev = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
        self._d = {"location": dev(self.location), "ext": dev(self.ext.view(np.int16)),
                   "dir_key": dev(self.dir_key.view(np.int64)), "flags": dev(self.flags),
                   "object": dev(self.object)}
        self._d_order = {k: dev(v) for k, v in self.order.items()}
        self._d_obj = {"kind": dev(self.o_kind), "flags": dev(self.o_flags),
                       "date_accessed": dev(self.o_date_accessed), "tag_obj": dev(self.tag_obj),
                       "tag_tag": dev(self.tag_tag)}
        self._d_o_order = {k: dev(v) for k, v in self.o_order.items()}

    def ext_id(self, name: str):
        """The dictionary id of an extension string, None when no row has it."""
        return self._ext_id.get(name)

    def name_rank(self, name: str) -> int:
        """The cursor's rank of a name: its row rank when a row has it, else the
        even number between its neighbours."""
        b = name.encode()
        i = bisect.bisect_left(self.names, b)
        return 2 * i + 1 if i < len(self.names) and self.names[i] == b else 2 * i

    def rows(self, order_field=None, eligible=None) -> Rows:
        import torch
        d = self._d
        el = None if eligible is None else torch.from_numpy(eligible).cuda()
        return Rows(len(self.table), d["location"], d["ext"], d["dir_key"], d["flags"],
                    self._d_order["dateCreated"], d["object"], el,
                    None if order_field is None else self._d_order[order_field])

    def objects(self, order_field=None) -> Objects:
        d = self._d_obj
        return Objects(len(self.object_ids), d["kind"], d["flags"], d["date_accessed"],
                       None if order_field is None else self._d_o_order[order_field],
                       d["tag_obj"], d["tag_tag"])

    def object_rows(self, order_field=None) -> Rows:
        """The Object columns as rows (object[i] = i) for search.objects."""
        import torch
        m = len(self.object_ids)
        ident = torch.arange(m, dtype=torch.int32, device="cuda")
        return Rows(m, object=ident,
                    order_key=None if order_field is None else self._d_o_order[order_field])


def _merge(q: Query, terms: dict) -> bool:
    """Adds terms to q; False when they contradict what q already asks for."""
    for k, v in terms.items():
        if k == "use":
            continue
        if k == "kind_mask":
            q.kind_mask = (q.kind_mask & v) if q.use & USE_KIND else v
            if q.kind_mask == 0:
                return False
        elif k == "favorite":
            if q.use & USE_FAVORITE and q.favorite != v:
                return False
            q.favorite = v
        elif k == "accessed_ne":
            if q.use & USE_ACCESSED_NE and q.accessed_ne != v:
                # `<> a AND <> b`: only "IS NOT NULL" can be folded into the other
                if NULL not in (q.accessed_ne, v):
                    raise ValueError("two different date_accessed exclusions")
                v = q.accessed_ne if v == NULL else v
            q.accessed_ne = v
        else:
            setattr(q, k, v)
    q.use |= terms.get("use", 0)
    return True


def _object_filter(q: Query, f: dict | None) -> bool:
    """ObjectFilterArgs::into_params (search.rs:302-324) into q; False: the
    filter matches nothing.  `hidden` defaults to Exclude (:265-283)."""
    f = f or {}
    if f.get("hidden", "exclude") == "exclude":
        q.use |= USE_HIDDEN_EXCLUDE
    if f.get("favorite") is not None:
        q.use |= USE_FAVORITE
        q.favorite = 1 if f["favorite"] else 0
    if "dateAccessed" in f:
        _merge(q, maybe_not_terms(f["dateAccessed"]))
    kinds = [k for k in f.get("kind", ()) if 0 <= k < 32]
    if f.get("kind"):
        if not kinds:
            return False
        q.use |= USE_KIND
        q.kind_mask = sum(1 << k for k in set(kinds))
    if f.get("tags"):
        tags = tuple(dict.fromkeys(f["tags"]))
        if len(tags) > 32:
            raise ValueError("at most 32 tags in one query")
        q.use |= USE_TAGS
        q.tags = tags
    if f.get("category") is not None:
        terms = category_terms(f["category"])
        if terms is None or not _merge(q, terms):
            return False
    return True


def _path_filter(cols: SearchColumns, q: Query, f: dict):
    """FilePathFilterArgs::into_params (search.rs:127-187) into q.  Returns
    (matches anything, eligible column or None, the directory string or None).
    Raises LookupError("Directory not found") as the reference does (:148-153)."""
    t = cols.table
    eligible = name_contains(t, f.get("search") or "") if "search" in f else None
    loc = f.get("locationId")
    if loc is not None:
        if loc not in set(t.location_id):
            raise LookupError(f"location {loc} not found")             # IdNotFound, :138
        q.use |= USE_LOCATION
        q.location = loc
    ok = True
    if f.get("extension") is not None:
        e = cols.ext_id(f["extension"])
        ok = e is not None
        q.use |= USE_EXTENSION
        q.ext = e if ok else 0
    created = f.get("createdAt") or {}
    if created.get("from") is not None:
        q.use |= USE_CREATED_FROM
        q.created_from = int(created["from"])
    if created.get("to") is not None:
        q.use |= USE_CREATED_TO
        q.created_to = int(created["to"])
    directory = None
    path = f.get("path")
    if path is not None:
        if path and path != "/" and loc is not None:
            directory = "/" + path.strip("/") + "/"
            parent, _, name = directory[:-1].rpartition("/")
            if not any(d and l == loc and mp == parent + "/" and nm == name
                       for d, l, mp, nm in zip(t.is_dir, t.location_id, t.materialized_path,
                                               t.name)):
                raise LookupError("Directory not found")
        else:
            directory = "/"
        from . import indexer
        q.use |= USE_DIR
        q.dir_key = int(indexer.dir_keys([directory], cols.salt, cols.ctx)[0])
    if "object" in f and f["object"] is not None:
        ok &= _object_filter(q, f["object"])
    return ok, eligible, directory


def _order(order):
    """FilePathOrder / ObjectOrder -> (field, descending, by Object)."""
    if order is None:
        return None, False, False
    if order["field"] == "object":
        inner = order["value"]
        return inner["field"], inner["value"] == "Desc", True
    return order["field"], order["value"] == "Desc", False


def _pagination(cols, q: Query, oap, group_directories: bool, object_rows: bool = False):
    """OrderAndPagination (search.rs:434-530, :611-661) into q; returns the order
    field and whether it is an Object's."""
    if oap is None:
        return None, False
    if "orderOnly" in oap:
        fld, desc, by_obj = _order(oap["orderOnly"])
    elif "offset" in oap:
        fld, desc, by_obj = _order(oap["offset"].get("order"))
        q.offset = int(oap["offset"]["offset"])
    else:
        cur = oap["cursor"]
        cid, c = int(cur["id"]), cur["cursor"]
        variant = c if object_rows else c["variant"]
        if not object_rows and group_directories and not c["isDir"]:
            q.flags |= FILES_ONLY                                       # :453-455
        q.flags |= CURSOR
        fld, desc, by_obj = None, False, False
        if variant != "none":
            (vname, item), = variant.items()
            if vname == "object":
                (vname, item), = item.items()
                by_obj = True
                q.flags |= CURSOR_STRICT                                # no tie arm, :497-515
            fld, desc = vname, item["order"] == "Desc"
            data = item["data"]
            q.cursor_key = cols.name_rank(data) if fld == "name" else int(data)
        # rows with id <= cid ascending, id < cid descending
        if object_rows:     # Object ids are any ascending numbers
            q.cursor_row = (bisect.bisect_left if desc else bisect.bisect_right)(
                cols.object_ids, cid)
        else:               # file_path ids are row index + 1
            q.cursor_row = cid - 1 if desc else cid
    if desc:
        q.flags |= DESC
    if by_obj:
        q.flags |= ORDER_BY_OBJECT
    return fld, by_obj


def _run(cols, rows, objects, q):
    page, counts = search_page(rows, objects, q, ctx=cols.ctx)
    counts = counts.cpu().numpy()
    return page[:int(counts[2])].cpu().numpy().astype("int64"), counts


def paths(cols: SearchColumns, take: int, order_and_pagination=None, filter=None,
          group_directories: bool = True, thumb_keys=None):
    """search.paths: the page's items, each {"row", "id", "has_local_thumbnail",
    "thumbnail_key"}.  `filter` / `order_and_pagination` are the reference's
    camelCase JSON (FilePathFilterArgs, OrderAndPagination); dates are int64
    nanoseconds.  The non-cursor filter is translated first (it may raise
    "Directory not found"), then order and cursor; take.min(100) (:421).  A
    category that matches no Object gives an empty page with no call.  dir_key
    hits are string-checked.  `thumb_keys`: device int64 tensor of the cas keys
    of the thumbnails on disk (thumbnailer.disk_keys) for has_local_thumbnail."""
    q = Query(take=min(int(take), REFERENCE_MAX_TAKE))
    ok, eligible, directory = _path_filter(cols, q, filter or {})
    if group_directories:
        q.flags |= GROUP_DIRS
    fld, by_obj = _pagination(cols, q, order_and_pagination, group_directories)
    if not ok:
        return []
    needs_objects = by_obj or q.use & (USE_FAVORITE | USE_HIDDEN_EXCLUDE | USE_KIND | USE_TAGS
                                       | USE_ACCESSED_EQ | USE_ACCESSED_NE)
    rows = cols.rows(None if by_obj else fld, eligible)
    page, _ = _run(cols, rows, cols.objects(fld if by_obj else None) if needs_objects else None, q)
    t = cols.table
    if directory is not None:
        page = [i for i in page.tolist() if t.materialized_path[i] == directory]
    else:
        page = page.tolist()
    return _items(t, page, thumb_keys, cols.ctx)


def _items(t, page, thumb_keys, ctx):
    import numpy as np
    import torch
    from . import thumbnailer
    present = [False] * len(page)
    if thumb_keys is not None and page:
        has = np.array([t.cas_id[i] is not None for i in page], np.uint8)
        keys = np.array([int.from_bytes(bytes.fromhex(t.cas_id[i]), "little")
                         if t.cas_id[i] is not None else 0 for i in page], np.uint64)
        pr = thumbnailer.thumbnail_exists(thumb_keys, torch.from_numpy(keys.view(np.int64)).cuda(),
                                          torch.from_numpy(has).cuda(), ctx=ctx)
        present = [bool(x) for x in pr.cpu().numpy()]
    return [{"row": i, "id": i + 1, "has_local_thumbnail": p,
             "thumbnail_key": None if t.cas_id[i] is None else [t.cas_id[i]]}
            for i, p in zip(page, present)]


def paths_count(cols: SearchColumns, filter=None) -> int:
    """search.pathsCount (search.rs:563-582): the filter alone.  With a `path`
    the count is over the 64-bit dir_key, with no string check: exact up to a
    key collision, where `paths` checks the strings of the rows it returns."""
    q = Query(take=0)
    ok, eligible, directory = _path_filter(cols, q, filter or {})
    if not ok:
        return 0
    needs_objects = q.use & (USE_FAVORITE | USE_HIDDEN_EXCLUDE | USE_KIND | USE_TAGS
                             | USE_ACCESSED_EQ | USE_ACCESSED_NE)
    _, counts = _run(cols, cols.rows(None, eligible), cols.objects() if needs_objects else None, q)
    return int(counts[0])


def objects(cols: SearchColumns, take: int, order_and_pagination=None, filter=None):
    """search.objects (search.rs:583-708) over the Object columns as rows: the
    page as Object ids.  The reference takes take.max(100) (:604, a u8, so at
    most 255) and pops the row past `take` as the next cursor; here the page is
    `take` rows, at most MAX_TAKE.  Deviation: ties go by id where the reference
    orders by pub_id (:657-658)."""
    q = Query(take=min(int(take), MAX_TAKE))
    if not _object_filter(q, filter):
        return []
    fld, _ = _pagination(cols, q, order_and_pagination, False, object_rows=True)
    page, _ = _run(cols, cols.object_rows(fld), cols.objects(), q)
    return [cols.object_ids[i] for i in page.tolist()]


def objects_count(cols: SearchColumns, filter=None) -> int:
    q = Query(take=0)
    if not _object_filter(q, filter):
        return 0
    _, counts = _run(cols, cols.object_rows(), cols.objects(), q)
    return int(counts[0])
