"""The indexer's decision on a rescan (core/src/location/indexer/walk.rs:
309-381 filter_existing_paths, :624-636 and indexer/mod.rs:305-388 the two
queries): which walked entries are new, which changed behind the library's
back, which file_path rows are gone from disk -- answered for one location by
one device call (sdgpu_indexer_diff_device) on 64-bit keys.

* ``path_keys`` / ``dir_keys`` -- BLAKE3-64 keys of (materialized_path, name,
  extension) and of a directory's materialized_path_for_children(), through K1.
* ``diff`` -- the device call on tensors; ``diff_host`` -- on numpy arrays.
* ``LocationIndex`` -- an in-memory stand-in for the indexer's columns.
* ``scan`` -- the walk (os.scandir) with ``accept`` standing for the rules.
* ``rescan`` -- walk, one device call, then the answer made exact on strings.
* ``apply`` -- remove, create, update; returns the ids whose cas_id / Object
  link the caller must clear (indexer/mod.rs:207-215).

Walking, the rules and the writes stay with the caller; only the
decision is a device call.

Deviations: 64-bit keys are made exact by ``rescan``'s check of
every matched pair's strings (re-keyed with another salt on a collision); a
file replaced by a directory of the same name is listed for creation and its
old row is not removed, as in the reference -- exposed as state 3.
"""
from __future__ import annotations

import os
from dataclasses import dataclass, field

from ._native import check, default_context

IS_DIR = 1
ANCESTOR = 2       # SDGPU_IDX_ANCESTOR (walked side)
NO_METADATA = 2    # SDGPU_IDX_NO_METADATA (row side)
MISS = 0xFFFFFFFF  # SDGPU_IDX_MISS
CREATE, UNCHANGED, UPDATE, KIND_CHANGED = 0, 1, 2, 3

# accept()'s third answer: a directory that is not indexed from its parent's
# listing but still walked (it failed an accept-by-glob rule, walk.rs:544-554
# after :535-541); it enters the walked entries as an ancestor of the first
# accepted entry below it (walk.rs:575-617).
WALK_ONLY = "walk"


def _keys(messages, ctx=None):
    """BLAKE3-64 of every message through K1 (cas.cas_batch): 16-B aligned
    offsets in one arena, the first 8 digest bytes little-endian."""
    import numpy as np
    from . import cas
    n = len(messages)
    if n == 0:
        return np.zeros(0, dtype=np.uint64)
    length = np.fromiter((len(m) for m in messages), dtype=np.uint32, count=n)
    room = (length.astype(np.uint64) + 15) // 16 * 16
    off = np.zeros(n, dtype=np.uint64)
    np.cumsum(room[:-1], out=off[1:])
    arena = np.zeros(int(off[-1] + room[-1]) + 16, dtype=np.uint8)
    for m, o in zip(messages, off.tolist()):
        arena[o:o + len(m)] = np.frombuffer(m, dtype=np.uint8)
    out, status = cas.cas_batch(arena, off, length, ctx=ctx)
    if status.any():
        raise ValueError("a path message was refused: status %d" % status[status != 0][0])
    return cas.keys_of(out).copy()


def path_message(materialized_path: str, name: str, extension: str, salt: int = 0) -> bytes:
    return (b"P" + bytes([salt]) + materialized_path.encode() + b"\0" + name.encode() + b"\0"
            + extension.encode())


def dir_message(children_path: str, salt: int = 0) -> bytes:
    # a directory row (mp, name) has the children path mp + name + "/": its
    # self key (dir_sizes.self_keys) is the key of that string
    return b"D" + bytes([salt]) + children_path.encode()


def path_keys(materialized_paths, names, extensions, salt: int = 0, ctx=None):
    """uint64 keys of the unique tuples (materialized_path, name, extension):
    BLAKE3-64 of b"P" + salt + mp + NUL + name + NUL + ext (UTF-8)."""
    return _keys([path_message(m, n, e, salt)
                  for m, n, e in zip(materialized_paths, names, extensions)], ctx)


def dir_keys(children_paths, salt: int = 0, ctx=None):
    """uint64 keys of materialized_path_for_children() strings (or a row's own
    materialized_path): BLAKE3-64 of b"D" + salt + path."""
    return _keys([dir_message(p, salt) for p in children_paths], ctx)


def _ptr(t):
    return t.data_ptr() if t is not None and t.numel() else None


def diff(w_key, w_flags, w_meta, wd_key, r_key, r_dirkey, r_flags, r_meta, ctx=None,
         trim: bool = True):
    """(create, update, remove, match, state, counts) for one location, all on
    the device.  Walked entries: `w_key` int64 [n_w], `w_flags` uint8 [n_w] or
    None, `w_meta` int64 [n_w, 3] (inode, device, modified_at ns).  `wd_key`
    int64 [n_wd]: the walked directories.  Rows in ascending id order: `r_key`,
    `r_dirkey` int64 [n_r], `r_flags` uint8 or None, `r_meta` int64 [n_r, 3].
    `create` / `update` (int32) list walked indices, `remove` row indices, all
    ascending; `match` (int32 bits, MISS = -1) and `state` (uint8) are per
    walked entry; `counts` (int32 [4]) = the three lengths and the state-3
    entries.  trim=False: full-length lists, no synchronisation."""
    import torch
    dev = r_key.device if r_key.numel() else w_key.device
    ctx = ctx or default_context(dev.index)
    n_w, n_wd, n_r = w_key.numel(), wd_key.numel(), r_key.numel()
    i32 = lambda n: torch.empty(max(n, 1), dtype=torch.int32, device=dev)  # noqa: E731
    create, update, remove, match = i32(n_w), i32(n_w), i32(n_r), i32(n_w)
    state = torch.empty(max(n_w, 1), dtype=torch.uint8, device=dev)
    counts = torch.empty(4, dtype=torch.int32, device=dev)
    s = torch.cuda.current_stream(dev).cuda_stream
    check(ctx.lib.sdgpu_indexer_diff_device(
        ctx.h, _ptr(w_key), _ptr(w_flags), _ptr(w_meta), n_w, _ptr(wd_key), n_wd, _ptr(r_key),
        _ptr(r_dirkey), _ptr(r_flags), _ptr(r_meta), n_r, match.data_ptr(), state.data_ptr(),
        create.data_ptr(), update.data_ptr(), remove.data_ptr(), counts.data_ptr(), s),
        "sdgpu_indexer_diff_device")
    match, state = match[:n_w], state[:n_w]
    if trim:
        c = counts.tolist()
        create, update, remove = create[:c[0]], update[:c[1]], remove[:c[2]]
    return create, update, remove, match, state, counts


def diff_host(w_key, w_flags, w_meta, wd_key, r_key, r_dirkey, r_flags, r_meta, ctx=None):
    """sdgpu_indexer_diff: the same on numpy arrays (uint64 keys and metadata,
    uint8 flags or None); returns uint32 / uint8 arrays, the lists trimmed."""
    import numpy as np
    ctx = ctx or default_context()
    u64 = lambda a: np.ascontiguousarray(a, dtype=np.uint64)  # noqa: E731
    u8 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.uint8)  # noqa: E731
    w_key, w_meta, wd_key = u64(w_key), u64(w_meta), u64(wd_key)
    r_key, r_dirkey, r_meta = u64(r_key), u64(r_dirkey), u64(r_meta)
    w_flags, r_flags = u8(w_flags), u8(r_flags)
    n_w, n_wd, n_r = w_key.size, wd_key.size, r_key.size
    if w_meta.size != 3 * n_w or r_meta.size != 3 * n_r or r_dirkey.size != n_r:
        raise ValueError("metadata is [n, 3], r_dirkey [n_r]")
    u32 = lambda n: np.empty(max(n, 1), dtype=np.uint32)  # noqa: E731
    create, update, remove, match = u32(n_w), u32(n_w), u32(n_r), u32(n_w)
    state = np.empty(max(n_w, 1), dtype=np.uint8)
    counts = np.zeros(4, dtype=np.uint32)
    data = lambda a: None if a is None or a.size == 0 else a.ctypes.data  # noqa: E731
    check(ctx.lib.sdgpu_indexer_diff(
        ctx.h, data(w_key), data(w_flags), data(w_meta), n_w, data(wd_key), n_wd, data(r_key),
        data(r_dirkey), data(r_flags), data(r_meta), n_r, match.ctypes.data, state.ctypes.data,
        create.ctypes.data, update.ctypes.data, remove.ctypes.data, counts.ctypes.data),
        "sdgpu_indexer_diff")
    c = counts.tolist()
    return create[:c[0]], update[:c[1]], remove[:c[2]], match[:n_w], state[:n_w], counts


class LocationIndex:
    """The indexer's columns of one location's file_path rows, in ascending id
    order: materialized_path, name, extension, is_dir, inode, device,
    date_modified (ns since the epoch; any of the three may be None) and the
    row id.  (file_identifier.FilePaths has neither metadata nor row removal.)"""

    def __init__(self):
        self.id: list[int] = []
        self.materialized_path: list[str] = []
        self.name: list[str] = []
        self.extension: list[str] = []
        self.is_dir: list[bool] = []
        self.inode: list[int | None] = []
        self.device: list[int | None] = []
        self.date_modified: list[int | None] = []
        self._next = 1
        self._tuples: set = set()           # the unique tuples that are there
        self._at: dict = {}                 # id -> position

    def __len__(self):
        return len(self.id)

    def tuples(self):
        return list(zip(self.materialized_path, self.name, self.extension))

    def rows(self):
        """[(id, mp, name, ext, is_dir, inode, device, date_modified)]"""
        return list(zip(self.id, self.materialized_path, self.name, self.extension, self.is_dir,
                        self.inode, self.device, self.date_modified))

    def add(self, materialized_path, name, extension, is_dir, inode=None, device=None,
            date_modified=None, skip_duplicates: bool = False):
        """A new row; its id.  skip_duplicates (create_many().skip_duplicates(),
        indexer/mod.rs:182): None when the unique tuple is already there."""
        if skip_duplicates and (materialized_path, name, extension) in self._tuples:
            return None
        fid = self._next
        self._next += 1
        self._tuples.add((materialized_path, name, extension))
        self._at[fid] = len(self.id)
        for col, v in ((self.id, fid), (self.materialized_path, materialized_path),
                       (self.name, name), (self.extension, extension),
                       (self.is_dir, bool(is_dir)), (self.inode, inode), (self.device, device),
                       (self.date_modified, date_modified)):
            col.append(v)
        return fid

    def remove(self, ids):
        gone = set(ids)
        keep = [i for i, fid in enumerate(self.id) if fid not in gone]
        for name in ("id", "materialized_path", "name", "extension", "is_dir", "inode", "device",
                     "date_modified"):
            col = getattr(self, name)
            setattr(self, name, [col[i] for i in keep])
        self._tuples = set(self.tuples())
        self._at = {fid: i for i, fid in enumerate(self.id)}

    def set_metadata(self, fid, inode, device, date_modified):
        i = self._at[fid]
        self.inode[i], self.device[i], self.date_modified[i] = inode, device, date_modified


@dataclass
class Entry:
    """One walked entry (walk.rs WalkingEntry)."""
    materialized_path: str
    name: str
    extension: str
    is_dir: bool
    inode: int
    device: int
    modified_at: int          # ns since the epoch
    ancestor: bool = False    # entered as an ancestor, in no listing of its parent


@dataclass
class Walk:
    entries: list = field(default_factory=list)   # [Entry], ancestors included
    dirs: list = field(default_factory=list)      # children paths of the listed directories


def split_name(full_name: str, is_dir: bool):
    """separate_name_and_extension_from_str (isolated_file_path_data.rs:
    160-180): split at the last dot unless it is the first character;
    directories keep their whole name and have an empty extension."""
    if is_dir:
        return full_name, ""
    i = full_name.rfind(".")
    return (full_name, "") if i <= 0 else (full_name[:i], full_name[i + 1:])


def scan(location_path, accept=None) -> Walk:
    """The walk of one location: every directory that is walked has its listing
    read (os.scandir, sorted by name; symlinks are ignored, walk.rs:496-499).
    ``accept(rel_path, is_dir)`` stands for the indexer rules: true = indexed
    (and walked, if a directory), false = rejected with all below it,
    WALK_ONLY = a directory that is walked but not indexed from its parent's
    listing.  An accepted entry pushes its not yet indexed ancestors below the
    root as ANCESTOR entries (walk.rs:575-617).  The root itself is no entry."""
    root = os.fspath(location_path)
    walk = Walk()
    seen = {}                                    # (mp, name, ext, is_dir) -> Entry
    todo = [""]                                  # rel paths of directories, breadth first

    def entry_of(rel, mp, full_name, is_dir, st, ancestor):
        name, ext = split_name(full_name, is_dir)
        return Entry(mp, name, ext, is_dir, st.st_ino, st.st_dev, st.st_mtime_ns, ancestor)

    def push(e):
        k = (e.materialized_path, e.name, e.extension, e.is_dir)
        if k in seen:
            return False
        seen[k] = e
        walk.entries.append(e)
        return True

    while todo:
        rel_dir = todo.pop(0)
        mp = "/" + rel_dir + ("/" if rel_dir else "")
        walk.dirs.append(mp)
        with os.scandir(os.path.join(root, rel_dir)) as it:
            listing = sorted(it, key=lambda d: d.name)
        for d in listing:
            if d.is_symlink():
                continue
            is_dir = d.is_dir(follow_symlinks=False)
            rel = rel_dir + "/" + d.name if rel_dir else d.name
            verdict = True if accept is None else accept(rel, is_dir)
            if not verdict:
                continue
            if is_dir:
                todo.append(rel)
            if verdict == WALK_ONLY:
                continue
            push(entry_of(rel, mp, d.name, is_dir, d.stat(follow_symlinks=False), False))
            parts = rel.split("/")[:-1]
            while parts:                         # nearest ancestor first
                a_mp = "/" + "/".join(parts[:-1]) + ("/" if len(parts) > 1 else "")
                st = os.stat(os.path.join(root, *parts))
                if not push(entry_of("/".join(parts), a_mp, parts[-1], True, st, True)):
                    break                        # its ancestors are there as well
                parts.pop()
    return walk


@dataclass
class Rescan:
    walk: Walk
    create: list           # walked indices (state 0 or 3), ascending
    update: list           # walked indices
    remove: list           # row ids
    match: list            # per walked entry: row id or None
    state: list            # per walked entry
    kind_changed: int
    salt: int


class KeyCollision(RuntimeError):
    pass


def _columns(walk: Walk, index: LocationIndex, salt: int, ctx):
    import numpy as np
    e = walk.entries
    w_key = path_keys([x.materialized_path for x in e], [x.name for x in e],
                      [x.extension for x in e], salt, ctx)
    w_flags = np.fromiter(((IS_DIR if x.is_dir else 0) | (ANCESTOR if x.ancestor else 0)
                           for x in e), dtype=np.uint8, count=len(e))
    w_meta = np.array([[x.inode, x.device, x.modified_at] for x in e],
                      dtype=np.int64).reshape(-1, 3)
    wd_key = dir_keys(walk.dirs, salt, ctx)
    r_key = path_keys(index.materialized_path, index.name, index.extension, salt, ctx)
    r_dirkey = dir_keys(index.materialized_path, salt, ctx)
    none = [a is None or b is None or c is None
            for a, b, c in zip(index.inode, index.device, index.date_modified)]
    r_flags = np.fromiter(((IS_DIR if d else 0) | (NO_METADATA if m else 0)
                           for d, m in zip(index.is_dir, none)), dtype=np.uint8, count=len(index))
    r_meta = np.array([[a or 0, b or 0, c or 0] for a, b, c in
                       zip(index.inode, index.device, index.date_modified)],
                      dtype=np.int64).reshape(-1, 3)
    return w_key, w_flags, w_meta, wd_key, r_key, r_dirkey, r_flags, r_meta


def rescan(index: LocationIndex, location_path, accept=None, ctx=None, walk: Walk | None = None,
           salt: int = 0) -> Rescan:
    """Walk the location, decide with one device call, and make the decision
    exact on strings: the keys must be unique on each side (paths and
    directories), and every pair (i, match[i]) must have equal tuples.  A false
    non-match cannot happen (equal strings give equal keys), and with unique
    keys the pair check covers every spared row.  On a violation both sides are
    re-keyed with salt + 1 (a byte: 255 is followed by 0) and the call is
    repeated, three times at the most; then KeyCollision is raised."""
    import numpy as np
    import torch
    walk = walk if walk is not None else scan(location_path, accept)
    w_tuples = [(x.materialized_path, x.name, x.extension) for x in walk.entries]
    r_tuples = index.tuples()
    dir_strings = sorted(set(walk.dirs) | set(index.materialized_path))
    for salt in ((salt + attempt) % 256 for attempt in range(3)):
        cols = _columns(walk, index, salt, ctx)
        w_key, _, _, _, r_key, _, _, _ = cols
        exact = (np.unique(w_key).size == len(set(w_tuples))
                 and np.unique(r_key).size == len(set(r_tuples))
                 and np.unique(dir_keys(dir_strings, salt, ctx)).size
                 == len(dir_strings))
        if exact:
            dev = [None if c is None else torch.from_numpy(c.view(np.int64) if c.dtype == np.uint64
                                                            else c).cuda() for c in cols]
            create, update, remove, match, state, counts = (t.cpu().numpy()
                                                            for t in diff(*dev, ctx=ctx))
            match = match.view(np.uint32)
            exact = all(j == MISS or w_tuples[i] == r_tuples[j]
                        for i, j in enumerate(match.tolist()))
        if exact:
            return Rescan(walk, create.tolist(), update.tolist(),
                          [index.id[j] for j in remove.tolist()],
                          [None if j == MISS else index.id[j] for j in match.tolist()],
                          state.tolist(), int(counts[3]), salt)
    raise KeyCollision("64-bit path keys collided under three salts")


def apply(index: LocationIndex, result: Rescan):
    """The indexer's writes in its order: the rows of `remove` go, the entries
    of `create` become rows (skipping a tuple that is still there: a
    KIND_CHANGED entry, create_many().skip_duplicates()), the rows of `update`
    take the disk's metadata.  Returns the ids of the updated rows: their
    cas_id and Object link must be cleared (indexer/mod.rs:207-215)."""
    index.remove(result.remove)
    e = result.walk.entries
    for i in result.create:
        x = e[i]
        index.add(x.materialized_path, x.name, x.extension, x.is_dir, x.inode, x.device,
                  x.modified_at, skip_duplicates=True)
    cleared = []
    for i in result.update:
        x = e[i]
        index.set_metadata(result.match[i], x.inode, x.device, x.modified_at)
        cleared.append(result.match[i])
    return cleared
