"""Recursive directory sizes of one location as one device call
(sdgpu_dir_sizes_device): what every directory of the location holds, summed
bottom-up over the directory tree with integer adds, so the answer is exact
whatever order the adds come in.

The reference stores the directory inode's size for a directory row
(FilePathMetadata.size_in_bytes into file_path.size_in_bytes_bytes,
core/src/location/indexer/mod.rs:126-136, 215-225) and orders and shows by that
column (api/search.rs:85, api/locations.rs:66-100); this is an opt-in
replacement for that value.

* ``self_keys`` -- the key of a directory row's materialized_path_for_children().
* ``sizes`` -- the device call on tensors; ``sizes_host`` -- on numpy arrays.
* ``sizes_oracle`` -- the same answer in plain numpy / Python.
* ``location_sizes`` -- the columns of a ``LocationIndex``, one device call, and
  the answer made exact on strings.

The caller supplies the keys and the file sizes, and writes size_in_bytes_bytes
for directory rows if it wants the totals stored.
"""
from __future__ import annotations

from . import indexer
from ._native import check, default_context

IS_DIR = indexer.IS_DIR
MISS = indexer.MISS                       # SDGPU_IDX_MISS
UNRESOLVED = 0xFFFFFFFFFFFFFFFF           # SDGPU_SIZE_UNRESOLVED
FILES_UNRESOLVED = 0xFFFFFFFF
MAX_ROWS = 1 << 31


def self_keys(materialized_paths, names, salt: int = 0, ctx=None):
    """uint64 keys of the directories (materialized_path, name): a directory's
    materialized_path_for_children() is mp + name + "/"
    (isolated_file_path_data.rs:150-158), and its self key is
    indexer.dir_keys of that string -- the key its children carry as the key of
    their own materialized_path (indexer.dir_message)."""
    return indexer.dir_keys([m + n + "/" for m, n in zip(materialized_paths, names)], salt, ctx)


def _ptr(t):
    return t.data_ptr() if t is not None and t.numel() else None


def sizes(r_dirkey, r_selfkey, r_flags, r_size, ctx=None, want_files: bool = True):
    """(parent, total, files, counts) of one location's rows in ascending id
    order, all on the device and without synchronisation.  `r_dirkey`,
    `r_selfkey`, `r_size` int64 [n_r] (the bits of the uint64 values),
    `r_flags` uint8 [n_r] or None (no directory rows; `r_selfkey` may then be
    None).  `parent` int32 [n_r] (bits of uint32, MISS = -1), `total` int64
    [n_r] (bits of uint64, UNRESOLVED = -1), `files` int32 [n_r] (None with
    want_files=False), `counts` int64 [4] = directory rows, resolved directory
    rows, parentless rows, the location's size."""
    import torch
    dev = r_dirkey.device
    ctx = ctx or default_context(dev.index)
    n = r_dirkey.numel()
    parent = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    total = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
    files = torch.empty(max(n, 1), dtype=torch.int32, device=dev) if want_files else None
    counts = torch.empty(4, dtype=torch.int64, device=dev)
    s = torch.cuda.current_stream(dev).cuda_stream
    check(ctx.lib.sdgpu_dir_sizes_device(
        ctx.h, _ptr(r_dirkey), _ptr(r_selfkey), _ptr(r_flags), _ptr(r_size), n,
        parent.data_ptr(), total.data_ptr(), None if files is None else files.data_ptr(),
        counts.data_ptr(), s), "sdgpu_dir_sizes_device")
    return parent[:n], total[:n], None if files is None else files[:n], counts


def sizes_host(r_dirkey, r_selfkey, r_flags, r_size, ctx=None):
    """sdgpu_dir_sizes: the same on numpy arrays (uint64 keys and sizes, uint8
    flags or None); returns uint32 parent, uint64 total, uint32 files, uint64
    counts."""
    import numpy as np
    ctx = ctx or default_context()
    u64 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.uint64)  # noqa: E731
    r_dirkey, r_selfkey, r_size = u64(r_dirkey), u64(r_selfkey), u64(r_size)
    r_flags = None if r_flags is None else np.ascontiguousarray(r_flags, dtype=np.uint8)
    n = r_dirkey.size
    if r_size.size != n or (r_flags is not None and (r_flags.size != n or r_selfkey is None
                                                     or r_selfkey.size != n)):
        raise ValueError("every column is [n_r]")
    parent = np.empty(max(n, 1), dtype=np.uint32)
    total = np.empty(max(n, 1), dtype=np.uint64)
    files = np.empty(max(n, 1), dtype=np.uint32)
    counts = np.empty(4, dtype=np.uint64)
    data = lambda a: None if a is None or a.size == 0 else a.ctypes.data  # noqa: E731
    check(ctx.lib.sdgpu_dir_sizes(
        ctx.h, data(r_dirkey), data(r_selfkey), data(r_flags), data(r_size), n,
        parent.ctypes.data, total.ctypes.data, files.ctypes.data, counts.ctypes.data),
        "sdgpu_dir_sizes")
    return parent[:n], total[:n], files[:n], counts


def sizes_oracle(r_dirkey, r_selfkey, r_flags, r_size):
    """The definition of include/sdgpu.h in plain numpy / Python: parent = the
    lowest directory row per self key; the members of cycles of `parent` found
    by marking every walk up from a directory row; then every resolved
    directory handed to its parent, the deepest first.  Returns uint32 parent,
    uint64 total, uint32 files, uint64 counts."""
    import numpy as np
    n = len(r_dirkey)
    dirkey = np.asarray(r_dirkey, dtype=np.uint64).tolist()
    is_dir = ([False] * n if r_flags is None
              else [bool(f & IS_DIR) for f in np.asarray(r_flags, dtype=np.uint8).tolist()])
    selfkey = [0] * n if r_flags is None else np.asarray(r_selfkey, dtype=np.uint64).tolist()
    size = np.asarray(r_size, dtype=np.uint64).tolist()
    owner: dict = {}
    for j in range(n):
        if is_dir[j]:
            owner.setdefault(selfkey[j], j)          # ascending j: the lowest row stays
    parent = [owner.get(dirkey[i], MISS) for i in range(n)]
    # marking: 0 unseen, 1 on the walk that is running, 2 done
    mark = [0] * n
    on_cycle = [False] * n
    for j in range(n):
        if not is_dir[j] or mark[j]:
            continue
        walk = []
        d = j
        while d != MISS and mark[d] == 0:
            mark[d] = 1
            walk.append(d)
            d = parent[d]
        if d != MISS and mark[d] == 1:               # the walk met itself: from d on, a cycle
            for x in walk[walk.index(d):]:
                on_cycle[x] = True
        for x in walk:
            mark[x] = 2
    # depth of every resolved directory: steps to a parentless row or to a cycle
    depth = [0] * n
    for j in range(n):
        if not is_dir[j] or on_cycle[j] or depth[j]:
            continue
        walk = []
        d = j
        while d != MISS and not on_cycle[d] and depth[d] == 0:
            walk.append(d)
            d = parent[d]
        base = 0 if d == MISS or on_cycle[d] else depth[d]
        for k, x in enumerate(reversed(walk)):
            depth[x] = base + k + 1
    total = [0 if is_dir[i] else size[i] for i in range(n)]
    files = [0] * n
    for i in range(n):
        if not is_dir[i] and parent[i] != MISS:
            total[parent[i]] = (total[parent[i]] + size[i]) & UNRESOLVED
            files[parent[i]] += 1
    for j in sorted((j for j in range(n) if is_dir[j] and not on_cycle[j]),
                    key=lambda j: -depth[j]):
        p = parent[j]
        if p != MISS:
            total[p] = (total[p] + total[j]) & UNRESOLVED
            files[p] += files[j]
    for j in range(n):
        if on_cycle[j]:
            total[j], files[j] = UNRESOLVED, FILES_UNRESOLVED
    dirs = sum(is_dir)
    top = [i for i in range(n) if parent[i] == MISS]
    counts = [dirs, dirs - sum(on_cycle), len(top), sum(total[i] for i in top) & UNRESOLVED]
    return (np.array(parent, dtype=np.uint32), np.array(total, dtype=np.uint64),
            np.array([f & FILES_UNRESOLVED for f in files], dtype=np.uint32),
            np.array(counts, dtype=np.uint64))


def location_sizes(index, size_of, salt: int = 0, ctx=None):
    """({row id: total}, the location's size) for the rows of a
    ``indexer.LocationIndex``; ``size_of(row_id)`` supplies the size_in_bytes of
    a file row.  One device call, then the answer made exact on strings: every
    pair (i, parent[i]) must satisfy materialized_path[i] ==
    materialized_path_for_children() of the directory row parent[i], and every
    directory must be resolved.  On a violation the rows are re-keyed with
    salt + 1 (a byte: 255 is followed by 0) and the call is repeated, three
    times at the most; then indexer.KeyCollision is raised."""
    import numpy as np
    import torch
    n = len(index)
    mp, name, is_dir = index.materialized_path, index.name, index.is_dir
    children = [m + nm + "/" if d else None for m, nm, d in zip(mp, name, is_dir)]
    flags = np.fromiter((IS_DIR if d else 0 for d in is_dir), dtype=np.uint8, count=n)
    size = np.fromiter((0 if d else size_of(fid) for fid, d in zip(index.id, is_dir)),
                       dtype=np.uint64, count=n)
    strings = sorted(set(mp) | {c for c in children if c is not None})
    ctx = ctx or default_context()
    where = torch.device("cuda", ctx.device)     # the context's device, not the current one
    dev = lambda a: torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(where)  # noqa: E731
    for salt in ((salt + attempt) % 256 for attempt in range(3)):
        keys = indexer.dir_keys(strings, salt, ctx)
        if np.unique(keys).size != len(strings):
            continue
        key_of = dict(zip(strings, keys.tolist()))
        dirkey = np.array([key_of[m] for m in mp], dtype=np.uint64)
        selfkey = np.array([0 if c is None else key_of[c] for c in children], dtype=np.uint64)
        parent, total, _, counts = sizes(dev(dirkey), dev(selfkey), dev(flags), dev(size),
                                         ctx=ctx, want_files=False)
        parent = parent.cpu().numpy().view(np.uint32).tolist()
        counts = counts.cpu().numpy().view(np.uint64).tolist()
        if counts[1] == counts[0] and all(j == MISS or children[j] == mp[i]
                                          for i, j in enumerate(parent)):
            total = total.cpu().numpy().view(np.uint64).tolist()
            return dict(zip(index.id, total)), counts[3]
    raise indexer.KeyCollision("64-bit directory keys collided under three salts")
