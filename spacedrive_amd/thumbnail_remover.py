"""The thumbnail remover's half-hourly sweep (core/src/object/
thumbnail_remover.rs:236-367, process_clean_up) with its database question --
`file_path.cas_id IN (a shard directory's stems)`, one full table scan per
directory and library -- answered for the whole cache by one device call
(sdgpu_stale_thumbnails_device): the thumbnails' cas keys against the cas key
columns the job tables already hold.

* ``stale_thumbnails`` -- the device call on tensors.
* ``scan_thumbnails`` -- the walk over the cache (thumbnail_remover.rs:249-299).
* ``process_clean_up`` -- scan, one ``stale_thumbnails`` call, unlink, rmdir.
* ``ThumbnailRemover`` -- the actor's state without its timers and channels.

``remove_by_cas_ids`` (thumbnail_remover.rs:215-234) is not restated: a
host-only unlink loop.
"""
from __future__ import annotations

import ctypes
import os
import re

from ._native import check, default_context

_HEX16 = re.compile(r"[0-9a-f]{16}\Z")


class NonUtf8PathError(OSError):
    """A thumbnail whose stem is not valid UTF-8 (the reference's error of the
    same name; it carries the shard directory's path)."""


def cas_key(stem: str):
    """The cas key of a thumbnail stem, or None when the stem can equal no
    database cas_id (anything but 16 characters of [0-9a-f]; uppercase hex
    included).  Little-endian, the convention of cas8."""
    if not _HEX16.match(stem):
        return None
    return int.from_bytes(bytes.fromhex(stem), "little")


def _pointer_table(ptrs):
    return (ctypes.c_void_p * max(len(ptrs), 1))(*ptrs)


def stale_thumbnails(thumb_keys, dir_start, columns, ctx=None, trim: bool = True):
    """(stale, stale_start): the positions in `thumb_keys` (int64 device tensor,
    listed directory by directory; `dir_start` int32 [n_dirs + 1] ascending
    offsets) of the thumbnails that no row of `columns` owns, in list order, and
    their per-directory offsets (stale_start[-1] = how many).  `columns`: up to
    64 (cas key column, has_key column or None) pairs of device tensors -- the
    libraries' file_paths, and the non-indexed set as one more column.
    trim=False: the full-length list, no synchronisation."""
    import torch
    dev = thumb_keys.device
    ctx = ctx or default_context(dev.index)
    n, n_dirs, n_cols = thumb_keys.numel(), dir_start.numel() - 1, len(columns)
    stale = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    start = torch.empty(n_dirs + 1, dtype=torch.int32, device=dev)
    keys = _pointer_table([k.data_ptr() for k, _ in columns])
    has = _pointer_table([h.data_ptr() if h is not None else None for _, h in columns])
    rows = (ctypes.c_uint64 * max(n_cols, 1))(*[k.numel() for k, _ in columns])
    s = torch.cuda.current_stream(dev).cuda_stream
    check(ctx.lib.sdgpu_stale_thumbnails_device(
        ctx.h, thumb_keys.data_ptr(), n, dir_start.data_ptr(), n_dirs, keys, has, rows, n_cols,
        stale.data_ptr(), start.data_ptr(), s), "sdgpu_stale_thumbnails_device")
    if not trim:
        return stale, start
    return stale[:int(start[-1].item())], start


def stale_thumbnails_host(thumb_keys, dir_start, columns, ctx=None):
    """sdgpu_stale_thumbnails: the same on numpy arrays (uint64 keys, uint32
    offsets, (uint64 keys, uint8 has_key or None) columns)."""
    import numpy as np
    ctx = ctx or default_context()
    thumb_keys = np.ascontiguousarray(thumb_keys, dtype=np.uint64)
    dir_start = np.ascontiguousarray(dir_start, dtype=np.uint32)
    cols = [(np.ascontiguousarray(k, dtype=np.uint64),
             None if h is None else np.ascontiguousarray(h, dtype=np.uint8)) for k, h in columns]
    n, n_dirs = thumb_keys.size, dir_start.size - 1
    stale = np.empty(max(n, 1), dtype=np.uint32)
    start = np.empty(n_dirs + 1, dtype=np.uint32)
    keys = _pointer_table([k.ctypes.data for k, _ in cols])
    has = _pointer_table([h.ctypes.data if h is not None else None for _, h in cols])
    rows = (ctypes.c_uint64 * max(len(cols), 1))(*[k.size for k, _ in cols])
    check(ctx.lib.sdgpu_stale_thumbnails(
        ctx.h, thumb_keys.ctypes.data, n, dir_start.ctypes.data, n_dirs, keys, has, rows,
        len(cols), stale.ctypes.data, start.ctypes.data), "sdgpu_stale_thumbnails")
    return stale[:int(start[-1])], start


def _split_name(name: bytes):
    """(stem, extension) of a file name as Rust's Path sees them: the extension
    is what follows the last dot, and a name that only starts with a dot has
    none (`.webp` -> no extension; `a.b.webp` -> stem `a.b`)."""
    i = name.rfind(b".")
    if i <= 0:
        return name, None
    return name[:i], name[i + 1:]


def _scan(thumbnails_directory):
    """The walk of thumbnail_remover.rs:249-299 in scan order.  Returns
    (directories, error): [(directory path, [stem, ...])] for the directories
    scanned before `error` (None: the whole cache was scanned)."""
    root = os.fspath(thumbnails_directory)
    os.makedirs(root, exist_ok=True)
    dirs = []
    try:
        with os.scandir(os.fsencode(root)) as top:
            for entry in top:
                # DirEntry::metadata does not follow symlinks (version.txt, links: skipped)
                if not entry.is_dir(follow_symlinks=False):
                    continue
                stems = []
                with os.scandir(entry.path) as shard:
                    for thumb in shard:
                        stem, ext = _split_name(thumb.name)
                        if ext != b"webp":
                            continue
                        try:
                            stems.append(stem.decode("utf-8"))
                        except UnicodeDecodeError:
                            raise NonUtf8PathError(os.fsdecode(entry.path)) from None
                dirs.append((os.fsdecode(entry.path), stems))
    except OSError as e:
        return dirs, e
    return dirs, None


def scan_thumbnails(thumbnails_directory):
    """[(shard directory path, [thumbnail stem, ...])] in scan order: the
    directory is created first; top-level entries that are not directories are
    skipped, symlinks not followed; inside a directory only names whose
    extension is exactly `webp` count.  A thumbnail belongs to the directory it
    was found in, not to cas_id[0..2].  Raises NonUtf8PathError for a stem that
    is not UTF-8, OSError as the reference's FileIOError."""
    dirs, err = _scan(thumbnails_directory)
    if err is not None:
        raise err
    return dirs


def _decide(dirs, libraries, non_indexed_cas_ids, ctx):
    """Per directory, the stems to remove (in scan order)."""
    keyed = []   # (directory, position in its list, key) of the stems a database could hold
    out = []
    for d, (_, stems) in enumerate(dirs):
        # a stem that is no cas key can equal no database cas_id: the host decides it
        stale = [s not in non_indexed_cas_ids for s in stems]
        for j, s in enumerate(stems):
            k = cas_key(s)
            if k is not None and libraries:
                keyed.append((d, j, k))
        out.append(stale)
    if keyed:
        import numpy as np
        import torch
        dev = libraries[0][0].device
        keys = np.array([k for _, _, k in keyed], dtype=np.uint64)
        counts = np.bincount([d for d, _, _ in keyed], minlength=len(dirs))
        start = np.concatenate(([0], np.cumsum(counts))).astype(np.int32)
        extra = [k for k in map(cas_key, non_indexed_cas_ids) if k is not None]
        columns = list(libraries)
        if extra:
            columns.append((torch.from_numpy(np.array(extra, dtype=np.uint64).view(np.int64))
                            .to(dev), None))
        stale, _ = stale_thumbnails(torch.from_numpy(keys.view(np.int64)).to(dev),
                                    torch.from_numpy(start).to(dev), columns, ctx)
        owned = np.ones(len(keyed), dtype=bool)
        owned[stale.cpu().numpy()] = False
        for (d, j, _), o in zip(keyed, owned):
            if o:
                out[d][j] = False
    return [[s for s, gone in zip(stems, flags) if gone]
            for (_, stems), flags in zip(dirs, out)]


def process_clean_up(thumbnails_directory, libraries, non_indexed_cas_ids, ctx=None,
                     dry_run: bool = False):
    """One sweep of the thumbnail cache.  `libraries`: a list of (cas key
    column, has_key column or None) device tensors, one per loaded library;
    `non_indexed_cas_ids`: a set of hex strings.  A thumbnail goes when no
    library row owns its cas_id and the non-indexed set does not hold its
    stem; a directory goes when it holds no thumbnail (:301-311) or when every
    thumbnail found in it went (:353-362).  Returns {"removed_files": [...],
    "removed_dirs": [...]} (paths, in sweep order); dry_run=True touches
    nothing.  OSErrors propagate; an error while scanning directory k is
    raised after the directories scanned before it were swept, as the
    reference, which works directory by directory, leaves them."""
    dirs, err = _scan(thumbnails_directory)
    remove = _decide(dirs, list(libraries), set(non_indexed_cas_ids), ctx)
    report = {"removed_files": [], "removed_dirs": []}
    for (path, stems), gone in zip(dirs, remove):
        for s in gone:
            f = os.path.join(path, s + ".webp")
            if not dry_run:
                os.unlink(f)
            report["removed_files"].append(f)
        if len(gone) == len(stems):  # nothing found, or everything found removed
            if not dry_run:
                os.rmdir(path)
            report["removed_dirs"].append(path)
    if err is not None:
        raise err
    return report


class ThumbnailRemover:
    """The actor's state (thumbnail_remover.rs:131-213) without its timers and
    channels: the loaded libraries' columns, the non-indexed cas_ids, and
    run() for the half-hourly tick."""

    def __init__(self, thumbnails_directory, ctx=None):
        self.thumbnails_directory = thumbnails_directory
        self.ctx = ctx
        self.libraries = {}
        self.non_indexed_cas_ids = set()

    def add_library(self, id, columns):
        """columns: (cas key column, has_key column or None) of the library's file_paths."""
        self.libraries[id] = columns

    def remove_library(self, id):
        self.libraries.pop(id, None)

    def new_non_indexed_thumbnail(self, cas_id: str):
        self.non_indexed_cas_ids.add(cas_id)

    def run(self, dry_run: bool = False):
        """One tick: sweeps only while at least one library is loaded (:176);
        returns process_clean_up's report, or None."""
        if not self.libraries:
            return None
        return process_clean_up(self.thumbnails_directory, list(self.libraries.values()),
                                self.non_indexed_cas_ids, self.ctx, dry_run)
