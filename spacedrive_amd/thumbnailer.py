"""The thumbnailer's side of the media processor (core/src/object/media/
thumbnail/mod.rs:204-359, process) with its one `stat` per row -- does
`<base>/<cas_id[0..2]>/<cas_id>.webp` exist -- answered for a whole column of
file_paths by one device call (sdgpu_thumbnail_worklist_device): the rows' cas
keys against the cas keys of the thumbnails on disk.

* ``work_list`` -- the device call on tensors: the rows to generate, ordered by
  shard directory, one per distinct cas_id.
* ``thumbnail_exists`` -- its presence-only mode, the explorer's
  `has_local_thumbnail` (api/search.rs:540-547, library/library.rs:122-130).
* ``work_list_host`` -- sdgpu_thumbnail_worklist on numpy arrays.
* ``eligible_rows`` -- the query of media_processor/mod.rs:74-116.
* ``disk_keys`` -- the cas keys of the thumbnails the reference's stat finds.
* ``process`` -- query, scan, one device call, then the generate loop.

Deviation: the reference generates two rows of one step of 10
that share a cas_id twice, the same file written twice, and counts both as
created; here every distinct cas_id is generated once.  The files on disk
afterwards are the same set; created / skipped differ by the in-step copies.

No image code is included: decoding, resizing and WebP encoding stay with the
caller's ``generate``.
"""
from __future__ import annotations

import os

from ._native import check, default_context
from .thumbnail_remover import cas_key, scan_thumbnails

REGENERATE = 1  # SDGPU_THUMBS_REGENERATE

# can_generate_thumbnail_for_image (thumbnail/mod.rs:195-202)
IMAGE_EXTENSIONS = ("jpg", "jpeg", "png", "webp", "gif", "svg", "heic", "heics", "heif", "heifs",
                    "avif", "bmp", "ico")
# what can_generate_thumbnail_for_video excludes (thumbnail/mod.rs:189-193)
_VIDEO_EXCLUDED = frozenset(("mpg", "swf", "m2v", "hevc", "m2ts", "mts", "ts"))


def video_extensions() -> tuple:
    """The Video extensions the thumbnailer accepts: every name of kind Video
    in the kind table but the seven can_generate_thumbnail_for_video excludes."""
    from .kind import ObjectKind, ext_table
    names = []
    for _, name, kind, _ in ext_table():
        if kind == ObjectKind.Video and name not in _VIDEO_EXCLUDED and name not in names:
            names.append(name)
    return tuple(names)


def _ptr(t):
    return t.data_ptr() if t is not None else None


def work_list(thumb_keys, keys, has_key=None, eligible=None, regenerate: bool = False,
              want_present: bool = False, ctx=None, trim: bool = True):
    """(work, dir_start, stats[, present]) for one column of file_path rows in
    ascending id order.  `thumb_keys`: int64 device tensor, the cas keys of the
    thumbnails on disk (duplicates allowed); `keys` int64 [n], `has_key` /
    `eligible` uint8 [n] or None (every row keyed / eligible).  A row is a
    candidate when it is keyed, eligible and (its thumbnail is missing or
    `regenerate`); `work` (int32) lists the lowest candidate row of every
    distinct key, ordered by shard directory (the first cas byte), ascending
    inside a directory; `dir_start` (int32 [257]) are the directories' offsets
    into it, dir_start[256] = len(work); `stats` (int32 [4]) = keyed rows whose
    thumbnail exists, keyed eligible rows, those of them whose thumbnail
    exists, len(work); `present` (uint8 [n]) = thumbnail_exists per row.
    trim=False: the full-length list, no synchronisation."""
    import torch
    dev = keys.device
    ctx = ctx or default_context(dev.index)
    n = keys.numel()
    work = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    start = torch.empty(257, dtype=torch.int32, device=dev)
    stats = torch.empty(4, dtype=torch.int32, device=dev)
    present = torch.empty(max(n, 1), dtype=torch.uint8, device=dev) if want_present else None
    s = torch.cuda.current_stream(dev).cuda_stream
    check(ctx.lib.sdgpu_thumbnail_worklist_device(
        ctx.h, thumb_keys.data_ptr(), thumb_keys.numel(), keys.data_ptr(), _ptr(has_key),
        _ptr(eligible), n, REGENERATE if regenerate else 0, _ptr(present), work.data_ptr(),
        start.data_ptr(), stats.data_ptr(), s), "sdgpu_thumbnail_worklist_device")
    if trim:
        work = work[:int(start[256].item())]
    out = (work, start, stats)
    return out + (present[:n],) if want_present else out


def thumbnail_exists(thumb_keys, keys, has_key=None, ctx=None):
    """present (uint8 [n]): 1 where the row has a cas_id and a thumbnail of it
    is on disk -- Library::thumbnail_exists for a page of rows, through the
    call's presence-only mode (no grouping runs)."""
    import torch
    dev = keys.device
    ctx = ctx or default_context(dev.index)
    n = keys.numel()
    present = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
    stats = torch.empty(4, dtype=torch.int32, device=dev)
    s = torch.cuda.current_stream(dev).cuda_stream
    check(ctx.lib.sdgpu_thumbnail_worklist_device(
        ctx.h, thumb_keys.data_ptr(), thumb_keys.numel(), keys.data_ptr(), _ptr(has_key), None, n,
        0, present.data_ptr(), None, None, stats.data_ptr(), s), "sdgpu_thumbnail_worklist_device")
    return present[:n]


def work_list_host(thumb_keys, keys, has_key=None, eligible=None, regenerate: bool = False,
                   want_present: bool = False, ctx=None):
    """sdgpu_thumbnail_worklist: the same on numpy arrays (uint64 keys, uint8
    masks or None); returns (work, dir_start, stats[, present]) as uint32 /
    uint8 arrays, work trimmed."""
    import numpy as np
    ctx = ctx or default_context()
    thumb_keys = np.ascontiguousarray(thumb_keys, dtype=np.uint64)
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    has_key = None if has_key is None else np.ascontiguousarray(has_key, dtype=np.uint8)
    eligible = None if eligible is None else np.ascontiguousarray(eligible, dtype=np.uint8)
    n = keys.size
    work = np.empty(max(n, 1), dtype=np.uint32)
    start = np.empty(257, dtype=np.uint32)
    stats = np.empty(4, dtype=np.uint32)
    present = np.empty(max(n, 1), dtype=np.uint8) if want_present else None
    data = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    check(ctx.lib.sdgpu_thumbnail_worklist(
        ctx.h, thumb_keys.ctypes.data, thumb_keys.size, keys.ctypes.data, data(has_key),
        data(eligible), n, REGENERATE if regenerate else 0, data(present), work.ctypes.data,
        start.ctypes.data, stats.ctypes.data), "sdgpu_thumbnail_worklist")
    out = (work[:int(start[256])], start, stats)
    return out + (present[:n],) if want_present else out


def _extension(name: str):
    """What follows the last dot of a file name; a name that only starts with a
    dot, or has none, has no extension."""
    i = name.rfind(".")
    return name[i + 1:] if i > 0 else None


def eligible_rows(table, location_id: int, extensions, under: str | None = None,
                  children_of: str | None = None):
    """The media processor's query (media_processor/mod.rs:74-116) on a
    FilePaths table, as a uint8 mask over its rows in id order: the location,
    not a directory, `extension IN extensions`, and materialized_path starting
    with `under` (get_all_children_files_by_extensions) or equal to
    `children_of` (get_files_by_extensions, the shallow job).  `cas_id NOT
    NULL` is the call's has_key column, not part of this mask.

    Case rule: a row's extension is what follows the last dot of its name, and
    it is compared exactly, byte for byte, with the given names -- the lower-
    case names of the kind table -- as the database's `IN` does: `A.JPG` is not
    eligible for "jpg"."""
    import numpy as np
    wanted = frozenset(extensions)
    out = np.zeros(len(table), dtype=np.uint8)
    for i in range(len(table)):
        if table.location_id[i] != location_id or table.is_dir[i]:
            continue
        mp = table.materialized_path[i]
        if (children_of is not None and mp != children_of) or \
                (under is not None and not mp.startswith(under)):
            continue
        if _extension(table.name[i]) in wanted:
            out[i] = 1
    return out


def disk_keys(thumbnails_directory):
    """The cas keys (numpy uint64) of the thumbnails the reference's stat of
    `<base>/<cas_id[0..2]>/<cas_id>.webp` can find: a stem of 16 lower-case hex
    characters lying in the shard directory its first two characters name.  A
    misplaced copy, which the remover takes where it finds it, does not count."""
    import numpy as np
    keys = []
    for path, stems in scan_thumbnails(thumbnails_directory):
        shard = os.path.basename(path)
        keys += [k for s, k in zip(stems, map(cas_key, stems)) if k is not None and s[:2] == shard]
    return np.array(keys, dtype=np.uint64)


def process(table, location_id: int, location_path, thumbnails_directory, generate,
            regenerate: bool = False, under: str | None = None, children_of: str | None = None,
            ctx=None):
    """thumbnail::process for a whole location (or sub-path) at once: the
    query, the scan of the cache, one device call, then `generate(kind,
    input_path, output_path)` for the work rows in work-list order -- shard
    directory by shard directory, each directory that has work created once
    first (to_create_dirs, mod.rs:258-265,284).  `kind` is "image" or "video",
    from the row's extension.  Returns (created, skipped, errors): created =
    the generate calls that returned; skipped = the eligible rows whose
    thumbnail existed (when not regenerating) plus the candidates dropped as
    later copies of a work row's cas_id; a generate that raises adds `Had an
    error generating thumbnail for "<input path>"` to errors and the loop goes
    on (mod.rs:350-353, process_single_thumbnail)."""
    import numpy as np
    import torch
    images, videos = frozenset(IMAGE_EXTENSIONS), frozenset(video_extensions())
    eligible = eligible_rows(table, location_id, images | videos, under, children_of)
    has = np.fromiter((c is not None for c in table.cas_id), dtype=np.uint8, count=len(table))
    keys = np.fromiter((int.from_bytes(bytes.fromhex(c), "little") if c is not None else 0
                        for c in table.cas_id), dtype=np.uint64, count=len(table))
    dev = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    work, start, stats = work_list(dev(disk_keys(thumbnails_directory).view(np.int64)),
                                   dev(keys.view(np.int64)), dev(has), dev(eligible),
                                   regenerate=regenerate, ctx=ctx)
    work, start, stats = work.cpu().numpy(), start.cpu().numpy(), stats.cpu().numpy()
    base, root = os.fspath(thumbnails_directory), os.fspath(location_path)
    created, errors = 0, []
    for d in np.flatnonzero(np.diff(start)):
        shard_dir = os.path.join(base, "%02x" % d)
        os.makedirs(shard_dir, exist_ok=True)
        for i in work[start[d]:start[d + 1]].tolist():
            input_path = os.path.join(root, table.rel_path(i + 1))
            kind = "image" if _extension(table.name[i]) in images else "video"
            try:
                generate(kind, input_path, os.path.join(shard_dir, table.cas_id[i] + ".webp"))
            except Exception:
                errors.append(f'Had an error generating thumbnail for "{input_path}"')
                continue
            created += 1
    # existing ones (stats[2], when not regenerating) + candidates that are no work rows
    return created, int(stats[1]) - int(stats[3]), errors
