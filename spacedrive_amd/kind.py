"""Object kind -- host mirror of sd-file-ext (crates/file-ext) over libsdgpu.

* ``ObjectKind``: the 24 values of crates/file-ext/src/kind.rs.
* ``ext_ids(paths)``: the extension id of each path (0 = no Extension, else
  1..215; magic.rs:180-186: Path::extension, to_str, to_lowercase, from_str).
* ``ext_table()``: the table, enumerated through the library.
* ``kind_of_file(path, verify=False)``: Extension::resolve_conflicting
  (magic.rs:176-236) as the reference does it -- the file is opened, and read
  only when the decision needs its first bytes.
* ``kind_batch_device``: the kinds of device-resident cas messages (k_kind,
  spacedrive_amd/csrc/kind.hip): the file's first bytes are the first bytes of
  its cas message behind the 8-byte size prefix.

The table and the matcher live in the library only
(spacedrive_amd/csrc/kind_table.hpp); nothing here decides a kind in Python.
"""
from __future__ import annotations

import ctypes
import enum
import os

import numpy as np

from ._native import check, default_context, load

VERIFY_MAGIC = 1  # SDGPU_KIND_VERIFY_MAGIC


class ObjectKind(enum.IntEnum):
    """crates/file-ext/src/kind.rs:6-55 (the order never changes)."""
    Unknown = 0
    Document = 1
    Folder = 2
    Text = 3
    Package = 4
    Image = 5
    Audio = 6
    Video = 7
    Archive = 8
    Executable = 9
    Alias = 10
    Encrypted = 11
    Key = 12
    Link = 13
    WebPageArchive = 14
    Widget = 15
    Album = 16
    Collection = 17
    Font = 18
    Mesh = 19
    Code = 20
    Database = 21
    Book = 22
    Config = 23


def _c_paths(paths):
    enc = [os.fsencode(os.fspath(p)) for p in paths]
    return (ctypes.c_char_p * len(enc))(*enc)


def ext_ids(paths) -> np.ndarray:
    """Extension id (uint16) of every path; 0 = no Extension."""
    paths = list(paths)
    out = np.zeros(len(paths), np.uint16)
    check(load().sdgpu_kind_ext_ids(_c_paths(paths), len(paths), out.ctypes.data),
          "sdgpu_kind_ext_ids")
    return out


def ext_table() -> list[tuple[int, str, int, int]]:
    """[(ext id, name, kind, second kind or 0)] for every id of the table."""
    lib = load()
    rows = []
    i = 1
    while True:
        name = ctypes.create_string_buffer(16)
        kinds = (ctypes.c_int32 * 2)()
        rc = lib.sdgpu_kind_ext_name(i, name, kinds)
        if rc == -2:  # -ENOENT: past the end
            return rows
        check(rc, "sdgpu_kind_ext_name")
        rows.append((i, name.value.decode(), int(kinds[0]), int(kinds[1])))
        i += 1


def kind_of_file(path, verify: bool = False) -> ObjectKind:
    """ObjectKind of one file by name and, where the decision needs them,
    first bytes; Unknown when the path has no Extension or cannot be opened."""
    k = ctypes.c_int32()
    check(load().sdgpu_kind_of_file(os.fsencode(os.fspath(path)), VERIFY_MAGIC if verify else 0,
                                    ctypes.byref(k)), "sdgpu_kind_of_file")
    return ObjectKind(k.value)


def kind_batch_device(arena, off, length, ext, verify: bool = False, out=None, ctx=None,
                      stream=None):
    """k_kind over device tensors (torch): arena uint8, off int64, length int32
    as for ``cas.cas_batch_device``, ext uint16 (``ext_ids``).  Returns
    kind[n] uint8 on the same device (0 for a message cas_batch_device would
    reject); asynchronous on `stream` (default: torch's current stream)."""
    import torch
    ctx = ctx or default_context(arena.device.index)
    n = off.numel()
    if ext.numel() != n or ext.element_size() != 2:
        raise ValueError("ext must hold one 16-bit id per message")
    if out is None:
        out = torch.empty(n, dtype=torch.uint8, device=arena.device)
    s = stream if stream is not None else torch.cuda.current_stream(arena.device).cuda_stream
    check(ctx.lib.sdgpu_kind_batch_device(ctx.h, arena.data_ptr(), arena.numel(), off.data_ptr(),
                                          length.data_ptr(), ext.data_ptr(), n,
                                          VERIFY_MAGIC if verify else 0, out.data_ptr(), s),
          "sdgpu_kind_batch_device")
    return out


__all__ = ["ObjectKind", "VERIFY_MAGIC", "ext_ids", "ext_table", "kind_of_file",
           "kind_batch_device"]
