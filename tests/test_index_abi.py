"""CPU: the library-lifetime Object index entry points (lookup, remove,
remove_objects, export, stats -- include/sdgpu.h, "ABI 6, additive") reject
NULL arguments without a device, the Python constant matches the header, and
the Rust crate wraps all five."""
import ctypes
import os
import re

from spacedrive_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_new_entry_points_reject_null_without_device():
    lib = _native.load()
    assert lib.sdgpu_index_lookup_device(None, None, 1, None, None) == -22
    assert lib.sdgpu_index_lookup(None, None, 1, None) == -22
    assert lib.sdgpu_index_remove_device(None, None, None, 1, None, None) == -22
    assert lib.sdgpu_index_remove_objects_device(None, None, 1, 10, None, None) == -22
    assert lib.sdgpu_index_export_device(None, None, None, 0, None, None) == -22
    assert lib.sdgpu_index_stats(None, None) == -22
    out = (ctypes.c_uint64 * 3)()
    assert lib.sdgpu_index_stats(None, out) == -22


def test_index_miss_matches_header():
    hdr = open(_native.HEADER_PATH).read()
    m = re.search(r"#define SDGPU_INDEX_MISS (0x[0-9a-fA-F]+)u?\b", hdr)
    assert m and int(m.group(1), 16) == _native.INDEX_MISS == 0xFFFFFFFF
    assert re.search(r"#define SDGPU_ABI_VERSION 6\b", hdr)


def test_header_marks_the_additions():
    hdr = open(_native.HEADER_PATH).read()
    for name in ("sdgpu_index_lookup_device", "sdgpu_index_lookup", "sdgpu_index_remove_device",
                 "sdgpu_index_remove_objects_device", "sdgpu_index_export_device",
                 "sdgpu_index_stats"):
        # the comment right above each declaration carries the marker
        before = hdr[:hdr.index("int " + name + "(")]
        last = before[before.rindex("/*"):]
        assert "(ABI 6, additive)" in last, name


def test_rust_identifier_names_the_five_wrappers():
    rs = open(os.path.join(ROOT, "crates", "sd-core-gpu", "src", "identifier.rs")).read()
    for fn in ("lookup", "remove", "remove_objects", "export", "stats"):
        assert re.search(r"pub fn " + fn + r"\(&self", rs), fn
    for sym in ("sdgpu_index_lookup", "sdgpu_index_remove_device",
                "sdgpu_index_remove_objects_device", "sdgpu_index_export_device",
                "sdgpu_index_stats"):
        assert "sys::" + sym + "(" in rs, sym


def test_python_index_has_the_methods():
    from spacedrive_amd import consumers, dedup
    for m in ("lookup", "remove", "remove_objects", "export", "stats"):
        assert callable(getattr(dedup.ObjectIndex, m)), m
    assert callable(consumers.remove_orphans_from_index)
