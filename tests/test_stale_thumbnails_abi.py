"""CPU: the thumbnail remover's entry points (include/sdgpu.h, "ABI 6,
additive") reject NULL arguments without a device, the Rust crate wraps them,
the Python module has its four names, and its host-only paths -- the scan of
the cache and a sweep with no library loaded -- equal the restatement of
thumbnail_remover.rs:236-367 in tests/thumb_oracle.py."""
import os
import re
import shutil

import pytest

from spacedrive_amd import _native
from tests import thumb_oracle as TO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KEPT = "00112233445566aa"       # held by the non-indexed set
UPPER = "AABBCCDDEEFF0011"      # uppercase hex: no database cas_id equals it


def test_entry_points_reject_null_without_device():
    lib = _native.load()
    assert lib.sdgpu_stale_thumbnails_device(None, None, 0, None, 0, None, None, None, 0, None,
                                             None, None) == -22
    assert lib.sdgpu_stale_thumbnails(None, None, 0, None, 0, None, None, None, 0, None,
                                      None) == -22


def test_header_marks_the_additions():
    hdr = open(_native.HEADER_PATH).read()
    assert re.search(r"#define SDGPU_ABI_VERSION 6\b", hdr)
    for name in ("sdgpu_stale_thumbnails_device", "sdgpu_stale_thumbnails"):
        before = hdr[:hdr.index("int " + name + "(")]
        last = before[before.rindex("/*"):]
        assert "(ABI 6, additive)" in last, name


def test_rust_names_the_wrapper():
    src = os.path.join(ROOT, "crates", "sd-core-gpu", "src")
    rs = open(os.path.join(src, "thumbnail_remover.rs")).read()
    assert re.search(r"pub fn stale_thumbnails\(", rs)
    assert re.search(r"pub fn process_clean_up\(", rs)
    assert "sys::sdgpu_stale_thumbnails(" in rs
    used = set(re.findall(r"sys::(sdgpu_\w+)\(", rs))
    assert used <= set(_native.declared_symbols()), used
    assert re.search(r"\bpub mod thumbnail_remover\b", open(os.path.join(src, "lib.rs")).read())


def test_python_module_has_the_names():
    import spacedrive_amd
    from spacedrive_amd import thumbnail_remover as T
    for name in ("stale_thumbnails", "scan_thumbnails", "process_clean_up", "ThumbnailRemover"):
        assert callable(getattr(T, name)), name
    assert spacedrive_amd.thumbnail_remover is T
    for m in ("add_library", "remove_library", "new_non_indexed_thumbnail", "run"):
        assert callable(getattr(T.ThumbnailRemover, m)), m
    text = open(T.__file__).read()
    assert "oracle" not in text


def make_odd_tree(root):
    """A cache with every oddity of thumbnail_remover.rs:249-299."""
    os.makedirs(root)
    with open(os.path.join(root, "version.txt"), "w") as f:
        f.write("1")
    files = {
        "00": [KEPT + ".webp", "00aabbccddeeff11.webp", ".webp", "X.WEBP"],
        "a1": ["a.b.webp", "not-a-cas-id.webp", UPPER + ".webp", "a1ffffffffffffff.webp"],
        "zz": ["a1000000000000aa.webp"],      # not in the directory its cas_id names
        "only_other": ["notes.txt"],          # nothing found: the reference removes it (and fails)
    }
    for d, names in files.items():
        os.makedirs(os.path.join(root, d))
        for n in names:
            with open(os.path.join(root, d, n), "wb") as f:
                f.write(b"w")
    os.makedirs(os.path.join(root, "ee"))     # an empty shard directory
    outside = root + "_outside"
    os.makedirs(outside)
    with open(os.path.join(outside, "ffffffffffffffff.webp"), "wb") as f:
        f.write(b"w")
    os.symlink(outside, os.path.join(root, "ln"))   # a symlinked directory: not followed
    return outside


def test_scan_matches_the_reference_rules(tmp_path):
    from spacedrive_amd import thumbnail_remover as T
    root = str(tmp_path / "thumbs")
    make_odd_tree(root)
    got = {os.path.basename(d): sorted(s) for d, s in T.scan_thumbnails(root)}
    assert got == {
        "00": sorted([KEPT, "00aabbccddeeff11"]),
        "a1": sorted(["a.b", "not-a-cas-id", UPPER, "a1ffffffffffffff"]),
        "zz": ["a1000000000000aa"],
        "only_other": [],
        "ee": [],
    }
    fresh = str(tmp_path / "made" / "thumbs")     # create_dir_all first
    assert T.scan_thumbnails(fresh) == [] and os.path.isdir(fresh)
    assert T.cas_key(UPPER) is None and T.cas_key("a.b") is None
    assert T.cas_key("0100000000000080") == 0x8000000000000001


def test_dry_run_without_libraries_equals_the_oracle(tmp_path):
    """No library loaded: nothing to probe, the host decides everything."""
    from spacedrive_amd import thumbnail_remover as T
    root = str(tmp_path / "thumbs")
    make_odd_tree(root)
    before = TO.listing(root)
    non_indexed = {KEPT, UPPER, "0000000000000001"}
    rep = T.process_clean_up(root, [], non_indexed, dry_run=True)
    files, dirs = TO.process_clean_up(root, [], non_indexed, dry_run=True)
    assert sorted(rep["removed_files"]) == files and sorted(rep["removed_dirs"]) == dirs
    assert TO.listing(root) == before
    names = {os.path.relpath(f, root) for f in files}
    assert names == {"00/00aabbccddeeff11.webp", "a1/a.b.webp", "a1/not-a-cas-id.webp",
                     "a1/a1ffffffffffffff.webp", "zz/a1000000000000aa.webp"}
    assert {os.path.basename(d) for d in dirs} == {"zz", "only_other", "ee"}


def test_sweep_without_libraries_equals_the_oracle(tmp_path):
    from spacedrive_amd import thumbnail_remover as T
    root, copy = str(tmp_path / "thumbs"), str(tmp_path / "copy")
    make_odd_tree(root)
    shutil.rmtree(os.path.join(root, "only_other"))   # its rmdir fails in the reference too
    shutil.copytree(root, copy, symlinks=True)
    non_indexed = {KEPT, UPPER}
    rep = T.process_clean_up(root, [], non_indexed)
    files, dirs = TO.process_clean_up(copy, [], non_indexed)
    assert TO.listing(root) == TO.listing(copy)
    assert sorted(os.path.relpath(f, root) for f in rep["removed_files"]) == \
        sorted(os.path.relpath(f, copy) for f in files)
    assert sorted(os.path.relpath(d, root) for d in rep["removed_dirs"]) == \
        sorted(os.path.relpath(d, copy) for d in dirs)
    assert os.path.exists(os.path.join(root + "_outside", "ffffffffffffffff.webp"))
    assert T.process_clean_up(root, [], non_indexed) == {"removed_files": [], "removed_dirs": []}


def test_directory_of_other_files_fails_like_the_reference(tmp_path):
    """A directory with no webp entry is removed with remove_dir (:301-311),
    which fails while other files are in it: the error propagates."""
    from spacedrive_amd import thumbnail_remover as T
    root = str(tmp_path / "thumbs")
    os.makedirs(os.path.join(root, "aa"))
    with open(os.path.join(root, "aa", "notes.txt"), "w") as f:
        f.write("x")
    with pytest.raises(OSError):
        T.process_clean_up(root, [], set())
    with pytest.raises(OSError):
        TO.process_clean_up(root, [], set())


def test_error_in_the_third_directory_leaves_the_first_two_swept(tmp_path):
    from spacedrive_amd import thumbnail_remover as T
    root = str(tmp_path / "thumbs")
    for d in ("11", "22", "33", "44", "55"):
        os.makedirs(os.path.join(root, d))
        for i in range(3):
            with open(os.path.join(root, d, f"{d}0000000000000{i}.webp"), "wb") as f:
                f.write(b"w")
    order = [n for n in os.listdir(root)]            # the scan's order
    with open(os.path.join(os.fsencode(root), os.fsencode(order[2]), b"\xff\xfe.webp"), "wb") as f:
        f.write(b"w")
    keep = order[0] + "00000000000001"               # one thumbnail of the first directory stays
    with pytest.raises(T.NonUtf8PathError) as e:
        T.process_clean_up(root, [], {keep})
    assert os.path.basename(str(e.value.args[0])) == order[2]
    assert os.listdir(os.path.join(root, order[0])) == [keep + ".webp"]
    assert not os.path.exists(os.path.join(root, order[1]))
    for d in order[2:]:
        assert len(os.listdir(os.path.join(root, d))) >= 3
    with pytest.raises(T.NonUtf8PathError):
        T.scan_thumbnails(root)
    with pytest.raises(TO.NonUtf8Path):               # the restatement stops at the same place
        TO.process_clean_up(root, [], {keep}, dry_run=True)
