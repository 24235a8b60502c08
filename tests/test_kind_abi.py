"""CPU: the Object-kind surface -- the five C entry points and their header
comments, the extension table against the fixture, path -> extension id,
sdgpu_kind_of_file on real files against the oracle (tests/kind_oracle.py) and
the fixture (tests/golden/kinds.json) in both modes, the staging-slab layout
with the kind regions, the Python names and the Rust items.  The library loads
without a GPU; nothing here opens a device."""
import ctypes
import inspect
import json
import os
import re
import shutil
import subprocess

import pytest

from spacedrive_amd import _native
from spacedrive_amd import kind as K
from tests import kind_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sdgpu_kind_ext_ids", "sdgpu_kind_ext_name", "sdgpu_kind_of_file",
       "sdgpu_kind_batch_device", "sdgpu_identify_kind_files")


@pytest.fixture(scope="module")
def fixture():
    with open(os.path.join(ROOT, "tests", "golden", "kinds.json")) as f:
        return json.load(f)


def test_symbols_exported_and_arguments_rejected_without_a_device():
    lib = _native.load()
    assert set(NEW) <= set(_native.declared_symbols())
    out = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert set(NEW) <= exported
    assert lib.sdgpu_abi_version() == 6
    assert lib.sdgpu_kind_ext_ids(None, 1, None) == -22
    assert lib.sdgpu_kind_ext_ids(None, 0, None) == 0
    assert lib.sdgpu_kind_ext_name(1, None, None) == -22
    k = ctypes.c_int32(99)
    assert lib.sdgpu_kind_of_file(None, 0, ctypes.byref(k)) == -22
    assert lib.sdgpu_kind_of_file(b"x.jpg", 0, None) == -22
    for flags in (2, 3, 0x80000000):  # anything but 0 / SDGPU_KIND_VERIFY_MAGIC
        assert lib.sdgpu_kind_of_file(b"x.jpg", flags, ctypes.byref(k)) == -22
        assert lib.sdgpu_kind_batch_device(None, None, 0, None, None, None, 0, flags, None,
                                           None) == -22
    assert lib.sdgpu_kind_batch_device(None, None, 0, None, None, None, 0, 0, None, None) == -22
    assert lib.sdgpu_identify_kind_files(None, None, None, 0, 0, None, None, None, None, None,
                                         None) == -22
    assert len(lib.sdgpu_kind_batch_device.argtypes) == 10
    assert len(lib.sdgpu_identify_kind_files.argtypes) == 11


def test_header_marks_the_additions_and_cites_the_reference():
    text = open(os.path.join(ROOT, "include", "sdgpu.h")).read()
    assert "#define SDGPU_ABI_VERSION 6" in text
    assert "#define SDGPU_KIND_VERIFY_MAGIC 1u" in text
    for name in NEW:
        m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int " + name + r"\(", text, flags=re.S)
        assert m, name
        assert m.group(1).lstrip().startswith("(ABI 6, additive)"), name
        assert re.search(r"\b(magic|extensions|mod)\.rs:\d+", m.group(1)), name


def test_table_equals_the_fixture(fixture):
    rows = K.ext_table()
    assert [list(r) for r in rows] == fixture["names"]
    assert len(rows) == 215 and [r[0] for r in rows] == list(range(1, 216))
    assert len({r[1] for r in rows}) == 213
    assert sorted(r[1] for r in rows if r[3] != 0) == ["mts", "ts"]
    assert all((r[2], r[3]) == (K.ObjectKind.Video, K.ObjectKind.Code) for r in rows if r[3])
    # every kind is one of the 15 extension categories
    assert {r[2] for r in rows} == set(O.KIND.values()) - {0}
    lib = _native.load()
    name = ctypes.create_string_buffer(16)
    kinds = (ctypes.c_int32 * 2)()
    for past in (0, 216, 217, 65535, 0xFFFFFFFF):
        assert lib.sdgpu_kind_ext_name(past, name, kinds) == -2, past
    # the fixture's table is the oracle's, and the oracle's counts are the reference's
    v = O.variants()
    assert [r[1] for r in rows] == [n for _, n, _ in v]
    alts = [a for _, _, al in v if al for a in al]
    assert len(alts) == 127 and sum(1 for p, _ in alts if not p) == 17
    assert {o for _, o in alts} == {0, 4, 28}
    assert max(o + len(p) for p, o in alts) == 36


def test_reference_unit_expectations():
    """extensions.rs:370-388."""
    assert O.from_str("jpg") == [("Image", "jpg")]
    assert O.from_str("ts") == [("Video", "ts"), ("Code", "ts")]
    assert O.from_str("jeff") == []
    by_name = {}
    for i, name, k0, k1 in K.ext_table():
        by_name.setdefault(name, (i, k0, k1))
    ids = K.ext_ids(["a.jpg", "a.ts", "a.jeff"])
    assert by_name["jpg"] == (ids[0], K.ObjectKind.Image, 0)
    assert by_name["ts"] == (ids[1], K.ObjectKind.Video, K.ObjectKind.Code)
    assert ids[2] == 0 and "jeff" not in by_name


def test_ext_ids_on_name_shapes():
    first = {}
    for i, name, _, _ in K.ext_table():
        first.setdefault(name, i)
    shapes = [
        ("a", 0), (".bashrc", 0), (".x.rs", first["rs"]), ("a.", 0), ("A.JPG", first["jpg"]),
        ("a.tar.GZ", first["gz"]), ("a.Kt", first["kt"]), ("a.K", 0),
        ("dir.d/x.y/file", 0), ("dir.jpg/file", 0), ("dir.jpg/file.PnG", first["png"]),
        ("/abs/p.a.t.h/.hidden", 0), ("a.jpg/", first["jpg"]), ("a.jpg/.", first["jpg"]),
        ("..", 0), ("a/..", 0), ("...", 0), ("", 0), ("/", 0), ("a.jeff", 0),
        ("a.3GP", first["3gp"]), ("a.7Z", first["7z"]), ("a.applescript", first["applescript"]),
        ("a.applescripts", 0), ("a.ts", first["ts"]), ("a.mts", first["mts"]),
        # the conflict is matched on the extension as written (magic.rs:217-232)
        ("a.TS", 0), ("a.Mts", 0), ("a.tsx", first["tsx"]),
        ("a.İni", 0), ("a.jpég", 0),
    ]
    got = K.ext_ids([s for s, _ in shapes])
    assert [(s, int(g)) for (s, _), g in zip(shapes, got)] == [(s, w) for s, w in shapes]
    # the oracle agrees on which of them have an Extension, and on its kind
    for s, w in shapes:
        want_kind = O.resolve_conflicting(s, b"", False)
        if w == 0:
            assert want_kind == 0, s
        else:
            assert want_kind in (K.ext_table()[w - 1][2], K.ext_table()[w - 1][3]), s
    # an extension that is not UTF-8 gives no Extension; neither does a
    # well-formed name behind ill-formed bytes elsewhere in the extension
    lib = _native.load()
    raw = [b"a.\xffpg", b"a.jp\xc3", b"a.\xe2\x84", b"a.\xe2\x84\xaat", b"\xff\xfe.jpg"]
    arr = (ctypes.c_char_p * len(raw))(*raw)
    out = (ctypes.c_uint16 * len(raw))()
    assert lib.sdgpu_kind_ext_ids(arr, len(raw), out) == 0
    assert list(out) == [0, 0, 0, first["kt"], first["jpg"]]
    assert [O.extension_of(r) is None for r in raw] == [True, True, True, False, False]


def test_kind_of_file_against_oracle_and_fixture(tmp_path, fixture):
    """Every non-empty alternative matching at exactly offset + length bytes,
    one byte shorter, with each fixed byte flipped; the empty alternatives on
    empty files; the ts / mts shapes -- on real files, both modes."""
    cases = O.cases()
    assert len(cases) == len(fixture["cases"]) > 1000
    seen_alts = 0
    for k, ((fname, content), rec) in enumerate(zip(cases, fixture["cases"])):
        assert rec[:3] == [fname, len(content), content[:48].hex()], k
        sub = tmp_path / str(k)
        sub.mkdir()
        path = os.path.join(os.fsencode(sub), fname.encode("utf-8"))
        with open(path, "wb") as f:
            f.write(content)
        for mode, verify in enumerate((False, True)):
            want = O.resolve_conflicting(fname, content, verify)
            assert rec[3 + mode] == want, (fname, content.hex(), verify)
            assert int(K.kind_of_file(path, verify)) == want, (fname, content.hex(), verify)
        seen_alts += 1
    by = {(n, bytes.fromhex(h)): (a, b) for n, s, h, a, b in fixture["cases"] if s <= 48}
    assert by[("x.ts", b"")] == (20, 20) and by[("x.mts", b"")] == (20, 20)
    assert by[("x.ts", b"\x47")] == (7, 7) and by[("x.mts", b"\x47")] == (7, 7)
    assert by[("x.ts", b"\x00\x01\x02\x47")] == (20, 20)
    assert by[("x.mts", b"\x00\x01\x02\x47")] == (7, 7)
    assert by[("f.mjpeg", b"")] == (7, 7) and by[("f.db", b"")] == (21, 21)
    # verify mode drops a verified name whose signature is absent, and only those
    assert by[("A.JPG", b"")] == (5, 0) and by[("f.pdf", b"")] == (1, 1)
    assert by[("f.epub", b"")] == (22, 22) and by[("f.txt", b"")] == (3, 3)


def test_kind_of_file_missing_path_and_directory(tmp_path):
    lib = _native.load()
    k = ctypes.c_int32(99)
    for flags in (0, 1):
        for name in ("missing.jpg", "missing.ts", "missing.txt"):
            k.value = 99
            assert lib.sdgpu_kind_of_file(os.fsencode(tmp_path / name), flags,
                                          ctypes.byref(k)) == 0
            assert k.value == 0, name
    d = tmp_path / "dir.ts"
    d.mkdir()
    assert K.kind_of_file(d) == K.ObjectKind.Code       # opens; read_exact fails
    d2 = tmp_path / "dir.png"
    d2.mkdir()
    assert K.kind_of_file(d2) == K.ObjectKind.Image and K.kind_of_file(d2, True) == 0
    # a name without an Extension is not opened at all: an unreadable path is no error
    assert K.kind_of_file(tmp_path / "missing") == K.ObjectKind.Unknown


def test_object_kind_enum_is_kind_rs():
    want = ["Unknown", "Document", "Folder", "Text", "Package", "Image", "Audio", "Video",
            "Archive", "Executable", "Alias", "Encrypted", "Key", "Link", "WebPageArchive",
            "Widget", "Album", "Collection", "Font", "Mesh", "Code", "Database", "Book", "Config"]
    assert [m.name for m in K.ObjectKind] == want
    assert [int(m) for m in K.ObjectKind] == list(range(24))
    assert all(int(K.ObjectKind[c]) == v for c, v in O.KIND.items())


_LAYOUT_MAIN = r'''
#include <stdio.h>
#include "spacedrive_amd/csrc/host_io.hpp"
int main() {
  const size_t caps[] = {4096, 65536 + 17, size_t(256) << 20};
  const unsigned files[] = {1, 7, 65536};
  for (size_t a : caps)
    for (unsigned f : files)
      for (int sums = 0; sums < 2; ++sums) {
        const auto L = sdgpu::hostio::slab_layout(a, f, sums != 0);
        const auto K = sdgpu::hostio::slab_layout(a, f, sums != 0, true);
        printf("%zu %u %d  %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu  "
               "%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", a, f, sums,
               L.off, L.len, L.out, L.status, L.whole, L.sum, L.has, L.ext, L.kind, L.total,
               K.off, K.len, K.out, K.status, K.whole, K.sum, K.has, K.ext, K.kind, K.total);
      }
  return 0;
}
'''


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_slab_layout_with_kind_regions(tmp_path):
    """slab_layout(a, f) and slab_layout(a, f, true) keep every offset (restated
    here); the kind regions lie behind everything else, disjoint, 256-B aligned
    and large enough (u16 ids up, u8 kinds back)."""
    src = tmp_path / "layout.cpp"
    src.write_text(_LAYOUT_MAIN)
    exe = tmp_path / "layout"
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", ROOT, "-pthread", str(src), "-o", str(exe)],
                   check=True, capture_output=True, text=True)
    rows = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    rows = [[int(x) for x in r.split()] for r in rows if r.strip()]
    assert len(rows) == 18
    up = lambda x: (x + 255) // 256 * 256  # noqa: E731
    for r in rows:
        a, f, sums = r[:3]
        off, ln, out, status, whole, sm, has, ext, kind, total = r[3:13]
        koff, kln, kout, kstatus, kwhole, ksm, khas, kext, kkind, ktotal = r[13:]
        want = [up(a)]
        want.append(up(want[0] + 8 * f))
        want.append(up(want[1] + 4 * f))
        want.append(up(want[2] + 8 * f))
        end = up(want[3] + 4 * f)
        assert [off, ln, out, status] == want, (a, f, sums)
        if sums:
            assert whole == end and sm == up(whole + f) and has == up(sm + 32 * f)
            end = up(has + f)
        else:
            assert (whole, sm, has) == (0, 0, 0)
        assert total == end and (ext, kind) == (0, 0)
        # with kinds: nothing before moves
        assert [koff, kln, kout, kstatus, kwhole, ksm, khas] == [off, ln, out, status, whole, sm, has]
        assert kext >= total and kkind >= kext + 2 * f and ktotal >= kkind + f
        assert kext % 256 == 0 and kkind % 256 == 0 and ktotal % 256 == 0


def test_python_names_and_unchanged_identify():
    import numpy as np

    from spacedrive_amd import file_identifier as fi
    assert list(inspect.signature(fi.identify).parameters) == ["paths", "sizes", "ctx", "checksums"]
    p = inspect.signature(fi.identify_metadata).parameters
    assert list(p) == ["paths", "sizes", "ctx", "checksums", "verify_magic"]
    assert p["checksums"].default is False and p["verify_magic"].default is False
    p = inspect.signature(K.kind_batch_device).parameters
    assert list(p) == ["arena", "off", "length", "ext", "verify", "out", "ctx", "stream"]
    assert list(inspect.signature(K.kind_of_file).parameters) == ["path", "verify"]
    assert callable(K.ext_ids) and callable(K.ext_table)
    r = fi.IdentifyResult(np.zeros((2, 8), np.uint8), np.ones(2, np.uint8), np.zeros(2, np.int32),
                          None)
    assert r.kind is None and r.kinds() == [None, None]
    fields = [f.name for f in fi.IdentifyResult.__dataclass_fields__.values()]
    assert fields[-1] == "kind" and fields[:6] == ["cas8", "has_key", "status", "sizes",
                                                   "checksum32", "has_checksum"]
    r = fi.IdentifyResult(r.cas8, r.has_key, np.array([0, -2], np.int32), None,
                          kind=np.array([5, 0], np.int32))
    assert r.kinds() == [K.ObjectKind.Image, None]
    assert inspect.signature(fi.FileIdentifierJob.__init__).parameters["kinds"].default is False
    assert inspect.signature(fi.shallow).parameters["kinds"].default is False
    t = fi.FilePaths()
    t.add(1, "/", "a.jpg")
    assert t.object_kind == {}
    # persisted like `checksums`
    assert '"kinds": self.kinds' in inspect.getsource(fi.FileIdentifierJob.state)
    assert 'state.get("kinds", False)' in inspect.getsource(fi.FileIdentifierJob.resume.__func__)


def test_file_metadata_docstring_has_no_unknown_caveat():
    from spacedrive_amd import file_identifier as fi
    assert "stays ObjectKind::Unknown" not in (fi.__doc__ or "")
    assert "kind_of_file" in inspect.getsource(fi.file_metadata)


def test_rust_items():
    src = open(os.path.join(ROOT, "crates", "sd-core-gpu", "src", "identifier.rs")).read()
    assert "pub fn identify_with_kinds(" in src
    assert "sys::sdgpu_identify_kind_files(" in src
    job = open(os.path.join(ROOT, "crates", "sd-core-gpu", "src", "job.rs")).read()
    assert "kind" in job[job.index("pub trait OrphanTable"):]
    sysrs = open(os.path.join(ROOT, "crates", "sdgpu-sys", "src", "lib.rs")).read()
    for name in NEW:
        assert f"pub fn {name}(" in sysrs
