"""CPU: the surface of the identifier call that also returns the
integrity_checksum of the files it read whole -- the two C entry points, their
header comments, the staging-slab layout with and without the checksum regions,
the Python names and the Rust wrapper.  No compute calls (no GPU here)."""
import inspect
import os
import re
import shutil
import subprocess

import pytest

from spacedrive_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sdgpu_cas_checksum_batch_device", "sdgpu_identify_checksum_files")


def test_symbols_exported_and_reject_null_without_a_device():
    lib = _native.load()
    assert set(NEW) <= set(_native.declared_symbols())
    out = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert set(NEW) <= exported
    assert lib.sdgpu_abi_version() == 6
    assert lib.sdgpu_cas_checksum_batch_device(None, None, 0, None, None, None, 0, None, None,
                                               None, None, None) == -22
    assert lib.sdgpu_identify_checksum_files(None, None, None, 0, None, None, None, None,
                                             None) == -22
    assert len(lib.sdgpu_cas_checksum_batch_device.argtypes) == 12
    assert len(lib.sdgpu_identify_checksum_files.argtypes) == 9


def test_header_marks_the_additions():
    text = open(os.path.join(ROOT, "include", "sdgpu.h")).read()
    assert "#define SDGPU_ABI_VERSION 6" in text
    for name in NEW:
        # the comment block that ends right before the declaration
        m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int " + name + r"\(", text, flags=re.S)
        assert m, name
        assert m.group(1).lstrip().startswith("(ABI 6, additive)"), name


_LAYOUT_MAIN = r'''
#include <stdio.h>
#include "spacedrive_amd/csrc/host_io.hpp"
int main() {
  const size_t caps[] = {4096, 65536 + 17, size_t(256) << 20};
  const unsigned files[] = {1, 7, 65536};
  for (size_t a : caps)
    for (unsigned f : files) {
      const auto L = sdgpu::hostio::slab_layout(a, f);
      const auto C = sdgpu::hostio::slab_layout(a, f, true);
      printf("%zu %u %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", a, f,
             L.off, L.len, L.out, L.status, L.total, L.whole, L.sum, L.has,
             C.off, C.len, C.out, C.status, C.whole, C.sum, C.has, C.total);
    }
  return 0;
}
'''


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_slab_layout_keeps_its_offsets(tmp_path):
    """slab_layout(a, f) gives the offsets it always gave (restated here), and
    the checksum regions of slab_layout(a, f, true) lie behind them, disjoint,
    256-B aligned and large enough."""
    src = tmp_path / "layout.cpp"
    src.write_text(_LAYOUT_MAIN)
    exe = tmp_path / "layout"
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", ROOT, "-pthread", str(src), "-o", str(exe)],
                   check=True, capture_output=True, text=True)
    rows = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    rows = [[int(x) for x in r.split()] for r in rows if r.strip()]
    assert len(rows) == 9
    up = lambda x: (x + 255) // 256 * 256  # noqa: E731
    for a, f, off, ln, out, status, total, w0, s0, h0, coff, cln, cout, cstatus, whole, sm, has, \
            ctotal in rows:
        want_off = up(a)
        want_len = up(want_off + 8 * f)
        want_out = up(want_len + 4 * f)
        want_status = up(want_out + 8 * f)
        want_total = up(want_status + 4 * f)
        assert (off, ln, out, status, total) == (want_off, want_len, want_out, want_status,
                                                 want_total), (a, f)
        assert (w0, s0, h0) == (0, 0, 0)
        assert (coff, cln, cout, cstatus) == (off, ln, out, status)
        assert whole >= status + 4 * f and sm >= whole + f and has >= sm + 32 * f
        assert ctotal >= has + f
        assert whole % 256 == 0 and sm % 256 == 0 and has % 256 == 0 and ctotal % 256 == 0


def test_python_names():
    from spacedrive_amd import cas, file_identifier as fi
    assert callable(cas.cas_checksum_batch_device)
    assert list(inspect.signature(cas.cas_checksum_batch_device).parameters)[:4] == \
        ["arena", "off", "length", "whole"]
    p = inspect.signature(fi.identify).parameters
    assert list(p) == ["paths", "sizes", "ctx", "checksums"] and p["checksums"].default is False
    import numpy as np
    r = fi.IdentifyResult(np.zeros((2, 8), np.uint8), np.ones(2, np.uint8), np.zeros(2, np.int32),
                          None)
    assert r.checksum32 is None and r.has_checksum is None and r.checksums() == [None, None]
    r = fi.IdentifyResult(r.cas8, r.has_key, r.status, None,
                          np.arange(64, dtype=np.uint8).reshape(2, 32), np.array([0, 1], np.uint8))
    assert r.checksums() == [None, bytes(range(32, 64)).hex()]
    assert inspect.signature(fi.FileIdentifierJob.__init__).parameters["checksums"].default is False
    assert inspect.signature(fi.shallow).parameters["checksums"].default is False


def test_file_paths_integrity_checksum_column_and_validator_query():
    from spacedrive_amd.file_identifier import FilePaths
    t = FilePaths()
    d = t.add(1, "/", "a", is_dir=True)
    f1 = t.add(1, "/", "x.bin")
    f2 = t.add(1, "/a/", "y.bin")
    f3 = t.add(1, "/a/b/", "z.bin")
    f4 = t.add(2, "/a/", "other_location.bin")
    assert t.integrity_checksum == [None] * 5
    assert t.unvalidated(1) == [f1, f2, f3] and d not in t.unvalidated(1)
    assert t.unvalidated(1, "a") == [f2, f3] and t.unvalidated(1, "/a/b/") == [f3]
    assert t.unvalidated(2) == [f4] and t.unvalidated(3) == []
    t.integrity_checksum[f2 - 1] = "00" * 32
    assert t.unvalidated(1) == [f1, f3] and t.unvalidated(1, "a") == [f3]


def test_rust_wrapper_calls_the_new_symbol():
    src = open(os.path.join(ROOT, "crates", "sd-core-gpu", "src", "identifier.rs")).read()
    assert "pub fn identify_with_checksums(" in src
    assert "sys::sdgpu_identify_checksum_files(" in src
    sysrs = open(os.path.join(ROOT, "crates", "sdgpu-sys", "src", "lib.rs")).read()
    for name in NEW:
        assert f"pub fn {name}(" in sysrs
