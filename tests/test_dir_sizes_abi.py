"""CPU: the directory-size entry points (include/sdgpu.h, "ABI 6, additive") are
exported, typed and bound, refuse bad arguments without a device, the header
still says ABI 6, and the Rust crate wraps only declared symbols."""
import ctypes
import os
import re

from spacedrive_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("sdgpu_dir_sizes_device", "sdgpu_dir_sizes")
EINVAL, E2BIG = -22, -7


def _buf(n, ctype=ctypes.c_uint64):
    return ctypes.cast((ctype * n)(), ctypes.c_void_p)


def test_entry_points_reject_bad_arguments_without_device():
    lib = _native.load()
    dev, host = lib.sdgpu_dir_sizes_device, lib.sdgpu_dir_sizes
    ctx = ctypes.c_void_p(0x1000)      # never dereferenced: every case is refused first
    k, o = _buf(4), _buf(4)
    ok = dict(c=ctx, dk=k, sk=k, fl=k, sz=k, n=4, parent=o, total=o, files=o, counts=o)

    def both(**over):
        a = dict(ok, **over)
        args = (a["c"], a["dk"], a["sk"], a["fl"], a["sz"], a["n"], a["parent"], a["total"],
                a["files"], a["counts"])
        x, y = dev(*args, None), host(*args)
        assert x == y
        return x

    assert both(c=None) == EINVAL                                  # no context
    for name in ("dk", "sz", "parent", "total", "counts"):         # required with rows
        assert both(**{name: None}) == EINVAL, name
    assert both(sk=None) == EINVAL                                 # flags without self keys
    assert both(n=0, counts=None) == EINVAL                        # the counts are always written
    assert both(n=(1 << 31) + 1) == E2BIG                          # the limit
    assert both(n=(1 << 64) - 1) == E2BIG
    assert both(n=(1 << 31) + 1, c=None) == EINVAL
    assert both(n=(1 << 31) + 1, counts=None) == EINVAL


def test_host_variant_with_nothing_needs_no_device():
    """n_r == 0: the four counts are 0, decided on the host."""
    lib = _native.load()
    counts = (ctypes.c_uint64 * 4)(7, 7, 7, 7)
    rc = lib.sdgpu_dir_sizes(ctypes.c_void_p(0x1000), None, None, None, None, 0, None, None, None,
                             ctypes.cast(counts, ctypes.c_void_p))
    assert rc == 0 and not any(counts)


def test_header_marks_the_additions():
    hdr = open(_native.HEADER_PATH).read()
    assert re.search(r"#define SDGPU_ABI_VERSION 6\b", hdr)
    assert re.search(r"#define SDGPU_SIZE_UNRESOLVED 0xFFFFFFFFFFFFFFFFull\b", hdr)
    for name in NAMES:
        before = hdr[:hdr.index("int " + name + "(")]
        last = before[before.rindex("/*"):]
        assert "(ABI 6, additive)" in last, name
    assert set(NAMES) <= set(_native.declared_symbols())
    doc = hdr[hdr.index("Recursive directory sizes"):hdr.index("int " + NAMES[0] + "(")]
    for cite in ("mod.rs:126-136, 215-225", "api/search.rs:85", "api/locations.rs:66-100",
                 "SDGPU_IDX_MISS", "-E2BIG", "modulo 2^64"):
        assert cite in doc, cite


def test_symbols_are_exported_and_bound():
    lib = _native.load()
    for name in NAMES:
        assert getattr(lib, name).argtypes is not None, name
    assert len(lib.sdgpu_dir_sizes_device.argtypes) == 11
    assert len(lib.sdgpu_dir_sizes.argtypes) == 10
    assert lib.sdgpu_abi_version() == 6


def test_rust_names_the_wrapper():
    src = os.path.join(ROOT, "crates", "sd-core-gpu", "src")
    rs = open(os.path.join(src, "dir_sizes.rs")).read()
    assert re.search(r"pub fn dir_sizes\(", rs) and re.search(r"pub struct Rows<", rs)
    for fld in ("dir_keys", "self_keys", "flags", "sizes"):
        assert re.search(r"pub %s:" % fld, rs), fld
    assert "sys::sdgpu_dir_sizes(" in rs
    used = set(re.findall(r"sys::(sdgpu_\w+)\(", rs))
    assert used and used <= set(_native.declared_symbols()), used
    assert re.search(r"\bpub mod dir_sizes\b", open(os.path.join(src, "lib.rs")).read())
    sysrs = open(os.path.join(ROOT, "crates", "sdgpu-sys", "src", "lib.rs")).read()
    assert "pub const SDGPU_SIZE_UNRESOLVED: u64 = 0xFFFFFFFFFFFFFFFF;" in sysrs
    for name in NAMES:
        assert f"pub fn {name}(" in sysrs
    for const in re.findall(r"sys::(SDGPU_\w+)", rs):
        assert f"pub const {const}:" in sysrs, const


def test_python_module_has_the_names():
    import spacedrive_amd
    from spacedrive_amd import dir_sizes as D
    for name in ("sizes", "sizes_host", "sizes_oracle", "self_keys", "location_sizes"):
        assert callable(getattr(D, name)), name
    assert spacedrive_amd.dir_sizes is D
    text = open(D.__file__).read()
    assert "from oracle" not in text and "import oracle" not in text
    assert (D.MISS, D.UNRESOLVED) == (0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF)
