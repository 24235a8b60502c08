"""CPU: the indexer diff's entry points (include/sdgpu.h, "ABI 6, additive") are
exported, typed and bound, refuse bad arguments without a device, the header
still says ABI 6, and the Rust crate wraps only declared symbols."""
import ctypes
import os
import re

from spacedrive_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("sdgpu_indexer_diff_device", "sdgpu_indexer_diff")


def _buf(n, ctype=ctypes.c_uint64):
    return ctypes.cast((ctype * n)(), ctypes.c_void_p)


def test_entry_points_reject_bad_arguments_without_device():
    lib = _native.load()
    dev, host = lib.sdgpu_indexer_diff_device, lib.sdgpu_indexer_diff
    ctx = ctypes.c_void_p(0x1000)      # never dereferenced: every case is refused first
    k, m, o = _buf(4), _buf(12), _buf(4)
    ok = dict(c=ctx, wk=k, wm=m, nw=4, dk=k, nd=4, rk=k, rd=k, rm=m, nr=4, match=o, state=o,
              create=o, update=o, remove=o, counts=o)

    def both(**over):
        a = dict(ok, **over)
        args = (a["c"], a["wk"], None, a["wm"], a["nw"], a["dk"], a["nd"], a["rk"], a["rd"], None,
                a["rm"], a["nr"], a["match"], a["state"], a["create"], a["update"], a["remove"],
                a["counts"])
        x, y = dev(*args, None), host(*args)
        assert x == y
        return x

    assert both(c=None) == -22                                   # no context
    for name in ("wk", "wm", "dk", "rk", "rd", "rm"):            # a required input
        assert both(**{name: None}) == -22, name
    for name in ("match", "state", "counts", "create", "update", "remove"):
        assert both(**{name: None}) == -22, name
    for name in ("nw", "nd", "nr"):                              # the limits
        assert both(**{name: 1 << 31}) == -22, name
        assert both(**{name: (1 << 64) - 1}) == -22, name
    # NULL counts, match or state with n_w > 0, whatever the other counts are
    for name in ("match", "state", "counts"):
        assert both(nd=0, nr=0, dk=None, rk=None, rd=None, rm=None, remove=None,
                    **{name: None}) == -22, name
    assert both(nw=0, nd=0, wk=None, wm=None, dk=None, match=None, state=None, create=None,
                update=None, remove=None) == -22                 # rows without a remove list
    assert both(nw=0, nr=0, counts=None) == -22                  # any count needs counts


def test_host_variant_with_nothing_needs_no_device():
    """n_w == n_r == 0: three empty lists, decided on the host."""
    lib = _native.load()
    counts = (ctypes.c_uint32 * 4)(7, 7, 7, 7)
    k = _buf(4)
    rc = lib.sdgpu_indexer_diff(ctypes.c_void_p(0x1000), None, None, None, 0, k, 4, None, None,
                                None, None, 0, None, None, None, None, None,
                                ctypes.cast(counts, ctypes.c_void_p))
    assert rc == 0 and not any(counts)
    args = (ctypes.c_void_p(0x1000), None, None, None, 0, None, 0, None, None, None, None, 0,
            None, None, None, None, None, None)
    assert lib.sdgpu_indexer_diff(*args) == 0
    assert lib.sdgpu_indexer_diff_device(*args, None) == 0


def test_header_marks_the_additions():
    hdr = open(_native.HEADER_PATH).read()
    assert re.search(r"#define SDGPU_ABI_VERSION 6\b", hdr)
    assert re.search(r"#define SDGPU_IDX_ANCESTOR 2u\b", hdr)
    assert re.search(r"#define SDGPU_IDX_NO_METADATA 2u\b", hdr)
    assert re.search(r"#define SDGPU_IDX_MISS 0xFFFFFFFFu\b", hdr)
    for name in NAMES:
        before = hdr[:hdr.index("int " + name + "(")]
        last = before[before.rindex("/*"):]
        assert "(ABI 6, additive)" in last, name
    assert set(NAMES) <= set(_native.declared_symbols())
    doc = hdr[hdr.index("Indexer rescan diff"):hdr.index("int " + NAMES[0] + "(")]
    for cite in ("walk.rs:\n * 309-381", ":624-636", "indexer/mod.rs:305-331", ":338-388",
                 "indexer/mod.rs:207-215", "isolated_file_path_data.rs:150-158",
                 "isolated_file_path_data.rs:\n *                  25-38", "walk.rs:560-617",
                 "walk.rs:349-354", "walk.rs:360-364"):
        assert cite in doc, cite


def test_symbols_are_exported_and_bound():
    lib = _native.load()
    for name in NAMES:
        assert getattr(lib, name).argtypes is not None, name
    assert len(lib.sdgpu_indexer_diff_device.argtypes) == 19
    assert len(lib.sdgpu_indexer_diff.argtypes) == 18
    assert lib.sdgpu_abi_version() == 6


def test_rust_names_the_wrapper():
    src = os.path.join(ROOT, "crates", "sd-core-gpu", "src")
    rs = open(os.path.join(src, "indexer.rs")).read()
    assert re.search(r"pub fn diff\(", rs)
    assert "sys::sdgpu_indexer_diff(" in rs
    used = set(re.findall(r"sys::(sdgpu_\w+)\(", rs))
    assert used and used <= set(_native.declared_symbols()), used
    assert re.search(r"\bpub mod indexer\b", open(os.path.join(src, "lib.rs")).read())
    sysrs = open(os.path.join(ROOT, "crates", "sdgpu-sys", "src", "lib.rs")).read()
    for const in ("SDGPU_IDX_ANCESTOR: u32 = 2;", "SDGPU_IDX_NO_METADATA: u32 = 2;",
                  "SDGPU_IDX_MISS: u32 = 0xFFFFFFFF;"):
        assert "pub const " + const in sysrs, const
    for name in NAMES:
        assert f"pub fn {name}(" in sysrs
    for const in re.findall(r"sys::(SDGPU_\w+)", rs):
        assert f"pub const {const}:" in sysrs, const


# strict and reserved keywords of Rust 2021 (the reference: "Keywords"); a
# parameter named like one is a parse error for the whole sys crate
RUST_KEYWORDS = frozenset("""as break const continue crate else enum extern false fn for if impl in
let loop match mod move mut pub ref return self Self static struct super trait true type unsafe use
where while async await dyn abstract become box do final macro override priv typeof unsized virtual
yield try""".split())


def test_no_generated_parameter_is_a_rust_keyword():
    """scripts/gen_rust_sys.py copies the header's parameter names: none of them,
    in any declaration of the sys crate, may be a Rust keyword."""
    sysrs = open(os.path.join(ROOT, "crates", "sdgpu-sys", "src", "lib.rs")).read()
    fns = re.findall(r"pub fn (\w+)\(([^)]*)\)", sysrs)
    assert len(fns) > 50 and {n for n, _ in fns} >= set(NAMES)
    seen = 0
    for name, params in fns:
        for p in filter(None, (x.strip() for x in params.split(","))):
            ident = p.split(":")[0].strip()
            assert re.fullmatch(r"[A-Za-z_]\w*", ident), (name, p)
            assert ident not in RUST_KEYWORDS, (name, ident)
            seen += 1
    assert seen > 300
    host = dict(fns)["sdgpu_indexer_diff"]
    assert "matched: *mut u32" in host and "state: *mut u8" in host


def test_python_module_has_the_names():
    import spacedrive_amd
    from spacedrive_amd import indexer as X
    for name in ("path_keys", "dir_keys", "diff", "diff_host", "scan", "rescan", "apply",
                 "LocationIndex"):
        assert callable(getattr(X, name)), name
    assert spacedrive_amd.indexer is X
    assert "oracle" not in open(X.__file__).read()
    assert (X.ANCESTOR, X.NO_METADATA, X.MISS) == (2, 2, 0xFFFFFFFF)


def test_name_split_follows_the_reference():
    """separate_name_and_extension_from_str (isolated_file_path_data.rs:160-180)."""
    from spacedrive_amd.indexer import split_name
    for full, want in (("a.txt", ("a", "txt")), (".hidden", (".hidden", "")),
                       ("noext", ("noext", "")), ("x.tar.gz", ("x.tar", "gz")),
                       ("trailing.", ("trailing", "")), (".a.b", (".a", "b"))):
        assert split_name(full, False) == want, full
    assert split_name("dir.d", True) == ("dir.d", "")


def test_scan_marks_ancestors_and_walked_directories(tmp_path):
    from spacedrive_amd import indexer as X
    for p in ("keep/a.txt", "skip/b.txt", "pass/deep/c.txt", "pass/d.bin", "empty_pass/x.bin"):
        f = tmp_path / p
        f.parent.mkdir(parents=True, exist_ok=True)
        f.write_bytes(b"x")

    def accept(rel, is_dir):
        if rel == "skip" or rel.endswith(".bin"):
            return False
        return X.WALK_ONLY if rel in ("pass", "empty_pass") else True

    w = X.scan(tmp_path, accept)
    got = {(e.materialized_path, e.name, e.extension, e.is_dir, e.ancestor) for e in w.entries}
    assert got == {("/", "keep", "", True, False), ("/keep/", "a", "txt", False, False),
                   ("/", "pass", "", True, True), ("/pass/", "deep", "", True, False),
                   ("/pass/deep/", "c", "txt", False, False)}
    assert w.dirs == ["/", "/empty_pass/", "/keep/", "/pass/", "/pass/deep/"]
    st = os.stat(tmp_path / "keep" / "a.txt")
    e = next(e for e in w.entries if e.name == "a")
    assert (e.inode, e.device, e.modified_at) == (st.st_ino, st.st_dev, st.st_mtime_ns)


def test_location_index_columns():
    from spacedrive_amd.indexer import LocationIndex
    t = LocationIndex()
    a = t.add("/", "a", "txt", False, 1, 2, 3)
    b = t.add("/", "b", "", True)
    assert (a, b) == (1, 2) and len(t) == 2
    assert t.add("/", "a", "txt", True, skip_duplicates=True) is None
    t.remove([a])
    assert t.id == [2] and t.tuples() == [("/", "b", "")]
    assert t.add("/", "c", "", False) == 3                        # ids are never reused
    t.set_metadata(3, 7, 8, 9)
    assert t.rows()[-1] == (3, "/", "c", "", False, 7, 8, 9)
    # a removed tuple can come back, and ids still find their rows after removals
    assert t.add("/", "a", "txt", False, skip_duplicates=True) == 4
    assert t.add("/", "a", "txt", False, skip_duplicates=True) is None
    ids = [t.add("/big/", "f%d" % i, "", False, skip_duplicates=True) for i in range(20_000)]
    t.remove(ids[::2] + [2])
    t.set_metadata(ids[-1], 1, 2, 3)
    assert t.rows()[-1][0] == ids[-1] and t.rows()[-1][5:] == (1, 2, 3)
    assert len(t) == 2 + 10_000 and t.add("/big/", "f1", "", False, skip_duplicates=True) is None
    assert t.add("/big/", "f0", "", False, skip_duplicates=True) == ids[-1] + 1
