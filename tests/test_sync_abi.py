"""CPU: the sync ingest's entry points (include/sdgpu.h, "ABI 6, additive") are
exported, typed and bound, refuse bad arguments without a device, the header
still says ABI 6 and carries the citations, and the Rust crate wraps only
declared symbols."""
import ctypes
import os
import re
import subprocess
import sys

from spacedrive_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("sdgpu_oplog_create", "sdgpu_oplog_destroy", "sdgpu_oplog_clear", "sdgpu_oplog_stats",
         "sdgpu_oplog_add_device", "sdgpu_oplog_latest_device", "sdgpu_sync_ingest_device",
         "sdgpu_sync_ingest")


def _buf(n, ctype=ctypes.c_uint64):
    return ctypes.cast((ctype * n)(), ctypes.c_void_p)


def test_ingest_rejects_bad_arguments_without_device():
    lib = _native.load()
    dev, host = lib.sdgpu_sync_ingest_device, lib.sdgpu_sync_ingest
    log = ctypes.c_void_p(0x1000)      # never dereferenced: every case is refused first
    b = _buf(4)
    ok = dict(log=log, key=b, tag=b, ts=b, inst=b, n=4, clock=b, ni=4, flags=0, apply=b,
              applied=b, winner=b, counts=b)

    def both(**over):
        a = dict(ok, **over)
        args = tuple(a[k] for k in ("log", "key", "tag", "ts", "inst", "n", "clock", "ni", "flags",
                                    "apply", "applied", "winner", "counts"))
        x, y = dev(*args, None), host(*args)
        assert x == y
        return x

    assert both(log=None) == -22                                      # no log
    for name in ("key", "tag", "ts", "apply", "applied", "winner", "counts"):
        assert both(**{name: None}) == -22, name                      # a required pointer
    for n in (1 << 31, (1 << 64) - 1):
        assert both(n=n) == -22                                       # the limit
    for flags in (2, 3, 1 << 31):
        assert both(flags=flags) == -22                               # unknown flag bits
    assert both(inst=None) == -22 and both(clock=None) == -22         # exactly one of the two
    assert both(inst=None, n=0) == -22 and both(clock=None, n=0, ni=0) == -22


def test_log_calls_reject_bad_arguments_without_device():
    lib = _native.load()
    log, b = ctypes.c_void_p(0x1000), _buf(4)
    out = ctypes.c_void_p()
    assert lib.sdgpu_oplog_create(None, 0, ctypes.byref(out)) == -22
    assert lib.sdgpu_oplog_create(ctypes.c_void_p(0x1000), 0, None) == -22
    assert lib.sdgpu_oplog_create(ctypes.c_void_p(0x1000), (1 << 30) + 1, ctypes.byref(out)) == -22
    assert lib.sdgpu_oplog_destroy(None) == -22 and lib.sdgpu_oplog_clear(None, None) == -22
    assert lib.sdgpu_oplog_stats(None, (ctypes.c_uint64 * 2)()) == -22
    assert lib.sdgpu_oplog_stats(log, None) == -22
    assert lib.sdgpu_oplog_add_device(None, b, b, b, 4, None, None) == -22
    for args in ((None, b, b), (b, None, b), (b, b, None)):
        assert lib.sdgpu_oplog_add_device(log, *args, 4, None, None) == -22
    assert lib.sdgpu_oplog_add_device(log, b, b, b, 1 << 31, None, None) == -22
    assert lib.sdgpu_oplog_add_device(log, None, None, None, 0, None, None) == 0
    assert lib.sdgpu_oplog_latest_device(None, b, 4, b, b, None) == -22
    for args in ((None, 4, b, b), (b, 4, None, b), (b, 4, b, None), (b, 1 << 31, b, b)):
        assert lib.sdgpu_oplog_latest_device(log, *args, None) == -22
    assert lib.sdgpu_oplog_latest_device(log, None, 0, None, None, None) == 0


def test_host_variant_with_no_op_needs_no_device():
    lib = _native.load()
    counts = (ctypes.c_uint32 * 4)(7, 7, 7, 7)
    log = ctypes.c_void_p(0x1000)
    rc = lib.sdgpu_sync_ingest(log, None, None, None, None, 0, None, 0, 0, None, None, None,
                               ctypes.cast(counts, ctypes.c_void_p))
    assert rc == 0 and not any(counts)
    assert lib.sdgpu_sync_ingest(log, None, None, None, None, 0, None, 0, 1, None, None, None,
                                 None) == 0
    assert lib.sdgpu_sync_ingest_device(log, None, None, None, None, 0, None, 0, 0, None, None,
                                        None, None, None) == 0


def test_header_marks_the_additions():
    hdr = open(_native.HEADER_PATH).read()
    assert re.search(r"#define SDGPU_ABI_VERSION 6\b", hdr)
    assert re.search(r"#define SDGPU_INGEST_NO_COMMIT 1u\b", hdr)
    assert "typedef struct sdgpu_oplog sdgpu_oplog;" in hdr
    for name in NAMES:
        before = hdr[:hdr.index("int " + name + "(")]
        last = before[before.rindex("/*"):]
        assert "(ABI 6, additive)" in last, name
    assert set(NAMES) <= set(_native.declared_symbols())
    doc = hdr[hdr.index("sync ingest: which CRDT operations apply"):
              hdr.index("int " + NAMES[-1] + "(")]
    for cite in ("ingest.rs:114-160", "ingest.rs:188-233", "ingest.rs:67-71", "ingest.rs:162-186",
                 "ingest.rs:119-126,151", "ingest.rs:213-220", "schema.prisma:21-53",
                 "crdt.rs:9-23,34-36,67-69", "manager.rs:130-199", "403-431"):
        assert cite in doc, cite
    for word in ("SIGNED", "UNSIGNED", "INT64_MIN", "re-delivered"):
        assert word in doc, word


def test_symbols_are_exported_and_bound():
    lib = _native.load()
    for name in NAMES:
        assert getattr(lib, name).argtypes is not None, name
    assert len(lib.sdgpu_sync_ingest_device.argtypes) == 14
    assert len(lib.sdgpu_sync_ingest.argtypes) == 13
    assert len(lib.sdgpu_oplog_add_device.argtypes) == 7
    assert lib.sdgpu_abi_version() == 6


def test_rust_sys_is_regenerated_and_the_wrapper_uses_declared_names():
    gen = os.path.join(ROOT, "scripts", "gen_rust_sys.py")
    assert subprocess.run([sys.executable, gen, "--check"]).returncode == 0
    sysrs = open(os.path.join(ROOT, "crates", "sdgpu-sys", "src", "lib.rs")).read()
    assert "pub struct sdgpu_oplog { _private: [u8; 0] }" in sysrs
    assert "pub const SDGPU_INGEST_NO_COMMIT: u32 = 1;" in sysrs
    for name in NAMES:
        assert f"pub fn {name}(" in sysrs
    assert "log: *mut sdgpu_oplog" in sysrs and "out: *mut *mut sdgpu_oplog" in sysrs
    src = os.path.join(ROOT, "crates", "sd-core-gpu", "src")
    rs = open(os.path.join(src, "sync.rs")).read()
    used = set(re.findall(r"sys::(sdgpu_\w+)\(", rs))
    assert {"sdgpu_oplog_create", "sdgpu_oplog_destroy", "sdgpu_sync_ingest"} <= used
    assert used <= set(_native.declared_symbols()), used
    for const in re.findall(r"sys::(SDGPU_\w+)", rs):
        assert f"pub const {const}:" in sysrs, const
    assert re.search(r"\bpub mod sync\b", open(os.path.join(src, "lib.rs")).read())


def test_python_module_has_the_names():
    import spacedrive_amd
    from spacedrive_amd import sync as S
    for name in ("op_message", "op_keys", "OpLog", "CRDTOperation", "SharedOperation",
                 "RelationOperation", "Ingester", "ingest_host"):
        assert callable(getattr(S, name)), name
    for name in ("add", "latest", "ingest", "stats"):
        assert callable(getattr(S.OpLog, name)), name
    assert spacedrive_amd.sync is S and S.NO_COMMIT == 1
    assert "oracle" not in open(S.__file__).read()
    t = ("shared", "tag", b"[1]", "u:name")
    assert S.op_message(*t)[:1] != S.op_message(*t, tag=True)[:1]
    assert S.op_message(*t, salt=1) != S.op_message(*t, salt=2)
    # the id is length-prefixed: moving a byte between id and kind changes the message
    assert S.op_message("shared", "m", b"ab", "c") != S.op_message("shared", "m", b"a", "bc")
    op = S.CRDTOperation(None, 5, None, S.SharedOperation({"a": [1, 2]}, "tag", "u", "name", 1))
    assert (op.table, op.name, op.id_bytes, op.kind) == ("shared", "tag", b'{"a":[1,2]}', "u:name")
    assert S.RelationOperation(1, 2, "r", "d").kind() == "d"
