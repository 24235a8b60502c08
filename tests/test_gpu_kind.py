"""GPU: Object kinds from the bytes already staged for the cas_id.

* k_kind (sdgpu_kind_batch_device) against the step-by-step oracle
  (tests/kind_oracle.py) in both modes: the shared case list as packed cas
  messages, every extension id on random bodies of 0..48 bytes, the edge
  messages (lengths 0 and 7, misaligned, over-long, past the arena, a sampled
  one, a last message ending exactly at arena_bytes), n = 0 / 1 / 63 / 64 / 65
  / everything, a non-default stream, and the arena left untouched.
* identify_metadata over a directory of every category: cas ids, statuses and
  checksums exactly identify()'s; kinds the oracle's on the bytes read.
* the job: an Object carries its creator row's kind whatever the step size,
  also across an interrupt; without kinds nothing changes.
"""
import copy
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from spacedrive_amd import cas
from spacedrive_amd import kind as K
from tests import kind_oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAT_OF = {v: c for c, v in O.KIND.items()}


def _msg(content: bytes, size=None) -> bytes:
    return int(len(content) if size is None else size).to_bytes(8, "little") + content


def _build_batch():
    """(arena, off, len, ext, want[2]) on the host: the messages and the
    oracle's kinds in the two modes.  The LAST message ends exactly at the end
    of the arena and is 9 bytes long (one body byte, reachable only by a byte
    load)."""
    rng = np.random.default_rng(11)
    table = K.ext_table()
    msgs, exts, want = [], [], []

    def add(m, e, w0, w1):
        msgs.append(m)
        exts.append(e)
        want.append((w0, w1))

    # the shared case list, as whole-read messages
    cs = O.cases()
    ids = K.ext_ids([n for n, _ in cs])
    for (name, content), e in zip(cs, ids):
        add(_msg(content), int(e), O.resolve_conflicting(name, content, False),
            O.resolve_conflicting(name, content, True))
    # every id (and ids past the table) on random bodies of every short length
    for e in list(range(0, 216)) + [216, 217, 1000, 65535]:
        for _ in range(7):
            body = rng.integers(0, 256, int(rng.integers(0, 49)), dtype=np.uint8).tobytes()
            if 1 <= e <= 215:
                _, name, k0, k1 = table[e - 1]
                if k1:
                    w = [O.resolve_conflicting("f." + name, body, v) for v in (False, True)]
                else:
                    w = [O.resolve_known(CAT_OF[k0], name, body, v) for v in (False, True)]
            else:
                w = [0, 0]
            add(_msg(body), e, *w)
    first = {}
    for i, name, _, _ in table:
        first.setdefault(name, i)
    # shorter than the prefix: zero body bytes, whatever the bytes are
    for name in ("ts", "mts", "mjpeg", "jpg", "txt", "db"):
        for ln in (0, 7):
            w = [O.resolve_conflicting("f." + name, b"", v) for v in (False, True)]
            add(b"\x47" * ln, first[name], *w)
    # a sampled message (57 352 bytes): the header of a > 100 KiB file
    head = b"\x00\x01\x02\x47" + bytes(rng.integers(0, 256, cas.SAMPLED_MSG_LEN - 12, dtype=np.uint8))
    add(_msg(head, 400_000), first["mts"], 7, 7)
    add(_msg(head, 400_000), first["ts"], 20, 20)
    add(_msg(head, 400_000), first["png"], 5, 0)
    # the longest valid message
    add(_msg(b"\xff\xd8" + bytes(cas.MINIMUM_FILE_SIZE - 2)), first["jpg"], 5, 5)
    # the last one: 9 bytes, ending with the arena
    add(_msg(b"\x47"), first["ts"], 7, 7)
    off = np.zeros(len(msgs), np.uint64)
    pos = 0
    for i, m in enumerate(msgs):
        off[i] = pos
        pos += (len(m) + 15) // 16 * 16
    arena = np.zeros(int(off[-1]) + len(msgs[-1]), np.uint8)
    for o, m in zip(off, msgs):
        arena[int(o):int(o) + len(m)] = np.frombuffer(m, np.uint8)
    ln = np.array([len(m) for m in msgs], np.uint32)
    return arena, off, ln, np.array(exts, np.uint16), np.array(want, np.uint8)


@pytest.fixture(scope="module")
def batch():
    return _build_batch()


def _dev(batch):
    import torch
    arena, off, ln, ext, _ = batch
    return (torch.from_numpy(arena).cuda(), torch.from_numpy(off.view(np.int64)).cuda(),
            torch.from_numpy(ln.view(np.int32)).cuda(), torch.from_numpy(ext.view(np.int16)).cuda())


@pytest.mark.parametrize("verify", [False, True], ids=["default", "verify"])
def test_kind_batch_against_oracle(ctx, batch, verify):
    import torch
    d_arena, d_off, d_len, d_ext = _dev(batch)
    want = batch[4][:, 1 if verify else 0]
    n = len(want)
    assert n > 2900 and int(batch[1][-1]) + int(batch[2][-1]) == batch[0].size
    before = d_arena.clone()
    got = K.kind_batch_device(d_arena, d_off, d_len, d_ext, verify=verify, ctx=ctx)
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, [(int(i), int(batch[3][i]), int(batch[2][i]), int(got[i]), int(want[i]))
                           for i in bad[:10]]
    assert torch.equal(d_arena, before)
    # prefixes of the batch: one lane, one wave minus / exactly / plus one
    for m in (0, 1, 63, 64, 65):
        out = torch.full((max(m, 1) + 3,), 0xEE, dtype=torch.uint8, device="cuda")
        K.kind_batch_device(d_arena, d_off[:m], d_len[:m], d_ext[:m], verify=verify, out=out[:m],
                            ctx=ctx)
        torch.cuda.synchronize()
        o = out.cpu().numpy()
        assert np.array_equal(o[:m], want[:m]) and (o[m:] == 0xEE).all(), m


def test_invalid_messages_get_kind_0(ctx, batch):
    """A misaligned offset, an over-long message and one that ends past the
    arena: kind 0, exactly where sdgpu_cas_batch_device says -EINVAL."""
    import torch
    jpg = int(K.ext_ids(["a.jpg"])[0])
    room = 2 * ((cas.MAX_MSG_LEN + 15) // 16 * 16)   # 16-B aligned, and K1 slots to spare
    arena = torch.zeros(room + 48, dtype=torch.uint8, device="cuda")
    arena[8:10] = torch.tensor([0xFF, 0xD8], dtype=torch.uint8)          # message at 0
    arena[16 + 4 + 8:16 + 4 + 10] = torch.tensor([0xFF, 0xD8], dtype=torch.uint8)
    off = torch.tensor([0, 20, 0, room, room, 0], dtype=torch.int64, device="cuda")
    ln = torch.tensor([20, 20, cas.MAX_MSG_LEN + 1, 49, 48, cas.MAX_MSG_LEN], dtype=torch.int32,
                      device="cuda")
    ext = torch.tensor([jpg] * 6, dtype=torch.int16, device="cuda")
    for verify in (False, True):
        got = K.kind_batch_device(arena, off, ln, ext, verify=verify, ctx=ctx)
        _, st = cas.cas_batch_device(arena, off, ln, ctx=ctx)
        torch.cuda.synchronize()
        assert st.cpu().tolist() == [0, -22, -22, -22, 0, 0]
        # row 4 lies inside the arena but holds zeros: Image by name, nothing when verified
        assert got.cpu().tolist() == [5, 0, 0, 0, 0 if verify else 5, 5]


def test_non_default_stream_and_cas_on_the_same_arguments(ctx, batch):
    import torch
    d_arena, d_off, d_len, d_ext = _dev(batch)
    want = batch[4][:, 0]
    cas0, st0 = cas.cas_batch_device(d_arena, d_off, d_len, ctx=ctx)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        got = K.kind_batch_device(d_arena, d_off, d_len, d_ext, ctx=ctx, stream=s.cuda_stream)
        cas1, st1 = cas.cas_batch_device(d_arena, d_off, d_len, ctx=ctx, stream=s.cuda_stream)
    s.synchronize()
    assert np.array_equal(got.cpu().numpy(), want)
    assert torch.equal(cas0, cas1) and torch.equal(st0, st1) and int(st0.abs().sum()) == 0


# ---- identify_metadata over a directory ---------------------------------------------------

def _library(root):
    """paths, sizes passed, and what the call reads (bytes; None: the open
    fails; an int: the row fails with that status)."""
    rng = np.random.default_rng(23)
    os.makedirs(root, exist_ok=True)
    paths, sizes, reads = [], [], []

    def put(name, content, size=None, create=True):
        p = os.path.join(root, name)
        if create:
            with open(p, "wb") as f:
                f.write(content)
        paths.append(p)
        sizes.append(len(content) if size is None else size)
        return p

    k = 0
    for cat, name, alts in O.variants():
        for want_match in (True, False):
            body = bytearray(rng.integers(0, 256, int(rng.integers(1, 3000)), dtype=np.uint8).tobytes())
            if want_match and alts:
                pat, off = alts[int(rng.integers(0, len(alts)))]
                if len(body) < off + len(pat):
                    body += bytes(off + len(pat))
                for j, b in enumerate(pat):
                    if b is not None:
                        body[off + j] = b
            put(f"v{k:04d}.{name}", bytes(body))
            reads.append(bytes(body))
            k += 1
    for name in ("e0.ts", "e1.mts", "e2.jpg", "e3.mjpeg", "e4.txt", "e5", "e6.db", "e7.TS"):
        put(name, b"")
        reads.append(b"")
    big = b"\x00\x01\x02\x47" + O_bytes(rng, 150_000)
    put("big.mts", big)
    reads.append(big[:8192])
    put("big.ts", big)
    reads.append(big[:8192])
    put("big.png", big)
    reads.append(big[:8192])
    grown = b"\x47" + O_bytes(rng, 200_000)   # far past the room its stated size reserves
    put("grown.ts", grown, size=1000)
    reads.append(grown)
    inside = b"\xff\xd8" + O_bytes(rng, 3000)  # longer than stated, inside the reservation
    put("inside.jpg", inside, size=10)
    reads.append(inside)
    put("missing.jpg", b"", size=5, create=False)
    reads.append(-2)
    d = os.path.join(root, "dir.ts")
    os.makedirs(d)
    paths.append(d)
    sizes.append(10)
    reads.append(-21)
    put("missing0.jpg", b"", size=0, create=False)   # size 0: not read, the open for the kind fails
    reads.append(None)
    put("missing0", b"", size=0, create=False)       # no Extension: not even opened
    reads.append(None)
    return paths, np.array(sizes, np.uint64), reads


def O_bytes(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


def _want_kinds(paths, reads, verify):
    out = []
    for p, r in zip(paths, reads):
        if isinstance(r, int):
            out.append(0)
        else:
            out.append(O.resolve_conflicting(os.path.basename(p), r, verify))
    return out


@pytest.fixture(scope="module")
def library(tmp_path_factory):
    return _library(str(tmp_path_factory.mktemp("kinds") / "lib"))


@pytest.mark.parametrize("verify", [False, True], ids=["default", "verify"])
def test_identify_metadata_directory(ctx, library, verify):
    from spacedrive_amd import file_identifier as fi
    paths, sizes, reads = library
    assert 400 < len(paths) < 500
    plain = fi.identify(paths, sizes, ctx=ctx)
    want_status = [r if isinstance(r, int) else 0 for r in reads]
    assert plain.status.tolist() == want_status
    res = fi.identify_metadata(paths, sizes, ctx=ctx, verify_magic=verify)
    np.testing.assert_array_equal(res.cas8, plain.cas8)
    np.testing.assert_array_equal(res.has_key, plain.has_key)
    np.testing.assert_array_equal(res.status, plain.status)
    assert res.checksum32 is None and res.has_checksum is None
    want = _want_kinds(paths, reads, verify)
    got = res.kind.tolist()
    assert got == want, [(os.path.basename(p), g, w) for p, g, w in zip(paths, got, want) if g != w][:10]
    assert set(want) >= set(O.KIND.values())          # every category, and Unknown
    assert res.kinds()[-4:] == [None, None, K.ObjectKind.Unknown, K.ObjectKind.Unknown]
    by = {os.path.basename(p): g for p, g in zip(paths, got)}
    assert (by["e0.ts"], by["e1.mts"], by["big.mts"], by["big.ts"], by["grown.ts"]) == (20, 20, 7, 20, 7)
    assert by["e7.TS"] == 0 and by["inside.jpg"] == 5 and by["big.png"] == (0 if verify else 5)
    # with the body pass
    sums = fi.identify(paths, sizes, ctx=ctx, checksums=True)
    both = fi.identify_metadata(paths, sizes, ctx=ctx, checksums=True, verify_magic=verify)
    for a, b in ((both.cas8, sums.cas8), (both.has_key, sums.has_key), (both.status, sums.status),
                 (both.checksum32, sums.checksum32), (both.has_checksum, sums.has_checksum)):
        np.testing.assert_array_equal(a, b)
    assert both.kind.tolist() == want and int(sums.has_checksum.sum()) > 400
    # sizes stat-ed by the library: the stale sizes are gone, the directory is -EISDIR
    fresh = fi.identify_metadata(paths, None, ctx=ctx, verify_magic=verify)
    ref = fi.identify(paths, None, ctx=ctx)
    np.testing.assert_array_equal(fresh.cas8, ref.cas8)
    np.testing.assert_array_equal(fresh.status, ref.status)
    ok = fresh.status == 0
    assert ok.sum() == len(paths) - 4 and not fresh.kind[~ok].any()
    want_fresh = [O.resolve_conflicting(os.path.basename(p), open(p, "rb").read(48), verify)
                  if o else 0 for p, o in zip(paths, ok)]
    assert fresh.kind.tolist() == want_fresh


_IO_CHILD = r'''
import json, sys
sys.path.insert(0, sys.argv[1])
import numpy as np
from spacedrive_amd import file_identifier as fi
from spacedrive_amd._native import Context
job = json.load(sys.stdin)
ctx = Context(0)
sizes = np.array(job["sizes"], np.uint64)
out = {}
plain = fi.identify(job["paths"], sizes, ctx=ctx)
out["cas"] = [bytes(c).hex() for c in plain.cas8]
out["status"] = [int(s) for s in plain.status]
for verify in (False, True):
    r = fi.identify_metadata(job["paths"], sizes, ctx=ctx, verify_magic=verify)
    assert [bytes(c).hex() for c in r.cas8] == out["cas"]
    assert [int(s) for s in r.status] == out["status"]
    assert r.has_key.tolist() == plain.has_key.tolist()
    out["kind%d" % verify] = [int(k) for k in r.kind]
print(json.dumps(out))
'''


@pytest.mark.parametrize("io", ["pread", "uring", "bounce"])
def test_identify_metadata_readers_agree(io, library):
    """The three staging readers, in a fresh process each (SDGPU_IO is read when
    the context opens): the same cas ids and statuses as identify(), the
    oracle's kinds in both modes."""
    paths, sizes, reads = library
    env = dict(os.environ)
    env.pop("SDGPU_IO", None)
    if io != "bounce":
        env["SDGPU_IO"] = io
    p = subprocess.run([sys.executable, "-c", _IO_CHILD, ROOT],
                       input=json.dumps({"paths": paths, "sizes": [int(s) for s in sizes]}),
                       capture_output=True, text=True, timeout=120, env=env)
    assert p.returncode == 0, p.stderr[-3000:]
    res = json.loads(p.stdout.strip().splitlines()[-1])
    assert res["status"] == [r if isinstance(r, int) else 0 for r in reads]
    assert res["kind0"] == _want_kinds(paths, reads, False)
    assert res["kind1"] == _want_kinds(paths, reads, True)


# ---- the job ---------------------------------------------------------------------------------

def _job_library(root):
    from spacedrive_amd.file_identifier import FilePaths
    rng = np.random.default_rng(31)
    loc = os.path.join(root, "loc")
    os.makedirs(loc)
    t = FilePaths()
    exts = ["jpg", "bin", "ts", "txt", "pdf", "zip", "", "mts", "rs", "db"]
    jpg = b"\xff\xd8" + O_bytes(rng, 700)
    other = O_bytes(rng, 900)
    content = {}
    for i in range(250):
        name = f"f{i:03d}" + ("." + exts[i % len(exts)] if exts[i % len(exts)] else "")
        data = (b"\x47" if i % 4 == 0 else b"\x00") + O_bytes(rng, int(rng.integers(0, 2000)))
        if i % 17 == 0:
            data = b""
        # duplicates with different names: the first row creates the Object
        name, data = {3: ("a.jpg", jpg), 5: ("b.bin", jpg), 150: ("c.bin", jpg),
                      7: ("d.bin", other), 160: ("e.png", other)}.get(i, (name, data))
        t.add(1, "/", name)
        content[name] = data
        if i == 11:
            continue  # no file: the row stays an orphan
        with open(os.path.join(loc, name), "wb") as f:
            f.write(data)
    return t, loc, content


def _check_object_kinds(t, content):
    creator = {}
    for i, obj in enumerate(t.object_id):   # ascending id: the first row of an Object created it
        if obj is not None:
            creator.setdefault(obj, t.name[i])
    assert set(t.object_kind) == set(creator)
    for obj, name in creator.items():
        assert t.object_kind[obj] == O.resolve_conflicting(name, content[name], False), name


def test_job_records_the_creators_kind(ctx, tmp_path):
    from spacedrive_amd import file_identifier as fi
    t0, loc, content = _job_library(str(tmp_path))
    tables = {}
    for cps in (1, 64):
        t = copy.deepcopy(t0)
        job = fi.FileIdentifierJob(t, 1, loc, chunks_per_step=cps, ctx=ctx, kinds=True).init()
        job.run()
        job.close()
        _check_object_kinds(t, content)
        tables[cps] = t
    t = tables[1]
    assert tables[64].object_kind == t.object_kind and tables[64].object_id == t.object_id
    row = {n: i for i, n in enumerate(t.name)}
    # a.jpg and b.bin share a chunk (an Object each); c.bin links to a.jpg's Object
    obj = t.object_id[row["c.bin"]]
    assert obj == t.object_id[row["a.jpg"]] != t.object_id[row["b.bin"]]
    assert t.object_kind[obj] == K.ObjectKind.Image
    assert t.object_kind[t.object_id[row["b.bin"]]] == K.ObjectKind.Unknown
    # e.png links to d.bin's Object, which stays Unknown
    assert t.object_id[row["e.png"]] == t.object_id[row["d.bin"]]
    assert t.object_kind[t.object_id[row["d.bin"]]] == K.ObjectKind.Unknown
    assert t.object_id[11] is None
    # interrupted after one step, resumed through its JSON state
    tr = copy.deepcopy(t0)
    j1 = fi.FileIdentifierJob(tr, 1, loc, chunks_per_step=1, ctx=ctx, kinds=True).init()
    j1.run(max_steps=1)
    state = json.loads(json.dumps(j1.state()))
    j1.close()
    assert state["kinds"] is True and 0 < len(tr.object_kind) < len(t.object_kind)
    j2 = fi.FileIdentifierJob.resume(tr, state, ctx=ctx)
    assert j2.kinds is True
    j2.run()
    j2.close()
    assert tr.object_kind == t.object_kind and tr.object_id == t.object_id
    # without kinds: exactly today's job
    tp = copy.deepcopy(t0)
    jp = fi.FileIdentifierJob(tp, 1, loc, chunks_per_step=1, ctx=ctx).init()
    meta = jp.run()
    jp.close()
    assert tp.object_kind == {} and jp.kinds is False and jp.state()["kinds"] is False
    assert (tp.cas_id, tp.object_id, tp.integrity_checksum) == (t.cas_id, t.object_id,
                                                                 t.integrity_checksum)
    assert meta.total_objects_created == len(t.object_kind)
    state.pop("kinds")
    old = fi.FileIdentifierJob.resume(copy.deepcopy(tr), state, ctx=ctx)
    assert old.kinds is False
    old.close()
    # shallow passes the flag on
    ts = copy.deepcopy(t0)
    fi.shallow(ts, 1, loc, ctx=ctx, kinds=True)
    assert ts.object_kind == t.object_kind


def test_file_metadata_returns_the_kind(ctx, tmp_path):
    from spacedrive_amd import file_identifier as fi
    for name, data in (("v.ts", b"\x47" + bytes(20)), ("c.ts", b"export {}\n"), ("p.JPG", b"\x00" * 9),
                       ("plain", b"abc"), ("e.mts", b"")):
        (tmp_path / name).write_bytes(data)
        m = fi.file_metadata(str(tmp_path), name, ctx)
        assert m.kind == O.resolve_conflicting(name, data, False), name
        assert (m.cas_id is None) == (len(data) == 0) and m.size == len(data)
