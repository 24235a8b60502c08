"""GPU: the identifier call that also returns the integrity_checksum of every
file it read whole -- K1's body pass (sdgpu_cas_checksum_batch_device), the
path call (sdgpu_identify_checksum_files) and the job that writes the column.
Every digest is compared bit for bit with the oracle's BLAKE3 / file_checksum,
every cas id and status with the call that returns no checksums."""
import json
import os

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

WHOLE_MAX = 100 * 1024


def _pack(lens, align=16):
    """16-B aligned offsets of messages of the given lengths, and the bytes used."""
    off = np.zeros(len(lens), np.uint64)
    pos = 0
    for i, n in enumerate(lens):
        off[i] = pos
        pos += (int(n) + align - 1) // align * align
    return off, pos


def _device_call(ctx, host, off, ln, whole, stream=None):
    """(out8, out32, has_checksum, status) as numpy, after a synchronise."""
    import torch
    from spacedrive_amd import cas
    arena = torch.from_numpy(host).cuda()
    d_off = torch.from_numpy(np.asarray(off, np.uint64).view(np.int64).copy()).cuda()
    d_len = torch.from_numpy(np.asarray(ln, np.uint32).view(np.int32).copy()).cuda()
    d_whole = torch.from_numpy(np.asarray(whole, np.uint8).copy()).cuda()
    r = cas.cas_checksum_batch_device(arena, d_off, d_len, d_whole, ctx=ctx, stream=stream)
    torch.cuda.synchronize()
    return (arena, d_off, d_len), tuple(x.cpu().numpy() for x in r)


def _check_bodies(ctx, host, off, ln):
    """Every message whole: digests against the oracle, cas ids and statuses
    against sdgpu_cas_batch_device on the same arguments.  A message longer
    than a cas message can be (8 + 100 KiB) is -EINVAL with both outputs zero."""
    import torch
    from spacedrive_amd import cas
    dev, (out8, out32, has, st) = _device_call(ctx, host, off, ln, np.ones(len(ln), np.uint8))
    ref8, ref_st = cas.cas_batch_device(*dev, ctx=ctx)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(st, ref_st.cpu().numpy())
    valid = np.asarray(ln) <= 8 + WHOLE_MAX
    assert st.tolist() == [0 if v else -22 for v in valid]
    np.testing.assert_array_equal(out8, ref8.cpu().numpy())
    np.testing.assert_array_equal(out8[valid], O.cas_batch(host, off[valid], ln[valid], threads=8))
    assert has.tolist() == [1 if v else 0 for v in valid]
    assert not out8[~valid].any() and not out32[~valid].any()
    bad = [int(ln[i]) - 8 for i in range(len(ln)) if valid[i] and
           bytes(out32[i]) != O.blake3(host[int(off[i]) + 8:int(off[i]) + int(ln[i])])]
    assert not bad, f"{len(bad)} wrong body digests, first body lengths {bad[:8]}"


def test_body_lengths_0_to_3100(ctx):
    """One message per body length 0..3100 (every block and chunk tail of the
    ragged path), 16-B aligned offsets, every message flagged whole."""
    ln = np.arange(0, 3101, dtype=np.uint32) + 8
    off, total = _pack(ln)
    host = np.random.default_rng(11).integers(0, 256, total, dtype=np.uint8)
    _check_bodies(ctx, host, off, ln)


def test_message_and_body_on_different_sides_of_a_boundary(ctx):
    """Body lengths where the unit count, the chunk count or the last block's
    length differ between the cas message and its body (L = 4096: five message
    chunks with one unit, four body chunks with none), the largest body, and a
    last message that ends exactly at arena_bytes with L a multiple of 1024.
    L = 4096 * 25 + 1 is one byte more than a whole-read file can hold: that
    message is rejected, by both calls alike."""
    ls = list(range(1015, 1026)) + [102400]
    for k in range(1, 26):
        ls += [4096 * k + d for d in (-9, -8, -7, -1, 0, 1)]
    ls.append(5 * 1024)  # the message at the very end of the arena
    ln = np.array(ls, np.uint32) + 8
    off, _ = _pack(ln)
    total = int(off[-1]) + int(ln[-1])  # no padding behind the last message
    assert (int(ln[-1]) - 8) % 1024 == 0
    host = np.random.default_rng(12).integers(0, 256, total, dtype=np.uint8)
    _check_bodies(ctx, host, off, ln)


def test_mixed_flags_invalid_messages_and_capacity(ctx):
    rng = np.random.default_rng(13)
    # alternating flags over sampled-length and short messages, then a whole
    # message of length 0 and of length 7 (no room for the prefix)
    ln = [57352, 57352, 100, 100, 57352, 3000, 57352, 8 + 4096, 0, 7]
    whole = [0, 1, 0, 1, 1, 0, 0, 1, 1, 1]
    off, total = _pack(ln)
    # a misaligned offset and an over-long message
    off = np.concatenate([off, np.array([8, 0], np.uint64)])
    ln = np.array(ln + [100, 102409], np.uint32)
    whole = np.array(whole + [1, 1], np.uint8)
    host = rng.integers(0, 256, max(total, 102416), dtype=np.uint8)
    dev, (out8, out32, has, st) = _device_call(ctx, host, off, ln, whole)
    assert st.tolist() == [0] * 10 + [-22, -22]
    import torch
    from spacedrive_amd import cas
    ref8, _ = cas.cas_batch_device(*dev, ctx=ctx)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out8, ref8.cpu().numpy())
    np.testing.assert_array_equal(
        out8[:10], O.cas_batch(host, off[:10], ln[:10], threads=4))  # len 0 and 7 keep their id
    assert has.tolist() == [0, 1, 0, 1, 1, 0, 0, 1, 0, 0, 0, 0]
    for i in range(ln.size):
        if has[i]:
            o = int(off[i])
            assert bytes(out32[i]) == O.blake3(host[o + 8:o + int(ln[i])]), i
        else:
            assert not out32[i].any(), i
    assert not out8[10:].any()
    # the shape of test_device_api_workspace_guards: 2000 copies of one 100 KiB
    # message in a 128 KiB arena, far beyond arena_bytes / 1024 + n CV slots
    n = 2000
    _, (o8, o32, h, s) = _device_call(ctx, host[:128 << 10].copy(), np.zeros(n, np.uint64),
                                      np.full(n, 102408, np.uint32), np.ones(n, np.uint8))
    assert set(s.tolist()) == {-105}  # -ENOBUFS
    assert not o8.any() and not o32.any() and not h.any()
    # the context still works afterwards
    _, (o8b, o32b, hb, sb) = _device_call(ctx, host, off, ln, whole)
    np.testing.assert_array_equal(o32b, out32)
    np.testing.assert_array_equal(o8b, out8)
    assert hb.tolist() == has.tolist() and sb.tolist() == st.tolist()


def test_two_streams_share_the_workspace(ctx):
    """Two calls back to back on different streams of one context, different
    arenas: the second waits for the first (both passes use one workspace)."""
    import torch
    from spacedrive_amd import cas
    rng = np.random.default_rng(14)
    jobs = []
    for seed in (0, 1):
        ln = rng.integers(8, 60_000, 400).astype(np.uint32)
        off, total = _pack(ln)
        host = rng.integers(0, 256, total, dtype=np.uint8)
        whole = (rng.random(ln.size) < 0.7).astype(np.uint8)
        t = (torch.from_numpy(host).cuda(),
             torch.from_numpy(off.view(np.int64).copy()).cuda(),
             torch.from_numpy(ln.view(np.int32).copy()).cuda(),
             torch.from_numpy(whole).cuda())
        jobs.append((host, off, ln, whole, t))
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    res = [cas.cas_checksum_batch_device(*j[4], ctx=ctx, stream=s.cuda_stream)
           for j, s in zip(jobs, streams)]
    torch.cuda.synchronize()
    for (host, off, ln, whole, _), r in zip(jobs, res):
        out8, out32, has, st = (x.cpu().numpy() for x in r)
        assert not st.any()
        np.testing.assert_array_equal(out8, O.cas_batch(host, off, ln, threads=8))
        np.testing.assert_array_equal(has, whole)
        for i in range(ln.size):
            o = int(off[i])
            want = O.blake3(host[o + 8:o + int(ln[i])]) if whole[i] else bytes(32)
            assert bytes(out32[i]) == want, i


# ---- the path call -----------------------------------------------------------------

@pytest.fixture(scope="module")
def boundary_files(tmp_path_factory):
    """One file per corpus.boundary_sizes() entry up to 131072 bytes, a missing
    path and a directory; the oracle's checksum of every file."""
    from spacedrive_amd import corpus
    root = tmp_path_factory.mktemp("idsum")
    sizes = [s for s in corpus.boundary_sizes() if s <= 131072]
    paths = []
    for i, s in enumerate(sizes):
        p = root / f"b{i:02d}.bin"
        p.write_bytes(O.synth_file_bytes(500 + i, 0, s))
        paths.append(str(p))
    sums = [O.file_checksum_path(p) for p in paths]
    return paths + [str(root / "missing"), str(root)], sizes + [10, 10], sums


def _check_path_result(res, plain, sizes, sums, rows):
    """res = identify(checksums=True) over the rows `rows` of the fixture,
    plain = identify() over the same rows."""
    np.testing.assert_array_equal(res.cas8, plain.cas8)
    np.testing.assert_array_equal(res.has_key, plain.has_key)
    np.testing.assert_array_equal(res.status, plain.status)
    got = res.checksums()
    for j, i in enumerate(rows):
        want = i < len(sums) and 0 < sizes[i] <= WHOLE_MAX
        assert res.has_checksum[j] == (1 if want else 0), (i, sizes[i])
        if want:
            assert res.status[j] == 0 and got[j] == sums[i], (i, sizes[i])
        else:
            assert got[j] is None and not res.checksum32[j].any(), (i, sizes[i])


@pytest.mark.parametrize("pass_sizes", [True, False], ids=["sizes", "stat"])
def test_path_call_on_a_directory(ctx, boundary_files, pass_sizes):
    from spacedrive_amd import file_identifier as fi
    paths, sizes, sums = boundary_files

    def both(rows):
        p = [paths[i] for i in rows]
        s = np.array([sizes[i] for i in rows], np.uint64) if pass_sizes else None
        return fi.identify(p, s, ctx=ctx, checksums=True), fi.identify(p, s, ctx=ctx)

    rows = list(range(len(paths)))
    res, plain = both(rows)
    assert res.status[-2] == -2 and res.status[-1] == -21  # ENOENT, EISDIR
    assert all(res.status[i] == 0 for i in range(len(sums)))
    _check_path_result(res, plain, sizes, sums, rows)
    # the small-batch routing: one file and three files per call
    for i in rows:
        _check_path_result(*both([i]), sizes, sums, [i])
    for i in range(0, len(rows) - 2, 3):
        _check_path_result(*both(rows[i:i + 3]), sizes, sums, rows[i:i + 3])


_IO_CHILD = r'''
import json, sys
sys.path.insert(0, sys.argv[1])
import numpy as np
from spacedrive_amd import file_identifier as fi
from spacedrive_amd._native import Context
job = json.load(sys.stdin)
ctx = Context(0)
out = []
for sizes in (np.array(job["sizes"], np.uint64), None):
    for rows in job["calls"]:
        p = [job["paths"][i] for i in rows]
        s = sizes[rows] if sizes is not None else None
        r = fi.identify(p, s, ctx=ctx, checksums=True)
        q = fi.identify(p, s, ctx=ctx)
        out.append({"rows": rows, "sums": r.checksums(), "has": [int(x) for x in r.has_checksum],
                    "same": bool((r.cas8 == q.cas8).all() and (r.has_key == q.has_key).all()
                                 and (r.status == q.status).all()),
                    "cas": r.cas_ids(), "status": [int(x) for x in r.status]})
print(json.dumps(out))
'''


@pytest.mark.parametrize("io", ["pread", "uring", "bounce"])
def test_path_call_readers_agree(io, boundary_files):
    """The three staging readers (SDGPU_IO, read when the context opens: a
    fresh process each) give the same checksums, with sizes passed and
    stat-ed, for the whole directory, one file and three files."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    paths, sizes, sums = boundary_files
    rows = list(range(len(paths)))
    whole_row = sizes.index(102400)
    job = {"paths": paths, "sizes": sizes,
           "calls": [rows, [whole_row], [sizes.index(1016)], [sizes.index(131072)],
                     [sizes.index(0), sizes.index(1024), sizes.index(102401)]]}
    env = dict(os.environ)
    env.pop("SDGPU_IO", None)
    if io != "bounce":
        env["SDGPU_IO"] = io
    p = subprocess.run([sys.executable, "-c", _IO_CHILD, root], input=json.dumps(job),
                       capture_output=True, text=True, timeout=120, env=env)
    assert p.returncode == 0, p.stderr[-3000:]
    calls = json.loads(p.stdout.strip().splitlines()[-1])
    assert len(calls) == 2 * len(job["calls"])
    for c in calls:
        assert c["same"], (io, c["rows"])
        for j, i in enumerate(c["rows"]):
            want = i < len(sums) and 0 < sizes[i] <= WHOLE_MAX
            assert c["has"][j] == (1 if want else 0), (io, i)
            assert c["sums"][j] == (sums[i] if want else None), (io, i)
            if i < len(sums) and sizes[i]:
                assert c["status"][j] == 0 and c["cas"][j] == O.cas_id_path(paths[i], sizes[i])


def test_stale_sizes(ctx, tmp_path):
    """The checksum is of the bytes the call read, whatever size was passed: a
    file longer than the size says (inside and beyond its slab reservation)."""
    from spacedrive_amd import file_identifier as fi
    a = tmp_path / "grown_a.bin"
    a.write_bytes(O.synth_file_bytes(71, 0, 5000))
    b = tmp_path / "grown_b.bin"
    b.write_bytes(O.synth_file_bytes(72, 0, 200_000))
    c = tmp_path / "grown_c.bin"  # 3000 bytes more than stated: inside the reservation
    c.write_bytes(O.synth_file_bytes(73, 0, 4000))
    paths = [str(a), str(b), str(c)]
    sizes = np.array([10, 1000, 1000], np.uint64)
    res = fi.identify(paths, sizes, ctx=ctx, checksums=True)
    assert res.status.tolist() == [0, 0, 0] and res.has_checksum.tolist() == [1, 1, 1]
    assert res.checksums() == [O.file_checksum_path(p) for p in paths]
    assert res.cas_ids() == [O.cas_id_path(p, int(s)) for p, s in zip(paths, sizes)]
    plain = fi.identify(paths, sizes, ctx=ctx)
    np.testing.assert_array_equal(res.cas8, plain.cas8)


# ---- the job -------------------------------------------------------------------------

def _job_library(root, n=300, seed=5):
    from spacedrive_amd.file_identifier import FilePaths
    rng = np.random.default_rng(seed)
    loc = os.path.join(root, "loc")
    os.makedirs(os.path.join(loc, "a"))
    t = FilePaths()
    t.add(1, "/", "a", is_dir=True)
    pool = [0, 0, 1, 1000, 4096, 102400, 102401, 150_000, 300_000]
    contents = []
    missing = None
    for i in range(n):
        if contents and rng.random() < 0.2:
            data = contents[rng.integers(0, len(contents))]
        else:
            size = pool[rng.integers(0, len(pool))] if rng.random() < 0.5 else \
                int(rng.integers(1, 50_000))
            data = O.synth_file_bytes(30_000 + i, 0, size)
            contents.append(data)
        d = "/a/" if i % 3 == 0 else "/"
        name = f"f{i:04d}.bin"
        fid = t.add(1, d, name)
        if i == 7:
            missing = fid  # no file: ENOENT, the row stays an orphan
            continue
        with open(os.path.join(loc, d.lstrip("/"), name), "wb") as f:
            f.write(data)
    return t, loc, missing


def test_job_fills_integrity_checksum(ctx, tmp_path):
    import copy
    from spacedrive_amd import validation
    from spacedrive_amd.file_identifier import FileIdentifierJob
    t0, loc, missing = _job_library(str(tmp_path))
    path_of = lambda t, f: os.path.join(loc, t.rel_path(f))  # noqa: E731

    def run_job(t, **kw):
        job = FileIdentifierJob(t, 1, loc, chunks_per_step=1, ctx=ctx, **kw).init()
        job.run()
        job.close()

    def validate(t, fids):
        done = validation.validator_job([path_of(t, f) for f in fids], ctx)
        for f in fids:
            t.integrity_checksum[f - 1] = done[path_of(t, f)]

    # A: identifier without checksums, the validator over every row
    ta = copy.deepcopy(t0)
    run_job(ta)
    assert ta.integrity_checksum == [None] * len(ta)
    todo = ta.unvalidated(1)
    assert todo == ta._file_rows[1]  # every file row of the location
    validate(ta, [f for f in todo if f != missing])
    # B: identifier with checksums, the validator over what is left
    tb = copy.deepcopy(t0)
    run_job(tb, checksums=True)
    left = tb.unvalidated(1)
    size_of = lambda f: os.path.getsize(path_of(tb, f))  # noqa: E731
    want_left = [f for f in tb._file_rows[1]
                 if f == missing or size_of(f) == 0 or size_of(f) > WHOLE_MAX]
    assert left == want_left and 20 < len(left) < len(todo) // 2
    assert tb.unvalidated(1, "a") == [f for f in left if tb.materialized_path[f - 1] == "/a/"]
    validate(tb, [f for f in left if f != missing])
    assert tb.integrity_checksum == ta.integrity_checksum
    assert tb.cas_id == ta.cas_id and tb.object_id == ta.object_id
    assert tb.integrity_checksum[missing - 1] is None
    f = next(f for f in tb._file_rows[1] if f != missing and 0 < size_of(f) <= WHOLE_MAX)
    assert tb.integrity_checksum[f - 1] == O.file_checksum_path(path_of(tb, f))
    # C: interrupted after one step, resumed through its JSON state
    tc = copy.deepcopy(t0)
    jc = FileIdentifierJob(tc, 1, loc, chunks_per_step=1, ctx=ctx, checksums=True).init()
    jc.run(max_steps=1)
    state = json.loads(json.dumps(jc.state()))
    jc.close()
    assert state["checksums"] is True
    jr = FileIdentifierJob.resume(tc, state, ctx=ctx)
    jr.run()
    jr.close()
    assert tc.unvalidated(1) == left
    validate(tc, [f for f in left if f != missing])
    assert tc.integrity_checksum == tb.integrity_checksum
    assert tc.cas_id == tb.cas_id and tc.object_id == tb.object_id
    # a state written before the flag existed resumes without checksums
    state.pop("checksums")
    old = FileIdentifierJob.resume(copy.deepcopy(tc), state, ctx=ctx)
    assert old.checksums is False
    old.close()
