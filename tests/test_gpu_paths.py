"""GPU parity of the path-based drop-ins (generate_cas_id(path, size),
file_checksum(path), the batched identifier) against the oracle's path-based
restatement of the reference I/O pattern."""
import os

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 57, 1024, 1025, 8192, 102399, 102400, 102401, 200_000, 1 << 20, 3_333_333]


@pytest.fixture()
def files(tmp_path):
    paths = []
    for i, s in enumerate(SIZES):
        p = tmp_path / f"file_{i}.bin"
        p.write_bytes(O.synth_file_bytes(900 + i, 0, s))
        paths.append(str(p))
    return paths


def test_generate_cas_id_path(ctx, files):
    from spacedrive_amd import cas
    for p, s in zip(files, SIZES):
        assert cas.generate_cas_id(p, s, ctx) == O.cas_id_path(p, s)


def test_generate_cas_id_errors(ctx, tmp_path):
    from spacedrive_amd import cas
    with pytest.raises(OSError) as ei:
        cas.generate_cas_id(tmp_path / "missing", 10, ctx)
    assert ei.value.errno == 2
    short = tmp_path / "short"
    short.write_bytes(bytes(50_000))
    with pytest.raises(OSError) as ei:  # read_exact past EOF: UnexpectedEof
        cas.generate_cas_id(short, 400_000, ctx)
    assert ei.value.errno == 61  # ENODATA
    with pytest.raises(OSError):
        O.cas_id_path(str(short), 400_000)


def test_identify_batch_and_job(ctx, files, tmp_path):
    from spacedrive_amd import file_identifier as fi
    dup = tmp_path / "dup.bin"
    dup.write_bytes(open(files[9], "rb").read())
    paths = files + [str(dup), str(tmp_path / "gone"), files[9]]
    res = fi.identify(paths, ctx=ctx)
    for i, p in enumerate(paths):
        if not os.path.exists(p):
            assert res.status[i] == -2 and res.has_key[i] == 0
            continue
        s = os.path.getsize(p)
        if s == 0:
            assert res.has_key[i] == 0 and res.status[i] == 0
        else:
            assert res.has_key[i] == 1
            assert bytes(res.cas8[i]).hex() == O.cas_id_path(p, s)
    job = fi.identifier_job(paths, ctx=ctx)
    ok = (job.identify.status == 0).astype(np.uint8)
    from spacedrive_amd.cas import keys_of
    ref = O.group_reps(keys_of(job.identify.cas8), job.identify.has_key & ok, 100)
    np.testing.assert_array_equal(job.rep, ref)
    # all rows sit in the first 100-row chunk: each duplicate gets its own Object
    assert job.rep[len(files)] == len(files) and job.rep[-1] == len(paths) - 1
    # with 10-row chunks the later duplicates (rows 12, 14) link to row 9's Object
    job10 = fi.identifier_job(paths, chunk_size=10, ctx=ctx)
    assert job10.rep[len(files)] == 9 and job10.rep[-1] == 9
    assert job10.linked == 2


def test_identify_many_files_pipelined(ctx, tmp_path):
    """More files than one staging slab's file budget is not needed; 3000
    files of mixed sizes exercise the threaded pread + H2D pipeline."""
    from spacedrive_amd import corpus
    from spacedrive_amd import file_identifier as fi
    sizes, seeds = corpus.config2_files(3000, seed=5)
    sizes = np.minimum(sizes, 3_000_000)
    paths = []
    for i in range(sizes.size):
        p = tmp_path / f"m{i}"
        with open(p, "wb") as f:
            f.write(O.synth_file_bytes(int(seeds[i]), 0, int(sizes[i])))
        paths.append(str(p))
    res = fi.identify(paths, sizes=sizes, ctx=ctx)
    assert np.all(res.status == 0)
    for i in range(0, sizes.size, 7):
        if sizes[i]:
            assert bytes(res.cas8[i]).hex() == O.cas_id_of_message(
                O.synth_cas_message(int(sizes[i]), int(seeds[i])))


def test_file_metadata(ctx, files):
    from spacedrive_amd import file_identifier as fi
    m = fi.file_metadata(os.path.dirname(files[5]), os.path.basename(files[5]), ctx)
    assert m.cas_id == O.cas_id_path(files[5], SIZES[5]) and m.size == SIZES[5]
    assert fi.file_metadata(os.path.dirname(files[0]), os.path.basename(files[0]), ctx).cas_id is None


def test_checksum_files_batched_validator(ctx, tmp_path):
    """sdgpu_checksum_files over a directory of mixed files: tiny, chunk
    boundaries, > 1 slab in total, one streamed (> 16 MiB) file, and errors."""
    from spacedrive_amd import validation
    sizes = [0, 1, 63, 64, 65, 1023, 1024, 1025, 2048, 16 * 1024 + 1, 1 << 20, (1 << 20) + 1,
             5_000_000, 17 << 20]
    rng = np.random.default_rng(3)
    sizes += [int(x) for x in rng.integers(0, 3_000_000, 150)]  # ~225 MB: crosses a slab
    paths = []
    for i, s in enumerate(sizes):
        p = tmp_path / f"v{i}"
        p.write_bytes(O.synth_file_bytes(4000 + i, 0, s))
        paths.append(str(p))
    paths += [str(tmp_path / "missing"), str(tmp_path)]
    out, st = validation.checksum_files(paths, ctx)
    assert st[-2] == -2 and st[-1] == -21  # ENOENT, EISDIR
    for i, p in enumerate(paths[:-2]):
        assert st[i] == 0, (i, st[i])
        assert bytes(out[i]).hex() == O.file_checksum_path(p), (i, sizes[i])
    assert not out[-2:].any()
    job = validation.validator_job(paths[:20], ctx)
    assert job[paths[5]] == O.file_checksum_path(paths[5])
    with pytest.raises(OSError):
        validation.validator_job(paths, ctx)


def test_identify_fresh_sizes_directory_is_an_error(ctx, files, tmp_path):
    """With sizes stat-ed by the library (size NULL), a directory is -EISDIR
    with no key -- also an empty one, whatever st_size the filesystem gives
    it -- never an empty file's cas_id None with status 0 (the reference
    asserts the path is not a directory, file_identifier/mod.rs:69-72)."""
    from spacedrive_amd import file_identifier as fi
    empty_dir = tmp_path / "empty_dir"
    empty_dir.mkdir()
    paths = [files[3], str(tmp_path), str(empty_dir), files[0]]
    res = fi.identify(paths, ctx=ctx)
    assert list(res.status) == [0, -21, -21, 0], res.status
    assert list(res.has_key) == [1, 0, 0, 0]
    assert bytes(res.cas8[0]).hex() == O.cas_id_path(files[3], SIZES[3])
    assert not res.cas8[1:].any()


_IO_CHILD = r'''
import json, sys
sys.path.insert(0, sys.argv[1])
from spacedrive_amd import file_identifier as fi
from spacedrive_amd._native import Context
paths = json.load(sys.stdin)  # not argv: one argument holds at most 128 KiB
ctx = Context(0)
res = fi.identify(paths, ctx=ctx)
print(json.dumps({"cas": [bytes(c).hex() for c in res.cas8], "status": [int(s) for s in res.status],
                  "has": [int(h) for h in res.has_key]}))
'''


@pytest.mark.parametrize("io", ["pread", "uring", "bounce"])
def test_identify_read_paths_agree(io, files, tmp_path):
    """The three staging readers of sdgpu_identify_files -- pread into the
    slab (SDGPU_IO=pread), io_uring chains (SDGPU_IO=uring; where the ring is
    refused it finishes through pread), and the default per-thread buffer
    streamed into the slab -- give the oracle's cas ids and statuses, in a
    fresh process each (the variable is read when the context opens)."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    paths = files + [str(tmp_path / "missing"), str(tmp_path)]
    env = dict(os.environ)
    env.pop("SDGPU_IO", None)
    if io != "bounce":
        env["SDGPU_IO"] = io
    p = subprocess.run([sys.executable, "-c", _IO_CHILD, root], input=json.dumps(paths),
                       capture_output=True, text=True, timeout=120, env=env)
    assert p.returncode == 0, p.stderr[-3000:]
    res = json.loads(p.stdout.strip().splitlines()[-1])
    for i, s in enumerate(SIZES):
        assert res["status"][i] == 0, (io, i)
        if s == 0:
            assert res["has"][i] == 0
        else:
            assert res["has"][i] == 1 and res["cas"][i] == O.cas_id_path(files[i], s), (io, i)
    assert res["status"][-2:] == [-2, -21] and res["has"][-2:] == [0, 0], res["status"][-2:]


@pytest.fixture(scope="module")
def config1_dir(tmp_path_factory):
    """2000 sparse config-1 files (1 KiB-10 MiB) and the oracle's cas ids."""
    from spacedrive_amd import corpus
    root = str(tmp_path_factory.mktemp("cfg1"))
    paths, sizes = corpus.write_config1_dir(root, 2000, seed=7)
    return paths, [O.cas_id_path(p, int(s)) for p, s in zip(paths, sizes)]


@pytest.mark.parametrize("env", [{"SDGPU_SLAB_DIV": "64"}, {"SDGPU_SLAB_TAPER": "1"},
                                 {"SDGPU_SLAB_DIV": "2", "SDGPU_SLAB_TAPER": "1"},
                                 {"SDGPU_IO_THREADS": "3"}, {"SDGPU_IO": "uring"}],
                         ids=["div64", "taper", "div2_taper", "threads3", "uring"])
def test_identify_staging_schedules_agree(env, config1_dir):
    """The staging schedule's settings (slab = call bytes / SDGPU_SLAB_DIV,
    a tail taper, the read-pool size, the io_uring reader) change how 2000
    config-1 files are cut into slabs and read, never their cas ids: each
    variant in a fresh process equals the oracle on every file."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    paths, want = config1_dir
    e = {k: v for k, v in os.environ.items() if not k.startswith("SDGPU_")}
    e.update(env)
    p = subprocess.run([sys.executable, "-c", _IO_CHILD, root], input=json.dumps(paths),
                       capture_output=True, text=True, timeout=180, env=e)
    assert p.returncode == 0, p.stderr[-3000:]
    res = json.loads(p.stdout.strip().splitlines()[-1])
    assert all(s == 0 for s in res["status"]) and all(h == 1 for h in res["has"])
    bad = [i for i, (g, w) in enumerate(zip(res["cas"], want)) if g != w]
    assert not bad, (env, len(bad), bad[:5])
