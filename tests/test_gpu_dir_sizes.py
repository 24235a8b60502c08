"""GPU: the recursive directory sizes of a location.  Every case compares all
four outputs of dir_sizes.sizes (device tensors) and dir_sizes.sizes_host (host
arrays) with dir_sizes.sizes_oracle for exact equality; each shape is the
smallest that reaches one thing the kernels can get wrong (the table of the
issue: empty call, no directories, empty directories, a chain longer than a
wave, a star, runs of length 1, a shuffled bushy tree, self keys that share
table slots, malformed parents, poisoned buffers, the Python layer)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:          # the poison case runs this file as a script
    sys.path.insert(0, ROOT)

from tests import dir_sizes_cases as C  # noqa: E402


def _dev(a):
    import torch
    if a is None:
        return None
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda()


def run_device(cols, ctx=None, poison=False, want_files=True):
    """dir_sizes.sizes on device copies of the columns, as numpy arrays of the
    header's types.  poison: the entry point itself, on output buffers filled
    with 0xA5 bytes and longer than the rows, whose tails must stay as they were."""
    import torch
    from spacedrive_amd import dir_sizes as D
    from spacedrive_amd._native import check, default_context
    d = [_dev(c) for c in cols]
    if not poison:
        parent, total, files, counts = D.sizes(*d, ctx=ctx, want_files=want_files)
    else:
        ctx = ctx or default_context(0)
        n, pad = cols[0].size, 64
        fill = lambda dt: torch.full((n + pad,), -0x5A5A5A5A5A5A5A5B if dt == torch.int64  # noqa: E731
                                     else -0x5A5A5A5B, dtype=dt, device="cuda")
        parent, total, files = fill(torch.int32), fill(torch.int64), fill(torch.int32)
        counts = torch.full((4 + pad,), -0x5A5A5A5A5A5A5A5B, dtype=torch.int64, device="cuda")
        ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None  # noqa: E731
        check(ctx.lib.sdgpu_dir_sizes_device(
            ctx.h, ptr(d[0]), ptr(d[1]), ptr(d[2]), ptr(d[3]), n, parent.data_ptr(),
            total.data_ptr(), files.data_ptr(), counts.data_ptr(),
            torch.cuda.current_stream().cuda_stream), "sdgpu_dir_sizes_device")
        torch.cuda.synchronize()
        for t, m in ((parent, n), (total, n), (files, n), (counts, 4)):
            tail = t[m:].cpu().numpy()
            assert (tail.view(np.uint8) == 0xA5).all(), "written past the rows"
        parent, total, files, counts = parent[:n], total[:n], files[:n], counts[:4]
    return (parent.cpu().numpy().view(np.uint32), total.cpu().numpy().view(np.uint64),
            None if files is None else files.cpu().numpy().view(np.uint32),
            counts.cpu().numpy().view(np.uint64))


def agree(cols, ctx=None, want=None, poison=False):
    """Both entry points against the oracle (or `want`); returns the oracle's."""
    from spacedrive_amd import dir_sizes as D
    want = want or D.sizes_oracle(*cols)
    names = ("parent", "total", "files", "counts")
    for what, got in (("device", run_device(cols, ctx, poison)),
                      ("host", D.sizes_host(*cols, ctx=ctx))):
        for g, w, name in zip(got, want, names):
            assert g.dtype == w.dtype, (what, name)
            np.testing.assert_array_equal(g, w, err_msg=f"{what} {name}")
    return want


pytestmark = pytest.mark.gpu


def test_empty_call(ctx):
    e = np.zeros(0, np.uint64)
    want = agree((e, e, np.zeros(0, np.uint8), e), ctx)
    assert want[3].tolist() == [0, 0, 0, 0]
    want = agree((e, None, None, e), ctx)
    assert want[3].tolist() == [0, 0, 0, 0]


def test_files_only(ctx):
    one = (np.array([9], np.uint64), None, None, np.array([1234], np.uint64))
    want = agree(one, ctx)
    assert want[1].tolist() == [1234] and want[3].tolist() == [0, 0, 1, 1234]
    rng = np.random.default_rng(1)
    n = 700
    cols = (rng.integers(0, 1 << 63, n, dtype=np.uint64).repeat(3)[:n], None, None,
            rng.integers(0, 1 << 50, n, dtype=np.uint64))
    want = agree(cols, ctx)
    assert want[3].tolist() == [0, 0, n, int(cols[3].sum())]
    # the same rows with a flags column of zeros: the self keys are never used
    agree((cols[0], np.zeros(n, np.uint64), np.zeros(n, np.uint8), cols[3]), ctx, want=want)


def test_empty_directories(ctx):
    cols = C.columns(C.empty_directories())
    want = agree(cols, ctx)
    assert not want[1].any() and not want[2].any()
    assert want[3].tolist() == [54, 54, 40, 0]


def test_chain_deeper_than_a_wave(ctx):
    cols = C.columns(C.chain(70))
    want = agree(cols, ctx)
    assert want[1].tolist() == [12345] * 71 and want[2][:70].tolist() == [1] * 70
    assert want[3].tolist() == [70, 70, 1, 12345]
    # the same chain listed from the bottom up
    agree(C.columns(C.chain(70)[::-1]), ctx)


def test_star(ctx):
    """5000 files in one directory: several workgroups on one address, runs
    carried across wave steps, carries past 2^32."""
    n = 5000
    cols = C.columns(C.star(n))
    want = agree(cols, ctx)
    assert int(want[1][0]) == n * (1 << 33) + n * (n - 1) // 2 and int(want[2][0]) == n
    # without file counts: the library's own counters stand in
    got = run_device(cols, ctx, want_files=False)
    assert got[2] is None
    np.testing.assert_array_equal(got[1], want[1])
    np.testing.assert_array_equal(got[3], want[3])


def test_star_alternating(ctx):
    """Runs of length 1."""
    want = agree(C.columns(C.star_alternating(3000)), ctx)
    assert want[2][:2].tolist() == [1500, 1500]


def test_bushy_shuffled(ctx):
    rows = C.bushy()
    assert len(rows) == 2 + 20 + 300 + 900
    # children precede parents somewhere, and siblings are scattered
    pos = {mp + nm + "/": i for i, (mp, nm, d, _) in enumerate(rows) if d}
    assert sum(1 for i, (mp, _, _, _) in enumerate(rows) if mp != "/" and pos[mp] > i) > 300
    want = agree(C.columns(rows), ctx)
    assert want[3][:3].tolist() == [322, 322, 2]
    assert int(want[3][3]) == sum(s for _, _, d, s in rows if not d)


@pytest.mark.parametrize("kind,n_keys,specials", [("one_home", 300, True), ("straddle", 200, True),
                                                  ("one_home", 512, False)])
def test_chosen_self_keys(ctx, kind, n_keys, specials):
    """Self keys that share home slots: chains that wrap around the table's end
    (at load exactly 1/2 for 512 keys in 1024 slots), the keys 0 and ~0, and
    absent keys whose walks run through the whole cluster."""
    from tests import hash_keys as H
    cols, sc = C.chosen_self_keys(kind, n_keys, specials)
    H.check_table_scenario(sc)
    want = agree(cols, ctx)
    nd = sc.keys.size
    assert want[3][:2].tolist() == [nd, nd]
    # every absent key is parentless, every file of a directory found its row
    n_abs = sc.absent.size
    assert (want[0][-n_abs:] == C.MISS).all() and (want[0][nd:-n_abs] != C.MISS).all()


def test_malformed(ctx):
    """UNRESOLVED exactly on the cycle members, everything else exact, counts
    as defined -- and the call returns."""
    cols, by_hand = C.malformed()
    want = agree(cols, ctx)
    for w, h in zip(want, by_hand):
        assert w.tolist() == h.tolist()
    # the same rows many times over with distinct keys per copy: cycles in
    # every workgroup, next to resolved rows
    reps = 600
    big = tuple(np.concatenate([np.where(c != 0, c + np.uint64(1000 * r), c) if i < 2 else c
                                for r in range(reps)]) for i, c in enumerate(cols))
    want = agree(big, ctx)
    assert want[3].tolist() == [6 * reps, 3 * reps, 3 * reps, 110 * reps]


def scenarios():
    rows = C.bushy(seed=8) + [("/x/", "f%d" % i, False, i) for i in range(9000)]
    return [("bushy_and_run", C.columns(rows)), ("malformed", C.malformed()[0]),
            ("star", C.columns(C.star(5000)))]


def child():
    sys.path.insert(0, ROOT)
    from spacedrive_amd._native import Context
    out = {}
    with Context(0) as ctx:
        for name, cols in scenarios():
            try:
                agree(cols, ctx, poison=True)
                out[name] = True
            except AssertionError as e:
                out[name] = str(e)[:300]
            print(f"scenario {name}", file=sys.stderr, flush=True)
    print(json.dumps(out))


def test_poisoned_workspace_and_outputs():
    """SDGPU_POISON_WS=1 in a fresh process (every buffer the library allocates
    for itself starts as 0xA5 bytes and is logged, csrc/ctx.hpp), outputs filled
    with 0xA5: the large call allocates and reads poison, the small one reads
    its leftovers."""
    env = dict(os.environ, SDGPU_POISON_WS="1")
    p = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True,
                       timeout=240, env=env, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    out = json.loads(p.stdout.strip().splitlines()[-1])
    assert len(out) == 3 and all(v is True for v in out.values()), out
    first = p.stderr[:p.stderr.index("scenario bushy_and_run")]
    assert "poisoned" in first and "link_ws" in first, p.stderr[-2000:]


def test_location_sizes_end_to_end(tmp_path):
    """indexer.scan + apply over a real tree, dir_sizes.location_sizes against
    os.walk sums, and explorer.paths ordered by sizeInBytes over those totals."""
    from spacedrive_amd import dir_sizes as D
    from spacedrive_amd import explorer as E
    from spacedrive_amd import indexer as X
    from spacedrive_amd.file_identifier import FilePaths
    tree = {"small/a.txt": 10, "small/b.txt": 20, "big/x.bin": 5000, "big/deep/y.bin": 7000,
            "big/deep/deeper/z.bin": 1, "mid/100%/q.dat": 900, "mid/ünï/r.dat": 800,
            "mid/s.dat": 1, "empty/.keep": 0, "top.txt": 3}
    for rel, sz in tree.items():
        f = tmp_path / rel
        f.parent.mkdir(parents=True, exist_ok=True)
        f.write_bytes(b"x" * sz)
    (tmp_path / "void").mkdir()
    index = X.LocationIndex()
    X.apply(index, X.rescan(index, tmp_path))
    rows = index.rows()
    full = {r[0]: r[1] + r[2] + ("." + r[3] if r[3] else "") for r in rows}   # id -> rel path
    full = {fid: p.lstrip("/") for fid, p in full.items()}
    totals, location = D.location_sizes(index, lambda fid: os.path.getsize(tmp_path / full[fid]))
    want = {}
    for fid, rel in full.items():
        p = tmp_path / rel
        want[fid] = (sum(os.path.getsize(os.path.join(d, f)) for d, _, fs in os.walk(p)
                         for f in fs) if p.is_dir() else os.path.getsize(p))
    assert totals == want
    assert location == sum(tree.values())
    by_path = {full[fid]: t for fid, t in totals.items()}
    assert (by_path["big"], by_path["big/deep"], by_path["mid"], by_path["empty"],
            by_path["void"]) == (12001, 7001, 1701, 0, 0)
    # the explorer's size column: directories carry their totals
    t = FilePaths()
    for r in rows:
        t.add(1, r[1], r[2] + ("." + r[3] if r[3] else ""), r[4])
    cols = E.SearchColumns(t, size_in_bytes=[totals[r[0]] for r in rows])
    got = E.paths(cols, 100, {"orderOnly": {"field": "sizeInBytes", "value": "Desc"}},
                  {"locationId": 1})
    assert len(got) == len(rows)
    dirs = [t.materialized_path[x["row"]].lstrip("/") + t.name[x["row"]] for x in got
            if t.is_dir[x["row"]]]
    assert dirs[:7] == ["big", "big/deep", "mid", "mid/100%", "mid/ünï", "small",
                        "big/deep/deeper"]
    assert sorted(dirs[7:]) == ["empty", "void"]
    top = E.paths(cols, 100, {"orderOnly": {"field": "sizeInBytes", "value": "Asc"}},
                  {"locationId": 1, "path": ""})
    names = [t.name[x["row"]] for x in top if t.is_dir[x["row"]]]
    assert names[2:] == ["small", "mid", "big"] and sorted(names[:2]) == ["empty", "void"]


if __name__ == "__main__":
    child()
