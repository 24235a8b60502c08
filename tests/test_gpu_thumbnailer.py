"""GPU: the thumbnailer's work list (sdgpu_thumbnail_worklist_device) and the
layers above it equal the restatement of thumbnail/mod.rs:204-359 and of the
header's contract in tests/thumbnailer_oracle.py: work, dir_start, stats and
present, exactly."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import thumbnailer_oracle as TO
from tests.test_gpu_stale_thumbnails import dev, pool

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = np.uint64(0xFFFFFFFFFFFFFFFF)
POISON32 = 0xA5A5A5A5


def expected(thumbs, keys, has=None, elig=None, regen=False):
    work, start, stats, present = TO.work_list(TO.rows_of(keys, has, elig),
                                               set(TO.hex_of_keys(thumbs)), regen)
    return (np.array(work, np.int64), np.array(start, np.int64), np.array(stats, np.int64),
            np.array(present, np.uint8))


def run(ctx, thumbs, keys, has=None, elig=None, regen=False, trim=True):
    from spacedrive_amd import thumbnailer as T
    work, start, stats, present = T.work_list(
        dev(thumbs), dev(keys), None if has is None else dev(has),
        None if elig is None else dev(elig), regenerate=regen, want_present=True, ctx=ctx,
        trim=trim)
    u32 = lambda t: t.cpu().numpy().view(np.uint32).astype(np.int64)  # noqa: E731
    return u32(work), u32(start), u32(stats), present.cpu().numpy()


def mismatches(got, want):
    """Per output, whether it differs from the oracle's (0 = equal).  got's work
    may be untrimmed: it is compared up to W, and must be untouched past it
    when it started as poison."""
    (work, start, stats, present), (e_work, e_start, e_stats, e_present) = got, want
    w = e_work.size
    return [int(not np.array_equal(work[:w], e_work)), int(not np.array_equal(start, e_start)),
            int(not np.array_equal(stats, e_stats)), int(not np.array_equal(present, e_present))]


def check(ctx, thumbs, keys, has=None, elig=None, regen=False):
    got, want = run(ctx, thumbs, keys, has, elig, regen), expected(thumbs, keys, has, elig, regen)
    for g, e, name in zip(got, want, ("work", "dir_start", "stats", "present")):
        np.testing.assert_array_equal(g, e, err_msg=name)
    return got


def column(seed, thumbs, rows):
    """rows keys drawn from (up to 3000 of) the thumbnails and 3000 foreign
    keys, about a tenth of the rows keyless and a fifth ineligible."""
    rng = np.random.default_rng(seed)
    col = rng.choice(np.concatenate([thumbs[:3000], pool()["foreign"][:3000]]), rows)
    has = (rng.random(rows) > 0.1).astype(np.uint8)
    elig = (rng.random(rows) > 0.2).astype(np.uint8)
    return col, has, elig


# the probe's 1024-row step, the 4096-row compaction tile, the 1024-slot minimum table, each +-1
@pytest.mark.parametrize("rows", [0, 1, 1023, 1024, 1025, 4095, 4096, 4097, 300_000])
@pytest.mark.parametrize("n_thumbs", [0, 1, 512, 1024, 1025, 4097])
def test_sizes(ctx, n_thumbs, rows):
    thumbs = pool()["keys"][:n_thumbs]
    col, has, elig = column(rows + n_thumbs, thumbs, rows)
    work, start, stats, present = check(ctx, thumbs, col, has, elig)
    if n_thumbs == 0:
        assert not present.any() and stats[0] == 0
    if rows == 300_000 and n_thumbs >= 512:
        assert 0 < stats[2] < stats[1] and 0 < stats[3] < stats[1] - stats[2]


def test_probe_walks(ctx):
    """1024 thumbnails in 2048 slots, load exactly 1/2: 409 of the pool's first
    1024 keys share their home slot with another, so both the build's and the
    probe's walks go past the first slot."""
    from oracle import oracle as O
    p = pool()
    thumbs = p["keys"][:1024]
    home = O.mix64(thumbs) & np.uint64(2047)
    _, inv, cnt = np.unique(home, return_inverse=True, return_counts=True)
    shared = int((cnt[inv] > 1).sum())
    assert shared >= 300 and shared == 409
    rng = np.random.default_rng(11)
    col = rng.permutation(np.concatenate([thumbs, p["foreign"][:5000], p["keys"][1024:3000]]))
    _, _, stats, present = check(ctx, thumbs, col)
    assert stats[0] == 1024 == present.sum()
    # keys that are no thumbnails but whose home slot is taken: they walk to an empty slot
    absent = p["keys"][1024:60_000]
    taken = np.isin(O.mix64(absent) & np.uint64(2047), home)
    assert taken.sum() > 10_000
    _, _, stats, _ = check(ctx, thumbs, absent[taken][:10_000])
    assert stats[0] == 0 and stats[3] == 10_000


def copies_column(case):
    p, rng = pool(), np.random.default_rng(31)
    if case == "one_to_five":      # copies land in other 1024-row blocks and 4096-row tiles
        base = p["keys"][:6000]
        col = rng.permutation(np.repeat(base, rng.integers(1, 6, base.size)))
    elif case == "one_key_70000":
        col = np.full(70_000, p["keys"][77], np.uint64)
    elif case == "one_directory":
        base = (p["keys"][:4000] & ~np.uint64(0xFF)) | np.uint64(0x5A)
        col = rng.permutation(np.repeat(base, 3))
    else:                          # every third directory, the others empty
        base = p["keys"][:5000]
        base = (base & ~np.uint64(0xFF)) | ((base & np.uint64(0xFF)) // np.uint64(3) * np.uint64(3))
        col = rng.permutation(np.repeat(base, 2))
    return col


@pytest.mark.parametrize("case", ["one_to_five", "one_key_70000", "one_directory", "sparse_directories"])
def test_copies(ctx, case):
    col = copies_column(case)
    thumbs = pool()["keys"][1000:2000]          # a sixth or so of the keys already have one
    work, start, stats, _ = check(ctx, thumbs, col)
    cand = stats[1] - stats[2]
    assert 0 < stats[3] < cand                  # neither everything dropped nor everything kept
    counts = np.diff(start)
    if case == "one_to_five":
        first = np.full(col.size, False)
        first[work] = True
        assert len({int(i) // 4096 for i in work}) > 3 and col.size > 4 * 4096
        # some dropped copy sits in another 4096-row tile than its work row
        pos = {int(k): int(i) for i, k in zip(work, col[work])}
        far = [i for i in np.flatnonzero(~first)[:5000]
               if int(col[i]) in pos and pos[int(col[i])] // 4096 != i // 4096]
        assert len(far) > 100
    if case == "one_key_70000":
        assert stats[3] == 1 and work[0] == 0
    if case == "one_directory":
        assert counts[0x5A] == stats[3] and counts.sum() == stats[3]
    if case == "sparse_directories":
        assert (counts[np.arange(256) % 3 != 0] == 0).all()
        assert (counts[::3] > 0).all()


@pytest.mark.parametrize("with_elig", [False, True])
@pytest.mark.parametrize("with_has", [False, True])
def test_masks(ctx, with_has, with_elig):
    thumbs = pool()["keys"][:3000]
    col, has, elig = column(5, thumbs, 20_000)
    check(ctx, thumbs, col, has if with_has else None, elig if with_elig else None)


def test_masked_rows_shadow_nothing(ctx):
    """Keyless and ineligible rows in front carry thumbnail keys and the keys of
    later candidates: they are not present (keyless), never candidates, and the
    lowest ELIGIBLE row of a key is its work row."""
    p = pool()
    thumbs = p["keys"][:2000]
    fresh = p["keys"][50_000:52_000]                       # no thumbnails of these
    col = np.concatenate([fresh[:1000], thumbs[:500],      # keyless
                          fresh[:1000], thumbs[:500],      # ineligible
                          fresh[500:], fresh, thumbs[:1000]])
    has = np.ones(col.size, np.uint8)
    elig = np.ones(col.size, np.uint8)
    has[:1500] = 0
    elig[1500:3000] = 0
    work, start, stats, present = check(ctx, thumbs, col, has, elig)
    assert not present[:1500].any() and present[2500:3000].all()   # present ignores eligible
    assert work.min() >= 3000 and stats[3] == 2000
    first = {int(k): 3000 + i for i, k in reversed(list(enumerate(col[3000:].tolist())))}
    assert sorted(work.tolist()) == sorted(first[int(k)] for k in fresh)
    assert stats.tolist() == [500 + 1000, 4500, 1000, 2000]


@pytest.mark.parametrize("special", [0, int(ALL)])
@pytest.mark.parametrize("case", ["thumbnail_only", "row_only", "both", "duplicated"])
def test_special_keys(ctx, special, case):
    """Key 0 and key ~0 (the table's empty marker) are ordinary keys."""
    p = pool()
    sp = np.uint64(special)
    thumbs = p["keys"][:300].copy()
    col = np.concatenate([p["keys"][:300:3], p["foreign"][:100]])
    has = np.ones(col.size, np.uint8)
    if case in ("thumbnail_only", "both", "duplicated"):
        thumbs[17] = sp
    if case in ("row_only", "both", "duplicated"):
        col[5] = sp
    if case == "duplicated":
        thumbs[250] = sp
        col[150], col[160] = sp, sp
        col[3], has[3] = sp, 0             # a keyless row holding it: not present
    work, _, stats, present = check(ctx, thumbs, col, has)
    if case == "row_only":
        assert present[5] == 0 and 5 in work
    if case in ("both", "duplicated"):
        assert present[5] == 1 and 5 not in work
    if case == "duplicated":
        assert present[3] == 0 and present[150] == 1 and present[160] == 1
        work, _, _, _ = check(ctx, thumbs, col, has, regen=True)
        assert 5 in work and 150 not in work and 3 not in work
    if case == "row_only":                 # copies of it further down are dropped
        col[150] = sp
        work, _, _, _ = check(ctx, thumbs, col, has)
        assert 5 in work and 150 not in work


def test_regenerate(ctx):
    thumbs = pool()["keys"][:3000]
    col, has, elig = column(9, thumbs, 30_000)
    _, _, plain, _ = check(ctx, thumbs, col, has, elig)
    work, _, stats, present = check(ctx, thumbs, col, has, elig, regen=True)
    assert stats[2] == plain[2] > 0 and stats[3] > plain[3]
    assert present[work].any() and not present[work].all()


@pytest.mark.parametrize("with_has", [False, True])
def test_presence_only_mode(ctx, with_has):
    import torch
    from spacedrive_amd import thumbnailer as T
    thumbs = pool()["keys"][:4097]
    col, has, elig = column(13, thumbs, 10_000)
    has = has if with_has else None
    _, _, e_stats, e_present = expected(thumbs, col, has)
    got = T.thumbnail_exists(dev(thumbs), dev(col), None if has is None else dev(has), ctx=ctx)
    np.testing.assert_array_equal(got.cpu().numpy(), e_present)
    # the raw call: an eligible column changes nothing, stats[1..3] are written as 0
    present = torch.full((col.size,), 0xA5, dtype=torch.uint8, device="cuda")
    stats = torch.full((4,), -1, dtype=torch.int32, device="cuda")
    d_thumbs, d_col, d_elig = dev(thumbs), dev(col), dev(elig)
    d_has = None if has is None else dev(has)
    rc = ctx.lib.sdgpu_thumbnail_worklist_device(
        ctx.h, d_thumbs.data_ptr(), thumbs.size, d_col.data_ptr(),
        None if d_has is None else d_has.data_ptr(), d_elig.data_ptr(), col.size, 0,
        present.data_ptr(), None, None, stats.data_ptr(),
        torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    np.testing.assert_array_equal(present.cpu().numpy(), e_present)
    assert stats.cpu().tolist() == [int(e_stats[0]), 0, 0, 0]


def test_host_variant_equals_the_device_variant(ctx):
    from spacedrive_amd import thumbnailer as T
    thumbs = pool()["keys"][:4097]
    col, has, elig = column(17, thumbs, 20_000)
    for regen in (False, True):
        got = run(ctx, thumbs, col, has, elig, regen)
        work, start, stats, present = T.work_list_host(thumbs, col, has, elig, regenerate=regen,
                                                       want_present=True, ctx=ctx)
        host = (work.astype(np.int64), start.astype(np.int64), stats.astype(np.int64), present)
        assert mismatches(host, got) == [0, 0, 0, 0] and host[0].size == got[0].size
        assert mismatches(host, expected(thumbs, col, has, elig, regen)) == [0, 0, 0, 0]
    # no masks, no present; then no thumbnails; then no rows
    work, start, stats = T.work_list_host(thumbs, col, ctx=ctx)
    e = expected(thumbs, col)
    np.testing.assert_array_equal(work, e[0])
    np.testing.assert_array_equal(stats, e[2])
    work, start, stats = T.work_list_host(thumbs[:0], col, has, elig, ctx=ctx)
    assert stats[0] == 0 and stats[3] == work.size == expected(thumbs[:0], col, has, elig)[2][3]
    work, start, stats = T.work_list_host(thumbs, col[:0], ctx=ctx)
    assert work.size == 0 and not start.any() and not stats.any()


def test_untrimmed_equals_trimmed(ctx):
    thumbs = pool()["keys"][:4097]
    col, has, elig = column(19, thumbs, 20_000)
    work, start, stats, present = run(ctx, thumbs, col, has, elig)
    full, start2, stats2, present2 = run(ctx, thumbs, col, has, elig, trim=False)
    assert full.size == col.size and work.size == stats[3] < col.size
    np.testing.assert_array_equal(full[:work.size], work)
    np.testing.assert_array_equal(start2, start)
    np.testing.assert_array_equal(stats2, stats)
    np.testing.assert_array_equal(present2, present)


# ---- workspace reuse, poisoned start, forced grouping paths ---------------------------

def reuse_shapes():
    """A large call, a small one over keys the large one found present, and the
    large one again."""
    p = pool()
    thumbs = p["keys"][:50_000]
    col, has, elig = column(23, p["keys"][20_000:], 200_000)
    col[::7] = thumbs[:col[::7].size]
    small = (p["foreign"][:10].copy(), thumbs[:130:2].copy(), None, None)
    return [(thumbs, col, has, elig), small, (thumbs, col, has, elig)]


def run_reuse(ctx, poisoned=False):
    """Large, small, stale_thumbnails, large again on one context: per call, the
    outputs that differ from the restatement (all 0 = equal).  poisoned: the
    wrappers' buffers start as 0xA5 bytes; work past W must still hold them."""
    from tests import test_gpu_stale_thumbnails as S
    shapes = reuse_shapes()
    want = [expected(*sh) for sh in shapes[:2]]
    bad = []
    for k, (sh, e) in enumerate(zip(shapes, want + want[:1])):
        if k == 2:      # the remover's table, in the same workspace, in between
            thumbs, start, cols = S.reuse_shapes()[1]
            stale, s = S.run(ctx, thumbs, start, cols)
            e_stale, e_s = S.expected(thumbs, start, cols)
            bad.append([int(not np.array_equal(stale, e_stale)), int(not np.array_equal(s, e_s))])
        got = run(ctx, *sh, trim=False)
        m = mismatches(got, e)
        if poisoned:
            m.append(int(not (got[0][e[0].size:] == POISON32).all()))
        bad.append(m)
    return bad


def test_workspace_reuse(ctx):
    """Old tables, masks and reps must not leak into a later call."""
    assert run_reuse(ctx) == [[0] * 4, [0] * 4, [0, 0], [0] * 4]
    thumbs, col, _, _ = reuse_shapes()[1]
    work, _, stats, present = run(ctx, thumbs, col)
    assert not present.any() and stats[3] == col.size      # nothing of the large call survives


def run_forced(ctx):
    """The composed call at 70 000 rows (copies, masks, a third present) with
    the kernel timer on: mismatches and the names of the kernels that ran."""
    p = pool()
    rng = np.random.default_rng(41)
    thumbs = p["keys"][:20_000]
    col = rng.choice(p["keys"][:60_000], 70_000)
    has = (rng.random(70_000) > 0.1).astype(np.uint8)
    elig = (rng.random(70_000) > 0.2).astype(np.uint8)
    ctx.set_timing(True)
    bad = []
    for regen in (False, True):
        e = expected(thumbs, col, has, elig, regen)
        assert 0 < e[2][3] < e[2][1] - (0 if regen else e[2][2])
        bad.append(mismatches(run(ctx, thumbs, col, has, elig, regen, trim=False), e))
    ctx.sync()
    return {"bad": bad, "kernels": sorted(ctx.kernel_times())}


_CHILD = r'''
import json, sys
sys.path.insert(0, sys.argv[1])
from spacedrive_amd._native import Context
from tests import test_gpu_thumbnailer as G
if sys.argv[2] == "poison":
    from tests._poison_child import install_output_poison
    install_output_poison()
    out = G.run_reuse(Context(0), poisoned=True)
else:
    out = G.run_forced(Context(0))
print(json.dumps(out), flush=True)
'''


def child(mode, env):
    e = dict(os.environ, SDGPU_POISON_WS="1")
    e.pop("SDGPU_GROUP_BITS", None)
    e.pop("SDGPU_GROUP_HIST", None)
    e.update(env)
    p = subprocess.run([sys.executable, "-c", _CHILD, ROOT, mode], capture_output=True, text=True,
                       timeout=240, env=e)
    assert p.returncode == 0, p.stderr[-3000:]
    return json.loads(p.stdout.strip().splitlines()[-1]), p.stderr


def test_first_calls_on_poisoned_workspace():
    """The same in a fresh process whose new workspaces and output buffers start
    as 0xA5 bytes: results equal the oracle, work past W is still 0xA5."""
    out, err = child("poison", {})
    assert out == [[0] * 5, [0] * 5, [0, 0], [0] * 5]
    assert "poisoned" in err and "link_ws" in err and "dedup_ws" in err


# bits 3: the direct partition with 8 buckets, every bucket past the LDS table;
# HIST alone: the plan 70 000 rows get anyway, the histogram flag set;
# bits 13: the two-level partition over runs, and with HIST over a histogram
FORCED = [({"SDGPU_GROUP_BITS": "3"}, None),
          ({"SDGPU_GROUP_HIST": "1"}, None),
          ({"SDGPU_GROUP_BITS": "13"}, {"bucket_scatter1", "bucket_fine_scan"}),
          ({"SDGPU_GROUP_BITS": "13", "SDGPU_GROUP_HIST": "1"},
           {"bucket_hist", "bucket_scatter1", "bucket_fine_scan"})]


@pytest.mark.parametrize("env,ran", FORCED, ids=["bits3", "hist", "bits13", "bits13_hist"])
def test_forced_grouping_paths(env, ran):
    """The composed call on the grouping's other partition paths (dedup.hip
    forced_plan), each in one fresh child on poisoned workspaces."""
    out, _ = child("forced", env)
    assert out["bad"] == [[0] * 4, [0] * 4]
    names = set(out["kernels"])
    assert {"thumb_present", "thumb_work_mask", "bucket_group"} <= names
    two_level = {"bucket_scatter1", "bucket_fine_scan"}
    if ran is None:
        assert not names & two_level
    else:
        assert ran <= names and ("bucket_hist" in names) == ("bucket_hist" in ran)


# ---- end to end ------------------------------------------------------------------------

def make_location(tmp_path, seed=3):
    """A table of two locations and a thumbnail cache that already holds some
    of their thumbnails (and a misplaced copy that does not count)."""
    from spacedrive_amd import thumbnailer as T
    from spacedrive_amd.file_identifier import FilePaths
    rng = np.random.default_rng(seed)
    ids = TO.hex_of_keys(np.unique(rng.integers(1, 2**63, 500, dtype=np.uint64))[:400])
    names = ["jpg", "png", "mp4", "mkv", "txt", "JPG", "ts", "webp"]
    t = FilePaths()
    cas, loc = [], str(tmp_path / "location")
    for i in range(1500):
        ext = names[int(rng.integers(0, len(names)))]
        mp = ["/", "/a/", "/a/b/", "/c/"][int(rng.integers(0, 4))]
        fid = t.add(1 if rng.random() > 0.1 else 2, mp, f"f{i}.{ext}")
        c = ids[int(rng.integers(0, len(ids)))] if rng.random() > 0.05 else None
        t.cas_id[fid - 1] = c
        cas.append(c)
    base = str(tmp_path / "thumbs")
    on_disk = set(ids[::4])
    for c in on_disk:
        os.makedirs(os.path.join(base, c[:2]), exist_ok=True)
        with open(os.path.join(base, c[:2], c + ".webp"), "wb") as f:
            f.write(b"old")
    os.makedirs(os.path.join(base, "zz"), exist_ok=True)
    with open(os.path.join(base, "zz", ids[1] + ".webp"), "wb") as f:     # misplaced
        f.write(b"old")
    exts = T.IMAGE_EXTENSIONS + T.video_extensions()
    return t, loc, base, on_disk, exts


def thumbs_in(base):
    return {n[:-5] for d in os.listdir(base) if d != "zz"
            for n in os.listdir(os.path.join(base, d)) if n.endswith(".webp")}


@pytest.mark.parametrize("under", [None, "/a/"])
def test_process_end_to_end(ctx, tmp_path, under):
    from spacedrive_amd import thumbnailer as T
    t, loc, base, on_disk, exts = make_location(tmp_path)
    elig = T.eligible_rows(t, 1, exts, under=under)
    rows = [(c, bool(e)) for c, e in zip(t.cas_id, elig.tolist())]
    written, created_ref, skipped_ref, rewrites = TO.reference_run(rows, on_disk)
    calls = []

    def generate(kind, input_path, output_path):
        assert os.path.isdir(os.path.dirname(output_path))
        with open(output_path, "wb") as f:
            f.write(kind.encode())
        calls.append((kind, input_path, output_path))

    created, skipped, errors = T.process(t, 1, loc, base, generate, under=under, ctx=ctx)
    assert thumbs_in(base) - on_disk == written and len(written) > 20
    assert errors == [] and created == len(written) == len(calls)
    # the deviation: the reference's counters differ by exactly what it writes twice
    assert created == created_ref - rewrites and skipped == skipped_ref + rewrites
    for kind, inp, outp in calls:
        ext = inp.rsplit(".", 1)[1]
        assert kind == ("image" if ext in T.IMAGE_EXTENSIONS else "video") and ext in exts
        assert inp.startswith(loc + os.sep) and (under is None or "/a/" in inp)
        stem = os.path.basename(outp)[:-5]
        assert os.path.basename(os.path.dirname(outp)) == stem[:2]
    shards = [os.path.basename(os.path.dirname(o)) for _, _, o in calls]
    assert shards == sorted(shards)                      # directory by directory
    # a second run creates nothing and skips everything
    again = T.process(t, 1, loc, base, generate, under=under, ctx=ctx)
    assert again == (0, int(sum(1 for c, e in rows if c is not None and e)), [])
    assert len(calls) == created
    # regenerate: every distinct eligible cas_id once
    calls.clear()
    created, skipped, errors = T.process(t, 1, loc, base, generate, regenerate=True, under=under,
                                         ctx=ctx)
    distinct = {c for c, e in rows if c is not None and e}
    assert created == len(distinct) == len(calls) and not errors
    assert {os.path.basename(o)[:-5] for _, _, o in calls} == distinct


def test_process_reports_a_failing_generate(ctx, tmp_path):
    from spacedrive_amd import thumbnailer as T
    t, loc, base, on_disk, exts = make_location(tmp_path, seed=4)
    rows = [(c, bool(e)) for c, e in zip(t.cas_id, T.eligible_rows(t, 1, exts).tolist())]
    written, _, _, _ = TO.reference_run(rows, on_disk)
    seen = []

    def generate(kind, input_path, output_path):
        seen.append(input_path)
        if len(seen) == 5:
            raise ValueError("cannot decode")
        with open(output_path, "wb") as f:
            f.write(b"new")

    created, skipped, errors = T.process(t, 1, loc, base, generate, ctx=ctx)
    assert errors == [f'Had an error generating thumbnail for "{seen[4]}"']
    assert created == len(written) - 1 == len(seen) - 1
    assert len(thumbs_in(base) - on_disk) == len(written) - 1
