"""Child-process harness of tests/test_gpu_poison_entry_points.py: every device
entry point on poisoned workspaces and poisoned output buffers.

The rule under test: no result may depend on a byte the call did not write.

* Workspaces: the parent starts this module with SDGPU_POISON_WS=1, so every
  buffer the library allocates for itself starts as 0xA5 bytes and is logged
  on stderr as ``sdgpu: poisoned <bytes> <what>`` (csrc/ctx.hpp).  A scenario
  runs on a fresh ``Context(0)``, so its first call is the one that allocates:
  it reads poison wherever it reads a word it did not write.  The second call
  is a smaller one of another shape (it sees the leftovers of the first), the
  third repeats the first.
* Outputs: ``torch.empty`` and the ``np.zeros`` / ``np.empty`` the wrapper
  modules of spacedrive_amd see hand out buffers filled with 0xA5 bytes
  (install_output_poison), so an element a kernel forgets to write is neither a
  lucky zero nor the right answer of an earlier identical call that torch's
  caching allocator handed back.

A scenario is ``build(tmp) -> (facts, run)``: ``build`` makes the inputs and
the reference on the host (no GPU; tests/test_poison_scenarios.py checks the
facts), ``run(R)`` makes the calls through ``R.call`` -- each returns the
number of positions that differ from the reference (0 = equal).  The child
prints one JSON object: per scenario the mismatch count of every call, how
many output buffers were poisoned, and the seconds it took.  Between calls it
writes a marker line to stderr, so the parent can tell which poisoned
allocations belong to which call (parse_log).

Elements the header leaves unspecified are not compared, and only these: the
tails of K7's lists, of the fused lists, of the orphan list and of the
thumbnail order past their counts with trim=False.
"""
import functools
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from oracle import oracle as O  # noqa: E402

POISON = 0xA5
MARK = "@@poison-child"
LOG_RE = re.compile(r"^sdgpu: poisoned (\d+) (\S+)$")
CAS_MAX = 102408       # SDGPU_CAS_MAX_MSG_LEN
WHOLE_MAX = 102400     # files up to here are read whole (cas.rs:27-29)
EXISTING = 0x80000000  # SDGPU_REP_EXISTING
MISS = 0xFFFFFFFF      # SDGPU_INDEX_MISS


# ---- poisoned outputs ------------------------------------------------------------

class _Count:
    n = 0


def _poisoned_numpy(fn):
    def alloc(*a, **k):
        arr = fn(*a, **k)
        arr.reshape(-1).view(np.uint8)[...] = POISON
        _Count.n += 1
        return arr
    return alloc


class _NumpyProxy:
    """numpy, except that zeros / empty return 0xA5-filled arrays."""

    def __init__(self, real):
        self._real = real
        self.zeros = _poisoned_numpy(real.zeros)
        self.empty = _poisoned_numpy(real.empty)

    def __getattr__(self, name):
        return getattr(self._real, name)


def install_output_poison():
    """Every output buffer the wrappers allocate starts as 0xA5 bytes.  The
    wrappers import torch inside their functions, so torch.empty itself is
    replaced (this process only); numpy is replaced per wrapper module."""
    import torch
    from spacedrive_amd import (cas, consumers, dedup, file_identifier, kind, thumbnail_remover,
                                validation)
    real_empty, real_empty_like = torch.empty, torch.empty_like

    def fill(t):
        if t.numel():
            t.view(-1).view(torch.uint8).fill_(POISON)
        _Count.n += 1
        return t

    torch.empty = lambda *a, **k: fill(real_empty(*a, **k))
    torch.empty_like = lambda *a, **k: fill(real_empty_like(*a, **k))
    proxy = _NumpyProxy(np)
    for mod in (cas, consumers, dedup, file_identifier, kind, thumbnail_remover, validation):
        if getattr(mod, "np", None) is np:
            mod.np = proxy


# ---- running --------------------------------------------------------------------

class Run:
    """The calls of one scenario: contexts opened through it are closed when
    the scenario ends; every call is announced on stderr first."""

    def __init__(self, name):
        self.name, self.bad, self.ctxs = name, [], []

    def context(self):
        from spacedrive_amd._native import Context
        c = Context(0)
        self.ctxs.append(c)
        return c

    def call(self, fn):
        import torch
        print(f"{MARK} {self.name} call {len(self.bad)}", file=sys.stderr, flush=True)
        bad = int(fn())
        torch.cuda.synchronize()
        self.bad.append(bad)

    def close(self):
        for c in self.ctxs:
            c.close()


def _ne(got, want):
    """Number of positions at which got differs from want."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return max(got.size, want.size) + 1
    return int(np.count_nonzero(got != want))


def _d(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _large_small_large(R, ctx, go, large, small):
    for b in (large, small, large):
        R.call(lambda b=b: go(ctx, b))


# ---- K1 and its body pass --------------------------------------------------------

def _k1_valid(off, ln, arena_bytes):
    """include/sdgpu.h on sdgpu_cas_batch_device: 16-B aligned offset, length
    <= SDGPU_CAS_MAX_MSG_LEN, inside the arena; else -EINVAL and a zeroed id."""
    off = off.astype(np.uint64)
    return (off % 16 == 0) & (ln <= CAS_MAX) & (off + ln <= arena_bytes)


def _k1_batch(seed, lens, reject):
    """Messages 16-B aligned with random 16-B gaps, random content, and what
    the header says about them.  reject: two more messages that it rejects (a
    misaligned offset, a length over the maximum)."""
    rng = np.random.default_rng(seed)
    ln = np.asarray(lens, np.uint32).copy()
    n = ln.size
    gaps = rng.integers(0, 4, n) * 16
    padded = (ln.astype(np.int64) + 15) // 16 * 16
    off = (np.cumsum(gaps) + np.concatenate([[0], np.cumsum(padded)[:-1]])).astype(np.uint64)
    total = int(off[-1] + padded[-1])
    arena = rng.integers(0, 256, max(total, 16), dtype=np.uint8)
    rejected = []
    if reject:
        i, j = n // 3, 2 * n // 3
        off[i] += 8
        ln[j] = CAS_MAX + 1
        rejected = [i, j]
    whole = rng.integers(0, 2, n).astype(np.uint8)
    k8 = np.flatnonzero(ln == 8)
    if k8.size:
        whole[k8[0]] = 1        # a whole message of 8 bytes: the empty body
    valid = _k1_valid(off, ln, arena.size)
    out8 = np.zeros((n, 8), np.uint8)
    out8[valid] = O.cas_batch(arena, off[valid], ln[valid], 8)
    status = np.where(valid, 0, -22).astype(np.int32)
    has = (valid & (whole != 0) & (ln >= 8)).astype(np.uint8)
    out32 = np.zeros((n, 32), np.uint8)
    for i in np.flatnonzero(has):
        o = int(off[i])
        out32[i] = np.frombuffer(O.blake3(arena[o + 8:o + int(ln[i])]), np.uint8)
    return dict(arena=arena, off=off, ln=ln, whole=whole, rejected=rejected, valid=valid,
                out8=out8, status=status, has=has, out32=out32)


@functools.lru_cache(None)
def _k1_batches():
    from tests.test_gpu_fuzz import _lengths
    edge = [0, 1, 8, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 57352, CAS_MAX]
    lens = np.concatenate([edge, _lengths(np.random.default_rng(71), 3000 - len(edge))])
    large = _k1_batch(72, lens, True)
    small = _k1_batch(73, [100, 0, 1025, 57352, 9], False)
    facts = {"n_large": int(lens.size), "n_small": 5, "rejected": large["rejected"],
             "invalid_rows": np.flatnonzero(~large["valid"]).tolist(),
             "rejected_status": large["status"][large["rejected"]].tolist(),
             "rejected_ids_zero": not large["out8"][large["rejected"]].any(),
             "small_invalid": int((~small["valid"]).sum()),
             "small_has_empty": bool((small["ln"] == 0).any()),
             "lengths_present": sorted(set(edge) & set(large["ln"].tolist())) == sorted(edge),
             "whole_flags": sorted(set(large["whole"].tolist())),
             "empty_body_has_checksum": bool(large["has"][np.flatnonzero(large["ln"] == 8)[0]]),
             "n_checksums": int(large["has"].sum())}
    return large, small, facts


def _k1_args(b):
    return _d(b["arena"]), _d(b["off"].view(np.int64)), _d(b["ln"].view(np.int32))


def build_k1_bulk(tmp):
    large, small, facts = _k1_batches()

    def go(ctx, b):
        from spacedrive_amd import cas
        out, st = cas.cas_batch_device(*_k1_args(b), ctx=ctx)
        return _ne(out.cpu().numpy(), b["out8"]) + _ne(st.cpu().numpy(), b["status"])

    return facts, lambda R: _large_small_large(R, R.context(), go, large, small)


def build_k1_body(tmp):
    large, small, facts = _k1_batches()

    def go(ctx, b):
        from spacedrive_amd import cas
        out, out32, has, st = cas.cas_checksum_batch_device(*_k1_args(b), _d(b["whole"]), ctx=ctx)
        return (_ne(out.cpu().numpy(), b["out8"]) + _ne(st.cpu().numpy(), b["status"]) +
                _ne(out32.cpu().numpy(), b["out32"]) + _ne(has.cpu().numpy(), b["has"]))

    return facts, lambda R: _large_small_large(R, R.context(), go, large, small)


# ---- kinds -------------------------------------------------------------------------

@functools.lru_cache(None)
def _kind_batch():
    from tests.test_gpu_kind import _build_batch
    return _build_batch()


def _build_kind(verify):
    arena, off, ln, ext, want = _kind_batch()
    want = want[:, 1 if verify else 0]
    facts = {"n": int(ln.size), "kinds": sorted(set(want.tolist())), "n_small": 3}

    def go(ctx, m):
        from spacedrive_amd import kind as K
        got = K.kind_batch_device(_d(arena), _d(off.view(np.int64))[:m], _d(ln.view(np.int32))[:m],
                                  _d(ext.view(np.int16))[:m], verify=verify, ctx=ctx)
        return _ne(got.cpu().numpy(), want[:m])

    return facts, lambda R: _large_small_large(R, R.context(), go, int(ln.size), 3)


def build_kind_default(tmp):
    return _build_kind(False)


def build_kind_verify(tmp):
    return _build_kind(True)


# ---- K2/K3 -----------------------------------------------------------------------

TREE_SIZES = [0, 1, 1024, 1025, 16384, 16385, (1 << 20) + 1, 5 * (1 << 20) + 123]


def build_tree(tmp):
    rng = np.random.default_rng(81)
    large = [rng.integers(0, 256, s, dtype=np.uint8) for s in TREE_SIZES]
    small = [rng.integers(0, 256, 1, dtype=np.uint8)]
    want = {id(b): np.array([np.frombuffer(O.blake3(f, 8), np.uint8) for f in b])
            for b in (large, small)}
    facts = {"sizes": [int(f.size) for f in large], "small": [1]}

    def go(ctx, b):
        import torch
        from spacedrive_amd import validation
        files = [_d(f) if f.size else torch.zeros(16, dtype=torch.uint8, device="cuda")[:0]
                 for f in b]
        return _ne(validation.checksum_batch_device(files, ctx=ctx).cpu().numpy(), want[id(b)])

    return facts, lambda R: _large_small_large(R, R.context(), go, large, small)


# ---- file_checksum / generate_cas_id on paths ------------------------------------------

def slice_bytes():
    """kSliceBytes of csrc/ctx.hpp: the streamed checksum's slice."""
    text = open(os.path.join(ROOT, "spacedrive_amd", "csrc", "ctx.hpp")).read()
    m = re.search(r"kSliceBytes = size_t\((\d+)\) << (\d+);", text)
    return int(m.group(1)) << int(m.group(2))


def _write(path, data):
    with open(path, "wb") as f:
        f.write(data)
    return path


def build_streamed(tmp):
    os.makedirs(tmp, exist_ok=True)
    sl = slice_bytes()
    data = np.random.default_rng(91).integers(0, 256, 2 * sl + 1, dtype=np.uint8)
    big = _write(os.path.join(tmp, "three_slices"), data)
    one = _write(os.path.join(tmp, "one_slice"), data[:sl - 1])
    want = {p: O.file_checksum_path(p) for p in (big, one)}
    facts = {"slice": sl, "sizes": [os.path.getsize(big), os.path.getsize(one)],
             "digests_differ": want[big] != want[one]}

    def go(ctx, p):
        from spacedrive_amd import validation
        return int(validation.file_checksum(p, ctx) != want[p])

    return facts, lambda R: _large_small_large(R, R.context(), go, big, one)


def _build_latency(tmp, sizes):
    os.makedirs(tmp, exist_ok=True)
    rng = np.random.default_rng(95)
    files = {}
    for s in sorted(set(sizes)):
        p = _write(os.path.join(tmp, f"f{s}"), rng.integers(0, 256, s, dtype=np.uint8))
        files[s] = (p, O.file_checksum_path(p), O.cas_id_path(p, s))
    facts = {"sizes": list(sizes)}

    def go(ctx, s):
        from spacedrive_amd import cas, validation
        p, sum_, cas_id = files[s]
        return int(validation.file_checksum(p, ctx) != sum_) + \
            int(cas.generate_cas_id(p, s, ctx) != cas_id)

    def run(R):
        ctx = R.context()
        for s in sizes:
            R.call(lambda s=s: go(ctx, s))

    return facts, run


def build_latency(tmp):
    """k_small_split on several groups first (its zeroed counters), then two
    groups, the largest latency file, one workgroup, and the first again."""
    return _build_latency(tmp, [300 << 10, 113 << 10, 1 << 20, 4 << 10, 300 << 10])


def build_latency_small_first(tmp):
    return _build_latency(tmp, [4 << 10, 300 << 10, 4 << 10])


# ---- identify from paths ----------------------------------------------------------

EXTS = ["jpg", "txt", "ts", "png", "mts", "db", "bin", ""]


def _directory(tmp, extra_whole):
    """Files at the size edges of generate_cas_id (11 of each, under names of
    several categories), one missing path; extra_whole more files of 100 KiB
    so that a call needs several staging slabs."""
    from spacedrive_amd import corpus
    from tests import kind_oracle as KO
    os.makedirs(tmp, exist_ok=True)
    sizes = [s for s in corpus.boundary_sizes() if s <= 131072] * 11 + [WHOLE_MAX] * extra_whole
    rows = []
    for i, s in enumerate(sizes):
        ext = EXTS[i % len(EXTS)]
        name = f"f{i:04d}" + ("." + ext if ext else "")
        data = O.synth_file_bytes(700 + i, 0, s)
        p = _write(os.path.join(tmp, name), data)
        whole = 0 < s <= WHOLE_MAX
        rows.append(dict(
            path=p, size=s, status=0, has=int(s > 0),
            cas=bytes.fromhex(O.cas_id_path(p, s)) if s else bytes(8),
            has32=int(whole), sum=bytes.fromhex(O.file_checksum_path(p)) if whole else bytes(32),
            # the bytes the call reads: the whole file, or the 8 KiB header of a sampled one
            kind=KO.resolve_conflicting(name, data if s <= WHOLE_MAX else data[:8192], False)))
    rows.insert(len(rows) // 2, dict(path=os.path.join(tmp, "missing.jpg"), size=10, status=-2,
                                     has=0, cas=bytes(8), has32=0, sum=bytes(32), kind=0))
    return rows


def _want_rows(rows):
    u8 = lambda key, w: np.array([np.frombuffer(r[key], np.uint8) for r in rows]).reshape(-1, w)  # noqa: E731
    return dict(paths=[r["path"] for r in rows],
                sizes=np.array([r["size"] for r in rows], np.uint64),
                status=np.array([r["status"] for r in rows], np.int32),
                has=np.array([r["has"] for r in rows], np.uint8), cas=u8("cas", 8),
                has32=np.array([r["has32"] for r in rows], np.uint8), sum=u8("sum", 32),
                kind=np.array([r["kind"] for r in rows], np.int32))


def _build_identify(tmp, form, extra_whole=0):
    rows = _directory(tmp, extra_whole)
    large = _want_rows(rows)
    two = [r for r in rows if r["size"] == 1025][:1] + [r for r in rows if r["size"] == 131072][:1]
    small = _want_rows(two)
    est = sum(16 if r["size"] == 0 or r["status"] else
              (8 + r["size"] + 4096 + 15) // 16 * 16 if r["size"] <= WHOLE_MAX else 57360
              for r in rows)
    facts = {"n": len(rows), "n_small": len(two), "missing": int((large["status"] == -2).sum()),
             "empty": int((large["sizes"] == 0).sum()), "keys": int(large["has"].sum()),
             "checksums": int(large["has32"].sum()), "kinds": sorted(set(large["kind"].tolist())),
             "staged_bytes": est}

    def go(ctx, b):
        from spacedrive_amd import file_identifier as fi
        if form == "files":
            r = fi.identify(b["paths"], b["sizes"], ctx=ctx)
        elif form == "checksum":
            r = fi.identify(b["paths"], b["sizes"], ctx=ctx, checksums=True)
        else:
            r = fi.identify_metadata(b["paths"], b["sizes"], ctx=ctx, checksums=True)
        bad = _ne(r.cas8, b["cas"]) + _ne(r.has_key, b["has"]) + _ne(r.status, b["status"])
        if form != "files":
            bad += _ne(r.checksum32, b["sum"]) + _ne(r.has_checksum, b["has32"])
        if form == "kind":
            bad += _ne(r.kind, b["kind"])
        return bad

    return facts, lambda R: _large_small_large(R, R.context(), go, large, small)


def build_identify_files(tmp):
    return _build_identify(tmp, "files")


def build_identify_checksum_files(tmp):
    return _build_identify(tmp, "checksum")


def build_identify_kind_files(tmp):
    return _build_identify(tmp, "kind")


# A call stages at most max(bytes / SDGPU_SLAB_DIV, 16 MiB) per slab once it
# holds more than 32 MiB, so slabs cycle only past that: 600 more whole files.
MANY_SLABS_EXTRA = 600


def build_identify_checksum_many_slabs(tmp):
    return _build_identify(tmp, "checksum", MANY_SLABS_EXTRA)


def build_identify_kind_many_slabs(tmp):
    return _build_identify(tmp, "kind", MANY_SLABS_EXTRA)


# ---- staged pinned K1 ------------------------------------------------------------

def _stage_batch(seed, lens, misalign_last):
    lens = np.asarray(lens, np.uint32)
    off = np.zeros(lens.size, np.uint64)
    pos = 0
    for i, n in enumerate(lens):
        off[i] = pos
        pos += (min(int(n), CAS_MAX) + 127) // 128 * 128
    if misalign_last:
        off[-1] = off[-2] + 8
    arena = np.random.default_rng(seed).integers(0, 256, pos + 256, dtype=np.uint8)
    valid = _k1_valid(off, lens, arena.size)
    out8 = np.zeros((lens.size, 8), np.uint8)
    out8[valid] = O.cas_batch(arena, off[valid], lens[valid], 4)
    return dict(arena=arena, off=off, ln=lens, valid=valid, out8=out8,
                status=np.where(valid, 0, -22).astype(np.int32))


def build_stage_pinned(tmp):
    # the lengths of test_gpu_stage_link.test_stage_pinned_edge_messages
    large = _stage_batch(5, [0, 1, 1024, 1025, 4096, 4097, 57352, CAS_MAX, CAS_MAX + 1, 64], True)
    small = _stage_batch(6, [3000], False)
    facts = {"status": large["status"].tolist(), "n_small": 1,
             "rejected_ids_zero": not large["out8"][8:].any()}

    def go(ctx, b):
        import torch
        from spacedrive_amd import cas
        h = torch.zeros(b["arena"].size, dtype=torch.uint8).pin_memory()
        h.numpy()[:] = b["arena"]
        out, st = cas.cas_stage_pinned(h, b["off"], b["ln"], ctx=ctx)
        torch.cuda.synchronize()
        return _ne(out.cpu().numpy(), b["out8"]) + _ne(st.cpu().numpy(), b["status"])

    return facts, lambda R: _large_small_large(R, R.context(), go, large, small)


# ---- K7 -------------------------------------------------------------------------

K7_N = 65_537  # 17 scan tiles of 4096 rows, the last one ragged


def _k7_rows(seed, n, with_valid, permute):
    rng = np.random.default_rng(seed)
    key, has, _ = O.synth_dedup_rows(seed, max(n, 2) * 2, max(n // 2, 1), 0, n)
    valid = (rng.random(n) > 0.03).astype(np.uint8) if with_valid else None
    if permute:
        rank = rng.permutation(n).astype(np.uint32)
        key_r, has_r = np.empty_like(key), np.empty_like(has)
        key_r[rank], has_r[rank] = key, has
        rep = O.group_reps(key_r, has_r, 100).astype(np.uint32)[rank]  # grouped in rank order
    else:
        rank = None
        rep = O.group_reps(key, has, 100).astype(np.uint32)
    c, lr, lo = O.link_batch(rep, rank, valid, 0)
    return dict(rep=rep, rank=rank, valid=valid, create=c, lrow=lr, lobj=lo)


def _build_k7(seed, with_valid, permute):
    large = _k7_rows(seed, K7_N, with_valid, permute)
    small = _k7_rows(seed + 1, 1, with_valid, permute)
    facts = {"n": K7_N, "creators": int(large["create"].size), "linked": int(large["lrow"].size),
             "invalid": int((large["valid"] == 0).sum()) if with_valid else 0,
             "rank_is_permutation": bool(permute and np.array_equal(np.sort(large["rank"]),
                                                                    np.arange(K7_N))),
             "rank_is_identity": bool(permute and np.array_equal(large["rank"], np.arange(K7_N)))}

    def go(ctx, b):
        from spacedrive_amd import dedup
        rank = _d(b["rank"].view(np.int32)) if b["rank"] is not None else None
        valid = _d(b["valid"]) if b["valid"] is not None else None
        # the full-length lists: entries past the counts are unspecified
        c, lr, lo, cnt = dedup.link_batch_device(_d(b["rep"].view(np.int32)), rank, valid, 0,
                                                 ctx=ctx, trim=False)
        nc, nl = b["create"].size, b["lrow"].size
        return (_ne(_u32(cnt), [nc, nl]) + _ne(_u32(c)[:nc], b["create"]) +
                _ne(_u32(lr)[:nl], b["lrow"]) + _ne(_u32(lo)[:nl], b["lobj"]))

    return facts, lambda R: _large_small_large(R, R.context(), go, large, small)


def build_k7_implicit(tmp):
    return _build_k7(101, False, False)


def build_k7_valid(tmp):
    return _build_k7(103, True, False)


def build_k7_permuted_ranks(tmp):
    return _build_k7(105, True, True)


# ---- fused write set through an Object index (extra entries) ------------------------

def _extra_rows(seed, n):
    """About 20 % keyless rows, 5 % invalid ones (keyless too), and about 30 %
    of the keyed rows decided by Objects registered before the call."""
    rng = np.random.default_rng(seed)
    pool = rng.integers(0, 2**64 - 1, max(n // 2, 2), dtype=np.uint64, endpoint=True)
    key = pool[rng.integers(0, pool.size, n)]
    valid = (rng.random(n) > 0.05).astype(np.uint8)
    has = ((rng.random(n) > 0.16) & (valid != 0)).astype(np.uint8)
    ek = np.unique(pool[rng.random(pool.size) < 0.3])
    if ek.size == 0:
        ek = pool[:1].copy()
    eh = (rng.permutation(ek.size).astype(np.uint32) * 5 + 7)
    rep = O.group_reps_existing(key, has, 100, ek, eh)
    c, lr, lo = O.link_batch(rep, None, valid, 0)
    o = np.argsort(lr, kind="stable")
    return dict(key=key, has=has, valid=valid, ek=ek, eh=eh, create=np.sort(c), lrow=lr[o],
                lobj=lo[o], by_index=float(((rep & EXISTING) != 0).sum()) / max(int(has.sum()), 1))


def _build_extra(seed, n, unaligned):
    large, small = _extra_rows(seed, n), _extra_rows(seed + 1, 3)
    facts = {"n": n, "keyless": float((large["has"] == 0).mean()),
             "invalid": float((large["valid"] == 0).mean()), "by_index": large["by_index"],
             "invalid_rows_are_keyless": not large["has"][large["valid"] == 0].any()}

    def mask(a):
        import torch
        if not unaligned:
            return _d(a)
        t = torch.zeros(a.size + 1, dtype=torch.uint8, device="cuda")
        t[1:] = _d(a)
        assert t[1:].data_ptr() % 16 == 1
        return t[1:]

    def go(ctx, b):
        from spacedrive_amd import dedup
        # an index of its own per call: the call adds its creators to it
        idx = dedup.ObjectIndex(ctx, 1000)
        idx.add_objects(_d(b["ek"].view(np.int64)), _d(b["eh"].view(np.int32)))
        who, obj, cnt = dedup.group_link_device(_d(b["key"].view(np.int64)), mask(b["has"]),
                                                mask(b["valid"]), None, 0, 100, ctx=ctx,
                                                trim=False, index=idx)
        cnt = _u32(cnt)
        nc, nl = b["create"].size, b["lrow"].size
        bad = _ne(cnt, [nc, nl, nc + nl])
        # the full-length lists: entries past counts[2] are unspecified
        e = min(int(cnt[2]), who.numel())
        c, lr, lo = dedup.split_link_lists(_u32(who)[:e], _u32(obj)[:e])
        bad += _ne(c, b["create"]) + _ne(lr, b["lrow"]) + _ne(lo, b["lobj"])
        idx.close()
        return bad

    return facts, lambda R: _large_small_large(R, R.context(), go, large, small)


def build_extra_4097(tmp):
    return _build_extra(111, 4097, False)


def build_extra_65537_unaligned(tmp):
    return _build_extra(113, 65_537, True)


# ---- consumers --------------------------------------------------------------------

def _orphan_rows(seed, n_obj, n_fp):
    rng = np.random.default_rng(seed)
    objs = rng.permutation(max(n_obj * 2, 1))[:n_obj].astype(np.int32) + 1
    max_id = int(objs.max())
    fp = rng.choice(objs, n_fp).astype(np.int32)
    u = rng.random(n_fp)
    fp[u < 0.10] = -1                                                  # object_id NULL
    past = (u >= 0.10) & (u < 0.15)
    fp[past] = max_id + 1 + rng.integers(0, max_id + 1, int(past.sum()))   # no such Object
    return dict(objs=objs, fp=fp, max_id=max_id, want=O.orphan_objects(objs, fp))


def _build_orphans(trim):
    large, small = _orphan_rows(121, 4097, 9000), _orphan_rows(122, 1, 0)
    facts = {"n_obj": 4097, "n_fp": 9000, "null": int((large["fp"] < 0).sum()),
             "past_max_id": int((large["fp"] > large["max_id"]).sum()),
             "orphans": int(large["want"].size), "small_orphans": small["want"].tolist(),
             "small_ids": small["objs"].tolist()}

    def go(ctx, b):
        from spacedrive_amd import consumers
        args = (_d(b["objs"]), _d(b["fp"]), b["max_id"], ctx)
        if trim:
            return _ne(consumers.orphan_objects(*args).cpu().numpy(), b["want"])
        # the full-length list: entries past the count are unspecified
        out, cnt = consumers.orphan_objects(*args, trim=False)
        return _ne(cnt.cpu().numpy(), [b["want"].size]) + \
            _ne(out.cpu().numpy()[:b["want"].size], b["want"])

    return facts, lambda R: _large_small_large(R, R.context(), go, large, small)


def build_orphans_trim(tmp):
    return _build_orphans(True)


def build_orphans_full(tmp):
    return _build_orphans(False)


def _shard_rows(seed, n):
    rng = np.random.default_rng(seed)
    cas8 = rng.integers(0, 256, (n, 8), dtype=np.uint8)
    valid = (rng.random(n) > 0.05).astype(np.uint8)
    order, counts = O.thumbnail_shards(cas8, valid)
    return dict(cas8=cas8, valid=valid, order=order, counts=counts)


def _build_shards(trim):
    large, small = _shard_rows(125, 10_000), _shard_rows(126, 1)
    facts = {"n": 10_000, "rows_ordered": int(large["counts"].sum()),
             "directories": int((large["counts"] > 0).sum())}

    def go(ctx, b):
        from spacedrive_amd import consumers
        order, counts = consumers.thumbnail_shards(_d(b["cas8"]), _d(b["valid"]), ctx, trim=trim)
        # trim=False: entries of the order past sum(counts) are unspecified
        return _ne(counts.cpu().numpy(), b["counts"]) + \
            _ne(order.cpu().numpy()[:b["order"].size], b["order"])

    return facts, lambda R: _large_small_large(R, R.context(), go, large, small)


def build_thumbnail_shards_trim(tmp):
    return _build_shards(True)


def build_thumbnail_shards_full(tmp):
    return _build_shards(False)


# ---- the Object index -------------------------------------------------------------

def _index_plan(seed, n):
    """Keys (the first one ~0), handles, and the steps' operands."""
    from tests.test_gpu_index_lifecycle import _pool
    rng = np.random.default_rng(seed)
    pool = _pool(seed, n + max(n // 8, 1))
    keys, absent = pool[:n], pool[n:]
    handles = rng.permutation(n).astype(np.uint32) * 2 + 10
    return dict(keys=keys, absent=absent, handles=handles,
                ask=rng.permutation(np.concatenate([keys, absent])))


def build_index(tmp):
    from tests.test_gpu_index_lifecycle import SPECIAL
    large, small = _index_plan(131, 4000), _index_plan(132, 3)
    facts = {"n": 4000, "first_key_is_all_ones": bool(large["keys"][0] == SPECIAL),
             "n_small": 3, "absent": int(large["absent"].size)}

    def go(ctx, p):
        from spacedrive_amd import dedup
        from tests.test_gpu_index_lifecycle import Model, _dk, _dv
        keys, handles, n = p["keys"], p["handles"], p["keys"].size
        idx, m = dedup.ObjectIndex(ctx, 256), Model()      # 1024 slots: grows by rehash
        bad = int(idx.stats()[2] != 1024)
        for a in range(0, n, 1000):
            idx.add_objects(_dk(keys[a:a + 1000]), _dv(handles[a:a + 1000]))
            m.register(keys[a:a + 1000], handles[a:a + 1000])
            bad += int(idx.count() != len(m.d))
        if n > 1000:
            bad += int(idx.stats()[2] <= 1024)
        bad += _ne(_u32(idx.lookup(_dk(p["ask"]))), m.lookup(p["ask"]))
        bad += _ne(idx.lookup(p["ask"]), m.lookup(p["ask"]))                # the host form
        # conditional removal: every other value stale
        some = keys[:max(n // 10, 1)]
        stored = m.lookup(some)
        given = stored.copy()
        given[::2] += 1
        bad += int(idx.remove(_dk(some), _dv(given)) != m.remove(some[1::2]))
        # removal by Object id: present handles, absent ones, a negative one
        hs = np.concatenate([handles[n // 2:n // 2 + max(n // 20, 1)], handles[:5] + 1,
                             [-1]]).astype(np.int32)
        removed = idx.remove_objects(_dv(hs, np.int32), int(handles.max()) + 2)
        bad += int(removed != len(m.remove_handles(hs.tolist())))
        bad += _ne(_u32(idx.lookup(_dk(p["ask"]))), m.lookup(p["ask"]))
        k, v = idx.export()
        got = dict(zip(k.cpu().numpy().view(np.uint64).tolist(), _u32(v).tolist()))
        bad += int(got != m.d) + int(k.numel() != len(m.d)) + int(idx.count() != len(m.d))
        idx.close()
        return bad

    return facts, lambda R: _large_small_large(R, R.context(), go, large, small)


# ---- host-API calls ----------------------------------------------------------------

def _host_rows(seed, n):
    rng = np.random.default_rng(seed)
    pool = rng.integers(0, 2**64 - 1, max(n // 3, 1), dtype=np.uint64, endpoint=True)
    key = pool[rng.integers(0, pool.size, n)]
    has = (rng.random(n) > 0.05).astype(np.uint8)
    ek = np.unique(rng.choice(pool, max(pool.size // 4, 1)))
    eh = rng.permutation(ek.size).astype(np.uint32) + 1
    return dict(key=key, has=has, ek=ek, eh=eh, rep=O.group_reps(key, has, 100),
                rep_existing=O.group_reps_existing(key, has, 100, ek, eh))


def _host_facts(large, small):
    return {"n": int(large["key"].size), "n_small": int(small["key"].size),
            "groups": int(np.unique(large["rep"]).size),
            "linked_to_existing": int(((large["rep_existing"] & EXISTING) != 0).sum())}


def build_host_dedup(tmp):
    large, small = _host_rows(141, 1000), _host_rows(142, 3)

    def go(ctx, b):
        from spacedrive_amd import dedup
        return _ne(dedup.group_reps(b["key"], b["has"], 100, ctx), b["rep"])

    return _host_facts(large, small), lambda R: _large_small_large(R, R.context(), go, large, small)


def build_host_dedup_batch(tmp):
    large, small = _host_rows(143, 1000), _host_rows(144, 3)

    def go(ctx, b):
        from spacedrive_amd import dedup
        bad = _ne(dedup.dedup_batch(b["key"], b["has"], 0, None, 100, ctx), b["rep"])
        idx = dedup.ObjectIndex(ctx, 256)
        idx.add_objects(_d(b["ek"].view(np.int64)), _d(b["eh"].view(np.int32)))
        bad += _ne(dedup.dedup_batch(b["key"], b["has"], 0, idx, 100, ctx), b["rep_existing"])
        idx.close()
        return bad

    return _host_facts(large, small), lambda R: _large_small_large(R, R.context(), go, large, small)


def build_host_dedup_sharded(tmp):
    large, small = _host_rows(145, 1000), _host_rows(146, 3)

    def run(R):
        from spacedrive_amd import dedup
        ctxs = [R.context() for _ in range(3)]
        for b in (large, small, large):
            R.call(lambda b=b: _ne(dedup.dedup_sharded(ctxs, b["key"], b["has"], 100), b["rep"]))

    return _host_facts(large, small), run


# name -> (build, buffers whose poisoning the first call must log; () = the
# entry point has no workspace, only its outputs are poisoned)
SCENARIOS = {
    "k1_bulk": (build_k1_bulk, ("batch_ws",)),
    "k1_body": (build_k1_body, ("batch_ws",)),
    "kind_default": (build_kind_default, ()),
    "kind_verify": (build_kind_verify, ()),
    "tree": (build_tree, ("tree_ws", "plan_pin")),
    "streamed": (build_streamed, ("io_a", "io_b", "pipe_h", "tree_ws")),
    "latency": (build_latency, ("small_ws", "pipe_h")),
    "latency_small_first": (build_latency_small_first, ("pipe_h",)),
    "identify_files": (build_identify_files, ("pipe_h", "pipe_d", "batch_ws")),
    "identify_checksum_files": (build_identify_checksum_files, ("pipe_h", "pipe_d", "batch_ws")),
    "identify_kind_files": (build_identify_kind_files, ("pipe_h", "pipe_d", "batch_ws")),
    "identify_checksum_many_slabs": (build_identify_checksum_many_slabs,
                                     ("pipe_h", "pipe_d", "batch_ws")),
    "identify_kind_many_slabs": (build_identify_kind_many_slabs, ("pipe_h", "pipe_d", "batch_ws")),
    "stage_pinned": (build_stage_pinned, ("stage_meta", "stage_slab", "batch_ws")),
    "k7_implicit": (build_k7_implicit, ("link_ws",)),
    "k7_valid": (build_k7_valid, ("link_ws",)),
    "k7_permuted_ranks": (build_k7_permuted_ranks, ("link_ws",)),
    "extra_4097": (build_extra_4097, ("link_ws", "dedup_ws", "index_table")),
    "extra_65537_unaligned": (build_extra_65537_unaligned, ("link_ws", "dedup_ws", "index_table")),
    "orphans_trim": (build_orphans_trim, ("link_ws",)),
    "orphans_full": (build_orphans_full, ("link_ws",)),
    "thumbnail_shards_trim": (build_thumbnail_shards_trim, ("link_ws",)),
    "thumbnail_shards_full": (build_thumbnail_shards_full, ("link_ws",)),
    "index": (build_index, ("index_table",)),
    "host_dedup": (build_host_dedup, ("dedup_rows", "dedup_ws")),
    "host_dedup_batch": (build_host_dedup_batch, ("dedup_batch_rows", "dedup_ws")),
    "host_dedup_sharded": (build_host_dedup_sharded, ("dedup_sharded_rows",)),
}


# their results are C strings the wrappers make with ctypes: no buffer of the
# wrappers' to poison, the workspaces only
NO_WRAPPER_OUTPUTS = {"streamed", "latency", "latency_small_first"}


def main(names):
    install_output_poison()
    res = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name in names:
            t0 = time.perf_counter()
            _, run = SCENARIOS[name][0](os.path.join(tmp, name))
            t1 = time.perf_counter()
            R, c0 = Run(name), _Count.n
            try:
                run(R)
            finally:
                R.close()
            res[name] = {"bad": R.bad, "outputs_poisoned": _Count.n - c0,
                         "host_seconds": round(t1 - t0, 2),
                         "gpu_seconds": round(time.perf_counter() - t1, 2)}
            print(f"{MARK} {name} end", file=sys.stderr, flush=True)
    print(json.dumps(res), flush=True)


# ---- the parent's side ---------------------------------------------------------------

def parse_log(stderr):
    """{scenario: [[buffer names poisoned during call 0], [call 1], ...]} from
    the child's stderr: the library's lines between the child's markers."""
    calls, cur = {}, None
    for line in stderr.splitlines():
        line = line.strip()
        if line.startswith(MARK):
            f = line.split()
            if f[2] == "call":
                cur = calls.setdefault(f[1], [])
                cur.append([])
            else:
                cur = None
            continue
        m = LOG_RE.match(line)
        if m and cur is not None:
            cur[-1].append(m.group(2))
    return calls


def launch(names, env=None, timeout=240):
    """Runs the scenarios in a fresh process with the knob set: (returncode,
    the child's JSON or None, parse_log of its stderr, its stderr)."""
    e = dict(os.environ, SDGPU_POISON_WS="1")
    e.update(env or {})
    p = subprocess.run([sys.executable, os.path.abspath(__file__)] + list(names),
                       capture_output=True, text=True, timeout=timeout, env=e, cwd=ROOT)
    out = None
    if p.returncode == 0 and p.stdout.strip():
        out = json.loads(p.stdout.strip().splitlines()[-1])
    return p.returncode, out, parse_log(p.stderr), p.stderr


if __name__ == "__main__":
    main(sys.argv[1:])
