#!/usr/bin/env python3
"""The measurements of the indexer's rescan diff; needs a
gfx950 GPU.

Two shapes, every array device-resident, keys random, the rows of a directory
adjacent (100 rows per directory):

  full_rescan      12.5 M rows x 12.5 M walked entries, every directory walked:
                   1 % of the entries new, 1 % changed (inode), 1 % of the rows
                   gone from disk.
  subtree_rescan   12.5 M rows x 100 k walked entries in 1 000 directories, the
                   same three per cent inside the sub-tree.

Per shape, in one process, alternating within every repeat:

  diff             sdgpu_indexer_diff_device: match, state, create, update,
                   remove, counts in one call.
  index_match      the match leg by existing calls on the same arrays:
                   sdgpu_index_add_objects_device (handle = row index) into an
                   empty index + sdgpu_index_lookup_device of the walked keys.
                   The index is cleared before every call, outside the events:
                   this leg is timed call by call, not back to back.
  index_clear      sdgpu_index_clear alone, beside it (the diff clears its own
                   table in every call; the yardstick does not count a clear).
  stale_antijoin   the anti-join leg: sdgpu_stale_thumbnails_device with the rows
                   as "thumbnails" and the walked keys as one column.

The yardstick is the sum of the two legs per repeat; its spread is max - min of
that sum over the repeats.  HIP events around --inner back-to-back calls of a
leg (every output buffer allocated beforehand), a warm-up of every leg,
--repeats repeats.  The outputs of the diff are compared with what the two
legs' outputs imply (not timed): match from the lookup's values, remove from
the stale positions that lie in a walked directory.  A disagreement is an
error: nothing is written and the exit status is 1.

    python scripts/indexer_diff_timing.py [--repeats 5] [--out FILE]

Prints one JSON line and writes it to --out
(profiles/indexer_diff/indexer_diff_timing.json).
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PER_DIR = 100
SHAPES = [("full_rescan", 12_500_000, None), ("subtree_rescan", 12_500_000, 1000)]
MISS = 0xFFFFFFFF


def spread(xs, nd=4):
    return {"median_ms": round(statistics.median(xs), nd), "min_ms": round(min(xs), nd),
            "max_ms": round(max(xs), nd), "spread_ms": round(max(xs) - min(xs), nd)}


def make_shape(n_r, walked_dirs, dev, seed):
    """Rows in n_r / 100 directories; the walk covers the first `walked_dirs`
    of them (None: all).  Of the covered rows 1 % are gone from disk, 1 % of
    the entries are new, 1 % have another inode."""
    import torch
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    lo, hi = -(2**63), 2**63 - 1
    rnd = lambda n: torch.rand(n, device=dev, generator=g)  # noqa: E731
    keys = lambda n: torch.randint(lo, hi, (n,), dtype=torch.int64, device=dev, generator=g)  # noqa: E731
    n_dirs = (n_r + PER_DIR - 1) // PER_DIR
    r_key = keys(n_r)
    dir_key = keys(n_dirs)
    r_dirkey = dir_key[torch.arange(n_r, device=dev) // PER_DIR]
    r_flags = (rnd(n_r) < 0.1).to(torch.uint8)
    r_meta = torch.randint(0, 2**40, (n_r, 3), dtype=torch.int64, device=dev, generator=g)
    n_wd = n_dirs if walked_dirs is None else min(walked_dirs, n_dirs)
    covered = min(n_wd * PER_DIR, n_r)
    on_disk = torch.nonzero(rnd(covered) >= 0.01).flatten()          # 1 % gone
    n_new = max(covered // 100, 1)
    w_key = torch.cat([r_key[on_disk], keys(n_new)])
    w_flags = torch.cat([r_flags[on_disk], torch.zeros(n_new, dtype=torch.uint8, device=dev)])
    w_meta = torch.cat([r_meta[on_disk], torch.zeros((n_new, 3), dtype=torch.int64, device=dev)])
    w_meta[:, 0] += (rnd(w_key.numel()) < 0.01).to(torch.int64)      # 1 % another inode
    order = torch.randperm(w_key.numel(), device=dev, generator=g)   # walk order is not id order
    w_key, w_flags, w_meta = w_key[order], w_flags[order], w_meta[order].contiguous()
    return w_key, w_flags, w_meta, dir_key[:n_wd].contiguous(), r_key, r_dirkey, r_flags, r_meta


def measure(ctx, name, n_r, walked_dirs, repeats, warmup, inner):
    import torch
    from spacedrive_amd._native import check
    from spacedrive_amd.dedup import ObjectIndex
    dev = torch.device("cuda", ctx.device)
    cols = make_shape(n_r, walked_dirs, dev, seed=n_r + (walked_dirs or 0))
    w_key, w_flags, w_meta, wd_key, r_key, r_dirkey, r_flags, r_meta = cols
    n_w, n_wd = w_key.numel(), wd_key.numel()
    lib, s = ctx.lib, torch.cuda.current_stream(dev).cuda_stream
    i32 = lambda n: torch.empty(max(n, 1), dtype=torch.int32, device=dev)  # noqa: E731
    match, create, update, remove, counts = i32(n_w), i32(n_w), i32(n_w), i32(n_r), i32(4)
    state = torch.empty(n_w, dtype=torch.uint8, device=dev)
    # the yardstick's arrays
    index = ObjectIndex(ctx, capacity=2 * n_r)
    handle = torch.arange(n_r, dtype=torch.int32, device=dev)
    value = i32(n_w)
    dirs = (torch.arange(257, dtype=torch.int64, device=dev) * n_r // 256).to(torch.int32)
    stale, stale_start = i32(n_r), i32(257)
    col_key = (ctypes.c_void_p * 1)(w_key.data_ptr())
    col_rows = (ctypes.c_uint64 * 1)(n_w)

    def diff():
        check(lib.sdgpu_indexer_diff_device(
            ctx.h, w_key.data_ptr(), w_flags.data_ptr(), w_meta.data_ptr(), n_w, wd_key.data_ptr(),
            n_wd, r_key.data_ptr(), r_dirkey.data_ptr(), r_flags.data_ptr(), r_meta.data_ptr(),
            n_r, match.data_ptr(), state.data_ptr(), create.data_ptr(), update.data_ptr(),
            remove.data_ptr(), counts.data_ptr(), s))

    def index_match():
        check(lib.sdgpu_index_add_objects_device(index.h, r_key.data_ptr(), handle.data_ptr(), n_r,
                                                 1, 0, s))
        check(lib.sdgpu_index_lookup_device(index.h, w_key.data_ptr(), n_w, value.data_ptr(), s))

    def stale_antijoin():
        check(lib.sdgpu_stale_thumbnails_device(
            ctx.h, r_key.data_ptr(), n_r, dirs.data_ptr(), 256, col_key, None, col_rows, 1,
            stale.data_ptr(), stale_start.data_ptr(), s))

    def index_clear():
        check(lib.sdgpu_index_clear(index.h, s))

    legs = {"diff": diff, "index_match": index_match, "stale_antijoin": stale_antijoin,
            "index_clear": index_clear}
    ms = {k: [] for k in legs}
    def timed(fn, before=None):
        """Mean ms of `inner` calls: back to back between two events, or, with
        `before`, call by call with `before()` outside the events."""
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        if before is None:
            a.record()
            for _ in range(inner):
                fn()
            b.record()
            b.synchronize()
            return a.elapsed_time(b) / inner
        total = 0.0
        for _ in range(inner):
            before()
            a.record()
            fn()
            b.record()
            b.synchronize()
            total += a.elapsed_time(b)
        return total / inner

    for it in range(warmup + repeats):
        for k, fn in legs.items():
            t = timed(fn, index_clear if k == "index_match" else None)
            if it >= warmup:
                ms[k].append(t)
    # what the two legs imply (not timed)
    c = [int(x) for x in counts.cpu().tolist()]
    implied_match = torch.where(value == -1, value, value & 0x7FFFFFFF)
    n_stale = int(stale_start[256].item())
    st = stale[:n_stale].to(torch.int64)
    implied_remove = st[torch.isin(r_dirkey[st], wd_key)].to(torch.int32)
    same = bool(torch.equal(implied_match, match[:n_w])) and \
        bool(torch.equal(implied_remove, remove[:c[2]])) and \
        c[0] == int(((state == 0) | (state == 3)).sum().item()) and \
        c[1] == int((state == 2).sum().item())
    yard = [a + b for a, b in zip(ms["index_match"], ms["stale_antijoin"])]
    out = {"file_path_rows": n_r, "walked_entries": n_w, "walked_directories": n_wd,
           "repeats": repeats, "inner_calls": inner, "counts": c, "yardstick_agrees": same}
    for k, xs in ms.items():
        out[k] = spread(xs)
    out["yardstick_sum"] = spread(yard)
    d, ys = out["diff"]["median_ms"], out["yardstick_sum"]
    out["diff_minus_yardstick_ms"] = round(d - ys["median_ms"], 4)
    out["within_sum_plus_spread"] = bool(d <= ys["median_ms"] + ys["spread_ms"])
    ctx.set_timing(True)
    diff()
    torch.cuda.synchronize()
    out["diff_kernels_ms"] = {k: round(v[0], 4) for k, v in sorted(ctx.kernel_times().items())}
    ctx.set_timing(False)
    index.close()
    if not same:
        raise SystemExit(f"{name}: the diff's outputs differ from what the yardstick legs imply")
    del cols, w_key, w_flags, w_meta, wd_key, r_key, r_dirkey, r_flags, r_meta
    torch.cuda.empty_cache()
    return name, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "indexer_diff",
                                                  "indexer_diff_timing.json"))
    ap.add_argument("--scale", type=float, default=1.0,
                    help="shrinks every shape (a rehearsal, not a measurement)")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured here")
    from spacedrive_amd._native import default_context
    ctx = default_context(0)
    out = {"device": torch.cuda.get_device_name(0), "scale": a.scale}
    for name, n_r, walked_dirs in SHAPES:
        k, v = measure(ctx, name, max(int(n_r * a.scale), PER_DIR), walked_dirs, a.repeats,
                       a.warmup, a.inner)
        out[k] = v
    text = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
