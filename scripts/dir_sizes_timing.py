#!/usr/bin/env python3
"""The measurements of the recursive directory sizes; needs a
gfx950 GPU.

Two shapes, every array device-resident, keys random 64-bit, rows in the order
a breadth-first walk gives them (the entries of one directory adjacent):

  tree   12.5 M rows of which 1 M are directories.  The directories are dealt
         breadth first: directory i gets floor(lognormal(MU, SIGMA)) child
         directories (a directory that would end the walk gets one more), the
         files are dealt over the directories with log-normal weights; seed
         SEED.  Sizes are random below 2^40.
  star   12.5 M files in one directory.

Per shape, in one process, alternating within every repeat:

  dir_sizes      sdgpu_dir_sizes_device: parent, total, files, counts in one
                 call (the join on keys included).
  torch_levels   the same totals on the same device by torch: the parent row of
                 every row and the depth of every directory are GIVEN
                 (pre-computed, not timed), files are added to their parents
                 with one index_add_, then one index_add_ per depth level from
                 the deepest up.  It does no join and no cycle handling: the
                 baseline's best case.

and, not alternating, dir_sizes.sizes_oracle on the host over the first
--oracle-rows rows' worth of the same generator (the pure-Python oracle at 12.5 M
rows would take minutes; its rows per second are what is reported).

HIP events around --inner back-to-back calls, a warm-up of every leg, --repeats
repeats.  Before anything is timed the call's totals and parents are compared
with the baseline's inputs and outputs, and the oracle's four outputs with the
call's on its shape.  A disagreement is an error: nothing is written and the
exit status is 1.

    python scripts/dir_sizes_timing.py [--repeats 5] [--out FILE]

Prints one JSON line and writes it to --out
(profiles/dir_sizes/dir_sizes_timing.json).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED = 20240611
MU, SIGMA = 0.0, 1.5          # child directories per directory: floor(lognormal)
FILE_SIGMA = 1.5              # weights of the files per directory
ROWS, DIRS = 12_500_000, 1_000_000


def spread(xs, nd=4):
    return {"median_ms": round(statistics.median(xs), nd), "min_ms": round(min(xs), nd),
            "max_ms": round(max(xs), nd), "spread_ms": round(max(xs) - min(xs), nd)}


def make_tree(n_rows, n_dirs, seed=SEED):
    """Host columns of the tree shape: (dirkey, selfkey, flags, size, parent
    row or -1, depth of directory rows (1 = top level, 0 for files))."""
    import numpy as np
    rng = np.random.default_rng(seed)
    # directory ids 1..n_dirs in breadth-first order, 0 = the location's root
    kids = np.floor(rng.lognormal(MU, SIGMA, n_dirs + 1)).astype(np.int64)
    # ends[i] = the last id among the children of directories 0..i; the walk
    # never runs dry: directory i + 1 must exist once i has been listed
    ends = np.maximum.accumulate(np.maximum(np.cumsum(kids), np.arange(1, n_dirs + 2)))
    ids = np.arange(1, n_dirs + 1)
    dir_parent = np.searchsorted(ends, ids, side="left")          # id of the parent directory
    assert (dir_parent < ids).all()
    # depths in id order: a parent's id is below its children's
    dp = dir_parent.tolist()
    dl = [0] * (n_dirs + 1)
    for k in range(1, n_dirs + 1):
        dl[k] = dl[dp[k - 1]] + 1
    depth = np.array(dl, np.int64)
    n_files = n_rows - n_dirs
    w = rng.lognormal(0.0, FILE_SIGMA, n_dirs + 1)
    file_dir = np.sort(rng.choice(n_dirs + 1, n_files, p=w / w.sum()))
    # rows: the entries of directory 0, then of 1, ... (child directories first)
    owner = np.concatenate([dir_parent, file_dir])                 # directory id that lists the row
    is_dir = np.concatenate([np.ones(n_dirs, np.uint8), np.zeros(n_files, np.uint8)])
    did = np.concatenate([ids, np.zeros(n_files, np.int64)])       # a directory row's own id
    order = np.argsort(owner, kind="stable")
    owner, is_dir, did = owner[order], is_dir[order], did[order]
    key = rng.integers(1, (1 << 64) - 1, n_dirs + 1, dtype=np.uint64)
    row_of_dir = np.full(n_dirs + 1, -1, np.int64)
    row_of_dir[did[is_dir == 1]] = np.flatnonzero(is_dir == 1)
    size = np.where(is_dir == 1, 0, rng.integers(0, 1 << 40, n_rows)).astype(np.uint64)
    return (key[owner], np.where(is_dir == 1, key[did], 0).astype(np.uint64), is_dir, size,
            row_of_dir[owner], np.where(is_dir == 1, depth[did], 0))


def make_star(n_rows):
    import numpy as np
    rng = np.random.default_rng(SEED + 1)
    key = rng.integers(1, (1 << 64) - 1, 2, dtype=np.uint64)
    is_dir = np.zeros(n_rows, np.uint8)
    is_dir[0] = 1
    dirkey = np.full(n_rows, key[1], np.uint64)
    dirkey[0] = key[0]
    selfkey = np.zeros(n_rows, np.uint64)
    selfkey[0] = key[1]
    size = rng.integers(0, 1 << 40, n_rows).astype(np.uint64)
    size[0] = 0
    parent = np.zeros(n_rows, np.int64)
    parent[0] = -1
    depth = np.zeros(n_rows, np.int64)
    depth[0] = 1
    return dirkey, selfkey, is_dir, size, parent, depth


def measure(ctx, name, cols, repeats, warmup, inner):
    import numpy as np
    import torch
    from spacedrive_amd._native import check
    dev = torch.device("cuda", ctx.device)
    up = lambda a: torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(dev)  # noqa: E731
    dirkey, selfkey, flags, size, want_parent, depth = (up(c) for c in cols)
    n = dirkey.numel()
    lib, s = ctx.lib, torch.cuda.current_stream(dev).cuda_stream
    parent = torch.empty(n, dtype=torch.int32, device=dev)
    total = torch.empty(n, dtype=torch.int64, device=dev)
    files = torch.empty(n, dtype=torch.int32, device=dev)
    counts = torch.empty(4, dtype=torch.int64, device=dev)
    # the baseline's givens
    is_file = flags == 0
    file_rows = torch.nonzero(is_file & (want_parent >= 0)).flatten()
    file_parent = want_parent[file_rows]
    file_size = size[file_rows]
    levels = []
    for d in range(int(depth.max().item()), 1, -1):
        rows = torch.nonzero(depth == d).flatten()
        levels.append((rows, want_parent[rows]))
    base_total = torch.empty(n, dtype=torch.int64, device=dev)

    def dir_sizes():
        check(lib.sdgpu_dir_sizes_device(ctx.h, dirkey.data_ptr(), selfkey.data_ptr(),
                                         flags.data_ptr(), size.data_ptr(), n, parent.data_ptr(),
                                         total.data_ptr(), files.data_ptr(), counts.data_ptr(), s))

    def torch_levels():
        base_total.copy_(size)
        base_total.index_add_(0, file_parent, file_size)
        for rows, par in levels:
            base_total.index_add_(0, par, base_total[rows])

    # every result checked equal before it is timed
    dir_sizes()
    torch_levels()
    torch.cuda.synchronize()
    c = counts.cpu().numpy().view(np.uint64).tolist()
    top = want_parent < 0
    same = (bool(torch.equal(parent.to(torch.int64), want_parent))    # MISS reads as -1
            and bool(torch.equal(total, base_total)) and c[0] == c[1] == int((flags != 0).sum())
            and c[2] == int(top.sum())
            and c[3] == int(base_total[top].sum().item()) & ((1 << 64) - 1))
    if not same:
        raise SystemExit(f"{name}: the call's outputs differ from the torch baseline's")
    legs = {"dir_sizes": dir_sizes, "torch_levels": torch_levels}
    ms = {k: [] for k in legs}
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for it in range(warmup + repeats):
        for k, fn in legs.items():
            a.record()
            for _ in range(inner):
                fn()
            b.record()
            b.synchronize()
            if it >= warmup:
                ms[k].append(a.elapsed_time(b) / inner)
    out = {"rows": n, "directories": c[0], "depth_levels": int(depth.max().item()),
           "location_bytes": c[3], "repeats": repeats, "inner_calls": inner,
           "baseline_agrees": same}
    for k, xs in ms.items():
        out[k] = spread(xs)
    out["dir_sizes_over_torch_levels"] = round(out["dir_sizes"]["median_ms"]
                                               / out["torch_levels"]["median_ms"], 3)
    ctx.set_timing(True)
    dir_sizes()
    torch.cuda.synchronize()
    out["dir_sizes_kernels_ms"] = {k: round(v[0], 4) for k, v in sorted(ctx.kernel_times().items())}
    ctx.set_timing(False)
    return out


def oracle_leg(ctx, n_rows, n_dirs):
    """sizes_oracle on the host, checked against the call on the same rows."""
    import numpy as np
    from spacedrive_amd import dir_sizes as D
    cols = make_tree(n_rows, n_dirs)[:4]
    t0 = time.perf_counter()
    want = D.sizes_oracle(*cols)
    dt = time.perf_counter() - t0
    got = D.sizes_host(*cols, ctx=ctx)
    if not all(np.array_equal(g, w) for g, w in zip(got, want)):
        raise SystemExit("oracle: the call's outputs differ from sizes_oracle's")
    return {"rows": n_rows, "directories": n_dirs, "seconds": round(dt, 3),
            "rows_per_second": round(n_rows / dt), "call_agrees": True}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--oracle-rows", type=int, default=1_250_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dir_sizes",
                                                  "dir_sizes_timing.json"))
    ap.add_argument("--scale", type=float, default=1.0,
                    help="shrinks every shape (a rehearsal, not a measurement)")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured here")
    from spacedrive_amd._native import default_context
    ctx = default_context(0)
    rows, dirs = max(int(ROWS * a.scale), 1000), max(int(DIRS * a.scale), 80)
    out = {"device": torch.cuda.get_device_name(0), "scale": a.scale, "seed": SEED,
           "fanout_lognormal": [MU, SIGMA], "file_weight_sigma": FILE_SIGMA}
    out["tree"] = measure(ctx, "tree", make_tree(rows, dirs), a.repeats, a.warmup, a.inner)
    torch.cuda.empty_cache()
    out["star"] = measure(ctx, "star", make_star(rows), a.repeats, a.warmup, a.inner)
    torch.cuda.empty_cache()
    out["star_over_tree"] = round(out["star"]["dir_sizes"]["median_ms"]
                                  / out["tree"]["dir_sizes"]["median_ms"], 3)
    o_rows = max(int(a.oracle_rows * a.scale), 1000)
    out["sizes_oracle_host"] = oracle_leg(ctx, o_rows, max(o_rows * DIRS // ROWS, 80))
    text = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
