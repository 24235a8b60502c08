#!/usr/bin/env python3
"""The measurements of the thumbnailer's work list; needs a
gfx950 GPU.

Per shape (thumbnails x file_path rows, every array device-resident, keys
random, 30 % of the rows carrying the key of a thumbnail, 20 % of the rows
copies of another row's key, one row in 1000 without a cas_id, one in 20
ineligible), in one process, alternating within every repeat:

  worklist       sdgpu_thumbnail_worklist_device: present, work, dir_start,
                 stats in one call.
  presence_only  the same entry point with work and dir_start NULL.
  yardstick      the three existing calls the work list is built from, on the
                 same arrays: sdgpu_stale_thumbnails_device over the column
                 (table build + probe + compaction), sdgpu_group_rows_device
                 on the candidate mask with chunk_rows = 1, and
                 sdgpu_thumbnail_shards_device on the work mask.  Their sum per
                 repeat is the yardstick; its spread is max - min of that sum
                 over the repeats.

HIP events around --inner back-to-back calls of a leg (every output buffer
allocated beforehand), a warm-up of every leg, --repeats repeats.  The work
list of the call is compared with the one the three calls' outputs imply (not
timed).  Beside it, the reference's cost per row: --stats `os.stat` calls on a
warm cache directory of that many thumbnails, on the host.

    python scripts/thumbnailer_timing.py [--repeats 5] [--out FILE]

Prints one JSON line and writes it to --out
(profiles/thumbnailer/thumbnailer_timing.json).
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [("1M_thumbs_12.5M_rows", 1_000_000, 12_500_000),
          ("100k_thumbs_1M_rows", 100_000, 1_000_000)]


def spread(xs, nd=4):
    return {"median_ms": round(statistics.median(xs), nd), "min_ms": round(min(xs), nd),
            "max_ms": round(max(xs), nd), "spread_ms": round(max(xs) - min(xs), nd)}


def make_shape(n_thumbs, rows, dev, seed):
    import torch
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    lo, hi = -(2**63), 2**63 - 1
    rnd = lambda n: torch.rand(n, device=dev, generator=g)  # noqa: E731
    thumbs = torch.randint(lo, hi, (n_thumbs,), dtype=torch.int64, device=dev, generator=g)
    key = torch.randint(lo, hi, (rows,), dtype=torch.int64, device=dev, generator=g)
    pick = torch.randint(0, n_thumbs, (rows,), dtype=torch.int64, device=dev, generator=g)
    key = torch.where(rnd(rows) < 0.3, thumbs[pick], key)           # the thumbnail exists
    other = torch.randint(0, rows, (rows,), dtype=torch.int64, device=dev, generator=g)
    key = torch.where(rnd(rows) < 0.2, key[other], key)             # a copy of another row
    has = (rnd(rows) >= 0.001).to(torch.uint8)
    elig = (rnd(rows) >= 0.05).to(torch.uint8)
    return thumbs, key, has, elig


def measure(ctx, name, n_thumbs, rows, repeats, warmup, inner):
    import torch
    from spacedrive_amd._native import check
    dev = torch.device("cuda", ctx.device)
    thumbs, key, has, elig = make_shape(n_thumbs, rows, dev, seed=n_thumbs + rows)
    lib, s = ctx.lib, torch.cuda.current_stream(dev).cuda_stream
    i32 = lambda n: torch.empty(n, dtype=torch.int32, device=dev)  # noqa: E731
    present = torch.empty(rows, dtype=torch.uint8, device=dev)
    work, start, stats = i32(rows), i32(257), i32(4)
    p_present, p_stats = torch.empty_like(present), i32(4)
    # the yardstick's arrays
    dirs = (torch.arange(257, dtype=torch.int64, device=dev) * n_thumbs // 256).to(torch.int32)
    stale, stale_start = i32(n_thumbs), i32(257)
    col_key = (ctypes.c_void_p * 1)(key.data_ptr())
    col_has = (ctypes.c_void_p * 1)(has.data_ptr())
    col_rows = (ctypes.c_uint64 * 1)(rows)
    rep, order, counts = i32(rows), i32(rows), i32(256)

    def worklist():
        check(lib.sdgpu_thumbnail_worklist_device(
            ctx.h, thumbs.data_ptr(), n_thumbs, key.data_ptr(), has.data_ptr(), elig.data_ptr(),
            rows, 0, present.data_ptr(), work.data_ptr(), start.data_ptr(), stats.data_ptr(), s))

    def presence_only():
        check(lib.sdgpu_thumbnail_worklist_device(
            ctx.h, thumbs.data_ptr(), n_thumbs, key.data_ptr(), has.data_ptr(), None, rows, 0,
            p_present.data_ptr(), None, None, p_stats.data_ptr(), s))

    worklist()
    torch.cuda.synchronize()
    cand = ((has != 0) & (elig != 0) & (present == 0)).to(torch.uint8)
    w = int(stats[3].item())
    mask = torch.zeros(rows, dtype=torch.uint8, device=dev)
    mask[work[:w].to(torch.int64)] = 1

    def stale_call():
        check(lib.sdgpu_stale_thumbnails_device(
            ctx.h, thumbs.data_ptr(), n_thumbs, dirs.data_ptr(), 256, col_key, col_has, col_rows,
            1, stale.data_ptr(), stale_start.data_ptr(), s))

    def group_call():
        check(lib.sdgpu_group_rows_device(ctx.h, key.data_ptr(), cand.data_ptr(), None, rows, 1, 0,
                                          rep.data_ptr(), s))

    def shards_call():
        check(lib.sdgpu_thumbnail_shards_device(ctx.h, key.data_ptr(), mask.data_ptr(), rows,
                                                order.data_ptr(), counts.data_ptr(), s))

    legs = {"worklist": worklist, "presence_only": presence_only, "stale_thumbnails": stale_call,
            "group_rows": group_call, "thumbnail_shards": shards_call}
    ms = {k: [] for k in legs}
    for it in range(warmup + repeats):
        for k, fn in legs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                fn()
            b.record()
            b.synchronize()
            if it >= warmup:
                ms[k].append(a.elapsed_time(b) / inner)
    # the three calls' outputs imply the same work list (not timed)
    idx = torch.arange(rows, dtype=torch.int32, device=dev)
    implied = ((cand != 0) & (rep == idx)).to(torch.uint8)
    same = bool(torch.equal(implied, mask)) and bool(torch.equal(order[:w], work[:w])) and \
        int(counts.sum().item()) == w and bool(torch.equal(p_present, present))
    yard = [a + b + c for a, b, c in zip(ms["stale_thumbnails"], ms["group_rows"],
                                         ms["thumbnail_shards"])]
    out = {"thumbnails": n_thumbs, "file_path_rows": rows, "repeats": repeats, "inner_calls": inner,
           "stats": [int(x) for x in stats.cpu().tolist()], "yardstick_agrees": same}
    for k, xs in ms.items():
        out[k] = spread(xs)
    out["yardstick_sum"] = spread(yard)
    wl, ys = out["worklist"]["median_ms"], out["yardstick_sum"]
    out["worklist_minus_yardstick_ms"] = round(wl - ys["median_ms"], 4)
    out["within_sum_plus_spread"] = bool(wl <= ys["median_ms"] + ys["spread_ms"])
    ctx.set_timing(True)
    worklist()
    torch.cuda.synchronize()
    out["worklist_kernels_ms"] = {k: round(v[0], 4) for k, v in sorted(ctx.kernel_times().items())}
    ctx.set_timing(False)
    del thumbs, key, has, elig
    torch.cuda.empty_cache()
    return name, out


def host_stats(n):
    """n os.stat calls on a warm cache directory holding n thumbnails in their
    shard directories (a third of the paths asked for do not exist)."""
    import numpy as np
    rng = np.random.default_rng(1)
    ids = ["%016x" % int(k) for k in rng.integers(0, 2**63, n, dtype=np.uint64)]
    with tempfile.TemporaryDirectory() as base:
        for d in range(256):
            os.mkdir(os.path.join(base, "%02x" % d))
        paths = [os.path.join(base, c[:2], c + ".webp") for c in ids]
        for i, p in enumerate(paths):
            if i % 3:
                open(p, "wb").close()
        best = None
        for _ in range(3):
            t0 = time.perf_counter()
            found = 0
            for p in paths:
                try:
                    os.stat(p)
                    found += 1
                except FileNotFoundError:
                    pass
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
    return {"stats": n, "found": found, "best_of_3_ms": round(best * 1e3, 2),
            "us_per_stat": round(best * 1e6 / n, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--stats", type=int, default=100_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "thumbnailer",
                                                  "thumbnailer_timing.json"))
    ap.add_argument("--scale", type=float, default=1.0,
                    help="shrinks every shape (a rehearsal, not a measurement)")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured here")
    from spacedrive_amd._native import default_context
    ctx = default_context(0)
    out = {"device": torch.cuda.get_device_name(0), "scale": a.scale}
    for name, n_thumbs, rows in SHAPES:
        k, v = measure(ctx, name, max(int(n_thumbs * a.scale), 1), max(int(rows * a.scale), 1),
                       a.repeats, a.warmup, a.inner)
        out[k] = v
    out["host_os_stat"] = host_stats(max(int(a.stats * a.scale), 1))
    text = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
