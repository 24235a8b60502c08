#!/usr/bin/env python3
"""The measurements of the stale-thumbnail anti-join; needs a
gfx950 GPU.

Per shape (thumbnails x file_path rows in one or two libraries, every array
device-resident, keys random, one row in 1000 without a cas_id, a tenth of the
thumbnails owned by no row), in one process, alternating within every repeat:

  stale_call    thumbnail_remover.stale_thumbnails (trim=False: no host
                synchronisation inside): a table of the THUMBNAILS, the
                file_path columns streamed once.
  index_route   what the same question costs without it: compact the keyed
                rows of every library, ObjectIndex.add_objects over them (a
                table of the LIBRARY), lookup of the thumbnails, the misses'
                positions.  The index is created once and cleared per call,
                so the route pays no allocation in the timed calls.

HIP events around each call, a warm-up of both, the median and min..max of
--repeats calls.  The two routes' stale sets are compared (not timed).  The
new call's algorithmic bytes -- 9 B per file_path row, 8 B per thumbnail, 4 B
per stale position and per directory offset -- are given as a share of the
8 TB/s HBM figure DESIGN.md uses.

    python scripts/stale_thumbnails_timing.py [--repeats 9] [--out FILE]

Prints one JSON line and writes it to --out
(profiles/thumbnail_remover/stale_timing.json).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [("1M_thumbs_12.5M_rows_1_library", 1_000_000, [12_500_000]),
          ("1M_thumbs_100M_rows_2_libraries", 1_000_000, [50_000_000, 50_000_000]),
          ("100k_thumbs_1M_rows_1_library", 100_000, [1_000_000])]
N_DIRS = 256
HBM_BYTES_PER_S = 8e12


def spread(xs, nd=4):
    return {"median_ms": round(statistics.median(xs), nd), "min_ms": round(min(xs), nd),
            "max_ms": round(max(xs), nd)}


def make_shape(n_thumbs, lib_rows, dev, seed):
    import torch
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    lo, hi = -(2**63), 2**63 - 1
    thumbs = torch.randint(lo, hi, (n_thumbs,), dtype=torch.int64, device=dev, generator=g)
    start = (torch.arange(N_DIRS + 1, dtype=torch.int64, device=dev) * n_thumbs // N_DIRS) \
        .to(torch.int32)
    owned = thumbs[: n_thumbs * 9 // 10]
    libs = []
    for rows in lib_rows:
        key = torch.randint(lo, hi, (rows,), dtype=torch.int64, device=dev, generator=g)
        pick = torch.randint(0, owned.numel(), (rows,), dtype=torch.int64, device=dev, generator=g)
        mine = torch.rand(rows, device=dev, generator=g) < 0.3     # rows whose file has a thumbnail
        key = torch.where(mine, owned[pick], key)
        has = (torch.rand(rows, device=dev, generator=g) >= 0.001).to(torch.uint8)
        libs.append((key, has))
    return thumbs, start, libs


def measure(ctx, name, n_thumbs, lib_rows, repeats, warmup):
    import torch
    from spacedrive_amd import dedup
    from spacedrive_amd import thumbnail_remover as T
    from spacedrive_amd._native import INDEX_MISS
    dev = torch.device("cuda", ctx.device)
    thumbs, start, libs = make_shape(n_thumbs, lib_rows, dev, seed=len(lib_rows) + n_thumbs)
    index = dedup.ObjectIndex(ctx)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def stale_call():
        return T.stale_thumbnails(thumbs, start, libs, ctx, trim=False)

    def index_route():
        index.clear(stream)
        for key, has in libs:
            keyed = key[has != 0]
            index.add_objects(keyed, torch.arange(keyed.numel(), dtype=torch.int32, device=dev))
        value = index.lookup(thumbs)
        return torch.nonzero(value == INDEX_MISS - (1 << 32)).flatten()   # int32 view of the miss

    legs = {"stale_call": stale_call, "index_route": index_route}
    ms = {k: [] for k in legs}
    for it in range(warmup + repeats):
        for k, fn in legs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if it >= warmup:
                ms[k].append(a.elapsed_time(b))
    stale, s = stale_call()
    total = int(s[-1].item())
    same = bool(torch.equal(stale[:total].to(torch.int64), index_route()))
    rows = sum(lib_rows)
    algo = 9 * rows + 8 * n_thumbs + 4 * total + 4 * (N_DIRS + 1)
    out = {"thumbnails": n_thumbs, "file_path_rows": rows, "libraries": len(lib_rows),
           "directories": N_DIRS, "stale": total, "repeats": repeats,
           "routes_agree": same, "algorithmic_bytes": algo}
    for k, xs in ms.items():
        out[k] = spread(xs)
    med = out["stale_call"]["median_ms"]
    out["stale_call_GB_per_s"] = round(algo / med / 1e6, 1)
    out["stale_call_share_of_8TBps"] = round(algo / (med * 1e-3) / HBM_BYTES_PER_S, 4)
    out["index_route_over_stale_call"] = round(out["index_route"]["median_ms"] / med, 2)
    index.close()
    del thumbs, start, libs
    torch.cuda.empty_cache()
    return name, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "thumbnail_remover",
                                                  "stale_timing.json"))
    ap.add_argument("--scale", type=float, default=1.0,
                    help="shrinks every shape (a rehearsal, not a measurement)")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured here")
    from spacedrive_amd._native import default_context
    ctx = default_context(0)
    out = {"device": torch.cuda.get_device_name(0), "scale": a.scale}
    for name, n_thumbs, lib_rows in SHAPES:
        k, v = measure(ctx, name, max(int(n_thumbs * a.scale), 1),
                       [max(int(r * a.scale), 1) for r in lib_rows], a.repeats, a.warmup)
        out[k] = v
    text = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
