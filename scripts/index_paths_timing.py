#!/usr/bin/env python3
"""Device times of the EXISTING paths through the Object index -- the probe and
the creators' insert of a two-batch grouping, plain and fused -- for comparing
two builds of the library (e.g. a checkout of the parent commit and this
tree): run it once per build, alternating, in the same session.

    python scripts/index_paths_timing.py [--root DIR] [--rows 12500000] [--repeats 10]

--root: the checkout whose spacedrive_amd package (and built libsdgpu.so) is
loaded; default: this tree.  Prints one JSON line with the median and the
min..max of every timed kernel.  Needs a gfx950 GPU.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--rows", type=int, default=12_500_000)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    import torch
    from spacedrive_amd import dedup
    from spacedrive_amd._native import default_context
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured here")
    ctx = default_context(0)
    n = a.rows
    g = torch.Generator(device="cuda").manual_seed(2)
    # two batches over one pool of n keys: the second links about 2/3 of its rows
    pool = torch.randint(-2**63, 2**63 - 1, (n,), dtype=torch.int64, device="cuda", generator=g)
    pick = torch.randint(0, n, (2 * n,), device="cuda", generator=g)
    key = pool[pick]
    del pick
    rank = torch.arange(2 * n, dtype=torch.int32, device="cuda")
    idx = dedup.ObjectIndex(ctx, 4 * n)
    names = ("index_probe", "index_insert")
    samples = {"plain": {k: [] for k in names}, "fused": {k: [] for k in names}}

    def run(kind):
        idx.clear()
        ctx.set_timing(True)
        for b in range(2):
            k, r = key[b * n:(b + 1) * n], rank[b * n:(b + 1) * n]
            if kind == "plain":
                dedup.group_rows_indexed(k, None, r, idx, 100)
            else:
                dedup.group_link_device(k, None, None, None, b * n, 100, ctx=ctx, trim=False,
                                        index=idx)
        torch.cuda.synchronize()
        t = ctx.kernel_times()
        return {k: t[k][0] / t[k][1] for k in names}

    for i in range(a.warmup + a.repeats):
        for kind in samples:
            t = run(kind)
            if i >= a.warmup:
                for k in names:
                    samples[kind][k].append(t[k])
    out = {"root": os.path.abspath(a.root), "rows_per_batch": n, "repeats": a.repeats,
           "index_keys": idx.count()}
    for kind, d in samples.items():
        out[kind] = {k: {"median_ms": round(statistics.median(xs), 4), "min_ms": round(min(xs), 4),
                         "max_ms": round(max(xs), 4)} for k, xs in d.items()}
    print(json.dumps(out))
    idx.close()


if __name__ == "__main__":
    main()
