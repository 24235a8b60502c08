#!/usr/bin/env python3
"""Device times of the library-lifetime Object index calls (index
section): index_lookup against index_probe on the same index and the same
keys, and the one-pass calls (remove_objects, export) as ms and as a share of
HBM bandwidth on capacity x 16 bytes.  Kernel times come from the library's
own event timers (sdgpu_set_timing); needs a gfx950 GPU.

    python scripts/index_lifecycle_timing.py [--rows 12500000] [--repeats 20]

Prints one JSON line.  lookup and probe alternate inside every repeat, so
drift hits both alike; medians and the min..max spread are reported.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_BYTES_PER_S = 8.0e12  # MI355X peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=12_500_000)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import torch
    from spacedrive_amd import dedup
    from spacedrive_amd._native import default_context
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured here")
    ctx = default_context(0)
    n = a.rows
    g = torch.Generator(device="cuda").manual_seed(1)
    key = torch.randint(-2**63, 2**63 - 1, (n,), dtype=torch.int64, device="cuda", generator=g)
    handle = torch.arange(n, dtype=torch.int32, device="cuda")
    # 2n: the groupings below reserve n more keys each and must not rebuild the table
    idx = dedup.ObjectIndex(ctx, 2 * n)
    idx.add_objects(key, handle)
    live, used, cap = idx.stats()

    def timed(name, fn):
        ctx.set_timing(True)  # also resets the accumulated times
        fn()
        torch.cuda.synchronize()
        ms, launches = ctx.kernel_times()[name]
        return ms / launches

    def lookup():
        idx.lookup(key)

    def probe():  # every row hits a registered Object: the probe decides all of them
        dedup.group_rows_indexed(key, None, None, idx, 100)

    absent = torch.arange(n, n + (1 << 20), dtype=torch.int32, device="cuda")

    def remove_none():  # 1 M ids that own nothing: the table stays as it is
        idx.remove_objects(absent, 2 * n, count=False)

    ek = torch.empty(live, dtype=torch.int64, device="cuda")
    ev = torch.empty(live, dtype=torch.int32, device="cuda")
    ec = torch.empty(1, dtype=torch.int32, device="cuda")

    def export():
        s = torch.cuda.current_stream().cuda_stream
        rc = ctx.lib.sdgpu_index_export_device(idx.h, ek.data_ptr(), ev.data_ptr(), live,
                                               ec.data_ptr(), s)
        assert rc == 0, rc

    legs = {"index_lookup": lookup, "index_probe": probe, "index_remove_objects": remove_none,
            "index_export": export}
    for _ in range(a.warmup):
        for name, fn in legs.items():
            timed(name, fn)
    samples = {name: [] for name in legs}
    for _ in range(a.repeats):
        for name, fn in legs.items():
            samples[name].append(timed(name, fn))
    assert idx.stats() == (live, used, cap), "the table changed under the measurement"
    # one real removal: 1 M Objects that own entries (changes the table: last, once)
    some = torch.arange(0, 1 << 20, dtype=torch.int32, device="cuda")
    real = timed("index_remove_objects", lambda: idx.remove_objects(some, 2 * n, count=False))
    out = {"rows": n, "live": live, "capacity": cap, "load": round(live / cap, 3),
           "repeats": a.repeats, "removed_live_after": idx.stats()[0]}
    for name, xs in samples.items():
        out[name] = {"median_ms": round(statistics.median(xs), 4), "min_ms": round(min(xs), 4),
                     "max_ms": round(max(xs), 4)}
    table_bytes = 16 * cap
    for name in ("index_remove_objects", "index_export"):
        med = out[name]["median_ms"] * 1e-3
        out[name]["hbm_share_on_capacity_x16"] = round(table_bytes / med / HBM_BYTES_PER_S, 3)
    out["index_remove_objects_1M_real_ms"] = round(real, 4)
    out["lookup_over_probe"] = round(out["index_lookup"]["median_ms"] /
                                     out["index_probe"]["median_ms"], 3)
    print(json.dumps(out))
    idx.close()


if __name__ == "__main__":
    main()
