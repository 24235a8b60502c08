#!/usr/bin/env python3
"""The two measurements of the identifier call that also returns the
integrity_checksum of the files it read whole (body-pass section);
needs a gfx950 GPU.

1. K1's body pass against K1 itself: the whole-read subset (size <= 100 KiB)
   of config2_files(--files), synthesised on the device.  Kernel times come from
   the library's own event timers (sdgpu_set_timing): cas_leaves + cas_fold of
   sdgpu_cas_batch_device against body_leaves + body_fold of
   sdgpu_cas_checksum_batch_device over the same arena.  The two calls alternate
   inside every repeat, so drift hits both alike.
2. One read instead of two: the <= 100 KiB half of write_config1_dir(--dir-files),
   page cache warm.  A = identify() then checksum_files() on the same paths,
   B = identify(checksums=True); A and B (and identify() alone) alternate in one
   process, wall-clock medians.

    python scripts/identify_checksum_timing.py [--files 200000] [--repeats 20]

Prints one JSON line; medians and the min..max spread are reported.
"""
from __future__ import annotations

import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WHOLE_MAX = 100 * 1024


def spread(xs, nd=4):
    return {"median_ms": round(statistics.median(xs), nd), "min_ms": round(min(xs), nd),
            "max_ms": round(max(xs), nd)}


def body_pass_against_k1(ctx, files, repeats, warmup):
    import torch
    from spacedrive_amd import cas, corpus
    sizes, seeds = corpus.config2_files(files)
    keep = sizes <= WHOLE_MAX
    sizes, seeds = sizes[keep], seeds[keep]
    arena, off, ln = corpus.synth_arena_device(sizes, seeds, ctx=ctx)
    n = off.numel()
    whole = torch.ones(n, dtype=torch.uint8, device=arena.device)
    out8 = torch.empty((n, 8), dtype=torch.uint8, device=arena.device)
    out32 = torch.empty((n, 32), dtype=torch.uint8, device=arena.device)
    has = torch.empty(n, dtype=torch.uint8, device=arena.device)
    st = torch.empty(n, dtype=torch.int32, device=arena.device)

    def kernels(fn, names):
        ctx.set_timing(True)  # also resets the accumulated times
        fn()
        torch.cuda.synchronize()
        t = ctx.kernel_times()
        return sum(t[k][0] for k in names)

    def k1():
        cas.cas_batch_device(arena, off, ln, out8, st, ctx=ctx)

    def both():
        cas.cas_checksum_batch_device(arena, off, ln, whole, out8, out32, has, st, ctx=ctx)

    cas_names, body_names = ("cas_leaves", "cas_fold"), ("body_leaves", "body_fold")
    for _ in range(warmup):
        kernels(k1, cas_names)
        kernels(both, body_names)
    t_cas, t_body = [], []
    for _ in range(repeats):
        t_cas.append(kernels(k1, cas_names))
        t_body.append(kernels(both, body_names))
    ctx.set_timing(False)
    assert int(has.sum()) == n and int(st.abs().sum()) == 0
    return {"files": int(n), "message_bytes": int(ln.to(torch.int64).sum()),
            "repeats": repeats, "k1_leaves_fold": spread(t_cas), "body_leaves_fold": spread(t_body),
            "body_over_k1": round(statistics.median(t_body) / statistics.median(t_cas), 3),
            "body_over_k1_per_repeat_min_max": [round(min(b / c for b, c in zip(t_body, t_cas)), 3),
                                                round(max(b / c for b, c in zip(t_body, t_cas)), 3)],
            "loader": "8-byte loads (uint2)"}


def one_read_instead_of_two(ctx, dir_files, calls):
    from spacedrive_amd import corpus, validation
    from spacedrive_amd import file_identifier as fi
    root = tempfile.mkdtemp(prefix="sd_idsum_")
    try:
        paths, sizes = corpus.write_config1_dir(root, dir_files)
        keep = [i for i in range(len(paths)) if 0 < sizes[i] <= WHOLE_MAX]
        pl = fi.PathList([paths[i] for i in keep])
        plain = list(pl)
        sz = sizes[keep]

        def two_reads():
            fi.identify(pl, sz, ctx=ctx)
            validation.checksum_files(plain, ctx)

        def one_read():
            return fi.identify(pl, sz, ctx=ctx, checksums=True)

        def identify_alone():
            fi.identify(pl, sz, ctx=ctx)

        legs = {"A_identify_then_checksum_files": two_reads, "B_identify_checksums": one_read,
                "identify_alone": identify_alone}
        for fn in legs.values():  # warm-up pass: page cache, slabs, workspaces
            fn()
        ms = {k: [] for k in legs}
        for _ in range(calls):
            for k, fn in legs.items():
                t0 = time.perf_counter()
                fn()
                ms[k].append((time.perf_counter() - t0) * 1e3)
        # the two routes agree (not timed)
        r = one_read()
        sums, st = validation.checksum_files(plain, ctx)
        assert not st.any() and r.has_checksum.all() and (r.checksum32 == sums).all()
        out = {"files": len(keep), "file_bytes": int(sz.sum()), "calls": calls}
        for k, xs in ms.items():
            out[k] = spread(xs, 3)
        a = out["A_identify_then_checksum_files"]["median_ms"]
        b = out["B_identify_checksums"]["median_ms"]
        out["B_over_A"] = round(b / a, 3)
        out["checksums_on_top_of_identify_ms"] = round(b - out["identify_alone"]["median_ms"], 3)
        # where that goes: the library's host and kernel timers over one more
        # call of each (not part of the wall-clock figures above)
        for k in ("identify_alone", "B_identify_checksums"):
            ctx.set_timing(True)
            legs[k]()
            out[k]["timers_ms_calls"] = {name: [round(v[0], 3), v[1]]
                                         for name, v in ctx.kernel_times().items()}
        ctx.set_timing(False)
        return out
    finally:
        shutil.rmtree(root, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=200_000)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dir-files", type=int, default=10_000)
    ap.add_argument("--calls", type=int, default=9)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured here")
    from spacedrive_amd._native import default_context
    ctx = default_context(0)
    out = {"body_pass_against_k1": body_pass_against_k1(ctx, a.files, a.repeats, a.warmup),
           "one_read_instead_of_two": one_read_instead_of_two(ctx, a.dir_files, a.calls)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
