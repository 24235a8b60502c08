#!/usr/bin/env python3
"""The measurements of the identifier call that also returns every file's
Object kind; needs a gfx950 GPU.

1. One call instead of two passes: write_config1_dir(--dir-files), every file
   renamed to carry one of the table's extension names in turn (so the
   reference's kind call would open each of them), page cache warm.  In one
   process, alternating within every repeat:
     identify_alone            identify()
     one_call                  identify_metadata()
     two_pass                  identify(), then kind_of_file() over the same
                               paths on 16 host threads -- what a host pays
                               today for FileMetadata::new's third output
   Wall-clock medians and min..max; the kinds of the two routes are compared
   (not timed).
2. k_kind alone: --messages device-resident messages (random, 8..56 bytes long
   at 64-byte strides, ids cycling over the table), timed by the
   library's event timers, against the bytes it moves (at most 48 B read, plus
   the 14 B of offset, length and id, and 1 B written per message).

    python scripts/identify_kind_timing.py [--dir-files 10000] [--calls 9]

Prints one JSON line.
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
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def spread(xs, nd=3):
    return {"median_ms": round(statistics.median(xs), nd), "min_ms": round(min(xs), nd),
            "max_ms": round(max(xs), nd)}


def one_call_instead_of_two_passes(ctx, dir_files, calls, threads):
    import numpy as np
    from spacedrive_amd import corpus
    from spacedrive_amd import file_identifier as fi
    from spacedrive_amd import kind as K
    root = tempfile.mkdtemp(prefix="sd_idkind_")
    try:
        paths, sizes = corpus.write_config1_dir(root, dir_files)
        names = [r[1] for r in K.ext_table()]
        renamed = []
        for i, p in enumerate(paths):
            q = os.path.splitext(p)[0] + "." + names[i % len(names)]
            os.rename(p, q)
            renamed.append(q)
        pl = fi.PathList(renamed)
        plain = list(pl)
        pool = ThreadPoolExecutor(threads)
        chunk = (len(plain) + threads - 1) // threads
        parts = [plain[i:i + chunk] for i in range(0, len(plain), chunk)]

        def host_kinds():
            out = pool.map(lambda ps: [int(K.kind_of_file(p)) for p in ps], parts)
            return [k for part in out for k in part]

        def identify_alone():
            return fi.identify(pl, sizes, ctx=ctx)

        def one_call():
            return fi.identify_metadata(pl, sizes, ctx=ctx)

        def two_pass():
            fi.identify(pl, sizes, ctx=ctx)
            return host_kinds()

        legs = {"identify_alone": identify_alone, "one_call": one_call, "two_pass": two_pass}
        for fn in legs.values():  # warm-up: page cache, slabs, workspaces, the thread pool
            fn()
        ms = {k: [] for k in legs}
        for _ in range(calls):
            for k, fn in legs.items():
                t0 = time.perf_counter()
                fn()
                ms[k].append((time.perf_counter() - t0) * 1e3)
        r = one_call()
        assert not r.status.any() and r.kind.tolist() == host_kinds()
        assert np.array_equal(r.cas8, identify_alone().cas8)
        out = {"files": len(plain), "calls": calls, "host_threads": threads,
               "kinds_seen": sorted(set(r.kind.tolist()))}
        for k, xs in ms.items():
            out[k] = spread(xs)
        alone = out["identify_alone"]
        out["one_call_minus_identify_ms"] = round(out["one_call"]["median_ms"] - alone["median_ms"], 3)
        out["identify_spread_ms"] = round(alone["max_ms"] - alone["min_ms"], 3)
        out["one_call_inside_identify_spread"] = bool(
            alone["min_ms"] <= out["one_call"]["median_ms"] <= alone["max_ms"])
        out["one_call_over_two_pass"] = round(out["one_call"]["median_ms"] /
                                              out["two_pass"]["median_ms"], 3)
        for k in ("identify_alone", "one_call"):
            ctx.set_timing(True)
            legs[k]()
            out[k]["timers_ms_calls"] = {name: [round(v[0], 3), v[1]]
                                         for name, v in ctx.kernel_times().items()}
        ctx.set_timing(False)
        pool.shutdown()
        return out
    finally:
        shutil.rmtree(root, ignore_errors=True)


def k_kind_alone(ctx, messages, repeats, warmup):
    import torch
    from spacedrive_amd import kind as K
    dev = torch.device("cuda", ctx.device)
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    stride = 64
    arena = torch.randint(0, 256, (messages * stride,), dtype=torch.uint8, device=dev, generator=g)
    off = torch.arange(messages, dtype=torch.int64, device=dev) * stride
    ln = torch.randint(8, 57, (messages,), dtype=torch.int32, device=dev, generator=g)
    ext = (torch.arange(messages, dtype=torch.int32, device=dev) % 216).to(torch.int16)
    out = torch.empty(messages, dtype=torch.uint8, device=dev)
    res = {"messages": messages, "repeats": repeats}
    for verify in (False, True):
        ts = []
        for it in range(warmup + repeats):
            ctx.set_timing(True)
            K.kind_batch_device(arena, off, ln, ext, verify=verify, out=out, ctx=ctx)
            torch.cuda.synchronize()
            if it >= warmup:
                ts.append(ctx.kernel_times()["kind"][0])
        ctx.set_timing(False)
        read = int(torch.clamp(ln, max=48).to(torch.int64).sum()) + 14 * messages
        med = statistics.median(ts)
        res["verify" if verify else "default"] = {
            **spread(ts, 4), "bytes_read": read, "bytes_written": messages,
            "GB_per_s": round((read + messages) / med / 1e6, 1),
            "messages_per_us": round(messages / med / 1e3, 1)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dir-files", type=int, default=10_000)
    ap.add_argument("--calls", type=int, default=9)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--messages", type=int, default=1 << 20)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured here")
    from spacedrive_amd._native import default_context
    ctx = default_context(0)
    out = {"one_call_instead_of_two_passes":
           one_call_instead_of_two_passes(ctx, a.dir_files, a.calls, a.threads),
           "k_kind_alone": k_kind_alone(ctx, a.messages, a.repeats, a.warmup)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
