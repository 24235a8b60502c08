#!/usr/bin/env python3
"""The measurements of the sync ingest.

Device cases (need a gfx950 GPU; every array device-resident, keys random):

  page_new_keys    a 1 M-op page of keys new to the log into logs of 1 M,
                   12.5 M and 100 M keys, and the ratio of the page time at
                   100 M logged keys to the time at 1 M (no threshold: the table
                   moves from cache to HBM).
  page_hot_keys    a 1 M-op page on 10 000 keys of a 1 M-key log, ascending
                   timestamps (every op applies, segments of 100 ops).
  page_1000        a 1000-op page, the reference's size, into a 1 M-key log:
                   device time between events and host wall time per call
                   (it is launch-bound).
  add_rows         sdgpu_oplog_add_device of 100 M rows into an empty log of
                   that capacity, with and without the tag check.
  torch_sort       torch.sort(stable=True) of the page's keys alone on the same
                   device: the floor of any torch formulation.

Before every timed call the log is rebuilt outside the events (clear, then add
of the base keys), so every repeat sees the same log and no call grows the
table: the capacity is reserved at creation.  HIP events around one call, a
warm-up, --repeats repeats, medians.  Per-kernel times of one page per log
size come from sdgpu_set_timing.

Host baseline (no GPU needed): the reference's three statements per op
(core/crates/sync/src/ingest.rs:114-233: the find_first of compare_message, the
op-log insert of apply_op, the instance update in a transaction of its own)
through sqlite3 on the schema of core/prisma/schema.prisma:21-53, --sqlite-ops
ops (20 000) against a --sqlite-rows (1 M) row log, without an index and with
one on (model, record_id, kind, timestamp).  --sqlite-scan-ops bounds the ops
of the run without an index (every op scans the log); the JSON records how
many ran.

    python scripts/sync_ingest_timing.py [--only device|host] [--repeats 5] [--out FILE]

Prints one JSON line and writes it to --out
(profiles/sync_ingest/sync_ingest_timing.json); with --only the other half of
an existing file is kept.
"""
from __future__ import annotations

import argparse
import json
import os
import platform
import sqlite3
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PAGE = 1_000_000
LOGS = [("log_1m", 1_000_000), ("log_12_5m", 12_500_000), ("log_100m", 100_000_000)]


def spread(xs, nd=4):
    return {"median_ms": round(statistics.median(xs), nd), "min_ms": round(min(xs), nd),
            "max_ms": round(max(xs), nd), "spread_ms": round(max(xs) - min(xs), nd)}


class Bench:
    def __init__(self, ctx, repeats, warmup):
        import torch
        self.ctx, self.repeats, self.warmup = ctx, repeats, warmup
        self.dev = torch.device("cuda", ctx.device)
        self.g = torch.Generator(device=self.dev)
        self.g.manual_seed(11)

    def keys(self, n):
        import torch
        return torch.randint(-(2**63), 2**63 - 1, (n,), dtype=torch.int64, device=self.dev,
                             generator=self.g)

    def stamps(self, n):
        import torch
        return torch.randint(0, 2**62, (n,), dtype=torch.int64, device=self.dev, generator=self.g)

    def timed(self, fn, before=None, wall=False):
        """ms of one call between two events per repeat (`before` runs outside
        them); wall: host time until the stream has drained instead."""
        import torch
        out = []
        for it in range(self.warmup + self.repeats):
            if before:
                before()
            torch.cuda.synchronize()
            if wall:
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ms = (time.perf_counter() - t0) * 1e3
            else:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                ms = a.elapsed_time(b)
            if it >= self.warmup:
                out.append(ms)
        return spread(out)

    def page_case(self, log, base, page, kernels=True, wall=False):
        """One page against the log rebuilt from `base` before every call."""
        import torch
        key, ts, inst = page
        clock = torch.zeros(8, dtype=torch.int64, device=self.dev)
        n = key.numel()
        apply = torch.empty(n, dtype=torch.uint8, device=self.dev)
        applied = torch.empty(n, dtype=torch.int32, device=self.dev)
        winner = torch.empty(n, dtype=torch.int32, device=self.dev)
        counts = torch.empty(4, dtype=torch.int32, device=self.dev)
        from spacedrive_amd._native import check
        lib, s = self.ctx.lib, torch.cuda.current_stream(self.dev).cuda_stream

        def rebuild():
            log.clear()
            log.add(base[0], base[0], base[1], collisions=False)

        def ingest():
            check(lib.sdgpu_sync_ingest_device(
                log.h, key.data_ptr(), key.data_ptr(), ts.data_ptr(), inst.data_ptr(), n,
                clock.data_ptr(), 8, 0, apply.data_ptr(), applied.data_ptr(), winner.data_ptr(),
                counts.data_ptr(), s))

        out = {"ops": n, "logged_keys": base[0].numel(), "slots": log.stats()[1]}
        out["page"] = self.timed(ingest, rebuild)
        if wall:
            out["page_host_wall"] = self.timed(ingest, rebuild, wall=True)
        out["counts"] = counts.tolist()
        if kernels:
            rebuild()
            self.ctx.set_timing(True)
            ingest()
            torch.cuda.synchronize()
            out["kernels_ms"] = {k: round(v[0], 4)
                                 for k, v in sorted(self.ctx.kernel_times().items())}
            self.ctx.set_timing(False)
        return out


def device_cases(a):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: the device cases are not measured here (--only host)")
    from spacedrive_amd._native import default_context
    from spacedrive_amd.sync import OpLog
    ctx = default_context(0)
    b = Bench(ctx, a.repeats, a.warmup)
    page_n = max(int(PAGE * a.scale), 1000)
    out = {"device": torch.cuda.get_device_name(0), "scale": a.scale, "repeats": a.repeats}
    page = (b.keys(page_n), b.stamps(page_n),
            torch.randint(0, 8, (page_n,), dtype=torch.int32, device=b.dev, generator=b.g))
    new = {}
    for name, n_log in LOGS:
        n_log = max(int(n_log * a.scale), 1000)
        base = (b.keys(n_log), b.stamps(n_log))
        log = OpLog(n_log + page_n, ctx)
        new[name] = b.page_case(log, base, page)
        if name == "log_1m":
            # 10 000 hot keys of the log, 100 ops each, ascending timestamps
            hot = base[0][torch.randint(0, min(10_000, n_log), (page_n,), device=b.dev,
                                        generator=b.g)]
            asc = torch.arange(page_n, dtype=torch.int64, device=b.dev) + 2**62
            out["page_hot_keys"] = b.page_case(log, base, (hot, asc, page[2]))
            small = tuple(t[:1000].contiguous() for t in page)
            out["page_1000"] = b.page_case(log, base, small, wall=True)
        log.close()
        del base, log
        torch.cuda.empty_cache()
    new["ratio_100m_to_1m"] = round(new["log_100m"]["page"]["median_ms"]
                                    / new["log_1m"]["page"]["median_ms"], 3)
    out["page_new_keys"] = new
    n_add = max(int(100_000_000 * a.scale), 1000)
    rows = (b.keys(n_add), b.stamps(n_add))
    log = OpLog(n_add, ctx)
    out["add_rows"] = {
        "rows": n_add,
        "add": b.timed(lambda: log.add(rows[0], rows[0], rows[1], collisions=False), log.clear),
        "add_with_tag_check": b.timed(lambda: log.add(rows[0], rows[0], rows[1]), log.clear)}
    log.close()
    del rows, log
    torch.cuda.empty_cache()
    out["torch_sort"] = {"ops": page_n,
                         "stable_sort_of_keys": b.timed(lambda: torch.sort(page[0], stable=True))}
    return out


def host_cases(a):
    """The reference's statements through sqlite3, one op at a time."""
    import random
    rnd = random.Random(5)
    models = ["tag", "label", "object", "file_path"]
    fields = ["name", "color", "note", "favorite", "hidden", "date_accessed"]

    def tuple_of(i):
        return (models[i % 4], b'{"pub_id":[%d]}' % (i // 24), "u:" + fields[(i // 4) % 6])

    n_tuples = a.sqlite_rows                       # one logged op per tuple
    ops = [(rnd.randrange(n_tuples + n_tuples // 10), rnd.randrange(1 << 40))
           for _ in range(a.sqlite_ops)]
    out = {"host": platform.processor() or platform.machine(), "log_rows": a.sqlite_rows}
    for name, index, n_ops in (("no_index", False, min(a.sqlite_scan_ops, a.sqlite_ops)),
                               ("index_model_record_kind_timestamp", True, a.sqlite_ops)):
        db = sqlite3.connect(":memory:", isolation_level=None)
        db.execute("CREATE TABLE instance (id INTEGER PRIMARY KEY, pub_id BLOB, timestamp BIGINT)")
        db.executemany("INSERT INTO instance VALUES (?,?,?)", [(i, b"%d" % i, 0) for i in range(8)])
        db.execute("CREATE TABLE shared_operation (id BLOB PRIMARY KEY, timestamp BIGINT,"
                   " model TEXT, record_id BLOB, kind TEXT, data BLOB, instance_id INTEGER)")
        db.execute("BEGIN")
        db.executemany("INSERT INTO shared_operation VALUES (?,?,?,?,?,?,?)",
                       ((b"r%d" % i, rnd.randrange(1 << 40), *tuple_of(i), b"1", i % 8)
                        for i in range(n_tuples)))
        db.execute("COMMIT")
        if index:
            db.execute("CREATE INDEX op_key ON shared_operation (model, record_id, kind, timestamp)")
        applied = 0
        t0 = time.perf_counter()
        for j, (i, t) in enumerate(ops[:n_ops]):
            model, record_id, kind = tuple_of(i)
            row = db.execute("SELECT timestamp FROM shared_operation WHERE timestamp >= ? AND"
                             " model = ? AND record_id = ? AND kind = ? ORDER BY timestamp DESC"
                             " LIMIT 1", (t, model, record_id, kind)).fetchone()
            if row is None or row[0] == t:
                db.execute("INSERT INTO shared_operation VALUES (?,?,?,?,?,?,?)",
                           (b"n%d" % j, t, model, record_id, kind, b"1", j % 8))
                applied += 1
            db.execute("BEGIN")
            db.execute("UPDATE instance SET timestamp = ? WHERE pub_id = ?", (t, b"%d" % (j % 8)))
            db.execute("COMMIT")
        s = time.perf_counter() - t0
        out[name] = {"ops": n_ops, "applied": applied, "seconds": round(s, 3),
                     "ms_per_op": round(s / max(n_ops, 1) * 1e3, 4)}
        db.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=("device", "host"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scale", type=float, default=1.0,
                    help="shrinks every device shape (a rehearsal, not a measurement)")
    ap.add_argument("--sqlite-ops", type=int, default=20_000)
    ap.add_argument("--sqlite-rows", type=int, default=1_000_000)
    ap.add_argument("--sqlite-scan-ops", type=int, default=20_000,
                    help="ops of the run without an index (each scans the whole log)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sync_ingest",
                                                  "sync_ingest_timing.json"))
    a = ap.parse_args()
    out = {}
    if a.only and os.path.exists(a.out):
        with open(a.out) as f:
            out = json.loads(f.read())
    if a.only != "host":
        out["device_cases"] = device_cases(a)
    if a.only != "device":
        out["host_sqlite"] = host_cases(a)
    text = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
