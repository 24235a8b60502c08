#!/usr/bin/env python3
"""The measurements of the explorer's search page; needs a
gfx950 GPU.

One shape, every column device-resident: 12.5 M file_path rows in directories
of 100, 10 % of them directories, 80 % of the files with one of 10 M Objects
(30 % Images, the rest uniform over the 24 ObjectKinds, 1 % hidden), name ranks
a random permutation,
date_created random nanoseconds of 2015-2024.  Three queries:

  folder_view      DIR + GROUP_DIRS, order by name rank, take 100.
  category_cursor  KIND (Image) + HIDDEN_EXCLUDE, GROUP_DIRS, order by
                   date_created descending, a cursor in the middle of the dates.
  category_offset  the same filter and order with offset 1 000 000.

Per query, in one process, alternating within every repeat:

  search      sdgpu_search_page_device.
  yardstick   the obvious alternative from the same columns with torch: boolean
              mask, nonzero, composite key, torch.sort (stable, so ties go by
              row), slice.

HIP events around --inner back-to-back calls of a leg, a warm-up of both,
--repeats repeats.  The two pages are compared (not timed); a disagreement is
an error: nothing is written and the exit status is 1.  The condition per
query: the search's median is no higher than the yardstick's median plus the
larger of the two spreads.  The KTimer breakdown of one more call is recorded
beside it.  For context only, the same three queries run on the host in an
in-memory sqlite3 at 1/10 of the shape.

    python scripts/explorer_search_timing.py [--repeats 5] [--out FILE]

Prints one JSON line and writes it to --out
(profiles/explorer_search/explorer_search_timing.json).
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

PER_DIR = 100
N_ROWS, N_OBJECTS = 12_500_000, 10_000_000
IMAGE = 5
NS_2015, NS_2024 = 1_420_070_400 * 10**9, 1_704_067_200 * 10**9


def spread(xs, nd=4):
    return {"median_ms": round(statistics.median(xs), nd), "min_ms": round(min(xs), nd),
            "max_ms": round(max(xs), nd), "spread_ms": round(max(xs) - min(xs), nd)}


def make_shape(n, m, dev, seed):
    import torch
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    rnd = lambda k: torch.rand(k, device=dev, generator=g)  # noqa: E731
    n_dirs = (n + PER_DIR - 1) // PER_DIR
    dir_keys = torch.randint(-(2**63), 2**63 - 1, (n_dirs,), dtype=torch.int64, device=dev,
                             generator=g)
    c = {"dir_key": dir_keys[torch.arange(n, device=dev) // PER_DIR],
         "flags": (rnd(n) < 0.1).to(torch.uint8),
         "name_rank": torch.randperm(n, device=dev, generator=g) * 2 + 1,
         "date_created": torch.randint(NS_2015, NS_2024, (n,), dtype=torch.int64, device=dev,
                                       generator=g)}
    obj = torch.randint(0, m, (n,), dtype=torch.int32, device=dev, generator=g)
    c["object"] = torch.where((rnd(n) < 0.8) & (c["flags"] == 0), obj, torch.full_like(obj, -1))
    kind = torch.randint(0, 24, (m,), dtype=torch.int32, device=dev, generator=g)
    c["kind"] = torch.where(rnd(m) < 0.3, torch.full_like(kind, IMAGE), kind)
    c["oflags"] = (rnd(m) < 0.01).to(torch.uint8) * 4
    c["some_dir_key"] = int(dir_keys[n_dirs // 3].item())
    return c


def queries(E, c, n):
    mid = (NS_2015 + NS_2024) // 2
    cat = dict(use=E.USE_KIND | E.USE_HIDDEN_EXCLUDE, kind_mask=1 << IMAGE)
    return {
        "folder_view": (E.Query(use=E.USE_DIR, dir_key=c["some_dir_key"] & (2**64 - 1),
                                flags=E.GROUP_DIRS, take=100), "name_rank"),
        "category_cursor": (E.Query(flags=E.GROUP_DIRS | E.DESC | E.CURSOR, cursor_key=mid,
                                    cursor_row=n // 2, take=100, **cat), "date_created"),
        "category_offset": (E.Query(flags=E.GROUP_DIRS | E.DESC, offset=min(1_000_000, n // 12),
                                    take=100, **cat), "date_created"),
    }


def torch_page(E, c, q, key):
    """The yardstick: mask, nonzero, composite key, stable sort, slice."""
    import torch
    n = key.numel()
    mask = torch.ones(n, dtype=torch.bool, device=key.device)
    if q.use & E.USE_DIR:
        dk = q.dir_key - 2**64 if q.dir_key >= 2**63 else q.dir_key
        mask &= c["dir_key"] == dk
    if q.use & (E.USE_KIND | E.USE_HIDDEN_EXCLUDE):
        ob = c["object"].to(torch.int64)
        has = ob >= 0
        ob = ob.clamp(min=0)
        mask &= has & (c["kind"][ob] == IMAGE) & ((c["oflags"][ob] & 4) == 0)
    if q.flags & E.CURSOR:
        idx = torch.arange(n, device=key.device)
        if q.flags & E.DESC:
            mask &= (key < q.cursor_key) | ((key == q.cursor_key) & (idx < q.cursor_row))
        else:
            mask &= (key > q.cursor_key) | ((key == q.cursor_key) & (idx >= q.cursor_row))
    rows = mask.nonzero().flatten()
    k = key[rows]
    if q.flags & E.DESC:
        k = -k
    if q.flags & E.GROUP_DIRS:     # files above every directory: the keys stay below 2^62
        k = k + ((c["flags"][rows] == 0).to(torch.int64) * 2 - 1) * (1 << 62)
    _, perm = torch.sort(k, stable=True)
    return rows[perm[q.offset:q.offset + q.take]]


def measure(ctx, E, n, m, repeats, warmup, inner):
    import torch
    dev = torch.device("cuda", ctx.device)
    c = make_shape(n, m, dev, seed=n)
    objs = E.Objects(m, kind=c["kind"], flags=c["oflags"])
    page = torch.empty(E.MAX_TAKE, dtype=torch.int32, device=dev)
    counts = torch.empty(4, dtype=torch.int32, device=dev)
    out = {}
    for name, (q, order) in queries(E, c, n).items():
        rows = E.Rows(n, dir_key=c["dir_key"], flags=c["flags"], object=c["object"],
                      order_key=c[order])
        search = lambda: E.search_page(rows, objs, q, ctx=ctx, page=page, counts=counts)  # noqa: E731
        yard = lambda: torch_page(E, c, q, c[order])  # noqa: E731
        legs = {"search": search, "yardstick": yard}
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
        search()
        torch.cuda.synchronize()
        cnt = [int(x) for x in counts.cpu().tolist()]
        same = bool(torch.equal(page[:cnt[2]].to(torch.int64), yard()))
        o = {"counts": cnt, "yardstick_agrees": same, "repeats": repeats, "inner_calls": inner}
        for k, xs in ms.items():
            o[k] = spread(xs)
        slack = max(o["search"]["spread_ms"], o["yardstick"]["spread_ms"])
        o["search_minus_yardstick_ms"] = round(o["search"]["median_ms"]
                                               - o["yardstick"]["median_ms"], 4)
        o["within_median_plus_spread"] = bool(o["search"]["median_ms"]
                                              <= o["yardstick"]["median_ms"] + slack)
        ctx.set_timing(True)
        search()
        torch.cuda.synchronize()
        o["search_kernels_ms"] = {k: round(v[0], 4) for k, v in sorted(ctx.kernel_times().items())}
        ctx.set_timing(False)
        if not same:
            raise SystemExit(f"{name}: the search's page differs from the yardstick's")
        out[name] = o
    return out, c


def sqlite_context(E, c, n, m, scale=10):
    """The same three queries in an in-memory sqlite3 over the first 1/scale of
    the rows and Objects, on the host; context only."""
    import sqlite3
    ns, msml = n // scale, m // scale
    col = lambda k, cnt: c[k][:cnt].cpu().tolist()  # noqa: E731
    db = sqlite3.connect(":memory:")
    db.execute("CREATE TABLE file_path (id INTEGER PRIMARY KEY, dir_key INTEGER, is_dir INTEGER,"
               " name_rank INTEGER, date_created INTEGER, object_id INTEGER)")
    db.execute("CREATE TABLE object (id INTEGER PRIMARY KEY, kind INTEGER, hidden INTEGER)")
    ob = [x + 1 if 0 <= x < msml else None for x in col("object", ns)]
    db.executemany("INSERT INTO file_path VALUES (?,?,?,?,?,?)",
                   zip(range(1, ns + 1), col("dir_key", ns), col("flags", ns),
                       col("name_rank", ns), col("date_created", ns), ob))
    db.executemany("INSERT INTO object VALUES (?,?,?)",
                   zip(range(1, msml + 1), col("kind", msml),
                       [1 if f else 0 for f in col("oflags", msml)]))
    db.execute("CREATE INDEX fp_dir ON file_path (dir_key)")
    db.execute("CREATE INDEX fp_obj ON file_path (object_id)")
    db.execute("CREATE INDEX o_kind ON object (kind)")
    mid = (NS_2015 + NS_2024) // 2
    cat = ("FROM file_path fp JOIN object o ON o.id = fp.object_id WHERE o.kind = 5 AND "
           "(o.hidden IS NULL OR o.hidden <> 1)")
    sql = {
        "folder_view": ("SELECT id FROM file_path fp WHERE dir_key = ? ORDER BY is_dir DESC, "
                        "name_rank, id LIMIT 100", [int(c["dir_key"][ns // 3].item())]),
        "category_cursor": ("SELECT fp.id " + cat + " AND (fp.date_created < ? OR "
                            "(fp.date_created = ? AND fp.id < ?)) ORDER BY fp.is_dir DESC, "
                            "fp.date_created DESC, fp.id LIMIT 100", [mid, mid, ns // 2 + 1]),
        "category_offset": ("SELECT fp.id " + cat + " ORDER BY fp.is_dir DESC, fp.date_created "
                            "DESC, fp.id LIMIT 100 OFFSET ?", [min(1_000_000, n // 12) // scale]),
    }
    out = {"file_path_rows": ns, "objects": msml}
    for name, (text, args) in sql.items():
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            got = db.execute(text, args).fetchall()
            ts.append((time.perf_counter() - t0) * 1e3)
        out[name] = dict(spread(ts, 3), rows=len(got))
    db.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "explorer_search",
                                                  "explorer_search_timing.json"))
    ap.add_argument("--scale", type=float, default=1.0,
                    help="shrinks the shape (a rehearsal, not a measurement)")
    ap.add_argument("--no-sqlite", action="store_true")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured here")
    from spacedrive_amd import explorer as E
    from spacedrive_amd._native import default_context
    ctx = default_context(0)
    n, m = max(int(N_ROWS * a.scale), 1000), max(int(N_OBJECTS * a.scale), 1000)
    out = {"device": torch.cuda.get_device_name(0), "scale": a.scale, "file_path_rows": n,
           "objects": m, "select_final_records": E.SELECT_FINAL_RECORDS}
    legs, cols = measure(ctx, E, n, m, a.repeats, a.warmup, a.inner)
    out.update(legs)
    if not a.no_sqlite:
        out["sqlite_host_tenth_scale"] = sqlite_context(E, cols, n, m)
    text = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
