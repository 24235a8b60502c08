"""GPU: the sync ingest on a poisoned workspace and a poisoned table.  The
pages run in a fresh child process with SDGPU_POISON_WS=1 (every buffer the
library allocates for itself starts as 0xA5 bytes and is logged, csrc/ctx.hpp),
as tests/test_gpu_search_poison.py starts its scenarios.  The large page runs
first, so it is the one that allocates and reads poison; a smaller one then
reads its leftovers; a log created at the smallest capacity grows (its new
table is poisoned too); the host entry point allocates on a context of its own.
Every output must equal the oracle's, and the log must show the workspace and
the table poisoned."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def pages():
    rng = np.random.default_rng(43)
    big = (rng.integers(0, 9000, 30_000).astype(np.uint64), rng.integers(-50, 50, 30_000),
           rng.integers(0, 6, 30_000))
    small = (rng.integers(0, 9000, 700).astype(np.uint64), rng.integers(-60, 60, 700),
             rng.integers(0, 6, 700))
    return [("large", *big), ("small", *small)]


def child():
    sys.path.insert(0, ROOT)
    import torch
    from tests import sync_oracle as SO
    from tests.test_gpu_sync_ingest import Log
    from spacedrive_amd import sync as S
    from spacedrive_amd._native import Context
    out = {}
    with Context(0) as ctx:
        log = Log(ctx, capacity_hint=20_000)
        print("scenario created", file=sys.stderr, flush=True)
        for name, key, ts, inst in pages():                 # Log.ingest asserts every output
            log.ingest(key, key ^ np.uint64(7), ts, inst, [0] * 4)
            out[name] = True
            print(f"scenario {name}", file=sys.stderr, flush=True)
        grown = Log(ctx, capacity_hint=1)
        print("scenario grown_created", file=sys.stderr, flush=True)
        for name, key, ts, inst in pages():
            grown.ingest(key, None, ts, inst, [5] * 6, commit=name == "small")
            got, want = grown.add(key, key, ts)
            out["grown_" + name] = got == want == 0
        out["grown_stats"] = grown.dev.stats()[0] == len(grown.model)
        print("scenario grown", file=sys.stderr, flush=True)
    with Context(0) as ctx:      # the host entry point allocates on a context of its own
        hlog = S.OpLog(0, ctx)
        model = {}
        for name, key, ts, inst in pages():
            clock = np.zeros(6, dtype=np.uint64)
            want = SO.ingest_keys(key, key, ts, inst, [0] * 6, model)
            apply, applied, winner, counts = S.ingest_host(hlog, key, key, ts, inst, clock)
            model = want[5]
            out["host_" + name] = bool(np.array_equal(apply, want[0])
                                       and np.array_equal(applied, want[1])
                                       and np.array_equal(winner, want[2])
                                       and np.array_equal(counts, want[3])
                                       and clock.tolist() == want[4])
            print(f"scenario host_{name}", file=sys.stderr, flush=True)
    torch.cuda.synchronize()
    print(json.dumps(out))


@pytest.mark.gpu
def test_sync_ingest_on_poisoned_workspace_and_table():
    env = dict(os.environ, SDGPU_POISON_WS="1")
    p = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True,
                       timeout=240, env=env, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    out = json.loads(p.stdout.strip().splitlines()[-1])
    assert len(out) == 7 and all(out.values()), out
    log = p.stderr
    # creating a log allocated, and so poisoned, its table
    assert "oplog_table" in log[:log.index("scenario created")], log[-2000:]
    # the first page of either context allocated, and so poisoned, its workspace
    first = log[log.index("scenario created"):log.index("scenario large")]
    assert "poisoned" in first and "link_ws" in first, log[-2000:]
    # the grown log's new tables
    grown = log[log.index("scenario grown_created"):log.index("scenario grown\n")]
    assert grown.count("oplog_table") >= 1, log[-2000:]
    host = log[log.index("scenario grown\n"):log.index("scenario host_large")]
    assert "oplog_table" in host and "link_ws" in host, log[-2000:]


if __name__ == "__main__":
    child()
