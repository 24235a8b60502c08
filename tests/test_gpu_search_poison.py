"""GPU: the explorer's search page on a poisoned workspace.  One representative
query of each selection path runs in a fresh child process with
SDGPU_POISON_WS=1 (every buffer the library allocates for itself starts as 0xA5
bytes and is logged, csrc/ctx.hpp), as tests/test_gpu_poison_entry_points.py
starts its scenarios: the direct path (at most SELECT_FINAL_RECORDS rows), the
passes with offset 0 (one selection with winners), the passes with an offset
(two selections), the tags' marks, and the host entry point.  The large call
runs first, so it is the one that allocates and reads poison; a smaller one
then reads its leftovers.  Page and counts must equal the oracle's, and the log
must show that the call's workspace was allocated, and so poisoned, by it."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def scenarios():
    from tests import search_oracle as SO
    from spacedrive_amd.explorer import SELECT_FINAL_RECORDS as S
    rng = np.random.default_rng(41)
    big_r, big_o = SO.random_table(rng, 4 * S + 1, 600, 1500)
    small_r, small_o = SO.random_table(rng, S - 100, 200, 300)
    tags = dict(use=SO.USE_TAGS | SO.USE_HIDDEN_EXCLUDE, tags=(2, 3, 5, 7, 11))
    return [
        ("passes_offset", big_r, big_o, SO.query(flags=SO.GROUP_DIRS, offset=5000, take=100)),
        ("direct", small_r, small_o, SO.query(flags=SO.DESC, offset=10, take=256)),
        ("passes_winners", big_r, big_o, SO.query(flags=SO.DESC | SO.GROUP_DIRS, take=256)),
        ("tags_by_object", big_r, big_o,
         SO.query(flags=SO.ORDER_BY_OBJECT, offset=3, take=100, **tags)),
        ("cursor", big_r, big_o,
         SO.query(flags=SO.CURSOR, cursor_key=0, cursor_row=7000, take=100)),
        ("direct_again", small_r, small_o, SO.query(take=100, **tags)),
    ]


def child():
    sys.path.insert(0, ROOT)
    import torch
    from tests import search_oracle as SO
    from tests.test_gpu_search import POISON, as_query, run_device
    from spacedrive_amd import explorer as E
    from spacedrive_amd._native import Context
    out = {}
    with Context(0) as ctx:
        for name, r, o, q in scenarios():
            want_page, want_counts = SO.search_page(r, o, q)
            page, counts = run_device(r, o, q, ctx=ctx)
            P = int(want_counts[2])
            out[name] = bool(np.array_equal(counts, want_counts)
                             and np.array_equal(page[:P], want_page)
                             and (page[P:] == POISON).all())
            print(f"scenario {name}", file=sys.stderr, flush=True)
    with Context(0) as ctx:      # the host entry point allocates on a context of its own
        for name, r, o, q in scenarios()[:2]:
            rows = E.Rows(r.n, *(getattr(r, c) for c in E.ROW_COLUMNS))
            objs = E.Objects(o.m, *(getattr(o, c) for c in E.OBJECT_COLUMNS))
            page, counts = E.search_page_host(rows, objs, as_query(q), ctx=ctx)
            want_page, want_counts = SO.search_page(r, o, q)
            out["host_" + name] = bool(np.array_equal(counts, want_counts)
                                       and np.array_equal(page, want_page))
            print(f"scenario host_{name}", file=sys.stderr, flush=True)
    torch.cuda.synchronize()
    print(json.dumps(out))


@pytest.mark.gpu
def test_search_page_on_poisoned_workspace():
    env = dict(os.environ, SDGPU_POISON_WS="1")
    p = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True,
                       timeout=240, env=env, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    out = json.loads(p.stdout.strip().splitlines()[-1])
    assert len(out) == 8 and all(out.values()), out
    # the first call of either context allocated, and so poisoned, its workspace
    log = p.stderr
    first = log[:log.index("scenario passes_offset")]
    assert "poisoned" in first and "link_ws" in first, log[-2000:]
    host = log[log.index("scenario direct_again"):log.index("scenario host_passes_offset")]
    assert "poisoned" in host and "link_ws" in host, log[-2000:]


if __name__ == "__main__":
    child()
