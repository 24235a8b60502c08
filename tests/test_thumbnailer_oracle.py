"""CPU: the two halves of tests/thumbnailer_oracle.py agree -- the files the
reference's thumbnail::process writes (thumbnail/mod.rs:204-359, in steps of
10 rows) are exactly the cas_ids of the contract's work rows, and its
`created` counter exceeds the work list's length by the copies it writes twice:
the in-step copies, and with `regenerate` every later copy of a cas_id."""
import random

import pytest

from tests import thumbnailer_oracle as TO


def random_rows(rng, n, n_ids):
    ids = ["%016x" % rng.getrandbits(64) for _ in range(n_ids)]
    rows = []
    for _ in range(n):
        c = rng.choice(ids) if rng.random() > 0.1 else None
        rows.append((c, rng.random() > 0.2))
    on_disk = {c for c in ids if rng.random() < 0.3} | {"%016x" % rng.getrandbits(64)}
    return rows, on_disk


@pytest.mark.parametrize("seed", range(20))
@pytest.mark.parametrize("regenerate", [False, True])
def test_reference_writes_the_work_rows(seed, regenerate):
    rng = random.Random(seed)
    n = rng.choice([0, 1, 9, 10, 11, 57, 300])
    rows, on_disk = random_rows(rng, n, rng.choice([1, 3, 40, 400]))
    written, created, skipped, rewrites = TO.reference_run(rows, on_disk, regenerate)
    work, dir_start, stats, present = TO.work_list(rows, on_disk, regenerate)
    assert written == {rows[i][0] for i in work}
    assert len(written) == len(work) == stats[3] == dir_start[256]
    assert created == len(work) + rewrites
    cand = TO.candidates(rows, on_disk, regenerate)
    if regenerate:     # every candidate is generated, however far apart the copies are
        assert created == cand == stats[1] and skipped == 0
    else:              # a copy in a later step finds the file: only in-step copies are rewritten
        assert rewrites == TO.in_batch_copies(rows, on_disk)
        assert created + skipped == stats[1] and skipped >= stats[2]
    # the product's counters (spacedrive_amd.thumbnailer.process) against the reference's
    assert len(work) == created - rewrites
    assert stats[1] - len(work) == skipped + rewrites


def test_work_list_contract_by_hand():
    a, b, c = "00" + "1" * 14, "ff" + "2" * 14, "00" + "3" * 14
    rows = [(b, False),      # ineligible: shadows nothing
            (None, True),    # keyless
            (b, True),       # the lowest eligible row of b
            (a, True),       # on disk
            (c, True), (b, True), (c, True)]
    work, start, stats, present = TO.work_list(rows, {a})
    assert work == [4, 2] and present == [0, 0, 0, 1, 0, 0, 0]
    assert start[0] == 0 and start[1] == 1 and start[255] == 1 and start[256] == 2
    assert stats == [1, 5, 1, 2]
    work, _, stats, _ = TO.work_list(rows, {a}, regenerate=True)
    assert work == [3, 4, 2] and stats == [1, 5, 1, 3]
    written, created, skipped, rewrites = TO.reference_run(rows, {a})
    assert written == {b, c} and (created, skipped, rewrites) == (4, 1, 2)
