"""CPU: the two oracles of the sync ingest agree with each other and with
SQLite running the reference's own query, and the Ingester's control flow
(failure path, winners_only) equals the sequential port."""
import sqlite3
import uuid

import numpy as np
import pytest

from tests import sync_oracle as SO
from spacedrive_amd import sync as S

INSTANCES = [uuid.UUID(int=i + 1) for i in range(3)]


def columns(ops, ids=None):
    ids = {} if ids is None else ids
    key = np.array([ids.setdefault((o.table, o.name, o.id_bytes, o.kind), len(ids)) for o in ops],
                   dtype=np.uint64)
    ts = np.array([o.stored_timestamp for o in ops], dtype=np.int64)
    inst = np.array([INSTANCES.index(o.instance) for o in ops])
    return key, ts, inst, ids


def model_of(shared, relation, ids):
    """{key: [L, tag]} of the op-log rows."""
    log = {}
    for table, rows, kind_at in (("shared", shared, 4), ("relation", relation, 5)):
        for r in rows:
            k = ids.setdefault((table, r[2], r[3], r[kind_at]), len(ids))
            log[k] = [max(r[1], log.get(k, [r[1]])[0]), k]
    return log


@pytest.mark.parametrize("seed", range(6))
def test_keys_contract_equals_the_sequential_port(seed):
    rng = np.random.default_rng(seed)
    pre = SO.random_ops(rng, 60, INSTANCES, high_bit=seed % 2 == 1)
    shared, relation, clocks = [], [], {INSTANCES[0]: 17}
    SO.ingest_sequential(pre, shared, relation, {})             # a pre-loaded log
    ops = SO.random_ops(rng, 400, INSTANCES, high_bit=seed % 2 == 1)
    ops += ops[:50]                                             # re-delivered ops
    key, ts, inst, ids = columns(ops)
    log = model_of(shared, relation, ids)
    clock0 = [clocks.get(u, 0) for u in INSTANCES]
    apply, applied, winners, counts, clock, log_after = SO.ingest_keys(key, key, ts, inst, clock0,
                                                                       log)
    done = SO.ingest_sequential(ops, shared, relation, clocks)
    assert applied.tolist() == done and apply.sum() == len(done)
    assert counts.tolist()[:2] == [len(done), winners.size] and counts[3] == 0
    assert [clocks[u] for u in INSTANCES] == clock
    want = model_of(shared, relation, ids)
    assert {k: v[0] for k, v in log_after.items() if v[0] is not None} == \
        {k: v[0] for k, v in want.items()}
    # the winner of a key is its last applied op
    last = {}
    for i in done:
        last[int(key[i])] = i
    assert winners.tolist() == sorted(last.values())


def _sqlite():
    db = sqlite3.connect(":memory:")
    db.execute("CREATE TABLE shared_operation (id BLOB PRIMARY KEY, timestamp BIGINT, model TEXT,"
               " record_id BLOB, kind TEXT, data BLOB, instance_id INTEGER)")
    db.execute("CREATE TABLE relation_operation (id BLOB PRIMARY KEY, timestamp BIGINT,"
               " relation TEXT, item_id BLOB, group_id BLOB, kind TEXT, data BLOB,"
               " instance_id INTEGER)")
    return db


def sqlite_ingest(db, ops):
    """The reference's statements, literally, one op at a time."""
    done = []
    for i, op in enumerate(ops):
        t = op.stored_timestamp
        if op.table == "shared":
            row = db.execute("SELECT timestamp FROM shared_operation WHERE timestamp >= ? AND"
                             " model = ? AND record_id = ? AND kind = ? ORDER BY timestamp DESC"
                             " LIMIT 1", (t, op.name, op.id_bytes, op.kind)).fetchone()
        else:
            row = db.execute("SELECT timestamp FROM relation_operation WHERE timestamp >= ? AND"
                             " relation = ? AND item_id = ? AND kind = ? ORDER BY timestamp DESC"
                             " LIMIT 1", (t, op.name, op.id_bytes, op.kind)).fetchone()
        if row is not None and row[0] != t:
            continue
        r = op.row()
        if op.table == "shared":
            db.execute("INSERT INTO shared_operation VALUES (?,?,?,?,?,?,?)",
                       (uuid.uuid4().bytes,) + r[1:6] + (INSTANCES.index(r[6]),))
        else:
            db.execute("INSERT INTO relation_operation VALUES (?,?,?,?,?,?,?,?)",
                       (uuid.uuid4().bytes,) + r[1:7] + (INSTANCES.index(r[7]),))
        done.append(i)
    return done


@pytest.mark.parametrize("seed", range(4))
def test_sequential_port_equals_sqlite(seed):
    rng = np.random.default_rng(100 + seed)
    ops = SO.random_ops(rng, 500, INSTANCES, high_bit=True)
    assert any(o.stored_timestamp < 0 for o in ops)
    shared, relation = [], []
    assert SO.ingest_sequential(ops, shared, relation, {}) == sqlite_ingest(_sqlite(), ops)


def test_apply_is_signed_and_the_clock_unsigned():
    """t = 2^63 is stored as INT64_MIN: older than t = 1 for SQLite's BigInt and
    so for apply, newer for the NTP64 clock."""
    typ = S.SharedOperation({"pub_id": [1]}, "tag", "u", "name", "x")
    a = S.CRDTOperation(INSTANCES[0], 1, uuid.UUID(int=1), typ)
    b = S.CRDTOperation(INSTANCES[0], 1 << 63, uuid.UUID(int=2), typ)
    assert b.stored_timestamp == -(1 << 63)
    clocks = {}
    assert SO.ingest_sequential([a, b], [], [], clocks) == [0]
    assert sqlite_ingest(_sqlite(), [a, b]) == [0]
    assert clocks == {INSTANCES[0]: 1 << 63}
    apply, _, _, _, clock, _ = SO.ingest_keys([4, 4], [4, 4], [1, -(1 << 63)], [0, 0], [0])
    assert apply.tolist() == [1, 0] and clock == [1 << 63]
    # the other order: both apply
    assert SO.ingest_sequential([b, a], [], [], {}) == [0, 1] == sqlite_ingest(_sqlite(), [b, a])


def test_pages_of_1000_equal_one_page():
    rng = np.random.default_rng(7)
    ops = SO.random_ops(rng, 3500, INSTANCES, records=40, t_hi=300)
    key, ts, inst, _ = columns(ops)
    whole = SO.ingest_keys(key, key, ts, inst, [0, 0, 0])
    log, clock, parts = {}, [0, 0, 0], []
    for a in range(0, 3500, 1000):
        apply, _, _, _, clock, log = SO.ingest_keys(key[a:a + 1000], key[a:a + 1000],
                                                    ts[a:a + 1000], inst[a:a + 1000], clock, log)
        parts.append(apply)
    assert np.array_equal(np.concatenate(parts), whole[0])
    assert clock == whole[4] and log == whole[5]


@pytest.mark.parametrize("seed", range(4))
def test_ingester_failure_path_equals_the_sequential_port(seed):
    rng = np.random.default_rng(200 + seed)
    pre = SO.random_ops(rng, 80, INSTANCES)
    shared, relation = [], []
    SO.ingest_sequential(pre, shared, relation, {})
    ops = SO.random_ops(rng, 300, INSTANCES)
    fail = {ops[i].id for i in rng.integers(0, 300, 25)}
    calls = [], []

    def apply_op(log):
        def f(op):
            if op.id in fail:
                raise RuntimeError("apply_op failed")
            log.append(op.id)
        return f

    ing = S.Ingester(shared, relation, {INSTANCES[1]: 9}, backend=SO.OracleBackend())
    clocks = {INSTANCES[1]: 9}
    want = SO.ingest_sequential(ops, shared, relation, clocks, apply_op(calls[0]))
    got = ing.receive_page(ops, apply_op(calls[1]))
    assert got == want and calls[0] == calls[1] and len(want) < 300
    assert ing.shared_operation == shared and ing.relation_operation == relation
    assert ing.timestamps == clocks
    # a second page through the same state
    more = SO.random_ops(rng, 100, INSTANCES)
    assert ing.receive_page(more, lambda op: None) == \
        SO.ingest_sequential(more, shared, relation, clocks)
    assert ing.shared_operation == shared and ing.timestamps == clocks


def test_winners_only_leaves_the_same_field_values():
    rng = np.random.default_rng(9)
    ops = [o for o in SO.random_ops(rng, 600, INSTANCES) if o.typ.data == "u"]

    def store():
        values = {}

        def f(op):
            values[(op.table, op.name, op.id_bytes, op.typ.field)] = op.typ.value
        return values, f

    every, f_every = store()
    winners, f_winners = store()
    a = S.Ingester(backend=SO.OracleBackend())
    b = S.Ingester(backend=SO.OracleBackend())
    done = a.receive_page(ops, f_every)
    assert b.receive_page(ops, f_winners, winners_only=True) == done
    assert every == winners and len(every) > 10
    assert a.shared_operation == b.shared_operation and a.timestamps == b.timestamps
    assert "shortcut, not the reference" in " ".join(S.Ingester.receive_page.__doc__.split())


def test_winners_only_with_a_failing_winner_logs_none_of_its_key():
    """The skipped predecessors of a winner whose apply_op fails never had their
    writes run: they are not logged, other keys are."""
    def upd(i, t, rec, value):
        return S.CRDTOperation(INSTANCES[0], t, uuid.UUID(int=i),
                               S.SharedOperation({"pub_id": [rec]}, "tag", "u", "name", value))
    a, d, b, c = upd(1, 1, 7, "a"), upd(2, 1, 8, "d"), upd(3, 2, 7, "b"), upd(4, 3, 7, "c")
    called = []

    def apply_op(op):
        called.append(op.typ.value)
        if op is c:
            raise RuntimeError("apply_op failed")

    ing = S.Ingester(backend=SO.OracleBackend())
    assert ing.receive_page([a, d, b, c], apply_op, winners_only=True) == [1]
    assert called == ["d", "c"] and ing.shared_operation == [d.row()]
    assert ing.timestamps == {INSTANCES[0]: 3}
    # the log holds nothing for record 7: an op older than a, b and c applies
    assert ing.receive_page([upd(5, 1, 7, "e"), upd(6, 0, 8, "old")], apply_op,
                            winners_only=True) == [0]
