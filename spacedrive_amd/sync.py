"""Sync ingest: which CRDT operations of a received page apply
(core/crates/sync/src/ingest.rs:114-233 receive_crdt_operation /
compare_message), decided for the whole page by one device call
(sdgpu_sync_ingest_device) against a device-resident op log on 64-bit keys.

* ``CRDTOperation`` / ``SharedOperation`` / ``RelationOperation`` -- the op
  types of crates/sync/src/crdt.rs:25-131.
* ``op_message`` / ``op_keys`` -- BLAKE3-64 key and tag of an op's (model,
  record_id, kind) or (relation, item_id, kind), through K1.
* ``OpLog`` -- the device log (sdgpu_oplog): ``add``, ``latest``, ``ingest``,
  ``stats`` on torch device columns.
* ``Ingester`` -- an in-memory stand-in for the actor's Ingesting state
  (ingest.rs:67-71) over shared_operation / relation_operation lists.

get_ops (manager.rs:130-199), apply_op's database writes, the HLC and the
transport stay with the caller; only the decision is a device
call.  Deviation: 64-bit keys; two tuples sharing a key are
detected through the tags (``KeyCollision``), not repaired.
"""
from __future__ import annotations

import json
import uuid
from dataclasses import dataclass
from typing import Any

from ._native import check, default_context
from .indexer import KeyCollision, _keys

NO_COMMIT = 1            # SDGPU_INGEST_NO_COMMIT
INT64_MIN = -(1 << 63)
SHARED, RELATION = "shared", "relation"


def _json(value) -> bytes:
    """serde_json::to_vec: compact separators."""
    return json.dumps(value, separators=(",", ":")).encode()


def _kind(data_kind: str, field) -> str:
    """OperationKind's Display (crdt.rs:9-23)."""
    if data_kind == "u":
        return "u:" + field
    if data_kind not in ("c", "d"):
        raise ValueError("kind is 'c', 'u' or 'd'")
    return data_kind


def _data(data_kind: str, field, value) -> bytes:
    """serde_json of SharedOperationData / RelationOperationData (crdt.rs:39-47,72-80)."""
    return _json({"u": {"field": field, "value": value}} if data_kind == "u" else data_kind)


@dataclass(frozen=True)
class SharedOperation:
    """crdt.rs:59-70; `data` is "c", "u" (with field and value) or "d"."""
    record_id: Any
    model: str
    data: str = "c"
    field: str | None = None
    value: Any = None

    def kind(self) -> str:
        return _kind(self.data, self.field)


@dataclass(frozen=True)
class RelationOperation:
    """crdt.rs:25-37."""
    relation_item: Any
    relation_group: Any
    relation: str
    data: str = "c"
    field: str | None = None
    value: Any = None

    def kind(self) -> str:
        return _kind(self.data, self.field)


@dataclass(frozen=True)
class CRDTOperation:
    """crdt.rs:123-131.  `timestamp` is the NTP64 as an unsigned 64-bit integer."""
    instance: uuid.UUID
    timestamp: int
    id: uuid.UUID
    typ: SharedOperation | RelationOperation

    @property
    def table(self) -> str:
        return SHARED if isinstance(self.typ, SharedOperation) else RELATION

    @property
    def name(self) -> str:
        """shared_operation.model / relation_operation.relation."""
        return self.typ.model if self.table == SHARED else self.typ.relation

    @property
    def id_bytes(self) -> bytes:
        """record_id / item_id as stored: serde_json::to_vec (ingest.rs:197-199,216-218)."""
        return _json(self.typ.record_id if self.table == SHARED else self.typ.relation_item)

    @property
    def kind(self) -> str:
        return self.typ.kind()

    @property
    def stored_timestamp(self) -> int:
        """`timestamp.as_u64() as i64`: what the BigInt column holds."""
        t = self.timestamp & ((1 << 64) - 1)
        return t - (1 << 64) if t >> 63 else t

    def row(self) -> tuple:
        """The op-log row apply_op writes (shared_op_db / relation_op_db): (id,
        timestamp, model, record_id, kind, data, instance) or (id, timestamp,
        relation, item_id, group_id, kind, data, instance)."""
        t = self.typ
        data = _data(t.data, t.field, t.value)
        if self.table == SHARED:
            return (self.id.bytes, self.stored_timestamp, t.model, self.id_bytes, self.kind, data,
                    self.instance)
        return (self.id.bytes, self.stored_timestamp, t.relation, self.id_bytes,
                _json(t.relation_group), self.kind, data, self.instance)


def op_message(table: str, name: str, id_bytes: bytes, kind: str, salt: int = 0,
               tag: bool = False) -> bytes:
    """The bytes hashed for an op's key (prefix b"O") or tag (prefix b"T"): the
    prefix, the salt, the table (b"s" / b"r"), the name, NUL, the id's length
    (u32 LE: ids are JSON and may hold any byte), the id, the kind."""
    if table not in (SHARED, RELATION):
        raise ValueError("table is 'shared' or 'relation'")
    return ((b"T" if tag else b"O") + bytes([salt]) + (b"s" if table == SHARED else b"r")
            + name.encode() + b"\0" + len(id_bytes).to_bytes(4, "little") + id_bytes
            + kind.encode())


def _tuple_keys(tuples, salt: int, ctx=None):
    """(key, tag) of (table, name, id_bytes, kind) tuples: one K1 batch."""
    n = len(tuples)
    both = _keys([op_message(*t, salt=salt) for t in tuples]
                 + [op_message(*t, salt=salt, tag=True) for t in tuples], ctx)
    return both[:n].copy(), both[n:].copy()


def op_keys(ops, salt: int = 0, ctx=None):
    """(key, tag): two uint64 arrays, BLAKE3-64 of every op's key message and of
    its tag message, in one K1 batch."""
    return _tuple_keys([(o.table, o.name, o.id_bytes, o.kind) for o in ops], salt, ctx)


def _ptr(t):
    return t.data_ptr() if t is not None and t.numel() else None


class OpLog:
    """sdgpu_oplog: key -> newest logged timestamp, on the device, for as long
    as the library is open.  Columns are torch device tensors: keys and tags
    int64 (the uint64 bits), timestamps int64, instances int32, clocks int64
    (the NTP64 bits)."""

    def __init__(self, capacity_hint: int = 0, ctx=None):
        import ctypes
        self.ctx = ctx or default_context()
        h = ctypes.c_void_p()
        check(self.ctx.lib.sdgpu_oplog_create(self.ctx.h, capacity_hint, ctypes.byref(h)),
              "sdgpu_oplog_create")
        self.h = h
        self.ctx.adopt(self)

    def close(self):
        if self.h:
            self.ctx.lib.sdgpu_oplog_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _stream(self, t):
        import torch
        return torch.cuda.current_stream(t.device).cuda_stream

    def clear(self):
        check(self.ctx.lib.sdgpu_oplog_clear(self.h, None), "sdgpu_oplog_clear")

    def stats(self):
        """(keys stored, capacity in slots); synchronises."""
        import ctypes
        out = (ctypes.c_uint64 * 2)()
        check(self.ctx.lib.sdgpu_oplog_stats(self.h, out), "sdgpu_oplog_stats")
        return int(out[0]), int(out[1])

    def add(self, key, tag, ts, collisions: bool = True):
        """L(key) = max(L(key), ts) for existing op-log rows, in any order.
        Returns the tag disagreements (an int; synchronises), or None with
        collisions=False (asynchronous)."""
        import torch
        n = key.numel()
        col = torch.zeros(1, dtype=torch.int32, device=key.device) if collisions else None
        if n == 0:
            return 0 if collisions else None
        check(self.ctx.lib.sdgpu_oplog_add_device(self.h, _ptr(key), _ptr(tag), _ptr(ts), n,
                                                  _ptr(col), self._stream(key)),
              "sdgpu_oplog_add_device")
        return int(col.item()) if collisions else None

    def latest(self, key):
        """(ts int64, found uint8) per key; INT64_MIN and 0 for a key that is
        absent or holds no timestamp yet."""
        import torch
        n = key.numel()
        ts = torch.empty(max(n, 1), dtype=torch.int64, device=key.device)
        found = torch.empty(max(n, 1), dtype=torch.uint8, device=key.device)
        if n:
            check(self.ctx.lib.sdgpu_oplog_latest_device(self.h, _ptr(key), n, ts.data_ptr(),
                                                         found.data_ptr(), self._stream(key)),
                  "sdgpu_oplog_latest_device")
        return ts[:n], found[:n]

    def ingest(self, key, tag, ts, instance=None, clock=None, commit: bool = True,
               trim: bool = True):
        """(apply uint8 [n], applied int32, winner int32, counts int32 [4]) for
        one page in arrival order; `clock` (int64 [n_instances]) is updated in
        place.  counts = applied, winners, keys new to the log, tag
        disagreements.  commit=False (SDGPU_INGEST_NO_COMMIT): the same
        decisions, no timestamp in the log changes.  trim=False: full-length
        lists, no synchronisation."""
        import torch
        if (instance is None) != (clock is None):
            raise ValueError("instance and clock go together")
        n = key.numel()
        dev = key.device
        apply = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
        applied = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        winner = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        counts = torch.empty(4, dtype=torch.int32, device=dev)
        check(self.ctx.lib.sdgpu_sync_ingest_device(
            self.h, _ptr(key), _ptr(tag), _ptr(ts),
            None if instance is None else instance.data_ptr(), n,
            None if clock is None else clock.data_ptr(), 0 if clock is None else clock.numel(),
            0 if commit else NO_COMMIT, apply.data_ptr(), applied.data_ptr(), winner.data_ptr(),
            counts.data_ptr(), self._stream(key)), "sdgpu_sync_ingest_device")
        apply = apply[:n]
        if trim:
            c = counts.tolist()
            applied, winner = applied[:c[0]], winner[:c[1]]
        return apply, applied, winner, counts


def ingest_host(log: OpLog, key, tag, ts, instance=None, clock=None, commit: bool = True):
    """sdgpu_sync_ingest: the same on numpy arrays (uint64 keys, tags and clocks,
    int64 timestamps, uint32 instances); `clock` is updated in place; returns
    (apply, applied, winner, counts), the lists trimmed."""
    import numpy as np
    key = np.ascontiguousarray(key, dtype=np.uint64)
    tag = np.ascontiguousarray(tag, dtype=np.uint64)
    ts = np.ascontiguousarray(ts, dtype=np.int64)
    if instance is not None:
        instance = np.ascontiguousarray(instance, dtype=np.uint32)
        if clock.dtype != np.uint64 or not clock.flags.c_contiguous:
            raise ValueError("clock is a contiguous uint64 array, updated in place")
    n = key.size
    apply = np.empty(max(n, 1), dtype=np.uint8)
    applied = np.empty(max(n, 1), dtype=np.uint32)
    winner = np.empty(max(n, 1), dtype=np.uint32)
    counts = np.full(4, 0xFFFFFFFF, dtype=np.uint32)
    data = lambda a: None if a is None or a.size == 0 else a.ctypes.data  # noqa: E731
    check(log.ctx.lib.sdgpu_sync_ingest(
        log.h, data(key), data(tag), data(ts), None if instance is None else instance.ctypes.data,
        n, None if instance is None else clock.ctypes.data, 0 if instance is None else clock.size,
        0 if commit else NO_COMMIT, apply.ctypes.data, applied.ctypes.data, winner.ctypes.data,
        counts.ctypes.data), "sdgpu_sync_ingest")
    c = counts.tolist()
    return apply[:n], applied[:c[0]], winner[:c[1]], counts


class DeviceBackend:
    """What the Ingester asks of the device: keys through K1, the page decision
    (NO_COMMIT) and the commit, on numpy columns."""

    def __init__(self, ctx=None, capacity_hint: int = 0):
        self.ctx = ctx or default_context()
        self.log = OpLog(capacity_hint, self.ctx)

    def close(self):
        self.log.close()

    def keys(self, tuples, salt):
        return _tuple_keys(tuples, salt, self.ctx)

    def _dev(self, a):
        import numpy as np
        import torch
        a = np.ascontiguousarray(a)
        if a.dtype == np.uint64:
            a = a.view(np.int64)
        return torch.from_numpy(a.copy()).to(torch.device("cuda", self.ctx.device))

    def decide(self, key, tag, ts, instance, n_instances):
        """(applied, winners, tag disagreements, clocks) of one page; no
        timestamp in the log changes."""
        import numpy as np
        import torch
        inst = self._dev(np.asarray(instance, dtype=np.int32))
        clock = torch.zeros(n_instances, dtype=torch.int64, device=inst.device)
        _, applied, winner, counts = self.log.ingest(self._dev(key), self._dev(tag), self._dev(ts),
                                                     inst, clock, commit=False)
        return (applied.tolist(), winner.tolist(), int(counts[3]),
                [c & ((1 << 64) - 1) for c in clock.tolist()])

    def add(self, key, tag, ts):
        return self.log.add(self._dev(key), self._dev(tag), self._dev(ts))


class Ingester:
    """The actor's Ingesting state (ingest.rs:67-71) over in-memory op-log
    tables: ``shared_operation`` and ``relation_operation`` hold the rows
    ``CRDTOperation.row`` describes, ``timestamps`` the clock per instance uuid
    (unsigned NTP64).  The device log is loaded from the rows once and follows
    every page.  ``backend`` (default: ``DeviceBackend``) answers keys, decide
    and add."""

    def __init__(self, shared_operation=None, relation_operation=None, timestamps=None,
                 salt: int = 0, ctx=None, capacity_hint: int = 0, backend=None):
        self.shared_operation = list(shared_operation or [])
        self.relation_operation = list(relation_operation or [])
        self.timestamps = dict(timestamps or {})
        self.salt = salt
        n = len(self.shared_operation) + len(self.relation_operation)
        self.backend = backend or DeviceBackend(ctx, max(capacity_hint, n))
        if n:
            msgs = [(SHARED, r[2], r[3], r[4]) for r in self.shared_operation] \
                + [(RELATION, r[2], r[3], r[5]) for r in self.relation_operation]
            ts = [r[1] for r in self.shared_operation] + [r[1] for r in self.relation_operation]
            self._commit(msgs, ts)

    def close(self):
        if hasattr(self.backend, "close"):
            self.backend.close()

    def _commit(self, tuples, ts):
        import numpy as np
        if not tuples:
            return
        key, tag = self.backend.keys(tuples, self.salt)
        if self.backend.add(key, tag, np.asarray(ts, dtype=np.int64)):
            raise KeyCollision("two op tuples share a 64-bit key: re-key with another salt")

    def receive_page(self, ops, apply_op, winners_only: bool = False):
        """Ingests one page in order and returns the indices of the ops that
        were applied and logged.  The page is decided by one device call with
        NO_COMMIT; ``apply_op(op)`` is called for the applied ops in page
        order; their rows are appended to the op-log tables and committed to
        the device log with ``add``; ``timestamps`` follows every op, old or
        not (ingest.rs:119-126,151).

        When ``apply_op`` raises at index f the reference does not log that op
        (ingest.rs:162-166 returns before the create) and goes on: the applied
        ops below f are committed and the ops after f are ingested as a new
        page.  That is exact, because no decision before f depends on f.

        winners_only=True calls ``apply_op`` only for the highest applied op of
        every key (the value that survives in the row); every applied op is
        still logged.  That is the caller's shortcut, not the reference's
        behaviour: the reference runs every applied op's write.  When a
        winner's ``apply_op`` raises, the applied ops of its key that were
        skipped for its sake are not logged either (their writes never ran, so
        the log must not say they did); like the failed op they are given up,
        and the ops after the failure are decided against the log without
        them."""
        import numpy as np
        ops = list(ops)
        done = []
        first = 0
        while first < len(ops):
            page = ops[first:]
            tuples = [(o.table, o.name, o.id_bytes, o.kind) for o in page]
            ts = [o.stored_timestamp for o in page]
            key, tag = self.backend.keys(tuples, self.salt)
            who = {}
            inst = [who.setdefault(o.instance, len(who)) for o in page]
            applied, winner, bad, clock = self.backend.decide(
                key, tag, np.asarray(ts, dtype=np.int64), inst, len(who))
            if bad:
                raise KeyCollision("two op tuples share a 64-bit key: re-key with another salt")
            for u, c in zip(who, clock):
                self.timestamps[u] = max(self.timestamps.get(u, c), c)
            call = set(winner) if winners_only else None
            failed = None
            ok = []
            for i in applied:
                if call is None or i in call:
                    try:
                        apply_op(page[i])
                    except Exception:
                        failed = i
                        break
                ok.append(i)
            if failed is not None and call is not None:
                ok = [i for i in ok if i in call or key[i] != key[failed]]
            for i in ok:
                (self.shared_operation if page[i].table == SHARED
                 else self.relation_operation).append(page[i].row())
            self._commit([tuples[i] for i in ok], [ts[i] for i in ok])
            done += [first + i for i in ok]
            first = len(ops) if failed is None else first + failed + 1
        return done
