"""A pure-Python restatement of the indexer's rescan decision, on string tuples
and dicts.  It imports nothing from the product.

``diff_tuples`` follows the reference line by line: the per-directory
`to_remove` query (walk.rs:624-636, indexer/mod.rs:338-388) and
filter_existing_paths (walk.rs:309-381, indexer/mod.rs:305-331).
``diff_keys`` restates the device call's contract (include/sdgpu.h) on integer
keys, so that it stays defined for duplicated keys.  ``to_columns`` turns the
first's input into the second's, and ``CASES`` pins each rule by hand.

An entry is (materialized_path, name, extension, is_dir, inode, device,
modified_at ns); a row is (id, materialized_path, name, extension, is_dir,
inode, device, date_modified ns), the last three possibly None.  A walk is a
list of (children_path, paths_buffer) per directory whose listing was read, in
walk order; an ancestor pushed from a deeper directory sits in that
directory's buffer (walk.rs:575-617).
"""

MISS = 0xFFFFFFFF
CREATE, UNCHANGED, UPDATE, KIND_CHANGED = 0, 1, 2, 3
T0 = 1_700_000_000_000_000_000
MS = 1_000_000


def diff_tuples(walk, rows):
    """(to_create [4-tuples], to_update [(row id, 4-tuple)], to_remove [row ids])."""
    indexed = {}       # HashSet<WalkingEntry>: Eq over the iso_file_path, is_dir included
    to_remove = set()
    for children_path, buffer in walk:
        # to_remove_db_fetcher_fn: the 4-term query does not look at is_dir ...
        wanted = {e[:3] for e in buffer}
        found_ids = {r[0] for r in rows if r[1:4] in wanted}
        # ... then materialized_path == the directory's AND id NOT IN found
        to_remove |= {r[0] for r in rows if r[1] == children_path and r[0] not in found_ids}
        for e in buffer:   # indexed_paths.extend(paths_buffer.drain(..))
            indexed.setdefault(e[:4], e)
    # filter_existing_paths: the 4-term query, then a HashMap keyed by
    # IsolatedFilePathData, whose Hash / Eq include is_dir
    wanted = {k[:3] for k in indexed}
    in_db = {r[1:5]: r for r in rows if r[1:4] in wanted}
    to_create, to_update = [], []
    for k, e in indexed.items():
        r = in_db.get(k)
        if r is None:
            to_create.append(k)
            continue
        inode, device, date_modified = r[5:8]
        if inode is not None and device is not None and date_modified is not None:
            if inode != e[4] or device != e[5] or e[6] - date_modified > MS:
                to_update.append((r[0], k))
    return to_create, to_update, sorted(to_remove)


def apply_tuples(rows, walk, result, next_id):
    """The rows after the indexer's writes: removes, create_many().
    skip_duplicates() (indexer/mod.rs:182), metadata updates.  Returns (rows,
    ids whose cas_id is cleared)."""
    to_create, to_update, to_remove = result
    entry = {}
    for _, buffer in walk:
        for e in buffer:
            entry.setdefault(e[:4], e)
    rows = [r for r in rows if r[0] not in set(to_remove)]
    for k in to_create:
        if k[:3] in {r[1:4] for r in rows}:
            continue
        rows.append((next_id,) + entry[k])
        next_id += 1
    cleared = []
    for rid, k in to_update:
        rows = [r[:5] + entry[k][4:7] if r[0] == rid else r for r in rows]
        cleared.append(rid)
    return rows, cleared


def diff_keys(w_key, w_flags, w_meta, wd_key, r_key, r_dirkey, r_flags, r_meta):
    """The contract on integer keys: (create, update, remove, match, state,
    counts).  Flags may be None (all 0); the modified_at column is signed."""
    n_w, n_r = len(w_key), len(r_key)
    w_flags = [0] * n_w if w_flags is None else w_flags
    r_flags = [0] * n_r if r_flags is None else r_flags
    first = {}
    for j, k in enumerate(r_key):
        first.setdefault(k, j)
    match, state = [], []
    for i, k in enumerate(w_key):
        j = first.get(k)
        if j is None:
            match.append(MISS)
            state.append(CREATE)
            continue
        match.append(j)
        if (r_flags[j] ^ w_flags[i]) & 1:
            state.append(KIND_CHANGED)
        elif not r_flags[j] & 2 and (w_meta[i][0] != r_meta[j][0] or w_meta[i][1] != r_meta[j][1]
                                     or w_meta[i][2] - r_meta[j][2] > MS):
            state.append(UPDATE)
        else:
            state.append(UNCHANGED)
    listed = {k for k, f in zip(w_key, w_flags) if not f & 2}
    walked_dirs = set(wd_key)
    create = [i for i, s in enumerate(state) if s in (CREATE, KIND_CHANGED)]
    update = [i for i, s in enumerate(state) if s == UPDATE]
    remove = [j for j in range(n_r) if r_dirkey[j] in walked_dirs and r_key[j] not in listed]
    counts = [len(create), len(update), len(remove), state.count(KIND_CHANGED)]
    return create, update, remove, match, state, counts


def to_columns(walk, rows):
    """The walk and the rows as the call's columns, with injective integer keys
    (an odd multiple of a string's rank, mod 2^64).  Also returns the walked
    4-tuples in entry order.  An entry is an ANCESTOR when no buffer of its own
    parent directory holds it."""
    paths = sorted({e[:3] for _, b in walk for e in b} | {r[1:4] for r in rows})
    dirs = sorted({cp for cp, _ in walk} | {r[1] for r in rows})
    pk = {p: (i + 1) * 0x9E3779B97F4A7C15 % 2**64 for i, p in enumerate(paths)}
    dk = {d: (i + 1) * 0xD1B54A32D192ED03 % 2**64 for i, d in enumerate(dirs)}
    indexed, listed = {}, set()
    for cp, buffer in walk:
        for e in buffer:
            indexed.setdefault(e[:4], e)
            if e[0] == cp:
                listed.add(e[:4])
    entries = list(indexed.values())
    w_key = [pk[e[:3]] for e in entries]
    w_flags = [(1 if e[3] else 0) | (0 if e[:4] in listed else 2) for e in entries]
    w_meta = [list(e[4:7]) for e in entries]
    wd_key = [dk[cp] for cp, _ in walk]
    r_key = [pk[r[1:4]] for r in rows]
    r_dirkey = [dk[r[1]] for r in rows]
    r_flags = [(1 if r[4] else 0) | (2 if None in r[5:8] else 0) for r in rows]
    r_meta = [[v or 0 for v in r[5:8]] for r in rows]
    return (w_key, w_flags, w_meta, wd_key, r_key, r_dirkey, r_flags, r_meta), \
        [e[:4] for e in entries]


def tuples_from_keys(result, names, rows):
    """diff_keys' lists in diff_tuples' terms."""
    create, update, remove, match, _, _ = result
    return ([names[i] for i in create], [(rows[match[i]][0], names[i]) for i in update],
            [rows[j][0] for j in remove])


def _f(mp, name, ext, inode=10, device=1, mtime=T0):
    return (mp, name, ext, False, inode, device, mtime)


def _d(mp, name, inode=20, device=1, mtime=T0):
    return (mp, name, "", True, inode, device, mtime)


def _row(rid, e, **over):
    m = dict(inode=e[4], device=e[5], mtime=e[6])
    m.update(over)
    return (rid,) + e[:4] + (m["inode"], m["device"], m["mtime"])


def _one(entry, **row_over):
    return [("/", [entry])], [_row(1, entry, **row_over)]


_A = _f("/", "a", "txt")
_SUB = _d("/", "sub")

# name -> (walk, rows, to_create, to_update, to_remove)
CASES = {
    "mtime_delta_exactly_1ms": _one(_f("/", "a", "txt", mtime=T0 + MS), mtime=T0) + ([], [], []),
    "mtime_delta_1ms_1ns": _one(_f("/", "a", "txt", mtime=T0 + MS + 1), mtime=T0)
    + ([], [(1, _A[:4])], []),
    "row_one_hour_newer": _one(_A, mtime=T0 + 3600 * 1000 * MS) + ([], [], []),
    "inode_only": _one(_A, inode=11) + ([], [(1, _A[:4])], []),
    "device_only": _one(_A, device=2) + ([], [(1, _A[:4])], []),
    "no_metadata_row": _one(_f("/", "a", "txt", inode=77, device=7, mtime=T0 + 5000 * MS),
                            inode=None) + ([], [], []),
    # the row says file, the disk says directory: created again, and NOT removed
    "file_replaced_by_directory": ([("/", [_d("/", "x")])], [_row(1, _f("/", "x", ""))],
                                   [("/", "x", "", True)], [], []),
    # /sub failed an accept rule in its parent's listing but was walked; its
    # accepted child pushed it as an ancestor: its row goes with the listing of
    # "/" and yet the entry is not created (the row was there when asked)
    "ancestor_only_entry": ([("/", []), ("/sub/", [_f("/sub/", "f", "txt"), _SUB])],
                            [_row(1, _SUB), _row(2, _f("/sub/", "f", "txt"))], [], [], [1]),
    "rule_rejected_entry": ([("/", [_A])], [_row(1, _f("/", "secret", "key")), _row(2, _A)],
                            [], [], [1]),
    "unwalked_directory": ([("/", [_SUB])], [_row(1, _SUB), _row(2, _f("/sub/", "f", "txt"))],
                           [], [], []),
    "vanished_sub_directory": ([("/", [])],
                               [_row(1, _d("/", "gone")), _row(2, _f("/gone/", "f", "txt")),
                                _row(3, _f("/gone/deep/", "g", ""))], [], [], [1]),
}
