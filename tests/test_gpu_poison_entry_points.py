"""GPU: no result of any device entry point depends on a byte the call did
not write -- neither in the library's workspaces nor in the output buffers.

Every scenario of tests/_poison_child.py runs in a fresh process with
SDGPU_POISON_WS=1 (every buffer the library allocates for itself starts as
0xA5 bytes and is logged, csrc/ctx.hpp) and with the wrappers' output buffers
filled with 0xA5 bytes, on a context of its own: a large call (the one that
allocates, so it reads poison), a small one of another shape (it reads the
large call's leftovers), and the large one again.  Every call must equal the
oracle at every element the header documents as written, and the first call's
log must show that the buffers the scenario is about were really allocated,
and so poisoned, by it: a scenario that ran warm proves nothing.
"""
import pytest

from tests import _poison_child as P

pytestmark = pytest.mark.gpu


def _check(names, env=None):
    rc, out, log, err = P.launch(names, env)
    assert rc == 0, err[-3000:]
    print({n: (r["host_seconds"], r["gpu_seconds"]) for n, r in out.items()})
    for name in names:
        r = out[name]
        assert len(r["bad"]) >= 3 and not any(r["bad"]), (name, r["bad"])
        assert (r["outputs_poisoned"] > 0) != (name in P.NO_WRAPPER_OUTPUTS), name
        assert len(log[name]) == len(r["bad"])
        for buf in P.SCENARIOS[name][1]:
            assert buf in log[name][0], (name, buf, log[name][0])


def test_k1_and_body_pass():
    """sdgpu_cas_batch_device / sdgpu_cas_checksum_batch_device: 3000 messages
    (units, ragged items, multi-unit folds, the sort histograms and the
    work-queue counter all live) with two rejected ones, then 5, then again."""
    _check(["k1_bulk", "k1_body"])


def test_kind_batch():
    """sdgpu_kind_batch_device in both modes (no workspace: outputs only)."""
    _check(["kind_default", "kind_verify"])


def test_tree_checksum_batch():
    """sdgpu_checksum_batch_device: 0 B .. 5 MiB in one plan, then one byte."""
    _check(["tree"])


def test_streamed_file_checksum():
    """sdgpu_file_checksum over three slices (both pipe slots, the slice CVs in
    a grown buffer), then one slice less a byte.  Writes and reads 192 MiB."""
    _check(["streamed"])


def test_latency_kernels():
    """file_checksum and generate_cas_id of small files: k_small_split first
    on a fresh context, and k_small_host first on another."""
    _check(["latency", "latency_small_first"])


def test_identify_from_paths():
    """sdgpu_identify_files / _checksum_files / _kind_files: 308 files at the
    size edges, a missing one, empty ones; then 2 files; then again."""
    _check(["identify_files", "identify_checksum_files", "identify_kind_files"])


def test_identify_from_paths_many_slabs():
    """The same with 600 more whole files, so that five slabs go through the
    three staging slots (SDGPU_SLAB_DIV=64: the smallest slabs allowed)."""
    _check(["identify_checksum_many_slabs", "identify_kind_many_slabs"], {"SDGPU_SLAB_DIV": "64"})


def test_stage_pinned():
    """sdgpu_cas_stage_pinned: the edge messages with two rejected ones."""
    _check(["stage_pinned"])


def test_link_batch():
    """K7 at 17 scan tiles (the last ragged): implicit ranks, a valid mask,
    and explicit ranks that are a permutation."""
    _check(["k7_implicit", "k7_valid", "k7_permuted_ranks"])


def test_fused_extra_entries_through_an_index():
    """sdgpu_group_link_device with registered Objects, keyless and invalid
    rows; once with has / valid at a 1-byte offset."""
    _check(["extra_4097", "extra_65537_unaligned"])


def test_consumers():
    """sdgpu_orphan_objects_device and sdgpu_thumbnail_shards_device, trimmed
    and full-length."""
    _check(["orphans_trim", "orphans_full", "thumbnail_shards_trim", "thumbnail_shards_full"])


def test_object_index():
    """Add with growth by rehash from 1024 slots, lookup (device and host),
    conditional removal, removal by Object id, export -- against the model."""
    _check(["index"])


def test_host_api_calls():
    """sdgpu_dedup, sdgpu_dedup_batch (with and without an index) and
    sdgpu_dedup_sharded at world 3: 1000 rows, then 3, then again."""
    _check(["host_dedup", "host_dedup_batch", "host_dedup_sharded"])
