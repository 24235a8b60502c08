"""CPU: the poison knob is reachable only behind SDGPU_POISON_WS, and the
reference side of every scenario of tests/_poison_child.py is well formed --
the oracle runs, the shapes are the ones the scenario is meant to have, and the
rejected messages are exactly the ones the header's rules reject.  (The GPU
side is tests/test_gpu_poison_entry_points.py.)"""
import glob
import os
import re

import numpy as np
import pytest

from tests import _poison_child as P

CSRC = os.path.join(P.ROOT, "spacedrive_amd", "csrc")


def _sources():
    return {p: open(p).read() for ext in ("hpp", "cpp", "hip")
            for p in sorted(glob.glob(os.path.join(CSRC, "*." + ext)))}


def _body(text, signature):
    """The brace-balanced body of the function whose definition starts with `signature`."""
    at = text.index(signature)
    i = text.index("{", at)
    depth, j = 0, i
    while True:
        depth += {"{": 1, "}": -1}.get(text[j], 0)
        if depth == 0:
            return text[i:j + 1]
        j += 1


def test_poison_is_reachable_only_behind_the_knob():
    src = _sources()
    ctx = src[os.path.join(CSRC, "ctx.hpp")]
    # the log line exists in the two fill helpers and nowhere else
    dev, host = _body(ctx, "inline int poison_dev("), _body(ctx, "inline void poison_host(")
    assert dev.count("sdgpu: poisoned") == 1 and host.count("sdgpu: poisoned") == 1
    assert sum(t.count("sdgpu: poisoned") for t in src.values()) == 2
    assert "hipDeviceSynchronize()" in dev and "0xA5" in dev and "0xA5" in host
    # the knob is read once, into a static
    knob = _body(ctx, "inline bool poison_ws()")
    assert re.search(r'static const bool on = std::getenv\("SDGPU_POISON_WS"\)', knob)
    # every call of a helper is the statement of an `if (poison_ws() ...)`
    calls = 0
    for path, text in src.items():
        for m in re.finditer(r"\bpoison_(dev|host)\(", text):
            line_start = text.rfind("\n", 0, m.start()) + 1
            line = text[line_start:text.index("\n", m.start())].strip()
            if line.startswith("inline "):
                continue  # the definitions
            assert re.match(r"if \((sdgpu::)?poison_ws\(\)( &&|\))", line), (path, line)
            calls += 1
    # ensure_dev, grow_dev_keep, ensure_pin, index_alloc, the three host-API calls
    assert calls == 7
    # the caller's own buffers are never filled
    sd = src[os.path.join(CSRC, "sdgpu.cpp")]
    for fn in ("int sdgpu_alloc_device(", "int sdgpu_alloc_pinned("):
        assert "poison" not in _body(sd, fn)


def test_parse_log_attributes_lines_to_calls():
    err = "\n".join([
        "sdgpu: poisoned 1048576 before_any_marker",
        f"{P.MARK} a call 0", "sdgpu: poisoned 1048576 batch_ws", "noise",
        "sdgpu: poisoned 65536 pipe_h",
        f"{P.MARK} a call 1",
        f"{P.MARK} a end", "sdgpu: poisoned 1 between",
        f"{P.MARK} b call 0", "sdgpu: poisoned 32800 index_table"])
    assert P.parse_log(err) == {"a": [["batch_ws", "pipe_h"], []], "b": [["index_table"]]}


@pytest.fixture(scope="module")
def facts(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("poison")
    cache = {}

    def get(name):
        if name not in cache:
            cache[name], run = P.SCENARIOS[name][0](str(tmp / name))
            assert callable(run)
        return cache[name]
    return get


def test_k1_batches(facts):
    f = facts("k1_bulk")
    assert f["n_large"] == 3000 and f["n_small"] == 5 and f["lengths_present"]
    # the header's rules reject the two messages built to be rejected, and only them
    assert f["invalid_rows"] == sorted(f["rejected"]) and len(f["rejected"]) == 2
    assert f["rejected_status"] == [-22, -22] and f["rejected_ids_zero"]
    assert f["small_invalid"] == 0 and f["small_has_empty"]
    assert f["whole_flags"] == [0, 1] and f["empty_body_has_checksum"]
    assert 1000 < f["n_checksums"] < 2000
    assert facts("k1_body") == f


def test_kind_batches(facts):
    for name in ("kind_default", "kind_verify"):
        f = facts(name)
        assert f["n"] > 2900 and f["n_small"] == 3 and len(f["kinds"]) > 10


def test_tree_plan(facts):
    f = facts("tree")
    assert f["sizes"] == [0, 1, 1024, 1025, 16384, 16385, (1 << 20) + 1, 5 * (1 << 20) + 123]
    assert f["small"] == [1]


def test_streamed_files(facts):
    f = facts("streamed")
    assert f["slice"] == 64 << 20
    assert f["sizes"] == [2 * f["slice"] + 1, f["slice"] - 1] and f["digests_differ"]


def test_latency_files(facts):
    assert facts("latency")["sizes"] == [300 << 10, 113 << 10, 1 << 20, 4 << 10, 300 << 10]
    assert facts("latency_small_first")["sizes"][0] == 4 << 10


def test_identify_directories(facts):
    for name in ("identify_files", "identify_checksum_files", "identify_kind_files"):
        f = facts(name)
        assert f["n"] == 309 and f["n_small"] == 2 and f["missing"] == 1 and f["empty"] == 11
        assert f["keys"] == 309 - 1 - 11 and f["checksums"] == 11 * 23
        assert len(f["kinds"]) >= 5 and 0 in f["kinds"]
        assert f["staged_bytes"] <= 32 << 20            # one slab
    for name in ("identify_checksum_many_slabs", "identify_kind_many_slabs"):
        f = facts(name)
        assert f["n"] == 909
        assert f["staged_bytes"] > 4 * (16 << 20)       # five slabs of 16 MiB, three slots


def test_stage_pinned_messages(facts):
    f = facts("stage_pinned")
    assert f["status"] == [0] * 8 + [-22, -22] and f["rejected_ids_zero"] and f["n_small"] == 1


def test_k7_rows(facts):
    for name, invalid in (("k7_implicit", False), ("k7_valid", True), ("k7_permuted_ranks", True)):
        f = facts(name)
        assert f["n"] == 65_537 and f["creators"] > 1000 and f["linked"] > 1000
        assert (f["invalid"] > 0) == invalid
        assert f["creators"] + f["linked"] + f["invalid"] == f["n"]
    f = facts("k7_permuted_ranks")
    assert f["rank_is_permutation"] and not f["rank_is_identity"]


def test_extra_entry_rows(facts):
    for name, n in (("extra_4097", 4097), ("extra_65537_unaligned", 65_537)):
        f = facts(name)
        assert f["n"] == n and f["invalid_rows_are_keyless"]
        assert 0.15 < f["keyless"] < 0.25 and 0.03 < f["invalid"] < 0.07
        assert 0.2 < f["by_index"] < 0.4


def test_consumer_rows(facts):
    for name in ("orphans_trim", "orphans_full"):
        f = facts(name)
        assert f["null"] > 500 and f["past_max_id"] > 200 and 0 < f["orphans"] < 4097
        assert f["small_orphans"] == f["small_ids"] and len(f["small_ids"]) == 1
    for name in ("thumbnail_shards_trim", "thumbnail_shards_full"):
        f = facts(name)
        assert 9000 < f["rows_ordered"] < 10_000 and f["directories"] == 256


def test_index_and_host_api_rows(facts):
    f = facts("index")
    assert f["n"] == 4000 and f["first_key_is_all_ones"] and f["absent"] == 500
    for name in ("host_dedup", "host_dedup_batch", "host_dedup_sharded"):
        f = facts(name)
        assert f["n"] == 1000 and f["n_small"] == 3
        assert 100 < f["groups"] < 1000 and f["linked_to_existing"] > 50


def test_every_scenario_is_checked_here(facts):
    """A scenario added to the child is also built on the CPU."""
    text = open(__file__).read()
    for name in P.SCENARIOS:
        assert f'"{name}"' in text, name
        facts(name)
    assert np.uint8(P.POISON) == 0xA5
