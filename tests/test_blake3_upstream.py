"""The oracle against the BLAKE3 project's own implementation (CPU).

tests/golden/blake3_upstream.json holds digests and chunk chaining values
computed by the official BLAKE3 C code that the ROCm toolchain's LLVM vendors
(tests/golden/make_blake3_upstream.py).  Every multi-chunk parity test of the
GPU suite compares with oracle/sd_oracle.c, which only oracle/blake3_py.py
checked, both written here from one reading of the specification; these tests
pin both to code from outside the repository: parent nodes, ROOT on a parent,
the left-subtree power-of-two rule (hash / cas entries up to 65537 chunks) and
chunk counters up to 2^64 - 2^32 (leaf_cv entries)."""
import subprocess
import sys

import numpy as np
import pytest

from oracle import blake3_py as P
from oracle import oracle as O
from tests import upstream_vectors as U

PY_MAX = 300 * 1024   # pure Python and byte-wise incremental hashing above this is slow
FAMILIES = ["mod251", "mix"]


def _cas_message(e) -> bytes:
    """The bytes generate_cas_id hashes for a file holding the family's first
    `size` bytes: u64_le(size) || whole file, or the sampled message."""
    body = U.data(e["family"], e["size"])
    if e["size"] <= U.WHOLE_READ_MAX:
        return e["size"].to_bytes(8, "little") + body.tobytes()
    return O.cas_build_message(body)


def _messages(family):
    """(label, message bytes as uint8 array, upstream digest hex) of every
    `hash` and `cas` entry of a family."""
    fix = U.fixture()
    for e in fix["hash"]:
        if e["family"] == family:
            yield ("hash", e["len"]), U.data(family, e["len"]), e["digest"]
    for e in fix["cas"]:
        if e["family"] == family:
            yield ("cas", e["size"]), np.frombuffer(_cas_message(e), np.uint8), e["digest"]


def test_fixture_shape():
    """The parts and cases the fixture must hold (a truncated or hand-edited
    file would let every test below pass on fewer entries)."""
    fix = U.fixture()
    edge = [2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 100, 101, 111, 112, 113, 127,
            128, 129, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 65535, 65536, 65537]
    lens = {f: sorted(e["len"] for e in fix["hash"] if e["family"] == f) for f in FAMILIES}
    want = {n for c in edge for n in (c * 1024 - 1023, c * 1024 - 1, c * 1024)}
    assert lens["mod251"] == sorted(want | set(U.PUBLISHED))
    assert lens["mix"] == sorted({n for n in want if n < 65535 * 1024 - 1023} | {0, 1, 64, 1024})
    for f in FAMILIES:
        sizes = sorted(e["size"] for e in fix["cas"] if e["family"] == f)
        assert sizes == [n for n in lens[f] if n <= U.WHOLE_READ_MAX] + [102401, 500000, 3145733]
        leaf = [e for e in fix["leaf_cv"] if e["family"] == f]
        ctr = sorted(e["chunk_counter"] for e in leaf if e["len"] == 1024)
        assert ctr == sorted(b + j for b in ((1 << 32) - 32, 1 << 32, (1 << 40) + (1 << 32),
                                             (1 << 64) - (1 << 32)) for j in range(32))
        assert sorted(e["len"] for e in leaf if e["len"] != 1024) == [1, 1023]
    assert len({e["cv"] for e in fix["leaf_cv"]}) == len(fix["leaf_cv"])
    by = {(e["family"], e["len"]): e["digest"] for e in fix["hash"]}
    assert by["mod251", 0] == "af1349b9f5f9a1a6a0404dea36dcc9499bcb25c9adc112b7cc9a93cae41f3262"
    assert by["mod251", 1025] == "d00278ae47eb27b34faecf67b4fe263f82d5412916c1ffd97c8cb7fb814b8444"
    assert by["mod251", 102400] == \
        "bc3e3d41a1146b069abffad3c0d44860cf664390afce4d9661f7902e7943e085"


@pytest.mark.parametrize("family", FAMILIES)
def test_c_oracle_matches_upstream(family):
    """orc_blake3 (one thread, 8 threads), the incremental hasher in pieces of
    1, 63 and 1025 bytes, the SIMD hasher and cas_id_of_message on every hash
    and cas entry."""
    n = 0
    for label, msg, want in _messages(family):
        d = bytes.fromhex(want)
        assert O.blake3(msg) == d, label
        assert O.blake3(msg, threads=8) == d, label
        assert O.blake3_simd(msg) == d, label
        assert O.cas_id_of_message(msg) == want[:16], label
        if msg.size <= PY_MAX:
            for piece in (1, 63, 1025):
                assert O.blake3_incremental(msg, piece) == d, (label, piece)
        n += 1
    fix = U.fixture()
    assert n == sum(e["family"] == family for e in fix["hash"] + fix["cas"]) and n > 100


@pytest.mark.parametrize("family", FAMILIES)
def test_python_restatement_matches_upstream_hash(family):
    """blake3_py on every hash entry of at most 300 KiB.  The inputs of a
    family are prefixes of one stream and finalize() does not change the
    hasher, so the stream is fed once and finalized at every length: what
    blake3(prefix) = Hasher().update(prefix).finalize() computes, without
    hashing each prefix from its first byte again.  The lengths up to 8193 are
    also hashed by blake3() itself."""
    lens = sorted(e["len"] for e in U.fixture()["hash"]
                  if e["family"] == family and e["len"] <= PY_MAX)
    want = {e["len"]: e["digest"] for e in U.fixture()["hash"] if e["family"] == family}
    assert len(lens) >= 80 and lens[-1] == 257 * 1024
    stream = U.data(family, lens[-1]).tobytes()
    h, fed = P.Hasher(), 0
    for n in lens:
        h.update(stream[fed:n])
        fed = n
        assert h.finalize().hex() == want[n], n
        if n <= 8193:
            assert P.blake3(stream[:n]).hex() == want[n], n


@pytest.mark.parametrize("family", FAMILIES)
def test_python_restatement_matches_upstream_cas(family):
    """blake3_py.blake3 on every cas message (all are below 300 KiB), and its
    own message builder (cas_id_of_file_bytes) on the sampled files."""
    n = 0
    for e in U.fixture()["cas"]:
        if e["family"] != family:
            continue
        assert P.blake3(_cas_message(e)).hex() == e["digest"], e["size"]
        if e["size"] > U.WHOLE_READ_MAX:
            body = U.data(family, e["size"]).tobytes()
            assert P.cas_id_of_file_bytes(body) == e["digest"][:16], e["size"]
        n += 1
    assert n > 50


def test_python_chunk_compression_with_recorded_counters():
    """A chunk's chaining value depends on its counter, low and high word:
    blake3_py's chunk state at the recorded counter gives the upstream CV, and
    at the counter's low word alone (what a kernel that dropped the high word
    would use) or at 0 it does not."""
    import struct
    fix = U.fixture()
    for e in fix["leaf_cv"]:
        chunk = U.data(e["family"], e["len"], e["input_offset"]).tobytes()

        def cv(counter):
            st = P._ChunkState(P.IV, counter, 0)
            st.update(chunk)
            return struct.pack("<8I", *st.output().chaining_value()).hex()

        assert cv(e["chunk_counter"]) == e["cv"], e
        assert e["chunk_counter"] >= (1 << 32) - 32
        assert cv(e["chunk_counter"] & 0xFFFFFFFF) != e["cv"] or e["chunk_counter"] < (1 << 32)
        assert cv(0) != e["cv"]
    assert len(fix["leaf_cv"]) == 2 * (4 * 32 + 2)


def test_fixture_regenerates_from_the_upstream_library():
    """make_blake3_upstream.py --check in a child process (the compiler library
    is not loaded beside torch): the committed fixture is what the toolchain's
    BLAKE3 computes today.  Skips only where no library exports the symbol."""
    r = subprocess.run([sys.executable, U.GENERATOR, "--check"], capture_output=True, text=True,
                       timeout=300)
    if r.returncode == 3:
        pytest.skip("no shared library exporting llvm_blake3_hasher_init on this machine")
    assert r.returncode == 0, r.stdout + r.stderr
    assert "matches" in r.stdout
