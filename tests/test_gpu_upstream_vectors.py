"""GPU parity against the BLAKE3 project's own implementation, one test per
hashing path: the digests and chunk chaining values of
tests/golden/blake3_upstream.json (made by the official C code the toolchain's
LLVM vendors, tests/golden/make_blake3_upstream.py) instead of the repository's
own oracle.  The inputs are rebuilt from the two formulas the fixture states;
nothing here loads the upstream library or the oracle's hashers.

Every test computes from the fixture the entries its path can take, runs all
of them, and asserts how many it consumed: no entry in a path's range is left
out for another reason.

What pins what: parent nodes, ROOT on a parent and the left-subtree rule by
the whole-message digests (up to 65537 chunks) on every path; chunk counters
at and beyond 2^32 by the leaf_cv entries through subtree_device."""
import os
import struct

import numpy as np
import pytest

from oracle import blake3_py as P
from tests import upstream_vectors as U

pytestmark = pytest.mark.gpu

FAMILIES = ["mod251", "mix"]
CAS_MAX = 102408                 # largest cas message: K1 and sdgpu_cas_batch take no longer one
LATENCY_MAX = (1 << 20) + 1024   # file_checksum: k_small_host / k_service / k_small_split, and
                                 # the first sizes past their 1 MiB limit
SAMPLED = [102401, 500000, 3 * (1 << 20) + 5]


def _hash(family=None, lo=0, hi=None):
    return [e for e in U.fixture()["hash"]
            if (family is None or e["family"] == family) and e["len"] >= lo
            and (hi is None or e["len"] <= hi)]


def _arena(entries):
    """(arena, off, len) of the entries' messages, 16-B aligned, disjoint."""
    off = np.zeros(len(entries), np.uint64)
    pos = 0
    for i, e in enumerate(entries):
        off[i] = pos
        pos += (e["len"] + 15) // 16 * 16 + 16
    arena = np.full(pos + 16, 0xA5, np.uint8)
    for i, e in enumerate(entries):
        arena[int(off[i]):int(off[i]) + e["len"]] = U.data(e["family"], e["len"])
    return arena, off, np.array([e["len"] for e in entries], np.uint32)


@pytest.fixture()
def svc_ctx():
    """A separate context with the resident latency service on (k_service)."""
    from spacedrive_amd._native import Context
    c = Context(0)
    c.latency_service(True)
    yield c
    c.latency_service(False)
    c.close()


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """{(family, len): path} of one file per hash length up to 1 MiB + 1024 and
    per sampled cas size."""
    root = tmp_path_factory.mktemp("upstream")
    out = {}
    want = {(e["family"], e["len"]) for e in _hash(hi=LATENCY_MAX)}
    want |= {(e["family"], e["size"]) for e in U.fixture()["cas"]}
    for fam, n in sorted(want):
        p = os.path.join(root, f"{fam}_{n}.bin")
        U.data(fam, n).tofile(p)
        out[fam, n] = p
    return out


@pytest.fixture(scope="module")
def device_streams():
    """{family: the family's byte stream on the device}; a message of n bytes
    is the view [:n] (16-B aligned, followed by more of the stream, not by
    zeros)."""
    import torch
    return {f: torch.from_numpy(np.array(U.data(f, max(e["len"] for e in _hash(f))))).cuda()
            for f in FAMILIES}


# ---- K1 bulk ------------------------------------------------------------------

def test_k1_bulk_arbitrary_messages(ctx):
    """k_leaves3 / k_fold3: every hash entry of at most 102 408 B as one message
    of a cas_batch_device call of more than 64 messages."""
    import torch
    from spacedrive_amd import cas
    entries = _hash(hi=CAS_MAX)
    eligible = len(entries)
    assert eligible > 0
    batch = entries + entries[:max(0, 65 - eligible)]   # repeats: the bulk path needs > 64
    assert len(batch) > 64
    arena, off, ln = _arena(batch)
    out, st = cas.cas_batch_device(torch.from_numpy(arena).cuda(),
                                   torch.from_numpy(off.view(np.int64)).cuda(),
                                   torch.from_numpy(ln.view(np.int32)).cuda(), ctx=ctx)
    torch.cuda.synchronize()
    assert not st.cpu().numpy().any()
    got = out.cpu().numpy()
    used = 0
    for i, e in enumerate(batch):
        assert bytes(got[i]).hex() == e["digest"][:16], (e["family"], e["len"])
        used += i < eligible
    assert used == eligible == len(_hash(hi=CAS_MAX))


# ---- k_small_host ---------------------------------------------------------------

def test_small_host_batches_of_1_and_64(ctx):
    """cas_batch of at most 64 messages is one k_small_host launch: the same
    messages one per call, then 64 per call."""
    from spacedrive_amd import cas
    entries = _hash(hi=CAS_MAX)
    assert entries
    for per in (1, 64):
        used = 0
        for a in range(0, len(entries), per):
            part = entries[a:a + per]
            arena, off, ln = _arena(part)
            out, st = cas.cas_batch(arena, off, ln, ctx)
            assert not st.any()
            for i, e in enumerate(part):
                assert bytes(out[i]).hex() == e["digest"][:16], (per, e["family"], e["len"])
                used += 1
        assert used == len(entries)


# ---- body pass, cas_id of real files ---------------------------------------------

def test_identify_whole_read_files(ctx, files):
    """One identify(checksums=True) over a file per cas entry of at most
    100 KiB: cas_id = the cas digest's first 8 bytes (K1 over size_le || file),
    integrity_checksum = the hash digest of the same bytes (k_leaves3<8> /
    k_fold3<8>, the message without its prefix)."""
    from spacedrive_amd import cas
    from spacedrive_amd import file_identifier as fi
    entries = [e for e in U.fixture()["cas"] if e["size"] <= U.WHOLE_READ_MAX]
    digest = {(e["family"], e["len"]): e["digest"] for e in _hash()}
    assert len(entries) > 64
    paths = [files[e["family"], e["size"]] for e in entries]
    res = fi.identify(paths, np.array([e["size"] for e in entries], np.uint64), ctx=ctx,
                      checksums=True)
    assert not res.status.any()
    ids, sums = res.cas_ids(), res.checksums()
    used = empty = 0
    for i, e in enumerate(entries):
        if e["size"] == 0:
            continue
        assert ids[i] == e["digest"][:16], (e["family"], e["size"])
        assert sums[i] == digest[e["family"], e["size"]], (e["family"], e["size"])
        used += 1
    # an empty file has no cas_id and no checksum in the batched call (its row
    # stays without an Object); the single-file drop-in hashes the 8 zero bytes
    for i, e in enumerate(entries):
        if e["size"] == 0:
            assert ids[i] is None and sums[i] is None
            assert cas.generate_cas_id(paths[i], 0, ctx) == e["digest"][:16]
            empty += 1
    assert empty == len(FAMILIES) and used + empty == len(entries)


def test_generate_cas_id_sampled_files(ctx, svc_ctx, files):
    """Files above 100 KiB: the 57 352-B sampled message, through the one-shot
    path and through the latency service."""
    from spacedrive_amd import cas
    entries = [e for e in U.fixture()["cas"] if e["size"] > U.WHOLE_READ_MAX]
    assert sorted(e["size"] for e in entries) == sorted(SAMPLED * len(FAMILIES))
    used = 0
    for e in entries:
        p = files[e["family"], e["size"]]
        for c in (ctx, svc_ctx):
            assert cas.generate_cas_id(p, e["size"], c) == e["digest"][:16], (e["family"],
                                                                                e["size"])
        used += 1
    assert used == len(entries)


# ---- k_service, k_small_split -------------------------------------------------------

@pytest.mark.parametrize("service", [False, True], ids=["launch", "service"])
def test_file_checksum_latency_paths(ctx, svc_ctx, files, service):
    """file_checksum of a file per hash length up to 1 MiB + 1024: k_small_host
    (launch) or k_service (service) up to 112 KiB, k_small_split up to 1 MiB,
    the streaming path just past it."""
    from spacedrive_amd import validation
    c = svc_ctx if service else ctx
    entries = _hash(hi=LATENCY_MAX)
    assert max(e["len"] for e in entries) == 1025 * 1024
    used = 0
    for e in entries:
        assert validation.file_checksum(files[e["family"], e["len"]], c) == e["digest"], \
            (e["family"], e["len"])
        used += 1
    assert used == len(_hash(hi=LATENCY_MAX)) and used > 150


# ---- K2/K3 ----------------------------------------------------------------------------

@pytest.mark.parametrize("family", FAMILIES)
def test_tree_one_plan_per_family(ctx, device_streams, family):
    """Every hash entry of a family as one checksum_batch_device plan: many
    segments of 1 to 4 (mix) or 5 (mod251) levels, group bases running across
    them."""
    import torch
    from spacedrive_amd import validation
    entries = _hash(family)
    assert len(entries) > 90
    dev = device_streams[family]
    out = validation.checksum_batch_device([dev[:e["len"]] for e in entries], ctx=ctx)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    used = 0
    for i, e in enumerate(entries):
        assert bytes(got[i]).hex() == e["digest"], (family, e["len"])
        used += 1
    assert used == len(entries)


def test_tree_large_entries_alone(ctx, device_streams):
    """The 4095..65537-chunk entries, each as a plan of its own (3, 4 and 5
    levels of 16 nodes per lane)."""
    import torch
    from spacedrive_amd import validation
    entries = [e for e in _hash() if 4095 <= U.chunks_of(e["len"]) <= 65537]
    assert len(entries) == 18 + 9
    used = 0
    for e in entries:
        out = validation.checksum_batch_device([device_streams[e["family"]][:e["len"]]], ctx=ctx)
        torch.cuda.synchronize()
        assert bytes(out[0].cpu().numpy()).hex() == e["digest"], (e["family"], e["len"])
        used += 1
    assert used == len(entries)


def test_checksum_bytes_published_lengths(ctx):
    """The BLAKE3 project's published vector set (input i % 251) through the
    host-buffer call."""
    from spacedrive_amd import validation
    entries = [e for e in _hash("mod251") if e["len"] in U.PUBLISHED]
    assert len(entries) == len(U.PUBLISHED) == 35
    for e in entries:
        assert validation.checksum_bytes(U.data("mod251", e["len"]), ctx).hex() == e["digest"], \
            e["len"]


def test_slice_edge_files(ctx, tmp_path):
    """Files of 65535, 65536 and 65537 chunks (one 64 MiB slice less a chunk,
    exactly one, one and a chunk): the validator job's checksum_files and the
    streaming file_checksum."""
    from spacedrive_amd import validation
    entries = [e for e in _hash() if U.chunks_of(e["len"]) >= 65535]
    assert len(entries) == 9 and {e["family"] for e in entries} == {"mod251"}
    used = 0
    for a in range(0, len(entries), 3):
        part = entries[a:a + 3]
        paths = []
        for e in part:
            p = os.path.join(tmp_path, f"s{e['len']}.bin")
            U.data(e["family"], e["len"]).tofile(p)
            paths.append(p)
        out, st = validation.checksum_files(paths, ctx)
        assert not st.any()
        for i, e in enumerate(part):
            assert bytes(out[i]).hex() == e["digest"], e["len"]
            assert validation.file_checksum(paths[i], ctx) == e["digest"], e["len"]
            os.unlink(paths[i])
            used += 1
    assert used == len(entries)


# ---- subtree and combine -----------------------------------------------------------------

def _pow2_below(n: int) -> int:
    p = 1
    while p * 2 < n:
        p *= 2
    return p


def test_subtree_slices_combine_to_the_digest(ctx, device_streams):
    """Entries of 32..4097 chunks cut into aligned slices -- 16 chunks each, and
    the largest power of two below the chunk count each -- hashed to chaining
    values by subtree_device and folded by combine_subtrees_device; the whole
    as one root slice."""
    import torch
    from spacedrive_amd import validation
    entries = [e for e in _hash() if 32 <= U.chunks_of(e["len"]) <= 4097]
    assert len(entries) > 100
    used = 0
    for e in entries:
        n, dev = e["len"], device_streams[e["family"]]
        chunks = U.chunks_of(n)
        for per in (16, _pow2_below(chunks)):
            k = (chunks + per - 1) // per
            assert k >= 2
            cvs = torch.empty((k, 32), dtype=torch.uint8, device="cuda")
            for i in range(k):
                validation.subtree_device(dev[i * per * 1024:min(n, (i + 1) * per * 1024)],
                                          i * per, False, out=cvs[i], ctx=ctx)
            d = validation.combine_subtrees_device(cvs, ctx=ctx)
            torch.cuda.synchronize()
            assert bytes(d.cpu().numpy()).hex() == e["digest"], (e["family"], n, per)
        d = validation.subtree_device(dev[:n], 0, True, ctx=ctx)
        torch.cuda.synchronize()
        assert bytes(d.cpu().numpy()).hex() == e["digest"], (e["family"], n)
        used += 1
    assert used == len(entries)


# ---- chunk counters at and beyond 2^32 ---------------------------------------------------

def _parent(left: bytes, right: bytes) -> bytes:
    words = struct.unpack("<16I", left + right)
    return struct.pack("<8I", *P.compress(P.IV, words, 0, 64, P.PARENT)[:8])


def _merge(cvs):
    """Root CV of a complete tree over 2^k leaf CVs, left to right pairwise."""
    while len(cvs) > 1:
        cvs = [_parent(cvs[i], cvs[i + 1]) for i in range(0, len(cvs), 2)]
    return cvs[0]


def test_high_chunk_counters(ctx, device_streams):
    """subtree_device on single chunks at counters around 2^32, 2^40 and
    2^64 - 2^32 (the counter's high word reaches the compression), ragged
    chunks of 1 and 1023 bytes included; 16- and 32-chunk aligned slices at the
    same bases equal the parent merge of the recorded leaf CVs."""
    import torch
    from spacedrive_amd import validation
    leaf = U.fixture()["leaf_cv"]
    assert len(leaf) == 2 * (4 * 32 + 2)
    out = torch.empty((len(leaf), 32), dtype=torch.uint8, device="cuda")
    for i, e in enumerate(leaf):
        o = e["input_offset"]
        validation.subtree_device(device_streams[e["family"]][o:o + e["len"]], e["chunk_counter"],
                                  False, out=out[i], ctx=ctx)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    for i, e in enumerate(leaf):
        assert bytes(got[i]).hex() == e["cv"], (e["family"], e["chunk_counter"], e["len"])

    slices = 0
    for fam in FAMILIES:
        full = {e["chunk_counter"]: (e["input_offset"], bytes.fromhex(e["cv"]))
                for e in leaf if e["family"] == fam and e["len"] == 1024}
        bases = sorted(c for c in full if c % 32 == 0)
        assert len(bases) == 4 and bases[-1] == (1 << 64) - (1 << 32)
        for base in bases:
            for first, count in ((0, 16), (16, 16), (0, 32)):
                ctrs = [base + first + j for j in range(count)]
                assert [full[c][0] for c in ctrs] == [(first + j) * 1024 for j in range(count)]
                want = _merge([full[c][1] for c in ctrs])
                part = device_streams[fam][first * 1024:(first + count) * 1024]
                cv = validation.subtree_device(part, base + first, False, ctx=ctx)
                torch.cuda.synchronize()
                assert bytes(cv.cpu().numpy()) == want, (fam, base, first, count)
                slices += 1
    assert slices == 2 * 4 * 3


# ---- the offset contract ----------------------------------------------------------------------

def test_subtree_offset_must_be_aligned(ctx, device_streams):
    """chunk_offset must be a multiple of the slice's chunk count rounded up to
    a power of two (a misaligned slice is a node of no tree): -EINVAL; a slice
    of at most one chunk may sit anywhere."""
    import torch
    from spacedrive_amd import validation
    from spacedrive_amd._native import SdgpuError
    dev = device_streams["mix"]
    for chunks, offset in ((16, 8), (17, 16), (16, 24), (2, 1), (15, 8), (17, 1 << 32 | 16)):
        with pytest.raises(SdgpuError) as ei:
            validation.subtree_device(dev[:chunks * 1024], offset, False, ctx=ctx)
        assert ei.value.errno == 22, (chunks, offset)
    with pytest.raises(SdgpuError):   # 16 chunks and one byte: 17 chunks
        validation.subtree_device(dev[:16 * 1024 + 1], 16, False, ctx=ctx)
    for nbytes, offset in ((16 * 1024, 16), (16 * 1024, 0), (17 * 1024, 32), (15 * 1024 + 1, 16),
                           (1024, 7), (1, 3), (1023, (1 << 64) - 1), (1024, 1 << 32 | 5)):
        validation.subtree_device(dev[:nbytes], offset, False, ctx=ctx)
    torch.cuda.synchronize()
