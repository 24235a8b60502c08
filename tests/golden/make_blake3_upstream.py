"""Generates tests/golden/blake3_upstream.json (run from the repo root:
`python tests/golden/make_blake3_upstream.py [LIBRARY]`; `--check` regenerates
in memory, compares with the committed file and exits non-zero on a difference).

Every digest and chaining value in the fixture is computed by the BLAKE3
project's official C implementation as LLVM vendors it: a shared library of the
ROCm toolchain's LLVM (lib/llvm/lib/libclang-cpp.so, or the library given on
the command line) exports llvm_blake3_hasher_{init,update,finalize} and
llvm_blake3_compress_subtree_wide.  That code is neither the reference project
nor this repository's, so the fixture pins what oracle/sd_oracle.c and
oracle/blake3_py.py only agree on between themselves: parent nodes, ROOT on a
parent, the left-subtree power-of-two rule and chunk counters other than 0.

The oracle is imported for one thing only: building the message of a sampled
file (O.cas_build_message, cas.rs:23-62); the upstream library hashes it.

Exit status: 0 written / identical, 1 the fixture differs, 3 no library with
the symbol was found.
"""
from __future__ import annotations

import ctypes
import glob
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

OUT = os.path.join(ROOT, "tests", "golden", "blake3_upstream.json")

IV = (0x6A09E667, 0xBB67AE85, 0x3C6EF372, 0xA54FF53A,
      0x510E527F, 0x9B05688C, 0x1F83D9AB, 0x5BE0CD19)

# the input lengths of the BLAKE3 project's published test_vectors.json
PUBLISHED = [0, 1, 2, 3, 4, 5, 6, 7, 8, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 2048, 2049,
             3072, 3073, 4096, 4097, 5120, 5121, 6144, 6145, 7168, 7169, 8192, 8193, 16384, 31744,
             102400]
# chunk counts where this project's paths change: K1's four-chunk units and its
# 102 408-B limit (100, 101), the 112 KiB limit of k_small_host / k_service
# (111-113), the 64 KiB groups and 1 MiB limit of k_small_split (63-65,
# 127-129, 1023-1025), the 16-nodes-per-lane levels of K2/K3 (16, 256, 4096,
# 65536 and their neighbours), the 64 MiB slices of the streaming file_checksum
EDGE_CHUNKS = [2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 100, 101, 111, 112, 113,
               127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 65535, 65536,
               65537]
SLICE_EDGE_CHUNKS = (65535, 65536, 65537)       # the three 64 MiB sizes: mod251 only
WHOLE_READ_MAX = 102400                         # cas.rs:15 MINIMUM_FILE_SIZE
SAMPLED_SIZES = [102401, 500000, 3 * (1 << 20) + 5]
COUNTER_BASES = [(1 << 32) - 32, 1 << 32, (1 << 40) + (1 << 32), (1 << 64) - (1 << 32)]
LEAF_CHUNKS = 32
RAGGED_BASE = 1 << 32
RAGGED_LENS = (1, 1023)

KNOWN = {  # asserted before anything is written
    0: "af1349b9f5f9a1a6a0404dea36dcc9499bcb25c9adc112b7cc9a93cae41f3262",
    1025: "d00278ae47eb27b34faecf67b4fe263f82d5412916c1ffd97c8cb7fb814b8444",
    102400: "bc3e3d41a1146b069abffad3c0d44860cf664390afce4d9661f7902e7943e085",
}

INPUTS = {
    "mod251": "byte[i] = i % 251",
    "mix": ("x = (i * 2654435761) mod 2^32; x = x xor (x >> 15); x = (x * 2246822519) mod 2^32; "
            "x = x xor (x >> 13); byte[i] = x mod 256   (i < 2^32, unsigned 32-bit arithmetic)"),
}


def family_bytes(family: str, n: int) -> np.ndarray:
    """The first n bytes of an input family (uint8 array), from its formula."""
    if family == "mod251":  # the period repeated: the 64 MiB sizes without a 64-bit index array
        return np.resize(np.arange(251, dtype=np.uint8), n)
    i = np.arange(n, dtype=np.uint64)
    if family == "mix":
        m = np.uint64(0xFFFFFFFF)
        x = (i * np.uint64(2654435761)) & m
        x ^= x >> np.uint64(15)
        x = (x * np.uint64(2246822519)) & m
        x ^= x >> np.uint64(13)
        return (x & np.uint64(0xFF)).astype(np.uint8)
    raise KeyError(family)


def edge_lengths(chunks) -> list[int]:
    return sorted({n for c in chunks for n in (c * 1024 - 1023, c * 1024 - 1, c * 1024)})


def hash_lengths(family: str) -> list[int]:
    if family == "mod251":
        return sorted(set(PUBLISHED) | set(edge_lengths(EDGE_CHUNKS)))
    rest = [c for c in EDGE_CHUNKS if c not in SLICE_EDGE_CHUNKS]
    return sorted({0, 1, 64, 1024} | set(edge_lengths(rest)))


# ---- the upstream library ----------------------------------------------------

def _candidates() -> list[str]:
    dirs = []
    for root in (os.environ.get("ROCM_PATH"), "/opt/rocm"):
        if root:
            d = os.path.join(root, "lib", "llvm", "lib")
            if d not in dirs:
                dirs.append(d)
    out = []
    for d in dirs:
        for pat in ("libclang-cpp.so*", "libLLVM*.so*"):
            out += sorted(glob.glob(os.path.join(d, pat)))
    return out


def find_library(path: str | None = None):
    """(CDLL, path) of a shared library exporting llvm_blake3_hasher_init, or None."""
    for p in ([path] if path else _candidates()):
        try:
            lib = ctypes.CDLL(p)
        except OSError:
            continue
        if hasattr(lib, "llvm_blake3_hasher_init"):
            return lib, p
    return None


class Upstream:
    def __init__(self, lib, path: str):
        self.lib, self.path = lib, path
        vp, sz = ctypes.c_void_p, ctypes.c_size_t
        lib.llvm_blake3_version.restype = ctypes.c_char_p
        lib.llvm_blake3_hasher_init.argtypes = [vp]
        lib.llvm_blake3_hasher_init.restype = None
        lib.llvm_blake3_hasher_update.argtypes = [vp, vp, sz]
        lib.llvm_blake3_hasher_update.restype = None
        lib.llvm_blake3_hasher_finalize.argtypes = [vp, vp, sz]
        lib.llvm_blake3_hasher_finalize.restype = None
        # (input, input_len, key[8], chunk_counter, flags, out); releases from
        # 1.8 on take a trailing `bool use_tbb`, passed as 0 (an extra integer
        # argument is harmless to the older six-argument form)
        lib.llvm_blake3_compress_subtree_wide.argtypes = [vp, sz, vp, ctypes.c_uint64,
                                                          ctypes.c_uint8, vp, ctypes.c_int]
        lib.llvm_blake3_compress_subtree_wide.restype = sz
        self.version = lib.llvm_blake3_version().decode()
        self._iv = (ctypes.c_uint32 * 8)(*IV)

    def hash(self, data: np.ndarray) -> str:
        data = np.ascontiguousarray(data, np.uint8)
        st = ctypes.create_string_buffer(4096)   # blake3_hasher is 1912 bytes
        out = ctypes.create_string_buffer(32)
        self.lib.llvm_blake3_hasher_init(st)
        if data.size:
            self.lib.llvm_blake3_hasher_update(st, data.ctypes.data, data.size)
        self.lib.llvm_blake3_hasher_finalize(st, out, 32)
        return out.raw.hex()

    def leaf_cvs(self, data: np.ndarray, counter: int) -> list[str]:
        """Chaining values of the 1 or 2 chunks of `data` (key IV, flags 0), the
        first at chunk counter `counter`: one CV per chunk."""
        data = np.ascontiguousarray(data, np.uint8)
        assert 0 < data.size <= 2048
        out = ctypes.create_string_buffer(64 * 32)
        k = self.lib.llvm_blake3_compress_subtree_wide(data.ctypes.data, data.size, self._iv,
                                                       counter, 0, out, 0)
        assert k == (data.size + 1023) // 1024, (k, data.size)
        return [out.raw[32 * j:32 * j + 32].hex() for j in range(k)]


# ---- the fixture ---------------------------------------------------------------

def generate(up: Upstream) -> dict:
    from oracle import oracle as O  # message building of sampled files only

    pat = family_bytes("mod251", 102400)
    for n, want in KNOWN.items():
        got = up.hash(pat[:n])
        assert got == want, ("the upstream library fails a published vector", n, got)

    fix = {
        "source": {"library": os.path.basename(up.path), "blake3_version": up.version,
                   "entry_points": "llvm_blake3_hasher_init/update/finalize, "
                                   "llvm_blake3_compress_subtree_wide (key = IV, flags = 0)"},
        "inputs": INPUTS,
        "hash": [], "cas": [], "leaf_cv": [],
    }
    for fam in INPUTS:
        lens = hash_lengths(fam)
        buf = family_bytes(fam, max(lens + SAMPLED_SIZES))
        for n in lens:
            fix["hash"].append({"family": fam, "len": n, "digest": up.hash(buf[:n])})
        for n in [n for n in lens if n <= WHOLE_READ_MAX]:
            msg = np.concatenate([np.frombuffer(n.to_bytes(8, "little"), np.uint8), buf[:n]])
            fix["cas"].append({"family": fam, "size": n, "digest": up.hash(msg)})
        for n in SAMPLED_SIZES:
            msg = O.cas_build_message(buf[:n])
            assert msg is not None and len(msg) == 57352
            fix["cas"].append({"family": fam, "size": n,
                               "digest": up.hash(np.frombuffer(msg, np.uint8))})
        for base in COUNTER_BASES:
            for j in range(0, LEAF_CHUNKS, 2):
                two = up.leaf_cvs(buf[j * 1024:(j + 2) * 1024], base + j)
                # the same chunks one per call: the counter is an argument, not
                # something the library advanced
                assert two == [up.leaf_cvs(buf[(j + k) * 1024:(j + k + 1) * 1024], base + j + k)[0]
                               for k in range(2)]
                for k in range(2):
                    fix["leaf_cv"].append({"family": fam, "input_offset": (j + k) * 1024,
                                           "len": 1024, "chunk_counter": base + j + k,
                                           "cv": two[k]})
        for n in RAGGED_LENS:
            o = LEAF_CHUNKS * 1024
            fix["leaf_cv"].append({"family": fam, "input_offset": o, "len": n,
                                   "chunk_counter": RAGGED_BASE + LEAF_CHUNKS,
                                   "cv": up.leaf_cvs(buf[o:o + n], RAGGED_BASE + LEAF_CHUNKS)[0]})
    # the counter matters: the same chunk at base 2^32 - 32 + j and at j differs
    low = up.leaf_cvs(family_bytes("mod251", 2048), 0)
    assert low != [e["cv"] for e in fix["leaf_cv"][:2]]
    return fix


def dumps(fix: dict) -> str:
    """JSON with one list entry per line (a reviewable diff, a small file)."""
    c = lambda v: json.dumps(v, separators=(",", ":"))  # noqa: E731
    parts = []
    for k, v in fix.items():
        if isinstance(v, list):
            parts.append(f' {c(k)}: [\n' + ",\n".join("  " + c(e) for e in v) + "\n ]")
        else:
            parts.append(f" {c(k)}: {json.dumps(v, indent=2).replace(chr(10), chr(10) + ' ')}")
    return "{\n" + ",\n".join(parts) + "\n}\n"


def main(argv) -> int:
    args = [a for a in argv if a != "--check"]
    found = find_library(args[0] if args else None)
    if found is None:
        print("no shared library exporting llvm_blake3_hasher_init was found", file=sys.stderr)
        return 3
    up = Upstream(*found)
    text = dumps(generate(up))
    assert json.loads(text)  # well-formed
    if "--check" in argv:
        with open(OUT) as f:
            have = f.read()
        # `source` names the library the committed file was made with; another
        # release of the toolchain is not a difference in the vectors
        a, b = json.loads(have), json.loads(text)
        bad = [part for part in sorted(set(a) | set(b))
               if part != "source" and a.get(part) != b.get(part)]
        if bad:
            print(f"blake3_upstream.json differs from {up.path} in {bad}", file=sys.stderr)
            return 1
        if have != text and a["source"] == b["source"]:
            print("blake3_upstream.json differs in formatting", file=sys.stderr)
            return 1
        print(f"blake3_upstream.json matches {os.path.basename(up.path)} "
              f"(BLAKE3 {up.version})")
        return 0
    with open(OUT, "w") as f:
        f.write(text)
    print(f"wrote {OUT} ({len(text)} bytes) from {up.path} (BLAKE3 {up.version})")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
