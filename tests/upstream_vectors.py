"""Access to tests/golden/blake3_upstream.json for the CPU and GPU tests: the
fixture, and the two input families rebuilt from the formulas it states.  No
test reads the upstream library through this module; only the generator
(tests/golden/make_blake3_upstream.py) and its --check child process do."""
from __future__ import annotations

import functools
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "blake3_upstream.json")
GENERATOR = os.path.join(HERE, "golden", "make_blake3_upstream.py")

CHUNK = 1024
WHOLE_READ_MAX = 102400   # cas.rs:15: files up to here are read whole
PUBLISHED = [0, 1, 2, 3, 4, 5, 6, 7, 8, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 2048, 2049,
             3072, 3073, 4096, 4097, 5120, 5121, 6144, 6145, 7168, 7169, 8192, 8193, 16384, 31744,
             102400]


@functools.lru_cache(maxsize=None)
def fixture() -> dict:
    with open(FIXTURE) as f:
        fix = json.load(f)
    assert set(fix["inputs"]) == {"mod251", "mix"}
    # the formulas below are the ones the fixture states
    assert fix["inputs"]["mod251"] == "byte[i] = i % 251"
    assert fix["inputs"]["mix"].startswith(
        "x = (i * 2654435761) mod 2^32; x = x xor (x >> 15); x = (x * 2246822519) mod 2^32; "
        "x = x xor (x >> 13); byte[i] = x mod 256")
    return fix


def _formula(family: str, n: int) -> np.ndarray:
    if family == "mod251":
        return np.resize(np.arange(251, dtype=np.uint8), n)
    i = np.arange(n, dtype=np.uint64)
    m = np.uint64(0xFFFFFFFF)
    x = (i * np.uint64(2654435761)) & m
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(2246822519)) & m
    x ^= x >> np.uint64(13)
    return (x & np.uint64(0xFF)).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _family(family: str) -> np.ndarray:
    fix = fixture()
    need = [e["len"] for e in fix["hash"] if e["family"] == family]
    need += [e["size"] for e in fix["cas"] if e["family"] == family]
    need += [e["input_offset"] + e["len"] for e in fix["leaf_cv"] if e["family"] == family]
    buf = _formula(family, max(need))
    buf.setflags(write=False)
    return buf


def data(family: str, n: int, offset: int = 0) -> np.ndarray:
    """Bytes [offset, offset + n) of an input family (read-only view)."""
    return _family(family)[offset:offset + n]


def chunks_of(n: int) -> int:
    """Chunks of an n-byte message (the empty message is one empty chunk)."""
    return max(1, (n + CHUNK - 1) // CHUNK)
