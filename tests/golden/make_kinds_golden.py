"""Writes tests/golden/kinds.json: the extension table (id, name, kind, second
kind) and the recorded kind cases (file name, size, first bytes as hex, kind in
the identifier's mode, kind in verify mode).

The expected kinds come from the pure-Python oracle (tests/kind_oracle.py, a
step-by-step restatement of crates/file-ext/src/magic.rs).  Before anything is
written, the library's table (sdgpu_kind_ext_name) and its single-file call
(sdgpu_kind_of_file, on real temporary files) are compared with the oracle on
every case; one disagreement and nothing is written.  Needs no GPU.

    python tests/golden/make_kinds_golden.py
"""
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from spacedrive_amd import kind as K  # noqa: E402
from tests import kind_oracle as O  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "kinds.json")


def table_rows():
    """The oracle's variants as the library enumerates them: a name of two
    categories carries its second kind on its first entry."""
    rows = []
    for i, (cat, name, _) in enumerate(O.variants(), start=1):
        both = O.from_str(name)
        second = O.KIND[both[1][0]] if len(both) > 1 and both[0][0] == cat else 0
        rows.append([i, name, O.KIND[cat], second])
    return rows


def main() -> int:
    names = table_rows()
    lib_names = [list(r) for r in K.ext_table()]
    if lib_names != names:
        bad = [(a, b) for a, b in zip(lib_names, names) if a != b][:5]
        print("table mismatch (library, oracle):", bad, len(lib_names), len(names))
        return 1
    cases = []
    wrong = []
    with tempfile.TemporaryDirectory() as d:
        for k, (fname, content) in enumerate(O.cases()):
            sub = os.path.join(d, str(k))
            os.mkdir(sub)
            path = os.path.join(os.fsencode(sub), fname.encode("utf-8"))
            with open(path, "wb") as f:
                f.write(content)
            want = [O.resolve_conflicting(fname, content, always) for always in (False, True)]
            got = [int(K.kind_of_file(path, verify)) for verify in (False, True)]
            if got != want:
                wrong.append((fname, content.hex(), got, want))
            cases.append([fname, len(content), content[:48].hex(), want[0], want[1]])
    if wrong:
        print(f"{len(wrong)} cases disagree (name, bytes, library, oracle):", wrong[:10])
        return 1
    with open(OUT, "w") as f:
        json.dump({"names": names, "cases": cases}, f, separators=(",", ":"))
        f.write("\n")
    print(f"{OUT}: {len(names)} names, {len(cases)} files x 2 modes, {os.path.getsize(OUT)} bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
