"""Pure-Python restatement of sd-file-ext's kind decision, for the tests.

It follows crates/file-ext/src/magic.rs step by step -- Path::extension and
to_str, Extension::from_str over the 15 category enums, magic_bytes_meta,
verify_magic_bytes (seek + read_exact per alternative, then the
any-alternative prefix test of has_magic_bytes) and resolve_conflicting -- and
never the product's flattened rule, so the two restatements differ in form.
The product's table (spacedrive_amd/csrc/kind_table.hpp) is not read here.

Also the deterministic case list the CPU and GPU tests and the fixture
tests/golden/kinds.json share (``cases()``).
"""
from __future__ import annotations

import random

# ObjectKind values (crates/file-ext/src/kind.rs)
KIND = {"Unknown": 0, "Document": 1, "Text": 3, "Image": 5, "Audio": 6, "Video": 7, "Archive": 8,
        "Executable": 9, "Encrypted": 11, "Key": 12, "Font": 18, "Mesh": 19, "Code": 20,
        "Database": 21, "Book": 22, "Config": 23}

# The order of the Extension enum (extensions.rs:11-29): from_str tries the
# categories in this order, so a conflict lists Video before Code.
ENUM_ORDER = ["Document", "Video", "Image", "Audio", "Archive", "Executable", "Text", "Encrypted",
              "Key", "Font", "Mesh", "Code", "Database", "Book", "Config"]

# Categories whose variants verify_magic_bytes is called for under
# always_check_magic_bytes (magic.rs:197-212).
VERIFIED = {"Image", "Audio", "Video", "Archive", "Executable", "Font", "Encrypted", "Mesh",
            "Database"}

# Every variant by its serde name (snake_case; `_3gp` -> 3gp, `_7z` -> 7z), in
# the order the category declares them.  `name=ALT|ALT` gives the variant's
# signature alternatives: hex byte pairs, `__` a wildcard, `+N` the offset; a
# bare `name=` is one empty alternative; a bare `name` has no MagicBytes impl.
_VARIANTS = {
    "Video": (
        "avi=52494646________41564920 qt=71742020 mov=6674797071742020+4 swf=5a5753|465753 mjpeg= "
        "ts=47 mts=47|______47 mpeg=47|000001ba|000001b3 mxf=060e2b34020501010d0102010102 "
        "m2v=000001ba mpg= mpe= m2ts= flv=464c56 wm= 3gp= m4v=667479704d3456+4 "
        "wmv=3026b2758e66cf11a6d900aa0062ce6c asf=3026b2758e66cf11a6d900aa0062ce6c mp4= "
        "webm=1a45dfa3 mkv=1a45dfa3 vob=000001ba ogv=4f676753 wtv=b7d800 hevc= "
        "f4v=6674797066726565+4"),
    "Image": (
        "jpg=ffd8 jpeg=ffd8 png=89504e470d0a1a0a apng=89504e470d0a1a0a0000000d49484452 "
        "gif=47494638__61 bmp=424d tiff=49492a00 webp=52494646________57454250 svg=3c737667 "
        "ico=00000100 heic=000000186674797068656963 heics=000000186674797068656963 heif= heifs= "
        "hif= avif= avci= avcs= raw= akw=414b5742 dng=49492a0008000000444e4700 "
        "cr2=49492a001000000043520200 dcr=49492a001000000044435200 nwr=49492a00100000004e575200 "
        "nef=49492a00080000004e454600 arw=49492a0008 rw2=49492a0018"),
    "Audio": (
        "mp3=494433 mp2=fffb|fffd m4a=667479704d344120+4 wav=52494646________57415645 "
        "aiff=464f524d________41494646 aif=464f524d________41494646 flac=664c6143 ogg=4f676753 "
        "oga=4f676753 opus=4f70757348656164+28 wma=3026b2758e66cf11a6d900aa0062ce6c "
        "amr=2321414d52 aac=fff1 wv=7776706b voc=437265617469766520566f6963652046696c65 "
        "tta=545441 loas=56e0 caf=63616666 aptx=4bbf4bbf adts=fff1 ast=5354524d"),
    "Archive": (
        "zip=504b0304 rar=526172211a0700 tar=7573746172 gz=1f8b08 bz2=425a68 7z=377abcaf271c "
        "xz=fd377a585a00"),
    "Executable": (
        "exe=4d5a app=4d5a apk=504b0304 deb=213c617263683e0a64656269616e2d62696e617279 "
        "dmg=7801730d626260 pkg=4d5a rpm=edabeedb msi=d0cf11e0a1b11ae1 jar=504b0304 bat="),
    "Document": (
        "pdf=255044462d key=504b0304 pages=504b0304 numbers=504b0304 doc=d0cf11e0a1b11ae1 "
        "docx=504b0304 xls=d0cf11e0a1b11ae1 xlsx=504b0304 ppt=d0cf11e0a1b11ae1 pptx=504b0304 "
        "odt=504b0304 ods=504b0304 odp=504b0304 ics=424547494e3a5643415244 hwp=d0cf11e0a1b11ae1"),
    "Text": (
        "txt rtf md markdown"),
    "Config": (
        "ini json yaml yml toml xml mathml rss csv cfg compose tsconfig"),
    "Encrypted": (
        "bytes=62616c6c617070 container=7364626f78 block=7364626c6f636b"),
    "Key": (
        "pgp pub pem p12 p8 keychain"),
    "Font": (
        "ttf=0001000000 otf=4f54544f00 woff=774f4646 woff2=774f4632"),
    "Mesh": (
        "fbx=46425820 obj=6f626a"),
    "Code": (
        "scpt scptd applescript sh zsh fish bash c cpp h hpp rb js mjs jsx html css sass scss "
        "less cr cs csx d dart dockerfile go hs java kt kts lua make nim nims m mm ml mli mll mly "
        "pl php php1 php2 php3 php4 php5 php6 phps phpt phtml ps1 psd1 psm1 py qml r rs sol sql "
        "swift ts tsx vala zig vue scala mdx astro mts"),
    "Database": (
        "sqlite=53514c69746520666f726d6174203300 db="),
    "Book": (
        "azw=52494646 azw3=52494646 epub=504b0304 mobi=4d4f4249"),
}


def _parse(tok: str):
    if "=" not in tok:
        return tok, None
    name, sig = tok.split("=", 1)
    alts = []
    for a in sig.split("|"):
        hexs, _, off = a.partition("+")
        pat = [None if hexs[i:i + 2] == "__" else int(hexs[i:i + 2], 16)
               for i in range(0, len(hexs), 2)]
        alts.append((pat, int(off) if off else 0))
    return name, alts


# category -> [(name, alternatives or None)]
TABLE = {cat: [_parse(t) for t in toks.split()] for cat, toks in _VARIANTS.items()}
assert sorted(TABLE) == sorted(ENUM_ORDER)


def variants():
    """[(category, name, alternatives)] in enum order, then declaration order."""
    return [(cat, name, alts) for cat in ENUM_ORDER for name, alts in TABLE[cat]]


def alternatives_of(cat: str, name: str):
    for n, alts in TABLE[cat]:
        if n == name:
            return alts
    raise KeyError((cat, name))


# ---- Path::extension().and_then(OsStr::to_str) ------------------------------------

def extension_of(path) -> str | None:
    """path: str, or bytes for names that are not UTF-8."""
    raw = path if isinstance(path, bytes) else path.encode("utf-8", "surrogateescape")
    comps = [c for c in raw.split(b"/") if c not in (b"", b".")]
    if not comps or comps[-1] == b"..":
        return None                       # file_name() is None
    name = comps[-1]
    before, dot, after = name.rpartition(b".")
    if not dot or not before:
        return None                       # no '.', or the only one leads the name
    try:
        return after.decode("utf-8")      # to_str: None when not UTF-8
    except UnicodeDecodeError:
        return None


# ---- Extension::from_str (magic.rs:63-79) -----------------------------------------

def from_str(s: str):
    """[] (None), one (category, name) (Known) or several (Conflicts)."""
    s = s.lower()
    return [(cat, name) for cat in ENUM_ORDER for name, _ in TABLE[cat] if name == s]


# ---- MagicBytes (magic.rs:135-155) --------------------------------------------------

def magic_bytes_meta(cat: str, name: str):
    return [(off, len(pat)) for pat, off in alternatives_of(cat, name)]


def has_magic_bytes(cat: str, name: str, buf: bytes) -> bool:
    """match (self, buf) { (Variant, &[b0, b1, .., ..]) => true, .. }: any
    alternative is a prefix of buf, whatever its offset."""
    for pat, _ in alternatives_of(cat, name):
        if len(buf) >= len(pat) and all(p is None or p == buf[j] for j, p in enumerate(pat)):
            return True
    return False


def verify_magic_bytes(cat: str, name: str, content: bytes) -> bool:
    """magic.rs:160-173; False stands for None."""
    for off, length in magic_bytes_meta(cat, name):
        buf = content[off:off + length]   # seek (never fails on a file) + read_exact
        if len(buf) < length:
            return False                  # read_exact: UnexpectedEof -> `.ok()?`
        if has_magic_bytes(cat, name, buf):
            return True
    return False


# ---- Extension::resolve_conflicting (magic.rs:176-236) ------------------------------

def resolve_known(cat: str, name: str, content: bytes, always: bool) -> int:
    """The Known(e) arm, for one variant."""
    if always and cat in VERIFIED:
        return KIND[cat] if verify_magic_bytes(cat, name, content) else 0
    return KIND[cat]


def resolve_conflicting(path, content: bytes | None, always: bool = False) -> int:
    """ObjectKind value; content None = File::open fails."""
    ext_str = extension_of(path)
    if ext_str is None:
        return 0
    ext = from_str(ext_str)
    if not ext:
        return 0
    if content is None:
        return 0
    if len(ext) == 1:
        return resolve_known(ext[0][0], ext[0][1], content, always)
    # the match is on ext_str as it stands in the path, not lower-cased
    if ext_str in ("ts", "mts") and any(c == "Video" for c, _ in ext):
        return KIND["Video"] if verify_magic_bytes("Video", ext_str, content) else KIND["Code"]
    return 0


# ---- the shared case list ---------------------------------------------------------------

def cases(seed: int = 20240) -> list[tuple[str, bytes]]:
    """(file name, content) pairs, deterministic: for every non-empty
    alternative of every variant a file exactly offset + length bytes long that
    matches (wildcards and the bytes before the offset random), the same one
    byte shorter, one byte longer and padded to 48 bytes, and one with each
    fixed byte flipped in turn; every empty alternative on an empty file and
    on a one-byte file; the `ts` / `mts` shapes; names without an Extension."""
    rng = random.Random(seed)
    out: list[tuple[str, bytes]] = []
    for cat, name, alts in variants():
        fname = "f." + name
        if alts is None:
            out.append((fname, b""))
            out.append((fname, rng.randbytes(9)))
            continue
        if all(pat for pat, _ in alts):
            out.append((fname, b""))      # no alternative can match an empty file
        for pat, off in alts:
            if not pat:
                out.append((fname, b""))
                out.append((fname, rng.randbytes(1)))
                continue
            good = bytearray(rng.randbytes(off))
            good += bytes(rng.randrange(256) if p is None else p for p in pat)
            good = bytes(good)
            out.append((fname, good))
            out.append((fname, good[:-1]))
            out.append((fname, good + rng.randbytes(1)))
            out.append((fname, good + rng.randbytes(48 - len(good))))
            for j, p in enumerate(pat):
                if p is None:
                    continue
                bad = bytearray(good)
                bad[off + j] ^= 1 << rng.randrange(8)
                out.append((fname, bytes(bad)))
    for n in ("x.ts", "x.mts", "X.TS", "x.Mts"):
        for body in (b"", b"\x47", b"\x00\x01\x02\x47", b"\x47\x00\x00\x00", b"\x00\x01\x02",
                     b"\x46" + bytes(39)):
            out.append((n, body))
    for n in ("a", ".bashrc", ".x.rs", "a.", "A.JPG", "a.tar.GZ", "a.\u212at", "a.\u212a",
              "a.jeff", "a.jpg.bak", "a.JpEg", "a.m\u212av", "a.\u0130ni"):
        out.append((n, b""))
        out.append((n, b"\xff\xd8\xff\xe0" + bytes(12)))
    return out
