// Object kind of a file from its name and first bytes: the extension table of
// sd-file-ext (crates/file-ext/src/extensions.rs:11-362), the magic-byte test
// (magic.rs:160-173) and Extension::resolve_conflicting (magic.rs:176-236), as
// ONE table and ONE decision function compiled for the host and for gfx950.
// The kernel (kind.hip), the single-file call, the empty files and the grown-
// file path of the identifier all go through kind_decide() below.
//
// Plain C++17, no HIP types: it also compiles in a host-only program.
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define KIND_HD __host__ __device__
#else
#define KIND_HD
#endif

namespace sdgpu {
namespace kind {

// ObjectKind values (crates/file-ext/src/kind.rs) of the 15 extension categories.
enum : uint8_t {
  kUnknown = 0, kDocument = 1, kText = 3, kImage = 5, kAudio = 6, kVideo = 7, kArchive = 8,
  kExecutable = 9, kEncrypted = 11, kKey = 12, kFont = 18, kMesh = 19, kCode = 20,
  kDatabase = 21, kBook = 22, kConfig = 23,
};

// One extension name.  sig: the variant's signature alternatives separated by
// '|', each a run of hex byte pairs with "__" for a byte that may be anything,
// optionally followed by "+N" (the alternative sits at file offset N); ""
// is one empty alternative (matches every file), nullptr a variant without a
// magic-byte test (the categories that are never verified).  kind2: the second
// category of the two names that have one (the first one's signature decides).
struct Src {
  const char* name;
  uint8_t kind, kind2;
  const char* sig;
};

// One entry per variant of the reference's 15 category enums (215 of them, 213
// distinct names).  Ids are positions in this list + 1 and are stable: new
// names go at the end.  Order: the categories as extensions.rs's Extension
// enum lists them, the variants as each category lists them.  `ts` and `mts`
// are variants of Video and of Code: a path resolves to the FIRST entry of its
// name (the Video one, which carries both kinds and the signature that
// decides between them); the Code entries stand for CodeExtension::Ts / Mts
// themselves and are always Code.
inline constexpr Src kSrc[] = {
    // Document (never verified; the signatures are recorded all the same)
    {"pdf", kDocument, 0, "255044462d"},
    {"key", kDocument, 0, "504b0304"},
    {"pages", kDocument, 0, "504b0304"},
    {"numbers", kDocument, 0, "504b0304"},
    {"doc", kDocument, 0, "d0cf11e0a1b11ae1"},
    {"docx", kDocument, 0, "504b0304"},
    {"xls", kDocument, 0, "d0cf11e0a1b11ae1"},
    {"xlsx", kDocument, 0, "504b0304"},
    {"ppt", kDocument, 0, "d0cf11e0a1b11ae1"},
    {"pptx", kDocument, 0, "504b0304"},
    {"odt", kDocument, 0, "504b0304"},
    {"ods", kDocument, 0, "504b0304"},
    {"odp", kDocument, 0, "504b0304"},
    {"ics", kDocument, 0, "424547494e3a5643415244"},
    {"hwp", kDocument, 0, "d0cf11e0a1b11ae1"},
    // Video
    {"avi", kVideo, 0, "52494646________41564920"},
    {"qt", kVideo, 0, "71742020"},
    {"mov", kVideo, 0, "6674797071742020+4"},
    {"swf", kVideo, 0, "5a5753|465753"},
    {"mjpeg", kVideo, 0, ""},
    {"ts", kVideo, kCode, "47"},
    {"mts", kVideo, kCode, "47|______47"},
    {"mpeg", kVideo, 0, "47|000001ba|000001b3"},
    {"mxf", kVideo, 0, "060e2b34020501010d0102010102"},
    {"m2v", kVideo, 0, "000001ba"},
    {"mpg", kVideo, 0, ""},
    {"mpe", kVideo, 0, ""},
    {"m2ts", kVideo, 0, ""},
    {"flv", kVideo, 0, "464c56"},
    {"wm", kVideo, 0, ""},
    {"3gp", kVideo, 0, ""},
    {"m4v", kVideo, 0, "667479704d3456+4"},
    {"wmv", kVideo, 0, "3026b2758e66cf11a6d900aa0062ce6c"},
    {"asf", kVideo, 0, "3026b2758e66cf11a6d900aa0062ce6c"},
    {"mp4", kVideo, 0, ""},
    {"webm", kVideo, 0, "1a45dfa3"},
    {"mkv", kVideo, 0, "1a45dfa3"},
    {"vob", kVideo, 0, "000001ba"},
    {"ogv", kVideo, 0, "4f676753"},
    {"wtv", kVideo, 0, "b7d800"},
    {"hevc", kVideo, 0, ""},
    {"f4v", kVideo, 0, "6674797066726565+4"},
    // Image
    {"jpg", kImage, 0, "ffd8"},
    {"jpeg", kImage, 0, "ffd8"},
    {"png", kImage, 0, "89504e470d0a1a0a"},
    {"apng", kImage, 0, "89504e470d0a1a0a0000000d49484452"},
    {"gif", kImage, 0, "47494638__61"},
    {"bmp", kImage, 0, "424d"},
    {"tiff", kImage, 0, "49492a00"},
    {"webp", kImage, 0, "52494646________57454250"},
    {"svg", kImage, 0, "3c737667"},
    {"ico", kImage, 0, "00000100"},
    {"heic", kImage, 0, "000000186674797068656963"},
    {"heics", kImage, 0, "000000186674797068656963"},
    {"heif", kImage, 0, ""},
    {"heifs", kImage, 0, ""},
    {"hif", kImage, 0, ""},
    {"avif", kImage, 0, ""},
    {"avci", kImage, 0, ""},
    {"avcs", kImage, 0, ""},
    {"raw", kImage, 0, ""},
    {"akw", kImage, 0, "414b5742"},
    {"dng", kImage, 0, "49492a0008000000444e4700"},
    {"cr2", kImage, 0, "49492a001000000043520200"},
    {"dcr", kImage, 0, "49492a001000000044435200"},
    {"nwr", kImage, 0, "49492a00100000004e575200"},
    {"nef", kImage, 0, "49492a00080000004e454600"},
    {"arw", kImage, 0, "49492a0008"},
    {"rw2", kImage, 0, "49492a0018"},
    // Audio
    {"mp3", kAudio, 0, "494433"},
    {"mp2", kAudio, 0, "fffb|fffd"},
    {"m4a", kAudio, 0, "667479704d344120+4"},
    {"wav", kAudio, 0, "52494646________57415645"},
    {"aiff", kAudio, 0, "464f524d________41494646"},
    {"aif", kAudio, 0, "464f524d________41494646"},
    {"flac", kAudio, 0, "664c6143"},
    {"ogg", kAudio, 0, "4f676753"},
    {"oga", kAudio, 0, "4f676753"},
    {"opus", kAudio, 0, "4f70757348656164+28"},
    {"wma", kAudio, 0, "3026b2758e66cf11a6d900aa0062ce6c"},
    {"amr", kAudio, 0, "2321414d52"},
    {"aac", kAudio, 0, "fff1"},
    {"wv", kAudio, 0, "7776706b"},
    {"voc", kAudio, 0, "437265617469766520566f6963652046696c65"},
    {"tta", kAudio, 0, "545441"},
    {"loas", kAudio, 0, "56e0"},
    {"caf", kAudio, 0, "63616666"},
    {"aptx", kAudio, 0, "4bbf4bbf"},
    {"adts", kAudio, 0, "fff1"},
    {"ast", kAudio, 0, "5354524d"},
    // Archive
    {"zip", kArchive, 0, "504b0304"},
    {"rar", kArchive, 0, "526172211a0700"},
    {"tar", kArchive, 0, "7573746172"},
    {"gz", kArchive, 0, "1f8b08"},
    {"bz2", kArchive, 0, "425a68"},
    {"7z", kArchive, 0, "377abcaf271c"},
    {"xz", kArchive, 0, "fd377a585a00"},
    // Executable
    {"exe", kExecutable, 0, "4d5a"},
    {"app", kExecutable, 0, "4d5a"},
    {"apk", kExecutable, 0, "504b0304"},
    {"deb", kExecutable, 0, "213c617263683e0a64656269616e2d62696e617279"},
    {"dmg", kExecutable, 0, "7801730d626260"},
    {"pkg", kExecutable, 0, "4d5a"},
    {"rpm", kExecutable, 0, "edabeedb"},
    {"msi", kExecutable, 0, "d0cf11e0a1b11ae1"},
    {"jar", kExecutable, 0, "504b0304"},
    {"bat", kExecutable, 0, ""},
    // Text
    {"txt", kText, 0, nullptr},
    {"rtf", kText, 0, nullptr},
    {"md", kText, 0, nullptr},
    {"markdown", kText, 0, nullptr},
    // Encrypted
    {"bytes", kEncrypted, 0, "62616c6c617070"},
    {"container", kEncrypted, 0, "7364626f78"},
    {"block", kEncrypted, 0, "7364626c6f636b"},
    // Key
    {"pgp", kKey, 0, nullptr},
    {"pub", kKey, 0, nullptr},
    {"pem", kKey, 0, nullptr},
    {"p12", kKey, 0, nullptr},
    {"p8", kKey, 0, nullptr},
    {"keychain", kKey, 0, nullptr},
    // Font
    {"ttf", kFont, 0, "0001000000"},
    {"otf", kFont, 0, "4f54544f00"},
    {"woff", kFont, 0, "774f4646"},
    {"woff2", kFont, 0, "774f4632"},
    // Mesh
    {"fbx", kMesh, 0, "46425820"},
    {"obj", kMesh, 0, "6f626a"},
    // Code (its `ts` and `mts` variants are never what a path resolves to: see above)
    {"scpt", kCode, 0, nullptr},
    {"scptd", kCode, 0, nullptr},
    {"applescript", kCode, 0, nullptr},
    {"sh", kCode, 0, nullptr},
    {"zsh", kCode, 0, nullptr},
    {"fish", kCode, 0, nullptr},
    {"bash", kCode, 0, nullptr},
    {"c", kCode, 0, nullptr},
    {"cpp", kCode, 0, nullptr},
    {"h", kCode, 0, nullptr},
    {"hpp", kCode, 0, nullptr},
    {"rb", kCode, 0, nullptr},
    {"js", kCode, 0, nullptr},
    {"mjs", kCode, 0, nullptr},
    {"jsx", kCode, 0, nullptr},
    {"html", kCode, 0, nullptr},
    {"css", kCode, 0, nullptr},
    {"sass", kCode, 0, nullptr},
    {"scss", kCode, 0, nullptr},
    {"less", kCode, 0, nullptr},
    {"cr", kCode, 0, nullptr},
    {"cs", kCode, 0, nullptr},
    {"csx", kCode, 0, nullptr},
    {"d", kCode, 0, nullptr},
    {"dart", kCode, 0, nullptr},
    {"dockerfile", kCode, 0, nullptr},
    {"go", kCode, 0, nullptr},
    {"hs", kCode, 0, nullptr},
    {"java", kCode, 0, nullptr},
    {"kt", kCode, 0, nullptr},
    {"kts", kCode, 0, nullptr},
    {"lua", kCode, 0, nullptr},
    {"make", kCode, 0, nullptr},
    {"nim", kCode, 0, nullptr},
    {"nims", kCode, 0, nullptr},
    {"m", kCode, 0, nullptr},
    {"mm", kCode, 0, nullptr},
    {"ml", kCode, 0, nullptr},
    {"mli", kCode, 0, nullptr},
    {"mll", kCode, 0, nullptr},
    {"mly", kCode, 0, nullptr},
    {"pl", kCode, 0, nullptr},
    {"php", kCode, 0, nullptr},
    {"php1", kCode, 0, nullptr},
    {"php2", kCode, 0, nullptr},
    {"php3", kCode, 0, nullptr},
    {"php4", kCode, 0, nullptr},
    {"php5", kCode, 0, nullptr},
    {"php6", kCode, 0, nullptr},
    {"phps", kCode, 0, nullptr},
    {"phpt", kCode, 0, nullptr},
    {"phtml", kCode, 0, nullptr},
    {"ps1", kCode, 0, nullptr},
    {"psd1", kCode, 0, nullptr},
    {"psm1", kCode, 0, nullptr},
    {"py", kCode, 0, nullptr},
    {"qml", kCode, 0, nullptr},
    {"r", kCode, 0, nullptr},
    {"rs", kCode, 0, nullptr},
    {"sol", kCode, 0, nullptr},
    {"sql", kCode, 0, nullptr},
    {"swift", kCode, 0, nullptr},
    {"ts", kCode, 0, nullptr},
    {"tsx", kCode, 0, nullptr},
    {"vala", kCode, 0, nullptr},
    {"zig", kCode, 0, nullptr},
    {"vue", kCode, 0, nullptr},
    {"scala", kCode, 0, nullptr},
    {"mdx", kCode, 0, nullptr},
    {"astro", kCode, 0, nullptr},
    {"mts", kCode, 0, nullptr},
    // Database
    {"sqlite", kDatabase, 0, "53514c69746520666f726d6174203300"},
    {"db", kDatabase, 0, ""},
    // Book (never verified)
    {"azw", kBook, 0, "52494646"},
    {"azw3", kBook, 0, "52494646"},
    {"epub", kBook, 0, "504b0304"},
    {"mobi", kBook, 0, "4d4f4249"},
    // Config
    {"ini", kConfig, 0, nullptr},
    {"json", kConfig, 0, nullptr},
    {"yaml", kConfig, 0, nullptr},
    {"yml", kConfig, 0, nullptr},
    {"toml", kConfig, 0, nullptr},
    {"xml", kConfig, 0, nullptr},
    {"mathml", kConfig, 0, nullptr},
    {"rss", kConfig, 0, nullptr},
    {"csv", kConfig, 0, nullptr},
    {"cfg", kConfig, 0, nullptr},
    {"compose", kConfig, 0, nullptr},
    {"tsconfig", kConfig, 0, nullptr},
};

constexpr uint32_t kExts = sizeof(kSrc) / sizeof(kSrc[0]);  // ids 1..kExts
constexpr uint32_t kAlts = 127;      // signature alternatives over all names
constexpr uint32_t kMaxSigs = 80;    // distinct alternatives (79 today)
constexpr uint32_t kBodyBytes = 40;  // file bytes the test may look at (the farthest ends at 36)
constexpr uint32_t kWords = kBodyBytes / 4;
constexpr uint32_t kNameMax = 15;    // longest name the table could hold (+ NUL = 16)

// One distinct alternative over the file's first kBodyBytes bytes, as little-
// endian words: it matches a file of L bytes when L >= need (= offset + length)
// and (word[w] & mask[w]) == val[w] for every w.  Wildcards and the bytes
// outside the alternative have mask 0; the empty alternative has need 0.
struct Sig {
  uint32_t val[kWords], mask[kWords];
  uint32_t need;
};
struct Ext {
  uint8_t kind, kind2, first, count;  // alternatives ref[first .. first + count)
};
// The compiled table: what the kernel copies into LDS.
struct Table {
  Ext ext[kExts + 1];  // [0]: no Extension
  uint8_t ref[kAlts + 1];
  Sig sig[kMaxSigs];
  uint32_t nsig, nref, nempty, max_need;
};

constexpr int hex_val(char c) {
  return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : -1;
}

constexpr bool sig_equal(const Sig& a, const Sig& b) {
  if (a.need != b.need) return false;
  for (uint32_t w = 0; w < kWords; ++w)
    if (a.val[w] != b.val[w] || a.mask[w] != b.mask[w]) return false;
  return true;
}

constexpr Table make_table() {
  Table t{};
  for (uint32_t e = 0; e < kExts; ++e) {
    Ext& x = t.ext[e + 1];
    x.kind = kSrc[e].kind;
    x.kind2 = kSrc[e].kind2;
    x.first = static_cast<uint8_t>(t.nref);
    const char* p = kSrc[e].sig;
    if (!p) continue;
    for (;;) {  // one alternative per turn
      uint8_t byte[kBodyBytes] = {}, fixed[kBodyBytes] = {};
      uint32_t len = 0, off = 0;
      while (*p && *p != '|' && *p != '+') {
        if (p[0] != '_') {
          byte[len] = static_cast<uint8_t>(hex_val(p[0]) * 16 + hex_val(p[1]));
          fixed[len] = 0xff;
        }
        ++len;
        p += 2;
      }
      if (*p == '+')
        for (++p; *p >= '0' && *p <= '9'; ++p) off = off * 10 + static_cast<uint32_t>(*p - '0');
      Sig s{};
      s.need = len ? off + len : 0;
      for (uint32_t j = 0; j < len; ++j) {
        const uint32_t at = off + j;
        s.val[at / 4] |= static_cast<uint32_t>(byte[j] & fixed[j]) << (8 * (at % 4));
        s.mask[at / 4] |= static_cast<uint32_t>(fixed[j]) << (8 * (at % 4));
      }
      uint32_t id = 0;
      while (id < t.nsig && !sig_equal(t.sig[id], s)) ++id;
      if (id == t.nsig) t.sig[t.nsig++] = s;
      t.ref[t.nref++] = static_cast<uint8_t>(id);
      ++x.count;
      if (!len) ++t.nempty;
      if (s.need > t.max_need) t.max_need = s.need;
      if (*p != '|') break;
      ++p;
    }
  }
  return t;
}

inline constexpr Table kTable = make_table();
static_assert(kExts == 215, "215 variants (extensions.rs:31-362)");
static_assert(kTable.nref == kAlts && kTable.nempty == 17, "127 alternatives, 17 of them empty");
static_assert(kTable.nsig <= kMaxSigs && kTable.max_need <= kBodyBytes, "table capacity");

constexpr uint32_t kVerifyMagic = 1u;  // SDGPU_KIND_VERIFY_MAGIC
// Categories whose signature is tested under always_check_magic_bytes
// (magic.rs:197-212): the other six are returned as they are.
constexpr uint32_t kVerified = 1u << kImage | 1u << kAudio | 1u << kVideo | 1u << kArchive |
                               1u << kExecutable | 1u << kFont | 1u << kEncrypted | 1u << kMesh |
                               1u << kDatabase;

// resolve_conflicting (magic.rs:176-236) for extension id `ext` and a file
// whose first min(size, kBodyBytes) bytes are `body` (little-endian words; L =
// how many of them are file bytes; the words past L are never looked at).
// T is kTable or a copy of it.
KIND_HD inline uint8_t kind_decide(const Table& T, uint32_t ext, const uint32_t* body, uint32_t L,
                                   uint32_t flags) {
  if (ext == 0 || ext > kExts) return kUnknown;
  const Ext e = T.ext[ext];
  const bool conflict = e.kind2 != 0;
  if (!conflict && !((flags & kVerifyMagic) && (kVerified >> e.kind & 1u))) return e.kind;
  bool hit = false;
  for (uint32_t a = e.first; a < static_cast<uint32_t>(e.first) + e.count; ++a) {
    const Sig& s = T.sig[T.ref[a]];
    bool m = L >= s.need;
    for (uint32_t w = 0; w < kWords; ++w) m = m && (body[w] & s.mask[w]) == s.val[w];
    hit = hit || m;
  }
  // a name of two categories falls back to its second one; a verified name
  // whose signature is absent has no Extension
  return hit ? e.kind : e.kind2;
}

// ---- host side -------------------------------------------------------------

// The same decision on a host buffer of L file bytes (any L; 40 are looked at).
inline uint8_t kind_of_bytes(uint32_t ext, const uint8_t* bytes, size_t L, uint32_t flags) {
  uint8_t b[kBodyBytes] = {};
  const uint32_t n = static_cast<uint32_t>(L < kBodyBytes ? L : kBodyBytes);
  if (n) memcpy(b, bytes, n);
  uint32_t w[kWords];
  for (uint32_t i = 0; i < kWords; ++i)
    w[i] = static_cast<uint32_t>(b[4 * i]) | static_cast<uint32_t>(b[4 * i + 1]) << 8 |
           static_cast<uint32_t>(b[4 * i + 2]) << 16 | static_cast<uint32_t>(b[4 * i + 3]) << 24;
  return kind_decide(kTable, ext, w, n, flags);
}

// Whether the decision for `ext` looks at file bytes at all under `flags`.
inline bool kind_reads_bytes(uint32_t ext, uint32_t flags) {
  if (ext == 0 || ext > kExts) return false;
  const Ext e = kTable.ext[ext];
  return e.kind2 != 0 || ((flags & kVerifyMagic) && (kVerified >> e.kind & 1u));
}

// Extension id of a lower-cased name of n bytes; 0 = not in the table.
inline uint16_t ext_id_of_name(const char* s, size_t n) {
  if (n == 0 || n > kNameMax) return 0;
  for (uint32_t e = 0; e < kExts; ++e)
    if (kSrc[e].name[0] == s[0] && strlen(kSrc[e].name) == n && memcmp(kSrc[e].name, s, n) == 0)
      return static_cast<uint16_t>(e + 1);
  return 0;
}

// Extension id of a path: Path::extension() -> to_str -> to_lowercase ->
// Extension::from_str (magic.rs:180-186).  The extension is what follows the
// last '.' of the file name (the last component; trailing '/' and "/." are
// skipped as Path::components does), none when the name has no '.', when its
// only '.' is its first byte, or when the name is "..".  Lower-casing: ASCII,
// and U+212A KELVIN SIGN, the one non-ASCII character whose lower case is an
// ASCII letter; any other byte >= 0x80 (which includes every ill-formed
// sequence, for which to_str gives None) cannot spell a table name.  One
// exception to the lower-casing is at the end of the function.
inline uint16_t ext_id_of_path(const char* path) {
  if (!path) return 0;
  size_t end = strlen(path);
  for (;;) {
    while (end > 1 && path[end - 1] == '/') --end;
    if (end >= 2 && path[end - 1] == '.' && path[end - 2] == '/') {
      --end;  // a trailing "/." is no component
      continue;
    }
    break;
  }
  size_t start = end;
  while (start > 0 && path[start - 1] != '/') --start;
  const char* name = path + start;
  const size_t nlen = end - start;
  if (nlen == 0 || (nlen == 2 && name[0] == '.' && name[1] == '.')) return 0;
  size_t dot = nlen;
  while (dot > 0 && name[dot - 1] != '.') --dot;
  if (dot <= 1) return 0;  // no '.', or only the leading one
  char low[kNameMax + 1];
  size_t n = 0;
  for (size_t i = dot; i < nlen; ++i) {
    const unsigned char ch = static_cast<unsigned char>(name[i]);
    char out;
    if (ch < 0x80) {
      out = ch >= 'A' && ch <= 'Z' ? static_cast<char>(ch + 32) : static_cast<char>(ch);
    } else if (ch == 0xE2 && i + 2 < nlen && static_cast<unsigned char>(name[i + 1]) == 0x84 &&
               static_cast<unsigned char>(name[i + 2]) == 0xAA) {
      out = 'k';
      i += 2;
    } else {
      return 0;
    }
    if (n == kNameMax) return 0;
    low[n++] = out;
  }
  const uint16_t id = ext_id_of_name(low, n);
  // A name of two categories is told apart by a match on the extension AS
  // WRITTEN (magic.rs:217-232: `match ext_str { "ts" .. "mts" .. _ => None }`),
  // so `x.TS` -- lower-cased into the conflict, but not spelled "ts" -- has no
  // Extension in the reference, and none here.
  if (id && kSrc[id - 1].kind2 && (nlen - dot != n || memcmp(name + dot, low, n) != 0)) return 0;
  return id;
}

}  // namespace kind
}  // namespace sdgpu
