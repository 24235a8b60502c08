// K4-K6: cas_id -> Object grouping as a radix partition + per-bucket group-by.
//
// Replaces the Object link/create decisions of identifier_job_step
// (/root/reference/core/src/object/file_identifier/mod.rs:136-333): the
// HashSet of chunk cas_ids (:136-141), the per-row `find` of an Object owning
// the same cas_id (:196-206) and the one-new-Object-per-remaining-row rule
// (:233-297), evaluated for ALL rows of a batch at once instead of 100 per job
// step.  The library-wide find_many over file_path.cas_id (:168-175), i.e.
// Objects that already exist before the batch, is the Object index of
// index.hip, consulted before this grouping (sdgpu_group_rows_indexed_device).
//
// Rows are (key, rank): key = the cas_id's 8 digest bytes as a little-endian
// u64, rank = position of the file_path in ascending-id order.  The grouping
// rule (canonical form):
//   f      = lowest rank carrying key k
//   rep(r) = r  if r / chunk_rows == f / chunk_rows   (new Object in f's chunk)
//            f  otherwise                               (linked to f's Object)
//
// Digits come from h = mix64(key) (splitmix64 finalizer), not from the raw key
// bits: the shard of the multi-GPU exchange is h's top 8 bits, a bucket is the
// `bits` hash bits below them, and the LDS slot uses h's low 32 bits.  Buckets
// are therefore balanced for any key distribution and any world size (raw key
// bits left half the buckets empty at 3 ranks), and the three are independent.
// mix64 is a bijection of u64, so the bucket records carry h itself in place of
// the key: the group-by compares hashes (equal iff the keys are) and never
// recomputes one.
//
// Pipeline (all asynchronous, no host synchronisation):
//   K6 partition: digit = `bits` hash bits below the top `skip` bits.
//      hist:    each of P blocks histograms its contiguous tile in LDS and
//               writes its counts (no global atomics): block-major rows for
//               the 12-bit bucket partition, digit-major elsewhere;
//      offsets: k_fine_scan (block-major: every block's start inside every
//               bucket, one launch; bucket starts scanned in the scatter's
//               prologue) or scan::exclusive (digit-major);
//      scatter: each block re-reads its tile and scatters its rows through LDS
//               cursors (16-B bucket records, or the exchange's send layout).
//      Used by shard (multi-GPU exchange) and by bucket; past 2^12 buckets the
//      bucket partition takes two passes, the coarse one counting every row's
//      final bucket for the second (group_layout).
//   K5 group:   one workgroup per bucket builds a linear-probing hash table of
//               (key -> min rank) in LDS (ds_cmpst_b64 / ds_min_u32), then maps
//               every row to its rep.  Buckets too large for LDS use a private
//               region of a global table instead (same code path, agent-scope
//               atomics), so any key distribution (e.g. one file duplicated a
//               million times) is handled.
// Kernels: part_device.hpp (shared with the exchange), bucket_part_device.hpp
// (K6), group_device.hpp (K5).  Here: the layout, the path choice, the entries.
#include <cerrno>
#include <cstdlib>

#include "bucket_part_device.hpp"
#include "group_device.hpp"
#include "scan_device.hpp"

namespace sdgpu {
namespace {

constexpr uint64_t kBucketRows = 3072; // target mean rows per bucket (bucket_bits_for)
// ~kBucketRows rows per bucket (LDS table load <= 75 % with slack), up to 2^15
// buckets: 100 M rows on one GPU still group in LDS.
uint32_t bucket_bits_for(uint64_t n) {
  uint32_t bits = 1;
  while (bits < kMaxBucketBits && (n >> bits) > kBucketRows) ++bits;
  return bits;
}

// The partition path of a call: direct below 12 bucket bits, staged at 12,
// two-level above -- over the coarse pass's runs while a second-pass block's
// run list holds them (kMaxRuns), else over a histogram (group_layout).
// Above 2^12 buckets (n > ~12.6 M rows) the partition runs in two passes: a
// coarse one on the top cbits = bits - 9 digit bits (<= 64 output streams per
// block) into rec1, which also counts every row's final bucket (fine counts),
// then a 9-bit LDS-staged pass per coarse segment into rec (16-record runs, 64
// blocks per segment).  A single 2^15-way scatter keeps 32 k partially written
// lines open per block and ran 3.7 ms for 100 M rows
// (profiles/r2/bench_r2b.json); the two passes move 2 x 32 B per row instead.
enum class Path { kDirect, kStaged12, kTwoLevelRuns, kTwoLevelHist };
static_assert(kMaxBucketBits - kStage2Bits <= 6, "coarse digits fit k_part_scatter_runs");
static_assert(kStage2Blocks <= kPartBlocks && kPartBlocks % kStage2Blocks == 0,
              "second-pass blocks per segment");
constexpr uint32_t kStage2Coarse = kPartBlocks / kStage2Blocks;  // per second-pass block
// one pass scatters at most 2^12 digits: its cursors fit the default dynamic LDS
static_assert((sizeof(uint32_t) << kStageBits) <= (64u << 10), "no hipFuncSetAttribute needed");

// TEST-ONLY overrides of the plan, read once per process like SDGPU_POISON_WS
// (ctx.hpp): the path of a call depends on its row count alone, so without
// them a test reaches a path only by being big enough for it -- the histogram
// one never (tests/test_gpu_forced_paths.py).  No benchmark and no default
// sets them; unset, group_layout decides as it always did.
//   SDGPU_GROUP_BITS=<1..kMaxBucketBits>  the bucket bits of every grouping
//       call of the process, bits_rows hint or not (other values: ignored);
//   SDGPU_GROUP_HIST=1  a two-level call takes Path::kTwoLevelHist whatever
//       its round count.
struct ForcedPlan {
  uint32_t bits = 0;  // 0: bucket_bits_for decides
  bool hist = false;
};
const ForcedPlan& forced_plan() {
  static const ForcedPlan f = [] {
    ForcedPlan p;
    if (const char* b = std::getenv("SDGPU_GROUP_BITS")) {
      char* end = nullptr;
      const long v = std::strtol(b, &end, 10);
      if (end != b && *end == 0 && v >= 1 && v <= static_cast<long>(kMaxBucketBits))
        p.bits = static_cast<uint32_t>(v);
    }
    const char* h = std::getenv("SDGPU_GROUP_HIST");
    p.hist = h && h[0] == '1' && h[1] == 0;
    return p;
  }();
  return f;
}

// A call's path and its workspace as typed arrays (ws null: only `total`).
constexpr uint32_t kLayoutArrays = 18;  // = the take() calls of group_layout
struct GroupLayout {
  Path path;
  bool rec12;  // 12-byte bucket records (rank_in_z); the direct path has 16-byte ones only
  uint32_t bits, cbits;
  uint32_t rounds;  // two-level: coarse rounds in the largest tile, of the record size used
  uint32_t *hist, *tiles, *hist1, *gmin;
  uint4 *rec, *rec1;
  uint64_t* gkey;
  uint32_t *fine, *fE, *ftot, *fbase, *ovf;  // block-major counts (12-bit and two-level)
  // k_part_private's run table [block][round][digit] (starts, lengths), segment sizes
  uint32_t *run_s, *run_l, *segtot;
  uint32_t* lcnt;        // ListOut: linked rows per bucket, keyed total
  uint32_t *xst, *xcnt;  // ListOut's keyless sink (KeylessSink)
  size_t total;
  // every array above in workspace order, as bytes (sdgpu_group_plan)
  struct Span {
    uint64_t off, bytes;
  } span[kLayoutArrays];
};

// bits_rows (0: n): the rows the buckets are sized for -- the keyed rows of a
// padded exchange receive, whose n counts the padding slots too (buckets
// over the LDS capacity stay correct through the global table, so the hint
// only chooses the layout).  with_sink: room for ListOut's keyless sink
// (~4 B per row; only the fused call without an index uses it).
// z_rank: the rows allow 12-byte records (rank_in_z).  The sizes depend on n,
// bits_rows and with_sink alone: the worst case over the paths.
GroupLayout group_layout(uint64_t n, uint64_t bits_rows, bool with_sink, bool z_rank,
                         void* ws = nullptr) {
  GroupLayout L;
  const ForcedPlan& forced = forced_plan();  // tests only
  L.bits = forced.bits ? forced.bits : bucket_bits_for(bits_rows && bits_rows < n ? bits_rows : n);
  L.cbits = L.bits > kStageBits ? L.bits - kStage2Bits : 0;
  L.rec12 = z_rank && L.bits >= kStageBits;
  // rounds in the largest coarse tile (kPartBlocks tiles); the run table is
  // sized for the shorter 4096-row rounds (k_part_private: priv_round)
  const uint64_t tile = L.cbits ? (n + kPartBlocks - 1) / kPartBlocks : 0;
  const auto rounds = [&](uint32_t r) { return static_cast<uint32_t>((tile + r - 1) / r); };
  const uint32_t table_rounds = rounds(priv_round<false>());
  L.rounds = L.rec12 ? rounds(priv_round<true>()) : table_rounds;
  const bool runs_fit = kStage2Coarse * static_cast<uint64_t>(L.rounds) <= kMaxRuns;
  L.path = L.bits < kStageBits         ? Path::kDirect
           : !L.cbits                  ? Path::kStaged12
           : runs_fit && !forced.hist  ? Path::kTwoLevelRuns
                                       : Path::kTwoLevelHist;
  const uint64_t nh = (static_cast<uint64_t>(1) << L.bits) * kMaxPartBlocks;
  const uint64_t nh1 = (static_cast<uint64_t>(1) << L.cbits) * kMaxPartBlocks;
  const uint64_t nf = static_cast<uint64_t>(1) << L.bits;
  const uint64_t nrun = static_cast<uint64_t>(kPartBlocks) * table_rounds * kRunMaxBins;
  const uint64_t nsink = with_sink ? static_cast<uint64_t>(kPartBlocks) * kSinkWaves : 0;
  size_t o = 0;
  uint32_t na = 0;
  const auto take = [&](auto*& p, uint64_t bytes) {  // the next 256-B aligned bytes
    p = reinterpret_cast<std::remove_reference_t<decltype(p)>>(reinterpret_cast<uintptr_t>(ws) + o);
    L.span[na++] = {o, bytes};
    o = align_up(o + bytes, 256);
  };
  take(L.hist, 4 * (nh + 1));
  take(L.tiles, 4 * (scan::tiles_for(nh) + 1));
  take(L.rec, 16 * n);
  take(L.hist1, 4 * (nh1 + 1));
  take(L.rec1, L.cbits ? 16 * n : 0);
  take(L.gkey, 8 * 4 * n);
  take(L.gmin, 4 * 4 * n);
  take(L.fine, 4 * nf * kPartBlocks);
  take(L.fE, 4 * nf * kPartBlocks);
  take(L.ftot, 4 * nf);
  take(L.fbase, 4 * (nf + 1));
  take(L.ovf, 4);
  take(L.run_s, 4 * nrun);
  take(L.run_l, 4 * nrun);
  take(L.segtot, 4 * kRunMaxBins);
  take(L.lcnt, 4 * (nf + 1));
  take(L.xst, 4 * nsink * sink_cap(n));
  take(L.xcnt, 4 * nsink);
  L.total = o;
  return L;
}

// The output's share of the workspace.  own_sink: the first partition pass
// collects the valid keyless rows into the workspace's segments.
void out_bind(RepOut&, const GroupLayout&, bool, uint64_t) {}
void out_bind(ListOut& o, const GroupLayout& L, bool own_sink, uint64_t n) {
  o.lcnt = L.lcnt;
  if (own_sink) o.x.st = L.xst, o.x.cnt = L.xcnt, o.x.cap = sink_cap(n);
}
KeylessSink sink_of(const RepOut&) { return KeylessSink{}; }
KeylessSink sink_of(const ListOut& o) { return o.x; }
hipError_t out_finish(const RepOut&, uint32_t, hipStream_t) { return hipSuccess; }
hipError_t out_finish(const ListOut& o, uint32_t nb, hipStream_t s) {
  k_list_finish<<<o.x.st ? 1 + kPartBlocks : 1u, 1024, 0, s>>>(o.lcnt, nb, o.counts, o.who, o.x,
                                                                 o.cap, o.nospc);
  return hipGetLastError();
}

// Rows whose bucket records can be 12 bytes {hash, z} with rank = rank_base
// + z: the caller's rows without a rank array (z = row), and received
// exchange records for an output that needs no row (RecRankIn: z = rank).
template <typename In>
constexpr bool kMayRankInZ = std::is_same<In, RowsIn>::value || std::is_same<In, RecRankIn>::value;
template <typename In>
bool rank_in_z(const In& in) {
  if constexpr (std::is_same<In, RowsIn>::value) return !in.rank;
  else return std::is_same<In, RecRankIn>::value;
}
template <typename In>
uint32_t z_rank_base(const In& in) {
  if constexpr (std::is_same<In, RowsIn>::value) return in.rank_base;
  else return 0u;
}

// One grouping call, as every path receives it.
template <typename In, typename Out>
struct GroupCall {
  In in;
  uint64_t n;
  uint32_t chunk_rows;
  uint32_t* rep;  // with init_rep: every row's rep starts as its rank (first scatter)
  bool init_rep;
  Out out;
  GroupLayout L;
  hipStream_t s;
  KTimer* timer;
};

// A runtime flag as a template argument, so a launch is written once.
template <typename F>
void with_flag(bool b, F f) {
  b ? f(std::true_type{}) : f(std::false_type{});
}
// with_flag for "this first pass fills the keyless sink": only one over the
// caller's rows (RowsIn) does, so the sinking kernels exist for RowsIn alone.
template <typename In, typename F>
void with_sink(const KeylessSink& xs, F f) {
  if constexpr (std::is_same<In, RowsIn>::value) {
    if (xs.st) return f(std::true_type{});
  }
  f(std::false_type{});
}

// A first-pass histogram, with the keyless sink when the output has one.
template <typename In, typename Out>
void hist_launch(const GroupCall<In, Out>& c, uint32_t bits, uint32_t* hist,
                 uint32_t* zero = nullptr, bool blk_major = false) {
  const KeylessSink xs = sink_of(c.out);
  const size_t lds = sizeof(uint32_t) << bits;
  with_sink<In>(xs, [&](auto sunk) {
    constexpr bool kX = decltype(sunk)::value;
    k_part_hist<In, kX><<<kPartBlocks, kPartThreads, lds, c.s>>>(
        c.in, c.n, kShardBits, bits, 0, hist, zero, blk_major, kX ? xs : KeylessSink{});
  });
}

// K5, one workgroup per bucket, then the output's finish: the direct path's
// 16-byte records at the scanned offsets, else 12- or 16-byte records for the
// packed table (>= 12 digit bits).  Round 5 measured a persistent,
// LDS-staged variant (one workgroup per CU copying the next bucket's records
// to LDS with global_load_lds while grouping the current one): 2.2x slower
// (it halves the resident workgroups of a VALU-bound kernel; DESIGN.md 4.3,
// commit 1346212).
template <bool kRec12, typename In, typename Out>
hipError_t group_kernel_launch(const GroupCall<In, Out>& c) {
  const uint32_t nb = 1u << c.L.bits;
  const ChunkOf chunk_of = ChunkOf::make(c.chunk_rows);
  KScope k(c.timer, "bucket_group", c.s);
  if (c.L.path == Path::kDirect)
    k_bucket_group<Out><<<nb, kGroupThreads, 0, c.s>>>(c.L.rec, c.L.hist, kPartBlocks, chunk_of,
                                                       c.L.gkey, c.L.gmin, c.out);
  else if constexpr (kRec12)
    k_bucket_group12_pk<Out><<<nb, kGroupThreads, 0, c.s>>>(
        reinterpret_cast<const uint3*>(c.L.rec), z_rank_base(c.in), c.L.fbase, c.L.bits, chunk_of,
        c.L.gkey, c.L.gmin, c.out);
  else
    k_bucket_group_pk<Out><<<nb, kGroupThreads, 0, c.s>>>(c.L.rec, c.L.fbase, 1, c.L.bits, chunk_of,
                                                          c.L.gkey, c.L.gmin, c.out);
  return out_finish(c.out, nb, c.s);
}

// Fewer than 2^12 buckets: digit-major histogram, scan, one scatter of
// 16-byte records; the group kernel has the 12-byte-slot table.
template <typename In, typename Out>
hipError_t direct_launch(const GroupCall<In, Out>& c) {
  const GroupLayout& L = c.L;
  const uint32_t bits = L.bits, nb = 1u << bits;
  const size_t lds = sizeof(uint32_t) << bits;
  {
    KScope k(c.timer, "bucket_hist", c.s);
    hist_launch(c, bits, L.hist);
  }
  scan::exclusive(L.hist, static_cast<uint64_t>(nb) * kPartBlocks, L.hist, L.tiles, nullptr, c.s);
  {
    KScope k(c.timer, "bucket_scatter", c.s);
    with_flag(c.init_rep, [&](auto init) {
      constexpr bool kInit = decltype(init)::value;
      k_part_scatter_rec<In, kInit><<<kPartBlocks, kPartThreads, lds, c.s>>>(
          c.in, c.n, kShardBits, bits, L.hist, L.rec, c.rep);
    });
  }
  return group_kernel_launch<false>(c);
}

// 12-bit digits: block-major counts, k_fine_scan for every block's start
// inside every bucket (one launch instead of the 3-launch scan), bucket
// starts scanned in the staged scatter's prologue.
template <bool kRec12, typename In, typename Out>
hipError_t staged12_launch(const GroupCall<In, Out>& c) {
  const GroupLayout& L = c.L;
  constexpr uint32_t nb = 1u << kStageBits;
  {
    KScope k(c.timer, "bucket_hist", c.s);
    hist_launch(c, kStageBits, L.fine, nullptr, true);
    k_fine_scan<kPartBlocks, 1><<<nb / 64, 1024, 0, c.s>>>(L.fine, nb, L.fE, L.ftot, L.ovf);
  }
  {
    KScope k(c.timer, "bucket_scatter", c.s);
    with_flag(c.init_rep, [&](auto init) {
      constexpr bool kInit = decltype(init)::value;
      if constexpr (!kRec12)
        k_part_scatter_rec_staged<In, kInit><<<kPartBlocks, kPartThreads, 0, c.s>>>(
            c.in, c.n, kShardBits, L.fE, L.rec, c.rep, nullptr, 0, L.ftot, L.fbase);
      else if constexpr (!kInit || std::is_same<In, RowsIn>::value)  // rep = rank_base + row
        k_part_scatter_ws<In, kInit><<<kPartBlocks, kPartThreads, 0, c.s>>>(
            c.in, c.n, kShardBits, L.fE, L.ftot, reinterpret_cast<uint3*>(L.rec), c.rep, L.fbase);
    });
  }
  return group_kernel_launch<kRec12>(c);
}

// Two-level partition (n > 4096 x kBucketRows) + group: see Path.  kStage2Bits
// digit bits per segment in the second pass, kStage2Slots-record staging runs,
// kStage2Rows rows per thread per round, kStage2Blocks blocks per segment.
// The second pass's offsets come from the coarse pass's fine counts
// (k_fine_scan; bucket starts scanned in the second pass's prologue): no
// histogram pass over the coarse records.  kRec12: rows without a rank array
// (rank = rank_base + row), 12-byte records in both passes.
// No histogram pass: the coarse pass writes each block's records into its
// own tile range as runs, the second pass reads segments as run lists.
template <bool kRec12, typename In, typename Out>
hipError_t two_level_runs_launch(const GroupCall<In, Out>& c) {
  using RecT = typename std::conditional<kRec12, uint3, uint4>::type;
  const GroupLayout& L = c.L;
  const uint32_t nfine = 1u << L.bits, nseg = 1u << L.cbits, skip2 = kShardBits + L.cbits;
  k_zero_runs<<<1, 64, 0, c.s>>>(L.segtot, L.ovf);
  {
    KScope k(c.timer, "bucket_scatter1", c.s);
    const KeylessSink xs = sink_of(c.out);
    auto coarse = [&](auto init, auto sunk) {
      constexpr bool kX = decltype(sunk)::value;
      k_part_private<In, decltype(init)::value, kRec12, kX><<<kPartBlocks, kPartThreads, 0, c.s>>>(
          c.in, c.n, kShardBits, L.cbits, L.rec1, c.rep, L.bits, L.fine, L.ovf, L.run_s, L.run_l,
          L.rounds, L.segtot, kX ? xs : KeylessSink{});
    };
    with_sink<In>(xs, [&](auto sunk) {
      if constexpr (decltype(sunk)::value)  // the write set: no rep array
        coarse(std::false_type{}, sunk);
      else
        with_flag(c.init_rep, [&](auto init) { coarse(init, sunk); });
    });
  }
  {
    KScope k(c.timer, "bucket_fine_scan", c.s);
    k_fine_recount_runs<kStage2Bits, RecT><<<kPartBlocks, kPartThreads, 0, c.s>>>(
        reinterpret_cast<const RecT*>(L.rec1), skip2, L.run_s, L.run_l, L.rounds, kPartBlocks, nseg,
        L.bits, L.fine, L.ovf);
    k_fine_scan<kStage2Blocks, kStage2Coarse><<<(nfine + 63) / 64, 1024, 0, c.s>>>(
        L.fine, nfine, L.fE, L.ftot, L.ovf);
  }
  // second pass over all segments, then the group-by over all buckets.
  // (Round 5 tried the two interleaved per group of segments, so the group
  // kernel would read records still in the Infinity Cache: slower at every
  // G, 1.807 -> 1.831-1.990 ms at 100 M rows, and removed in round 6 --
  // DESIGN.md 4.3, "segment groups".)
  {
    KScope k(c.timer, "bucket_scatter", c.s);
    k_part2_runs<kRec12, kStage2Bits, kStage2Slots, kStage2Rows, kStage2Slots>
        <<<dim3(kStage2Blocks, nseg), kPartThreads, 0, c.s>>>(L.rec1, skip2, L.fE, L.rec, L.run_s,
                                                              L.run_l, L.rounds, kPartBlocks,
                                                              kStage2Coarse, L.segtot, L.ftot,
                                                              L.fbase);
  }
  return group_kernel_launch<kRec12>(c);
}

// The two-level partition when a block's coarse rounds outgrow the second
// pass's run list (kMaxRuns): a histogram pass and a scan give the coarse
// pass global offsets, and the staged scatter reads whole segments.  Only
// above ~2^28 rows per call; tests/test_gpu_forced_paths.py reaches it at small
// row counts through SDGPU_GROUP_HIST (forced_plan).
template <bool kRec12, typename In, typename Out>
hipError_t two_level_hist_launch(const GroupCall<In, Out>& c) {
  using RecT = typename std::conditional<kRec12, uint3, uint4>::type;
  const GroupLayout& L = c.L;
  const uint32_t nfine = 1u << L.bits, nseg = 1u << L.cbits, skip2 = kShardBits + L.cbits;
  // pass 1: coarse partition on the top cbits digit bits (rep initialised
  // here), counting every row's final bucket on the way
  {
    KScope k(c.timer, "bucket_hist", c.s);
    hist_launch(c, L.cbits, L.hist1, L.ovf);
  }
  scan::exclusive(L.hist1, static_cast<uint64_t>(nseg) * kPartBlocks, L.hist1, L.tiles, nullptr,
                  c.s);
  {
    KScope k(c.timer, "bucket_scatter1", c.s);
    with_flag(c.init_rep, [&](auto init) {
      k_part_scatter_runs<In, decltype(init)::value, kRec12><<<kPartBlocks, kPartThreads, 0, c.s>>>(
          c.in, c.n, kShardBits, L.cbits, L.hist1, L.rec1, c.rep, L.bits, L.fine, L.ovf);
    });
  }
  // pass 2: kStage2Bits bits below, per coarse segment, staged in
  // kStage2Slots-record runs
  using In2 = typename std::conditional<kRec12, Rec12In, Rec16In>::type;
  In2 in2;
  if constexpr (kRec12)
    in2 = Rec12In{reinterpret_cast<const uint3*>(L.rec1), z_rank_base(c.in)};
  else
    in2 = Rec16In{L.rec1};
  {
    KScope k(c.timer, "bucket_fine_scan", c.s);
    k_fine_recount<kStage2Bits, RecT><<<kPartBlocks, kPartThreads, 0, c.s>>>(
        reinterpret_cast<const RecT*>(L.rec1), skip2, L.hist1, kPartBlocks, nseg, L.bits, L.fine,
        L.ovf);
    k_fine_scan<kStage2Blocks, kStage2Coarse><<<(nfine + 63) / 64, 1024, 0, c.s>>>(
        L.fine, nfine, L.fE, L.ftot, L.ovf);
  }
  {
    KScope k(c.timer, "bucket_scatter", c.s);
    k_part_scatter_rec_staged<In2, false, kStage2Bits, kStage2Slots, kStage2Rows, kRec12>
        <<<dim3(kStage2Blocks, nseg), kPartThreads, 0, c.s>>>(in2, 0, skip2, L.fE, L.rec, nullptr,
                                                              L.hist1, kPartBlocks, L.ftot, L.fbase,
                                                              kStage2Coarse);
  }
  return group_kernel_launch<kRec12>(c);
}

template <bool kRec12, typename In, typename Out>
hipError_t path_launch(const GroupCall<In, Out>& c) {
  switch (c.L.path) {
    case Path::kStaged12: return staged12_launch<kRec12>(c);
    case Path::kTwoLevelRuns: return two_level_runs_launch<kRec12>(c);
    case Path::kTwoLevelHist: return two_level_hist_launch<kRec12>(c);
    case Path::kDirect: break;
  }
  return direct_launch(c);
}

// own_sink: the first pass collects ListOut's valid keyless rows into ws.
template <typename In, typename Out>
hipError_t group_launch(In in, const GroupInput& gi, uint32_t chunk_rows, uint32_t* rep,
                        bool init_rep, Out out, bool own_sink, void* ws, hipStream_t s,
                        KTimer* timer) {
  GroupCall<In, Out> c{in, gi.n, chunk_rows, rep, init_rep, out,
                       group_layout(gi.n, gi.bits_rows, own_sink, rank_in_z(in), ws), s, timer};
  out_bind(c.out, c.L, own_sink, gi.n);
  if constexpr (kMayRankInZ<In>) {
    if (c.L.rec12) return path_launch<true>(c);
  }
  return path_launch<false>(c);
}

}  // namespace

size_t dedup_workspace_bytes(uint64_t n, bool with_sink) {
  return group_layout(n, 0, with_sink, false).total;
}

hipError_t dedup_local_launch(const GroupInput& in, uint32_t chunk_rows, uint32_t* rep,
                              bool init_rep, void* ws, hipStream_t s, KTimer* timer) {
  if (in.n == 0) return hipSuccess;
  if (in.rec12)
    return group_launch(RecIn{reinterpret_cast<const uint3*>(in.rec12), in.valid}, in, chunk_rows,
                        rep, init_rep, RepOut{rep}, false, ws, s, timer);
  return group_launch(RowsIn{in.key, in.valid, in.rank, in.rank_base}, in, chunk_rows, rep,
                      init_rep, RepOut{rep}, false, ws, s, timer);
}

hipError_t dedup_list_launch(const GroupInput& in, uint32_t chunk_rows, uint32_t* who,
                             uint32_t* obj, uint32_t* counts, void* ws, hipStream_t s,
                             KTimer* timer, bool sink_keyless, const uint8_t* keyless_valid,
                             uint32_t cap, uint32_t* nospc, const KeylessSink* moved) {
  if (in.n == 0) return hipSuccess;
  const bool sink = sink_keyless && !in.rec12 && in.valid;
  ListOut out{who, obj, counts, nullptr, KeylessSink{}};  // lcnt, the sink's segments: out_bind
  if (nospc) out.cap = cap, out.nospc = nospc;
  if (sink) out.x.valid = keyless_valid;
  else if (moved) out.x = *moved;  // segments filled by the exchange's partition (k_part_padded)
  if (in.rec12)  // the list needs no row index: 12-byte bucket records carrying the rank
    return group_launch(RecRankIn{{reinterpret_cast<const uint3*>(in.rec12), in.valid}}, in,
                        chunk_rows, nullptr, false, out, sink, ws, s, timer);
  return group_launch(RowsIn{in.key, in.valid, in.rank, in.rank_base}, in, chunk_rows, nullptr,
                      false, out, sink, ws, s, timer);
}

}  // namespace sdgpu

// The plan of a grouping call -- what group_layout decides from the row count
// (and the test-only overrides), without touching a device: for tests
// (internal.hpp; not part of the C ABI of include/sdgpu.h).
extern "C" int sdgpu_group_plan(uint64_t n, uint64_t bits_rows, int implicit_rank, int with_sink,
                                uint64_t* out, uint32_t cap) {
  using namespace sdgpu;
  constexpr uint32_t kHead = 7, kWords = kHead + 2 * kLayoutArrays;
  if (!out || cap < kWords || n == 0) return -EINVAL;
  const GroupLayout L = group_layout(n, bits_rows, with_sink != 0, implicit_rank != 0);
  out[0] = L.bits;
  out[1] = L.cbits;
  out[2] = L.rec12;
  out[3] = L.rounds;  // as passed to the two-level kernels
  out[4] = static_cast<uint64_t>(L.path);
  out[5] = L.total;
  out[6] = dedup_workspace_bytes(n, with_sink != 0);  // what a caller allocates for n rows
  for (uint32_t a = 0; a < kLayoutArrays; ++a) {  // GroupLayout's arrays in workspace order
    out[kHead + 2 * a] = L.span[a].off;
    out[kHead + 1 + 2 * a] = L.span[a].bytes;
  }
  return static_cast<int>(kWords);
}
