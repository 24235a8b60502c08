// K6 bucket partition of the grouping (dedup.hip): the scatter kernels of its
// four paths -- direct, 12-bit staged, two-level over runs, two-level over a
// histogram -- and the fine-count kernels between the two levels.
#pragma once

#include "part_device.hpp"

namespace sdgpu {
namespace {

constexpr uint32_t kMaxBucketBits = 15;  // 2^15 buckets: 100 M rows stay in LDS

// Bucket partition writing ONE 16-byte record {hash lo, hash hi, rank, row}
// per keyed row (a single scattered store instead of three).  kInitRep: every
// row's rep is first set to its own rank here (one coalesced store); rows
// without a key are not partitioned, and K5 rewrites only the rows that link
// to an earlier chunk.  (The indexed grouping initialises rep in its probe.)
template <typename In, bool kInitRep>
__global__ __launch_bounds__(kPartThreads) void k_part_scatter_rec(
    In in, uint64_t n, uint32_t skip, uint32_t bits, const uint32_t* __restrict__ offs,
    uint4* __restrict__ rec, uint32_t* __restrict__ rep) {
  extern __shared__ __attribute__((aligned(16))) uint32_t cur[];
  const uint32_t nbins = 1u << bits;
  for (uint32_t b = threadIdx.x; b < nbins; b += kPartThreads)
    cur[b] = offs[static_cast<uint64_t>(b) * gridDim.x + part_block()];
  __syncthreads();
  uint64_t t0, t1;
  tile_of(n, gridDim.x, t0, t1);
  constexpr int U = kUnroll;
  for (uint64_t i0 = t0 + threadIdx.x; i0 < t1; i0 += U * kPartThreads) {
    RowBatch<U> q;
    in.template load_many<U>(i0, kPartThreads, t1, i0, q);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint64_t i = i0 + static_cast<uint64_t>(u) * kPartThreads;
      const uint32_t r = in.rank_of(q, u);
      // every row starts as its own Object (coalesced store): rows without a
      // key stay so (mod.rs:238-239); K5 overwrites only the rows that link
      if (kInitRep && q.in[u]) rep[i] = r;
      if (!in.valid_of(q, u)) continue;
      const uint64_t h = in_hash<In>(in.key_of(q, u));
      const uint32_t p = atomicAdd(&cur[digit_of(h, skip, bits)], 1u);
      rec[p] = make_uint4(static_cast<uint32_t>(h), static_cast<uint32_t>(h >> 32), r,
                          in.row_of(q, u));
    }
  }
}

// Partition into few digits (<= 64: the coarse pass of the two-level
// partition) in sorted runs: each round the block's kPartThreads x 4 rows are
// counting-sorted by digit in LDS (64 KiB) and leave as one contiguous run per
// digit (~4096 / nbins records, consecutive lanes on consecutive addresses)
// instead of one scattered 16-B store per row.  The next round's rows are
// loaded during the current one (ping-pong batches, LDS-only barriers).
// The block also counts its rows per FINAL bucket (the fbits hash bits below
// `skip`: coarse digit + second-pass digit) in 16-bit LDS counters and writes
// them to fine[block][bucket] -- the second pass's histogram, which therefore
// needs no pass over the records of its own.  A counter that would pass 65535
// (one key filling more than 64 Ki rows of a block's tile) sets *ovf, and
// k_fine_recount rebuilds the counts from the records instead.
// kRec12: 12-byte records {hash lo, hash hi, row} (rank = rank_base + row).
constexpr uint32_t kRunMaxBins = 64;
template <typename In, bool kInitRep, bool kRec12 = false>
__global__ __launch_bounds__(kPartThreads) void k_part_scatter_runs(
    In in, uint64_t n, uint32_t skip, uint32_t bits, const uint32_t* __restrict__ offs,
    uint4* __restrict__ rec, uint32_t* __restrict__ rep, uint32_t fbits,
    uint32_t* __restrict__ fine, uint32_t* __restrict__ ovf) {
  constexpr int U = 4;
  constexpr uint32_t R = U * kPartThreads;
  using RecT = typename std::conditional<kRec12, uint3, uint4>::type;
  __shared__ RecT buf[R];
  RecT* __restrict__ out = reinterpret_cast<RecT*>(rec);
  __shared__ uint32_t cnt[kRunMaxBins], base[kRunMaxBins + 1], cur[kRunMaxBins];
  __shared__ uint32_t fc[1u << (kMaxBucketBits - 1)];  // 2 x 16-bit counters per word
  const uint32_t nbins = 1u << bits, nfine = 1u << fbits;
  if (threadIdx.x < nbins)
    cur[threadIdx.x] = offs[static_cast<uint64_t>(threadIdx.x) * gridDim.x + part_block()];
  for (uint32_t b = threadIdx.x; b < nfine / 2; b += kPartThreads) fc[b] = 0;
  bool over = false;
  uint64_t t0, t1;
  tile_of(n, gridDim.x, t0, t1);
  auto round = [&](const RowBatch<U>& q, uint64_t i0) {
    if (threadIdx.x < nbins) cnt[threadIdx.x] = 0;
    lds_barrier();
    uint32_t dg[U], lr[U];
    RecT rq[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint64_t i = i0 + threadIdx.x + static_cast<uint64_t>(u) * kPartThreads;
      dg[u] = ~0u;
      if (!q.in[u]) continue;
      const uint32_t r = in.rank_of(q, u);
      if (kInitRep) rep[i] = r;
      if (!in.valid_of(q, u)) continue;
      const uint64_t h = in_hash<In>(in.key_of(q, u));
      dg[u] = digit_of(h, skip, bits);
      lr[u] = atomicAdd(&cnt[dg[u]], 1u);
      const uint32_t fb = digit_of(h, skip, fbits), sh = (fb & 1u) << 4;
      over |= ((atomicAdd(&fc[fb >> 1], 1u << sh) >> sh) & 0xFFFFu) == 0xFFFFu;
      if constexpr (kRec12)
        rq[u] = make_uint3(static_cast<uint32_t>(h), static_cast<uint32_t>(h >> 32), in.row_of(q, u));
      else
        rq[u] = make_uint4(static_cast<uint32_t>(h), static_cast<uint32_t>(h >> 32), r,
                           in.row_of(q, u));
    }
    lds_barrier();
    if (threadIdx.x < 64) {  // the (<= 64) run starts: one wave's shuffle scan
      static_assert(kRunMaxBins <= 64, "one wave scans the run starts");
      const uint32_t lane = threadIdx.x;
      const uint32_t v = lane < nbins ? cnt[lane] : 0u;
      uint32_t inc = v;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(inc, d);
        if (lane >= static_cast<uint32_t>(d)) inc += o;
      }
      if (lane < nbins) base[lane] = inc - v;
      if (lane == nbins - 1) base[nbins] = inc;
    }
    lds_barrier();
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (dg[u] != ~0u) buf[base[dg[u]] + lr[u]] = rq[u];
    lds_barrier();
    const uint32_t total = base[nbins];
    for (uint32_t k = threadIdx.x; k < total; k += kPartThreads) {
      const RecT v = buf[k];
      const uint32_t b = digit_of((static_cast<uint64_t>(v.y) << 32) | v.x, skip, bits);
      out[cur[b] + (k - base[b])] = v;
    }
    lds_barrier();
    if (threadIdx.x < nbins) cur[threadIdx.x] += cnt[threadIdx.x];
  };
  constexpr uint64_t kStep = R;
  if (t0 < t1) {
    RowBatch<U> qa, qb;
    in.template load_many<U>(t0 + threadIdx.x, kPartThreads, t1, t0, qa);
    for (uint64_t i0 = t0;; i0 += 2 * kStep) {  // uniform trip count
      in.template load_many<U>(i0 + kStep + threadIdx.x, kPartThreads, t1, t0, qb);
      round(qa, i0);
      if (i0 + kStep >= t1) break;
      in.template load_many<U>(i0 + 2 * kStep + threadIdx.x, kPartThreads, t1, t0, qa);
      round(qb, i0 + kStep);
      if (i0 + 2 * kStep >= t1) break;
    }
  }
  if (over) *ovf = 1u;
  __syncthreads();
  uint32_t* f = fine + static_cast<uint64_t>(part_block()) * nfine;
  for (uint32_t b = threadIdx.x; b < nfine; b += kPartThreads)
    f[b] = (fc[b >> 1] >> ((b & 1u) << 4)) & 0xFFFFu;
}

// The coarse pass WITHOUT a histogram pass before it (round 3): each block
// writes its keyed rows into its own tile's range of the record array,
// [t0, t0 + keyed rows), round after round, each round counting-sorted by
// coarse digit in LDS and stored as ONE contiguous chunk; a run table records
// where every (block, round, digit) run starts and how long it is, and the
// block adds its per-digit totals to segtot (the segment sizes).  The second
// pass (k_part2_runs) reads a segment's records as those runs, so no global
// offsets -- and no k_part_hist pass over all rows -- are needed.  Fine
// counts per final bucket as in k_part_scatter_runs.
// Rows per thread per round of k_part_private: 12-byte records take 8192-row
// rounds (96 KiB of sort buffer beside 8-bit fine counters): half the runs of
// 4096-row rounds, each twice as long, for the second pass to read.  16-byte
// records keep 4096-row rounds and 16-bit counters (64 KiB + 64 KiB).
template <bool kRec12>
constexpr int priv_rows() { return kRec12 ? 8 : 4; }
template <bool kRec12>
constexpr uint32_t priv_round() { return static_cast<uint32_t>(priv_rows<kRec12>()) * kPartThreads; }

template <typename In, bool kInitRep, bool kRec12 = false, bool kX = false>
__global__ __launch_bounds__(kPartThreads) void k_part_private(
    In in, uint64_t n, uint32_t skip, uint32_t bits, uint4* __restrict__ rec,
    uint32_t* __restrict__ rep, uint32_t fbits, uint32_t* __restrict__ fine,
    uint32_t* __restrict__ ovf, uint32_t* __restrict__ run_start, uint32_t* __restrict__ run_len,
    uint32_t max_rounds, uint32_t* __restrict__ segtot, KeylessSink xs = KeylessSink{}) {
  constexpr int U = priv_rows<kRec12>();
  constexpr uint32_t R = priv_round<kRec12>();
  using RecT = typename std::conditional<kRec12, uint3, uint4>::type;
  __shared__ RecT buf[R];
  RecT* __restrict__ out = reinterpret_cast<RecT*>(rec);
  __shared__ uint32_t cnt[2][kRunMaxBins];  // digit counts, by round parity
  // fine counters, kFc bits each, 32 / kFc per word, added to without a
  // return value.  A counter that wraps (a key filling 256 / 65536 rows of
  // one tile's final bucket) loses 2^kFc and gives its neighbour at most 1,
  // so the block's counters then sum to less than its rows: that sets the
  // overflow flag, and k_fine_recount_runs rebuilds every count from the
  // records.
  constexpr uint32_t kFc = kRec12 ? 8u : 16u, kFcPer = 32u / kFc, kFcMax = (1u << kFc) - 1u;
  constexpr uint32_t kFcShift = kRec12 ? 2u : 1u;
  static_assert((1u << kFcShift) == kFcPer, "counters per word");
  __shared__ uint32_t fc[(1u << kMaxBucketBits) / kFcPer];
  const uint32_t nbins = 1u << bits, nfine = 1u << fbits;
  const uint32_t blk = part_block();
  uint32_t wn = 0;  // the wave's keyless rows (KeylessSink)
  for (uint32_t b = threadIdx.x; b < nfine / kFcPer; b += kPartThreads) fc[b] = 0;
  uint64_t t0, t1;
  tile_of(n, gridDim.x, t0, t1);
  uint32_t acc = 0, r = 0, dsum = 0;  // records written, rounds done; wave 0: its digit's total
  // KeylessSink: the keyless rows of kKmRounds rounds as bits of km (bit U k + u:
  // round rbase + k, the thread's row u), sunk together -- the rounds' own
  // loops carry one OR on their rare keyless branch, nothing else (a ballot
  // test per round measured +0.02 ms at 100 M rows)
  constexpr uint32_t kKmRounds = 32u / U;
  static_assert((kKmRounds & (kKmRounds - 1)) == 0, "rounds per sink flush: a power of two");
  uint32_t km = 0;
  auto flush = [&](uint32_t rbase) {
    if constexpr (kX) {
      for (uint64_t b = __ballot(km != 0); b; b = __ballot(km != 0)) {
        const uint32_t p = __ffs(__shfl(km, __ffsll(static_cast<unsigned long long>(b)) - 1)) - 1;
        const uint64_t i = t0 + static_cast<uint64_t>(rbase + p / U) * R + threadIdx.x +
                           static_cast<uint64_t>(p % U) * kPartThreads;
        sink_keyless<kRec12>(xs, in, (km >> p) & 1u, i, wn);
        km &= ~(1u << p);
      }
    }
    (void)rbase;
  };
  // Digit counters by round parity: every wave reads round r's after the
  // first barrier, so wave 0 zeroes the OTHER array (read in round r - 1)
  // for round r + 1 -- no barrier of its own.  Three barriers per round:
  // counted, sorted into the buffer, stored.
  if (threadIdx.x < 2 * kRunMaxBins) (&cnt[0][0])[threadIdx.x] = 0;
  __syncthreads();
  auto round = [&](const RowBatch<U>& q, uint64_t i0) {
    const uint32_t p = r & 1u;
    uint32_t dg[U], lr[U];
    RecT rq[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint64_t i = i0 + threadIdx.x + static_cast<uint64_t>(u) * kPartThreads;
      dg[u] = ~0u;
      if (!q.in[u]) continue;
      const uint32_t rk = in.rank_of(q, u);
      if (kInitRep) rep[i] = rk;
      if (!in.valid_of(q, u)) {
        if constexpr (kX) km |= 1u << (U * (r & (kKmRounds - 1)) + u);  // sunk every kKmRounds
        continue;
      }
      const uint64_t h = in_hash<In>(in.key_of(q, u));
      dg[u] = digit_of(h, skip, bits);
      lr[u] = atomicAdd(&cnt[p][dg[u]], 1u);
      const uint32_t fb = digit_of(h, skip, fbits), sh = (fb & (kFcPer - 1u)) * kFc;
      atomicAdd(&fc[fb >> kFcShift], 1u << sh);
      if constexpr (kRec12)
        rq[u] = make_uint3(static_cast<uint32_t>(h), static_cast<uint32_t>(h >> 32), in.row_of(q, u));
      else
        rq[u] = make_uint4(static_cast<uint32_t>(h), static_cast<uint32_t>(h >> 32), rk,
                           in.row_of(q, u));
    }
    lds_barrier();
    // every wave scans the (<= 64) digit counts itself, lane d holding digit
    // d's run start, so the buffer scatter reads its bases by a lane shuffle
    // instead of from LDS written behind a second barrier
    static_assert(kRunMaxBins <= 64, "one wave scans the run starts");
    const uint32_t lane = __lane_id();
    const uint32_t v = lane < nbins ? cnt[p][lane] : 0u;
    uint32_t inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t o = __shfl_up(inc, d);
      if (lane >= static_cast<uint32_t>(d)) inc += o;
    }
    const uint32_t excl = inc - v;
    const uint32_t total = __shfl(inc, 63);
    if (threadIdx.x < 64) {  // the run table row; the other parity's counters zeroed
      if (lane < nbins) cnt[p ^ 1u][lane] = 0;
      const uint64_t e = (static_cast<uint64_t>(blk) * max_rounds + r) * kRunMaxBins + lane;
      run_start[e] = static_cast<uint32_t>(t0) + acc + excl;
      run_len[e] = v;
      dsum += v;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint32_t bb = __shfl(excl, static_cast<int>(dg[u] & 63u));
      if (dg[u] != ~0u) buf[bb + lr[u]] = rq[u];
    }
    lds_barrier();
    for (uint32_t k = threadIdx.x; k < total; k += kPartThreads) out[t0 + acc + k] = buf[k];
    acc += total;
    ++r;
    if constexpr (kX)
      if ((r & (kKmRounds - 1)) == 0) flush(r - kKmRounds);
    lds_barrier();
  };
  constexpr uint64_t kStep = R;
  if (t0 < t1) {
    RowBatch<U> qa, qb;
    in.template load_many<U>(t0 + threadIdx.x, kPartThreads, t1, t0, qa);
    for (uint64_t i0 = t0;; i0 += 2 * kStep) {  // uniform trip count
      in.template load_many<U>(i0 + kStep + threadIdx.x, kPartThreads, t1, t0, qb);
      round(qa, i0);
      if (i0 + kStep >= t1) break;
      in.template load_many<U>(i0 + 2 * kStep + threadIdx.x, kPartThreads, t1, t0, qa);
      round(qb, i0 + kStep);
      if (i0 + 2 * kStep >= t1) break;
    }
  }
  if constexpr (kX) flush(r & ~(kKmRounds - 1));
  if (threadIdx.x < 64) {  // rounds this tile did not have: empty runs
    for (uint32_t rr = r; rr < max_rounds; ++rr)
      run_len[(static_cast<uint64_t>(blk) * max_rounds + rr) * kRunMaxBins + threadIdx.x] = 0u;
    if (threadIdx.x < nbins && dsum) atomicAdd(&segtot[threadIdx.x], dsum);
  }
  __syncthreads();
  if constexpr (kX) sink_count(xs, wn);
  uint32_t* f = fine + static_cast<uint64_t>(blk) * nfine;
  uint32_t fsum = 0;
  for (uint32_t b = threadIdx.x; b < nfine; b += kPartThreads) {
    const uint32_t v = (fc[b >> kFcShift] >> ((b & (kFcPer - 1u)) * kFc)) & kFcMax;
    f[b] = v;
    fsum += v;
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) fsum += __shfl_xor(fsum, d);
  __shared__ uint32_t wsum[kPartThreads / 64];
  if (__lane_id() == 0) wsum[threadIdx.x >> 6] = fsum;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t tsum = 0;
    for (uint32_t w = 0; w < kPartThreads / 64; ++w) tsum += wsum[w];
    if (tsum != acc) *ovf = 1u;  // a counter wrapped (see fc)
  }
}

// Only after a 16-bit counter overflow in k_part_scatter_runs (*ovf): for
// every (coarse block j, segment c) -- a grid-stride loop, so the usual call
// costs one small launch -- recount the records j wrote to segment c
// ([seg[c * P + j], seg[c * P + j + 1])) on the kB2 second-pass digit bits.
template <uint32_t kB2, typename RecT = uint4>
__global__ __launch_bounds__(kPartThreads) void k_fine_recount(const RecT* __restrict__ rec,
                                                                uint32_t skip,
                                                                const uint32_t* __restrict__ seg,
                                                                uint32_t P, uint32_t nseg,
                                                                uint32_t fbits,
                                                                uint32_t* __restrict__ fine,
                                                                const uint32_t* __restrict__ ovf) {
  if (*ovf == 0) return;
  constexpr uint32_t nb = 1u << kB2;
  __shared__ uint32_t cnt[nb];
  for (uint32_t jc = blockIdx.x; jc < P * nseg; jc += gridDim.x) {
    const uint32_t j = jc % P, c = jc / P;
    for (uint32_t b = threadIdx.x; b < nb; b += kPartThreads) cnt[b] = 0;
    __syncthreads();
    const uint32_t s0 = seg[static_cast<uint64_t>(c) * P + j];
    const uint32_t s1 = seg[static_cast<uint64_t>(c) * P + j + 1];
    for (uint32_t i = s0 + threadIdx.x; i < s1; i += kPartThreads) {
      const RecT v = rec[i];
      atomicAdd(&cnt[digit_of((static_cast<uint64_t>(v.y) << 32) | v.x, skip, kB2)], 1u);
    }
    __syncthreads();
    uint32_t* f = fine + static_cast<uint64_t>(j) * (1u << fbits) + (static_cast<uint64_t>(c) << kB2);
    for (uint32_t b = threadIdx.x; b < nb; b += kPartThreads) f[b] = cnt[b];
    __syncthreads();
  }
}

// k_fine_recount for the run layout of k_part_private: the records coarse
// block j wrote to segment c are its runs (j, r, c), r < max_rounds.
template <uint32_t kB2, typename RecT = uint4>
__global__ __launch_bounds__(kPartThreads) void k_fine_recount_runs(
    const RecT* __restrict__ rec, uint32_t skip, const uint32_t* __restrict__ run_start,
    const uint32_t* __restrict__ run_len, uint32_t max_rounds, uint32_t P, uint32_t nseg,
    uint32_t fbits, uint32_t* __restrict__ fine, const uint32_t* __restrict__ ovf) {
  if (*ovf == 0) return;
  constexpr uint32_t nb = 1u << kB2;
  __shared__ uint32_t cnt[nb];
  for (uint32_t jc = blockIdx.x; jc < P * nseg; jc += gridDim.x) {
    const uint32_t j = jc % P, c = jc / P;
    for (uint32_t b = threadIdx.x; b < nb; b += kPartThreads) cnt[b] = 0;
    __syncthreads();
    for (uint32_t r = 0; r < max_rounds; ++r) {
      const uint64_t e = (static_cast<uint64_t>(j) * max_rounds + r) * kRunMaxBins + c;
      const uint32_t s0 = run_start[e], len = run_len[e];
      for (uint32_t i = threadIdx.x; i < len; i += kPartThreads) {
        const RecT v = rec[s0 + i];
        atomicAdd(&cnt[digit_of((static_cast<uint64_t>(v.y) << 32) | v.x, skip, kB2)], 1u);
      }
    }
    __syncthreads();
    uint32_t* f = fine + static_cast<uint64_t>(j) * (1u << fbits) + (static_cast<uint64_t>(c) << kB2);
    for (uint32_t b = threadIdx.x; b < nb; b += kPartThreads) f[b] = cnt[b];
    __syncthreads();
  }
}

// Per final bucket b: E[j][b] = rows of b that coarse blocks [0, kR j) wrote
// (the start of second-pass block j inside bucket b; block j takes coarse
// blocks [kR j, kR (j + 1))) and tot[b] = the bucket's size.  A block covers 64
// buckets x kP2 blocks: thread (bi, jg) sums the fine counts of its kP2 / 16
// second-pass blocks (each wave reads 256 contiguous bytes per load), then the
// 16 partial sums of a bucket are scanned in LDS.  Resets *ovf for the next call.
template <uint32_t kP2, uint32_t kR>
__global__ __launch_bounds__(1024) void k_fine_scan(const uint32_t* __restrict__ fine,
                                                    uint32_t nfine, uint32_t* __restrict__ E,
                                                    uint32_t* __restrict__ tot,
                                                    uint32_t* __restrict__ ovf) {
  static_assert(kP2 % 16 == 0, "second-pass blocks per thread");
  constexpr uint32_t kJ = kP2 / 16;
  __shared__ uint32_t part[16][64];
  const uint32_t bi = threadIdx.x & 63u, jg = threadIdx.x >> 6;
  const uint32_t b = blockIdx.x * 64 + bi;
  if (blockIdx.x == 0 && threadIdx.x == 0) *ovf = 0;
  uint32_t sj[kJ], local = 0;
#pragma unroll
  for (uint32_t k = 0; k < kJ; ++k) {
    const uint64_t j = jg * kJ + k;
    uint32_t v = 0;
#pragma unroll
    for (uint32_t r = 0; r < kR; ++r)
      v += b < nfine ? fine[(j * kR + r) * nfine + b] : 0u;
    sj[k] = v;
    local += v;
  }
  part[jg][bi] = local;
  __syncthreads();
  uint32_t pre = 0, all = 0;
#pragma unroll
  for (uint32_t g = 0; g < 16; ++g) {
    const uint32_t v = part[g][bi];
    pre += g < jg ? v : 0u;
    all += v;
  }
  if (b >= nfine) return;
#pragma unroll
  for (uint32_t k = 0; k < kJ; ++k) {
    E[static_cast<uint64_t>(jg * kJ + k) * nfine + b] = pre;
    pre += sj[k];
  }
  if (jg == 0) tot[b] = all;
}

// Bucket partition with LDS staging (12-bit digits, 2 slots in the product): a
// keyed row is parked in its bucket's kSlots-record LDS slot and leaves with
// the slot's other rows as one kSlots x 16-B run, so the scattered writes are
// kSlots times fewer and wider.  Rows arriving at a full slot are written
// directly.  Rows are taken kRows per thread per round; each round ends with a
// flush of the full slots; partly filled slots go out at the end.
// Two-level use (n > 4096 x kBucketRows): blockIdx.y = segment c of a first,
// coarse pass ([seg[c * P1], seg[(c + 1) * P1]) of its records), the digit is
// the kBits hash bits below the segment's, and the offsets are laid out
// [c][digit][block] -- so the group kernel sees 2^(cbits + kBits) buckets.
constexpr uint32_t kStageBits = 12;
// Second pass of the two-level partition: 9 digit bits, 16-record runs, 4 rows
// per thread per round, 128 blocks per coarse segment (each takes what 2
// coarse blocks wrote to its segment).  Wider runs write fewer partial lines:
// on the staged scatter alone 12/2 0.163 ms, 10/8 0.123 ms
// (profiles/r2/exp_scatter_slots_r2t.log); at 100 M rows the 6 + 9-bit split
// with 16-record runs beat 5 + 10 with 8 (profiles/r2/exp_twolevel_r2E.log).
// Blocks per segment at 100 M rows (scripts/exp_twolevel_s2.hip,
// profiles/r3/exp_twolevel_s2/): 64 -> 128 2.25 -> 2.21 ms, 256 2.40 ms;
// 8-record runs (two blocks per CU) 2.37 ms; 2 or 8 rows per thread slower.
constexpr uint32_t kStage2Bits = 9;
constexpr uint32_t kStage2Slots = 16;
constexpr int kStage2Rows = 4;
constexpr uint32_t kStage2Blocks = 128;
// kRec12: 12-byte records {hash lo, hash hi, row} for rows whose rank is
// rank_base + row (RowsIn without a rank array): a quarter less to write here
// and to read in the group kernel (k_bucket_group12_pk).
template <typename In, bool kInitRep, uint32_t kBits = kStageBits, uint32_t kSlots = 2, int kRows = 2,
          bool kRec12 = false>
__global__ __launch_bounds__(kPartThreads) void k_part_scatter_rec_staged(
    In in, uint64_t n, uint32_t skip, const uint32_t* __restrict__ offs, uint4* __restrict__ rec,
    uint32_t* __restrict__ rep, const uint32_t* __restrict__ seg, uint32_t P1,
    const uint32_t* __restrict__ ftot = nullptr, uint32_t* __restrict__ fbase = nullptr,
    uint32_t R = 1) {
  constexpr uint32_t nbins = 1u << kBits;
  using RecT = typename std::conditional<kRec12, uint3, uint4>::type;
  __shared__ RecT stage[nbins][kSlots];
  RecT* __restrict__ out = reinterpret_cast<RecT*>(rec);
  __shared__ uint32_t fill[nbins];
  __shared__ uint32_t cur[nbins];
  // Fewer buckets than threads (the two-level second pass): the row that
  // fills a bucket's kSlots slots lists the bucket, and the flush writes each
  // listed bucket's run with kSlots ADJACENT lanes, so a store instruction
  // covers 64 / kSlots whole runs.  (Two lanes per bucket, each writing every
  // other record, touched 32 runs per instruction: the store pattern, not the
  // bytes, set the pass's time -- scripts/exp_stores.hip, runs of 2 vs 16:
  // 0.133 vs 0.033 ms for 201 MB.)  full_n by round parity: the count of
  // round r + 1 is cleared during round r's flush, when nothing reads it.
  constexpr bool kCoop = nbins < kPartThreads;
  static_assert(!kCoop || (64 % kSlots == 0 && kPartThreads % kSlots == 0),
                "a bucket's run is written by lanes of one wave");
  // (absent from the 12-bit 16-byte variant, whose stage, fill and cur fill
  // the 160 KiB exactly: referenced only under kCoop)
  __shared__ uint16_t full[kCoop ? nbins : 1];
  __shared__ uint32_t full_n[kCoop ? 2 : 1];
  const uint32_t c = blockIdx.y;
  uint64_t t0 = 0, t1 = 0;
  if (ftot) {
    // offsets from block-major counts (k_fine_scan): offs = E[j][bucket], the
    // rows of each bucket that blocks before j hold; ftot = bucket sizes.
    // Two-level second pass (seg): block j takes what coarse blocks
    // [R j, R (j + 1)) wrote to segment c, whose first record is seg[c P1].
    // One level (no seg): block j takes tile j of the rows.  Bucket starts:
    // segment start + exclusive scan of the segment's bucket sizes, scanned
    // here (kPerT per thread); block 0 of each segment publishes them (fbase,
    // + the total) for the group kernel.
    constexpr uint32_t kPerT = nbins > kPartThreads ? nbins / kPartThreads : 1u;
    static_assert(nbins <= kPartThreads || nbins % kPartThreads == 0, "buckets per thread");
    uint32_t* wsum = fill;  // scratch for the 16 wave sums (LDS is full)
    const uint32_t j = part_block(), t = threadIdx.x, lane = __lane_id();
    const uint64_t nfine = static_cast<uint64_t>(gridDim.y) << kBits, b0 = static_cast<uint64_t>(c) << kBits;
    // every prologue load issued up front (clamped, selected at use): the
    // bucket sizes, this block's starts inside them and the segment bounds
    uint32_t v[kPerT], ov[kPerT], sum = 0;
#pragma unroll
    for (uint32_t k = 0; k < kPerT; ++k) {
      const uint32_t b = min(t * kPerT + k, nbins - 1);
      v[k] = ftot[b0 + b];
      ov[k] = offs[j * nfine + b0 + b];
    }
    uint32_t seg_c = 0, seg_t0 = 0, seg_t1 = 0, seg_end = 0;
    if (seg) {
      seg_c = seg[static_cast<uint64_t>(c) * P1];
      seg_t0 = seg[static_cast<uint64_t>(c) * P1 + min(P1, R * j)];
      seg_t1 = seg[static_cast<uint64_t>(c) * P1 + min(P1, R * (j + 1))];
      seg_end = seg[static_cast<uint64_t>(gridDim.y) * P1];
    }
#pragma unroll
    for (uint32_t k = 0; k < kPerT; ++k) {
      if (t * kPerT + k >= nbins) v[k] = 0u;
      sum += v[k];
    }
    uint32_t inc = sum;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t o = __shfl_up(inc, d);
      if (lane >= static_cast<uint32_t>(d)) inc += o;
    }
    if (lane == 63) wsum[t >> 6] = inc;
    __syncthreads();
    uint32_t base = seg_c + inc - sum, total = 0;
    for (uint32_t w = 0; w < kPartThreads / 64; ++w) {
      if (w < (t >> 6)) base += wsum[w];
      total += wsum[w];
    }
    __syncthreads();  // wsum (= fill) is cleared below
#pragma unroll
    for (uint32_t k = 0; k < kPerT; ++k) {
      const uint32_t b = t * kPerT + k;
      if (b < nbins) {
        cur[b] = base + ov[k];
        fill[b] = 0;
        if (j == 0) fbase[b0 + b] = base;
      }
      base += v[k];
    }
    if (j == 0 && c == gridDim.y - 1 && t == 0)
      fbase[nfine] = seg ? seg_end : total;
    if (seg) {
      t0 = seg_t0;
      t1 = seg_t1;
    } else {
      tile_of(n, gridDim.x, t0, t1);
    }
  } else {
    const uint64_t obase = static_cast<uint64_t>(c) * nbins * gridDim.x;
    for (uint32_t b = threadIdx.x; b < nbins; b += kPartThreads) {
      cur[b] = offs[obase + static_cast<uint64_t>(b) * gridDim.x + part_block()];
      fill[b] = 0;
    }
  }
  if constexpr (kCoop)
    if (threadIdx.x == 0) full_n[0] = full_n[1] = 0;
  __syncthreads();
  if (ftot) {
    // tile set above
  } else if (seg) {
    const uint64_t s0 = seg[static_cast<uint64_t>(c) * P1], s1 = seg[static_cast<uint64_t>(c + 1) * P1];
    tile_of(s1 - s0, gridDim.x, t0, t1);
    t0 += s0;
    t1 += s0;
  } else {
    tile_of(n, gridDim.x, t0, t1);
  }
  constexpr int U = kRows;
  constexpr uint64_t kStep = static_cast<uint64_t>(U) * kPartThreads;
  // one round: stage (or write) the batch's rows, then flush the full slots.
  // The round barriers wait for LDS only (lds_barrier), so the next round's
  // loads and this round's record stores stay in flight across them.
  auto round = [&](const RowBatch<U>& q, uint64_t i0, uint32_t par) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint64_t i = i0 + threadIdx.x + static_cast<uint64_t>(u) * kPartThreads;
      if (!q.in[u]) continue;
      const uint32_t r = in.rank_of(q, u);
      if (kInitRep) rep[i] = r;
      if (!in.valid_of(q, u)) continue;
      const uint64_t h = in_hash<In>(in.key_of(q, u));
      const uint32_t b = digit_of(h, skip, kBits);
      RecT rq;
      if constexpr (kRec12)
        rq = make_uint3(static_cast<uint32_t>(h), static_cast<uint32_t>(h >> 32), in.row_of(q, u));
      else
        rq = make_uint4(static_cast<uint32_t>(h), static_cast<uint32_t>(h >> 32), r, in.row_of(q, u));
      const uint32_t sl = atomicAdd(&fill[b], 1u);
      if (sl < kSlots) {
        stage[b][sl] = rq;
        if constexpr (kCoop)
          if (sl == kSlots - 1)
            full[atomicAdd(&full_n[par & (kCoop ? 1u : 0u)], 1u)] = static_cast<uint16_t>(b);
      } else {
        out[atomicAdd(&cur[b], 1u)] = rq;
      }
    }
    lds_barrier();
    // unrolled, not a loop: the compiler drains every load in flight before a
    // store-only loop that reads registers loaded outside it (vmcnt(0))
    if constexpr (nbins >= kPartThreads) {
      static_assert(nbins % kPartThreads == 0, "flush slots per thread");
#pragma unroll
      for (uint32_t j = 0; j < nbins / kPartThreads; ++j) {
        const uint32_t b = threadIdx.x + j * kPartThreads;
        if (fill[b] >= kSlots) {
          const uint32_t p = cur[b];
          cur[b] = p + kSlots;
#pragma unroll
          for (uint32_t k = 0; k < kSlots; ++k) out[p + k] = stage[b][k];
          fill[b] = 0;
        }
      }
    } else {
      // lane group x / kSlots writes listed bucket e's record x % kSlots; the
      // group's lanes read cur[b] in the same instruction, before its first
      // lane advances it
      const uint32_t nf = full_n[par & (kCoop ? 1u : 0u)];
      if (threadIdx.x == 0) full_n[(par ^ 1u) & (kCoop ? 1u : 0u)] = 0;
      for (uint32_t x = threadIdx.x; x < nf * kSlots; x += kPartThreads) {
        const uint32_t e = x / kSlots, k = x % kSlots;
        const uint32_t b = full[e];
        const uint32_t p = cur[b];
        out[p + k] = stage[b][k];
        if (k == 0) {
          cur[b] = p + kSlots;
          fill[b] = 0;
        }
      }
    }
    lds_barrier();
  };
  // Software pipeline: round r + 1's rows are loaded while round r is staged
  // and flushed.  Two batches in ping-pong (a register copy between rounds
  // would wait for the loads just issued), and the prefetches unconditional
  // (past the tile they re-read row t0) so that the compiler's wait counts need
  // not cover a path without them.
  if (t0 < t1) {
    RowBatch<U> qa, qb;
    in.template load_many<U>(t0 + threadIdx.x, kPartThreads, t1, t0, qa);
    for (uint64_t i0 = t0;; i0 += 2 * kStep) {  // uniform trip count
      in.template load_many<U>(i0 + kStep + threadIdx.x, kPartThreads, t1, t0, qb);
      round(qa, i0, 0u);
      if (i0 + kStep >= t1) break;
      in.template load_many<U>(i0 + 2 * kStep + threadIdx.x, kPartThreads, t1, t0, qa);
      round(qb, i0 + kStep, 1u);
      if (i0 + 2 * kStep >= t1) break;
    }
  }
  // the slots' remainders, kSlots adjacent lanes per bucket (as k_part2_runs)
  for (uint32_t x = threadIdx.x; x < nbins * kSlots; x += kPartThreads) {
    const uint32_t b = x / kSlots, k = x % kSlots;
    if (k < fill[b]) out[cur[b] + k] = stage[b][k];
  }
}

// Second pass of the two-level partition over k_part_private's runs: block
// (j, c) takes the runs coarse blocks [R j, R (j + 1)) wrote for segment c --
// up to kMaxRuns (block, round) runs, listed with their exclusive prefix in LDS
// -- and stages their records exactly as k_part_scatter_rec_staged's second
// pass does (kS2-record slots, listed full buckets flushed by adjacent lanes).
// Record k of the block's virtual range is found by a 9-step binary search
// of the run prefix.  Segment starts from segtot (sizes summed by the first
// pass); bucket starts from the fine scan's sizes as before.  kF: a bucket is
// listed for the round-end flush once it holds kF records (kF = kS2: full
// buckets only).  Flushing from 8 or 12 staged records cuts the arrivals that
// meet a full slot array (single-record stores, ~20 % of records at kF = 16)
// but measured slower at 100 M rows (2.02 ms at 16, 2.06 at 12, 2.10 at 8,
// profiles/r3/exp_twolevel_s2/run_r3I.log): a block's stores into one bucket
// fill one contiguous range, so the L2 merges the single stores anyway.
constexpr uint32_t kMaxRuns = 512;  // R x rounds (host: group_layout picks the path)
template <bool kRec12, uint32_t kB2, uint32_t kS2, int kRows, uint32_t kF = kS2>
__global__ __launch_bounds__(kPartThreads) void k_part2_runs(
    const uint4* __restrict__ rec1, uint32_t skip, const uint32_t* __restrict__ offs,
    uint4* __restrict__ rec, const uint32_t* __restrict__ run_start,
    const uint32_t* __restrict__ run_len, uint32_t max_rounds, uint32_t P1, uint32_t R,
    const uint32_t* __restrict__ segtot, const uint32_t* __restrict__ ftot,
    uint32_t* __restrict__ fbase) {
  constexpr uint32_t nbins = 1u << kB2;
  using RecT = typename std::conditional<kRec12, uint3, uint4>::type;
  static_assert(nbins < kPartThreads && 64 % kS2 == 0 && kPartThreads % kS2 == 0,
                "listed buckets flushed by adjacent lanes of one wave");
  static_assert(kF >= 1 && kF <= kS2, "flush threshold within the slots");
  static_assert(kMaxRuns < kPartThreads, "one run per thread in the prologue");
  __shared__ RecT stage[nbins][kS2];
  __shared__ uint32_t fill[nbins], cur[nbins];
  __shared__ uint16_t full[nbins];
  __shared__ uint32_t full_n[2];
  __shared__ uint32_t rpre[kMaxRuns + 1], rst[kMaxRuns];
  __shared__ uint32_t wsum[kPartThreads / 64], wsumb[kPartThreads / 64];
  __shared__ uint32_t s_segbase, s_all;
  const RecT* __restrict__ in = reinterpret_cast<const RecT*>(rec1);
  RecT* __restrict__ out = reinterpret_cast<RecT*>(rec);
  const uint32_t c = blockIdx.y, j = part_block(), t = threadIdx.x, lane = __lane_id();
  const uint32_t nseg = gridDim.y;
  const uint64_t nfine = static_cast<uint64_t>(nseg) << kB2, b0 = static_cast<uint64_t>(c) << kB2;
  const uint32_t nr = R * max_rounds;
  // Every prologue load is issued here, up front and unconditionally (clamped
  // indices, values selected at use): their addresses are independent, so the
  // block waits out ONE memory latency instead of four in a row (a block's
  // prologue overlaps nothing else: one block per CU).
  const uint32_t seg_v = segtot[min(t, nseg - 1)];
  const uint32_t tr = min(t, nr - 1), cb = R * j + tr / max_rounds, rr = tr % max_rounds;
  const uint64_t e = (static_cast<uint64_t>(min(cb, P1 - 1)) * max_rounds + rr) * kRunMaxBins + c;
  const uint32_t len_v = run_len[e], st_v = run_start[e];
  const uint32_t tb = min(t, nbins - 1);
  const uint32_t ft_v = ftot[b0 + tb];
  const uint32_t off_v = offs[static_cast<uint64_t>(j) * nfine + b0 + tb];
  if (t < 64) {  // this segment's start and the total, from the (<= 64) segment sizes
    const uint32_t v = t < nseg ? seg_v : 0u;
    uint32_t inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t o = __shfl_up(inc, d);
      if (lane >= static_cast<uint32_t>(d)) inc += o;
    }
    if (t == c) s_segbase = inc - v;
    if (t == 63) s_all = inc;
  }
  {  // the block's runs (prefix of their lengths) and its bucket starts
     // (segment start + the segment's bucket sizes scanned): both block
     // scans share their barriers (two, not four: a block lives ~2 rounds)
    static_assert(nbins <= kPartThreads, "one bucket per thread");
    const bool has = t < nr && cb < P1;
    const uint32_t len = has ? len_v : 0u, st = has ? st_v : 0u;
    const uint32_t v = t < nbins ? ft_v : 0u;
    uint32_t inc = len, incb = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t o = __shfl_up(inc, d), ob = __shfl_up(incb, d);
      if (lane >= static_cast<uint32_t>(d)) {
        inc += o;
        incb += ob;
      }
    }
    if (lane == 63) {
      wsum[t >> 6] = inc;
      wsumb[t >> 6] = incb;
    }
    __syncthreads();  // wsum, wsumb; s_segbase / s_segend / s_all (wave 0 above)
    uint32_t before = 0, base = s_segbase + incb - v;
    for (uint32_t w = 0; w < (t >> 6); ++w) {
      before += wsum[w];
      base += wsumb[w];
    }
    if (t <= kMaxRuns) rpre[t] = before + inc - len;  // rpre[kMaxRuns] = the block's total
    if (t < kMaxRuns) rst[t] = st;
    if (t < nbins) {
      cur[t] = base + off_v;
      fill[t] = 0;
      if (j == 0) fbase[b0 + t] = base;
    }
    if (j == 0 && c == nseg - 1 && t == 0) fbase[nfine] = s_all;
    if (t == 0) full_n[0] = full_n[1] = 0;
  }
  __syncthreads();
  const uint32_t T = rpre[kMaxRuns];
  constexpr uint32_t kStep = static_cast<uint32_t>(kRows) * kPartThreads;
  // record k of the block's runs (k < T): the run whose prefix is the last <= k
  auto src_of = [&](uint32_t k) {
    uint32_t pos = 0;
#pragma unroll
    for (uint32_t s = kMaxRuns / 2; s >= 1; s >>= 1)
      if (rpre[pos + s] <= k) pos += s;
    return rst[pos] + (k - rpre[pos]);
  };
  struct Batch {
    RecT v[kRows];
  };
  auto load = [&](uint32_t k0, Batch& q) {
    uint32_t s[kRows];
#pragma unroll
    for (int u = 0; u < kRows; ++u) s[u] = src_of(min(k0 + t + u * kPartThreads, T - 1));
#pragma unroll
    for (int u = 0; u < kRows; ++u) q.v[u] = in[s[u]];
  };
  auto round = [&](const Batch& q, uint32_t k0, uint32_t par) {
#pragma unroll
    for (int u = 0; u < kRows; ++u) {
      if (k0 + t + u * kPartThreads >= T) continue;
      const RecT rq = q.v[u];
      const uint32_t b = digit_of((static_cast<uint64_t>(rq.y) << 32) | rq.x, skip, kB2);
      const uint32_t sl = atomicAdd(&fill[b], 1u);
      if (sl < kS2) {
        stage[b][sl] = rq;
        if (sl == kF - 1) full[atomicAdd(&full_n[par], 1u)] = static_cast<uint16_t>(b);
      } else {
        out[atomicAdd(&cur[b], 1u)] = rq;
      }
    }
    lds_barrier();
    const uint32_t nf = full_n[par];
    if (t == 0) full_n[par ^ 1u] = 0;
    for (uint32_t x = t; x < nf * kS2; x += kPartThreads) {
      const uint32_t e = x / kS2, k = x % kS2;
      const uint32_t b = full[e];
      const uint32_t p = cur[b], len = min(fill[b], kS2);
      if (k < len) out[p + k] = stage[b][k];
      if (k == 0) {
        cur[b] = p + len;
        fill[b] = 0;
      }
    }
    lds_barrier();
  };
  if (T > 0) {  // the next round's records are loaded during the current one
    Batch qa, qb;
    load(0, qa);
    for (uint32_t k0 = 0;; k0 += 2 * kStep) {  // uniform trip count
      load(k0 + kStep, qb);
      round(qa, k0, 0u);
      if (k0 + kStep >= T) break;
      load(k0 + 2 * kStep, qa);
      round(qb, k0 + kStep, 1u);
      if (k0 + 2 * kStep >= T) break;
    }
  }
  // what is left in the slots (< kS2 per bucket, ~40 % of a block's records
  // at 100 M rows): kS2 adjacent lanes per bucket, so a store instruction
  // writes a few short runs instead of one record in each of 64 buckets
  for (uint32_t x = t; x < nbins * kS2; x += kPartThreads) {
    const uint32_t b = x / kS2, k = x % kS2;
    if (k < fill[b]) out[cur[b] + k] = stage[b][k];
  }
}

// The 12-bit staged scatter of rows in rank order (RowsIn without a rank
// array: 12-byte records, rank = rank_base + row), WARP-SPECIALISED.  Waves
// 0-7 only load and stage: their rows are prefetched two rounds ahead and they
// never store, so the compiler's waits before a round cover their loads only
// (in k_part_scatter_rec_staged the conditional record stores sit between a
// round's prefetch and its use, and the waits there drain them too).  Waves
// 8-15 only store: the full slot pairs, the rows that met a full slot (an LDS
// overflow list, kept in arrival order per bucket by an LDS cursor) and, with
// kInitRep, rep = rank of the round's rows (computed, nothing loaded).  Two
// barriers per round: staged (A), flushed (B) -- the bucket cursors advance
// atomically and the overflow count alternates by round parity, so the
// barrier between the pair flush and the overflow rows (round 3-4's M) is
// gone.
// scripts/exp_scatter_align.hip: 12.5 M rows 0.136 -> 0.123 ms
// (profiles/r3/exp_scatter_align/run.log).
constexpr uint32_t kWsProd = 512;   // producer threads (waves 0-7)
constexpr int kWsRows = 4;          // rows per producer thread per round
// In: the caller's rows (RowsIn, rank = rank_base + row) or received exchange
// records (RecRankIn: the rank in the record's third word).
template <typename In, bool kInitRep>
__global__ __launch_bounds__(kPartThreads) void k_part_scatter_ws(
    In in, uint64_t n, uint32_t skip, const uint32_t* __restrict__ offs,
    const uint32_t* __restrict__ ftot, uint3* __restrict__ out, uint32_t* __restrict__ rep,
    uint32_t* __restrict__ fbase) {
  constexpr uint32_t nbins = 1u << kStageBits;
  constexpr uint32_t kRound = kWsProd * kWsRows;  // 2048 rows
  static_assert(2 * kWsProd == kPartThreads, "half producers, half consumers");
  __shared__ uint3 stage[nbins][2];
  __shared__ uint32_t fill[nbins], cur[nbins];
  __shared__ uint3 ovf[kRound];
  __shared__ uint32_t ovf_n[2];  // by round parity (no barrier to reset it)
  // bucket starts: the segment's sizes scanned here, block 0 publishes them
  constexpr uint32_t kPerT = nbins / kPartThreads;
  const uint32_t t = threadIdx.x, lane = __lane_id();
  const uint32_t j = part_block();
  // the block's starts inside its buckets loaded with the bucket sizes (one
  // memory latency for both, not one after the other around the scan)
  uint32_t v[kPerT], ov[kPerT], sum = 0;
#pragma unroll
  for (uint32_t k = 0; k < kPerT; ++k) {
    v[k] = ftot[t * kPerT + k];
    ov[k] = offs[static_cast<uint64_t>(j) * nbins + t * kPerT + k];
  }
#pragma unroll
  for (uint32_t k = 0; k < kPerT; ++k) sum += v[k];
  uint32_t inc = sum;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t o = __shfl_up(inc, d);
    if (lane >= static_cast<uint32_t>(d)) inc += o;
  }
  if (lane == 63) fill[t >> 6] = inc;
  __syncthreads();
  uint32_t base = inc - sum, total = 0;
  for (uint32_t w = 0; w < kPartThreads / 64; ++w) {
    if (w < (t >> 6)) base += fill[w];
    total += fill[w];
  }
  __syncthreads();
#pragma unroll
  for (uint32_t k = 0; k < kPerT; ++k) {
    const uint32_t b = t * kPerT + k;
    cur[b] = base + ov[k];
    fill[b] = 0;
    if (j == 0) fbase[b] = base;
    base += v[k];
  }
  if (j == 0 && t == 0) fbase[nbins] = total;
  if (t < 2) ovf_n[t] = 0;
  __syncthreads();
  uint64_t t0, t1;
  tile_of(n, gridDim.x, t0, t1);
  const uint32_t rounds = t1 > t0 ? static_cast<uint32_t>((t1 - t0 + kRound - 1) / kRound) : 0u;
  if (t < kWsProd) {
    RowBatch<kWsRows> qa, qb;
    in.template load_many<kWsRows>(t0 + t, kWsProd, t1, t0, qa);
    in.template load_many<kWsRows>(t0 + kRound + t, kWsProd, t1, t0, qb);
    auto stage_round = [&](const RowBatch<kWsRows>& q, uint32_t par) {
#pragma unroll
      for (int u = 0; u < kWsRows; ++u) {
        if (!in.valid_of(q, u)) continue;
        const uint64_t h = in_hash<In>(in.key_of(q, u));
        const uint32_t b = digit_of(h, skip, kStageBits);
        const uint3 rq = make_uint3(static_cast<uint32_t>(h), static_cast<uint32_t>(h >> 32),
                                    in.row_of(q, u));
        const uint32_t sl = atomicAdd(&fill[b], 1u);
        if (sl < 2)
          stage[b][sl] = rq;
        else
          ovf[atomicAdd(&ovf_n[par], 1u)] = rq;
      }
    };
    // per round exactly the consumers' two barriers (A, B); the loads of
    // round r + 2 go out between A and B, while the consumers store
    for (uint32_t r = 0; r < rounds; r += 2) {
      stage_round(qa, 0u);
      lds_barrier();  // A
      in.template load_many<kWsRows>(t0 + (r + 2) * static_cast<uint64_t>(kRound) + t, kWsProd, t1,
                                     t0, qa);
      lds_barrier();  // B
      if (r + 1 >= rounds) break;
      stage_round(qb, 1u);
      lds_barrier();  // A
      in.template load_many<kWsRows>(t0 + (r + 3) * static_cast<uint64_t>(kRound) + t, kWsProd, t1,
                                     t0, qb);
      lds_barrier();  // B
    }
  } else {
    const uint32_t c = t - kWsProd;
    for (uint32_t r = 0; r < rounds; ++r) {
      lds_barrier();  // A
      if constexpr (kInitRep) {
        // every row starts as its own Object: rows without a key stay so
        // (mod.rs:238-239); K5 overwrites only the rows that link
        const uint64_t r0 = t0 + static_cast<uint64_t>(r) * kRound;
#pragma unroll
        for (uint32_t u = 0; u < kRound / kWsProd; ++u) {
          const uint64_t i = r0 + c + u * kWsProd;
          if (i < t1) rep[i] = in.rank_base + static_cast<uint32_t>(i);
        }
      }
#pragma unroll
      for (uint32_t k = 0; k < nbins / kWsProd; ++k) {
        const uint32_t b = c + k * kWsProd;
        if (fill[b] >= 2) {
          // an atomic cursor: the overflow rows below advance it too, with
          // no barrier between (a pair and an overflow row of one bucket may
          // take either order; every position is taken once)
          const uint32_t p = atomicAdd(&cur[b], 2u);
          out[p] = stage[b][0];
          out[p + 1] = stage[b][1];
          fill[b] = 0;
        }
      }
      const uint32_t par = r & 1u, no = ovf_n[par];
      if (c == 0) ovf_n[par ^ 1u] = 0;  // last round's, read by every consumer before its B
      for (uint32_t o = c; o < no; o += kWsProd) {
        const uint3 rq = ovf[o];
        out[atomicAdd(&cur[digit_of((static_cast<uint64_t>(rq.y) << 32) | rq.x, skip, kStageBits)],
                      1u)] = rq;
      }
      lds_barrier();  // B
    }
  }
  __syncthreads();
  for (uint32_t b = threadIdx.x; b < nbins; b += kPartThreads)
    for (uint32_t k = 0; k < fill[b]; ++k) out[cur[b] + k] = stage[b][k];
}

// the segment sizes k_part_private adds to, and the fine-count overflow flag
__global__ void k_zero_runs(uint32_t* __restrict__ segtot, uint32_t* __restrict__ ovf) {
  if (threadIdx.x < kRunMaxBins) segtot[threadIdx.x] = 0;
  if (threadIdx.x == 0) *ovf = 0;
}

}  // namespace
}  // namespace sdgpu
