// K6 radix partition, the part shared by the grouping (dedup.hip) and the
// multi-GPU exchange (exchange.hip): the partition constants, digits, tiles
// and block numbering, the keyless sink's device side, and the histogram
// kernel.  Internal linkage: each translation unit gets its own kernels.
#pragma once

#include <type_traits>

#include "internal.hpp"
#include "rows_device.hpp"

namespace sdgpu {
namespace {

constexpr int kPartThreads = 1024;
// Blocks of a partition: one per CU.  Each block keeps one open output line
// per bucket, so the blocks resident on one XCD hold blocks/8 x buckets x
// 128 B of partially written lines in its 4 MB L2.
constexpr uint32_t kPartBlocks = 256;
constexpr uint32_t kMaxPartBlocks = 1024;  // bucket partition: sizes the workspace

// `bits` hash bits below the top `skip` bits of h.
__device__ __forceinline__ uint32_t digit_of(uint64_t h, uint32_t skip, uint32_t bits) {
  return bits == 0 ? 0u : static_cast<uint32_t>((h << skip) >> (64u - bits));
}

// XCD-aware block numbering: workgroups are dispatched round-robin over the 8
// XCDs, so physical block i runs on XCD i % 8.  Logical block (i % 8) * P/8 +
// i / 8 gives each XCD a contiguous run of logical blocks; the 16 per-block
// counters of one digit that share a 64-B line of the digit-major histogram
// (and the offsets the scatter reads back) then come from one XCD's L2.
__device__ __forceinline__ uint32_t part_block() {
  const uint32_t P = gridDim.x;
  return (P & 7u) ? blockIdx.x : (blockIdx.x & 7u) * (P >> 3) + (blockIdx.x >> 3);
}

__device__ __forceinline__ void tile_of(uint64_t n, uint32_t P, uint64_t& t0, uint64_t& t1) {
  const uint64_t per = (n + P - 1) / P;
  t0 = min<uint64_t>(n, per * part_block());
  t1 = min<uint64_t>(n, t0 + per);
}

// Rows per thread per step of the partition kernels: the loads of a step are
// issued back to back, so one tile costs a few memory latencies, not one per row.
constexpr int kUnroll = 8;

// Workgroup barrier for LDS hand-offs only: waits for this wave's LDS
// operations, not for its global loads and stores (__syncthreads' release
// fence waits for all of them: vmcnt(0) before every round barrier).  The
// "memory" clobber keeps the compiler from moving memory accesses across it.
__device__ __forceinline__ void lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// Partition digit of a row hash: the destination rank of the multi-GPU
// exchange when world != 0 (shard s = top `bits` hash bits belongs to rank
// s * world >> bits), else `bits` hash bits below the top `skip` bits.
__device__ __forceinline__ uint32_t part_digit(uint64_t h, uint32_t skip, uint32_t bits,
                                               uint32_t world) {
  return world ? static_cast<uint32_t>(((h >> (64 - bits)) * world) >> bits)
               : digit_of(h, skip, bits);
}

// Wave-aggregated LDS counter add for few, heavily shared bins (the exchange's
// W destination ranks): one atomic per distinct digit in the wave instead of
// one per row.  Every active lane of the wave must call it (v = row counts;
// digits d < 2^nbits); returns the row's slot (base of its bin + its rank
// among the wave's lanes with the same digit).  The lanes sharing a digit
// come from nbits ballots, one per digit bit, and the groups' atomics issue
// together (round 5: a loop over the distinct digits took up to W dependent
// atomic round trips per row step).
__device__ __forceinline__ uint32_t wave_add(uint32_t* cnt, uint32_t d, bool v, uint32_t nbits) {
  const uint32_t lane = __lane_id();
  uint64_t peers = __ballot(v);
  for (uint32_t k = 0; k < nbits; ++k) {  // wave-uniform
    const bool bit = (d >> k) & 1u;
    const uint64_t mk = __ballot(bit);
    peers &= bit ? mk : ~mk;
  }
  const uint32_t rank = static_cast<uint32_t>(__popcll(peers & ((1ull << lane) - 1ull)));
  uint32_t base = 0;
  if (v && rank == 0) base = atomicAdd(&cnt[d], static_cast<uint32_t>(__popcll(peers)));
  const int leader = __ffsll(static_cast<unsigned long long>(peers)) - 1;
  base = __shfl(base, v ? leader : static_cast<int>(lane));
  return v ? base + rank : 0u;
}
// digit bits of bins 0 .. world - 1
__device__ __forceinline__ uint32_t world_bits(uint32_t world) {
  return world > 1 ? 32u - static_cast<uint32_t>(__clz(world - 1)) : 0u;
}

// The valid keyless rows of a fused grouping call (ListOut without an Object
// index; mod.rs:238-239: each is its own Object), collected by the FIRST
// partition pass that already reads every row's has_key.  Each WAVE appends the
// ranks of its keyless rows with valid[i] != 0 (valid null: all) to its own
// segment st[(block * 16 + wave) * cap, ...), counting them in a register (a
// ballot per test, no LDS atomic and no barrier), and stores the count in
// cnt[block * 16 + wave]; k_list_finish moves them behind the keyed entries.
// This replaced a separate pass over has_key / valid (three launches, 0.062 ms
// at 100 M rows, 0.017 ms at 12.5 M).  The segments: KeylessSink, internal.hpp.
constexpr uint32_t kSinkWaves = kPartThreads / 64;

// Called by every lane of a wave that is still in the partition's row loop
// (the lanes that left it never return to it, so the active lanes' `wn`
// agree, and lane 0 -- the last to leave -- holds the wave's count);
// `keyless`: row i is in range with has_key == 0.  kImplicit: in.rank is
// null (rank = rank_base + row; no load).  Segment offsets fit 32 bits (n <
// 2^31, 16 x 256 segments of a 16th of a tile + 520 rows).
template <bool kImplicit = false>
__device__ __forceinline__ void sink_keyless(const KeylessSink& x, const RowsIn& in, bool keyless,
                                             uint64_t i, uint32_t& wn) {
  const bool e = keyless && (!x.valid || x.valid[i] != 0);
  const uint64_t b = __ballot(e);
  if (!b) return;
  if (e) {
    const uint32_t seg = part_block() * kSinkWaves + (threadIdx.x >> 6);
    const uint32_t r = in.rank_base + static_cast<uint32_t>(i);
    x.st[seg * x.cap + wn + __popcll(b & ((1ull << __lane_id()) - 1ull))] =
        kImplicit ? r : (in.rank ? in.rank[i] : r);
  }
  wn += static_cast<uint32_t>(__popcll(b));
}
__device__ __forceinline__ void sink_count(const KeylessSink& x, uint32_t wn) {
  if (__lane_id() == 0) x.cnt[part_block() * kSinkWaves + (threadIdx.x >> 6)] = wn;
}

template <typename In, bool kX = false>
__global__ __launch_bounds__(kPartThreads) void k_part_hist(In in, uint64_t n, uint32_t skip,
                                                            uint32_t bits, uint32_t world,
                                                            uint32_t* __restrict__ hist,
                                                            uint32_t* __restrict__ zero = nullptr,
                                                            bool blk_major = false,
                                                            KeylessSink xs = KeylessSink{}) {
  extern __shared__ __attribute__((aligned(16))) uint32_t cnt[];
  uint32_t wn = 0;  // the wave's keyless rows (KeylessSink)
  const uint32_t nbins = world ? world : 1u << bits;
  if (zero && blockIdx.x == 0 && threadIdx.x == 0) *zero = 0;  // a flag of the next kernels
  for (uint32_t b = threadIdx.x; b < nbins; b += kPartThreads) cnt[b] = 0;
  __syncthreads();
  auto sink_done = [&]() {
    if constexpr (kX) sink_count(xs, wn);
  };
  uint64_t t0, t1;
  tile_of(n, gridDim.x, t0, t1);
  if constexpr (std::is_same<In, RowsIn>::value) {
    // Row order does not matter to a histogram: the keys of row pairs as one
    // 16-B load per lane (8-B loads run at ~0.6x the 16-B rate), has_key as
    // one 2-B load; the odd rows at the tile's ends one by one.
    if (!world && (reinterpret_cast<uintptr_t>(in.key) & 15u) == 0 &&
        (reinterpret_cast<uintptr_t>(in.valid) & 1u) == 0) {
      auto count = [&](uint64_t k, bool v) {
        if (v) atomicAdd(&cnt[part_digit(row_hash(k), skip, bits, 0)], 1u);
      };
      const uint64_t p0 = (t0 + 1) / 2, p1 = t1 / 2;  // whole pairs: rows [2 p0, 2 p1)
      const bool e0 = (t0 & 1u) && t0 < t1, e1 = (t1 & 1u) && t1 - 1 >= 2 * p0;
      if (threadIdx.x == 0 && e0) count(in.key[t0], !in.valid || in.valid[t0]);
      if (threadIdx.x == 1 && e1) count(in.key[t1 - 1], !in.valid || in.valid[t1 - 1]);
      if constexpr (kX) {
        if (threadIdx.x < 64) {  // the whole wave 0 (its ballots)
          sink_keyless(xs, in, threadIdx.x == 0 && e0 && !in.valid[t0], t0, wn);
          sink_keyless(xs, in, threadIdx.x == 1 && e1 && !in.valid[t1 - 1], t1 - 1, wn);
        }
      }
      const uint4* __restrict__ k4 = reinterpret_cast<const uint4*>(in.key);
      const uint16_t* __restrict__ v2 = reinterpret_cast<const uint16_t*>(in.valid);
      constexpr int kP = kUnroll / 2;
      for (uint64_t q0 = p0 + threadIdx.x; q0 < p1; q0 += kP * kPartThreads) {
        uint4 kk[kP];
        uint32_t vv[kP];
#pragma unroll
        for (int u = 0; u < kP; ++u) {
          const uint64_t q = q0 + static_cast<uint64_t>(u) * kPartThreads;
          kk[u] = k4[q < p1 ? q : q0];
          vv[u] = v2 ? v2[q < p1 ? q : q0] : 0x0101u;
        }
#pragma unroll
        for (int u = 0; u < kP; ++u) {
          const uint64_t q = q0 + static_cast<uint64_t>(u) * kPartThreads;
          if (q >= p1) continue;
          count((static_cast<uint64_t>(kk[u].y) << 32) | kk[u].x, (vv[u] & 0xFFu) != 0);
          count((static_cast<uint64_t>(kk[u].w) << 32) | kk[u].z, (vv[u] >> 8) != 0);
        }
        if constexpr (kX) {  // keyless rows are rare: bit 2 u + h = row 2 q_u + h
          uint32_t km = 0;
#pragma unroll
          for (int u = 0; u < kP; ++u)
            if (q0 + static_cast<uint64_t>(u) * kPartThreads < p1)
              km |= (static_cast<uint32_t>((vv[u] & 0xFFu) == 0) |
                     (static_cast<uint32_t>((vv[u] & 0xFF00u) == 0) << 1)) << (2 * u);
          // one pass per bit position some lane has (usually none, else one)
          for (uint64_t b = __ballot(km != 0); b; b = __ballot(km != 0)) {
            const uint32_t p = __ffs(__shfl(km, __ffsll(static_cast<unsigned long long>(b)) - 1)) - 1;
            const uint64_t q = q0 + static_cast<uint64_t>(p >> 1) * kPartThreads;
            sink_keyless(xs, in, (km >> p) & 1u, 2 * q + (p & 1u), wn);
            km &= ~(1u << p);
          }
        }
      }
      __syncthreads();
      for (uint32_t b = threadIdx.x; b < nbins; b += kPartThreads)
        hist[blk_major ? static_cast<uint64_t>(part_block()) * nbins + b
                       : static_cast<uint64_t>(b) * gridDim.x + part_block()] = cnt[b];
      sink_done();
      return;
    }
  }
  for (uint64_t i0 = t0 + threadIdx.x; i0 < t1; i0 += kUnroll * kPartThreads) {
    RowBatch<kUnroll> q;
    in.template load_many<kUnroll>(i0, kPartThreads, t1, i0, q);
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const bool v = in.valid_of(q, u);
      const uint64_t k = in.key_of(q, u);
      if constexpr (kX) sink_keyless(xs, in, q.in[u] && !v, q.row[u], wn);
      if (world) {
        (void)wave_add(cnt, v ? part_digit(in_hash<In>(k), skip, bits, world) : 0u, v, world_bits(world));
      } else if (v) {
        atomicAdd(&cnt[part_digit(in_hash<In>(k), skip, bits, world)], 1u);
      }
    }
  }
  __syncthreads();
  // digit-major [digit][block] for scan::exclusive, or block-major (one
  // coalesced row per block) for k_fine_scan
  for (uint32_t b = threadIdx.x; b < nbins; b += kPartThreads)
    hist[blk_major ? static_cast<uint64_t>(part_block()) * nbins + b
                   : static_cast<uint64_t>(b) * gridDim.x + part_block()] = cnt[b];
  sink_done();
}

inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// Rows per KeylessSink wave segment: at least the rows one wave of a first-pass
// block reads -- a 16th of the block's tile plus one step of rows
// (k_part_private: 256 per round; k_part_hist: 512 per step, +2 edge rows).
uint32_t sink_cap(uint64_t n) {
  const uint64_t tile = (n + kPartBlocks - 1) / kPartBlocks;
  return static_cast<uint32_t>((tile + kSinkWaves - 1) / kSinkWaves + 520);
}

}  // namespace
}  // namespace sdgpu
