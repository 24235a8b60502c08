// K5 group-by of the grouping (dedup.hip): one workgroup per bucket builds an
// LDS hash table of (key -> min rank) and maps every record to its rep; the
// two outputs (rep array, Object write set) and the write set's finish.
#pragma once

#include "part_device.hpp"

namespace sdgpu {
namespace {

constexpr int kGroupThreads = 1024;
// 6144 slots x 12 B = 72 KiB of LDS, so two buckets share a CU (8 waves/SIMD)
// and one bucket's loads overlap the other's LDS atomics.  The slot count is
// not a power of two: slots are indexed by the high half of hash * tsize.
constexpr uint32_t kLdsSlots = 6144;
constexpr uint32_t kLdsCap = 4608;     // rows per bucket handled in LDS (load <= 75%)
constexpr uint64_t kEmpty = ~0ull;
constexpr uint32_t kPadRow = 0xFFFFFFFFu;  // a record's row field: padding, not a row

// First probe slot of a record in the LDS table (kLdsSlots, any size): the
// low 32 bits of its hash, scaled.  The digit bits (the top ones) are constant
// inside a bucket, the low ones are not.
__device__ __forceinline__ uint32_t lds_slot(uint64_t h) {
  return static_cast<uint32_t>((static_cast<uint64_t>(static_cast<uint32_t>(h)) * kLdsSlots) >> 32);
}

// Double hashing: a key's probe step is 1 + 6 * (10 low hash bits, below the
// slot's), coprime with the 6144 (= 2^11 * 3) slots, so every probe sequence
// visits every slot and sequences of different keys do not run together in
// clusters.  A wave probes until its longest chain is placed; with linear
// probing those chains were clustered: 12.5 M rows 0.099 -> 0.081 ms
// (scripts/exp_group_persist.hip, profiles/r2/exp_group_persist_r2AG.log).
// (Round 5: the 10 bits are the LOW bits of h lo -- bits 40-49 overlapped the
// bucket's own digit bits, so inside a bucket the step took only 2^(10 -
// overlap) values; the slot comes from the top bits of h lo.)
__device__ __forceinline__ uint32_t lds_step(uint64_t h) {
  return 1u + 6u * (static_cast<uint32_t>(h) & 1023u);
}

__device__ __forceinline__ uint32_t next_slot(uint32_t h, uint32_t step) {
  const uint32_t s = h + step;  // h, step < kLdsSlots
  return s >= kLdsSlots ? s - kLdsSlots : s;
}

// Global-table slot (tsize a power of two, up to 2^34 for a 2^32-row bucket).
__device__ __forceinline__ uint64_t global_slot(uint64_t h, uint64_t tsize) {
  return h & (tsize - 1);
}

constexpr int kPer = (kLdsCap + kGroupThreads - 1) / kGroupThreads;

// Where K5 puts a bucket's result.  Per record: live (a keyed row of the
// bucket), r (its rank), w (its row), f (the lowest rank of its key).
//   RepOut:  rep[w] = f for the rows that link to an earlier chunk (the
//            partition initialised rep = rank): one scattered 4-B store each.
//   ListOut: the Object write set itself (round 4; sdgpu_group_link_device),
//            in the bucket's own record range [start, end) -- one entry per
//            keyed row, so the positions need no global coordination:
//            creators from the front, who = rank; linked rows from the back,
//            who = rank | SDGPU_LINKED, obj = f.  Coalesced;
//            no rep array.  lcnt[bucket] = its linked rows; the last bucket
//            stores the keyed total in lcnt[buckets]; k_list_finish then sets
//            counts[0..2] (no same-address atomics: 32 k workgroups adding
//            to one word serialised at ~4 ns each, +0.29 ms at 100 M rows in
//            r4e's fused_job leg).
struct RepOut {
  static constexpr int kScratch = 1;
  uint32_t* rep;
  template <int kSteps>
  __device__ __forceinline__ void emit(const bool (&)[kSteps], const bool (&lk)[kSteps],
                                       const uint32_t (&)[kSteps], const uint32_t (&w)[kSteps],
                                       const uint32_t (&f)[kSteps], uint32_t, uint32_t,
                                       uint32_t*) const {
#pragma unroll
    for (int j = 0; j < kSteps; ++j)
      if (lk[j]) rep[w[j]] = f[j];  // others keep rank
  }
};
// Block 0 sets counts[] from the buckets' linked counts lcnt[] and K = the
// keyed entries, lcnt[nb] (the last bucket's end): counts[1] = L, [0] = K - L
// + E, [2] = K + E -- loads issued 8 at a time (a plain loop over the 32 k
// counts of 100 M rows took ~10 us).  With a keyless sink (KeylessSink, E rows)
// block 1 + j moves the 16 wave segments of first-pass block j (valid keyless
// rows, who = rank: own Objects) to who[K + (rows of the segments before)
// ...], one wave per segment.  (Every block reducing a slice and adding it
// with atomics took 9 us: 512 same-address atomics, r4zd.)
__device__ __forceinline__ uint32_t block_sum(uint32_t v, uint32_t* sw) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
  if (__lane_id() == 0) sw[threadIdx.x >> 6] = v;
  __syncthreads();
  uint32_t t = 0;
  for (uint32_t w = 0; w < blockDim.x / 64; ++w) t += sw[w];
  __syncthreads();  // sw reusable
  return t;
}
// cap / nospc: the caller's list capacity (ListOut); sink rows past it are
// not written and the total past it raises *nospc.
__global__ __launch_bounds__(1024) void k_list_finish(const uint32_t* __restrict__ lcnt,
                                                      uint32_t nb, uint32_t* __restrict__ counts,
                                                      uint32_t* __restrict__ who, KeylessSink xs,
                                                      uint32_t cap, uint32_t* __restrict__ nospc) {
  __shared__ uint32_t sw[16], sseg[kSinkWaves];
  constexpr uint32_t kPerT = kPartBlocks * kSinkWaves / 1024;
  static_assert(kPartBlocks * kSinkWaves % 1024 == 0, "segments per thread");
  const uint32_t lane = __lane_id(), wv = threadIdx.x >> 6;
  const uint32_t seg0 = blockIdx.x ? (blockIdx.x - 1) * kSinkWaves : 0u;
  uint32_t e = 0, bf = 0;  // sink rows: all, in the segments before this block's
  if (xs.st) {             // the segment counts loaded together (one latency)
    uint32_t cv[kPerT];
#pragma unroll
    for (uint32_t k = 0; k < kPerT; ++k) cv[k] = xs.cnt[threadIdx.x + k * 1024];
#pragma unroll
    for (uint32_t k = 0; k < kPerT; ++k) {
      const uint32_t g = threadIdx.x + k * 1024;
      e += cv[k];
      if (g < seg0) bf += cv[k];
      if (blockIdx.x && g - seg0 < kSinkWaves) sseg[g - seg0] = cv[k];
    }
  }
  if (blockIdx.x == 0) {
    const uint32_t K = lcnt[nb];
    uint32_t l = 0;
    constexpr uint32_t kB = 8;
    for (uint32_t i0 = 0; i0 < nb; i0 += kB * 1024) {
      uint32_t v[kB];
#pragma unroll
      for (uint32_t k = 0; k < kB; ++k) {
        const uint32_t i = i0 + threadIdx.x + k * 1024;
        v[k] = i < nb ? lcnt[i] : 0u;
      }
#pragma unroll
      for (uint32_t k = 0; k < kB; ++k) l += v[k];
    }
    const uint32_t L = block_sum(l, sw), E = block_sum(e, sw);
    if (threadIdx.x == 0) {
      counts[1] = L;
      counts[0] = K - L + E;
      counts[2] = K + E;
      if (nospc && static_cast<uint64_t>(K) + E > cap) *nospc = 1u;
    }
    return;
  }
  const uint32_t before = block_sum(bf, sw);
  uint32_t o = lcnt[nb] + before;  // wave wv copies segment wv of first-pass block j
  for (uint32_t w = 0; w < wv; ++w) o += sseg[w];
  const uint32_t c = sseg[wv];
  const uint32_t* src = xs.st + static_cast<uint64_t>(seg0 + wv) * xs.cap;
  for (uint32_t k = lane; k < c; k += 64)
    if (o + k < cap) who[o + k] = src[k];
}
// ListOut: each wave reserves the slots of ALL its entries with ONE LDS
// atomic per list on the bucket's creator / linked counters (scr[0..1],
// zeroed with the table) and places step j's entries after those of steps
// < j (round 5: one atomic round trip per wave instead of one per step and
// list -- the group kernel is VALU-issue bound).  No barrier
// in emit, one at the end for the linked total.  The entries' order inside a
// bucket depends on wave timing (not part of the contract).  Workgroup-wide
// ranks in record order (two barriers + a one-wave scan per emit) measured
// slower: 100 M rows 1.870 -> 1.850 ms, 12.5 M rows 0.246 -> 0.244 ms
// (profiles/r4/listranks_ab/).
constexpr uint32_t kLinkedBit = 0x80000000u;
struct ListOut {
  static constexpr int kScratch = 2;
  uint32_t* who;
  uint32_t* obj;
  uint32_t* counts;
  uint32_t* lcnt;  // [bucket]: linked rows; [buckets]: the keyed total
  KeylessSink x;         // the valid keyless rows, when the partition collects them
  // entries who / obj hold (the sharded write set's caller capacity): a
  // bucket ending past it writes nothing and sets *nospc (the call then
  // fails with -ENOSPC); ~0: unbounded (n entries at most)
  uint32_t cap = 0xFFFFFFFFu;
  uint32_t* nospc = nullptr;
  template <int kSteps>
  __device__ __forceinline__ void emit(const bool (&live)[kSteps], const bool (&lk)[kSteps],
                                       const uint32_t (&r)[kSteps], const uint32_t (&w)[kSteps],
                                       const uint32_t (&f)[kSteps], uint32_t start, uint32_t end,
                                       uint32_t* scr) const {
    if (end > cap) {  // uniform per bucket
      if (threadIdx.x == 0) *nospc = 1u;
      return;
    }
    uint64_t bc[kSteps], bl[kSteps];
    uint32_t nc = 0, nl = 0;
#pragma unroll
    for (int j = 0; j < kSteps; ++j) {
      bc[j] = __ballot(live[j] && !lk[j]);
      bl[j] = __ballot(lk[j]);
      nc += static_cast<uint32_t>(__popcll(bc[j]));
      nl += static_cast<uint32_t>(__popcll(bl[j]));
    }
    uint32_t cb = 0, lb = 0;
    if (__lane_id() == 0) {
      if (nc) cb = atomicAdd(&scr[0], nc);
      if (nl) lb = atomicAdd(&scr[1], nl);
    }
    cb = __builtin_amdgcn_readfirstlane(cb);  // lane 0 is active here
    lb = __builtin_amdgcn_readfirstlane(lb);
#pragma unroll
    for (int j = 0; j < kSteps; ++j) {
      const uint32_t bc_lo = static_cast<uint32_t>(bc[j]), bc_hi = static_cast<uint32_t>(bc[j] >> 32);
      const uint32_t bl_lo = static_cast<uint32_t>(bl[j]), bl_hi = static_cast<uint32_t>(bl[j] >> 32);
      if (live[j] && !lk[j])
        who[start + cb + __builtin_amdgcn_mbcnt_hi(bc_hi, __builtin_amdgcn_mbcnt_lo(bc_lo, 0u))] = r[j];
      if (lk[j]) {
        const uint32_t p =
            end - 1 - (lb + __builtin_amdgcn_mbcnt_hi(bl_hi, __builtin_amdgcn_mbcnt_lo(bl_lo, 0u)));
        who[p] = r[j] | kLinkedBit;
        obj[p] = f[j];
      }
      cb += static_cast<uint32_t>(__popcll(bc[j]));
      lb += static_cast<uint32_t>(__popcll(bl[j]));
    }
    (void)w;
  }
};
__device__ __forceinline__ void out_init(const RepOut&, uint32_t*) {}
__device__ __forceinline__ void out_init(const ListOut&, uint32_t* scr) {
  if (threadIdx.x < 2) scr[threadIdx.x] = 0;  // before the bucket's first barrier
}
__device__ __forceinline__ void out_done(const ListOut& o, uint32_t end, const uint32_t* scr) {
  __syncthreads();  // every wave's atomics on the counters are done
  if (threadIdx.x == 0) {
    o.lcnt[blockIdx.x] = scr[1];
    if (blockIdx.x == gridDim.x - 1) o.lcnt[gridDim.x] = end;
  }
}
__device__ __forceinline__ void out_done(const RepOut&, uint32_t, const uint32_t*) {}

// Bucket records as {hash lo, hash hi, rank, row}: 16-byte records as stored,
// or 12-byte ones {hash lo, hash hi, row} with rank = rank_base + row.
struct Rec16Src {
  const uint4* __restrict__ p;
  __device__ __forceinline__ uint4 operator()(uint32_t i) const { return p[i]; }
};
struct Rec12Src {
  const uint3* __restrict__ p;
  uint32_t rank_base;
  __device__ __forceinline__ uint4 operator()(uint32_t i) const {
    const uint3 v = p[i];
    return make_uint4(v.x, v.y, rank_base + v.z, v.z);
  }
};

// LDS-sized bucket: every thread loads its (at most kPer) records at once and
// keeps them in registers for both phases.
template <typename Src>
__device__ __forceinline__ void load_bucket(Src rec, uint32_t start, uint32_t end,
                                            uint4 (&q_reg)[kPer]) {
  if (end - start > kLdsCap || end == start) return;
  // unconditional loads, selected after (see group_bucket_packed)
#pragma unroll
  for (int j = 0; j < kPer; ++j) q_reg[j] = rec(min(start + threadIdx.x + j * kGroupThreads, end - 1));
#pragma unroll
  for (int j = 0; j < kPer; ++j)
    if (start + threadIdx.x + j * kGroupThreads >= end) q_reg[j] = make_uint4(0, 0, 0, 0);
}

// Group-by of one bucket too large for LDS: a private region of the global
// table (4 slots per row, agent-scope atomics).  The results leave in chunks of
// kGroupThreads records (uniform trip count: the list output ranks each chunk
// across the workgroup).
template <typename Src, typename Out>
__device__ __forceinline__ void group_bucket_global(Src rec, uint32_t start, uint32_t end,
                                                    ChunkOf chunk_of, uint64_t* __restrict__ gkey,
                                                    uint32_t* __restrict__ gmin, const Out& out,
                                                    uint32_t& special_min, uint32_t* scr) {
  const uint32_t m = end - start;
  uint64_t tsize = 1;
  while (tsize * 2 <= 4ull * m) tsize *= 2;  // 2m < tsize <= 4m (64-bit: no wrap)
  uint64_t* tk = gkey + 4ull * start;
  uint32_t* tm = gmin + 4ull * start;
  for (uint64_t s = threadIdx.x; s < tsize; s += kGroupThreads) {
    tk[s] = kEmpty;
    tm[s] = 0xFFFFFFFFu;
  }
  if (threadIdx.x == 0) special_min = 0xFFFFFFFFu;
  out_init(out, scr);
  __syncthreads();
  for (uint32_t i = start + threadIdx.x; i < end; i += kGroupThreads) {
    const uint4 q = rec(i);
    const uint64_t k = (static_cast<uint64_t>(q.y) << 32) | q.x;
    const uint32_t r = q.z;
    if (k == kEmpty) {
      atomicMin(&special_min, r);
      continue;
    }
    uint64_t h = global_slot(k, tsize);
    for (;;) {
      const uint64_t prev = atomicCAS(reinterpret_cast<unsigned long long*>(&tk[h]),
                                      static_cast<unsigned long long>(kEmpty),
                                      static_cast<unsigned long long>(k));
      if (prev == kEmpty || prev == k) {
        atomicMin(&tm[h], r);
        break;
      }
      h = (h + 1) & (tsize - 1);
    }
  }
  __syncthreads();
  for (uint32_t i0 = start; i0 < end; i0 += kGroupThreads) {
    const uint32_t i = i0 + threadIdx.x;
    bool live[1] = {false}, lk[1] = {false};
    uint32_t r[1] = {0}, w[1] = {0}, f[1] = {0};
    if (i < end) {
      const uint4 q = rec(i);
      const uint64_t k = (static_cast<uint64_t>(q.y) << 32) | q.x;
      uint32_t fv;
      if (k == kEmpty) {
        fv = special_min;
      } else {
        uint64_t h = global_slot(k, tsize);
        for (;;) {
          const uint64_t kk =
              __hip_atomic_load(&tk[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          if (kk == k) break;
          h = (h + 1) & (tsize - 1);
        }
        fv = __hip_atomic_load(&tm[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      live[0] = true;
      r[0] = q.z;
      w[0] = q.w;
      f[0] = fv;
      lk[0] = chunk_of(q.z) != chunk_of(fv);
    }
    out.template emit<1>(live, lk, r, w, f, start, end, scr);
  }
  out_done(out, end, scr);
}

// Group-by of one bucket, rows [start, end) of rec (q_reg preloaded by
// load_bucket when the bucket fits the LDS table).
template <typename Src, typename Out>
__device__ __forceinline__ void group_bucket(Src rec, uint32_t start,
                                             uint32_t end, const uint4 (&q_reg)[kPer],
                                             ChunkOf chunk_of, uint64_t* __restrict__ gkey,
                                             uint32_t* __restrict__ gmin, const Out& out,
                                             uint64_t* lkey, uint32_t* lmin, uint32_t& special_min,
                                             uint32_t* scr) {
  const uint32_t m = end - start;
  if (m == 0) {
    out_init(out, scr);  // an empty bucket: counters zeroed for done
    out_done(out, end, scr);
    return;
  }
  if (m > kLdsCap) {
    group_bucket_global(rec, start, end, chunk_of, gkey, gmin, out, special_min, scr);
    return;
  }
  // (the LDS code names lkey / lmin directly: through generic pointers shared
  // with the global table the compiler emits FLAT atomics, ~30 % slower)
  for (uint32_t s = threadIdx.x; s < kLdsSlots; s += kGroupThreads) {
    lkey[s] = kEmpty;
    lmin[s] = 0xFFFFFFFFu;
  }
  if (threadIdx.x == 0) special_min = 0xFFFFFFFFu;
  out_init(out, scr);
  __syncthreads();
  // A thread's records probe in lock step: every pass issues the LDS
  // round trips of all its pending records back to back and only then
  // inspects the results, so their latencies overlap (the probe loops are
  // latency-bound, not LDS-bandwidth-bound).
  uint32_t h[kPer], step[kPer];
  uint32_t live = 0, pend = 0;  // bit j: record j exists / is still probing
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const uint64_t k = (static_cast<uint64_t>(q_reg[j].y) << 32) | q_reg[j].x;
    h[j] = lds_slot(k);
    step[j] = lds_step(k);
    if (start + threadIdx.x + j * kGroupThreads < end) {
      live |= 1u << j;
      if (k == kEmpty)
        atomicMin(&special_min, q_reg[j].z);
      else
        pend |= 1u << j;
    }
  }
  const uint32_t keyed = pend;
  while (pend) {
    uint64_t prev[kPer];
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
      const uint64_t k = (static_cast<uint64_t>(q_reg[j].y) << 32) | q_reg[j].x;
      prev[j] = (pend >> j & 1u)
                    ? atomicCAS(reinterpret_cast<unsigned long long*>(&lkey[h[j]]),
                                static_cast<unsigned long long>(kEmpty),
                                static_cast<unsigned long long>(k))
                    : 0ull;
    }
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
      if (!(pend >> j & 1u)) continue;
      const uint64_t k = (static_cast<uint64_t>(q_reg[j].y) << 32) | q_reg[j].x;
      if (prev[j] == kEmpty || prev[j] == k) {
        atomicMin(&lmin[h[j]], q_reg[j].z);
        pend &= ~(1u << j);
      } else {
        h[j] = next_slot(h[j], step[j]);
      }
    }
  }
  __syncthreads();
  // every keyed record's final probe slot h[j] holds its key: read the
  // group minimum there (no second probe sequence needed)
  bool lv[kPer], lk[kPer];
  uint32_t r[kPer], w[kPer], f[kPer];
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    lv[j] = live >> j & 1u;
    r[j] = q_reg[j].z;
    w[j] = q_reg[j].w;
    f[j] = lv[j] ? ((keyed >> j & 1u) ? lmin[h[j]] : special_min) : 0u;
    lk[j] = lv[j] && chunk_of(r[j]) != chunk_of(f[j]);
  }
  out.template emit<kPer>(lv, lk, r, w, f, start, end, scr);
  out_done(out, end, scr);
}

// K5 with a PACKED 8-byte LDS table, for buckets of 12-15 digit bits (the
// one-level 12-bit path and the two-level path).  Inside a bucket the digit
// bits of h are implied, so a key is known by its other 64 - bits (<= 52)
// bits; with the record's index in the bucket + 1 (12 bits, 0 = empty) a
// slot is ONE 64-bit word.  The CAS that places or finds a key also names the
// record that owns it, the group minimum lives per owner (lmin[4096]), and
// 7680 slots fit where 6144 twelve-byte ones did: load ~0.4 instead of ~0.5,
// shorter probe chains.  scripts/exp/exp_group_packed.hip: 12.5 M rows 0.078
// -> 0.072 ms (profiles/r3/exp_group_packed/run.log).
// Round 5: the kernel is VALU-issue bound (SQ counters,
// VALU busy 73 % of the SIMD cycles at 12.5 M rows, 82 % at
// 100 M), so the VALU per record was cut twice.  First: the word assembled
// from 32-bit halves, and a double-hashing step from the LOW bits of h lo
// (the old one overlapped the digit bits: nearly linear probing).  Second:
// 2^13 slots (a step wraps as a 16-bit add of byte offsets; the odd step
// from the 13 low bits of h lo, the slot from its 13 top bits); the probe
// loop without branches per record (see below); the owner read from the
// record's final slot after the loop.  Probe-loop VALU per record and round
// ~16 -> 7.  64 KiB of table + a 4096-word area = exactly half the CU's LDS
// (two workgroups per CU, as before); the area holds lmin[kPkCap],
// special_min and the output's scratch, so kPkCap = 4093.  (Linear probing,
// step 1, lengthened the probe chains: 12.5 M rows 0.079 -> 0.085 ms,
// profiles/r5/pk_ab/.)
// Buckets above kPkCap records take the global table; pads (row ~0) are skipped.
constexpr uint32_t kPkSlots = 8192;  // 2^13
constexpr uint32_t kPkWords = 4096;  // lmin[kPkCap] | special_min | scr[2]
constexpr uint32_t kPkCap = kPkWords - 3;

// The packed group-by of one bucket whose records are in registers (q[j] =
// {h lo, h hi, rank, row}, row kPadRow past the end), m = end - start <=
// kPkCap, bits in 12..15 (the word's key field; group_launch picks this
// kernel only for those).
template <int kP, typename Out>
__device__ __forceinline__ void group_packed_regs(const uint4 (&q)[kP], uint32_t start, uint32_t end,
                                                  uint32_t bits, ChunkOf chunk_of, const Out& out,
                                                  uint64_t* tab, uint32_t* lmin, uint32_t* scr) {
  for (uint32_t s = threadIdx.x; s < kPkSlots; s += kGroupThreads) tab[s] = 0ull;
  for (uint32_t s = threadIdx.x; s < kPkCap; s += kGroupThreads) lmin[s] = 0xFFFFFFFFu;
  out_init(out, scr);
  __syncthreads();
  // word hi: the 24 - bits hi-word bits below the digit, the 8 shard bits
  // above it, then index + 1 in bits 20..31 (bits in 12..15: <= 20 key bits)
  const uint32_t kb = 24u - bits, lowm = (1u << kb) - 1u;
  uint32_t sa[kP], sst[kP], own1[kP], khi[kP];
  uint64_t word[kP];  // the record's word; 0 for a pad
  bool live[kP];
#pragma unroll
  for (int j = 0; j < kP; ++j) {
    const uint32_t idx1 = threadIdx.x + j * kGroupThreads + 1u;
    khi[j] = (q[j].y & lowm) | ((q[j].y >> 24) << kb);
    live[j] = q[j].w != kPadRow;
    word[j] = live[j] ? (static_cast<uint64_t>(khi[j] | (idx1 << 20)) << 32) | q[j].x : 0ull;
    // byte offsets: the slot from the top 13 bits of h lo, the (odd) step
    // from its low 13 bits -- both independent of the digit bits (h hi)
    // (a pad: a slot of its own lane -- pads share the last record's h, and
    // 64 lanes CASing one word serialise)
    sa[j] = live[j] ? (q[j].x >> 16) & 0xFFF8u : threadIdx.x << 3;
    sst[j] = ((q[j].x << 3) | 8u) & 0xFFF8u;
  }
  // The records of a thread probe in lock step, without branches: every
  // round CASes all four words and the round's results decide.  A record
  // that has found its key CASes the same slot again, which holds that key
  // (its own word or its owner's) and so leaves it unchanged and finds it
  // again; a pad's word is 0, and CAS(0 -> 0) changes nothing.  Branches
  // per record (the lanes' pending masks) made the compiler wait out each
  // CAS before issuing the next.
  for (;;) {
    uint64_t prev[kP];
#pragma unroll
    for (int j = 0; j < kP; ++j)
      prev[j] = atomicCAS(reinterpret_cast<unsigned long long*>(reinterpret_cast<char*>(tab) + sa[j]),
                          0ull, static_cast<unsigned long long>(word[j]));
    bool all = true;
#pragma unroll
    for (int j = 0; j < kP; ++j) {
      const uint32_t plo = static_cast<uint32_t>(prev[j]), phi = static_cast<uint32_t>(prev[j] >> 32);
      const bool hit = !live[j] || prev[j] == 0ull || (plo == q[j].x && (phi & 0xFFFFFu) == khi[j]);
      sa[j] = static_cast<uint16_t>(sa[j] + (hit ? 0u : sst[j]));  // 2^13 slots x 8 B
      all = all && hit;
    }
    if (all) break;
  }
  // each record's slot now holds its key's word: the owner's index + 1 (a
  // pad's slot may be empty: index 0 then, so that its unused lmin read
  // stays inside lmin)
#pragma unroll
  for (int j = 0; j < kP; ++j)
    own1[j] = max(1u, *reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(tab) + sa[j] + 4) >> 20);
#pragma unroll
  for (int j = 0; j < kP; ++j)
    if (live[j]) atomicMin(&lmin[own1[j] - 1u], q[j].z);
  __syncthreads();
  bool lk[kP];
  uint32_t r[kP], w[kP], f[kP];
#pragma unroll
  for (int j = 0; j < kP; ++j) {
    r[j] = q[j].z;
    w[j] = q[j].w;
    f[j] = lmin[own1[j] - 1u];
    lk[j] = live[j] && r[j] != f[j] && chunk_of(r[j]) != chunk_of(f[j]);
  }
  out.template emit<kP>(live, lk, r, w, f, start, end, scr);
}

// Records of a bucket into registers, kP per thread: every load issued
// unconditionally (past the end: the bucket's last record) and the pad
// selected after -- a guarded `i < end ? rec(i) : pad` made the compiler
// branch around each load and wait out its latency before the next one
// (four serial memory latencies per workgroup).  Only the row marks a pad:
// nothing reads a pad's other fields.
template <int kP, typename Src, typename Out>
__device__ __forceinline__ void group_packed_load(Src rec, uint32_t start, uint32_t end,
                                                  uint32_t bits, ChunkOf chunk_of, const Out& out,
                                                  uint64_t* tab, uint32_t* lmin, uint32_t* scr) {
  uint4 q[kP];
#pragma unroll
  for (int j = 0; j < kP; ++j) q[j] = rec(min(start + threadIdx.x + j * kGroupThreads, end - 1));
#pragma unroll
  for (int j = 0; j < kP; ++j)
    if (start + threadIdx.x + j * kGroupThreads >= end) q[j].w = kPadRow;
  group_packed_regs(q, start, end, bits, chunk_of, out, tab, lmin, scr);
}

template <typename Src, typename Out>
__device__ __forceinline__ void group_bucket_packed(Src rec, uint32_t start, uint32_t end,
                                                    uint32_t bits, ChunkOf chunk_of,
                                                    uint64_t* __restrict__ gkey,
                                                    uint32_t* __restrict__ gmin, const Out& out,
                                                    uint64_t* tab, uint32_t* lmin,
                                                    uint32_t& special_min, uint32_t* scr) {
  const uint32_t m = end - start;
  if (m == 0) {
    out_init(out, scr);  // an empty bucket: counters zeroed for done
    out_done(out, end, scr);
    return;
  }
  if (m > kPkCap) {
    group_bucket_global(rec, start, end, chunk_of, gkey, gmin, out, special_min, scr);
    return;
  }
  // three records per thread when they suffice (uniform per bucket; ~3 k
  // records is the mean bucket): a fourth of pads would still probe
  static_assert(kPkCap <= 4 * kGroupThreads, "four records per thread hold a bucket");
  if (m <= 3 * kGroupThreads)
    group_packed_load<3>(rec, start, end, bits, chunk_of, out, tab, lmin, scr);
  else
    group_packed_load<4>(rec, start, end, bits, chunk_of, out, tab, lmin, scr);
  out_done(out, end, scr);
}

// One workgroup per bucket.  Rows of bucket b: [offs[b*P], offs[(b+1)*P]).
template <typename Out>
__global__ __launch_bounds__(kGroupThreads, 8) void k_bucket_group(
    const uint4* __restrict__ rec, const uint32_t* __restrict__ offs, uint32_t P,
    ChunkOf chunk_of, uint64_t* __restrict__ gkey, uint32_t* __restrict__ gmin, Out out) {
  __shared__ uint64_t lkey[kLdsSlots];
  __shared__ uint32_t lmin[kLdsSlots];
  __shared__ uint32_t special_min;  // min rank of key == kEmpty (sentinel clash)
  __shared__ uint32_t scr[Out::kScratch];
  const uint32_t b = blockIdx.x;
  const uint32_t start = offs[static_cast<uint64_t>(b) * P];
  const uint32_t end = offs[static_cast<uint64_t>(b + 1) * P];  // offs[nb*P] = total
  uint4 q_reg[kPer];
  load_bucket(Rec16Src{rec}, start, end, q_reg);
  group_bucket(Rec16Src{rec}, start, end, q_reg, chunk_of, gkey, gmin, out, lkey, lmin,
               special_min, scr);
}

// Packed-table K5 (>= 12 digit bits): rows of bucket b in [offs[b*P], offs[(b+1)*P]).
template <typename Out>
__global__ __launch_bounds__(kGroupThreads, 8) void k_bucket_group_pk(
    const uint4* __restrict__ rec, const uint32_t* __restrict__ offs, uint32_t P, uint32_t bits,
    ChunkOf chunk_of, uint64_t* __restrict__ gkey, uint32_t* __restrict__ gmin, Out out) {
  __shared__ uint64_t tab[kPkSlots];
  __shared__ uint32_t lw[kPkWords];  // lmin | special_min | scr (80 KiB in all)
  static_assert(Out::kScratch <= 2, "scratch fits the word area");
  uint32_t* lmin = lw;
  uint32_t& special_min = lw[kPkCap];
  uint32_t* scr = lw + kPkCap + 1;
  const uint32_t b = blockIdx.x;
  group_bucket_packed(Rec16Src{rec}, offs[static_cast<uint64_t>(b) * P],
                      offs[static_cast<uint64_t>(b + 1) * P], bits, chunk_of, gkey, gmin, out, tab,
                      lmin, special_min, scr);
}

template <typename Out>
__global__ __launch_bounds__(kGroupThreads, 8) void k_bucket_group12_pk(
    const uint3* __restrict__ rec, uint32_t rank_base, const uint32_t* __restrict__ offs,
    uint32_t bits, ChunkOf chunk_of, uint64_t* __restrict__ gkey, uint32_t* __restrict__ gmin,
    Out out) {
  __shared__ uint64_t tab[kPkSlots];
  __shared__ uint32_t lw[kPkWords];  // lmin | special_min | scr (80 KiB in all)
  static_assert(Out::kScratch <= 2, "scratch fits the word area");
  uint32_t* lmin = lw;
  uint32_t& special_min = lw[kPkCap];
  uint32_t* scr = lw + kPkCap + 1;
  const uint32_t b = blockIdx.x;
  group_bucket_packed(Rec12Src{rec, rank_base}, offs[b], offs[b + 1], bits, chunk_of, gkey, gmin,
                      out, tab, lmin, special_min, scr);
}

}  // namespace
}  // namespace sdgpu
