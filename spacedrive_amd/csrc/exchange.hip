// Device steps of the multi-GPU exchange (shard.cpp): the partition of the
// caller's rows by destination rank or shard (scanned offsets, or one pass
// into fixed-capacity padded messages), the message headers and summaries,
// and the return of the reps to their rows (full gather or compact pairs).
// Digits come from h = mix64(key) as in the grouping (dedup.hip): the shard
// is h's top kShardBits bits.
#include "compact_device.hpp"
#include "internal.hpp"
#include "part_device.hpp"
#include "scan_device.hpp"

#include <algorithm>

namespace sdgpu {
namespace {

// Shard partition of the multi-GPU exchange: keyed rows packed by digit (the
// destination rank, or a shard) at the scanned offsets.
//   kRec12: one packed 12-byte send record {key lo, key hi, rank} per row
//           (what travels over xGMI) and, per SOURCE row i, out_pos[i] = its
//           send position (~0 for keyless rows): a coalesced write, and the
//           reps come back through a gather (k_gather_rep);
//   else:   separate key / rank arrays and out_pos[p] = source row of packed
//           row p (the single-step ABI for hosts with their own collectives).
// kRec12 with out_pos null: the write-set form, which needs no send
// positions (no rep comes back).
template <typename In, bool kRec12>
__global__ __launch_bounds__(kPartThreads) void k_part_scatter(
    In in, uint64_t n, uint32_t skip, uint32_t bits, uint32_t world,
    const uint32_t* __restrict__ offs, uint64_t* __restrict__ out_key,
    uint32_t* __restrict__ out_rank, uint3* __restrict__ out_rec, uint32_t* __restrict__ out_pos) {
  extern __shared__ __attribute__((aligned(16))) uint32_t cur[];
  const uint32_t nbins = world ? world : 1u << bits;
  for (uint32_t b = threadIdx.x; b < nbins; b += kPartThreads)
    cur[b] = offs[static_cast<uint64_t>(b) * gridDim.x + part_block()];
  __syncthreads();
  uint64_t t0, t1;
  tile_of(n, gridDim.x, t0, t1);
  constexpr int U = kUnroll / 2;
  for (uint64_t i0 = t0 + threadIdx.x; i0 < t1; i0 += U * kPartThreads) {
    RowBatch<U> q;
    in.template load_many<U>(i0, kPartThreads, t1, i0, q);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint64_t i = i0 + static_cast<uint64_t>(u) * kPartThreads;
      const bool v = in.valid_of(q, u);
      const uint64_t k = in.key_of(q, u);
      const uint32_t d = v ? part_digit(in_hash<In>(k), skip, bits, world) : 0u;
      const uint32_t p = world ? wave_add(cur, d, v, world_bits(world)) : (v ? atomicAdd(&cur[d], 1u) : 0u);
      if (!v) {
        if (kRec12 && q.in[u] && out_pos) out_pos[i] = 0xFFFFFFFFu;
        continue;
      }
      const uint32_t r = in.rank_of(q, u);
      if (kRec12) {
        out_rec[p] = make_uint3(static_cast<uint32_t>(k), static_cast<uint32_t>(k >> 32), r);
        if (out_pos) out_pos[i] = p;
      } else {
        out_key[p] = k;
        out_rank[p] = r;
        out_pos[p] = static_cast<uint32_t>(i);
      }
    }
  }
}

// Padded exchange partition (round 5; shard.cpp padded exchange): ONE pass
// over the caller's rows, no histogram or scan.  Each round of kPadR rows a
// block counting-sorts its keyed rows by owner in LDS, reserves each owner's
// run inside that owner's fixed-capacity message with ONE global atomic per
// owner (cursor[d], zeroed before the launch), and copies the runs out
// coalesced.  Message d = slots d * (cap + 1) .. of the send buffer (slot 0
// its header, k_pad_fill); the message to this rank itself (d == me) is
// written straight into the receive buffer (self_out, same slots): no copy.
// The order of the rows inside a message follows the reservations, not row
// order -- the grouping reads ranks, not positions.  Slots past cap are not
// written (cursor[d] > cap: k_pad_fill raises the overflow bit).  out_pos
// (rep form; null for the write set): the send slot of row i, ~0 for keyless
// or unsent rows.  xs (the write set): the valid keyless rows are collected
// into the KeylessSink segments on the way (as the fused call's first pass does),
// for the owner's k_list_finish -- no extra-entry pass.  Round r + 1's rows
// are loaded before round r's atomics.
constexpr int kPadU = 4;
constexpr uint32_t kPadR = kPadU * kPartThreads;
__global__ __launch_bounds__(kPartThreads) void k_part_padded(
    RowsIn in, uint64_t n, uint32_t world, uint32_t me, uint32_t cap, uint3* __restrict__ out,
    uint3* __restrict__ self_out, uint32_t* __restrict__ out_pos,
    uint32_t* __restrict__ cursor, KeylessSink xs) {
  __shared__ uint3 buf[kPadR];
  __shared__ uint32_t cnt[kMaxWorld], lb[kMaxWorld + 1], gb[kMaxWorld];
  const uint64_t c1 = cap + 1ull;
  uint32_t wn = 0;  // the wave's keyless rows (KeylessSink)
  uint64_t t0, t1;
  tile_of(n, gridDim.x, t0, t1);
  auto round = [&](const RowBatch<kPadU>& q, uint64_t i0) {
    if (threadIdx.x < world) cnt[threadIdx.x] = 0;
    lds_barrier();
    uint32_t dg[kPadU], lr[kPadU];
#pragma unroll
    for (int u = 0; u < kPadU; ++u) {
      const bool v = in.valid_of(q, u);
      const uint32_t d = v ? part_digit(row_hash(in.key_of(q, u)), 0, kShardBits, world) : 0u;
      lr[u] = wave_add(cnt, d, v, world_bits(world));
      dg[u] = v ? d : ~0u;
      if (xs.st)  // uniform; a ballot, and a store only for the rare valid keyless row
        sink_keyless(xs, in, q.in[u] && !v, i0 + threadIdx.x + static_cast<uint64_t>(u) * kPartThreads,
                     wn);
    }
    lds_barrier();
    if (threadIdx.x < 64) {  // one wave: the round's run starts and the reservations
      const uint32_t lane = threadIdx.x;
      const uint32_t c = lane < world ? cnt[lane] : 0u;
      uint32_t inc = c;
#pragma unroll
      for (int s = 1; s < 64; s <<= 1) {
        const uint32_t o = __shfl_up(inc, s);
        if (lane >= static_cast<uint32_t>(s)) inc += o;
      }
      if (lane < world) lb[lane] = inc - c;
      if (lane == world - 1) lb[world] = inc;
      if (lane < world && c) gb[lane] = atomicAdd(&cursor[lane], c);
    }
    lds_barrier();
#pragma unroll
    for (int u = 0; u < kPadU; ++u) {
      const uint64_t i = i0 + threadIdx.x + static_cast<uint64_t>(u) * kPartThreads;
      if (dg[u] == ~0u) {
        if (out_pos && q.in[u]) out_pos[i] = 0xFFFFFFFFu;
        continue;
      }
      const uint32_t d = dg[u];
      const uint64_t k = in.key_of(q, u);
      buf[lb[d] + lr[u]] = make_uint3(static_cast<uint32_t>(k), static_cast<uint32_t>(k >> 32),
                                      in.rank_of(q, u));
      if (out_pos) {
        const uint32_t pos = gb[d] + lr[u];
        out_pos[i] = pos < cap ? static_cast<uint32_t>(d * c1 + 1 + pos) : 0xFFFFFFFFu;
      }
    }
    lds_barrier();
    const uint32_t total = lb[world];
    for (uint32_t k = threadIdx.x; k < total; k += kPartThreads) {
      uint32_t lo = 0, hi = world - 1;  // the owner of slot k: last d with lb[d] <= k
      while (lo < hi) {
        const uint32_t mid = (lo + hi + 1) >> 1;
        if (lb[mid] <= k) lo = mid;
        else hi = mid - 1;
      }
      const uint32_t pos = gb[lo] + (k - lb[lo]);
      if (pos < cap) (lo == me ? self_out : out)[lo * c1 + 1 + pos] = buf[k];
    }
    lds_barrier();  // buf, cnt and lb are rewritten by the next round
  };
  if (t0 < t1) {
    RowBatch<kPadU> qa, qb;
    in.template load_many<kPadU>(t0 + threadIdx.x, kPartThreads, t1, t0, qa);
    for (uint64_t i0 = t0;; i0 += 2 * kPadR) {  // uniform trip count
      in.template load_many<kPadU>(i0 + kPadR + threadIdx.x, kPartThreads, t1, t0, qb);
      round(qa, i0);
      if (i0 + kPadR >= t1) break;
      in.template load_many<kPadU>(i0 + 2 * kPadR + threadIdx.x, kPartThreads, t1, t0, qa);
      round(qb, i0 + kPadR);
      if (i0 + 2 * kPadR >= t1) break;
    }
  }
  if (xs.st) sink_count(xs, wn);
}

__global__ __launch_bounds__(256) void k_fill_init(uint32_t* __restrict__ dst, uint64_t n,
                                                   const uint32_t* __restrict__ init) {
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * 256;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x; i < n; i += stride)
    dst[i] = init ? init[i] : static_cast<uint32_t>(i);
}

__global__ __launch_bounds__(256) void k_scatter(const uint32_t* __restrict__ src,
                                                 const uint32_t* __restrict__ pos, uint64_t n,
                                                 uint32_t* __restrict__ dst) {
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * 256;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x; i < n; i += stride)
    dst[pos[i]] = src[i];
}

__global__ void k_copy_counts(const uint32_t* __restrict__ offs, uint32_t nbins,
                              uint64_t* __restrict__ counts) {
  const uint32_t b = threadIdx.x;
  if (b < nbins)
    counts[b] = offs[static_cast<uint64_t>(b + 1) * kPartBlocks] -
                offs[static_cast<uint64_t>(b) * kPartBlocks];
}

// Rows per destination rank of the exchange, from the scanned offsets of the
// destination-digit partition.
// msgs (may be NULL): the count messages of the exchange, {rows for d, n,
// code} per destination d (every rank learns every rank's n with the counts;
// code = the call's form and return leg, which every rank must share --
// checked by the receivers).
__global__ void k_dest_counts(const uint32_t* __restrict__ offs, uint32_t world,
                              int64_t* __restrict__ counts, int64_t* __restrict__ msgs,
                              int64_t n, int64_t code) {
  const uint32_t d = threadIdx.x;
  if (d < world) {
    const int64_t c = static_cast<int64_t>(offs[static_cast<uint64_t>(d + 1) * kPartBlocks]) -
                      offs[static_cast<uint64_t>(d) * kPartBlocks];
    counts[d] = c;
    if (msgs) {
      msgs[3 * d] = c;
      msgs[3 * d + 1] = n;
      msgs[3 * d + 2] = code;
    }
  }
}

// rep[i] of the sender's rows from the reps returned in send order: row i was
// sent at position pos[i] (~0: no key, it keeps its own rank).  Every sent
// position holds a rep: the full return writes all of them, the compact one
// starts from each record's own rank (k_back_init).  (Round 4 marked "no
// pair came back" with back == ~0, which is also the legal rep
// SDGPU_REP_EXISTING | 0x7FFFFFFF: ADVICE r4.)
// Positions in [self_lo, self_hi) read self[p]: the padded exchange's
// message to this rank itself, whose reps the owner side wrote locally.
__global__ __launch_bounds__(256) void k_gather_rep(const uint32_t* __restrict__ back,
                                                    const uint32_t* __restrict__ pos,
                                                    const uint32_t* __restrict__ rank, uint64_t n,
                                                    uint32_t* __restrict__ rep,
                                                    const uint32_t* __restrict__ self,
                                                    uint32_t self_lo, uint32_t self_hi) {
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * 256;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x; i < n; i += stride) {
    const uint32_t p = pos[i];
    const bool mine = p - self_lo < self_hi - self_lo;  // never for p == ~0 (< 2^32 slots)
    const uint32_t b = (mine ? self : back)[p == 0xFFFFFFFFu ? 0u : p];
    rep[i] = p == 0xFFFFFFFFu ? rank[i] : b;
  }
}

// Compact return leg, source side: back[p] = the rank in send record p (a
// row whose rep is its own rank gets no pair back).
__global__ __launch_bounds__(256) void k_back_init(const uint3* __restrict__ srec, uint64_t n,
                                                   uint32_t* __restrict__ back) {
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * 256;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x; i < n; i += stride)
    back[i] = srec[i].z;
}

// Fixed-capacity exchange messages (shard.cpp, padded exchange): the message
// to rank d is C1 = cap + 1 12-byte slots at d * C1 of the send buffer --
// slot 0 the header {rows for d | this source's overflow bit << 31, this
// source's n, kPadRank}, slots 1..cap the records (k_part_scatter with
// k_part_padded), the rest padding {0, 0, kPadRank}; the message to this
// rank itself lives in the receive buffer (self_out).  The owner's grouping drops
// every kPadRank record (RecIn::valid_of).  The overflow bit (some count of
// this source > cap: rows were not sent) goes to EVERY owner, so all ranks
// learn the same "some message overflowed" from their headers.  Block (0, 0)
// also writes summary[3] = rows this source sent, clears summary[4] (the
// list kernels' -ENOSPC flag) and zero3[0..2] (the write set's counts).
// counts (cnt: the reservation cursors) < 2^31 (n < 2^31 on this path).
__global__ __launch_bounds__(256) void k_pad_fill(const uint32_t* __restrict__ cnt, uint32_t world,
                                                  uint32_t me, uint32_t cap, uint32_t n,
                                                  uint3* __restrict__ out,
                                                  uint3* __restrict__ self_out,
                                                  uint32_t* __restrict__ summary,
                                                  uint32_t* __restrict__ zero3,
                                                  uint32_t* __restrict__ next_cursor) {
  const uint32_t d = blockIdx.y;
  bool ovf = false;
  uint32_t sent = 0;
  for (uint32_t p = 0; p < world; ++p) {
    const uint32_t c = cnt[p];
    ovf |= c > cap;
    sent += min(c, cap);
  }
  uint3* rec = d == me ? self_out : out;
  const uint64_t base = static_cast<uint64_t>(d) * (cap + 1ull);
  const uint32_t c = cnt[d];
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    rec[base] = make_uint3(c | (ovf ? 0x80000000u : 0u), n, kPadRank);
    if (d == 0) {
      summary[3] = sent;
      summary[4] = 0u;
      if (world == 1) {  // nothing to receive: the owner's summary is this one
        summary[0] = ovf ? 1u : 0u;
        summary[1] = n;
        summary[2] = sent;
      }
      if (zero3) zero3[0] = zero3[1] = zero3[2] = 0u;
    }
  }
  // the next call's reservation cursors (the previous call used them; this
  // call's stay untouched while its blocks read them)
  if (blockIdx.x == 0 && threadIdx.x == 0) next_cursor[d] = 0u;
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * 256;
  for (uint64_t j = min(c, cap) + static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x; j < cap;
       j += stride)
    rec[base + 1 + j] = make_uint3(0u, 0u, kPadRank);
}

// Owner side, after the records arrived: summary[0] = some source overflowed
// (the same on every rank), [1] = the largest source n, [2] = rows received.
__global__ void k_recv_summary(const uint3* __restrict__ rrec, uint32_t world, uint32_t cap,
                               uint32_t* __restrict__ summary) {
  const uint32_t p = threadIdx.x;
  uint32_t ovf = 0, nmax = 0, rows = 0;
  if (p < world) {
    const uint3 h = rrec[static_cast<uint64_t>(p) * (cap + 1ull)];
    ovf = h.x >> 31;
    nmax = h.y;
    rows = min(h.x & 0x7FFFFFFFu, cap);
  }
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) {
    ovf |= __shfl_xor(ovf, s);
    nmax = max(nmax, __shfl_xor(nmax, s));
    rows += __shfl_xor(rows, s);
  }
  if (p == 0) {
    summary[0] = ovf;
    summary[1] = nmax;
    summary[2] = rows;
  }
}

// Compact return leg of the exchange (round 4): an owner sends back only the
// received rows whose rep is not their own rank, as {index of the row inside
// its (source -> owner) message, rep} -- 8 B per linked row instead of 4 B
// per row.  Tiles of kRetTile received rows never straddle a source's
// segment (the host lays them out per segment, RetTiles), so the pairs come
// out grouped by source in row order: the shared tile compaction
// (compact_device.hpp) per segment.
constexpr int kRetThreads = compact::kThreads;
constexpr int kRetRows = compact::kRows;
constexpr uint32_t kRetTile = compact::kTile;
static_assert(kRetTile == kRetTileRows, "the host lays the tiles out");

__device__ __forceinline__ uint32_t ret_segment(const RetTiles& st, uint32_t blk) {
  uint32_t p = 0;
  while (p + 1 < st.world && st.tstart[p + 1] <= blk) ++p;
  return p;
}

__global__ __launch_bounds__(kRetThreads) void k_ret_count(RetTiles st, const uint3* __restrict__ rrec,
                                                           const uint32_t* __restrict__ rrep,
                                                           uint32_t* __restrict__ cnt) {
  const uint32_t blk = blockIdx.x;
  uint32_t f = 0;
  if (blk < st.tstart[st.world]) {
    const uint32_t p = ret_segment(st, blk);
    const uint32_t k0 = st.roff[p] + (blk - st.tstart[p]) * kRetTile, k1 = st.roff[p + 1];
#pragma unroll
    for (int u = 0; u < kRetRows; ++u) {
      const uint32_t k = k0 + u * kRetThreads + threadIdx.x;
      if (k < k1) f |= (rrep[k] != rrec[k].z ? 1u : 0u) << u;
    }
  }
  const uint32_t c = compact::tile_count(f);
  if (threadIdx.x == 0) cnt[blk] = c;
}

// cnt: exclusive scan of the tile counts (cnt[tiles] = total).  retcnt[p] =
// pairs for source p (int64, the count exchange's unit).
__global__ __launch_bounds__(kRetThreads) void k_ret_write(RetTiles st, const uint3* __restrict__ rrec,
                                                           const uint32_t* __restrict__ rrep,
                                                           const uint32_t* __restrict__ cnt,
                                                           uint2* __restrict__ ret,
                                                           int64_t* __restrict__ retcnt) {
  __shared__ uint32_t oc[kRetRows][compact::kWaves];
  const uint32_t blk = blockIdx.x, w = threadIdx.x >> 6;
  if (blk == 0 && threadIdx.x < st.world)
    retcnt[threadIdx.x] = static_cast<int64_t>(cnt[st.tstart[threadIdx.x + 1]]) -
                          static_cast<int64_t>(cnt[st.tstart[threadIdx.x]]);
  if (blk >= st.tstart[st.world]) return;  // the one block of an empty receive
  const uint32_t p = ret_segment(st, blk);
  const uint32_t k0 = st.roff[p] + (blk - st.tstart[p]) * kRetTile, k1 = st.roff[p + 1];
  uint32_t f = 0, v[kRetRows], pr[kRetRows];
#pragma unroll
  for (int u = 0; u < kRetRows; ++u) {
    const uint32_t k = k0 + u * kRetThreads + threadIdx.x;
    const uint32_t kk = k < k1 ? k : k1 - 1;
    v[u] = rrep[kk];
    f |= (k < k1 && v[u] != rrec[kk].z ? 1u : 0u) << u;
  }
  // index inside the segment's pairs
  compact::tile_offsets(f, [&] { return cnt[blk] - cnt[st.tstart[p]]; }, oc, pr);
  const uint32_t seg0 = cnt[st.tstart[p]];
#pragma unroll
  for (int u = 0; u < kRetRows; ++u)
    if (f >> u & 1u) {
      const uint32_t k = k0 + u * kRetThreads + threadIdx.x;
      ret[seg0 + oc[u][w] + pr[u]] = make_uint2(k - st.roff[p], v[u]);
    }
}

// Source side: back[soff[d] + idx] = rep for every pair received from owner d
// (pairs of d at [poff[d], poff[d + 1]) of rback); back was set to ~0.
__global__ __launch_bounds__(256) void k_ret_apply(RetApply ap, const uint2* __restrict__ rback,
                                                   uint32_t* __restrict__ back) {
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * 256;
  const uint64_t total = ap.poff[ap.world];
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x; i < total; i += stride) {
    uint32_t d = 0;
    while (d + 1 < ap.world && ap.poff[d + 1] <= i) ++d;
    const uint2 q = rback[i];
    back[ap.soff[d] + q.x] = q.y;
  }
}

size_t shard_hist_bytes(uint32_t shard_bits) {
  const uint64_t nh = (static_cast<uint64_t>(1) << shard_bits) * kPartBlocks;
  return align_up(4 * (nh + 1), 256);
}

// Shard histogram + scan (+ scatter when outputs are given) of the caller's
// rows; digit = destination rank when world != 0, else the top shard_bits.
// ws: the histogram (scanned in place: the offsets), then the scan's tiles.
hipError_t shard_partition(const RowsIn& in, uint64_t n, uint32_t shard_bits, uint32_t world,
                           void* ws, uint64_t* okey, uint32_t* orank, uint3* orec, uint32_t* opos,
                           hipStream_t s, KTimer* timer) {
  uint32_t* hist = static_cast<uint32_t*>(ws);
  uint32_t* tiles = hist + shard_hist_bytes(shard_bits) / 4;
  const uint32_t nbins = world ? world : 1u << shard_bits;
  const uint64_t nh = static_cast<uint64_t>(nbins) * kPartBlocks;
  const size_t lds = sizeof(uint32_t) * nbins;
  {
    KScope k(timer, "shard_hist", s);
    k_part_hist<RowsIn><<<kPartBlocks, kPartThreads, lds, s>>>(in, n, 0, shard_bits, world, hist);
  }
  scan::exclusive(hist, nh, hist, tiles, nullptr, s);
  if (opos || orec) {
    KScope k(timer, "shard_scatter", s);
    if (orec)
      k_part_scatter<RowsIn, true><<<kPartBlocks, kPartThreads, lds, s>>>(
          in, n, 0, shard_bits, world, hist, nullptr, nullptr, orec, opos);
    else
      k_part_scatter<RowsIn, false><<<kPartBlocks, kPartThreads, lds, s>>>(
          in, n, 0, shard_bits, world, hist, okey, orank, nullptr, opos);
  }
  return hipGetLastError();
}

}  // namespace

size_t shard_workspace_bytes(uint32_t shard_bits) {
  const uint64_t nh = (static_cast<uint64_t>(1) << shard_bits) * kPartBlocks;
  return shard_hist_bytes(shard_bits) + align_up(4 * (scan::tiles_for(nh) + 1), 256) +
         align_up(8 * (static_cast<uint64_t>(1) << shard_bits), 256);
}

hipError_t shard_count_launch(const uint64_t* key, const uint8_t* has_key, uint64_t n,
                              uint32_t shard_bits, uint64_t* d_counts, void* ws, hipStream_t s) {
  hipError_t e = shard_partition(RowsIn{key, has_key, nullptr, 0}, n, shard_bits, 0, ws, nullptr,
                                 nullptr, nullptr, nullptr, s, nullptr);
  if (e != hipSuccess) return e;
  k_copy_counts<<<1, 256, 0, s>>>(static_cast<const uint32_t*>(ws), 1u << shard_bits, d_counts);
  return hipGetLastError();
}

hipError_t shard_partition_launch(const uint64_t* key, const uint8_t* has_key,
                                  const uint32_t* rank, uint64_t n, uint32_t shard_bits,
                                  uint64_t* out_key, uint32_t* out_rank, uint32_t* out_pos,
                                  void* ws, hipStream_t s, KTimer* timer) {
  return shard_partition(RowsIn{key, has_key, rank, 0}, n, shard_bits, 0, ws, out_key, out_rank,
                         nullptr, out_pos, s, timer);
}

hipError_t shard_exchange_launch(const uint64_t* key, const uint8_t* has_key,
                                 const uint32_t* rank, uint64_t n, uint32_t shard_bits,
                                 uint32_t world, uint64_t* out_key, uint32_t* out_rank,
                                 uint32_t* out_rec12, uint32_t* out_pos, int64_t* d_dest_counts,
                                 void* ws, hipStream_t s, KTimer* timer, int64_t* d_count_msgs,
                                 int64_t msg_code) {
  hipError_t e = shard_partition(RowsIn{key, has_key, rank, 0}, n, shard_bits, world, ws, out_key,
                                 out_rank, reinterpret_cast<uint3*>(out_rec12), out_pos, s, timer);
  if (e != hipSuccess) return e;
  k_dest_counts<<<1, 64, 0, s>>>(static_cast<const uint32_t*>(ws), world, d_dest_counts,
                                 d_count_msgs, static_cast<int64_t>(n), msg_code);
  return hipGetLastError();
}

uint32_t ret_tiles(const RetTiles& st) { return st.tstart[st.world]; }

size_t ret_workspace_bytes(uint32_t tiles) {
  return align_up(4ull * (tiles + 2), 256) + align_up(4ull * (scan::tiles_for(tiles + 1) + 1), 256);
}

hipError_t ret_compact_launch(const RetTiles& st, const uint32_t* rrec, const uint32_t* rrep,
                              uint2* ret, int64_t* retcnt, void* ws, hipStream_t s, KTimer* timer) {
  const uint32_t nt = st.tstart[st.world];
  uint8_t* b = static_cast<uint8_t*>(ws);
  uint32_t* cnt = reinterpret_cast<uint32_t*>(b);
  uint32_t* tiles = reinterpret_cast<uint32_t*>(b + align_up(4ull * (nt + 2), 256));
  KScope k(timer, "ret_compact", s);
  const uint32_t g = nt ? nt : 1;  // one block writes the (zero) counts of an empty receive
  const uint3* rr = reinterpret_cast<const uint3*>(rrec);
  if (nt) {
    k_ret_count<<<nt, kRetThreads, 0, s>>>(st, rr, rrep, cnt);
    scan::exclusive(cnt, nt, cnt, tiles, nullptr, s);
  } else {
    const hipError_t e = hipMemsetAsync(cnt, 0, 4, s);
    if (e != hipSuccess) return e;
  }
  k_ret_write<<<g, kRetThreads, 0, s>>>(st, rr, rrep, cnt, ret, retcnt);
  return hipGetLastError();
}

hipError_t ret_apply_launch(const RetApply& ap, const uint2* rback, uint32_t* back,
                            uint64_t n_back, const uint32_t* srec12, hipStream_t s) {
  if (n_back) {
    const uint64_t g = std::min<uint64_t>((n_back + 255) / 256, 16384);
    k_back_init<<<static_cast<uint32_t>(g), 256, 0, s>>>(reinterpret_cast<const uint3*>(srec12),
                                                         n_back, back);
  }
  const uint64_t total = ap.poff[ap.world];
  if (total) {
    const uint64_t g = std::min<uint64_t>((total + 255) / 256, 16384);
    k_ret_apply<<<static_cast<uint32_t>(g), 256, 0, s>>>(ap, rback, back);
  }
  return hipGetLastError();
}

hipError_t gather_rep_launch(const uint32_t* back, const uint32_t* pos, const uint32_t* rank,
                             uint64_t n, uint32_t* rep, hipStream_t s, const uint32_t* self,
                             uint64_t self_lo, uint64_t self_hi) {
  if (n) {
    const uint64_t g = std::min<uint64_t>((n + 255) / 256, 16384);
    k_gather_rep<<<static_cast<uint32_t>(g), 256, 0, s>>>(
        back, pos, rank, n, rep, self ? self : back, static_cast<uint32_t>(self_lo),
        static_cast<uint32_t>(self ? self_hi : self_lo));
  }
  return hipGetLastError();
}

hipError_t padded_partition_launch(const uint64_t* key, const uint8_t* has_key,
                                   const uint32_t* rank, uint64_t n, uint32_t world, uint32_t me,
                                   uint32_t cap, uint32_t* out_rec12, uint32_t* self_rec12,
                                   uint32_t* out_pos, uint32_t* cursor, const KeylessSink* sink,
                                   hipStream_t s, KTimer* timer) {
  if (n) {
    KScope k(timer, "shard_padded", s);
    k_part_padded<<<kPartBlocks, kPartThreads, 0, s>>>(
        RowsIn{key, has_key, rank, 0}, n, world, me, cap, reinterpret_cast<uint3*>(out_rec12),
        reinterpret_cast<uint3*>(self_rec12), out_pos, cursor, sink ? *sink : KeylessSink{});
  } else if (sink) {  // no rows: the segments are empty
    const hipError_t e =
        hipMemsetAsync(sink->cnt, 0, 4ull * keyless_sink_segments(), s);
    if (e != hipSuccess) return e;
  }
  return hipGetLastError();
}

uint32_t keyless_sink_segments() { return kPartBlocks * kSinkWaves; }
uint32_t keyless_sink_cap(uint64_t n) { return sink_cap(n); }

hipError_t pad_fill_launch(const uint32_t* cursor, uint32_t world, uint32_t me, uint32_t cap,
                           uint64_t n, uint32_t* rec12, uint32_t* self_rec12, uint32_t* summary,
                           uint32_t* zero3, uint32_t* next_cursor, hipStream_t s) {
  const uint32_t bx = std::min<uint32_t>(64u, (cap + 1023u) / 1024u + 1u);
  k_pad_fill<<<dim3(bx, world), 256, 0, s>>>(cursor, world, me, cap, static_cast<uint32_t>(n),
                                             reinterpret_cast<uint3*>(rec12),
                                             reinterpret_cast<uint3*>(self_rec12), summary, zero3,
                                             next_cursor);
  return hipGetLastError();
}

hipError_t recv_summary_launch(const uint32_t* rrec12, uint32_t world, uint32_t cap,
                               uint32_t* summary, hipStream_t s) {
  k_recv_summary<<<1, 64, 0, s>>>(reinterpret_cast<const uint3*>(rrec12), world, cap, summary);
  return hipGetLastError();
}

hipError_t scatter_rep_launch(const uint32_t* src, const uint32_t* pos, uint64_t n, uint32_t* dst,
                              uint64_t n_dst, const uint32_t* init, bool do_init, hipStream_t s) {
  if (do_init && n_dst) {
    const uint64_t g = std::min<uint64_t>((n_dst + 255) / 256, 16384);
    k_fill_init<<<static_cast<uint32_t>(g), 256, 0, s>>>(dst, n_dst, init);
  }
  if (n) {
    const uint64_t g = std::min<uint64_t>((n + 255) / 256, 16384);
    k_scatter<<<static_cast<uint32_t>(g), 256, 0, s>>>(src, pos, n, dst);
  }
  return hipGetLastError();
}

}  // namespace sdgpu
