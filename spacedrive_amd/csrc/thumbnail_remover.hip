// Thumbnail remover: the stale-thumbnail sweep as one device
// anti-join.
//
// Reference: core/src/object/thumbnail_remover.rs:236-367 (process_clean_up).
// Every half hour, for every shard directory of the thumbnail cache, it asks
// every loaded library `file_path.cas_id IN (the directory's <cas_id>.webp
// stems)` -- a full table scan per directory and library, the schema has no
// index on cas_id -- drops the stems the in-memory set of non-indexed
// thumbnails holds, unlinks the rest, and removes a directory when everything
// it found there went.
//
// Here the table is built on the SMALL side: the thumbnail keys go into a key
// set in the context's workspace (keyset_device.hpp: 8-byte slots, the key ~0
// owns the slot one past the table), every thumbnail remembers the slot it
// ended in (slot_of), and the LARGE side -- the cas key columns of the
// file_paths, plus the non-indexed set as one more column -- is streamed once:
// a row whose key sits in the table stores hit[slot] = 1, a plain byte store
// (idempotent: no atomics in that pass); a one-bit-per-hash filter in front of
// the table keeps most rows that own no thumbnail out of it (k_stale_probe).
// The thumbnails whose slot was not hit are then compacted in list order (the
// shared tile compaction of compact_device.hpp), and every directory boundary
// gets its offset into that list from its tile's offset plus a count of the
// tile's rows before it.  A key listed twice (a misplaced copy in a
// second directory) ends in one slot, so both copies get one answer.
//
// The same table answers the opposite question, which file_paths still need a
// thumbnail (thumbnailer.hip): k_thumb_present probes it per row.
#include "compact_device.hpp"
#include "internal.hpp"
#include "keyset_device.hpp"
#include "scan_device.hpp"

namespace sdgpu {

namespace {

using compact::kRows;
using compact::kThreads;
using compact::kTile;
using compact::kWaves;
constexpr uint32_t kMaxGrid = 2048;

struct StaleWs {
  uint64_t cap;       // slots; the key ~0 owns slot `cap`
  uint64_t* table;    // [cap]
  uint8_t* hit;       // [cap + 2]; hit[cap + 1]: a thumbnail key is ~0 (set by the build)
  uint32_t* bits;     // [cap / 4] the probe's filter: a bit per thumbnail key's hash
  uint32_t* slot_of;  // [n]
  uint32_t* cnt;      // [blocks + 1] stale per tile, then their offsets
  uint32_t* tiles;    // scan::exclusive's tile sums
  size_t bytes;
};

StaleWs stale_ws(uint64_t n, void* ws) {
  StaleWs w;
  w.cap = keyset_cap(n);
  const uint64_t blocks = compact::tiles_for(n);
  Carve c(ws);
  w.table = c.take<uint64_t>(w.cap);
  w.hit = c.take(w.cap + 2);
  w.bits = c.take<uint32_t>(w.cap / 4);
  w.slot_of = c.take<uint32_t>(n);
  w.cnt = c.take<uint32_t>(blocks + 1);
  w.tiles = c.take<uint32_t>(static_cast<size_t>(scan::tiles_for(blocks)) + 1);
  w.bytes = c.bytes();
  return w;
}

// slot_of[i] = the slot thumbnail key[i] ends in (keyset_insert).
// Also sets the key's filter bit (one atomicOr per thumbnail), and for the key
// ~0, which has no slot in the table, the byte hit[cap + 1] that tells
// k_thumb_present the thumbnail exists (a plain byte store, idempotent).
__global__ __launch_bounds__(kThreads) void k_stale_build(const uint64_t* __restrict__ key,
                                                          uint64_t n, uint64_t* __restrict__ table,
                                                          uint64_t cap,
                                                          uint32_t* __restrict__ bits,
                                                          uint32_t* __restrict__ slot_of,
                                                          uint8_t* __restrict__ hit) {
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kThreads;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x; i < n;
       i += stride) {
    const uint64_t k = key[i];
    uint64_t h = cap;
    if (k != kEmptyKey) {
      const uint64_t hb = row_hash(k) & (8 * cap - 1);
      atomicOr(&bits[hb >> 5], 1u << (hb & 31));
      h = keyset_insert(table, cap, k);
    } else {
      hit[cap + 1] = 1;
    }
    slot_of[i] = static_cast<uint32_t>(h);
  }
}

// One pass over a file_path column, one lane per row, kPRows rows per thread:
// keys, has_key bytes and the rows' filter words are loaded unconditionally
// (rows past the end read the last row) and masked afterwards, so a thread's
// loads are in flight together (the RowBatch / k_mark idiom).  Only a row whose
// filter bit is set reads the table, and only a probe that has to walk on
// reads it again.  kHas = false: every row is keyed.
//
// The filter: bit (row_hash(key) & (8 cap - 1)) of `bits` is set for every
// thumbnail key -- 16 bits or more per thumbnail, so 15 of 16 rows that own no
// thumbnail stop at a word of a map of cap BYTES (2 MiB at 1 M thumbnails,
// which an XCD's 4 MiB L2 holds) instead of pulling a line of the 8 x larger
// table out of the Infinity Cache for 8 useful bytes.  Measured at 1 M
// thumbnails, 30 % of the rows owning one: 100 M rows 2.58 -> 1.85 ms,
// 12.5 M rows 0.53 -> 0.43 ms.
constexpr int kPRows = 4;
template <bool kHas>
__global__ __launch_bounds__(kThreads) void k_stale_probe(const uint64_t* __restrict__ key,
                                                          const uint8_t* __restrict__ has,
                                                          uint64_t n,
                                                          const uint64_t* __restrict__ table,
                                                          uint64_t cap,
                                                          const uint32_t* __restrict__ bits,
                                                          uint8_t* __restrict__ hit) {
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kThreads * kPRows;
  for (uint64_t i0 = static_cast<uint64_t>(blockIdx.x) * kThreads * kPRows + threadIdx.x; i0 < n;
       i0 += stride) {
    uint64_t k[kPRows], h[kPRows], s[kPRows];
    uint32_t w[kPRows];
    uint8_t b[kPRows];
    bool live[kPRows];
#pragma unroll
    for (int u = 0; u < kPRows; ++u)
      k[u] = key[min(i0 + static_cast<uint64_t>(u) * kThreads, n - 1)];
#pragma unroll
    for (int u = 0; u < kPRows; ++u)
      b[u] = kHas ? has[min(i0 + static_cast<uint64_t>(u) * kThreads, n - 1)] : uint8_t(1);
#pragma unroll
    for (int u = 0; u < kPRows; ++u) {
      h[u] = row_hash(k[u]);
      w[u] = bits[(h[u] & (8 * cap - 1)) >> 5];
    }
#pragma unroll
    for (int u = 0; u < kPRows; ++u) {
      live[u] = i0 + static_cast<uint64_t>(u) * kThreads < n && b[u] != 0;
      if (live[u] && k[u] == kEmptyKey) hit[cap] = 1;
      live[u] = live[u] && k[u] != kEmptyKey && (w[u] >> (h[u] & 31) & 1u);
      h[u] &= cap - 1;
    }
#pragma unroll
    for (int u = 0; u < kPRows; ++u) s[u] = live[u] ? table[h[u]] : kEmptyKey;
#pragma unroll
    for (int u = 0; u < kPRows; ++u) {
      if (!live[u]) continue;
      const uint64_t slot = keyset_find(table, cap, k[u], h[u], s[u]);
      if (slot != ~0ull) hit[slot] = 1;
    }
  }
}

// The probe in the other direction (the thumbnailer's work list,
// thumbnailer.hip): a per-row answer instead of hit[slot].  Same loads, filter
// bit first, same walk; a block's threads share their trip count, so every
// ballot is of whole waves.  Per row two plain coalesced byte stores:
//   present[i] = keyed and the key is among the thumbnail keys (the key ~0:
//                hit[cap + 1], which the build set);
//   cand[i]    = keyed, eligible, and (not present or regen)  (cand non-null).
// stats (zeroed by the caller) += [0] present rows, and with cand [1] keyed
// eligible rows, [2] those of them that are present: wave ballots, summed per
// block, one atomic per block and counter.  kHas / kElig = false: every row is
// keyed / eligible.
template <bool kHas, bool kElig>
__global__ __launch_bounds__(kThreads) void k_thumb_present(const uint64_t* __restrict__ key,
                                                            const uint8_t* __restrict__ has,
                                                            const uint8_t* __restrict__ elig,
                                                            uint64_t n,
                                                            const uint64_t* __restrict__ table,
                                                            uint64_t cap,
                                                            const uint32_t* __restrict__ bits,
                                                            const uint8_t* __restrict__ hit,
                                                            bool regen,
                                                            uint8_t* __restrict__ present,
                                                            uint8_t* __restrict__ cand,
                                                            uint32_t* __restrict__ stats) {
  __shared__ uint32_t sw[kThreads / 64][3];
  const bool special = hit[cap + 1] != 0;
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kThreads * kPRows;
  uint32_t c0 = 0, c1 = 0, c2 = 0;  // wave-uniform
  for (uint64_t base = static_cast<uint64_t>(blockIdx.x) * kThreads * kPRows; base < n;
       base += stride) {
    const uint64_t i0 = base + threadIdx.x;
    uint64_t k[kPRows], h[kPRows], s[kPRows];
    uint32_t w[kPRows];
    uint8_t b[kPRows], e[kPRows];
    bool in[kPRows], keyed[kPRows], live[kPRows];
#pragma unroll
    for (int u = 0; u < kPRows; ++u)
      k[u] = key[min(i0 + static_cast<uint64_t>(u) * kThreads, n - 1)];
#pragma unroll
    for (int u = 0; u < kPRows; ++u)
      b[u] = kHas ? has[min(i0 + static_cast<uint64_t>(u) * kThreads, n - 1)] : uint8_t(1);
#pragma unroll
    for (int u = 0; u < kPRows; ++u)
      e[u] = kElig ? elig[min(i0 + static_cast<uint64_t>(u) * kThreads, n - 1)] : uint8_t(1);
#pragma unroll
    for (int u = 0; u < kPRows; ++u) {
      h[u] = row_hash(k[u]);
      w[u] = bits[(h[u] & (8 * cap - 1)) >> 5];
    }
#pragma unroll
    for (int u = 0; u < kPRows; ++u) {
      in[u] = i0 + static_cast<uint64_t>(u) * kThreads < n;
      keyed[u] = in[u] && b[u] != 0;
      live[u] = keyed[u] && k[u] != kEmptyKey && (w[u] >> (h[u] & 31) & 1u);
      h[u] &= cap - 1;
    }
#pragma unroll
    for (int u = 0; u < kPRows; ++u) s[u] = live[u] ? table[h[u]] : kEmptyKey;
#pragma unroll
    for (int u = 0; u < kPRows; ++u) {
      bool p = keyed[u] && k[u] == kEmptyKey && special;
      if (live[u] && keyset_find(table, cap, k[u], h[u], s[u]) != ~0ull) p = true;
      const bool q = keyed[u] && e[u] != 0;
      if (in[u]) {
        const uint64_t i = i0 + static_cast<uint64_t>(u) * kThreads;
        present[i] = p ? 1 : 0;
        if (cand) cand[i] = q && (!p || regen) ? 1 : 0;
      }
      c0 += __popcll(__ballot(p));
      c1 += __popcll(__ballot(q));
      c2 += __popcll(__ballot(q && p));
    }
  }
  if (__lane_id() == 0) {
    sw[threadIdx.x >> 6][0] = c0;
    sw[threadIdx.x >> 6][1] = c1;
    sw[threadIdx.x >> 6][2] = c2;
  }
  __syncthreads();
  if (threadIdx.x < (cand ? 3u : 1u)) {
    uint32_t t = 0;
    for (int v = 0; v < kThreads / 64; ++v) t += sw[v][threadIdx.x];
    if (t) atomicAdd(&stats[threadIdx.x], t);
  }
}

// The thumbnail list in tiles of kRows x kThreads positions: position
// tile + k * kThreads + t, and (k, t) order is list order.  Bit k of the
// result: this thread's k-th thumbnail is stale (its slot was not hit).
__device__ __forceinline__ uint32_t stale_bits(const uint32_t* __restrict__ slot_of, uint64_t n,
                                               uint64_t tile, const uint8_t* __restrict__ hit) {
  uint32_t sl[kRows];
  uint8_t m[kRows];
#pragma unroll
  for (int k = 0; k < kRows; ++k) sl[k] = slot_of[min(tile + k * kThreads + threadIdx.x, n - 1)];
#pragma unroll
  for (int k = 0; k < kRows; ++k) m[k] = hit[sl[k]];
  uint32_t f = 0;
#pragma unroll
  for (int k = 0; k < kRows; ++k)
    f |= (tile + k * kThreads + threadIdx.x < n && m[k] == 0 ? 1u : 0u) << k;
  return f;
}

__global__ __launch_bounds__(kThreads) void k_stale_count(const uint32_t* __restrict__ slot_of,
                                                          uint64_t n,
                                                          const uint8_t* __restrict__ hit,
                                                          uint32_t* __restrict__ cnt) {
  const uint64_t tile = static_cast<uint64_t>(blockIdx.x) * kTile;
  const uint32_t t = compact::tile_count(stale_bits(slot_of, n, tile, hit));
  if (threadIdx.x == 0) cnt[blockIdx.x] = t;
}

// stable compaction: tile b writes the positions of its stale thumbnails from
// the scanned offset, in order
__global__ __launch_bounds__(kThreads) void k_stale_write(const uint32_t* __restrict__ slot_of,
                                                          uint64_t n,
                                                          const uint8_t* __restrict__ hit,
                                                          const uint32_t* __restrict__ offs,
                                                          uint32_t* __restrict__ out) {
  __shared__ uint32_t off[kRows][kWaves];
  const uint64_t tile = static_cast<uint64_t>(blockIdx.x) * kTile;
  const uint32_t w = threadIdx.x >> 6;
  const uint32_t f = stale_bits(slot_of, n, tile, hit);
  uint32_t pre[kRows];
  compact::tile_offsets(f, [&] { return offs[blockIdx.x]; }, off, pre);
#pragma unroll
  for (int k = 0; k < kRows; ++k)
    if (f >> k & 1u)
      out[off[k][w] + pre[k]] = static_cast<uint32_t>(tile + k * kThreads + threadIdx.x);
}

// stale_start[d] = stale thumbnails before position dir_start[d]: the offset
// of the boundary's tile plus the stale ones of that tile before the boundary
// (at most a tile's rows, one wave per boundary).  A boundary past the list
// (an inconsistent dir_start) counts as the list's end.
__global__ __launch_bounds__(kThreads) void k_stale_dirs(const uint32_t* __restrict__ slot_of,
                                                         uint64_t n,
                                                         const uint8_t* __restrict__ hit,
                                                         const uint32_t* __restrict__ offs,
                                                         const uint32_t* __restrict__ dir_start,
                                                         uint64_t n_bounds,
                                                         uint32_t* __restrict__ stale_start) {
  const uint32_t lane = __lane_id();
  const uint64_t waves = static_cast<uint64_t>(gridDim.x) * kWaves;
  for (uint64_t d = static_cast<uint64_t>(blockIdx.x) * kWaves + (threadIdx.x >> 6); d < n_bounds;
       d += waves) {
    const uint64_t p = min(static_cast<uint64_t>(dir_start[d]), n);
    const uint64_t t = p / kTile;
    uint32_t c = 0;
    for (uint64_t i = t * kTile + lane; i < p; i += 64) c += hit[slot_of[i]] == 0 ? 1u : 0u;
    c = compact::wave_sum(c);
    if (lane == 0) stale_start[d] = offs[t] + c;
  }
}

}  // namespace

size_t stale_workspace_bytes(uint64_t n_thumbs) { return stale_ws(n_thumbs, nullptr).bytes; }

hipError_t stale_build_launch(const uint64_t* thumb_key, uint64_t n, void* ws, hipStream_t s) {
  const StaleWs w = stale_ws(n, ws);
  // every call clears its own table: the workspace is shared and may hold anything
  hipError_t e = hipMemsetAsync(w.table, 0xFF, 8 * w.cap, s);
  if (e != hipSuccess) return e;
  e = hipMemsetAsync(w.hit, 0, w.cap + 2, s);
  if (e != hipSuccess) return e;
  e = hipMemsetAsync(w.bits, 0, w.cap, s);
  if (e != hipSuccess) return e;
  if (n) k_stale_build<<<grid_for(n, kThreads, kMaxGrid), kThreads, 0, s>>>(thumb_key, n, w.table, w.cap,
                                                                   w.bits, w.slot_of, w.hit);
  return hipGetLastError();
}

hipError_t stale_probe_launch(uint64_t n_thumbs, const uint64_t* col_key, const uint8_t* col_has,
                              uint64_t rows, void* ws, hipStream_t s) {
  if (rows == 0) return hipSuccess;
  const StaleWs w = stale_ws(n_thumbs, ws);
  const uint32_t grid = grid_for(rows, kThreads * kPRows, kMaxGrid);
  if (col_has)
    k_stale_probe<true><<<grid, kThreads, 0, s>>>(col_key, col_has, rows, w.table, w.cap, w.bits,
                                                  w.hit);
  else
    k_stale_probe<false><<<grid, kThreads, 0, s>>>(col_key, nullptr, rows, w.table, w.cap, w.bits,
                                                   w.hit);
  return hipGetLastError();
}

hipError_t thumb_present_launch(uint64_t n_thumbs, const uint64_t* key, const uint8_t* has,
                                const uint8_t* elig, uint64_t rows, bool regen, uint8_t* present,
                                uint8_t* cand, uint32_t* stats, void* ws, hipStream_t s,
                                KTimer* timer) {
  if (rows == 0) return hipSuccess;
  const StaleWs w = stale_ws(n_thumbs, ws);
  const uint32_t grid = grid_for(rows, kThreads * kPRows, kMaxGrid);
  KScope k(timer, "thumb_present", s);
#define SD_THUMB_PRESENT(H, E)                                                                   \
  k_thumb_present<H, E><<<grid, kThreads, 0, s>>>(key, has, elig, rows, w.table, w.cap, w.bits, \
                                                  w.hit, regen, present, cand, stats)
  if (has && elig) SD_THUMB_PRESENT(true, true);
  else if (has) SD_THUMB_PRESENT(true, false);
  else if (elig) SD_THUMB_PRESENT(false, true);
  else SD_THUMB_PRESENT(false, false);
#undef SD_THUMB_PRESENT
  return hipGetLastError();
}

hipError_t stale_compact_launch(uint64_t n, const uint32_t* dir_start, uint32_t n_dirs,
                                uint32_t* stale, uint32_t* stale_start, void* ws, hipStream_t s) {
  const StaleWs w = stale_ws(n, ws);
  const uint64_t blocks = compact::tiles_for(n);
  const uint64_t bounds = static_cast<uint64_t>(n_dirs) + 1;
  if (blocks == 0) return hipMemsetAsync(stale_start, 0, 4 * bounds, s);
  k_stale_count<<<static_cast<uint32_t>(blocks), kThreads, 0, s>>>(w.slot_of, n, w.hit, w.cnt);
  scan::exclusive(w.cnt, blocks, w.cnt, w.tiles, nullptr, s);
  k_stale_write<<<static_cast<uint32_t>(blocks), kThreads, 0, s>>>(w.slot_of, n, w.hit, w.cnt,
                                                                   stale);
  k_stale_dirs<<<grid_for(bounds, kWaves, kMaxGrid), kThreads, 0, s>>>(w.slot_of, n, w.hit, w.cnt,
                                                              dir_start, bounds, stale_start);
  return hipGetLastError();
}

}  // namespace sdgpu
