// Indexer: the rescan diff (to_create / to_update / to_remove) of one location
// as one device join.
//
// Reference: core/src/location/indexer/walk.rs:309-381 (filter_existing_paths)
// fetches the file_path rows of the walked entries with an OR of 4-term ANDs
// per 200 paths (indexer/mod.rs:305-331), probes a HashMap keyed by
// IsolatedFilePathData per entry, and compares inode, device and date_modified
// (:349-369); walk.rs:624-636 asks per walked directory which rows of that
// directory were not found (`id NOT IN (...)`, indexer/mod.rs:338-388).
//
// Here: the rows' keys go into a key set in the context's workspace
// (keyset_device.hpp: 8-byte slots, the key ~0 owns the slot one past the
// table); every slot keeps the lowest row that holds its key (first_row,
// atomicMin) and every row the slot it ended in (slot_of).  The walked
// directories go into a second, small key set.  Then
//   k_idx_probe  one lane per walked entry: match, state, and hit[slot] = 1 (a
//                plain byte store, idempotent) for entries that were in their
//                parent's listing;
//   k_idx_rows   one lane per row: remove_flag = directory walked && !hit;
//   k_idx_count / scan / k_idx_write: the three lists as ONE compaction
//                (compact_device.hpp) -- the tiles of create, update and
//                remove are laid behind one another, counted, scanned once,
//                and every list's offsets and length are differences of that
//                one scan.
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
constexpr uint32_t kMiss = 0xFFFFFFFFu;
constexpr uint32_t kMaxGrid = 2048;

constexpr uint8_t kIsDir = 1, kAncestor = 2, kNoMetadata = 2;
constexpr uint8_t kCreate = 0, kUnchanged = 1, kUpdate = 2, kKindChanged = 3;

struct IdxWs {
  uint64_t cap, dcap;    // slots of the row table / the directory set
  // one 0xFF fill: table | dtable | first_row
  uint64_t* table;       // [cap]
  uint64_t* dtable;      // [dcap]
  uint32_t* first_row;   // [cap + 1]; [cap]: the key ~0
  size_t fill_bytes;
  // one zero fill: hit[cap] the key ~0's rows were walked; hit[cap + 1] a
  // walked directory's key is ~0
  uint8_t* hit;          // [cap + 2]
  uint32_t* slot_of;     // [n_r]
  uint8_t* remove_flag;  // [n_r]
  uint64_t bw, br;       // tiles of the walked entries / the rows
  uint32_t* cnt;         // [2 bw + br + 1] per tile: create | update | remove, then offsets
  uint32_t* tiles;       // scan::exclusive's tile sums
  size_t bytes;
};

IdxWs idx_ws(uint64_t n_w, uint64_t n_wd, uint64_t n_r, void* ws) {
  IdxWs w;
  w.cap = keyset_cap(n_r);
  w.dcap = keyset_cap(n_wd);
  w.bw = compact::tiles_for(n_w);
  w.br = compact::tiles_for(n_r);
  Carve c(ws);
  w.table = c.take<uint64_t>(w.cap);
  w.dtable = c.take<uint64_t>(w.dcap);
  w.first_row = c.take<uint32_t>(w.cap + 1);
  w.fill_bytes = c.bytes();
  w.hit = c.take(w.cap + 2);
  w.slot_of = c.take<uint32_t>(n_r);
  w.remove_flag = c.take(n_r);
  const uint64_t blocks = 2 * w.bw + w.br;
  w.cnt = c.take<uint32_t>(blocks + 1);
  w.tiles = c.take<uint32_t>(static_cast<size_t>(scan::tiles_for(blocks)) + 1);
  w.bytes = c.bytes();
  return w;
}

// Items [0, n_r): slot_of[j] = the slot r_key[j] ends in (keyset_insert) and
// first_row[slot] = min(j).  Items [n_r, n_r + n_wd): the walked directories'
// keys into their set table.
__global__ __launch_bounds__(kThreads) void k_idx_build(const uint64_t* __restrict__ r_key,
                                                        uint64_t n_r,
                                                        const uint64_t* __restrict__ wd_key,
                                                        uint64_t n_wd, uint64_t* __restrict__ table,
                                                        uint64_t cap, uint64_t* __restrict__ dtable,
                                                        uint64_t dcap,
                                                        uint32_t* __restrict__ first_row,
                                                        uint32_t* __restrict__ slot_of,
                                                        uint8_t* __restrict__ hit) {
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kThreads;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x; i < n_r + n_wd;
       i += stride) {
    const bool row = i < n_r;
    const uint64_t k = row ? r_key[i] : wd_key[i - n_r];
    uint64_t* t = row ? table : dtable;
    const uint64_t c = row ? cap : dcap;
    uint64_t h = c;
    if (k != kEmptyKey) {
      h = keyset_insert(t, c, k);
    } else if (!row) {
      hit[cap + 1] = 1;
    }
    if (row) {
      atomicMin(&first_row[h], static_cast<uint32_t>(i));
      slot_of[i] = static_cast<uint32_t>(h);
    }
  }
}

// One lane per walked entry, kWRows entries per thread: key, flag byte, the
// 24-byte metadata and the key's home slot are loaded unconditionally (entries
// past the end read the last one) and masked afterwards, so a thread's loads
// are in flight together (the RowBatch / k_stale_probe idiom).  Only a hit
// reads first_row and the metadata of row j0.
constexpr int kWRows = 2;
template <bool kWF, bool kRF>
__global__ __launch_bounds__(kThreads) void k_idx_probe(
    const uint64_t* __restrict__ w_key, const uint8_t* __restrict__ w_flags,
    const uint64_t* __restrict__ w_meta, uint64_t n, const uint64_t* __restrict__ table,
    uint64_t cap, const uint32_t* __restrict__ first_row, const uint8_t* __restrict__ r_flags,
    const uint64_t* __restrict__ r_meta, uint8_t* __restrict__ hit, uint32_t* __restrict__ match,
    uint8_t* __restrict__ state) {
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kThreads * kWRows;
  for (uint64_t i0 = static_cast<uint64_t>(blockIdx.x) * kThreads * kWRows + threadIdx.x; i0 < n;
       i0 += stride) {
    uint64_t k[kWRows], h[kWRows], s[kWRows], m[kWRows][3];
    uint8_t f[kWRows];
#pragma unroll
    for (int u = 0; u < kWRows; ++u)
      k[u] = w_key[min(i0 + static_cast<uint64_t>(u) * kThreads, n - 1)];
#pragma unroll
    for (int u = 0; u < kWRows; ++u)
      f[u] = kWF ? w_flags[min(i0 + static_cast<uint64_t>(u) * kThreads, n - 1)] : uint8_t(0);
#pragma unroll
    for (int u = 0; u < kWRows; ++u) {
      const uint64_t* p = w_meta + 3 * min(i0 + static_cast<uint64_t>(u) * kThreads, n - 1);
      m[u][0] = p[0];
      m[u][1] = p[1];
      m[u][2] = p[2];
    }
#pragma unroll
    for (int u = 0; u < kWRows; ++u) {
      h[u] = row_hash(k[u]) & (cap - 1);
      s[u] = table[h[u]];
    }
#pragma unroll
    for (int u = 0; u < kWRows; ++u) {
      const uint64_t i = i0 + static_cast<uint64_t>(u) * kThreads;
      if (i >= n) continue;
      const uint64_t slot = k[u] == kEmptyKey ? cap : keyset_find(table, cap, k[u], h[u], s[u]);
      // the key ~0: its slot exists always, first_row tells whether a row has it
      const uint32_t j0 = slot == ~0ull ? kMiss : first_row[slot];
      uint8_t st = kCreate;
      if (j0 != kMiss) {
        const uint8_t rf = kRF ? r_flags[j0] : uint8_t(0);
        const uint64_t* q = r_meta + 3 * static_cast<uint64_t>(j0);
        const uint64_t ino = q[0], dev = q[1], mt = q[2];
        // the difference of the two times in 64-bit two's complement
        const int64_t d = static_cast<int64_t>(m[u][2] - mt);
        if ((rf ^ f[u]) & kIsDir) st = kKindChanged;
        else if (!(rf & kNoMetadata) && (ino != m[u][0] || dev != m[u][1] || d > 1000000))
          st = kUpdate;
        else st = kUnchanged;
        if (!(f[u] & kAncestor)) hit[slot] = 1;
      }
      match[i] = j0;
      state[i] = st;
    }
  }
}

// One lane per row: remove_flag[j] = the row's directory was walked and no
// entry of a listing has its key.
constexpr int kRRows = 4;
__global__ __launch_bounds__(kThreads) void k_idx_rows(const uint64_t* __restrict__ r_dirkey,
                                                       const uint32_t* __restrict__ slot_of,
                                                       uint64_t n,
                                                       const uint64_t* __restrict__ dtable,
                                                       uint64_t dcap,
                                                       const uint8_t* __restrict__ hit,
                                                       uint64_t cap,
                                                       uint8_t* __restrict__ remove_flag) {
  const bool special = hit[cap + 1] != 0;
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kThreads * kRRows;
  for (uint64_t i0 = static_cast<uint64_t>(blockIdx.x) * kThreads * kRRows + threadIdx.x; i0 < n;
       i0 += stride) {
    uint64_t k[kRRows], h[kRRows], s[kRRows];
    uint32_t sl[kRRows];
    uint8_t b[kRRows];
#pragma unroll
    for (int u = 0; u < kRRows; ++u)
      k[u] = r_dirkey[min(i0 + static_cast<uint64_t>(u) * kThreads, n - 1)];
#pragma unroll
    for (int u = 0; u < kRRows; ++u)
      sl[u] = slot_of[min(i0 + static_cast<uint64_t>(u) * kThreads, n - 1)];
#pragma unroll
    for (int u = 0; u < kRRows; ++u) {
      h[u] = row_hash(k[u]) & (dcap - 1);
      s[u] = dtable[h[u]];
      b[u] = hit[sl[u]];
    }
#pragma unroll
    for (int u = 0; u < kRRows; ++u) {
      const uint64_t i = i0 + static_cast<uint64_t>(u) * kThreads;
      if (i >= n) continue;
      const bool in_set =
          k[u] == kEmptyKey ? special : keyset_find(dtable, dcap, k[u], h[u], s[u]) != ~0ull;
      remove_flag[i] = in_set && b[u] == 0 ? 1 : 0;
    }
  }
}

// The three lists as one run of tiles: blocks [0, bw) create, [bw, 2 bw) update
// (both over state[n_w]), [2 bw, 2 bw + br) remove (over remove_flag[n_r]).
struct Lists {
  const uint8_t* state;
  const uint8_t* remove_flag;
  uint64_t n_w, n_r;
  uint32_t bw;
};
struct TileOf {
  const uint8_t* src;
  uint64_t n, tile;
  uint32_t list, first;  // first: the list's first block
};
__device__ __forceinline__ TileOf tile_of(const Lists& l, uint32_t b) {
  TileOf t;
  t.list = b < l.bw ? 0u : (b < 2 * l.bw ? 1u : 2u);
  t.first = t.list * l.bw;
  t.src = t.list == 2 ? l.remove_flag : l.state;
  t.n = t.list == 2 ? l.n_r : l.n_w;
  t.tile = static_cast<uint64_t>(b - t.first) * kTile;
  return t;
}

// A tile is kRows x kThreads positions: position tile + k * kThreads + t, and
// (k, t) order is index order.  Bit k of `f`: this thread's k-th position is
// listed; of `kc`: it is a KIND_CHANGED entry (create tiles only).
__device__ __forceinline__ void list_bits(const TileOf& t, uint32_t& f, uint32_t& kc) {
  uint8_t v[kRows];
#pragma unroll
  for (int k = 0; k < kRows; ++k) v[k] = t.src[min(t.tile + k * kThreads + threadIdx.x, t.n - 1)];
  f = 0;
  kc = 0;
#pragma unroll
  for (int k = 0; k < kRows; ++k) {
    const bool in = t.tile + k * kThreads + threadIdx.x < t.n;
    const bool on = t.list == 0 ? (v[k] == kCreate || v[k] == kKindChanged)
                                : (t.list == 1 ? v[k] == kUpdate : v[k] != 0);
    f |= (in && on ? 1u : 0u) << k;
    kc |= (in && t.list == 0 && v[k] == kKindChanged ? 1u : 0u) << k;
  }
}

__global__ __launch_bounds__(kThreads) void k_idx_count(Lists l, uint32_t* __restrict__ cnt,
                                                        uint32_t* __restrict__ counts) {
  const TileOf t = tile_of(l, blockIdx.x);
  uint32_t f[2], a[2];  // listed, KIND_CHANGED
  list_bits(t, f[0], f[1]);
  compact::tile_count(f, a);
  if (threadIdx.x == 0) {
    cnt[blockIdx.x] = a[0];
    if (a[1]) atomicAdd(&counts[3], a[1]);  // counts[3] is zero on entry
  }
}

// Stable compaction: a tile writes its listed positions from the scanned
// offset, relative to its list's first tile, in order.  Block 0 also writes
// the three lengths.
__global__ __launch_bounds__(kThreads) void k_idx_write(Lists l, uint32_t br,
                                                        const uint32_t* __restrict__ offs,
                                                        uint32_t* __restrict__ create,
                                                        uint32_t* __restrict__ update,
                                                        uint32_t* __restrict__ remove,
                                                        uint32_t* __restrict__ counts) {
  __shared__ uint32_t off[kRows][kWaves];
  const TileOf t = tile_of(l, blockIdx.x);
  uint32_t* out = t.list == 0 ? create : (t.list == 1 ? update : remove);
  const uint32_t w = threadIdx.x >> 6;
  uint32_t f, kc;
  list_bits(t, f, kc);
  uint32_t pre[kRows];
  compact::tile_offsets(f, [&] { return offs[blockIdx.x] - offs[t.first]; }, off, pre);
#pragma unroll
  for (int k = 0; k < kRows; ++k)
    if (f >> k & 1u)
      out[off[k][w] + pre[k]] = static_cast<uint32_t>(t.tile + k * kThreads + threadIdx.x);
  if (blockIdx.x == 0 && threadIdx.x < 3) {
    const uint32_t lo = threadIdx.x * l.bw;
    const uint32_t hi = threadIdx.x == 2 ? 2 * l.bw + br : lo + l.bw;
    counts[threadIdx.x] = offs[hi] - offs[lo];
  }
}

}  // namespace

size_t indexer_workspace_bytes(uint64_t n_w, uint64_t n_wd, uint64_t n_r) {
  return idx_ws(n_w, n_wd, n_r, nullptr).bytes;
}

hipError_t indexer_diff_launch(const IndexerIn& in, uint32_t* match, uint8_t* state,
                               uint32_t* create, uint32_t* update, uint32_t* remove,
                               uint32_t* counts, void* ws, hipStream_t s, KTimer* timer) {
  const IdxWs w = idx_ws(in.n_w, in.n_wd, in.n_r, ws);
  hipError_t e = hipMemsetAsync(counts, 0, 4 * sizeof(uint32_t), s);
  if (e != hipSuccess) return e;
  const uint64_t blocks = 2 * w.bw + w.br;
  if (blocks == 0) return hipSuccess;  // no entries, no rows: three empty lists
  // every call clears its own tables: the workspace is shared and may hold anything
  e = hipMemsetAsync(w.table, 0xFF, w.fill_bytes, s);
  if (e != hipSuccess) return e;
  e = hipMemsetAsync(w.hit, 0, w.cap + 2, s);
  if (e != hipSuccess) return e;
  if (in.n_r + in.n_wd) {
    KScope k(timer, "idx_build", s);
    k_idx_build<<<grid_for(in.n_r + in.n_wd, kThreads, kMaxGrid), kThreads, 0, s>>>(
        in.r_key, in.n_r, in.wd_key, in.n_wd, w.table, w.cap, w.dtable, w.dcap, w.first_row,
        w.slot_of, w.hit);
  }
  if (in.n_w) {
    KScope k(timer, "idx_probe", s);
    const uint32_t grid = grid_for(in.n_w, kThreads * kWRows, kMaxGrid);
#define SD_IDX_PROBE(WF, RF)                                                                    \
  k_idx_probe<WF, RF><<<grid, kThreads, 0, s>>>(in.w_key, in.w_flags, in.w_meta, in.n_w,        \
                                                 w.table, w.cap, w.first_row, in.r_flags,       \
                                                 in.r_meta, w.hit, match, state)
    if (in.w_flags && in.r_flags) SD_IDX_PROBE(true, true);
    else if (in.w_flags) SD_IDX_PROBE(true, false);
    else if (in.r_flags) SD_IDX_PROBE(false, true);
    else SD_IDX_PROBE(false, false);
#undef SD_IDX_PROBE
  }
  if (in.n_r) {
    KScope k(timer, "idx_rows", s);
    k_idx_rows<<<grid_for(in.n_r, kThreads * kRRows, kMaxGrid), kThreads, 0, s>>>(
        in.r_dirkey, w.slot_of, in.n_r, w.dtable, w.dcap, w.hit, w.cap, w.remove_flag);
  }
  const Lists l{state, w.remove_flag, in.n_w, in.n_r, static_cast<uint32_t>(w.bw)};
  {
    KScope k(timer, "idx_count", s);
    k_idx_count<<<static_cast<uint32_t>(blocks), kThreads, 0, s>>>(l, w.cnt, counts);
  }
  {
    KScope k(timer, "idx_scan", s);
    scan::exclusive(w.cnt, blocks, w.cnt, w.tiles, nullptr, s);
  }
  {
    KScope k(timer, "idx_write", s);
    k_idx_write<<<static_cast<uint32_t>(blocks), kThreads, 0, s>>>(
        l, static_cast<uint32_t>(w.br), w.cnt, create, update, remove, counts);
  }
  return hipGetLastError();
}

}  // namespace sdgpu
