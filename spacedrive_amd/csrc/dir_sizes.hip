// Indexer: the recursive size of every directory of one location as one device
// call -- a bottom-up accumulation over the directory tree with integer adds,
// which give the same sums in any order.
//
// Reference: FilePathMetadata.size_in_bytes goes into
// file_path.size_in_bytes_bytes for every entry (core/src/location/indexer/
// mod.rs:126-136, 215-225); for a directory that is the size of the directory
// inode.  search.paths orders by the column (api/search.rs:85) and
// ExplorerItem hands it to the UI (api/locations.rs:66-100).
//
// Here: the rows are in id order and carry the key of their own
// materialized_path (r_dirkey); directory rows also carry the key of their
// materialized_path_for_children() (r_selfkey).
//   k_ds_init    one lane per row: total = size of a file row, 0 of a
//                directory row; files = 0; the arrival word = 0; counts[0] =
//                the directory rows.  Every later kernel sizes the table from
//                counts[0] on the device: 2 x the directory rows rounded up to
//                a power of two, so the host never waits for the number.
//   k_ds_clear / k_ds_build
//                the key set of the directory self keys (keyset_device.hpp);
//                first_row[slot] = the lowest row that holds the slot's key.
//   k_ds_probe   one lane per row, 64 consecutive rows per wave step: parent =
//                first_row of the slot of r_dirkey.  Rows arrive in id order, so
//                lanes with one r_dirkey form runs: only a run's first lane
//                walks the table, a segmented wave scan sums the run, and the
//                run's last lane makes ONE atomic add per accumulator.  A run
//                that reaches the wave's last lane is carried into the wave's
//                next step, so a directory of 100 000 files costs about a
//                hundred adds on its address.
//   k_ds_climb   one lane per directory row without child directories (the
//                refit pattern): add the directory's sums to its parent's,
//                fence, count one arrival at the parent; the lane whose arrival
//                is the parent's last carries on with the parent, every other
//                lane stops.  No lane waits for another, and a lane takes at
//                most (directory rows) steps.  The members of a cycle of
//                `parent` always lack one arrival, so nothing ever climbs into
//                or around a cycle.
//   k_ds_final   directory rows that lack an arrival get the UNRESOLVED values;
//                the four counts.
//
// The accumulators are the outputs themselves (total[], files[]): 8-byte and
// 4-byte device-scope atomic adds, which execute at the memory side and are
// coherent across the XCDs' L2s.  Within k_ds_climb every access to an
// accumulator or an arrival word is such an atomic (a read is an add of 0), so
// no value passes through a cache that another XCD cannot see.
#include "compact_device.hpp"
#include "internal.hpp"
#include "keyset_device.hpp"

namespace sdgpu {

namespace {

using compact::kThreads;
using compact::kWaves;
constexpr uint32_t kMiss = 0xFFFFFFFFu;
constexpr uint64_t kUnresolved = ~0ull;
constexpr uint32_t kMaxGrid = 2048;
constexpr int kSteps = 16;                         // wave steps of 64 rows in k_ds_probe
constexpr uint32_t kProbeTile = kThreads * kSteps; // rows per workgroup there

// Slots of the table for nd directory rows (host and device agree).
__host__ __device__ inline uint64_t ds_cap(uint64_t nd) {
  uint64_t cap = 1024;
  while (cap < 2 * nd) cap <<= 1;
  return cap;
}

struct DsWs {
  uint64_t* table;      // [cap(max_dirs)]
  uint32_t* first_row;  // [cap(max_dirs) + 1]; the last used one: the key ~0
  // per row: child directories << 32 | arrived child directories
  unsigned long long* arrive;  // [n_r]
  uint32_t* files;      // [n_r], when the caller wants no file counts
  size_t bytes;
};

DsWs ds_ws(uint64_t n_r, uint64_t max_dirs, bool own_files, void* ws) {
  DsWs w;
  const uint64_t cap = ds_cap(max_dirs);
  Carve c(ws);
  w.table = c.take<uint64_t>(cap);
  w.first_row = c.take<uint32_t>(cap + 1);
  w.arrive = c.take<unsigned long long>(n_r);
  w.files = c.take<uint32_t>(own_files ? n_r : 0);
  w.bytes = c.bytes();
  return w;
}

__device__ __forceinline__ bool is_dir(const uint8_t* __restrict__ flags, uint64_t i) {
  return flags != nullptr && (flags[i] & 1u) != 0;
}

// Sum of v over the workgroup, in thread 0 (0 elsewhere).  Every thread calls
// it; `slot` tells the calls of one kernel apart.
__device__ __forceinline__ uint64_t block_sum(uint64_t v, int slot) {
  __shared__ uint64_t sw[4][kWaves];
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
  if (__lane_id() == 0) sw[slot][threadIdx.x >> 6] = v;
  __syncthreads();
  uint64_t t = 0;
  if (threadIdx.x == 0) {
    for (int w = 0; w < kWaves; ++w) t += sw[slot][w];
  }
  return t;
}

__global__ __launch_bounds__(kThreads) void k_ds_init(const uint8_t* __restrict__ flags,
                                                      const uint64_t* __restrict__ size,
                                                      uint64_t n, uint64_t* __restrict__ total,
                                                      uint32_t* __restrict__ files,
                                                      unsigned long long* __restrict__ arrive,
                                                      unsigned long long* __restrict__ counts) {
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kThreads;
  uint64_t dirs = 0;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x; i < n;
       i += stride) {
    const bool d = is_dir(flags, i);
    total[i] = d ? 0ull : size[i];
    files[i] = 0;
    arrive[i] = 0;
    dirs += d ? 1u : 0u;
  }
  const uint64_t t = block_sum(dirs, 0);
  if (threadIdx.x == 0 && t) atomicAdd(&counts[0], static_cast<unsigned long long>(t));
}

__global__ __launch_bounds__(kThreads) void k_ds_clear(const unsigned long long* __restrict__ counts,
                                                       uint64_t* __restrict__ table,
                                                       uint32_t* __restrict__ first_row) {
  const uint64_t cap = ds_cap(counts[0]);
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kThreads;
  for (uint64_t j = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x; j <= cap;
       j += stride) {
    if (j < cap) table[j] = kEmptyKey;
    first_row[j] = kMiss;
  }
}

__global__ __launch_bounds__(kThreads) void k_ds_build(const uint64_t* __restrict__ selfkey,
                                                       const uint8_t* __restrict__ flags,
                                                       uint64_t n,
                                                       const unsigned long long* __restrict__ counts,
                                                       uint64_t* __restrict__ table,
                                                       uint32_t* __restrict__ first_row) {
  const uint64_t cap = ds_cap(counts[0]);
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kThreads;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x; i < n;
       i += stride) {
    if (!is_dir(flags, i)) continue;
    const uint64_t k = selfkey[i];
    const uint64_t h = k == kEmptyKey ? cap : keyset_insert(table, cap, k);
    atomicMin(&first_row[h], static_cast<uint32_t>(i));
  }
}

// What a run of rows adds to its parent: bytes, and files | child directories
// << 16 (a wave's kSteps steps hold at most 64 x kSteps = 1024 of either).
struct Run {
  uint64_t bytes;
  uint32_t cnt;
};
static_assert(64 * kSteps < (1 << 16), "the two counts of a run share a word");

__device__ __forceinline__ void run_flush(uint32_t p, Run r, uint64_t* __restrict__ total,
                                          uint32_t* __restrict__ files,
                                          unsigned long long* __restrict__ arrive) {
  if (p == kMiss) return;
  if (r.bytes) atomicAdd(reinterpret_cast<unsigned long long*>(&total[p]),
                         static_cast<unsigned long long>(r.bytes));
  if (r.cnt & 0xFFFFu) atomicAdd(&files[p], r.cnt & 0xFFFFu);
  if (r.cnt >> 16) atomicAdd(&arrive[p], static_cast<unsigned long long>(r.cnt >> 16) << 32);
}

__global__ __launch_bounds__(kThreads) void k_ds_probe(
    const uint64_t* __restrict__ dirkey, const uint8_t* __restrict__ flags,
    const uint64_t* __restrict__ size, uint64_t n, const unsigned long long* __restrict__ counts,
    const uint64_t* __restrict__ table, const uint32_t* __restrict__ first_row,
    uint32_t* __restrict__ parent, uint64_t* __restrict__ total, uint32_t* __restrict__ files,
    unsigned long long* __restrict__ arrive) {
  const uint64_t cap = ds_cap(counts[0]);
  const uint32_t lane = __lane_id();
  // a wave owns 64 x kSteps consecutive rows
  const uint64_t base = static_cast<uint64_t>(blockIdx.x) * kProbeTile +
                        static_cast<uint64_t>(threadIdx.x >> 6) * (64 * kSteps);
  uint32_t cp = kMiss;  // the run carried from the step before (wave-uniform)
  Run cr{0, 0};
  for (int st = 0; st < kSteps; ++st) {
    const uint64_t i0 = base + static_cast<uint64_t>(st) * 64;
    if (i0 >= n) break;  // wave-uniform
    const uint64_t i = i0 + lane;
    const bool valid = i < n;
    const uint64_t k = valid ? dirkey[i] : 0ull;
    const bool d = valid && is_dir(flags, i);
    Run v{valid && !d ? size[i] : 0ull, valid ? (d ? 1u << 16 : 1u) : 0u};
    // runs: lanes with one key, one after another; a lane past the end is a
    // run of its own without a parent
    const uint64_t kp = __shfl_up(static_cast<unsigned long long>(k), 1);
    const bool head = lane == 0 || !valid || k != kp;
    const uint64_t heads = __ballot(head);
    const uint32_t start = 63u - static_cast<uint32_t>(__clzll(heads & (~0ull >> (63u - lane))));
    uint32_t p = kMiss;
    if (head && valid) {
      uint64_t slot = cap;  // the key ~0
      if (k != kEmptyKey) {
        const uint64_t h = row_hash(k) & (cap - 1);
        slot = keyset_find(table, cap, k, h, table[h]);
      }
      if (slot != ~0ull) p = first_row[slot];
    }
    p = __shfl(p, start);
    if (valid) parent[i] = p;
    // the carried run goes on in lane 0's, or is done
    const uint32_t p0 = __shfl(p, 0);
    if (lane == 0) {
      if (p0 == cp) {
        v.bytes += cr.bytes;
        v.cnt += cr.cnt;
      } else {
        run_flush(cp, cr, total, files, arrive);
      }
    }
    // inclusive sums within the runs
#pragma unroll
    for (uint32_t s = 1; s < 64; s <<= 1) {
      const uint64_t ob = __shfl_up(static_cast<unsigned long long>(v.bytes), s);
      const uint32_t oc = __shfl_up(v.cnt, s);
      if (lane >= s && lane - s >= start) {
        v.bytes += ob;
        v.cnt += oc;
      }
    }
    const bool tail = lane == 63 || (heads >> 1 >> lane & 1ull);
    if (tail && lane != 63) run_flush(p, v, total, files, arrive);
    cp = __shfl(p, 63);
    cr.bytes = __shfl(static_cast<unsigned long long>(v.bytes), 63);
    cr.cnt = __shfl(v.cnt, 63);
  }
  if (lane == 0) run_flush(cp, cr, total, files, arrive);
}

// A read as an atomic add of 0.  The 0 is hidden from the compiler, which
// otherwise turns the add into a load: the read must be served where the adds
// of other XCDs are made, not by this XCD's L2.
__device__ __forceinline__ unsigned long long ld_atomic(unsigned long long* p) {
  unsigned long long z = 0;
  asm volatile("" : "+v"(z));
  return atomicAdd(p, z);
}
__device__ __forceinline__ uint32_t ld_atomic(uint32_t* p) {
  uint32_t z = 0;
  asm volatile("" : "+v"(z));
  return atomicAdd(p, z);
}

__global__ __launch_bounds__(kThreads) void k_ds_climb(const uint8_t* __restrict__ flags,
                                                       uint64_t n,
                                                       const unsigned long long* __restrict__ counts,
                                                       const uint32_t* __restrict__ parent,
                                                       uint64_t* total, uint32_t* files,
                                                       unsigned long long* arrive) {
  const uint64_t dirs = counts[0];
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kThreads;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x; i < n;
       i += stride) {
    if (!is_dir(flags, i)) continue;
    // a directory without child directories has an arrival word of 0 for the
    // whole kernel: nothing ever arrives at it
    if (ld_atomic(&arrive[i]) != 0) continue;
    uint32_t d = static_cast<uint32_t>(i);
    for (uint64_t step = 0; step < dirs; ++step) {
      const uint32_t p = parent[d];
      if (p == kMiss) break;
      const unsigned long long t = ld_atomic(reinterpret_cast<unsigned long long*>(&total[d]));
      const uint32_t f = ld_atomic(&files[d]);
      if (t) atomicAdd(reinterpret_cast<unsigned long long*>(&total[p]), t);
      if (f) atomicAdd(&files[p], f);
      // the adds are done before the arrival is counted
      __threadfence();
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      const unsigned long long old = atomicAdd(&arrive[p], 1ull);
      // the last child directory to arrive carries on with the parent: every
      // other child's adds were done before its arrival, which came before
      // this one, and the reads above are atomics issued after this one returned
      if ((old & 0xFFFFFFFFull) + 1 != old >> 32) break;
      d = p;
    }
  }
}

__global__ __launch_bounds__(kThreads) void k_ds_final(const uint8_t* __restrict__ flags,
                                                       uint64_t n,
                                                       const uint32_t* __restrict__ parent,
                                                       const unsigned long long* __restrict__ arrive,
                                                       uint64_t* __restrict__ total,
                                                       uint32_t* __restrict__ files,
                                                       unsigned long long* __restrict__ counts) {
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kThreads;
  const uint64_t rounds = (n + stride - 1) / stride;  // every lane of a wave takes part in the ballots
  uint64_t resolved = 0, top = 0, sum = 0;            // the two counts: in lane 0 of a wave
  for (uint64_t r = 0; r < rounds; ++r) {
    const uint64_t i = r * stride + static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x;
    const bool valid = i < n;
    const bool d = valid && is_dir(flags, i);
    bool ok = false;
    if (d) {
      const unsigned long long a = arrive[i];
      ok = (a & 0xFFFFFFFFull) == a >> 32;
      if (!ok) {
        total[i] = kUnresolved;
        files[i] = 0xFFFFFFFFu;
      }
    }
    const bool miss = valid && parent[i] == kMiss;
    if (miss) sum += total[i];
    const uint64_t b_ok = __ballot(ok), b_miss = __ballot(miss);
    if (__lane_id() == 0) {
      resolved += __popcll(b_ok);
      top += __popcll(b_miss);
    }
  }
  const uint64_t t1 = block_sum(resolved, 1), t2 = block_sum(top, 2), t3 = block_sum(sum, 3);
  if (threadIdx.x == 0) {
    if (t1) atomicAdd(&counts[1], static_cast<unsigned long long>(t1));
    if (t2) atomicAdd(&counts[2], static_cast<unsigned long long>(t2));
    if (t3) atomicAdd(&counts[3], static_cast<unsigned long long>(t3));
  }
}

}  // namespace

size_t dir_sizes_workspace_bytes(uint64_t n_r, uint64_t max_dirs, bool own_files) {
  return ds_ws(n_r, max_dirs, own_files, nullptr).bytes;
}

hipError_t dir_sizes_launch(const uint64_t* dirkey, const uint64_t* selfkey, const uint8_t* flags,
                            const uint64_t* size, uint64_t n_r, uint64_t max_dirs,
                            uint32_t* parent, uint64_t* total, uint32_t* files, uint64_t* counts,
                            void* ws, hipStream_t s, KTimer* timer) {
  const DsWs w = ds_ws(n_r, max_dirs, files == nullptr, ws);
  hipError_t e = hipMemsetAsync(counts, 0, 4 * sizeof(uint64_t), s);
  if (e != hipSuccess || n_r == 0) return e;
  if (!files) files = w.files;
  unsigned long long* cnt = reinterpret_cast<unsigned long long*>(counts);
  const uint32_t grid = grid_for(n_r, kThreads, kMaxGrid);
  {
    KScope k(timer, "ds_init", s);
    k_ds_init<<<grid, kThreads, 0, s>>>(flags, size, n_r, total, files, w.arrive, cnt);
  }
  {
    // every call clears its own table: the workspace is shared and may hold anything
    KScope k(timer, "ds_build", s);
    k_ds_clear<<<grid_for(ds_cap(max_dirs) + 1, kThreads, kMaxGrid), kThreads, 0, s>>>(
        cnt, w.table, w.first_row);
    if (flags) k_ds_build<<<grid, kThreads, 0, s>>>(selfkey, flags, n_r, cnt, w.table, w.first_row);
  }
  {
    KScope k(timer, "ds_probe", s);
    k_ds_probe<<<static_cast<uint32_t>((n_r + kProbeTile - 1) / kProbeTile), kThreads, 0, s>>>(
        dirkey, flags, size, n_r, cnt, w.table, w.first_row, parent, total, files, w.arrive);
  }
  if (flags) {
    KScope k(timer, "ds_climb", s);
    k_ds_climb<<<grid, kThreads, 0, s>>>(flags, n_r, cnt, parent, total, files, w.arrive);
  }
  {
    KScope k(timer, "ds_final", s);
    k_ds_final<<<grid, kThreads, 0, s>>>(flags, n_r, parent, w.arrive, total, files, cnt);
  }
  return hipGetLastError();
}

}  // namespace sdgpu
