// Thumbnailer: the missing-thumbnail work list as one device semi-join.
//
// Reference: core/src/object/media/thumbnail/mod.rs:204-359 (process) stats
// <base>/<cas_id[0..2]>/<cas_id>.webp for every row of a step and generates
// where the file is missing (or `regenerate` is on); the rows come from one
// query (media_processor/mod.rs:74-116), in batches of 10 (job.rs:34,151).
// The explorer stats the same path per item (api/search.rs:540-547, library/
// library.rs:122-130 thumbnail_exists).
//
// Here the pieces the project already has are strung together, all on one
// stream with no host synchronisation:
//   1. the table of the thumbnail keys with its bit filter, as the remover
//      builds it (stale_build_launch);
//   2. the probe in the other direction (k_thumb_present, thumbnail_remover.hip):
//      present[i] and the candidate byte cand[i] per row, stats[0..2];
//   3. first-of-key over the candidates: the grouping with one row per chunk
//      (dedup_local_launch, chunk_rows = 1) gives rep[i] = the lowest candidate
//      row of key[i];
//   4. the work mask cand[i] &= rep[i] == i (k_work_mask), ordered by shard
//      directory = the first cas byte (thumbnail_shards_launch);
//   5. a one-wave scan of the 256 directory counts (k_dir_offsets).
#include "internal.hpp"

namespace sdgpu {

namespace {

constexpr int kThreads = 256;
constexpr uint32_t kDirs = 256;

struct WorkWs {
  void* table;        // the remover's workspace (stale_workspace_bytes)
  uint8_t* present;   // [n] when the caller wants none
  uint8_t* cand;      // [n] candidates, then the work mask
  uint32_t* rep;      // [n]
  uint32_t* counts;   // [256] rows per directory
  void* shards;       // thumbnail_shards_launch's workspace
  size_t bytes;
};

WorkWs work_ws(uint64_t n_thumbs, uint64_t n, bool with_work, void* ws) {
  WorkWs w;
  Carve c(ws);
  w.table = c.take(stale_workspace_bytes(n_thumbs));
  w.present = c.take(n);
  w.cand = c.take(with_work ? n : 0);
  w.rep = c.take<uint32_t>(with_work ? n : 0);
  w.counts = c.take<uint32_t>(with_work ? kDirs : 0);
  w.shards = c.take(with_work ? thumb_workspace_bytes() : 0);
  w.bytes = c.bytes();
  return w;
}

// cand[i] &= rep[i] == i: of the candidates, the lowest row of every key.  Four
// rows per thread (a 16-byte load of rep, a 4-byte load and store of cand; both
// arrays start 256-byte aligned), the last rows one by one.
__global__ __launch_bounds__(kThreads) void k_work_mask(const uint32_t* __restrict__ rep,
                                                        uint64_t n, uint8_t* __restrict__ cand) {
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kThreads * 4;
  for (uint64_t i = (static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x) * 4; i < n;
       i += stride) {
    if (i + 4 <= n) {
      const uint4 r = *reinterpret_cast<const uint4*>(rep + i);
      const uint32_t c = *reinterpret_cast<const uint32_t*>(cand + i);
      const uint32_t i32 = static_cast<uint32_t>(i);
      const uint32_t m = (r.x == i32 ? 0xFFu : 0u) | (r.y == i32 + 1 ? 0xFF00u : 0u) |
                         (r.z == i32 + 2 ? 0xFF0000u : 0u) | (r.w == i32 + 3 ? 0xFF000000u : 0u);
      *reinterpret_cast<uint32_t*>(cand + i) = c & m;
    } else {
      for (uint64_t j = i; j < n; ++j)
        if (rep[j] != static_cast<uint32_t>(j)) cand[j] = 0;
    }
  }
}

// One wave: dir_start[0..256] = exclusive scan of the 256 counts (four per
// lane), stats[3] = their sum.
__global__ __launch_bounds__(64) void k_dir_offsets(const uint32_t* __restrict__ counts,
                                                    uint32_t* __restrict__ dir_start,
                                                    uint32_t* __restrict__ stats) {
  static_assert(kDirs == 4 * 64, "four directories per lane");
  const uint32_t lane = threadIdx.x;
  const uint4 c = *reinterpret_cast<const uint4*>(counts + 4 * lane);
  const uint32_t a = c.x + c.y + c.z + c.w;
  uint32_t inc = a;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t x = __shfl_up(inc, d);
    if (lane >= static_cast<uint32_t>(d)) inc += x;
  }
  uint32_t run = inc - a;
  dir_start[4 * lane] = run;
  dir_start[4 * lane + 1] = run += c.x;
  dir_start[4 * lane + 2] = run += c.y;
  dir_start[4 * lane + 3] = run += c.z;
  if (lane == 63) {
    dir_start[kDirs] = inc;
    stats[3] = inc;
  }
}

}  // namespace

size_t thumb_worklist_workspace_bytes(uint64_t n_thumbs, uint64_t n, bool with_work) {
  return work_ws(n_thumbs, n, with_work, nullptr).bytes;
}

hipError_t thumb_worklist_launch(const uint64_t* thumb_key, uint64_t n_thumbs, const uint64_t* key,
                                 const uint8_t* has, const uint8_t* elig, uint64_t n, bool regen,
                                 uint8_t* present, uint32_t* work, uint32_t* dir_start,
                                 uint32_t* stats, void* ws, void* group_ws, hipStream_t s,
                                 KTimer* timer) {
  const bool with_work = work != nullptr;
  const WorkWs w = work_ws(n_thumbs, n, with_work, ws);
  hipError_t e = hipMemsetAsync(stats, 0, 4 * sizeof(uint32_t), s);
  if (e != hipSuccess) return e;
  if (n == 0) return with_work ? hipMemsetAsync(dir_start, 0, 4 * (kDirs + 1), s) : hipSuccess;
  // no thumbnails: an empty table and filter, nothing is present
  e = stale_build_launch(thumb_key, n_thumbs, w.table, s);
  if (e != hipSuccess) return e;
  e = thumb_present_launch(n_thumbs, key, has, elig, n, regen, present ? present : w.present,
                           with_work ? w.cand : nullptr, stats, w.table, s, timer);
  if (e != hipSuccess || !with_work) return e;
  GroupInput in;
  in.key = key;
  in.valid = w.cand;
  in.n = n;
  // init_rep: the grouping stores only the reps that differ from the row's own
  // rank, so a work row's rep[i] == i is the initial value
  e = dedup_local_launch(in, 1, w.rep, true, group_ws, s, timer);
  if (e != hipSuccess) return e;
  {
    KScope k(timer, "thumb_work_mask", s);
    k_work_mask<<<grid_for(n, 4 * kThreads, 2048), kThreads, 0, s>>>(w.rep, n, w.cand);
  }
  e = thumbnail_shards_launch(reinterpret_cast<const uint8_t*>(key), w.cand, n, work, w.counts,
                              w.shards, s);
  if (e != hipSuccess) return e;
  k_dir_offsets<<<1, 64, 0, s>>>(w.counts, dir_start, stats);
  return hipGetLastError();
}

}  // namespace sdgpu
