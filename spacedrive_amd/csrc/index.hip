// Object index: the library-wide "which Object already owns this cas_id"
// lookup of identifier_job_step, on the device.
//
// Reference: file_identifier/mod.rs:168-185 fetches every Object that has a
// file_path whose cas_id is in the step's set (library-wide, across locations
// and earlier runs), and :189-225 links each row whose cas_id matches one of
// them to that Object; only the remaining rows (:233-241) create new Objects.
// A batch grouped in isolation would miss those links, so the grouping of a
// batch first probes this index and then, after the batch, records the keys
// whose Objects it created.  Batches processed in id order then give exactly
// the grouping of the whole run (test_gpu_index.py).
//
// Table: open addressing in HBM, 16-byte slots {key lo, key hi, value, removed},
// linear probing from row_hash(key) & (cap - 1) (four slots per 64-B line, so a
// probe is one line read at load <= 1/2).  Empty slot: key == ~0; the key ~0
// itself lives in a separate special slot.  Inserts: 64-bit agent-scope CAS
// on the key, then atomicMin on the value's slot encoding, so one key keeps
// the first Object in this order: any pre-existing Object (lowest handle)
// before any Object created during the run (lowest rank) -- the reference's
// find_many (mod.rs:168-185) returns Objects already in the database, so an
// Object registered with add_objects wins whatever the call order.  Slot
// encoding: enc = value ^ EXISTING (existing handles map below 2^31, ranks
// above; the empty value 0xFFFFFFFF stays above both).
//
// Values: a row rank r (< 2^31) -- the Object created by row r of this or an
// earlier batch of the same run -- or SDGPU_REP_EXISTING | handle for an
// Object that existed before the run (registered by the caller).  The probe of
// a keyed row r that finds value v writes
//   rep[r] = v                       if v is an existing Object,
//            r  if chunk(r) == chunk(v), else v   (the grouping rule of a6),
// and removes the row from the batch's own grouping; other rows keep rep = r
// and valid = 1.  After the grouping, the rows that created an Object
// (rep == rank) are inserted with their rank.
//
// Removal (a library-lifetime index: the orphan remover, the watcher's delete
// path): linear probing cannot free a slot in place, so a removed entry keeps
// its key and gets the empty value 0xFFFFFFFF -- the "no value yet" encoding
// an insert's atomicMin already starts from, so a later insert of the key
// revives the slot with no special case, and a probe that meets the key with
// the empty value misses.  Two counters: t.count = slots in use (key CAS
// winners; drives growth) and t.dead = removed slots still in the table; live
// keys = count - dead.  Each transition is seen by exactly one thread: a new
// slot by the winner of its key CAS (count + 1); a removal by the thread whose
// exchange / CAS on the value word returned a value (dead + 1), which also
// raises the slot's fourth word (removed flag, 0 otherwise); a revival by the
// thread whose exchange on a raised flag returned it (dead - 1).  An insert
// that finds its key in place reads that flag (never raised while inserts
// run).  The common insert -- a new key -- therefore costs what it did before
// removal existed: one per-wave atomic on count.  (A live counter fed by every
// insert was measured first: a second same-address atomic per wave, 0.67 ->
// 0.98 ms on the creators' insert of 12.5 M new keys.)  The rehash drops
// removed slots, so a table worn out by churn is rebuilt at the size its live
// keys need.  The key ~0 keeps its own slot special[2] and is in neither
// counter (the host adds it).
#include "internal.hpp"
#include "rows_device.hpp"

namespace sdgpu {

namespace {

constexpr uint64_t kEmptyKey = ~0ull;
constexpr uint32_t kEmptyVal = 0xFFFFFFFFu;  // slot encoding: no value (yet, or removed)
constexpr int kThreads = 256;

__device__ __forceinline__ uint64_t slot_key(const uint4& q) {
  return (static_cast<uint64_t>(q.y) << 32) | q.x;
}

__device__ __forceinline__ uint32_t enc_value(uint32_t v) { return v ^ kRepExisting; }

// What a thread's inserts added: slots taken (key CAS won) and removed slots
// brought back.  The caller adds both up per wave (count_added): one atomic
// per wave and counter instead of one per key -- same-address device atomics
// serialise at a few ns each.
struct Added {
  uint32_t slots = 0, revived = 0;
};

// Insert (k, v): keeps the minimum enc_value over inserts (existing Objects
// first).
__device__ __forceinline__ void index_insert(const IndexRef& t, uint64_t k, uint32_t v, Added& a) {
  const uint32_t e = enc_value(v);
  if (k == kEmptyKey) {
    atomicMax(&t.special[0], 1u);
    atomicMin(&t.special[1], e);
    return;
  }
  uint64_t h = row_hash(k) & (t.cap - 1);
  for (;;) {
    unsigned long long* kp = reinterpret_cast<unsigned long long*>(&t.slots[h]);
    const unsigned long long prev =
        atomicCAS(kp, static_cast<unsigned long long>(kEmptyKey), static_cast<unsigned long long>(k));
    if (prev == kEmptyKey) {
      atomicMin(&t.slots[h].z, e);
      a.slots += 1;
      return;
    }
    if (prev == k) {
      // the key is in place: live, just taken by another thread (flag 0), or
      // removed by an earlier call (flag 1: one of its inserters lowers it)
      if (t.slots[h].w != 0 && atomicExch(&t.slots[h].w, 0u) != 0) a.revived += 1;
      atomicMin(&t.slots[h].z, e);
      return;
    }
    h = (h + 1) & (t.cap - 1);
  }
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t x) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) x += __shfl_xor(x, d);
  return x;
}

// after a grid-stride loop (every lane of the wave arrives): the wave's new
// slots onto count, its revived ones (rare) off dead
__device__ __forceinline__ void count_added(const IndexRef& t, const Added& a) {
  const uint32_t slots = wave_sum(a.slots), revived = wave_sum(a.revived);
  if (__lane_id() == 0 && slots) atomicAdd(t.count, static_cast<unsigned long long>(slots));
  if (__lane_id() == 0 && revived)
    atomicAdd(t.dead, ~static_cast<unsigned long long>(revived) + 1ull);  // -= revived
}

// Slot holding k (its value word may be empty: a removed key), or null; the
// key ~0 has no slot of this kind (special[2]).
__device__ __forceinline__ uint4* index_slot(const IndexRef& t, uint64_t k) {
  uint64_t h = row_hash(k) & (t.cap - 1);
  for (;;) {
    const uint4 q = t.slots[h];
    const uint64_t sk = slot_key(q);
    if (sk == k) return &t.slots[h];
    if (sk == kEmptyKey) return nullptr;
    h = (h + 1) & (t.cap - 1);
  }
}

// Take the value out of *zp (cond: only while it is `e`); true for the one
// thread that saw the value go.
__device__ __forceinline__ bool take_value(uint32_t* zp, bool cond, uint32_t e) {
  if (cond) return e != kEmptyVal && atomicCAS(zp, e, kEmptyVal) == e;
  return atomicExch(zp, kEmptyVal) != kEmptyVal;
}

// Value of k, or false (absent, or removed: its value word is empty).
__device__ __forceinline__ bool index_find(const IndexRef& t, uint64_t k, uint32_t& v) {
  if (k == kEmptyKey) {
    const uint32_t e = t.special[1];
    v = enc_value(e);
    return t.special[0] != 0 && e != kEmptyVal;
  }
  uint64_t h = row_hash(k) & (t.cap - 1);
  for (;;) {
    const uint4 q = t.slots[h];
    const uint64_t sk = slot_key(q);
    if (sk == k) {
      v = enc_value(q.z);
      return q.z != kEmptyVal;
    }
    if (sk == kEmptyKey) return false;
    h = (h + 1) & (t.cap - 1);
  }
}

__global__ __launch_bounds__(kThreads) void k_index_clear(IndexRef t) {
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kThreads;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x; i < t.cap;
       i += stride)
    t.slots[i] = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0u);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    *t.count = 0;
    *t.dead = 0;
    t.special[0] = 0;
    t.special[1] = 0xFFFFFFFFu;
  }
}

// Re-insert every live entry of `from` into the (cleared) `to`; removed slots
// (a key with the empty value) are dropped.
__global__ __launch_bounds__(kThreads) void k_index_rehash(IndexRef from, IndexRef to) {
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kThreads;
  Added added;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x; i < from.cap;
       i += stride) {
    const uint4 q = from.slots[i];
    if (slot_key(q) != kEmptyKey && q.z != kEmptyVal)
      index_insert(to, slot_key(q), enc_value(q.z), added);
  }
  count_added(to, added);
  if (blockIdx.x == 0 && threadIdx.x == 0 && from.special[0] && from.special[1] != kEmptyVal) {
    to.special[0] = 1;
    to.special[1] = from.special[1];
  }
}

// Pre-existing Objects: key[i] -> EXISTING | handle[i], for the keys whose
// shard (top 8 hash bits) belongs to `rank` of `world` (world 1: every key).
__global__ __launch_bounds__(kThreads) void k_index_objects(IndexRef t, const uint64_t* __restrict__ key,
                                                            const uint32_t* __restrict__ handle,
                                                            uint64_t n, uint32_t world,
                                                            uint32_t rank) {
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kThreads;
  Added added;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x; i < n;
       i += stride) {
    const uint64_t k = key[i];
    if (world > 1 && ((row_hash(k) >> 56) * world) >> 8 != rank) continue;
    index_insert(t, k, kRepExisting | (handle[i] & ~kRepExisting), added);
  }
  count_added(t, added);
}

template <typename In>
__global__ __launch_bounds__(kThreads) void k_index_probe(IndexRef t, In in, uint64_t n,
                                                          uint32_t chunk_rows,
                                                          uint32_t* __restrict__ rep,
                                                          uint8_t* __restrict__ valid_out) {
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kThreads;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x; i < n;
       i += stride) {
    uint64_t k;
    uint32_t r;
    bool v;
    in.get(i, k, r, v);
    uint32_t out = r, f;
    bool group = v;
    if (v && index_find(t, k, f)) {
      group = false;
      if (f & kRepExisting) out = f;                         // existing Object (mod.rs:189-225)
      else if (r / chunk_rows != f / chunk_rows) out = f;    // Object of an earlier chunk
    }
    rep[i] = out;
    valid_out[i] = group ? 1 : 0;
  }
}

// After the grouping: rows that created an Object (grouped, rep == rank).
// skip (may be null): *skip != 0 -- the rows of a padded exchange that
// overflowed, whose grouping is re-run through the counted exchange -- inserts
// nothing (the index must not learn creators of an incomplete grouping).
template <typename In>
__global__ __launch_bounds__(kThreads) void k_index_creators(IndexRef t, In in, uint64_t n,
                                                             const uint32_t* __restrict__ rep,
                                                             const uint8_t* __restrict__ grouped,
                                                             const uint32_t* __restrict__ skip) {
  if (skip && *skip) return;
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kThreads;
  Added added;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x; i < n;
       i += stride) {
    if (!grouped[i]) continue;
    uint64_t k;
    uint32_t r;
    bool v;
    in.get(i, k, r, v);
    if (rep[i] == r) index_insert(t, k, r, added);
  }
  count_added(t, added);
}

// value[i] = the stored value of key[i] as a grouping's rep shows it (a rank,
// or EXISTING | handle), kIndexMiss when the key is absent or removed.
__global__ __launch_bounds__(kThreads) void k_index_lookup(IndexRef t,
                                                           const uint64_t* __restrict__ key,
                                                           uint64_t n,
                                                           uint32_t* __restrict__ value) {
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kThreads;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x; i < n;
       i += stride) {
    uint32_t f;
    value[i] = index_find(t, key[i], f) ? f : kIndexMiss;
  }
}

// the wave's removals: onto the dead count (the key ~0 is in no counter:
// `counted` excludes it) and onto *removed (may be null)
__device__ __forceinline__ void count_removed(const IndexRef& t, uint32_t counted, uint32_t all,
                                              uint32_t* removed) {
  counted = wave_sum(counted);
  all = wave_sum(all);
  if (__lane_id() == 0 && counted) atomicAdd(t.dead, static_cast<unsigned long long>(counted));
  if (__lane_id() == 0 && all && removed) atomicAdd(removed, all);
}

// Remove key[i] (when value is given: only if it still holds value[i]).  The
// exchange / CAS on the value word returns a value to exactly one thread per
// live key, so a key listed several times counts once.
__global__ __launch_bounds__(kThreads) void k_index_remove(IndexRef t,
                                                           const uint64_t* __restrict__ key,
                                                           const uint32_t* __restrict__ value,
                                                           uint64_t n,
                                                           uint32_t* __restrict__ removed) {
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kThreads;
  uint32_t counted = 0, all = 0;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x; i < n;
       i += stride) {
    const uint64_t k = key[i];
    const uint32_t e = value ? enc_value(value[i]) : 0u;
    if (k == kEmptyKey) {
      if (t.special[0] && take_value(&t.special[1], value != nullptr, e)) ++all;
      continue;
    }
    uint4* q = index_slot(t, k);
    if (!q || !take_value(&q->z, value != nullptr, e)) continue;
    q->w = 1u;  // removed: the insert that brings the key back counts it
    ++all;
    ++counted;
  }
  count_removed(t, counted, all, removed);
}

// mark[h] = 1 for every handle of the list (ids as the orphan remover writes
// them: int32; negative ones and ones past max_handle name no entry).  Plain
// byte stores: marking is idempotent.
__global__ __launch_bounds__(kThreads) void k_index_mark(const int32_t* __restrict__ handle,
                                                         uint64_t n, uint32_t max_handle,
                                                         uint8_t* __restrict__ mark) {
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kThreads;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x; i < n;
       i += stride) {
    const int32_t h = handle[i];
    if (h >= 0 && static_cast<uint32_t>(h) <= max_handle) mark[h] = 1;
  }
}

// slot encoding e is a marked existing handle (existing handles encode below
// 2^31, ranks above)
__device__ __forceinline__ bool marked(uint32_t e, const uint8_t* __restrict__ mark,
                                       uint32_t max_handle) {
  return e < kRepExisting && e <= max_handle && mark[e] != 0;
}

// One pass over the slots: entries of marked handles lose their value; rank
// entries are never touched.
__global__ __launch_bounds__(kThreads) void k_index_remove_marked(IndexRef t,
                                                                  const uint8_t* __restrict__ mark,
                                                                  uint32_t max_handle,
                                                                  uint32_t* __restrict__ removed) {
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kThreads;
  uint32_t counted = 0, all = 0;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x; i < t.cap;
       i += stride) {
    const uint4 q = t.slots[i];
    if (slot_key(q) == kEmptyKey || !marked(q.z, mark, max_handle)) continue;
    // (nothing else writes while this runs, but keep the transition exact)
    if (atomicCAS(&t.slots[i].z, q.z, kEmptyVal) == q.z) {
      t.slots[i].w = 1u;
      ++counted;
    }
  }
  all = counted;
  if (blockIdx.x == 0 && threadIdx.x == 0 && t.special[0]) {
    const uint32_t e = t.special[1];
    if (marked(e, mark, max_handle) && atomicCAS(&t.special[1], e, kEmptyVal) == e) ++all;
  }
  count_removed(t, counted, all, removed);
}

// Dense (key, value) arrays of the live entries, in no particular order.  A
// wave takes tiles of kExportRows x 64 consecutive slots (cap is a power of two
// >= 1024: whole tiles): ranks inside the tile from per-row ballots, ONE atomic
// per wave and tile on the count (one per 64 slots measured 11.9 ms for a
// 67 M-slot table: ~10 ns per same-address atomic, a million of them).  The
// count runs past cap when the arrays are too short; nothing is written there.
constexpr int kExportRows = 16;
constexpr uint64_t kExportTile = static_cast<uint64_t>(kExportRows) * 64;
__global__ __launch_bounds__(kThreads) void k_index_export(IndexRef t, uint64_t* __restrict__ key,
                                                           uint32_t* __restrict__ value,
                                                           uint64_t cap_out,
                                                           uint32_t* __restrict__ count) {
  const uint32_t lane = __lane_id();
  const uint64_t lt = (1ull << lane) - 1ull;
  const uint64_t waves = static_cast<uint64_t>(gridDim.x) * (kThreads / 64);
  const uint64_t wave = static_cast<uint64_t>(blockIdx.x) * (kThreads / 64) + (threadIdx.x >> 6);
  for (uint64_t i0 = wave * kExportTile; i0 < t.cap; i0 += waves * kExportTile) {
    uint4 q[kExportRows];
#pragma unroll
    for (int u = 0; u < kExportRows; ++u) q[u] = t.slots[i0 + u * 64 + lane];
    uint32_t pre[kExportRows], total = 0, mine = 0;
#pragma unroll
    for (int u = 0; u < kExportRows; ++u) {
      const bool is = slot_key(q[u]) != kEmptyKey && q[u].z != kEmptyVal;
      const uint64_t b = __ballot(is);
      mine |= (is ? 1u : 0u) << u;
      pre[u] = total + __popcll(b & lt);
      total += __popcll(b);
    }
    if (total == 0) continue;  // wave-uniform
    uint32_t base = 0;
    if (lane == 0) base = atomicAdd(count, total);
    base = __shfl(base, 0);
#pragma unroll
    for (int u = 0; u < kExportRows; ++u) {
      const uint64_t o = static_cast<uint64_t>(base) + pre[u];
      if ((mine >> u & 1u) && o < cap_out) {
        key[o] = slot_key(q[u]);
        value[o] = enc_value(q[u].z);
      }
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0 && t.special[0] && t.special[1] != kEmptyVal) {
    const uint32_t o = atomicAdd(count, 1u);
    if (o < cap_out) {
      key[o] = kEmptyKey;
      value[o] = enc_value(t.special[1]);
    }
  }
}

constexpr uint32_t kMaxGrid = 8192;

}  // namespace

hipError_t index_clear_launch(const IndexRef& t, hipStream_t s) {
  k_index_clear<<<grid_for(t.cap, kThreads, kMaxGrid), kThreads, 0, s>>>(t);
  return hipGetLastError();
}

hipError_t index_rehash_launch(const IndexRef& from, const IndexRef& to, hipStream_t s) {
  k_index_clear<<<grid_for(to.cap, kThreads, kMaxGrid), kThreads, 0, s>>>(to);
  k_index_rehash<<<grid_for(from.cap, kThreads, kMaxGrid), kThreads, 0, s>>>(from, to);
  return hipGetLastError();
}

hipError_t index_objects_launch(const IndexRef& t, const uint64_t* key, const uint32_t* handle,
                                uint64_t n, uint32_t world, uint32_t rank, hipStream_t s) {
  if (n)
    k_index_objects<<<grid_for(n, kThreads, kMaxGrid), kThreads, 0, s>>>(t, key, handle, n, world,
                                                                          rank);
  return hipGetLastError();
}

hipError_t index_probe_launch(const IndexRef& t, const GroupInput& in, uint32_t chunk_rows,
                              uint32_t* rep, uint8_t* valid_out, hipStream_t s, KTimer* timer) {
  if (in.n == 0) return hipSuccess;
  KScope k(timer, "index_probe", s);
  if (in.rec12)
    k_index_probe<<<grid_for(in.n, kThreads, kMaxGrid), kThreads, 0, s>>>(
        t, RecIn{reinterpret_cast<const uint3*>(in.rec12), in.valid}, in.n, chunk_rows, rep,
        valid_out);
  else
    k_index_probe<<<grid_for(in.n, kThreads, kMaxGrid), kThreads, 0, s>>>(
        t, RowsIn{in.key, in.valid, in.rank, in.rank_base}, in.n, chunk_rows, rep, valid_out);
  return hipGetLastError();
}

hipError_t index_creators_launch(const IndexRef& t, const GroupInput& in, const uint32_t* rep,
                                 const uint8_t* grouped, hipStream_t s, KTimer* timer,
                                 const uint32_t* skip) {
  if (in.n == 0) return hipSuccess;
  KScope k(timer, "index_insert", s);
  if (in.rec12)
    k_index_creators<<<grid_for(in.n, kThreads, kMaxGrid), kThreads, 0, s>>>(
        t, RecIn{reinterpret_cast<const uint3*>(in.rec12), nullptr}, in.n, rep, grouped, skip);
  else
    k_index_creators<<<grid_for(in.n, kThreads, kMaxGrid), kThreads, 0, s>>>(
        t, RowsIn{in.key, nullptr, in.rank, in.rank_base}, in.n, rep, grouped, skip);
  return hipGetLastError();
}

hipError_t index_lookup_launch(const IndexRef& t, const uint64_t* key, uint64_t n,
                               uint32_t* value, hipStream_t s, KTimer* timer) {
  if (n == 0) return hipSuccess;
  KScope k(timer, "index_lookup", s);
  k_index_lookup<<<grid_for(n, kThreads, kMaxGrid), kThreads, 0, s>>>(t, key, n, value);
  return hipGetLastError();
}

hipError_t index_remove_launch(const IndexRef& t, const uint64_t* key, const uint32_t* value,
                               uint64_t n, uint32_t* removed, hipStream_t s, KTimer* timer) {
  if (removed) {
    const hipError_t e = hipMemsetAsync(removed, 0, sizeof(uint32_t), s);
    if (e != hipSuccess) return e;
  }
  if (n == 0) return hipSuccess;
  KScope k(timer, "index_remove", s);
  k_index_remove<<<grid_for(n, kThreads, kMaxGrid), kThreads, 0, s>>>(t, key, value, n, removed);
  return hipGetLastError();
}

size_t index_mark_workspace_bytes(uint32_t max_handle) {
  return (static_cast<size_t>(max_handle) + 1 + 255) / 256 * 256;
}

hipError_t index_remove_objects_launch(const IndexRef& t, const int32_t* handle, uint64_t n,
                                       uint32_t max_handle, uint32_t* removed, void* ws,
                                       hipStream_t s, KTimer* timer) {
  if (removed) {
    const hipError_t e = hipMemsetAsync(removed, 0, sizeof(uint32_t), s);
    if (e != hipSuccess) return e;
  }
  if (n == 0) return hipSuccess;
  uint8_t* mark = static_cast<uint8_t*>(ws);
  // every call clears its own map: the workspace is shared and may hold anything
  const hipError_t e = hipMemsetAsync(mark, 0, index_mark_workspace_bytes(max_handle), s);
  if (e != hipSuccess) return e;
  KScope k(timer, "index_remove_objects", s);
  k_index_mark<<<grid_for(n, kThreads, kMaxGrid), kThreads, 0, s>>>(handle, n, max_handle, mark);
  k_index_remove_marked<<<grid_for(t.cap, kThreads, kMaxGrid), kThreads, 0, s>>>(
      t, mark, max_handle, removed);
  return hipGetLastError();
}

hipError_t index_export_launch(const IndexRef& t, uint64_t* key, uint32_t* value, uint64_t cap_out,
                               uint32_t* d_count, hipStream_t s, KTimer* timer) {
  const hipError_t e = hipMemsetAsync(d_count, 0, sizeof(uint32_t), s);
  if (e != hipSuccess) return e;
  KScope k(timer, "index_export", s);
  k_index_export<<<grid_for(t.cap / kExportRows, kThreads, kMaxGrid), kThreads, 0, s>>>(
      t, key, value, cap_out, d_count);
  return hipGetLastError();
}

}  // namespace sdgpu
