// Sync ingest: which CRDT operations of a page apply, as one device call.
//
// Reference: core/crates/sync/src/ingest.rs:114-160 (receive_crdt_operation)
// takes one op at a time; compare_message (:188-233) finds the newest logged op
// of the op's (model, record_id, kind) with timestamp >= t -- the op is old
// exactly when one exists with another timestamp, i.e. when L(key) > t in the
// signed order of the BigInt column -- and an op that is not old is applied and
// logged (:162-186), so later ops of the page see it.  Whatever the outcome
// the instance's clock becomes max(clock, t) in NTP64 (unsigned) order
// (:119-126,151).
//
// Here: the op log is an open-addressing table that lives as long as the
// library (32-byte slots {key, timestamp, tag, spare}: a probe costs one
// sector; capacity a power of two, linear probing from row_hash(key), empty
// slot ~0; the key ~0 owns the slot one past the table, the convention of
// keyset_device.hpp's 8-byte sets).  The timestamp is stored biased by 1 << 63, so unsigned
// 64-bit order is the signed order and the empty value 0 is INT64_MIN.  A page:
//   k_log_slot   one lane per op: probe or insert the key; slot_of[i], the
//                slot's logged timestamp base[i]; new keys counted from wave
//                ballots; clocks folded per workgroup in LDS;
//   k_sort_hist / scan / k_sort_scatter
//                stable LSD radix sort of (slot, i) on the slot bits in 8-bit
//                digits (2-4 passes): each key's ops end up adjacent, in
//                arrival order, however skewed the page is;
//   k_seg_agg / k_seg_carry / k_seg_apply
//                one segmented scan over the sorted pairs carrying (running
//                max, op that last reached it) seeded with the logged
//                timestamp: the exclusive value decides apply, the segment's
//                tail commits the maximum (the one writer of its slot) and
//                marks the winner; tiles are joined by an aggregate pass and a
//                one-workgroup scan of the aggregates;
//   k_ing_count / scan / k_ing_write
//                applied and winner as ONE compaction (compact_device.hpp; the
//                two lists' tiles behind one another, one scan).
#include "compact_device.hpp"
#include "internal.hpp"
#include "rows_device.hpp"
#include "scan_device.hpp"

namespace sdgpu {

namespace {

constexpr uint64_t kEmptyKey = ~0ull;
constexpr uint64_t kBias = 1ull << 63;
constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr uint32_t kClockLds = 1024;  // instances folded in LDS; more go straight to memory

// sort and segmented scan: tiles of kTile ops
constexpr int kRounds = 8;
constexpr uint32_t kTile = kRounds * kThreads;  // 2048
constexpr uint32_t kBins = 256;

static_assert(kThreads == compact::kThreads, "k_ing_count / k_ing_write");
constexpr uint32_t kMaxGrid = 4096;
using compact::wave_sum;

// slot s of the table: words [4 s, 4 s + 4) = key, biased timestamp, tag, spare
__device__ __forceinline__ uint64_t* slot_at(const OplogRef& t, uint64_t s) {
  return t.slots + 4 * s;
}

// Every slot empty (key ~0, timestamp 0 = none, tag 0), the key ~0's slot
// included; no key stored.
__global__ __launch_bounds__(kThreads) void k_log_clear(OplogRef t) {
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kThreads;
  for (uint64_t s = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x; s <= t.cap;
       s += stride) {
    uint64_t* p = slot_at(t, s);
    p[0] = kEmptyKey;
    p[1] = 0;
    p[2] = 0;
    p[3] = 0;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) *t.count = 0;
}

// The slot of key k, entered if it is absent (`fresh`: this thread entered it).
// The host reserved capacity (load <= 1/2 with every key of the call entered):
// an empty slot ends every walk.  The key ~0 lives in slot cap, whose key word
// is ~0 (not entered) or 0 (entered).
__device__ __forceinline__ uint64_t enter_slot(const OplogRef& t, uint64_t k, bool& fresh) {
  fresh = false;
  if (k == kEmptyKey) {
    unsigned long long* w = reinterpret_cast<unsigned long long*>(slot_at(t, t.cap));
    if (*w == kEmptyKey) fresh = atomicCAS(w, static_cast<unsigned long long>(kEmptyKey), 0ull) ==
                                 kEmptyKey;
    return t.cap;
  }
  const uint64_t m = t.cap - 1;
  uint64_t h = row_hash(k) & m;
  for (;;) {
    unsigned long long* w = reinterpret_cast<unsigned long long*>(slot_at(t, h));
    unsigned long long cur = *w;
    if (cur == kEmptyKey) {
      cur = atomicCAS(w, static_cast<unsigned long long>(kEmptyKey),
                      static_cast<unsigned long long>(k));
      if (cur == kEmptyKey) {
        fresh = true;
        return h;
      }
    }
    if (cur == k) return h;
    h = (h + 1) & m;
  }
}

// The slot of key k or ~0: a pure read.
__device__ __forceinline__ uint64_t find_slot(const OplogRef& t, uint64_t k) {
  if (k == kEmptyKey) return *slot_at(t, t.cap) == kEmptyKey ? ~0ull : t.cap;
  const uint64_t m = t.cap - 1;
  uint64_t h = row_hash(k) & m;
  for (;;) {
    const uint64_t cur = *slot_at(t, h);
    if (cur == k) return h;
    if (cur == kEmptyKey) return ~0ull;
    h = (h + 1) & m;
  }
}

// New keys of a workgroup: *t.count += the ordinary ones, *fresh_out (may be
// null) += all of them.  Every thread of the workgroup calls it.
__device__ __forceinline__ void count_fresh(const OplogRef& t, bool fresh, bool special,
                                            uint32_t* fresh_out) {
  const uint32_t a = __popcll(__ballot(fresh)), b = __popcll(__ballot(fresh && !special));
  if (__lane_id() == 0) {
    if (b) atomicAdd(t.count, static_cast<unsigned long long>(b));
    if (a && fresh_out) atomicAdd(fresh_out, a);
  }
}

// sdgpu_oplog_add_device: L(key) = max(L(key), ts); the entering thread stores
// the tag.  slot_of (may be null): for k_log_tags.
__global__ __launch_bounds__(kThreads) void k_log_add(OplogRef t, const uint64_t* __restrict__ key,
                                                      const uint64_t* __restrict__ tag,
                                                      const int64_t* __restrict__ ts, uint64_t n,
                                                      uint32_t* __restrict__ slot_of) {
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kThreads;
  const uint64_t end = (n + kThreads - 1) / kThreads * kThreads;  // uniform trip count
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x; i < end;
       i += stride) {
    bool fresh = false, special = false;
    if (i < n) {
      const uint64_t k = key[i];
      special = k == kEmptyKey;
      const uint64_t s = enter_slot(t, k, fresh);
      uint64_t* p = slot_at(t, s);
      if (fresh) p[2] = tag[i];
      const uint64_t v = static_cast<uint64_t>(ts[i]) ^ kBias;
      if (v) atomicMax(reinterpret_cast<unsigned long long*>(p + 1),
                       static_cast<unsigned long long>(v));
      if (slot_of) slot_of[i] = static_cast<uint32_t>(s);
    }
    count_fresh(t, fresh, special, nullptr);
  }
}

// *out += the ops whose tag is not the one stored with their key (a kernel of
// its own: the entering thread's store has landed).
__global__ __launch_bounds__(kThreads) void k_log_tags(OplogRef t,
                                                       const uint64_t* __restrict__ tag,
                                                       const uint32_t* __restrict__ slot_of,
                                                       uint64_t n, uint32_t* __restrict__ out) {
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kThreads;
  uint32_t bad = 0;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x; i < n; i += stride)
    bad += slot_at(t, slot_of[i])[2] != tag[i] ? 1u : 0u;
  bad = wave_sum(bad);
  if (__lane_id() == 0 && bad) atomicAdd(out, bad);
}

__global__ __launch_bounds__(kThreads) void k_log_latest(OplogRef t,
                                                         const uint64_t* __restrict__ key,
                                                         uint64_t n, int64_t* __restrict__ ts,
                                                         uint8_t* __restrict__ found) {
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kThreads;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x; i < n;
       i += stride) {
    const uint64_t s = find_slot(t, key[i]);
    const uint64_t v = s == ~0ull ? 0ull : slot_at(t, s)[1];
    ts[i] = static_cast<int64_t>(v ^ kBias);
    found[i] = v != 0 ? 1 : 0;
  }
}

// Growth: every stored key with its timestamp and tag into the cleared table
// `to` (keys are unique: plain stores behind the CAS).
__global__ __launch_bounds__(kThreads) void k_log_rehash(OplogRef from, OplogRef to) {
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kThreads;
  const uint64_t end = (from.cap + kThreads) / kThreads * kThreads;
  for (uint64_t s = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x; s < end;
       s += stride) {
    bool fresh = false;
    if (s < from.cap) {
      const uint64_t* p = slot_at(from, s);
      if (p[0] != kEmptyKey) {
        uint64_t* q = slot_at(to, enter_slot(to, p[0], fresh));
        q[1] = p[1];
        q[2] = p[2];
      }
    } else if (s == from.cap) {
      const uint64_t* p = slot_at(from, s);
      uint64_t* q = slot_at(to, to.cap);
      q[0] = p[0];
      q[1] = p[1];
      q[2] = p[2];
    }
    count_fresh(to, fresh, false, nullptr);
  }
}

// One lane per op: slot_of[i], base[i] = the slot's logged timestamp (biased; no
// timestamp changes before k_seg_apply), new keys into counts[2], clocks.
__global__ __launch_bounds__(kThreads) void k_log_slot(OplogRef t,
                                                       const uint64_t* __restrict__ key,
                                                       const uint64_t* __restrict__ tag,
                                                       const int64_t* __restrict__ ts,
                                                       const uint32_t* __restrict__ instance,
                                                       uint64_t n, uint64_t* __restrict__ clock,
                                                       uint32_t n_instances,
                                                       uint32_t* __restrict__ slot_of,
                                                       uint64_t* __restrict__ base,
                                                       uint32_t* __restrict__ counts) {
  __shared__ unsigned long long lclk[kClockLds];
  const bool fold = clock && n_instances <= kClockLds;
  if (fold) {
    for (uint32_t j = threadIdx.x; j < n_instances; j += kThreads) lclk[j] = 0;
    __syncthreads();
  }
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kThreads;
  const uint64_t end = (n + kThreads - 1) / kThreads * kThreads;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x; i < end;
       i += stride) {
    bool fresh = false, special = false;
    if (i < n) {
      const uint64_t k = key[i];
      special = k == kEmptyKey;
      const uint64_t s = enter_slot(t, k, fresh);
      uint64_t* p = slot_at(t, s);
      if (fresh) p[2] = tag[i];
      base[i] = p[1];
      slot_of[i] = static_cast<uint32_t>(s);
      if (clock) {
        const uint32_t who = instance[i];
        const unsigned long long v = static_cast<unsigned long long>(ts[i]);
        if (who < n_instances && v) {
          if (fold) atomicMax(&lclk[who], v);
          else atomicMax(reinterpret_cast<unsigned long long*>(clock + who), v);
        }
      }
    }
    count_fresh(t, fresh, special, counts + 2);
  }
  if (fold) {
    __syncthreads();
    for (uint32_t j = threadIdx.x; j < n_instances; j += kThreads)
      if (lclk[j]) atomicMax(reinterpret_cast<unsigned long long*>(clock + j), lclk[j]);
  }
}

// ---- the stable sort of (slot, i) ------------------------------------------------
// Pass 0 reads slot_of (i implicit), later passes the pairs of the pass before.
template <bool kFirst>
__device__ __forceinline__ uint2 sort_item(const uint32_t* __restrict__ slot_of,
                                           const uint2* __restrict__ src, uint64_t p) {
  if constexpr (kFirst) return make_uint2(slot_of[p], static_cast<uint32_t>(p));
  else return src[p];
}

template <bool kFirst>
__global__ __launch_bounds__(kThreads) void k_sort_hist(const uint32_t* __restrict__ slot_of,
                                                        const uint2* __restrict__ src, uint64_t n,
                                                        uint32_t shift,
                                                        uint32_t* __restrict__ cnt) {
  __shared__ uint32_t h[kBins];
  static_assert(kBins == kThreads, "one bin per thread");
  h[threadIdx.x] = 0;
  __syncthreads();
  const uint64_t t0 = static_cast<uint64_t>(blockIdx.x) * kTile;
#pragma unroll
  for (int r = 0; r < kRounds; ++r) {
    const uint64_t p = t0 + r * kThreads + threadIdx.x;
    if (p < n) atomicAdd(&h[(sort_item<kFirst>(slot_of, src, p).x >> shift) & 255u], 1u);
  }
  __syncthreads();
  cnt[static_cast<uint64_t>(threadIdx.x) * gridDim.x + blockIdx.x] = h[threadIdx.x];  // digit-major
}

// Stable within the tile, one round of kThreads items at a time: an item's
// place in its bin = cursor + items with its digit in earlier waves of the
// round + earlier lanes of its own wave with its digit (8 ballots, one per bit
// of the digit: k_thumb_scatter's ranks).
template <bool kFirst>
__global__ __launch_bounds__(kThreads) void k_sort_scatter(const uint32_t* __restrict__ slot_of,
                                                           const uint2* __restrict__ src,
                                                           uint64_t n, uint32_t shift,
                                                           const uint32_t* __restrict__ offs,
                                                           uint2* __restrict__ dst) {
  __shared__ uint32_t cur[kBins];
  __shared__ uint32_t wcnt[kWaves][kBins];
  cur[threadIdx.x] = offs[static_cast<uint64_t>(threadIdx.x) * gridDim.x + blockIdx.x];
  const uint32_t lane = __lane_id(), wave = threadIdx.x >> 6;
  const uint64_t t0 = static_cast<uint64_t>(blockIdx.x) * kTile;
  for (int r = 0; r < kRounds; ++r) {  // uniform trip count
    const uint64_t p = t0 + r * kThreads + threadIdx.x;
    const bool v = p < n;
    const uint2 it = v ? sort_item<kFirst>(slot_of, src, p) : make_uint2(0u, 0u);
    const uint32_t b = (it.x >> shift) & 255u;
    for (uint32_t k = threadIdx.x; k < kWaves * kBins; k += kThreads) (&wcnt[0][0])[k] = 0;
    __syncthreads();
    uint64_t peers = __ballot(v);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const bool bit = (b >> k) & 1u;
      const uint64_t mk = __ballot(bit);
      peers &= bit ? mk : ~mk;
    }
    const uint32_t rank = static_cast<uint32_t>(__popcll(peers & ((1ull << lane) - 1ull)));
    if (v && rank == 0) wcnt[wave][b] = static_cast<uint32_t>(__popcll(peers));
    __syncthreads();
    if (v) {
      uint32_t q = cur[b] + rank;
      for (uint32_t w = 0; w < wave; ++w) q += wcnt[w][b];
      dst[q] = it;  // q < n: the scanned counts of all tiles sum to n
    }
    __syncthreads();
    uint32_t add = 0;
#pragma unroll
    for (uint32_t w = 0; w < kWaves; ++w) add += wcnt[w][threadIdx.x];
    cur[threadIdx.x] += add;
    __syncthreads();
  }
}

// ---- the segmented scan -----------------------------------------------------------
// (m, pos): the running maximum (biased) of a key's logged timestamp and its ops
// so far, and the op that last reached it (kNone: the logged one still stands).
// head: the run starts a key.  A later op with an equal timestamp wins.
struct Seg {
  uint64_t m;
  uint32_t pos;
  uint32_t head;
};
__device__ __forceinline__ Seg seg_none() { return Seg{0ull, kNone, 0u}; }
// a then b; pos == kNone without head is only seg_none(): every op has a pos,
// and a head run at least its head mark
__device__ __forceinline__ Seg seg_join(const Seg& a, const Seg& b) {
  if (b.head) return b;
  if (b.pos == kNone) return a;
  return b.m >= a.m ? Seg{b.m, b.pos, a.head} : a;
}
__device__ __forceinline__ Seg seg_shfl_up(const Seg& v, int d) {
  Seg r;
  r.m = __shfl_up(static_cast<unsigned long long>(v.m), d);
  r.pos = __shfl_up(v.pos, d);
  r.head = __shfl_up(v.head, d);
  return r;
}

// Exclusive scan of one Seg per thread over a workgroup of kN threads, in
// thread order; `total` = the join of all.  sw: kN / 64 entries of LDS.
template <int kN>
__device__ __forceinline__ Seg seg_block_exclusive(const Seg& mine, Seg* sw, Seg& total) {
  const uint32_t lane = __lane_id(), w = threadIdx.x >> 6;
  Seg inc = mine;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const Seg o = seg_shfl_up(inc, d);
    if (lane >= static_cast<uint32_t>(d)) inc = seg_join(o, inc);
  }
  if (lane == 63) sw[w] = inc;
  Seg ex = seg_shfl_up(inc, 1);
  if (lane == 0) ex = seg_none();
  __syncthreads();
  Seg pre = seg_none();
  total = seg_none();
  for (uint32_t k = 0; k < kN / 64; ++k) {
    const Seg x = sw[k];
    if (k < w) pre = seg_join(pre, x);
    total = seg_join(total, x);
  }
  __syncthreads();  // sw may be rewritten by the caller's next round
  return seg_join(pre, ex);
}

// A thread's kRounds consecutive sorted positions from p0: op i, its slot, and
// whether it starts / ends its key's run.
struct SegItems {
  uint32_t slot[kRounds], i[kRounds];
  uint64_t v[kRounds];  // the op's biased timestamp
  uint32_t head, tail, in;  // bit r
};
__device__ __forceinline__ void seg_load(const uint2* __restrict__ pairs,
                                         const int64_t* __restrict__ ts, uint64_t n, uint64_t p0,
                                         SegItems& q) {
  q.head = q.tail = q.in = 0;
  const uint32_t before = p0 > 0 && p0 <= n ? pairs[p0 - 1].x : kNone;
  uint32_t after = kNone;
#pragma unroll
  for (int r = 0; r < kRounds; ++r) {
    const uint64_t p = p0 + r;
    const uint2 it = pairs[min(p, n - 1)];
    q.slot[r] = it.x;
    q.i[r] = it.y;
    q.in |= (p < n ? 1u : 0u) << r;
  }
  if (p0 + kRounds < n) after = pairs[p0 + kRounds].x;
#pragma unroll
  for (int r = 0; r < kRounds; ++r) q.v[r] = static_cast<uint64_t>(ts[q.i[r]]) ^ kBias;
#pragma unroll
  for (int r = 0; r < kRounds; ++r) {
    const uint64_t p = p0 + r;
    if (p >= n) continue;
    const bool h = r == 0 ? (p == 0 || before != q.slot[0]) : q.slot[r - 1] != q.slot[r];
    const bool t = p + 1 == n ||
                   (r == kRounds - 1 ? after != q.slot[r] : q.slot[r + 1] != q.slot[r]);
    q.head |= (h ? 1u : 0u) << r;
    q.tail |= (t ? 1u : 0u) << r;
  }
}
// the op at round r as a run of one: a head is seeded with the logged timestamp
__device__ __forceinline__ Seg seg_item(const SegItems& q, int r, uint64_t logged) {
  if (q.head >> r & 1u)
    return q.v[r] >= logged ? Seg{q.v[r], q.i[r], 1u} : Seg{logged, kNone, 1u};
  return Seg{q.v[r], q.i[r], 0u};
}

__device__ __forceinline__ Seg seg_thread(const SegItems& q, const uint64_t* __restrict__ base) {
  Seg a = seg_none();
#pragma unroll
  for (int r = 0; r < kRounds; ++r) {
    if (!(q.in >> r & 1u)) continue;
    const uint64_t logged = (q.head >> r & 1u) ? base[q.i[r]] : 0ull;
    a = seg_join(a, seg_item(q, r, logged));
  }
  return a;
}

__global__ __launch_bounds__(kThreads) void k_seg_agg(const uint2* __restrict__ pairs,
                                                      const int64_t* __restrict__ ts,
                                                      const uint64_t* __restrict__ base,
                                                      uint64_t n, Seg* __restrict__ agg) {
  __shared__ Seg sw[kWaves];
  SegItems q;
  seg_load(pairs, ts, n, static_cast<uint64_t>(blockIdx.x) * kTile + threadIdx.x * kRounds, q);
  Seg total;
  (void)seg_block_exclusive<kThreads>(seg_thread(q, base), sw, total);
  if (threadIdx.x == 0) agg[blockIdx.x] = total;
}

// One workgroup: agg[b] = the join of the tiles before b.
constexpr int kCarryThreads = 1024;
__global__ __launch_bounds__(kCarryThreads) void k_seg_carry(Seg* __restrict__ agg,
                                                             uint32_t tiles) {
  __shared__ Seg sw[kCarryThreads / 64];
  Seg carry = seg_none();
  for (uint32_t b0 = 0; b0 < tiles; b0 += kCarryThreads) {
    const uint32_t b = b0 + threadIdx.x;
    const Seg mine = b < tiles ? agg[b] : seg_none();
    Seg total;
    const Seg ex = seg_block_exclusive<kCarryThreads>(mine, sw, total);
    if (b < tiles) agg[b] = seg_join(carry, ex);
    carry = seg_join(carry, total);
  }
}

// apply[i] for every op from the exclusive value of its position; a run's tail
// commits the run's maximum (unless no op of it reached the logged one, or
// NO_COMMIT) and marks the winner; the ops whose tag is not their slot's are
// counted into counts[3].
__global__ __launch_bounds__(kThreads) void k_seg_apply(
    OplogRef t, const uint2* __restrict__ pairs, const int64_t* __restrict__ ts,
    const uint64_t* __restrict__ tag, const uint64_t* __restrict__ base, uint64_t n,
    const Seg* __restrict__ carry, bool commit, uint8_t* __restrict__ apply,
    uint8_t* __restrict__ win, uint32_t* __restrict__ counts) {
  __shared__ Seg sw[kWaves];
  SegItems q;
  seg_load(pairs, ts, n, static_cast<uint64_t>(blockIdx.x) * kTile + threadIdx.x * kRounds, q);
  uint64_t stored[kRounds], mine[kRounds];
#pragma unroll
  for (int r = 0; r < kRounds; ++r) {  // the slot's sector: k_log_slot just touched it
    stored[r] = slot_at(t, q.slot[r])[2];
    mine[r] = tag[q.i[r]];
  }
  Seg total;
  Seg run = seg_join(carry[blockIdx.x],
                     seg_block_exclusive<kThreads>(seg_thread(q, base), sw, total));
  uint32_t bad = 0;
#pragma unroll
  for (int r = 0; r < kRounds; ++r) {
    if (!(q.in >> r & 1u)) continue;
    const bool head = q.head >> r & 1u;
    const uint64_t logged = head ? base[q.i[r]] : 0ull;
    const uint64_t before = head ? logged : run.m;
    apply[q.i[r]] = q.v[r] >= before ? 1 : 0;
    run = seg_join(run, seg_item(q, r, logged));
    if ((q.tail >> r & 1u) && run.pos != kNone) {
      if (commit) slot_at(t, q.slot[r])[1] = run.m;
      win[run.pos] = 1;
    }
    bad += stored[r] != mine[r] ? 1u : 0u;
  }
  bad = wave_sum(bad);
  if (__lane_id() == 0 && bad) atomicAdd(&counts[3], bad);
}

// ---- applied and winner as one compaction -------------------------------------------
// Blocks [0, bt) list apply[n], [bt, 2 bt) win[n]; a tile is compact::kRows x kThreads
// positions, position tile + k * kThreads + t, and (k, t) order is index order.
__device__ __forceinline__ uint32_t list_bits(const uint8_t* __restrict__ src, uint64_t n,
                                              uint64_t tile) {
  uint8_t v[compact::kRows];
#pragma unroll
  for (int k = 0; k < compact::kRows; ++k) v[k] = src[min(tile + k * kThreads + threadIdx.x, n - 1)];
  uint32_t f = 0;
#pragma unroll
  for (int k = 0; k < compact::kRows; ++k)
    f |= (tile + k * kThreads + threadIdx.x < n && v[k] != 0 ? 1u : 0u) << k;
  return f;
}

__global__ __launch_bounds__(kThreads) void k_ing_count(const uint8_t* __restrict__ apply,
                                                        const uint8_t* __restrict__ win,
                                                        uint64_t n, uint32_t bt,
                                                        uint32_t* __restrict__ cnt) {
  const bool second = blockIdx.x >= bt;
  const uint32_t f = list_bits(second ? win : apply, n,
                               static_cast<uint64_t>(blockIdx.x - (second ? bt : 0)) * compact::kTile);
  const uint32_t a = compact::tile_count(f);
  if (threadIdx.x == 0) cnt[blockIdx.x] = a;
}

__global__ __launch_bounds__(kThreads) void k_ing_write(const uint8_t* __restrict__ apply,
                                                        const uint8_t* __restrict__ win,
                                                        uint64_t n, uint32_t bt,
                                                        const uint32_t* __restrict__ offs,
                                                        uint32_t* __restrict__ applied,
                                                        uint32_t* __restrict__ winner,
                                                        uint32_t* __restrict__ counts) {
  __shared__ uint32_t off[compact::kRows][compact::kWaves];
  const bool second = blockIdx.x >= bt;
  const uint32_t first = second ? bt : 0;
  const uint64_t tile = static_cast<uint64_t>(blockIdx.x - first) * compact::kTile;
  uint32_t* out = second ? winner : applied;
  const uint32_t w = threadIdx.x >> 6;
  const uint32_t f = list_bits(second ? win : apply, n, tile);
  uint32_t pre[compact::kRows];
  compact::tile_offsets(f, [&] { return offs[blockIdx.x] - offs[first]; }, off, pre);
#pragma unroll
  for (int k = 0; k < compact::kRows; ++k)
    if (f >> k & 1u)
      out[off[k][w] + pre[k]] = static_cast<uint32_t>(tile + k * kThreads + threadIdx.x);
  if (blockIdx.x == 0 && threadIdx.x < 2)
    counts[threadIdx.x] = offs[(threadIdx.x + 1) * bt] - offs[threadIdx.x * bt];
}

struct IngWs {
  uint32_t* slot_of;  // [n]
  uint64_t* base;     // [n] the logged timestamp of every op's slot (biased)
  uint2* pair[2];     // [n] each: the sort's two buffers
  uint8_t* win;       // [n] zeroed by the call
  uint32_t tiles;     // sort / scan tiles
  uint32_t* cnt;      // [256 tiles + 1] digit-major tile counts, then offsets
  uint32_t* cnt_sums; // scan::exclusive's tile sums
  Seg* agg;           // [tiles]
  uint32_t bt;        // compaction tiles per list
  uint32_t* lcnt;     // [2 bt + 1]
  uint32_t* lcnt_sums;
  size_t bytes;
};

IngWs ing_ws(uint64_t n, void* ws) {
  IngWs w;
  Carve c(ws);
  w.tiles = static_cast<uint32_t>((n + kTile - 1) / kTile);
  w.bt = static_cast<uint32_t>(compact::tiles_for(n));
  w.slot_of = c.take<uint32_t>(n);
  w.base = c.take<uint64_t>(n);
  w.pair[0] = c.take<uint2>(n);
  w.pair[1] = c.take<uint2>(n);
  w.win = c.take(n);
  const uint64_t nh = static_cast<uint64_t>(kBins) * w.tiles;
  w.cnt = c.take<uint32_t>(nh + 1);
  w.cnt_sums = c.take<uint32_t>(static_cast<size_t>(scan::tiles_for(nh)) + 1);
  w.agg = c.take<Seg>(w.tiles);
  w.lcnt = c.take<uint32_t>(2ull * w.bt + 1);
  w.lcnt_sums = c.take<uint32_t>(static_cast<size_t>(scan::tiles_for(2ull * w.bt)) + 1);
  w.bytes = c.bytes();
  return w;
}

}  // namespace

uint32_t oplog_sort_passes(uint64_t cap) {
  uint32_t bits = 1;  // slot numbers are 0 .. cap, the key ~0's slot included
  while ((1ull << bits) <= cap) ++bits;
  return (bits + 7) / 8;
}

hipError_t oplog_clear_launch(const OplogRef& t, hipStream_t s) {
  k_log_clear<<<grid_for(t.cap + 1, kThreads, kMaxGrid), kThreads, 0, s>>>(t);
  return hipGetLastError();
}

hipError_t oplog_rehash_launch(const OplogRef& from, const OplogRef& to, hipStream_t s) {
  k_log_clear<<<grid_for(to.cap + 1, kThreads, kMaxGrid), kThreads, 0, s>>>(to);
  k_log_rehash<<<grid_for(from.cap + 1, kThreads, kMaxGrid), kThreads, 0, s>>>(from, to);
  return hipGetLastError();
}

size_t oplog_add_workspace_bytes(uint64_t n, bool collisions) { return collisions ? 4 * n : 0; }

hipError_t oplog_add_launch(const OplogRef& t, const uint64_t* key, const uint64_t* tag,
                            const int64_t* ts, uint64_t n, uint32_t* collisions, void* ws,
                            hipStream_t s, KTimer* timer) {
  if (collisions) {
    const hipError_t e = hipMemsetAsync(collisions, 0, sizeof(uint32_t), s);
    if (e != hipSuccess) return e;
  }
  if (n == 0) return hipSuccess;
  uint32_t* slot_of = collisions ? static_cast<uint32_t*>(ws) : nullptr;
  {
    KScope k(timer, "log_add", s);
    k_log_add<<<grid_for(n, kThreads, kMaxGrid), kThreads, 0, s>>>(t, key, tag, ts, n, slot_of);
  }
  if (collisions) {
    KScope k(timer, "log_tags", s);
    k_log_tags<<<grid_for(n, kThreads, kMaxGrid), kThreads, 0, s>>>(t, tag, slot_of, n, collisions);
  }
  return hipGetLastError();
}

hipError_t oplog_latest_launch(const OplogRef& t, const uint64_t* key, uint64_t n, int64_t* ts,
                               uint8_t* found, hipStream_t s, KTimer* timer) {
  if (n == 0) return hipSuccess;
  KScope k(timer, "log_latest", s);
  k_log_latest<<<grid_for(n, kThreads, kMaxGrid), kThreads, 0, s>>>(t, key, n, ts, found);
  return hipGetLastError();
}

size_t sync_ingest_workspace_bytes(uint64_t n) { return ing_ws(n, nullptr).bytes; }

hipError_t sync_ingest_launch(const OplogRef& t, const uint64_t* key, const uint64_t* tag,
                              const int64_t* ts, const uint32_t* instance, uint64_t n,
                              uint64_t* clock, uint32_t n_instances, bool commit, uint8_t* apply,
                              uint32_t* applied, uint32_t* winner, uint32_t* counts, void* ws,
                              hipStream_t s, KTimer* timer) {
  hipError_t e = hipMemsetAsync(counts, 0, 4 * sizeof(uint32_t), s);
  if (e != hipSuccess || n == 0) return e;
  const IngWs w = ing_ws(n, ws);
  e = hipMemsetAsync(w.win, 0, n, s);
  if (e != hipSuccess) return e;
  {
    KScope k(timer, "ing_slot", s);
    k_log_slot<<<grid_for(n, kThreads, kMaxGrid), kThreads, 0, s>>>(t, key, tag, ts, instance, n, clock,
                                                          n_instances, w.slot_of, w.base, counts);
  }
  const uint32_t passes = oplog_sort_passes(t.cap);
  const uint64_t nh = static_cast<uint64_t>(kBins) * w.tiles;
  {
    KScope k(timer, "ing_sort", s);
    for (uint32_t pass = 0; pass < passes; ++pass) {
      const uint2* src = pass ? w.pair[(pass - 1) & 1] : nullptr;
      uint2* dst = w.pair[pass & 1];
      if (pass == 0) k_sort_hist<true><<<w.tiles, kThreads, 0, s>>>(w.slot_of, src, n, 0, w.cnt);
      else k_sort_hist<false><<<w.tiles, kThreads, 0, s>>>(w.slot_of, src, n, 8 * pass, w.cnt);
      scan::exclusive(w.cnt, nh, w.cnt, w.cnt_sums, nullptr, s);
      if (pass == 0)
        k_sort_scatter<true><<<w.tiles, kThreads, 0, s>>>(w.slot_of, src, n, 0, w.cnt, dst);
      else
        k_sort_scatter<false><<<w.tiles, kThreads, 0, s>>>(w.slot_of, src, n, 8 * pass, w.cnt, dst);
    }
  }
  const uint2* sorted = w.pair[(passes - 1) & 1];
  {
    KScope k(timer, "ing_scan", s);
    k_seg_agg<<<w.tiles, kThreads, 0, s>>>(sorted, ts, w.base, n, w.agg);
    k_seg_carry<<<1, kCarryThreads, 0, s>>>(w.agg, w.tiles);
    k_seg_apply<<<w.tiles, kThreads, 0, s>>>(t, sorted, ts, tag, w.base, n, w.agg, commit, apply,
                                             w.win, counts);
  }
  {
    KScope k(timer, "ing_lists", s);
    k_ing_count<<<2 * w.bt, kThreads, 0, s>>>(apply, w.win, n, w.bt, w.lcnt);
    scan::exclusive(w.lcnt, 2ull * w.bt, w.lcnt, w.lcnt_sums, nullptr, s);
    k_ing_write<<<2 * w.bt, kThreads, 0, s>>>(apply, w.win, n, w.bt, w.lcnt, applied, winner,
                                              counts);
  }
  return hipGetLastError();
}

}  // namespace sdgpu
