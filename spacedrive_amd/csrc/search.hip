// Explorer: one search page (filter, order, cursor, take) as one device query.
//
// Reference: core/src/api/search.rs:393-562 (search.paths) builds a WHERE clause
// over file_path and its Object (:127-187, :302-324), orders by is_dir DESC,
// <field>, id, applies a keyset cursor (:446-528) or an offset and takes at most
// 100 rows; pathsCount (:563-582) is the filter alone.  include/sdgpu.h states
// the semantics; here they run over columns that already live on the device, on
// one stream with no host synchronisation:
//   1. k_search_tags (only with TAGS): one pass over the tag_on_object pairs,
//      mark[obj] = 1 when the pair's tag is in the query's set -- a plain byte
//      store, the remover's hit[slot] = 1 idiom;
//   2. k_search_filter: one pass over the rows, loading only the columns the
//      query uses and gathering the Object columns through object[i]; counts
//      from wave ballots; every candidate is appended as a record {okey, row}
//      (12 bytes, kept as two arrays) with one atomic per workgroup tile.  With
//      k63 = key + 2^62 (0 for NULL and for no order key)
//        okey = (GROUP_DIRS && !is_dir) << 63 | (DESC ? 2^63 - 1 - k63 : k63)
//      so (okey, row) is a 96-bit key with no duplicates whose ascending order
//      is the page's order;
//   3. the selection: an MSB-first radix select over the 96-bit key, 11-bit
//      digits (eight of them, then the last 8 bits).  A pass histograms the
//      survivors' digit (LDS, then global), finds the bucket that holds the
//      wanted rank and compacts that bucket into the other buffer.  The host
//      enqueues the fixed worst-case sequence; a pass whose input already has
//      at most kFinal records returns on the state the pass before it left.
//      Then one workgroup sorts the survivors in LDS (bitonic) and writes the
//      page.
//      offset == 0 (cursor mode, the explorer's own): one selection of the ranks
//      [0, take): the buckets below the one that holds rank take - 1 are wholly
//      in the page and go to a winners list of at most 255 records, which the
//      final sort merges with the survivors.
//      offset > 0: first the record R of rank offset (one selection of a single
//      rank, no winners), then the take smallest records not below R: the same
//      selection with the filter (okey, row) >= R.  The work does not grow with
//      offset.
#include "../../include/sdgpu.h"
#include "internal.hpp"

namespace sdgpu {

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr uint32_t kFinal = SDGPU_SEARCH_SELECT_FINAL;  // records the last sort takes from a pass
constexpr uint32_t kMaxTake = SDGPU_SEARCH_MAX_TAKE;
constexpr uint32_t kSortCap = 4096;                     // LDS sort: survivors + winners
static_assert(kFinal + kMaxTake <= kSortCap, "the final sort holds the survivors and the winners");
constexpr int kPasses = 9;                              // 8 x 11 bits + 8 bits = 96
constexpr uint32_t kBins = 2048;
constexpr int64_t kNull = SDGPU_SEARCH_NULL;

constexpr int kFRows = 4;                               // rows per thread and tile of the filter
constexpr uint64_t kFTile = static_cast<uint64_t>(kFRows) * kThreads;
constexpr int kSRows = 8;                               // records per thread and tile of a pass
constexpr uint64_t kSTile = static_cast<uint64_t>(kSRows) * kThreads;
constexpr uint32_t kSelBlocks = 512;                    // two workgroups per CU

// One selection's control block; zeroed on the stream before the filter runs,
// except state[] and r_*, which k_sel_begin and the passes write before any
// kernel reads them.
struct SelState {
  uint32_t scan;  // records in the pass's source buffer
  uint32_t k;     // wanted rank among those of them that pass the filter
  uint32_t fin;   // pass + 1 whose source buffer the final sort reads, 0: none yet
  uint32_t pad;
};
struct SelCtl {
  uint32_t hist[kPasses][kBins];
  uint32_t cursor[kPasses];  // records compacted by each pass
  uint32_t wcount;           // winners
  uint32_t P;                // the page's length
  SelState state[kPasses + 1];
  uint64_t r_key;            // the filter: records (okey, row) >= (r_key, r_row)
  uint32_t r_row;
  uint32_t pad;
};

struct SearchWs {
  uint8_t* mark;     // [m] Objects with a wanted tag
  SelCtl* ctl;       // [2]
  uint64_t* key[3];  // candidates, then the passes' two buffers
  uint32_t* row[3];
  uint64_t* wkey;    // [kMaxTake] winners
  uint32_t* wrow;
  size_t bytes;
};

SearchWs search_ws(uint64_t n, uint64_t m, void* ws) {
  SearchWs w;
  Carve c(ws);
  w.mark = c.take(m);
  w.ctl = c.take<SelCtl>(2);
  for (int b = 0; b < 3; ++b) {
    w.key[b] = c.take<uint64_t>(n);
    w.row[b] = c.take<uint32_t>(n);
  }
  w.wkey = c.take<uint64_t>(kMaxTake);
  w.wrow = c.take<uint32_t>(kMaxTake);
  w.bytes = c.bytes();
  return w;
}

// Device pointers and operands of one call, by value.
struct SearchArgs {
  sdgpu_search_rows_t r;
  sdgpu_search_objects_t o;  // m == 0 and NULL columns when the call has none
  sdgpu_search_query_t q;
  bool have_objects;
};

struct TagSet {
  int32_t tag[32];
  uint32_t n;
};

__global__ __launch_bounds__(kThreads) void k_search_tags(const int32_t* __restrict__ tag_obj,
                                                          const int32_t* __restrict__ tag_tag,
                                                          uint64_t n_pairs, uint64_t m, TagSet set,
                                                          uint8_t* __restrict__ mark) {
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kThreads;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x; i < n_pairs;
       i += stride) {
    const int32_t t = tag_tag[i];
    bool in = false;
    for (uint32_t j = 0; j < set.n; ++j) in |= set.tag[j] == t;
    const int32_t o = tag_obj[i];
    if (in && o >= 0 && static_cast<uint64_t>(o) < m) mark[o] = 1;
  }
}

__device__ inline uint32_t lane_id() { return threadIdx.x & 63u; }
__device__ inline uint32_t rank_in(uint64_t ballot) {
  return static_cast<uint32_t>(__popcll(ballot & ((1ull << lane_id()) - 1ull)));
}

// One pass over the rows, kFRows rows per thread in tiles of kFTile.  The
// branches on q.use / q.flags are uniform over the grid.  counts[0], [1], [3]
// (zero on entry); counts[1] doubles as the append cursor, advanced once per
// tile by the workgroup's first thread.
__global__ __launch_bounds__(kThreads) void k_search_filter(SearchArgs a,
                                                            const uint8_t* __restrict__ mark,
                                                            uint64_t* __restrict__ out_key,
                                                            uint32_t* __restrict__ out_row,
                                                            uint32_t* __restrict__ counts) {
  __shared__ uint32_t s_wave[kWaves];
  __shared__ uint32_t s_base;
  __shared__ uint32_t s_tot[2][kWaves];
  const sdgpu_search_rows_t& r = a.r;
  const sdgpu_search_objects_t& ob = a.o;
  const sdgpu_search_query_t& q = a.q;
  const uint32_t use = q.use, fl = q.flags;
  const bool obj_terms =
      (use & (SDGPU_SEARCH_USE_FAVORITE | SDGPU_SEARCH_USE_HIDDEN_EXCLUDE | SDGPU_SEARCH_USE_KIND |
              SDGPU_SEARCH_USE_TAGS | SDGPU_SEARCH_USE_ACCESSED_EQ |
              SDGPU_SEARCH_USE_ACCESSED_NE)) != 0;
  const bool need_obj = obj_terms || (fl & SDGPU_SEARCH_NEEDS_OBJECT);
  const bool by_obj = (fl & SDGPU_SEARCH_ORDER_BY_OBJECT) != 0;
  const bool load_obj = need_obj || by_obj;
  const bool desc = (fl & SDGPU_SEARCH_DESC) != 0;
  const int64_t* okcol = by_obj ? ob.order_key : r.order_key;
  // ORDER_BY_OBJECT is an order key even with no Object column to read (m == 0):
  // every row's key is then NULL
  const bool has_key = by_obj || r.order_key != nullptr;
  const uint32_t wave = threadIdx.x >> 6;
  uint32_t n_match = 0, n_dirs = 0;  // per wave, kept by every lane alike

  const uint64_t tiles = (r.n + kFTile - 1) / kFTile;
  for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    uint64_t okey[kFRows];
    uint64_t cb[kFRows];
    uint32_t mine = 0;
#pragma unroll
    for (int u = 0; u < kFRows; ++u) {
      const uint64_t i = t * kFTile + static_cast<uint64_t>(u) * kThreads + threadIdx.x;
      bool match = i < r.n;
      bool is_dir = false;
      int64_t v = kNull;
      if (match) {
        if (r.eligible) match = r.eligible[i] != 0;
        if (r.flags) is_dir = (r.flags[i] & 1u) != 0;
        if (use & SDGPU_SEARCH_USE_LOCATION) {
          const int32_t x = r.location[i];
          match &= x != -1 && x == q.location;
        }
        if (use & SDGPU_SEARCH_USE_EXTENSION) {
          const uint16_t x = r.ext[i];
          match &= x != 0xFFFFu && x == q.ext;
        }
        if (use & (SDGPU_SEARCH_USE_CREATED_FROM | SDGPU_SEARCH_USE_CREATED_TO)) {
          const int64_t x = r.date_created[i];
          match &= x != kNull;
          if (use & SDGPU_SEARCH_USE_CREATED_FROM) match &= x >= q.created_from;
          if (use & SDGPU_SEARCH_USE_CREATED_TO) match &= x <= q.created_to;
        }
        if (use & SDGPU_SEARCH_USE_DIR) match &= r.dir_key[i] == q.dir_key;
        int32_t o = -1;
        if (load_obj) {
          o = r.object[i];
          // an index past the Object columns is read as no Object
          if (o < 0 || (a.have_objects && static_cast<uint64_t>(o) >= ob.m)) o = -1;
        }
        if (need_obj) match &= o >= 0;
        if (obj_terms && match) {
          if (use & (SDGPU_SEARCH_USE_FAVORITE | SDGPU_SEARCH_USE_HIDDEN_EXCLUDE)) {
            const uint32_t f = ob.flags[o];
            if (use & SDGPU_SEARCH_USE_HIDDEN_EXCLUDE) match &= (f & 4u) == 0;
            if (use & SDGPU_SEARCH_USE_FAVORITE)
              match &= q.favorite ? (f & 1u) != 0 : (f & 3u) == 0;
          }
          if (use & SDGPU_SEARCH_USE_KIND) {
            const int32_t k = ob.kind[o];
            match &= k >= 0 && k < 32 && ((q.kind_mask >> k) & 1u);
          }
          if (use & SDGPU_SEARCH_USE_TAGS) match &= mark[o] != 0;
          if (use & (SDGPU_SEARCH_USE_ACCESSED_EQ | SDGPU_SEARCH_USE_ACCESSED_NE)) {
            const int64_t x = ob.date_accessed[o];
            if (use & SDGPU_SEARCH_USE_ACCESSED_EQ) match &= x == q.accessed_eq;
            if (use & SDGPU_SEARCH_USE_ACCESSED_NE)
              match &= q.accessed_ne == kNull ? x != kNull : (x != kNull && x != q.accessed_ne);
          }
        }
        if (has_key && match) {
          if (!by_obj) v = okcol[i];
          else if (o >= 0) v = okcol[o];
        }
      }
      bool cand = match;
      if (fl & SDGPU_SEARCH_FILES_ONLY) cand &= !is_dir;
      if (fl & SDGPU_SEARCH_CURSOR) {
        const int64_t cr = q.cursor_row;
        const int64_t ii = static_cast<int64_t>(i);
        if (!has_key) {
          cand &= ii >= cr;
        } else {
          const int64_t c = q.cursor_key;
          const bool tie = !(fl & SDGPU_SEARCH_CURSOR_STRICT) && v == c;
          const bool pass = desc ? (v < c || (tie && ii < cr)) : (v > c || (tie && ii >= cr));
          cand &= v != kNull && pass;
        }
      }
      const uint64_t k63 =
          (has_key && v != kNull) ? (static_cast<uint64_t>(v) + (1ull << 62)) & ~(1ull << 63) : 0;
      okey[u] = (((fl & SDGPU_SEARCH_GROUP_DIRS) && !is_dir) ? 1ull << 63 : 0ull) |
                (desc ? (1ull << 63) - 1 - k63 : k63);
      n_match += static_cast<uint32_t>(__popcll(__ballot(match)));
      n_dirs += static_cast<uint32_t>(__popcll(__ballot(match && is_dir)));
      cb[u] = __ballot(cand);
      mine += static_cast<uint32_t>(__popcll(cb[u]));
    }
    // reserve the tile's slots: wave totals, one atomic, then every wave's base
    if (lane_id() == 0) s_wave[wave] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
      uint32_t tot = 0;
#pragma unroll
      for (int w = 0; w < kWaves; ++w) tot += s_wave[w];
      s_base = tot ? atomicAdd(&counts[1], tot) : 0;
    }
    __syncthreads();
    uint32_t at = s_base;
    for (uint32_t w = 0; w < wave; ++w) at += s_wave[w];
#pragma unroll
    for (int u = 0; u < kFRows; ++u) {
      if ((cb[u] >> lane_id()) & 1ull) {
        const uint32_t slot = at + rank_in(cb[u]);
        out_key[slot] = okey[u];
        out_row[slot] = static_cast<uint32_t>(t * kFTile + static_cast<uint64_t>(u) * kThreads +
                                              threadIdx.x);
      }
      at += static_cast<uint32_t>(__popcll(cb[u]));
    }
    __syncthreads();  // s_wave / s_base are rewritten by the next tile
  }
  if (lane_id() == 0) {
    s_tot[0][wave] = n_match;
    s_tot[1][wave] = n_dirs;
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    uint32_t tot = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) tot += s_tot[threadIdx.x][w];
    if (tot) atomicAdd(&counts[threadIdx.x == 0 ? 0 : 3], tot);
  }
}

// After the filter: the page's length and the first state of both selections.
// with_rank (offset > 0): ctl[0] selects the record of rank offset, ctl[1] then
// the P smallest records not below it; otherwise ctl[1] alone runs.
__global__ void k_sel_begin(uint32_t* __restrict__ counts, int64_t offset, uint32_t take,
                            SelCtl* __restrict__ ctl) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const int64_t cand = counts[1];
  int64_t left = cand - offset;
  if (left < 0) left = 0;
  const uint32_t P = static_cast<uint32_t>(left < take ? left : take);
  counts[2] = P;
  for (int c = 0; c < 2; ++c) {
    ctl[c].P = P;
    ctl[c].r_key = 0;
    ctl[c].r_row = 0;
    ctl[c].state[0].scan = P ? static_cast<uint32_t>(cand) : 0;
    ctl[c].state[0].fin = 0;
  }
  ctl[0].state[0].k = static_cast<uint32_t>(P ? offset : 0);
  ctl[1].state[0].k = P ? P - 1 : 0;
}

__device__ inline uint32_t digit_of(uint64_t key, uint32_t row, int pass) {
  if (pass < 5) return static_cast<uint32_t>(key >> (53 - 11 * pass)) & 0x7FFu;  // key bits
  const uint64_t lo = (key << 32) | row;  // the low 64 of the 96 bits
  if (pass < 8) return static_cast<uint32_t>(lo >> (85 - 11 * pass)) & 0x7FFu;
  return row & 0xFFu;
}
__device__ inline bool not_below(uint64_t key, uint32_t row, uint64_t rk, uint32_t rr) {
  return key > rk || (key == rk && row >= rr);
}

// Histogram of the pass's digit over the source records that pass the filter.
__global__ __launch_bounds__(kThreads) void k_sel_hist(SelCtl* __restrict__ ctl, int pass,
                                                       const uint64_t* __restrict__ key,
                                                       const uint32_t* __restrict__ row) {
  __shared__ uint32_t s_hist[kBins];
  const SelState st = ctl->state[pass];
  if (st.fin || st.scan <= kFinal) return;
  const uint64_t tiles = (st.scan + kSTile - 1) / kSTile;
  if (blockIdx.x >= tiles) return;
  for (uint32_t b = threadIdx.x; b < kBins; b += kThreads) s_hist[b] = 0;
  __syncthreads();
  const uint64_t rk = ctl->r_key;
  const uint32_t rr = ctl->r_row;
  for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
#pragma unroll
    for (int u = 0; u < kSRows; ++u) {
      const uint64_t i = t * kSTile + static_cast<uint64_t>(u) * kThreads + threadIdx.x;
      if (i < st.scan) {
        const uint64_t k = key[i];
        const uint32_t r = row[i];
        if (not_below(k, r, rk, rr)) atomicAdd(&s_hist[digit_of(k, r, pass)], 1u);
      }
    }
  }
  __syncthreads();
  for (uint32_t b = threadIdx.x; b < kBins; b += kThreads)
    if (s_hist[b]) atomicAdd(&ctl->hist[pass][b], s_hist[b]);
}

// Every workgroup finds the bucket that holds rank k from the pass's global
// histogram, then compacts that bucket's records into dst (slots reserved with
// one atomic per tile, as the filter does); with `collect` the
// records of the buckets below it, all of them in the page, go to the winners.
// The first workgroup leaves the next pass's state.
__global__ __launch_bounds__(kThreads) void k_sel_compact(SelCtl* __restrict__ ctl, int pass,
                                                          bool collect,
                                                          const uint64_t* __restrict__ key,
                                                          const uint32_t* __restrict__ row,
                                                          uint64_t* __restrict__ dst_key,
                                                          uint32_t* __restrict__ dst_row,
                                                          uint64_t* __restrict__ wkey,
                                                          uint32_t* __restrict__ wrow) {
  __shared__ uint32_t s_sum[kThreads];
  __shared__ uint32_t s_bucket, s_below, s_size;
  __shared__ uint32_t s_wave[kWaves];
  __shared__ uint32_t s_base;
  const SelState st = ctl->state[pass];
  if (st.fin || st.scan <= kFinal) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      SelState nx = st;
      if (!nx.fin) nx.fin = static_cast<uint32_t>(pass) + 1;
      ctl->state[pass + 1] = nx;
    }
    return;
  }
  const uint64_t tiles = (st.scan + kSTile - 1) / kSTile;
  if (blockIdx.x >= tiles) return;
  // bins 8 t .. 8 t + 7 belong to thread t
  constexpr uint32_t kPer = kBins / kThreads;
  uint32_t h[kPer];
  uint32_t mine = 0;
#pragma unroll
  for (uint32_t j = 0; j < kPer; ++j) {
    h[j] = ctl->hist[pass][threadIdx.x * kPer + j];
    mine += h[j];
  }
  s_sum[threadIdx.x] = mine;
  if (threadIdx.x == 0) {
    s_bucket = kBins - 1;
    s_below = 0;
    s_size = 0;
  }
  __syncthreads();
  // inclusive scan of the 256 sums (Hillis-Steele in LDS)
  for (uint32_t d = 1; d < kThreads; d <<= 1) {
    const uint32_t x = threadIdx.x >= d ? s_sum[threadIdx.x - d] : 0;
    __syncthreads();
    s_sum[threadIdx.x] += x;
    __syncthreads();
  }
  {
    uint32_t below = s_sum[threadIdx.x] - mine;
    if (st.k >= below && st.k < below + mine) {
#pragma unroll
      for (uint32_t j = 0; j < kPer; ++j) {
        if (st.k >= below && st.k < below + h[j]) {
          s_bucket = threadIdx.x * kPer + j;
          s_below = below;
          s_size = h[j];
        }
        below += h[j];
      }
    }
  }
  __syncthreads();
  const uint32_t bucket = s_bucket, below = s_below;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    SelState nx;
    nx.scan = s_size;
    nx.k = st.k - below;
    nx.fin = 0;
    nx.pad = 0;
    ctl->state[pass + 1] = nx;
  }
  const uint64_t rk = ctl->r_key;
  const uint32_t rr = ctl->r_row;
  const uint32_t wave = threadIdx.x >> 6;
  for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    uint64_t k[kSRows], kb[kSRows];
    uint32_t r[kSRows];
    uint32_t mine = 0;
#pragma unroll
    for (int u = 0; u < kSRows; ++u) {
      const uint64_t i = t * kSTile + static_cast<uint64_t>(u) * kThreads + threadIdx.x;
      uint32_t d = kBins;
      k[u] = 0;
      r[u] = 0;
      if (i < st.scan) {
        k[u] = key[i];
        r[u] = row[i];
        if (not_below(k[u], r[u], rk, rr)) d = digit_of(k[u], r[u], pass);
      }
      kb[u] = __ballot(d == bucket);
      mine += static_cast<uint32_t>(__popcll(kb[u]));
      if (collect && d < bucket) {  // fewer than kMaxTake records in the whole pass
        const uint32_t slot = atomicAdd(&ctl->wcount, 1u);
        if (slot < kMaxTake) {
          wkey[slot] = k[u];
          wrow[slot] = r[u];
        }
      }
    }
    // reserve the tile's slots: wave totals, one atomic, then every wave's base
    if (lane_id() == 0) s_wave[wave] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
      uint32_t tot = 0;
#pragma unroll
      for (int w = 0; w < kWaves; ++w) tot += s_wave[w];
      s_base = tot ? atomicAdd(&ctl->cursor[pass], tot) : 0;
    }
    __syncthreads();
    uint32_t at = s_base;
    for (uint32_t w = 0; w < wave; ++w) at += s_wave[w];
#pragma unroll
    for (int u = 0; u < kSRows; ++u) {
      if ((kb[u] >> lane_id()) & 1ull) {
        const uint32_t slot = at + rank_in(kb[u]);
        if (slot < st.scan) {  // a bucket is no larger than its source
          dst_key[slot] = k[u];
          dst_row[slot] = r[u];
        }
      }
      at += static_cast<uint32_t>(__popcll(kb[u]));
    }
    __syncthreads();  // s_wave / s_base are rewritten by the next tile
  }
}

struct SelBufs {
  const uint64_t* key[3];
  const uint32_t* row[3];
};
// pass p reads buffer 0 (the candidates) when p == 0, else 1 + (p - 1) % 2
__host__ __device__ inline int src_of(int pass) { return pass == 0 ? 0 : 1 + ((pass - 1) & 1); }

// One workgroup: the survivors that pass the filter and the winners into LDS,
// padded to a power of two with keys above every record, bitonic sort, then
// either the record of rank k as the next selection's filter (next != null) or
// the page.
constexpr int kSortThreads = 1024;
__global__ __launch_bounds__(kSortThreads) void k_sel_final(SelCtl* __restrict__ ctl, SelBufs b,
                                                            const uint64_t* __restrict__ wkey,
                                                            const uint32_t* __restrict__ wrow,
                                                            SelCtl* __restrict__ next,
                                                            uint32_t* __restrict__ page,
                                                            bool direct) {
  __shared__ uint64_t s_key[kSortCap];
  __shared__ uint32_t s_row[kSortCap];
  __shared__ uint32_t s_n;
  // direct: no pass ran, the candidates are the survivors
  const SelState st = ctl->state[direct ? 0 : kPasses];
  const uint32_t P = ctl->P;
  if (P == 0) return;
  const int src = direct ? 0 : src_of(st.fin ? static_cast<int>(st.fin) - 1 : kPasses);
  const uint64_t* key = b.key[src];
  const uint32_t* row = b.row[src];
  const uint32_t scan = st.scan < kFinal ? st.scan : kFinal;
  const uint32_t nw = ctl->wcount < kMaxTake ? ctl->wcount : kMaxTake;
  const uint64_t rk = ctl->r_key;
  const uint32_t rr = ctl->r_row;
  if (threadIdx.x == 0) s_n = 0;
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < scan + nw; i += kSortThreads) {
    const uint64_t k = i < scan ? key[i] : wkey[i - scan];
    const uint32_t r = i < scan ? row[i] : wrow[i - scan];
    if (not_below(k, r, rk, rr)) {
      const uint32_t slot = atomicAdd(&s_n, 1u);
      s_key[slot] = k;
      s_row[slot] = r;
    }
  }
  __syncthreads();
  const uint32_t cnt = s_n;
  uint32_t N = 64;
  while (N < cnt) N <<= 1;
  for (uint32_t i = cnt + threadIdx.x; i < N; i += kSortThreads) {
    s_key[i] = ~0ull;
    s_row[i] = 0xFFFFFFFFu;
  }
  __syncthreads();
  for (uint32_t k = 2; k <= N; k <<= 1) {
    for (uint32_t j = k >> 1; j > 0; j >>= 1) {
      for (uint32_t t = threadIdx.x; t < N / 2; t += kSortThreads) {
        const uint32_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
        const uint32_t l = i | j;
        const uint64_t ki = s_key[i], kl = s_key[l];
        const uint32_t ri = s_row[i], rl = s_row[l];
        const bool gt = ki > kl || (ki == kl && ri > rl);
        if (gt == ((i & k) == 0)) {
          s_key[i] = kl;
          s_row[i] = rl;
          s_key[l] = ki;
          s_row[l] = ri;
        }
      }
      __syncthreads();
    }
  }
  if (next) {
    if (threadIdx.x == 0 && st.k < cnt) {
      next->r_key = s_key[st.k];
      next->r_row = s_row[st.k];
    }
  } else {
    const uint32_t out = P < cnt ? P : cnt;
    for (uint32_t i = threadIdx.x; i < out; i += kSortThreads) page[i] = s_row[i];
  }
}

// The fixed worst-case sequence of one selection.
hipError_t select_launch(const SearchWs& w, int c, bool collect, bool passes, SelCtl* next,
                         uint32_t* page, hipStream_t s, KTimer* timer) {
  SelCtl* ctl = w.ctl + c;
  if (passes) {
    KScope k(timer, "search_passes", s);
    for (int p = 0; p < kPasses; ++p) {
      const int src = src_of(p), dst = src_of(p + 1);
      k_sel_hist<<<kSelBlocks, kThreads, 0, s>>>(ctl, p, w.key[src], w.row[src]);
      k_sel_compact<<<kSelBlocks, kThreads, 0, s>>>(ctl, p, collect, w.key[src], w.row[src],
                                                    w.key[dst], w.row[dst], w.wkey, w.wrow);
    }
  }
  SelBufs b;
  for (int i = 0; i < 3; ++i) {
    b.key[i] = w.key[i];
    b.row[i] = w.row[i];
  }
  // !passes: at most kFinal rows, the candidates go to the sort as they are
  {
    KScope k(timer, "search_sort", s);
    k_sel_final<<<1, kSortThreads, 0, s>>>(ctl, b, w.wkey, w.wrow, next, page, !passes);
  }
  return hipGetLastError();
}

}  // namespace

size_t search_workspace_bytes(uint64_t n, uint64_t m) { return search_ws(n, m, nullptr).bytes; }

hipError_t search_page_launch(const sdgpu_search_rows_t& rows, const sdgpu_search_objects_t* objects,
                              const sdgpu_search_query_t& q, uint32_t* page, uint32_t* counts,
                              void* ws, hipStream_t s, KTimer* timer) {
  hipError_t e = hipMemsetAsync(counts, 0, 4 * sizeof(uint32_t), s);
  if (e != hipSuccess || rows.n == 0) return e;
  SearchArgs a;
  a.r = rows;
  a.q = q;
  a.have_objects = objects != nullptr;
  if (objects) {
    a.o = *objects;
  } else {
    a.o = sdgpu_search_objects_t{};
  }
  const SearchWs w = search_ws(rows.n, a.o.m, ws);
  const bool tags = (q.use & SDGPU_SEARCH_USE_TAGS) != 0;
  if (tags && a.o.m) {
    e = hipMemsetAsync(w.mark, 0, a.o.m, s);
    if (e != hipSuccess) return e;
    if (a.o.n_pairs) {
      KScope k(timer, "search_tags", s);
      TagSet set;
      set.n = q.n_tags;
      for (uint32_t j = 0; j < 32; ++j) set.tag[j] = j < q.n_tags ? q.tags[j] : 0;
      k_search_tags<<<grid_for(a.o.n_pairs, kThreads, 2048), kThreads, 0, s>>>(
          a.o.tag_obj, a.o.tag_tag, a.o.n_pairs, a.o.m, set, w.mark);
    }
  }
  {
    KScope k(timer, "search_filter", s);
    k_search_filter<<<grid_for(rows.n, kFTile, 2048), kThreads, 0, s>>>(a, w.mark, w.key[0],
                                                                       w.row[0], counts);
  }
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (q.take == 0) return hipSuccess;  // the count call: counts[2] stays 0
  // hist, cursor and wcount of both selections
  e = hipMemsetAsync(w.ctl, 0, 2 * sizeof(SelCtl), s);
  if (e != hipSuccess) return e;
  k_sel_begin<<<1, 64, 0, s>>>(counts, q.offset, q.take, w.ctl);
  const bool passes = rows.n > kFinal;
  if (q.offset > 0) {
    e = select_launch(w, 0, false, passes, w.ctl + 1, nullptr, s, timer);
    if (e != hipSuccess) return e;
  }
  return select_launch(w, 1, true, passes, nullptr, page, s, timer);
}

}  // namespace sdgpu
