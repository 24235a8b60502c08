// Stable compaction of flagged positions in tiles of 4096: the device half
// every list-producing feature shares.
//
// A workgroup of kThreads takes a tile of kRows x kThreads positions: thread t
// holds position tile + k * kThreads + t for row step k (coalesced loads), as
// bit k of a flag word.  (k, t) order is position order, so ranks made of
//   the listed lanes before this one in its wave (a ballot per row step),
//   the listed positions of earlier (row step, wave) pairs (one wave scans
//   the kRows x kWaves = 64 counts), and
//   the tile's offset (an exclusive scan of the tile counts, scan_device.hpp)
// keep a list in position order.  A caller runs two kernels around that scan:
// one that stores tile_count's totals, one that calls tile_offsets and stores
// its own payload at off[k][w] + pre[k].  The predicate, the payload and the
// way several lists share one scan stay with the caller; N flag words are N
// lists over the same positions, ranked together (link.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sdgpu {
namespace compact {

constexpr int kThreads = 256;
constexpr int kRows = 16;  // row steps: positions per thread
constexpr int kWaves = kThreads / 64;
constexpr uint32_t kTile = kThreads * kRows;
static_assert(kRows * kWaves == 64, "one wave scans the (row step, wave) counts");

inline uint64_t tiles_for(uint64_t n) { return (n + kTile - 1) / kTile; }

// Sum over the 64 lanes of a wave, in every lane; N values side by side.
template <int N>
__device__ __forceinline__ void wave_sum(uint32_t (&v)[N]) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1)
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] += __shfl_xor(v[i], d);
}
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
  uint32_t a[1] = {v};
  wave_sum(a);
  return a[0];
}

// Inclusive prefix sum over the 64 lanes of a wave; N values side by side.
template <int N>
__device__ __forceinline__ void wave_scan(uint32_t (&v)[N]) {
  const uint32_t lane = __lane_id();
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    uint32_t x[N];
#pragma unroll
    for (int i = 0; i < N; ++i) x[i] = __shfl_up(v[i], d);
    if (lane >= static_cast<uint32_t>(d)) {
#pragma unroll
      for (int i = 0; i < N; ++i) v[i] += x[i];
    }
  }
}
__device__ __forceinline__ uint32_t wave_scan(uint32_t v) {
  uint32_t a[1] = {v};
  wave_scan(a);
  return a[0];
}

// total[i] = set bits of f[i] over the workgroup, in thread 0 (0 elsewhere).
// Every thread calls it; one barrier.
template <int N>
__device__ __forceinline__ void tile_count(const uint32_t (&f)[N], uint32_t (&total)[N]) {
  __shared__ uint32_t sw[kWaves][N];
  uint32_t c[N];
#pragma unroll
  for (int i = 0; i < N; ++i) c[i] = __popc(f[i]);
  wave_sum(c);
  if (__lane_id() == 0) {
#pragma unroll
    for (int i = 0; i < N; ++i) sw[threadIdx.x >> 6][i] = c[i];
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < N; ++i) total[i] = 0;
  if (threadIdx.x == 0) {
    for (int w = 0; w < kWaves; ++w) {
#pragma unroll
      for (int i = 0; i < N; ++i) total[i] += sw[w][i];
    }
  }
}
__device__ __forceinline__ uint32_t tile_count(uint32_t f) {
  const uint32_t a[1] = {f};
  uint32_t total[1];
  tile_count(a, total);
  return total[0];
}

// Bit k of f[i]: this thread's position of row step k is on list i.  base(i):
// where the tile's part of list i starts; a callable, so that only the
// scanning wave reads it, between the barriers.  Afterwards (two barriers; every
// thread calls it) the position of row step k goes to
// off[i][k][threadIdx.x >> 6] + pre[i][k].  off and pre: the caller's
// uint32_t off[N][kRows][kWaves] (LDS) and pre[N][kRows].
template <int N, class Base>
__device__ __forceinline__ void tile_offsets(const uint32_t (&f)[N], Base base,
                                             uint32_t (*off)[kRows][kWaves],
                                             uint32_t (*pre)[kRows]) {
  const uint32_t lane = __lane_id(), w = threadIdx.x >> 6;
  const uint64_t lt = (1ull << lane) - 1ull;
#pragma unroll
  for (int k = 0; k < kRows; ++k) {
#pragma unroll
    for (int i = 0; i < N; ++i) {
      const uint64_t b = __ballot(f[i] >> k & 1u);
      pre[i][k] = __popcll(b & lt);
      if (lane == 0) off[i][k][w] = __popcll(b);
    }
  }
  __syncthreads();
  if (threadIdx.x < 64) {  // (k, wave) order -- k-major, the array's order -- is position order
    uint32_t a[N], inc[N];
#pragma unroll
    for (int i = 0; i < N; ++i) inc[i] = a[i] = (&off[i][0][0])[lane];
    wave_scan(inc);
#pragma unroll
    for (int i = 0; i < N; ++i) (&off[i][0][0])[lane] = base(i) + inc[i] - a[i];
  }
  __syncthreads();
}
template <class Base>  // one list: base()
__device__ __forceinline__ void tile_offsets(uint32_t f, Base base, uint32_t (&off)[kRows][kWaves],
                                             uint32_t (&pre)[kRows]) {
  const uint32_t a[1] = {f};
  tile_offsets(a, [&](int) { return base(); }, &off, &pre);
}

}  // namespace compact
}  // namespace sdgpu
