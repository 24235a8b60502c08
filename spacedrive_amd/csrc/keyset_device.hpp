// A set of 64-bit keys as an open-addressing table of 8-byte slots (DESIGN.md
// §4.12): the slot holds the key itself, an empty slot ~0; probing is linear
// from row_hash(key); capacity is a power of two >= 2 x the keys, so an empty
// slot ends every walk.  The key ~0 cannot sit in a slot: it owns slot number
// `cap`, one past the table, and every caller handles it before calling here.
// What hangs off a slot number (first_row, hit bytes, slot_of) is the
// caller's.  The tables of sync.hip (32-byte slots) and index.hip (packed
// slots) are their own.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rows_device.hpp"

namespace sdgpu {

constexpr uint64_t kEmptyKey = ~0ull;

inline uint64_t keyset_cap(uint64_t n) {
  uint64_t cap = 1024;
  // 2^31 slots at the most: a slot number, the special one included, is a u32
  while (cap < 2 * n && cap < (1ull << 31)) cap <<= 1;
  return cap;
}

// The slot key k (not ~0) ends in: the first thread to claim an empty slot
// (64-bit CAS) places the key, every other copy of it finds it.
__device__ __forceinline__ uint64_t keyset_insert(uint64_t* __restrict__ table, uint64_t cap,
                                                  uint64_t k) {
  uint64_t h = row_hash(k) & (cap - 1);
  for (;;) {
    const unsigned long long prev =
        atomicCAS(reinterpret_cast<unsigned long long*>(&table[h]),
                  static_cast<unsigned long long>(kEmptyKey), static_cast<unsigned long long>(k));
    if (prev == kEmptyKey || prev == k) return h;
    h = (h + 1) & (cap - 1);
  }
}

// The slot of key k (not ~0) in a table whose first probed slot h =
// row_hash(k) & (cap - 1) holds `sk` (loaded by the caller, with its other
// loads), or ~0 when the table does not hold k.
__device__ __forceinline__ uint64_t keyset_find(const uint64_t* __restrict__ table, uint64_t cap,
                                                uint64_t k, uint64_t h, uint64_t sk) {
  for (;;) {
    if (sk == k) return h;
    if (sk == kEmptyKey) return ~0ull;
    h = (h + 1) & (cap - 1);
    sk = table[h];
  }
}

}  // namespace sdgpu
