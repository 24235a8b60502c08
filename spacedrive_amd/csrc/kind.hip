// Object kind of every cas message of a batch (k_kind) and the host-only kind
// calls of the C ABI.  The table and the decision are kind_table.hpp's; this
// unit only brings a message's first bytes to them.
#include <errno.h>
#include <fcntl.h>
#include <string.h>
#include <unistd.h>

#include <algorithm>

#include <hip/hip_runtime.h>

#include "../../include/sdgpu.h"
#include "internal.hpp"
#include "kind_table.hpp"

namespace sdgpu {

namespace {

constexpr uint32_t kKindThreads = 256;
// Enough blocks to fill the device; each copies the table into LDS once and
// then strides over the messages.
constexpr uint32_t kKindMaxBlocks = 1024;

// The device's copy of the table (constant-initialised from the same
// constexpr builder as the host's kind::kTable).
__device__ const kind::Table d_kind_table = kind::make_table();

// The (up to) 4 bytes at p[0 .. rem) as a little-endian word, rem in [0, 4):
// byte loads, so nothing at or past p + rem is touched.
__device__ __forceinline__ uint32_t load_tail(const uint8_t* p, uint32_t rem) {
  uint32_t w = 0;
  if (rem > 0) w |= static_cast<uint32_t>(p[0]);
  if (rem > 1) w |= static_cast<uint32_t>(p[1]) << 8;
  if (rem > 2) w |= static_cast<uint32_t>(p[2]) << 16;
  return w;
}

// One lane per message.  Message i is arena[off .. off + len): the 8-byte size
// prefix, then the file's first bytes (the whole file, or the 8192-byte header
// of a sampled one).  The lane reads message bytes [0, min(len, 48)): 16-byte
// loads for the quarters that lie wholly inside the message, 4-byte and byte
// loads for the last partial one -- never a byte at or beyond off + len.  The
// signatures sit in LDS: lanes of a wave hold different extension ids, so the
// table index is divergent.
__global__ __launch_bounds__(kKindThreads) void k_kind(const uint8_t* __restrict__ arena,
                                                        uint64_t arena_bytes,
                                                        const uint64_t* __restrict__ off,
                                                        const uint32_t* __restrict__ len,
                                                        const uint16_t* __restrict__ ext, uint32_t n,
                                                        uint32_t max_len, uint32_t flags,
                                                        uint8_t* __restrict__ out) {
  __shared__ kind::Table T;
  {
    static_assert(sizeof(kind::Table) % 4 == 0, "table copied as words");
    const uint32_t* src = reinterpret_cast<const uint32_t*>(&d_kind_table);
    uint32_t* dst = reinterpret_cast<uint32_t*>(&T);
    for (uint32_t k = threadIdx.x; k < sizeof(kind::Table) / 4; k += kKindThreads) dst[k] = src[k];
  }
  __syncthreads();
  for (uint32_t i = blockIdx.x * kKindThreads + threadIdx.x; i < n; i += gridDim.x * kKindThreads) {
    const uint64_t o = off[i];
    const uint32_t l = len[i];
    const uint32_t e = ext[i];
    // sdgpu_cas_batch_device's validity rule (b3_batch.hip msg_ok)
    const bool ok = l <= max_len && (o & 15u) == 0 && o <= arena_bytes && l <= arena_bytes - o;
    uint8_t k = kind::kUnknown;
    if (ok && e != 0) {
      const uint32_t avail = l < 48u ? l : 48u;
      const uint8_t* p = arena + o;
      uint32_t w[12];
#pragma unroll
      for (uint32_t q = 0; q < 3; ++q) {
        if (avail >= 16 * q + 16) {
          const uint4 v = *reinterpret_cast<const uint4*>(p + 16 * q);
          w[4 * q] = v.x;
          w[4 * q + 1] = v.y;
          w[4 * q + 2] = v.z;
          w[4 * q + 3] = v.w;
        } else {
          const uint32_t rem = avail > 16 * q ? avail - 16 * q : 0;
#pragma unroll
          for (uint32_t j = 0; j < 4; ++j) {
            if (rem >= 4 * j + 4) w[4 * q + j] = *reinterpret_cast<const uint32_t*>(p + 16 * q + 4 * j);
            else if (rem > 4 * j) w[4 * q + j] = load_tail(p + 16 * q + 4 * j, rem - 4 * j);
            else w[4 * q + j] = 0;
          }
        }
      }
      // a message shorter than its prefix has zero body bytes
      const uint32_t L = avail >= 8 ? avail - 8 : 0;
      static_assert(kind::kWords == 10, "body = message words [2, 12)");
      k = kind::kind_decide(T, e, w + 2, L, flags);
    }
    out[i] = k;
  }
}

}  // namespace

hipError_t kind_launch(const uint8_t* arena, uint64_t arena_bytes, const uint64_t* off,
                       const uint32_t* len, const uint16_t* ext, uint32_t n, uint32_t max_len,
                       uint32_t flags, uint8_t* out, hipStream_t s, KTimer* timer) {
  if (n == 0) return hipSuccess;
  KScope scope(timer, "kind", s);
  const uint32_t blocks = std::min<uint32_t>((n + kKindThreads - 1) / kKindThreads, kKindMaxBlocks);
  k_kind<<<blocks, kKindThreads, 0, s>>>(arena, arena_bytes, off, len, ext, n, max_len, flags, out);
  return hipGetLastError();
}

}  // namespace sdgpu

// ---- host-only entry points (no context, no device) ---------------------------

extern "C" {

int sdgpu_kind_ext_ids(const char* const* paths, uint32_t n, uint16_t* ext_id_out) {
  if (n && (!paths || !ext_id_out)) return -EINVAL;
  for (uint32_t i = 0; i < n; ++i) ext_id_out[i] = sdgpu::kind::ext_id_of_path(paths[i]);
  return 0;
}

int sdgpu_kind_ext_name(uint32_t ext_id, char out[16], int32_t kinds[2]) {
  if (!out || !kinds) return -EINVAL;
  if (ext_id == 0 || ext_id > sdgpu::kind::kExts) return -ENOENT;
  const sdgpu::kind::Src& s = sdgpu::kind::kSrc[ext_id - 1];
  memset(out, 0, 16);
  strncpy(out, s.name, 15);
  kinds[0] = s.kind;
  kinds[1] = s.kind2;
  return 0;
}

int sdgpu_kind_of_file(const char* path, uint32_t flags, int32_t* kind) {
  if (!path || !kind || (flags & ~SDGPU_KIND_VERIFY_MAGIC)) return -EINVAL;
  *kind = 0;
  const uint16_t ext = sdgpu::kind::ext_id_of_path(path);
  if (ext == 0) return 0;  // no Extension: the file is not opened (magic.rs:180-186)
  const int fd = open(path, O_RDONLY | O_CLOEXEC);
  if (fd < 0) return 0;  // magic.rs:188-190
  uint8_t buf[sdgpu::kind::kBodyBytes];
  size_t got = 0;
  if (sdgpu::kind::kind_reads_bytes(ext, flags)) {
    // only now are bytes read, and only the ones a signature can reach
    while (got < sizeof(buf)) {
      const ssize_t r = pread(fd, buf + got, sizeof(buf) - got, static_cast<off_t>(got));
      if (r < 0 && errno == EINTR) continue;
      if (r <= 0) break;  // a read error ends the walk like a short file (magic.rs:165)
      got += static_cast<size_t>(r);
    }
  }
  close(fd);
  *kind = sdgpu::kind::kind_of_bytes(ext, buf, got, flags);
  return 0;
}

}  // extern "C"
