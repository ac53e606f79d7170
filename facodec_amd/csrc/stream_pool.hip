// Slots of a running streaming session: fac_slot_copy re-initialises slots from a donor slot between two hops,
// fac_rows_pick scatters the live streams' hops into the session's input and gathers their rows of its outputs.  Layouts and
// contracts: the header comment of include/facodec_hip.h.  Both are bandwidth kernels: no LDS, no matrix pipe, no atomics.
#include "common.h"

namespace fac {

struct SlotDsts {
  int d[FAC_SLOT_MAX_DST];
};

__device__ __forceinline__ long long slot_offset(const fac_slot_seg& s, int b) {
  return (long long)(b >> 5) * s.slot_hi + (long long)(b & 31) * s.slot_lo;
}

// One workgroup = one tile (<= FAC_SLOT_TILE elements of one segment's per-slot range) for one destination.  256 lanes x 4 float4:
// the four loads of a lane are issued before its four stores, consecutive lanes take consecutive 16 bytes.
__global__ __launch_bounds__(256) void slot_copy_kernel(const fac_slot_seg* __restrict__ segs, const int2* __restrict__ tiles,
                                                        int src, SlotDsts dsts) {
  const int2 tile = tiles[blockIdx.x];
  const fac_slot_seg s = segs[tile.x];
  const int dst = dsts.d[blockIdx.y];
  const float* sp = s.base + slot_offset(s, src);
  float* dp = s.base + slot_offset(s, dst);
  const int e0 = tile.y;
  const int e1 = min(e0 + FAC_SLOT_TILE, s.elems);
  const int tid = threadIdx.x;
  const bool vec = (s.row_len & 3) == 0 && (s.rows == 1 || (s.row_stride & 3) == 0) &&
                   ((((uintptr_t)sp) | ((uintptr_t)dp)) & 15) == 0;
  if (vec) {
    float4 v[4];
    long long o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int e = e0 + 4 * (tid + 256 * j);       // row_len % 4 == 0: the 4 elements lie in one run, and e < e1 => e + 3 < e1
      o[j] = -1;
      if (e < e1) {
        const int row = s.rows == 1 ? 0 : e / s.row_len;
        o[j] = (long long)row * s.row_stride + (e - row * s.row_len);
        v[j] = *reinterpret_cast<const float4*>(sp + o[j]);
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (o[j] >= 0) *reinterpret_cast<float4*>(dp + o[j]) = v[j];
    return;
  }
  for (int eb = e0; eb < e1; eb += 1024) {
    float v[4];
    long long o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int e = eb + tid + 256 * j;
      o[j] = -1;
      if (e < e1) {
        const int row = s.rows == 1 ? 0 : e / s.row_len;
        o[j] = (long long)row * s.row_stride + (e - row * s.row_len);
        v[j] = sp[o[j]];
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (o[j] >= 0) dp[o[j]] = v[j];
  }
}

// grid (ceil(row_words / 1024), n_dst): 256 lanes x 4 words (one 16-byte access when VEC) of one destination row.
template <bool VEC>
__global__ __launch_bounds__(256) void rows_pick_kernel(const uint32_t* __restrict__ src, long long src_stride,
                                                        uint32_t* __restrict__ dst, const int* __restrict__ map, int n_src,
                                                        int row_words) {
  const int r = blockIdx.y;
  const int m = map[r];
  const bool have = m >= 0 && m < n_src;
  const uint32_t* sp = src + (have ? (long long)m * src_stride : 0);
  uint32_t* dp = dst + (long long)r * row_words;
  if constexpr (VEC) {
    const int w = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (w >= row_words) return;
    u32x4 v = {0u, 0u, 0u, 0u};
    if (have) v = *reinterpret_cast<const u32x4*>(sp + w);
    *reinterpret_cast<u32x4*>(dp + w) = v;
  } else {
    const int w0 = blockIdx.x * 1024 + threadIdx.x;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int w = w0 + 256 * j;
      if (w < row_words) dp[w] = have ? sp[w] : 0u;
    }
  }
}

}  // namespace fac

using namespace fac;

extern "C" int fac_slot_copy(const fac_slot_seg* segs, int n_seg, const int32_t* tiles, int n_tiles, int B, int src,
                             const int32_t* dst, int n_dst, fac_stream_t stream) {
  FAC_REQUIRE(segs && tiles, "slot_copy: null table (segs=%p tiles=%p)", (const void*)segs, (const void*)tiles);
  FAC_REQUIRE(n_seg > 0 && n_tiles > 0 && B > 0, "slot_copy: bad arguments (n_seg=%d n_tiles=%d B=%d)", n_seg, n_tiles, B);
  FAC_REQUIRE(dst && n_dst >= 1 && n_dst <= FAC_SLOT_MAX_DST, "slot_copy: %d destinations (1 .. %d per launch)", n_dst,
              FAC_SLOT_MAX_DST);
  FAC_REQUIRE(src >= 0 && src < B, "slot_copy: source slot %d outside [0, %d)", src, B);
  SlotDsts d;
  for (int i = 0; i < FAC_SLOT_MAX_DST; ++i) d.d[i] = 0;
  for (int i = 0; i < n_dst; ++i) {
    FAC_REQUIRE(dst[i] >= 0 && dst[i] < B, "slot_copy: destination slot %d outside [0, %d)", dst[i], B);
    FAC_REQUIRE(dst[i] != src, "slot_copy: slot %d is both source and destination", src);
    for (int j = 0; j < i; ++j) FAC_REQUIRE(dst[j] != dst[i], "slot_copy: duplicate destination slot %d", dst[i]);
    d.d[i] = dst[i];
  }
  hipLaunchKernelGGL(slot_copy_kernel, dim3((unsigned)n_tiles, (unsigned)n_dst), dim3(256), 0, (hipStream_t)stream, segs,
                     reinterpret_cast<const int2*>(tiles), src, d);
  return check_launch("slot_copy");
}

extern "C" int fac_rows_pick(const void* src, int64_t src_stride, void* dst, const int32_t* map, int n_dst, int n_src,
                             int row_words, fac_stream_t stream) {
  FAC_REQUIRE(src && dst && map, "rows_pick: null pointer");
  FAC_REQUIRE(n_dst > 0 && n_dst <= 65535 && n_src > 0 && row_words > 0 && src_stride >= row_words,
              "rows_pick: bad arguments (n_dst=%d n_src=%d row_words=%d src_stride=%lld)", n_dst, n_src, row_words,
              (long long)src_stride);
  const bool vec = (row_words & 3) == 0 && (src_stride & 3) == 0 && ((((uintptr_t)src) | ((uintptr_t)dst)) & 15) == 0;
  const dim3 grid((unsigned)((row_words + 1023) / 1024), (unsigned)n_dst);
  if (vec) {
    hipLaunchKernelGGL(rows_pick_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, (const uint32_t*)src,
                       (long long)src_stride, (uint32_t*)dst, map, n_src, row_words);
  } else {
    hipLaunchKernelGGL(rows_pick_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, (const uint32_t*)src,
                       (long long)src_stride, (uint32_t*)dst, map, n_src, row_words);
  }
  return check_launch("rows_pick");
}
