// One row of a carried stream as the streaming front-end kernels read it (csrc/denoise.hip, csrc/aec.hip): sample n, absolute,
// of [carry | block], where the block's first sample has the index n0 and the carry holds the cn samples in front of it.  A
// sample before the row's start, at or behind its end, or in front of the carry reads as 0.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fac {

struct StreamSrc {
  const float* carry;       // the row's cn samples in front of the block, or nullptr
  const float* x;           // the row's block
  int cn;
  long long n0, start, end;
  __device__ __forceinline__ float sample(long long n) const {
    if (n < start || n >= end) return 0.f;
    long long r = n - n0;
    if (r >= 0) return x[r];
    r += cn;
    return carry && r >= 0 ? carry[r] : 0.f;
  }
};

// Another signal of the same row and call (the far end next to the microphone): s with that signal's carry and block, the
// same n0, start and end.
__device__ __forceinline__ StreamSrc stream_src_like(StreamSrc s, const float* carry_in, int cn, const float* x, long long x_bs, int b) {
  s.carry = carry_in ? carry_in + (long long)b * cn : nullptr;
  s.x = x ? x + (long long)b * x_bs : nullptr;
  s.cn = cn;
  return s;
}

// Row b of a call: carry_in (B, cn) or nullptr, x (B, k) at a row pitch of x_bs; lens[b] clamped to 0 .. k replaces k, starts[b]
// clamped at 0 is the row's first sample.
__device__ __forceinline__ StreamSrc stream_src(const float* carry_in, int cn, const float* x, long long x_bs, const int32_t* lens,
                                                const int64_t* starts, long long n0, int k, int b) {
  StreamSrc s;
  int kb = k;
  if (lens) {
    const int len = lens[b];
    kb = len < 0 ? 0 : (len < k ? len : k);
  }
  s.n0 = n0, s.end = n0 + kb;
  s.start = starts ? (starts[b] > 0 ? starts[b] : 0) : 0;
  return stream_src_like(s, carry_in, cn, x, x_bs, b);
}

// The row's next carry: the last cn samples of [carry | block of k samples], by the n_threads threads of a workgroup.
__device__ __forceinline__ void stream_carry_out(const StreamSrc& s, float* carry_out, int k, int b, int tid, int n_threads) {
  float* out = carry_out + (long long)b * s.cn;
  for (int t = tid; t < s.cn; t += n_threads) out[t] = s.sample(s.n0 + k - s.cn + t);
}

}  // namespace fac
