// The 512-point fp64 transform of DESIGN.md 33.1 as device functions, the one copy every kernel that transforms uses:
// stoi_bands_kernel (csrc/metrics.hip), ns_power_kernel and ns_synth_kernel (csrc/denoise.hip), aec_kernel (csrc/aec.hip).  A
// radix-2 decimation in frequency, and the same flow graph run backwards (decimation in time from bit-reversed input,
// conjugated twiddles).  One wave transforms one 512-entry double2 buffer in LDS in place; bin k of the forward transform ends
// at the bit-reversed index fft512_rev(k), and the inverse starts from that order, so no reordering pass lies between the two.
// The twiddles come from a 256-entry table the workgroup computes once with sincospi and publishes with a workgroup barrier.
//
// A buffer belongs to one wave, so the stages of a whole transform are ordered by fft512_wave_sync(), not by a workgroup
// barrier: the 64 lanes run in lockstep, LDS operations of one wave retire in order, and the fence keeps the compiler from
// moving the next stage's reads over this stage's writes.  The other waves of the workgroup are free to do something else.
#pragma once
#include <hip/hip_runtime.h>

namespace fac {

constexpr int FFT512_N = 512;

// tw[j] = exp(-2 pi i j / 512), j = tid < 256
__device__ __forceinline__ void fft512_table(double2* tw, int tid) {
  double s, c;
  sincospi((double)tid / (double)(FFT512_N / 2), &s, &c);
  tw[tid] = make_double2(c, -s);
}

__device__ __forceinline__ int fft512_rev(int k) { return (int)(__brev((unsigned)k) >> 23); }   // 9-bit reversal

__device__ __forceinline__ void fft512_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// one stage of the forward transform: (u, v) <- (u + v, (u - v) t).  A lane's four butterflies touch eight different entries:
// all are read before any is written, so that the reads are in flight together.
__device__ __forceinline__ void fft512_dif(double2* z, const double2* tw, int lane, int half) {
  const int step = (FFT512_N / 2) / half;
  int lo[4];
  double2 u[4], v[4], t[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = lane + 64 * r;
    const int pos = i & (half - 1);
    lo[r] = ((i - pos) << 1) + pos;
    u[r] = z[lo[r]], v[r] = z[lo[r] + half], t[r] = tw[pos * step];
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const double dx = u[r].x - v[r].x, dy = u[r].y - v[r].y;
    z[lo[r]] = make_double2(u[r].x + v[r].x, u[r].y + v[r].y);
    z[lo[r] + half] = make_double2(dx * t[r].x - dy * t[r].y, dx * t[r].y + dy * t[r].x);
  }
}

// one stage of the inverse: q = v * conj(t), (u, v) <- (u + q, u - q)
__device__ __forceinline__ void fft512_dit(double2* z, const double2* tw, int lane, int half) {
  const int step = (FFT512_N / 2) / half;
  int lo[4];
  double2 u[4], v[4], t[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = lane + 64 * r;
    const int pos = i & (half - 1);
    lo[r] = ((i - pos) << 1) + pos;
    u[r] = z[lo[r]], v[r] = z[lo[r] + half], t[r] = tw[pos * step];
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const double qx = v[r].x * t[r].x + v[r].y * t[r].y, qy = v[r].y * t[r].x - v[r].x * t[r].y;
    z[lo[r]] = make_double2(u[r].x + qx, u[r].y + qy);
    z[lo[r] + half] = make_double2(u[r].x - qx, u[r].y - qy);
  }
}

// z (natural order, written by this wave or ordered against its writer by the caller) -> the spectrum, bin k at fft512_rev(k).
// Returns with the result visible to the wave.
__device__ __forceinline__ void fft512_forward(double2* z, const double2* tw, int lane) {
  fft512_wave_sync();
#pragma unroll
  for (int half = FFT512_N / 2; half >= 1; half >>= 1) {
    fft512_dif(z, tw, lane, half);
    fft512_wave_sync();
  }
}

// the spectrum, bin k at fft512_rev(k) -> 512 times the signal, natural order: the caller scales by 1 / 512
__device__ __forceinline__ void fft512_inverse(double2* z, const double2* tw, int lane) {
  fft512_wave_sync();
#pragma unroll
  for (int half = 1; half <= FFT512_N / 2; half <<= 1) {
    fft512_dit(z, tw, lane, half);
    fft512_wave_sync();
  }
}

}  // namespace fac
