// Shared helpers for the libfacodec_hip.so translation units (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>
#include "../../include/facodec_hip.h"

namespace fac {

void set_error(const char* fmt, ...);

inline int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("%s: launch failed: %s", what, hipGetErrorString(e));
    return FAC_ERR_LAUNCH;
  }
  return FAC_OK;
}

#define FAC_REQUIRE(cond, ...)          \
  do {                                  \
    if (!(cond)) {                      \
      ::fac::set_error(__VA_ARGS__);    \
      return FAC_ERR_ARG;               \
    }                                   \
  } while (0)

// Device-side twin of fac_cin_pad (include/facodec_hip.h): packed weights have zero rows up to a
// multiple of 48 input channels.
__host__ __device__ constexpr int cin_pad_dev(int c) { return ((c + 47) / 48) * 48; }

// sin(y)^2 to ~1 ulp of sin: Cody-Waite reduction by pi/2 (3 constants, exact products via fma for
// |k| < 2^13) + the Cephes single-precision minimax polynomials on [-pi/4, pi/4]; the quadrant only
// decides WHICH polynomial is squared (sign drops out).  Arguments beyond +-4096 take libm's sinf.
// The rare paths are kept OUT of line on purpose: libm's sinf / tanhf / log1pf bodies are hundreds of
// instructions each, and inlining them at every Snake site made the staging loop of the conv kernel
// overflow the instruction cache (staging then ran at ~20k cycles per chunk -- profiles/ ablation).
// sin_sq2 / snake_apply2 below are the same operations on two values at once (v_pk_fma/mul/add_f32, bit-equal per component): used by
// the all-waves epilogue of conv1d_bsplit_kernel.h, where no MFMA runs on the CU; beside MFMAs packed f32 costs more than the scalar
// pair it replaces, and the other Snake sites measured no gain or a loss with it, so they keep the scalar form.
__device__ __attribute__((noinline)) float sin_sq_slow(float y) {
  const float s = sinf(y);
  return __fmul_rn(s, s);
}

__device__ __forceinline__ float sin_sq(float y) {
  if (__builtin_expect(fabsf(y) > 4096.0f, 0)) return sin_sq_slow(y);
  const float k = rintf(y * 0.63661977236758134308f);
  float r = fmaf(k, -1.5703125f, y);
  r = fmaf(k, -4.837512969970703125e-4f, r);
  r = fmaf(k, -7.54978995489188216e-8f, r);
  const float z = r * r;
  float ps = fmaf(z, -1.9515295891e-4f, 8.3321608736e-3f);
  ps = fmaf(ps, z, -1.6666654611e-1f);
  const float sn = fmaf(ps * z, r, r);
  float pc = fmaf(z, 2.443315711809948e-5f, -1.388731625493765e-3f);
  pc = fmaf(pc, z, 4.166664568298827e-2f);
  const float cs = fmaf(pc * z, z, fmaf(z, -0.5f, 1.0f));
  const float v = (((int)k) & 1) ? cs : sn;
  return __fmul_rn(v, v);
}

// Snake activation, dac/nn/layers.py:18-24:  x + (alpha + 1e-9)^-1 * sin(alpha*x)^2.
// inv = 1/(alpha+1e-9) is computed with a true division; the multiply and the add stay separate
// roundings (no fma contraction) like the reference expression.
__device__ __forceinline__ float snake_inv(float alpha) { return __fdiv_rn(1.0f, __fadd_rn(alpha, 1e-9f)); }
__device__ __forceinline__ float snake_apply(float x, float alpha, float inv) {
  return __fadd_rn(x, __fmul_rn(inv, sin_sq(__fmul_rn(alpha, x))));
}

// Two values per instruction: operation for operation the scalar functions above (fma -> llvm.fma.v2f32, * and + stay separate
// roundings under -ffp-contract=off); rint, the |y| > 4096 test and the parity select work per component, and sin_sq_slow is called,
// out of line, for exactly the components beyond 4096.
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef int i32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f32x2 sin_sq2(f32x2 y) {
  const f32x2 k = __builtin_elementwise_rint(y * 0.63661977236758134308f);
  f32x2 r = __builtin_elementwise_fma(k, (f32x2)(-1.5703125f), y);
  r = __builtin_elementwise_fma(k, (f32x2)(-4.837512969970703125e-4f), r);
  r = __builtin_elementwise_fma(k, (f32x2)(-7.54978995489188216e-8f), r);
  const f32x2 z = r * r;
  f32x2 ps = __builtin_elementwise_fma(z, (f32x2)(-1.9515295891e-4f), (f32x2)(8.3321608736e-3f));
  ps = __builtin_elementwise_fma(ps, z, (f32x2)(-1.6666654611e-1f));
  const f32x2 sn = __builtin_elementwise_fma(ps * z, r, r);
  f32x2 pc = __builtin_elementwise_fma(z, (f32x2)(2.443315711809948e-5f), (f32x2)(-1.388731625493765e-3f));
  pc = __builtin_elementwise_fma(pc, z, (f32x2)(4.166664568298827e-2f));
  const f32x2 cs = __builtin_elementwise_fma(pc * z, z, __builtin_elementwise_fma(z, (f32x2)(-0.5f), (f32x2)(1.0f)));
  const i32x2 ki = __builtin_convertvector(k, i32x2);
  f32x2 v;
  v.x = (ki.x & 1) ? cs.x : sn.x;
  v.y = (ki.y & 1) ? cs.y : sn.y;
  v = v * v;
  const bool bx = fabsf(y.x) > 4096.0f, by = fabsf(y.y) > 4096.0f;
  if (__builtin_expect(bx || by, 0)) {
    if (bx) v.x = sin_sq_slow(y.x);
    if (by) v.y = sin_sq_slow(y.y);
  }
  return v;
}
__device__ __forceinline__ f32x2 snake_apply2(f32x2 x, float alpha, float inv) { return x + inv * sin_sq2(alpha * x); }

// Epilogue activations other than Snake (cold: once per output element of a few small layers).
__device__ __attribute__((noinline)) float apply_act_slow(float v, int act) {
  if (act == FAC_ACT_TANH) return tanhf(v);
  if (act == FAC_ACT_MISH) {
    // x * tanh(softplus(x)); softplus with torch's threshold 20 (modules/style_encoder.py:6-10)
    const float sp = v > 20.f ? v : log1pf(expf(v));
    return v * tanhf(sp);
  }
  if (act == FAC_ACT_LOG_MEL) return (logf(1e-5f + v) + 4.0f) / 4.0f;   // modules/quantize.py:241
  return v;
}

__device__ __forceinline__ float sigmoid_f(float x) { return __fdiv_rn(1.0f, 1.0f + expf(-x)); }

// Index into x (length T) of position `t` of the reflect-padded signal, or -1 where the value
// is zero.  Text = max(T, max_pad+1) is the length of pad1d's temporary zero extension
// (dac/model/encodec.py:96-113): for T > pad it is plain reflection (-j -> j, T-1+j -> T-1-j).
__device__ __forceinline__ int reflect_index(int t, int T, int Text) {
  int j;
  if (t < 0) j = -t;
  else if (t < Text) j = t;
  else j = 2 * (Text - 1) - t;
  return (j >= 0 && j < T) ? j : -1;
}

// ---- primitives shared by the split-bf16 kernels (conv1d_bsplit* / gemm_split / pw_split / wgrad_split, lstm_persist, the P8 pre-pass)

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// x = h + m + l up to the rounding of the last residual: three round-to-nearest-even bf16 planes, each the bf16 of what the planes
// before it left over (both subtractions are exact).  "bf16 pipe, fp32-grade" and the bit-exact gates rest on this one function:
// the weight packers, the staging waves, the weight-gradient plane kernels, the LSTM resident kernel and the P8 pre-pass all
// call it, so an operand split ahead of time and one split inside a kernel are the same bits.
__device__ __forceinline__ void split3(float x, __bf16& h, __bf16& m, __bf16& l) {
  h = (__bf16)x;
  const float r1 = x - (float)h;
  m = (__bf16)r1;
  l = (__bf16)(r1 - (float)m);
}
// split3 with both subtractions pinned to scalar v_sub_f32 (the same bits).  Unrolled over adjacent values, plain split3 is
// SLP-packed into v_pk_add_f32, and packed f32 issued beside the partner wave's MFMAs costs more than the two scalar
// instructions it replaces: the staging waves of conv1d_bsplit_kernel (one MFMA wave and one staging wave per SIMD) use this
// form, -4 .. 6 % per k = 7 launch.  Not a general win: with three waves per SIMD (conv1d_pws_kernel) it measured
// slower, and in conv1d_gemm_split_kernel no different.
__device__ __forceinline__ void split3_scalar_sub(float x, __bf16& h, __bf16& m, __bf16& l) {
  h = (__bf16)x;
  float r1, r2;
  asm("v_sub_f32 %0, %1, %2" : "=v"(r1) : "v"(x), "v"((float)h));
  m = (__bf16)r1;
  asm("v_sub_f32 %0, %1, %2" : "=v"(r2) : "v"(r1), "v"((float)m));
  l = (__bf16)r2;
}

// Raw workgroup barrier between compiler fences: no s_waitcnt of its own (the caller has waited for exactly what it needs).
__device__ __forceinline__ void wg_barrier() {
  asm volatile("" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

// Position in the logical tile order of virtual workgroup v of n.  Workgroups are dispatched round-robin over the 8 XCDs
// (observed: block i -> XCD i % 8, speed only, never correctness): the remap makes each XCD walk a CONTIGUOUS range of the
// logical order (the first n % 8 XCDs take one tile more).  With a tile list ordered (co-tile slowest, then batch/phase, then time
// tile) the workgroups resident on one XCD then share one C_out tile, i.e. stream the same weight slabs through that XCD's
// private L2.  The kernels keep only their own unpacking of the id.  V is int or unsigned, whichever the caller's id is (the
// shift then is the one that kernel was measured with).
template <class V>
__host__ __device__ constexpr int xcd_contiguous_id(V v, int n) {
  const int q8 = n >> 3, r8 = n & 7;
  const int xcd = v & 7, within = v >> 3;
  return (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + within;
}
constexpr bool xcd_contiguous_is_permutation(int n) {
  bool seen[64] = {};
  for (int v = 0; v < n; ++v) {
    const int id = xcd_contiguous_id(v, n);
    if (id < 0 || id >= n || seen[id]) return false;
    seen[id] = true;
  }
  return true;
}
static_assert(xcd_contiguous_is_permutation(1) && xcd_contiguous_is_permutation(7) && xcd_contiguous_is_permutation(8) &&
                  xcd_contiguous_is_permutation(9) && xcd_contiguous_is_permutation(13) && xcd_contiguous_is_permutation(64),
              "xcd_contiguous_id must map [0, n) onto [0, n)");

// The same idea for launches padded to a multiple of 8 workgroups: XCD k takes [k * per_xcd, (k + 1) * per_xcd) of the logical
// order.  Host half: per_xcd and the padded 1-D grid for `total` workgroups.  The device half stays written out in its two
// kernels (vq_fwd_kernel, conv1d_wgrad_kmajor_kernel): logical = (blockIdx.x & 7) * per_xcd + (blockIdx.x >> 3), and the overhang
// workgroups (blockIdx.x >> 3 >= per_xcd, or logical >= total) return at once -- behind a helper, with an id-or-minus-one or a
// bool result alike, the compiler emitted a different test and schedule for both kernels.
struct XcdGrid {
  int per_xcd;
  unsigned grid;
};
inline XcdGrid xcd_padded_grid(long long total) {
  const int per_xcd = (int)((total + 7) / 8);
  return {per_xcd, (unsigned)(8 * per_xcd)};
}

// ---- host-side launch helpers

constexpr size_t FAC_LDS_MAX = 160 * 1024;   // LDS of one gfx950 CU: the most dynamic shared memory a kernel can be opted in to

// Opts kernel Kern in to `bytes` of dynamic LDS, once per process.  The flag belongs to the kernel VALUE, not to its type: kernels
// of one signature (every ConvArgs kernel) each get their own.
template <auto Kern>
inline void allow_dynamic_lds(size_t bytes = FAC_LDS_MAX) {
  static bool done = false;
  if (!done) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(Kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    done = true;
  }
}

// Compute units of the current device (cached per device), 0 when unknown: each caller decides what "unknown" means to it.
constexpr int FAC_MAX_DEV = 16;
inline int device_cus() {
  static int cus[FAC_MAX_DEV] = {0};
  int dev = 0, v = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= FAC_MAX_DEV) return 0;
  if (cus[dev] == 0 && hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess) cus[dev] = v;
  return cus[dev];
}

}  // namespace fac

// Issue priorities (s_setprio) of the two wave roles of the split-bf16 kernels (conv1d_bsplit / bsplit2 / gemm_split / wgrad k-major):
// MFMA waves and staging waves share a SIMD; the arbiter picks the higher priority when both have an instruction ready.
#define FAC_PRIO_STAGE 3
#define FAC_PRIO_MFMA 0

