// The epilogue of the forward conv kernels that hand their accumulators to all waves through an fp32 tile in LDS (and of
// conv1d_cin1_kernel, whose quads come from FMAs): one lane takes four consecutive output samples of one channel,
//   x = v + bias;  x = snake(x, alpha_out);  x = act(x);  y = x + res;  y2 = snake(y, alpha2)
// in this order, with the scalar snake_apply / snake_inv / apply_act_slow of common.h.  The order is what the kernels' bit-exactness
// claims rest on: it is written here once.  A site keeps what really differs: its quad loop, the gather of v[4], the output offset,
// which samples are its own (`ok`) and whether the quad may move as 16 bytes (`vec`).
#pragma once
#include "common.h"

namespace fac {

// Per-channel constants: bias, alpha_out and 1 / (alpha_out + 1e-9), alpha2 and 1 / (alpha2 + 1e-9).  An absent operand leaves zeros.
struct EpiRow {
  float bs, al, inv, a2, i2;
};
__device__ __forceinline__ EpiRow epi_row_load(bool valid, int co, const float* bias, const float* alpha, const float* alpha2) {
  EpiRow r = {0.f, 0.f, 0.f, 0.f, 0.f};
  if (valid) {
    if (bias) r.bs = bias[co];
    if (alpha) { r.al = alpha[co]; r.inv = snake_inv(r.al); }
    if (alpha2) { r.a2 = alpha2[co]; r.i2 = snake_inv(r.a2); }
  }
  return r;
}

// 16-byte accesses are possible at every offset that is a multiple of 4 floats: strides and the bases of the operands present.
__device__ __forceinline__ bool epi_vec_ok(const float* y, const float* y2, const float* res, long long y_cs, long long y_bs) {
  return (y_cs & 3) == 0 && (y_bs & 3) == 0 && (!y || (reinterpret_cast<unsigned long long>(y) & 15) == 0) &&
         (!y2 || (reinterpret_cast<unsigned long long>(y2) & 15) == 0) && (!res || (reinterpret_cast<unsigned long long>(res) & 15) == 0);
}

// `ok` mask of a quad of which the first n samples exist (n >= 1): the end of a row
__device__ __forceinline__ unsigned epi_first(long long n) { return n >= 4 ? 15u : (1u << (int)n) - 1u; }

// bias, Snake, the cold activation: the value the residual is added to
__device__ __forceinline__ float epi_pre(float x, const EpiRow& row, bool has_alpha, int act) {
  x += row.bs;
  if (has_alpha) x = snake_apply(x, row.al, row.inv);
  if (act != FAC_ACT_NONE) x = apply_act_slow(x, act);
  return x;
}

// One sample at offset o.  A null y / y2 / res: that operand is absent.
__device__ __forceinline__ void epi_one(float x, const EpiRow& row, bool has_alpha, int act, float* y, float* y2, const float* res,
                                        long long o) {
  x = epi_pre(x, row, has_alpha, act);
  if (res) x += res[o];
  if (y) y[o] = x;
  if (y2) y2[o] = snake_apply(x, row.a2, row.i2);
}

// Four samples of one channel at offsets o + i * step.  ok: bit i set = sample i is this lane's to write; vec: all four are, step == 1
// and o is 16-byte aligned in every operand (epi_vec_ok): one float4 residual load, float4 stores.  Otherwise sample by sample under
// `ok`.  The residual quad is read before any store (y may alias res).  A sample without a residual adds 0.f (so a -0.f result leaves
// as +0.f, unlike epi_one's); RES = false is for a kernel that takes no residual and adds nothing (conv1d_cin1_kernel).
template <bool RES = true>
__device__ __forceinline__ void epi_quad(float (&v)[4], const EpiRow& row, bool has_alpha, int act, float* y, float* y2, const float* res,
                                         long long o, long long step, unsigned ok, bool vec) {
  float rv[4] = {0.f, 0.f, 0.f, 0.f};
  if (RES && res) {
    if (vec) {
      const float4 r4 = *reinterpret_cast<const float4*>(res + o);
      rv[0] = r4.x; rv[1] = r4.y; rv[2] = r4.z; rv[3] = r4.w;
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) rv[i] = (ok >> i & 1) ? res[o + i * step] : 0.f;
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    v[i] = epi_pre(v[i], row, has_alpha, act);
    if (RES) v[i] += rv[i];
  }
  float w[4] = {0.f, 0.f, 0.f, 0.f};
  if (y2) {
#pragma unroll
    for (int i = 0; i < 4; ++i) w[i] = snake_apply(v[i], row.a2, row.i2);
  }
  if (vec) {
    if (y) *reinterpret_cast<float4*>(y + o) = make_float4(v[0], v[1], v[2], v[3]);
    if (y2) *reinterpret_cast<float4*>(y2 + o) = make_float4(w[0], w[1], w[2], w[3]);
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (!(ok >> i & 1)) continue;
      if (y) y[o + i * step] = v[i];
      if (y2) y2[o + i * step] = w[i];
    }
  }
}

}  // namespace fac
