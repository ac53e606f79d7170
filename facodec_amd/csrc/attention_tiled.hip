// The StyleEncoder's softmax attention (modules/attentions.py:168-199) with both products register-tiled: the form fac_attention
// launches on its LDS route wherever fac_attention_form says FAC_ATTN_FORM_TILED.  Every output is computed by the operations of
// attention_kernel (misc.hip) in the same order -- scores: an fmaf chain over d ascending on queries pre-divided by sqrtf(dk); the
// -1e4 mask rule; the softmax: lane-strided max and sum, xor-shuffle reduction, expf, __fdiv_rn; out: an fmaf chain over tk
// ascending -- so the two kernels return the same bits.  Only who computes what, the LDS layout and the load schedule differ.
//
// One workgroup of 4 waves owns ATTN_TILED_QT = 32 queries of one (b, head); wave w owns queries 8w .. 8w + 7 in both products.
//   scores  S[q][tk] = sum_d qs[d][q] K[d][tk]: a lane owns 4 consecutive keys (one 16-byte global load per row of K) x the
//           wave's 8 queries (two broadcast ds_read_b128 of qs[d]): 32 FMAs per 3 loads.  Rows of K are requested 8 ahead.
//   out     O[d][q] = sum_tk P[q][tk] V[d][tk]: V passes through LDS in passes of ATTN_TILED_KC = 32 keys x all dk rows; a lane
//           owns the rows d = lane + 64 i (i < 4) x the wave's 8 queries and walks a pass 4 keys at a time: 4 ds_read_b128 of V
//           (row stride 36 floats: the 16 rows a lane group reads fall into 16 different 16-byte slots) and 8 broadcast
//           ds_read_b128 of P feed 128 FMAs.  The next pass's rows are requested into registers before the FMAs of this one; the
//           first pass is requested before the softmax.
// The score rows are padded with +0 up to a multiple of KC keys and the last V pass with -0: fmaf(+0, -0, a) == a for EVERY a (a
// NaN, an infinity and -0 included), so the padded steps at the end of a chain change no bit of it.
// LDS: max(dk x 32 queries, 256 x 36 of a V pass) -- the queries are dead once the scores are written -- + 32 x round32(T) scores.
#include "common.h"

namespace fac {

constexpr int ATTN_TILED_QT = 32;                  // queries per workgroup (8 per wave)
constexpr int ATTN_TILED_KC = 32;                  // keys per V pass
constexpr int ATTN_TILED_VS = ATTN_TILED_KC + 4;   // LDS row stride of a V pass in floats
constexpr int ATTN_TILED_DK = 256;                 // most rows of q / k / v per head: 4 per lane in the P V product
static_assert(ATTN_TILED_DK * ATTN_TILED_QT <= ATTN_TILED_DK * ATTN_TILED_VS, "the queries share the V pass's LDS");

static inline int attn_tiled_ts(int T) { return (T + ATTN_TILED_KC - 1) / ATTN_TILED_KC * ATTN_TILED_KC; }
static inline size_t attn_tiled_lds(int T) {
  return ((size_t)ATTN_TILED_DK * ATTN_TILED_VS + (size_t)ATTN_TILED_QT * attn_tiled_ts(T)) * sizeof(float);
}

// row[t .. t + 3], `fill` where t + i >= T.  vec: T % 4 == 0 and the tensors are 16-byte aligned, so t % 4 == 0 makes the four
// one aligned piece that lies wholly below T or wholly past it.
__device__ __forceinline__ float4 attn_ld4(const float* __restrict__ row, int t, int T, bool vec, float fill) {
  if (vec) return t < T ? *reinterpret_cast<const float4*>(row + t) : make_float4(fill, fill, fill, fill);
  float4 r;
  r.x = t < T ? row[t] : fill;
  r.y = t + 1 < T ? row[t + 1] : fill;
  r.z = t + 2 < T ? row[t + 2] : fill;
  r.w = t + 3 < T ? row[t + 3] : fill;
  return r;
}

__device__ __forceinline__ float attn_f4(const float4& v, int i) { return i == 0 ? v.x : i == 1 ? v.y : i == 2 ? v.z : v.w; }

__global__ __launch_bounds__(256) void attention_tiled_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                              const float* __restrict__ v, const float* __restrict__ mask,
                                                              float* __restrict__ out, int n_heads, int dk, int T, int TS, int vec) {
  constexpr int QT = ATTN_TILED_QT, KC = ATTN_TILED_KC, VS = ATTN_TILED_VS;
  extern __shared__ __align__(16) float sm[];
  float* qs = sm;                          // [dk][QT] pre-scaled queries, until the scores are written
  float* vs = sm;                          // [256][VS] one pass of V, after that
  float* sc = sm + ATTN_TILED_DK * VS;     // [QT][TS]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int tq0 = blockIdx.x * QT, j0 = wave * 8;
  const int h = blockIdx.y, b = blockIdx.z;
  const long long base = ((long long)b * n_heads + h) * dk * T;
  const float* qg = q + base;
  const float* kg = k + base;
  const float* vg = v + base;
  const float* mrow = mask ? mask + (long long)b * T : nullptr;
  const float scale = sqrtf((float)dk);
  for (int i = threadIdx.x; i < dk * QT; i += 256) {
    const int d = i / QT, j = i - d * QT;
    const int tq = tq0 + j;
    qs[i] = tq < T ? __fdiv_rn(qg[(long long)d * T + tq], scale) : 0.f;
  }
  __syncthreads();

  // ---- scores[j][tk] = sum_d qs[d][j] * k[d][tk], d ascending; 256 keys per step of the wave, 4 per lane
  float mq[8];
#pragma unroll
  for (int jj = 0; jj < 8; ++jj) mq[jj] = mrow && tq0 + j0 + jj < T ? mrow[tq0 + j0 + jj] : 1.f;
  for (int kb = 0; kb < TS; kb += 256) {
    const int tk0 = kb + lane * 4;
    float4 acc[8];
#pragma unroll
    for (int jj = 0; jj < 8; ++jj) acc[jj] = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 cur[8], nxt[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) cur[u] = u < dk ? attn_ld4(kg + (long long)u * T, tk0, T, vec, 0.f) : make_float4(0.f, 0.f, 0.f, 0.f);
    for (int d0 = 0; d0 < dk; d0 += 8) {
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int dn = d0 + 8 + u;
        nxt[u] = dn < dk ? attn_ld4(kg + (long long)dn * T, tk0, T, vec, 0.f) : make_float4(0.f, 0.f, 0.f, 0.f);
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        if (d0 + u < dk) {
          const float4 qa = *reinterpret_cast<const float4*>(qs + (d0 + u) * QT + j0);
          const float4 qb = *reinterpret_cast<const float4*>(qs + (d0 + u) * QT + j0 + 4);
#pragma unroll
          for (int jj = 0; jj < 8; ++jj) {
            const float qv = jj < 4 ? attn_f4(qa, jj) : attn_f4(qb, jj - 4);
            acc[jj].x = fmaf(qv, cur[u].x, acc[jj].x);
            acc[jj].y = fmaf(qv, cur[u].y, acc[jj].y);
            acc[jj].z = fmaf(qv, cur[u].z, acc[jj].z);
            acc[jj].w = fmaf(qv, cur[u].w, acc[jj].w);
          }
        }
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) cur[u] = nxt[u];
    }
    if (tk0 < TS) {
      float mk[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) mk[i] = mrow && tk0 + i < T ? mrow[tk0 + i] : 1.f;
#pragma unroll
      for (int jj = 0; jj < 8; ++jj) {
        const bool live = mrow && tq0 + j0 + jj < T;     // the mask rule holds for the queries below T only, as in attention_kernel
        float s[4] = {acc[jj].x, acc[jj].y, acc[jj].z, acc[jj].w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          if (live && mq[jj] * mk[i] == 0.f) s[i] = -1e4f;
          if (tk0 + i >= T) s[i] = 0.f;                  // the +0 padding of the row
        }
        *reinterpret_cast<float4*>(sc + (j0 + jj) * TS + tk0) = make_float4(s[0], s[1], s[2], s[3]);
      }
    }
  }

  // the first pass of V is on its way while the softmax runs.  Thread i stages the float4 pieces i + 256 u: row (i >> 3) + 32 u,
  // keys 4 (i & 7) .. + 3 of the pass.
  float4 pf[8];
  const int srow = threadIdx.x >> 3, scol = (threadIdx.x & 7) * 4;
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    const int r = srow + 32 * u;
    pf[u] = r < dk ? attn_ld4(vg + (long long)r * T, scol, T, vec, -0.f) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  __syncthreads();

  // ---- softmax over tk: one wave handles 8 query rows (the rows of queries past T are never used: left as they are)
  for (int j = wave; j < QT && tq0 + j < T; j += 4) {
    float mx = -INFINITY;
    for (int tk = lane; tk < T; tk += 64) mx = fmaxf(mx, sc[j * TS + tk]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    float sum = 0.f;
    for (int tk = lane; tk < T; tk += 64) {
      const float e = expf(sc[j * TS + tk] - mx);
      sc[j * TS + tk] = e;
      sum += e;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    for (int tk = lane; tk < T; tk += 64) sc[j * TS + tk] = __fdiv_rn(sc[j * TS + tk], sum);
  }
  __syncthreads();     // the probabilities are final, and no wave reads the queries any more

  // ---- out[d][tq] = sum_tk p[tq][tk] * v[d][tk], tk ascending
  float acc[4][8];
#pragma unroll
  for (int dd = 0; dd < 4; ++dd)
#pragma unroll
    for (int jj = 0; jj < 8; ++jj) acc[dd][jj] = 0.f;
  for (int tk0 = 0; tk0 < TS; tk0 += KC) {
    if (tk0) __syncthreads();              // every wave is done with the pass before
#pragma unroll
    for (int u = 0; u < 8; ++u) *reinterpret_cast<float4*>(vs + (srow + 32 * u) * VS + scol) = pf[u];
    __syncthreads();
    if (tk0 + KC < TS) {
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int r = srow + 32 * u;
        pf[u] = r < dk ? attn_ld4(vg + (long long)r * T, tk0 + KC + scol, T, vec, -0.f) : make_float4(0.f, 0.f, 0.f, 0.f);
      }
    }
#pragma unroll
    for (int t4 = 0; t4 < KC; t4 += 4) {
      float4 pp[8], vv[4];
#pragma unroll
      for (int jj = 0; jj < 8; ++jj) pp[jj] = *reinterpret_cast<const float4*>(sc + (j0 + jj) * TS + tk0 + t4);
#pragma unroll
      for (int dd = 0; dd < 4; ++dd)
        if (dd * 64 < dk) vv[dd] = *reinterpret_cast<const float4*>(vs + (lane + 64 * dd) * VS + t4);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int dd = 0; dd < 4; ++dd)
          if (dd * 64 < dk) {
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) acc[dd][jj] = fmaf(attn_f4(pp[jj], i), attn_f4(vv[dd], i), acc[dd][jj]);
          }
    }
  }
#pragma unroll
  for (int dd = 0; dd < 4; ++dd) {
    const int d = lane + 64 * dd;
    if (d < dk) {
      float* orow = out + base + (long long)d * T + tq0 + j0;
#pragma unroll
      for (int g = 0; g < 8; g += 4) {
        if (vec) {
          if (tq0 + j0 + g < T) *reinterpret_cast<float4*>(orow + g) = make_float4(acc[dd][g], acc[dd][g + 1], acc[dd][g + 2], acc[dd][g + 3]);
        } else {
#pragma unroll
          for (int jj = g; jj < g + 4; ++jj)
            if (tq0 + j0 + jj < T) orow[jj] = acc[dd][jj];
        }
      }
    }
  }
}

}  // namespace fac

using namespace fac;

// Whether the tiled kernel takes (dk, T): at most 256 rows per head, and a V pass (256 x 36 floats) plus 32 score rows of T rounded
// up to 32 keys in the 160 KiB of LDS: T <= 992.  Shapes only.
extern "C" int fac_attention_tiled_fits(int dk, int T) {
  return dk > 0 && T > 0 && dk <= ATTN_TILED_DK && T <= (1 << 20) && attn_tiled_lds(T) <= FAC_LDS_MAX ? 1 : 0;
}

extern "C" int fac_attention_tiled(const float* q, const float* k, const float* v, const float* mask, float* out, int B,
                                   int n_heads, int dk, int T, fac_stream_t stream) {
  FAC_REQUIRE(q && k && v && out && B > 0 && n_heads > 0 && dk > 0 && T > 0, "attention_tiled: bad arguments");
  FAC_REQUIRE(fac_attention_tiled_fits(dk, T), "attention_tiled: dk=%d T=%d outside the tiled layout (dk <= %d, T <= 992)", dk, T,
              ATTN_TILED_DK);
  FAC_REQUIRE(B <= 65535 && n_heads <= 65535, "attention_tiled: B or heads above 65535");
  const int vec = T % 4 == 0 && ((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)out) % 16 == 0;
  allow_dynamic_lds<attention_tiled_kernel>();
  dim3 grid((T + ATTN_TILED_QT - 1) / ATTN_TILED_QT, n_heads, B);
  hipLaunchKernelGGL(attention_tiled_kernel, grid, dim3(256), attn_tiled_lds(T), (hipStream_t)stream, q, k, v, mask, out, n_heads,
                     dk, T, attn_tiled_ts(T), vec);
  return check_launch("attention_tiled");
}
