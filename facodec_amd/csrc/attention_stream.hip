// Softmax attention with a running max and sum (modules/attentions.py:168-199) for any number of frames: the route fac_attention
// takes where attention_kernel's 16 x T score tile no longer fits the LDS (misc.hip).  Same layouts and semantics: q, k, v, out
// (B, H*dk, T) fp32 with T contiguous, queries pre-divided by sqrtf(dk) (IEEE division), a pair with mask[b,tq] * mask[b,tk] == 0
// REPLACED by the score -1e4 (so a masked query has uniform weights over all T keys, masked ones included), softmax over keys,
// out = P v.  Keys past T in the last key tile are no keys at all: score -inf, weight exactly 0.
//
// One workgroup of 8 waves owns ATTN_STREAM_QT = 128 query columns of one (b, head), 16 per wave, and walks the
// keys in tiles of ATTN_STREAM_KT = 64.  Both products run on the exact-fp32 matrix pipe (v_mfma_f32_16x16x4_f32), transposed so
// that the QUERY is the column (= lane & 15) of every accumulator:
//   S^T[key][query] = sum_d K[d][key] q[d][query]      A = K tile (LDS), B = q (registers, loaded once, already in operand order)
//   O^T[d][query]  += sum_key V[d][key] P^T[key][query] A = V tile (LDS), B = P^T
// The running max m, the running sum l and the rescale exp(m_old - m_new) are then one value per lane, and a 16 x 16 block of P^T
// in accumulator layout (lane group j = lane >> 4 holds rows 4j .. 4j+3) already IS a B operand for every register r: the k index
// of the 16x16x4 step is the lane group, so step (a, r) sums over the four keys the four lane groups hold in register r of block
// a.  No lane movement, no LDS round trip for P; the A operand (V) is read from LDS at those same four keys.  Block a of S^T takes
// the keys 4 rho + a (rho = accumulator row), not 16 a + rho: then lane (i, j) needs K[d][4i .. 4i+3] for the four blocks and
// V[d][16j + 4r .. + 3] for the four steps of register r, one ds_read_b128 each.
// The K tile and the V tile each have an LDS buffer of (dk rounded up to 16) x 64 floats with a row stride of 68 (17 float4: the 16
// rows a quarter wave reads V from fall into 16 different bank groups), and the key tile's 64 mask values: 2 x 68 KiB at dk = 256, whatever T is; one workgroup per
// CU, two waves per SIMD.  Global latency hides behind the other product: the V tile is loaded into registers before the score
// product and stored to LDS after it, the next K tile before and after the P V product; two barriers per key tile.
#include "common.h"

namespace fac {

constexpr int ATTN_STREAM_QT = 128;   // queries per workgroup (32 per wave)
constexpr int ATTN_STREAM_KT = 64;    // keys per LDS tile
constexpr int ATTN_STREAM_LD = ATTN_STREAM_KT + 4;   // LDS row stride in floats
constexpr int ATTN_STREAM_THREADS = 512;   // 8 waves of 16 queries, two per SIMD

// NB: 16-row blocks of d (dk <= 16 NB; rows dk .. 16 NB - 1 are zero in LDS and in the q registers, and are not stored)
template <int NB>
__global__ __launch_bounds__(ATTN_STREAM_THREADS) void attention_stream_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                               const float* __restrict__ v, const float* __restrict__ mask,
                                                               float* __restrict__ out, int n_heads, int dk, int T) {
  constexpr int QT = ATTN_STREAM_QT, KT = ATTN_STREAM_KT, LD = ATTN_STREAM_LD, DKP = 16 * NB;
  constexpr int QB = 1;             // 16-query blocks per wave
  constexpr int NTH = ATTN_STREAM_THREADS;
  constexpr int NV = DKP * KT / (NTH * 4);   // float4 of one tile per thread
  static_assert(NV * NTH * 4 == DKP * KT && QT == NTH / 64 * 16 * QB, "tile split");
  extern __shared__ float lds[];
  float* kt = lds;                  // [DKP][LD] K tile
  float* vt = lds + DKP * LD;       // [DKP][LD] V tile
  float* mt = vt + DKP * LD;        // [KT] the key tile's mask values (1 where there is no mask)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i = lane & 15, j = lane >> 4;
  const int h = blockIdx.y, b = blockIdx.z;
  const long long base = ((long long)b * n_heads + h) * dk * T;
  const float* qg = q + base;
  const float* kg = k + base;
  const float* vg = v + base;
  const float* mrow = mask ? mask + (long long)b * T : nullptr;
  const float scale = sqrtf((float)dk);
  int tq[QB];        // this lane's queries (every accumulator's column)
  float mq[QB];
  float qr[QB][DKP / 4];   // B operand of the score product, step ks: q[4 ks + j][tq] / sqrt(dk)
#pragma unroll
  for (int u = 0; u < QB; ++u) {
    tq[u] = blockIdx.x * QT + wave * (16 * QB) + 16 * u + i;
#pragma unroll
    for (int ks = 0; ks < DKP / 4; ++ks) {
      const int d = 4 * ks + j;
      qr[u][ks] = (d < dk && tq[u] < T) ? __fdiv_rn(qg[(long long)d * T + tq[u]], scale) : 0.f;
    }
    mq[u] = (mrow && tq[u] < T) ? mrow[tq[u]] : 1.f;
  }

  f32x4 o[QB][NB];
  float m[QB], l[QB];   // running max; running sum over the keys THIS lane group holds (summed over the groups at the end)
#pragma unroll
  for (int u = 0; u < QB; ++u) {
    m[u] = -INFINITY;
    l[u] = 0.f;
#pragma unroll
    for (int db = 0; db < NB; ++db) o[u][db] = f32x4{0.f, 0.f, 0.f, 0.f};
  }

  // One tile in flight between global memory and LDS.  Thread tid moves, in pass `it`, the keys vc .. vc + 3 of row
  // it * NTH / 16 + vd: a 32-bit lane offset that changes with neither the pass nor the tile, on a uniform 64-bit base (below 2^30
  // floats: fac_attention_stream refuses T above 2^24, and vd < 32).  A row starts wherever d * T puts it, so the 16-byte loads
  // are only 4-byte aligned (memcpy: the compiler may not assume more; global memory takes them).  Only the LAST tile can reach
  // past T -- and a 16-byte load there past the end of the tensor: it is not fetched ahead but moved key by key, zero past T, when
  // the tile is stored.  Rows past dk are zero.
  f32x4 st[NV];
  const int vd = tid >> 4, vc = (tid & 15) * 4;
  const unsigned voff = (unsigned)((long long)vd * T + vc);
  auto fetch = [&](const float* __restrict__ src, int tk0) {
    if (tk0 + KT <= T) {
#pragma unroll
      for (int it = 0; it < NV; ++it) {
        const int d0 = it * (NTH / 16);
        st[it] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (d0 + vd < dk) __builtin_memcpy(&st[it], &(src + ((long long)d0 * T + tk0))[voff], sizeof(f32x4));
      }
    }
  };
  auto stash = [&](float* dst, const float* __restrict__ src, int tk0) {
    if (tk0 + KT <= T) {
#pragma unroll
      for (int it = 0; it < NV; ++it) *reinterpret_cast<f32x4*>(dst + (it * (NTH / 16) + vd) * LD + vc) = st[it];
    } else {
#pragma unroll 1
      for (int it = 0; it < NV; ++it) {
        const int d = it * (NTH / 16) + vd;
        f32x4 t4;
#pragma unroll
        for (int w = 0; w < 4; ++w) t4[w] = (d < dk && tk0 + vc + w < T) ? src[(long long)d * T + tk0 + vc + w] : 0.f;
        *reinterpret_cast<f32x4*>(dst + d * LD + vc) = t4;
      }
    }
  };

  fetch(kg, 0);
  stash(kt, kg, 0);
  __syncthreads();
  for (int tk0 = 0; tk0 < T; tk0 += KT) {
    const bool more = tk0 + KT < T;
    fetch(vg, tk0);                       // in flight during the score product
    const float mk = (mrow && tid < KT && tk0 + tid < T) ? mrow[tk0 + tid] : 1.f;
    __builtin_amdgcn_sched_barrier(0);
    // ---- S^T: block a, row rho = 4 j + r of this lane  <->  key tk0 + 4 rho + a = tk0 + 16 j + 4 r + a
    f32x4 s[QB][4];
#pragma unroll
    for (int u = 0; u < QB; ++u)
#pragma unroll
      for (int a = 0; a < 4; ++a) s[u][a] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < DKP / 4; ++ks) {
      const f32x4 kv = *reinterpret_cast<const f32x4*>(kt + (4 * ks + j) * LD + 4 * i);
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int u = 0; u < QB; ++u) s[u][a] = __builtin_amdgcn_mfma_f32_16x16x4f32(kv[a], qr[u][ks], s[u][a], 0, 0, 0);
      if ((ks & 3) == 3) __builtin_amdgcn_sched_barrier(0);   // keeps the scheduler from hoisting every LDS read of the unrolled loop
    }
    __builtin_amdgcn_sched_barrier(0);
    stash(vt, vg, tk0);                        // nobody reads the V buffer between the barrier that ended the last tile and the next one
    if (tid < KT) mt[tid] = mk;
    __syncthreads();   // V tile and mask tile complete; every wave is done with the K tile
    if (more) fetch(kg, tk0 + KT);        // in flight during the softmax step and the P V product
    __builtin_amdgcn_sched_barrier(0);
    // ---- mask replacement, tail keys, running max / sum
#pragma unroll
    for (int u = 0; u < QB; ++u) {
      float mx = -INFINITY;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const f32x4 mkv = *reinterpret_cast<const f32x4*>(mt + 16 * j + 4 * r);
#pragma unroll
        for (int a = 0; a < 4; ++a) {
          const int tk = tk0 + 16 * j + 4 * r + a;
          float sv = s[u][a][r];
          if (mq[u] * mkv[a] == 0.f) sv = -1e4f;     // masked pair: the score is REPLACED (still a key)
          if (tk >= T) sv = -INFINITY;               // not a key: weight exactly 0
          s[u][a][r] = sv;
          mx = fmaxf(mx, sv);
        }
      }
      mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      const float m_new = fmaxf(m[u], mx);          // finite: key tk0 is below T
      const float alpha = expf(m[u] - m_new);       // 0 on the first tile (m = -inf)
      float psum = 0.f;
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float p = expf(s[u][a][r] - m_new);
          s[u][a][r] = p;
          psum += p;
        }
      l[u] = l[u] * alpha + psum;
      m[u] = m_new;
#pragma unroll
      for (int db = 0; db < NB; ++db)
#pragma unroll
        for (int r = 0; r < 4; ++r) o[u][db][r] *= alpha;
    }
    // ---- O^T += V P^T: step (a, r) sums over the keys tk0 + 16 j + 4 r + a of the four lane groups j
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int db = 0; db < NB; ++db) {
        const f32x4 vv = *reinterpret_cast<const f32x4*>(vt + (16 * db + i) * LD + 16 * j + 4 * r);
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
          for (int u = 0; u < QB; ++u) o[u][db] = __builtin_amdgcn_mfma_f32_16x16x4f32(vv[a], s[u][a][r], o[u][db], 0, 0, 0);
        if ((db & 3) == 3) __builtin_amdgcn_sched_barrier(0);
      }
    __builtin_amdgcn_sched_barrier(0);
    if (more) stash(kt, kg, tk0 + KT);
    __syncthreads();   // next K tile complete; every wave is done with the V tile
  }

#pragma unroll
  for (int u = 0; u < QB; ++u) {
    float lt = l[u];
    lt += __shfl_xor(lt, 16, 64);
    lt += __shfl_xor(lt, 32, 64);
    if (tq[u] < T) {
#pragma unroll
      for (int db = 0; db < NB; ++db)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int d = 16 * db + 4 * j + r;     // accumulator row
          if (d < dk) out[base + (long long)d * T + tq[u]] = __fdiv_rn(o[u][db][r], lt);
        }
    }
  }
}

template <int NB>
static int launch_attention_stream(const float* q, const float* k, const float* v, const float* mask, float* out, int B, int n_heads,
                                   int dk, int T, hipStream_t stream) {
  const size_t lds = ((size_t)2 * 16 * NB * ATTN_STREAM_LD + ATTN_STREAM_KT) * sizeof(float);   // K tile + V tile + mask tile
  allow_dynamic_lds<attention_stream_kernel<NB>>();
  dim3 grid((T + ATTN_STREAM_QT - 1) / ATTN_STREAM_QT, n_heads, B);
  hipLaunchKernelGGL(attention_stream_kernel<NB>, grid, dim3(ATTN_STREAM_THREADS), lds, stream, q, k, v, mask, out, n_heads, dk, T);
  return check_launch("attention_stream");
}

}  // namespace fac

using namespace fac;

extern "C" int fac_attention_stream_tile(int which) { return which == 0 ? ATTN_STREAM_QT : ATTN_STREAM_KT; }

extern "C" int fac_attention_stream(const float* q, const float* k, const float* v, const float* mask, float* out, int B,
                                    int n_heads, int dk, int T, fac_stream_t stream) {
  FAC_REQUIRE(q && k && v && out && B > 0 && n_heads > 0 && dk > 0 && T > 0, "attention_stream: bad arguments");
  FAC_REQUIRE(dk <= 256, "attention_stream: dk=%d above 256 (one wave holds 16 queries x dk of output and of q in registers)", dk);
  FAC_REQUIRE(B <= 65535 && n_heads <= 65535, "attention_stream: B or heads above 65535");
  FAC_REQUIRE(T <= (1 << 24), "attention_stream: T=%d above 2^24 frames (32-bit lane offsets inside a key tile's rows)", T);
  hipStream_t s = (hipStream_t)stream;
  if (dk <= 32) return launch_attention_stream<2>(q, k, v, mask, out, B, n_heads, dk, T, s);
  if (dk <= 64) return launch_attention_stream<4>(q, k, v, mask, out, B, n_heads, dk, T, s);
  if (dk <= 128) return launch_attention_stream<8>(q, k, v, mask, out, B, n_heads, dk, T, s);
  return launch_attention_stream<16>(q, k, v, mask, out, B, n_heads, dk, T, s);
}
