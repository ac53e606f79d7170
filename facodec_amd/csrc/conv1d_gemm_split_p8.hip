// The split GEMM of conv1d_gemm_split.hip for launches whose input arrives as P8 planes (fac_conv_desc.x_p8): the same arithmetic in
// the same order -- every output equals conv1d_gemm_split_kernel's bit for bit -- in a workgroup small enough for two to share a CU.
//
// A P8 unit (16 bytes per (8-channel group, time step)) IS the B fragment of one lane of v_mfma_f32_32x32x16_bf16, so the input needs
// neither LDS nor staging waves: every lane loads its fragments straight from the planes (global_load_dwordx4, L2 hits: the
// co-resident workgroups of an XCD cover all row tiles of a few column tiles), a few K steps ahead of their MFMAs.
//   tile 64 rows x (64 * NCB) columns, 4 waves, all of them MFMA waves: each owns 64 rows x (16 * NCB) columns = 2 x (NCB / 2) blocks;
//   A (weights): the packed buffer of fac_pack_gemm_w_split unchanged ([row tile 128][chunk][plane][tap][128 rows][64 B], swizzle
//                piece ^ ((row >> 2) & 3)); a workgroup takes the upper or lower 4 KB of each (plane, tap) block by LDS-DMA, issued by
//                its own waves two chunks ahead (three stages of 12 KB x K);
//   B (inputs):  lane (column lane & 31, k-half lane >> 5) of K step ks of chunk c reads the unit of 8-channel group
//                4 c + 2 ks + (lane >> 5) at its column's time index (tap 1: one time step over); columns outside the signal read the
//                plane's trailing zero unit; a ragged last chunk clamps the group (its weights are zero);
//   epilogue:    the fp32 tile through the freed stage memory, as the 128 x 128 form's: bias, Snake / activation, residual, second
//                pre-activated output, row_phases interleave, 16-byte stores; row_phases 1 / 2 / 5 / 6 are compile-time cases, so no
//                run-time integer division is left per output quad.
// No barrier, register or stage is shared with the other workgroup of the CU: one's prologue, epilogue and store drain run under
// the other's MFMAs.
#include "conv1d_mfma.h"

namespace fac {

constexpr int GP_ROWS = 64;                    // output rows per workgroup: half a 128-row tile of the packed weights
constexpr int GP_PACK_ROWS = 128;              // rows per tile of the packed weights (fac_pack_gemm_w_split)
constexpr int GP_RB = 64;                      // bytes per weight row of a chunk: 32 bf16
constexpr int GP_BLK = GP_ROWS * GP_RB;        // one (plane, tap) of a workgroup's weights: 4 KB
constexpr int GP_NST = 3;                      // weight stages
constexpr int GP_D = 2;                        // K steps an input fragment is requested ahead of its MFMAs

__host__ __device__ constexpr int gp_stage_bytes(int K) { return 3 * K * GP_BLK; }
__host__ __device__ constexpr size_t gp_lds_bytes(int K, int NCB) {
  const size_t st = (size_t)GP_NST * gp_stage_bytes(K), epi = (size_t)GP_ROWS * (64 * NCB + 4) * sizeof(float);
  return st > epi ? st : epi;
}
static_assert(gp_lds_bytes(2, 4) <= 80 * 1024 && gp_lds_bytes(1, 4) <= 80 * 1024, "two workgroups must fit the 160 KB of a CU");

// 16 bytes per lane, 1 KiB per wave, global -> LDS at byte address `lds` (wave-uniform) + lane * 16.  Inline assembly, so that the
// compiler does not count it: it would make every later ds_read wait for the youngest of these (requested two chunks ahead).  The
// kernel waits for them itself (s_waitcnt vmcnt before the chunk's barrier).  M0 is saved and restored inside the statement.
__device__ __forceinline__ void gp_dma16(const unsigned char* src, unsigned lds) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(src), "s"(lds) : "memory");
}

typedef const __attribute__((address_space(1))) bf16x8 glb_bf16x8;

// ---- epilogue: one lane = 4 consecutive output samples of one channel (the value chain of conv1d_epilogue.h, as the 128 x 128 form).
// RPT: row_phases as a compile-time constant (0: taken from a.rp).  Rows of the packed tile are (channel cl, phase p), p fastest,
// 128 / rp channels per 128 rows; this workgroup holds rows [h64, h64 + 64) of them, so a channel may straddle the two workgroups of
// a packed tile (rp = 5: channel 12 is rows 60 .. 64): each emits the samples whose rows it owns.
template <int RPT, int COLS>
__device__ __forceinline__ void gp_epilogue(const ConvArgs& a, const float* tile, int tid, int rt64, int n0, int b, bool flat,
                                            long long n_total) {
  constexpr int EP = COLS + 4;
  const int rp = RPT > 0 ? RPT : a.rp;
  const int cpt = GP_PACK_ROWS / rp;                      // channels per packed tile (rp == 1: 128)
  const int QPR = (COLS * rp) / 4;                        // output quads per channel in this tile
  const int h64 = (rt64 & 1) * GP_ROWS;
  const int ch_base = (rt64 >> 1) * cpt;
  const int cl_lo = h64 / rp;
  int cl_hi = (h64 + GP_ROWS - 1) / rp;
  cl_hi = cl_hi < cpt - 1 ? cl_hi : cpt - 1;
  const int nq = (cl_hi - cl_lo + 1) * QPR;
  const long long u_tot = n_total * rp;                   // outputs per (clip | batch) row
  const long long u0 = (long long)n0 * rp;
  const bool al_ok = epi_vec_ok(a.y, a.y2, a.res, a.y_cs, a.y_bs) && (!flat || (a.T_out & 3) == 0);
  const bool has_alpha = a.alpha_out != nullptr;
  for (int q = tid; q < nq; q += 256) {
    const int cq = q / QPR, uq = q - cq * QPR;
    const int cl = cl_lo + cq;
    const int co = ch_base + cl;
    const long long u = u0 + 4 * uq;
    if (co >= a.C_out || u >= u_tot) continue;
    float v[4];
    unsigned own = 15u;                                    // samples whose tile rows this workgroup holds
    if (RPT == 1) {
      const float4 av = *reinterpret_cast<const float4*>(tile + (cl - h64) * EP + 4 * uq);
      v[0] = av.x; v[1] = av.y; v[2] = av.z; v[3] = av.w;
    } else {
      own = 0u;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int ul = 4 * uq + i, tl = ul / rp, p = ul - tl * rp;
        const int lr = cl * rp + p - h64;
        const bool mine = lr >= 0 && lr < GP_ROWS;
        own |= (unsigned)mine << i;
        v[i] = mine ? tile[lr * EP + tl] : 0.f;
      }
    }
    const EpiRow row = epi_row_load(true, co, a.bias, a.alpha_out, a.y2 ? a.alpha2 : nullptr);
    // output address of sample u (flat: u -> (clip, time); a quad never straddles clips when T_out % 4 == 0)
    long long o, lim = u_tot - u;
    if (flat) {
      const long long bb = u / a.T_out, tt = u - bb * a.T_out;
      o = bb * a.y_bs + (long long)co * a.y_cs + tt;
      lim = lim < a.T_out - tt ? lim : a.T_out - tt;
      if (lim < 4) {
        // ragged quad of the flattened layout (T_out % 4 != 0): sample by sample, each with its own (clip, time)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const long long ui = u + i;
          if (ui >= u_tot || !(own >> i & 1)) continue;
          const long long bi = ui / a.T_out, ti = ui - bi * a.T_out;
          epi_one(v[i], row, has_alpha, a.act, a.y, a.y2, a.res, bi * a.y_bs + (long long)co * a.y_cs + ti);
        }
        continue;
      }
    } else {
      o = (long long)b * a.y_bs + (long long)co * a.y_cs + u;
    }
    epi_quad(v, row, has_alpha, a.act, a.y, a.y2, a.res, o, 1, epi_first(lim) & own, al_ok && lim >= 4 && own == 15u);
  }
}

template <int K, int NCB>
__global__ __launch_bounds__(256, 2) void conv1d_gemm_split_p8_kernel(ConvArgs a) {
  constexpr int COLS = 64 * NCB;               // columns per workgroup
  constexpr int NBW = NCB / 2;                 // 32-column blocks per wave
  constexpr int STAGE = gp_stage_bytes(K);
  constexpr int PACK_CHUNK = 3 * K * GP_PACK_ROWS * GP_RB;     // one (row tile, chunk) slab of the packed weights
  constexpr int NSTEP = 2 * K;                 // K = 16 steps per chunk: step = tap * 2 + ks
  constexpr int RING = GP_D + 1;               // input fragment sets: GP_D in flight, one in use
  constexpr int LB = 3 * NBW;                  // input loads per lane and step
  constexpr int NA = 3 * K;                    // weight DMA instructions per wave and chunk
  static_assert(GP_D <= NSTEP && (GP_NST * NSTEP) % RING == 0, "static ring slots need NST * NSTEP to be a multiple of the ring");
  extern __shared__ __attribute__((aligned(16))) unsigned char sm[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const bool flat = a.gflat != 0;

  // XCD-aware work decode, as the 128 x 128 form's, over 64-row tiles
  int n0, rt64, b;
  {
    const int id = xcd_contiguous_id<unsigned>(blockIdx.x, gridDim.x);
    const int nt = a.n_t_tiles, nb = flat ? 1 : a.B;
    if (a.grt > 0) {         // row tile fastest: co-resident workgroups share the input lines of a few column tiles in their XCD's L2
      rt64 = id % a.grt;
      const int rest = id / a.grt;
      n0 = (rest % nt) * COLS;
      b = rest / nt;
    } else {
      n0 = (id % nt) * COLS;
      const int rest = id / nt;
      b = rest % nb;
      rt64 = rest / nb;
    }
  }
  const int S = (K == 2 && a.stride > 1) ? a.stride : 1;      // input stride: S phase sub-signals as virtual channel chunks
  const int n_chunks = ((a.C_in + 31) / 32) * S;
  const long long n_total = flat ? (long long)a.B * a.T_out : (long long)a.T_out;     // columns of this (clip | whole batch)

  const int l31 = lane & 31, kq = lane >> 5;
  const int C8 = a.C_in / 8;
  const unsigned zero_off = (unsigned)(((long long)a.B * C8 * a.T_in) * 16);          // the plane's trailing zero unit
  const unsigned grp_bytes = (unsigned)a.T_in * 16u;                                  // one 8-channel group of one clip
  const unsigned clip_off = flat ? 0u : (unsigned)((((long long)b * C8) * a.T_in) * 16);

  // ---- weights: wave w copies KiB w of each of the 3 K (plane, tap) blocks of a chunk
  const unsigned lds0 = __builtin_amdgcn_readfirstlane((unsigned)(size_t)(lds_void_t*)sm);
  const unsigned char* wsrc = reinterpret_cast<const unsigned char*>(a.w) + (long long)(rt64 >> 1) * n_chunks * PACK_CHUNK +
                              (rt64 & 1) * GP_BLK + wave * 1024 + lane * 16;
  auto issue_a = [&](int chunk, int buf) {
    const unsigned char* src = wsrc + (long long)chunk * PACK_CHUNK;
    const unsigned dst = lds0 + buf * STAGE + wave * 1024;
#pragma unroll
    for (int j = 0; j < NA; ++j) gp_dma16(src + j * (GP_PACK_ROWS * GP_RB), dst + j * GP_BLK);
  };

  // ---- inputs: byte offset inside a plane of this lane's column (+ tap) for channel group 0, or zero_off outside the signal
  unsigned coff[NBW][K];
#pragma unroll
  for (int n = 0; n < NBW; ++n)
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int r = wave * (32 * NBW) + n * 32 + l31 + k;     // row of the 128 x 128 form's staged window: column + tap
      unsigned off = zero_off;
      if (flat) {
        const long long nn = (long long)n0 + r;
        if (nn < n_total) {
          const long long bb = nn / a.T_out;
          off = (unsigned)(((bb * C8) * a.T_in + (nn - bb * a.T_out)) * 16);
        }
      } else if (S == 1) {
        const int tin = n0 - a.pad_left + r;
        if (tin >= 0 && tin < a.T_in) off = clip_off + (unsigned)tin * 16u;
      } else {
        off = (unsigned)r;                                    // strided: resolved per chunk (phase-dependent), see col_off
      }
      coff[n][k] = off;
    }
  auto col_off = [&](int n, int k, int ph) -> unsigned {
    if (S == 1) return coff[n][k];
    // column r of the window <-> sample (n0 + r) * S + phase - pad_left of the padded signal
    const int tin = (n0 + (int)coff[n][k]) * S + ph - a.pad_left;
    int idx;
    if (a.pad_mode == FAC_PAD_REFLECT) idx = reflect_index(tin, a.T_in, a.T_ext);
    else idx = (tin >= 0 && tin < a.T_in) ? tin : -1;
    return idx >= 0 ? clip_off + (unsigned)idx * 16u : zero_off;
  };
  const unsigned char* pl[3];
#pragma unroll
  for (int p = 0; p < 3; ++p) pl[p] = a.x_p8 + (long long)p * a.x_p8_ps;
  // the fragments of step `step` (tap step >> 1, K half step & 1) of chunk `chunk`: plain loads, counted by the compiler
  auto ld_b = [&](int chunk, int step, bf16x8 (&Bf)[NBW][3]) {
    const int k = step >> 1, ks = step & 1;
    const int c32 = chunk / S, ph = chunk - c32 * S;
    int g8 = c32 * 4 + ks * 2 + kq;
    g8 = g8 < C8 ? g8 : C8 - 1;                               // ragged last chunk: zero weights, any finite input will do
#pragma unroll
    for (int n = 0; n < NBW; ++n) {
      const unsigned off = col_off(n, k, ph);
      const unsigned goff = off == zero_off ? zero_off : off + (unsigned)g8 * grp_bytes;
#pragma unroll
      for (int p = 0; p < 3; ++p) Bf[n][p] = *(glb_bf16x8*)(pl[p] + goff);
    }
  };

  // ---- weight fragments from LDS: rows l31 (+ 32) of the workgroup's 64, slot (ks * 2 + kq) ^ ((row >> 2) & 3)
  const int swa = (l31 >> 2) & 3;
  int apo[2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) apo[ks] = l31 * GP_RB + (((ks * 2 + kq) ^ swa) * 16);
  auto ld_a = [&](const unsigned char* st, int step, bf16x8 (&A)[2][3]) {
    const int k = step >> 1, ks = step & 1;
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
      for (int m = 0; m < 2; ++m) A[m][p] = *reinterpret_cast<const bf16x8*>(st + (p * K + k) * GP_BLK + m * 32 * GP_RB + apo[ks]);
  };

  f32x16 acc[2][NBW];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < NBW; ++n)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[m][n][r] = 0.f;

  // prologue: weights of chunks 0 and 1 and the input fragments of the first GP_D steps in flight
  bf16x8 A[2][2][3], Bf[RING][NBW][3];
  issue_a(0, 0);
  if (n_chunks > 1) issue_a(1, 1);
#pragma unroll
  for (int s = 0; s < GP_D; ++s) ld_b(s / NSTEP, s % NSTEP, Bf[s]);       // GP_D <= NSTEP: chunk 0

  for (int base = 0; base < n_chunks; base += GP_NST) {
#pragma unroll
    for (int i = 0; i < GP_NST; ++i) {
      const int c = base + i;
      if (c >= n_chunks) break;
      {
        // This wave's share of chunk c's weights has landed: vector memory operations complete in order, and at least NA (when
        // chunk c + 1 was requested) + GP_D * LB younger ones were issued after it (the fragments of 2 * NSTEP >= GP_D steps).
        if (c + 1 < n_chunks) asm volatile("s_waitcnt vmcnt(%0)" : : "n"(NA + GP_D * LB) : "memory");
        else asm volatile("s_waitcnt vmcnt(%0)" : : "n"(GP_D * LB) : "memory");
        wg_barrier();                       // ... and every wave's; every wave has left chunk c - 1, whose stage chunk c + 2 takes
        if (c + 2 < n_chunks) issue_a(c + 2, (i + 2) % GP_NST);
        const unsigned char* st = sm + i * STAGE;
        ld_a(st, 0, A[0]);
#pragma unroll
        for (int step = 0; step < NSTEP; ++step) {
          const int gs = i * NSTEP + step;                      // static: GP_NST * NSTEP is a multiple of RING
          {
            // Request the fragments GP_D steps ahead.  Past the end the last chunk's are requested again and never used: a
            // conditional request would make the compiler wait for ALL requests where the two paths join (it merges their
            // counts pessimistically), and the ring would hide nothing.
            const int s2 = step + GP_D;
            const int c2 = c + s2 / NSTEP;
            ld_b(c2 < n_chunks ? c2 : n_chunks - 1, s2 % NSTEP, Bf[(gs + GP_D) % RING]);
          }
          if (step + 1 < NSTEP) ld_a(st, step + 1, A[(step + 1) & 1]);
          __builtin_amdgcn_sched_barrier(0);
          constexpr int TA[6] = {1, 2, 0, 1, 0, 0}, TB[6] = {1, 0, 2, 0, 1, 0};     // smallest terms first
#pragma unroll
          for (int q = 0; q < 6; ++q)
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
              for (int n = 0; n < NBW; ++n)
                acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[step & 1][m][TA[q]], Bf[gs % RING][n][TB[q]], acc[m][n], 0, 0, 0);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
    }
  }
  wg_barrier();      // every wave has left the last chunk; no DMA is in flight (the last chunk's wait left none behind)

  // accumulators -> fp32 tile in LDS
  {
    float* tile = reinterpret_cast<float*>(sm);
    constexpr int EP = COLS + 4;
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int n = 0; n < NBW; ++n)
#pragma unroll
        for (int r = 0; r < 16; ++r)
          tile[(m * 32 + (r & 3) + 8 * (r >> 2) + 4 * kq) * EP + wave * (32 * NBW) + n * 32 + l31] = acc[m][n][r];
  }
  __syncthreads();
  const float* tile = reinterpret_cast<const float*>(sm);
  switch (a.rp) {
    case 1: gp_epilogue<1, COLS>(a, tile, tid, rt64, n0, b, flat, n_total); break;
    case 2: gp_epilogue<2, COLS>(a, tile, tid, rt64, n0, b, flat, n_total); break;
    case 5: gp_epilogue<5, COLS>(a, tile, tid, rt64, n0, b, flat, n_total); break;
    case 6: gp_epilogue<6, COLS>(a, tile, tid, rt64, n0, b, flat, n_total); break;
    default: gp_epilogue<0, COLS>(a, tile, tid, rt64, n0, b, flat, n_total); break;
  }
}

// ---- host side

// Column blocks per tile for a launch of n_rt64 row tiles over `cols` columns in each of `nb` column ranges (clips, or 1 when
// flattened), on `slots` co-resident workgroups (2 per CU).  Cost of a form = rounds of `slots` workgroups x columns per tile: the
// padded columns of the last tile of a range and the idle slots of the last round both count.  Ties go to the wide tile (it reads
// the weights half as often).  1024 -> 4096 over 5120 columns on 512 slots: 64 x 256 is 1280 workgroups = 3 rounds x 256 = 768;
// 64 x 128 is 2560 = 5 rounds x 128 = 640.
int gp_choose_ncb(long long n_rt64, long long cols, long long nb, int slots) {
  long long cost[2];
  for (int i = 0; i < 2; ++i) {
    const int w = i == 0 ? 256 : 128;
    const long long n_wg = n_rt64 * ((cols + w - 1) / w) * nb;
    cost[i] = ((n_wg + slots - 1) / slots) * w;
  }
  return cost[1] < cost[0] ? 2 : 4;
}

static int gp_slots() {
  const int cus = device_cus();
  return 2 * (cus > 0 ? cus : 256);
}

// The launches that run on this form.  Every launch the split GEMM takes with a P8 input computes the same bits on either form;
// which shapes go here is a matter of measured speed only.
int conv_gsplit_p8_ncb(const ConvArgs& a) {
  if (a.x_p8 == nullptr || a.gs_cols_req < 0 || a.C_in % 8 != 0) return 0;
  if (a.gs_cols_req > 0) return a.gs_cols_req / 64;
  // The wired list: the shapes measured faster here than on the 128 x 128 form by more than twice the listing's spread.
  //   K = 1, the LSTM input projections (1024 -> 4096, 1536 -> 6144 over 5120 flattened columns): -19 %, -17 %;
  //   K = 2 over per-clip columns, the all-phases transposed convs 768 -> 384 (T 960) and 384 -> 192 (T 4800): -12 %, -19 %.
  // Measured slower, so they stay: the strided launches (+60 .. 75 %: a lane's units lie `stride` time steps apart, so a wave touches
  // 2.5 - 3 x the L2 sectors of its fragments) and the one flattened 2-tap signal (1536 -> 768, 87 MB of split weights: +4 .. 9 %).
  const bool lstm_proj = a.K == 1 && a.stride == 1 && a.rp == 1 && a.C_in >= 1024 && a.C_out >= 4096;
  const bool convtr_clips = a.K == 2 && a.stride == 1 && a.rp > 1 && a.B > 1 && a.C_in >= 384 && a.T_out >= 960;
  if (!lstm_proj && !convtr_clips) return 0;
  const bool flat = a.K == 1 && a.stride == 1;
  const int rows = a.rp > 1 ? a.C_out_pad : a.C_out;
  return gp_choose_ncb((rows + GP_ROWS - 1) / GP_ROWS, flat ? (long long)a.B * a.T_out : (long long)a.T_out, flat ? 1 : a.B, gp_slots());
}

template <int K, int NCB>
static int gp_launch(ConvArgs& a, hipStream_t s) {
  constexpr auto kern = conv1d_gemm_split_p8_kernel<K, NCB>;
  allow_dynamic_lds<kern>(80 * 1024);
  a.gflat = (K == 1) ? 1 : 0;
  const long long n_total = a.gflat ? (long long)a.B * a.T_out : (long long)a.T_out;
  a.n_t_tiles = (int)((n_total + 64 * NCB - 1) / (64 * NCB));
  const int rows = a.rp > 1 ? a.C_out_pad : a.C_out;
  const int n_rt = (rows + GP_ROWS - 1) / GP_ROWS;
  const long long n_wg = (long long)a.n_t_tiles * n_rt * (a.gflat ? 1 : a.B);
  {
    // order of the tiles inside an XCD's share, by the bytes that leave the L2s (the model of the 128 x 128 form, with 64
    // co-resident workgroups per XCD): row tile fastest unless re-reading the input per row tile is the cheaper side
    const double x_bytes = 6.0 * a.B * a.C_in * (double)a.T_in;
    const double w_bytes = 6.0 * rows * (double)a.C_in * K * (a.stride > 1 && K == 2 ? a.stride : 1);
    const double n_ct = (double)a.n_t_tiles * (a.gflat ? 1 : a.B);
    const double g = 64.0 / n_rt > 1.0 ? 64.0 / n_rt : 1.0;
    const double slow = x_bytes * n_rt + w_bytes;
    const double fast = x_bytes + (w_bytes <= 3.5 * 1048576.0 ? 8.0 * w_bytes : w_bytes * n_ct / g);
    a.grt = (n_rt > 1 && fast < 0.8 * slow) ? n_rt : 0;
  }
  if (n_wg > 0x7fffffffll) {
    set_error("conv1d(gemm split, P8 fragments): too many workgroups (%lld)", n_wg);
    return FAC_ERR_ARG;
  }
  hipLaunchKernelGGL(kern, dim3((unsigned)n_wg), dim3(256), gp_lds_bytes(K, NCB), s, a);
  return check_launch("conv1d_gemm_split_p8");
}

int conv_dispatch_gsplit_p8(ConvArgs& a, hipStream_t s) {
  const bool k1 = a.K == 1 && a.stride == 1;
  if (a.gs_ncb == 4) return k1 ? gp_launch<1, 4>(a, s) : gp_launch<2, 4>(a, s);
  if (a.gs_ncb == 2) return k1 ? gp_launch<1, 2>(a, s) : gp_launch<2, 2>(a, s);
  set_error("conv1d(gemm split, P8 fragments): no form with %d column blocks", a.gs_ncb);
  return FAC_ERR_ARG;
}

}  // namespace fac

extern "C" int fac_gsplit_p8_tile_cols(int64_t rows, int64_t cols, int64_t ranges, int slots) {
  if (rows <= 0 || cols <= 0 || ranges <= 0 || slots <= 0) return 0;
  return 64 * fac::gp_choose_ncb((rows + fac::GP_ROWS - 1) / fac::GP_ROWS, cols, ranges, slots);
}
