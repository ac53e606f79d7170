// The 96-row form of the k = 7 split-bf16 kernel (conv1d_bsplit_kernel.h, design notes in conv1d_bsplit.hip): tile 96 x 256, 4 MFMA
// waves of 96 x 64 (3 x 2 MFMA blocks, 36 MFMAs per step on 9 weight + 6 input fragments) + 4 staging waves.  The decoder's channel
// counts (768 / 384 / 192 / 96) are multiples of 96: no padded rows at C = 96, and every staged input column feeds 1.5 x the matrix
// work of the 64-row tile.
// LDS: a G = 2 weight stage at 96 rows is 3 planes x 14 half slots x 96 co x 16 B = 63 KiB, two full stages 184 KiB -- more than a
// CU has.  So the stage is G = 1: 8 input channels x (7 taps + one zero tap) = 8 half slots, 4 MFMA steps of tap pairs:
//   weights 3 x 8 x 96 x 16 B = 36 KiB, inputs 3 x (256 + 7 d) x 16 B <= 15 KiB, two stages <= 102 KiB; with the tile walk the
//   epilogue's 96 x 260 fp32 tile (97.5 KiB) replaces stage 1: 148.5 KiB.
// Weights: fac_pack_conv_w_split_rows(rows = 96): [co tile of 96][stage][plane][half slot][96 co][8 ci].
// Its own translation unit: the kernel names the landing registers of inflight_regs.h, and tools/check_inflight_regs.py counts
// such kernels per file.
#include "conv1d_bsplit_kernel.h"

namespace fac {

bool conv_bsplit96_ok(const ConvArgs& a) {
  if (!(a.K == 7 && a.stride == 1 && a.n_phase == 1 && a.phase_shift == 0 && a.y_tstride == 1 && !a.alpha_in && !a.w1 && !a.w_batched &&
        (long long)a.B * a.T_out > 640))
    return false;
  // full co tiles only; 8-channel stages; the staged columns (the zero tap's included) fit the staging waves' units
  return a.C_out % BS96_CO == 0 && a.C_in % 8 == 0 && (256 + 7 * a.dil + 63) / 64 <= BS_NSW * BS_XU &&
         a.x_cs * (long long)a.C_in < (1ll << 31);
}

bool conv_bsplit96_p8_ok(const ConvArgs& a) { return conv_bsplit96_ok(a) && (long long)a.T_in * 16 < (1ll << 32); }

int conv_dispatch_bsplit96(ConvArgs& a, hipStream_t s) { return bsplit_launch<7, 1, 4, BS_NSW_WIDE, 3>(a, s); }

}  // namespace fac
