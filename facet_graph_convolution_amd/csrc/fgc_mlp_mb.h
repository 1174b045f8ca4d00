// What the two kernel families of the MLP head that run on the bf16 matrix pipe share (fgc_mlp_bf16.hip: bf16-stored
// activations; fgc_mlp_split.hip: fp32 activations as three-term bf16 operand splits): tile constants, the walker count and
// the dynamic-LDS sizes the plan (fgc_mlp.h) hands to the launches.  (The two forward kernels are the same walk on one
// fragment plane and on three; written as one inlined body they compile to other instruction streams - DESIGN.md section
// 3.8 - so each file keeps its own.)
//
// Fragment layouts of v_mfma_f32_16x16x32_bf16 (MI355X guide): lane l = (lr = l & 15, lq = l >> 4) holds
//   A[row lr][k = 8*lq + j],  B[k = 8*lq + j][col lr],  j = 0..7  (16 bytes each);  C/D: col = lr, row = 4*lq + reg.
#pragma once
#include "fgc_common.h"

namespace fgc {

constexpr int MB_THREADS = 256;
constexpr int MB_FWD_T = 64;       // rows per forward tile (as the fp32-MFMA kernel: fgc_mlp_num_partials counts these)
constexpr int MB_FWD_RT = MB_FWD_T / 16;
constexpr int MB_T = 32;           // rows per backward tile
constexpr int MB_RT = MB_T / 16;
constexpr int MBB_THREADS = 256;
constexpr int MBB_WAVES = MBB_THREADS / 64;
constexpr int MBW_HCW = 64;               // hidden columns per wave of the parameter-gradient kernel
constexpr int MBW_CT = MBW_HCW / 16;

// row walkers of the parameter-gradient kernels (bf16: waves, split: workgroups): each keeps its partial sums in registers and
// writes one slab
static inline int mb_gx(int n) {
    const int ntiles = cdiv(n, MB_T);
    const int wg = cdiv(ntiles, 4);
    return (wg < 32 ? wg : 32) * 4;
}
// dynamic LDS of mlp_bwd_w_bf16_kernel: per wave a transposed x tile [cin][MB_T bf16 + 8 bytes] and the tile's dy [MB_T][4]
static inline size_t mb_w_lds(int cin) { return (size_t)MBB_WAVES * ((size_t)cin * (MB_T * 2 + 8) + MB_T * 16); }
// ... of mlp_bwd_w_split_kernel (x tile: row = [plane 0 | plane 1 | plane 2 | 32 pad bytes], so that two workgroups of four
// waves fit a CU's 160 KB): 2 x { x [32 rows][3 planes | pad] bf16, dy [32][4] fp32, dy operand [32][3 lane groups] }
#define MBS_XTS(CIN_) (3 * (CIN_) * 2 + 32)
#define MBS_TILE_LDS(CIN_) (MB_T * MBS_XTS(CIN_) + MB_T * 16 + MB_T * 48)
#define MBS_WG_LDS(CIN_) (2 * MBS_TILE_LDS(CIN_))

}  // namespace fgc
