// Weight-gradient GEMMs C[P, Q] = A^T X over the rows of a layer (fgc_gemm_tn.hip): job descriptions and host entry points.
#pragma once
#include "fgc_common.h"

namespace fgc {

// The weight-gradient GEMMs of several layers in ONE launch (fgc_conv_bwd_reduce with FGC_CONV_DEFER_DW): every job is what
// one launch of the kernel would be - same tiles, same slabs, same sums, bit-identical gradients -, its workgroups are the
// range [block0, block0 + tn_grid) of the grid.  On the bf16 network a layer's GEMM is 5-15 us of ramp and tail around a few
// microseconds of streaming: eight of them back to back cost four times what their work takes.
struct TnArgs {
    const void* A;
    const void* x0;
    const void* x1;
    float* slab;
    int lda, P, c0, c1, shift, rows, rps;
    int block0;
};
constexpr int TN_MAX_JOBS = 8;
struct TnJobs {
    TnArgs job[TN_MAX_JOBS];
    int njobs;
};
constexpr int TNB_PC = 320;   // columns of A per workgroup of the bf16 kernel

// ---- which kernel computes a layer's weight gradient, and with what arguments: shared by the per-layer launch (stage 8) and
// ---- the grouped launch of fgc_conv_bwd_reduce (FGC_CONV_DEFER_DW)
enum TnVariant { TN_STREAM2 = 0, TN_STREAM4, TN_STREAM2_BF, TN_STREAM4_BF, TN_BF16_4, TN_BF16_2, TN_PLAIN_V4, TN_PLAIN, TN_NVARIANTS };
struct TnPlan {
    int variant;
    TnArgs a;
    int ntiles, nsplits;
};
static inline bool tn_groupable(int v) { return v <= TN_BF16_2; }
static inline dim3 tn_grid(int ntiles, int nsplits) { return dim3((unsigned)(ntiles * 8 * cdiv(nsplits, 8))); }
// rows x [PL columns of A] against [c0 + c1 columns of x0 | x1]; lda: row stride of A (0 = PL)
TnPlan tn_plan_of(bool bf16, bool vec4, bool stream_ok, const void* A, int PL, const void* x0, const void* x1, int c0, int c1,
                  int shift, int rows, int rps, float* slab, int lda = 0);
int tn_launch_one(const TnPlan& pl, const char* tag, hipStream_t st);
int tn_launch_group(int variant, TnJobs& J, int nblocks, const char* tag, hipStream_t st);   // empties J

bool tn_bf16_ok(int P, int c0, int c1);
int tn_rows_per_slab(int n, int splits);
int tn_splits(int P, int Q, int rows);                     // slab count of a layer's GEMM from the TN_SLOTS option
int tn_balanced_splits(int desired, int maxs, int rows);   // ... near `desired`, XCD-balanced
// streaming TN GEMM: slab[split][P][c0] = A[rows of the split, P]^T x0[rows of the split, c0]
int launch_gemm_tn_stream(const char* tag, const float* A, int lda, int P, const float* x0, int c0, int rows,
                          int rows_per_split, int nsplits, float* slab, hipStream_t st);

}  // namespace fgc
