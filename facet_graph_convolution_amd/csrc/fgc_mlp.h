// The per-facet MLP head cin -> hidden -> cout on the host: everything that follows from (shape, storage type, options, pointer
// alignment) - kernel form, template selectors, grids, dynamic LDS, packed operands, workspace layout - decided in ONE place
// (plan_mlp_fwd / plan_mlp_bwd, fgc_mlp.hip) and read by everything else: the size queries, fgc_mlp_layout_id, the MLP jobs of
// fgc_conv_pack, the four entry points and the launch functions of the three kernel families.
#pragma once
#include "fgc_pack.h"
#include "fgc_reduce.h"

namespace fgc {

// tile geometry of the fp32-MFMA kernels (fgc_mlp_f32.hip); the other two families: fgc_mlp_mb.h
#ifndef FGC_MLP_T
#define FGC_MLP_T 64
#endif
#ifndef FGC_MLP_BWD_T
#define FGC_MLP_BWD_T 32
#endif
constexpr int MLP_T = FGC_MLP_T;       // rows per forward tile, every form (fgc_mlp_num_partials counts these)
constexpr int MLP_RT = MLP_T / 16;
constexpr int BWD_T = FGC_MLP_BWD_T;   // rows per backward tile, every form
constexpr int BWD_RT = BWD_T / 16;
constexpr int MLP_COUT_MAX = 4;
constexpr int MLP_THREADS = 256;
// LDS row strides (floats).  ds_read_b32 / ds_write_b32 bank = dword % 32 within a 32-lane half, ds_read_b128 bank =
// dword % 64 within a 16-lane group: a stride == 4 mod 8 keeps both the row-per-lane b128 reads (16 rows -> 16
// distinct 16-byte slots) and the 4-rows-apart b32 accesses of lanes l, l+16 (4 * stride == 16 mod 32) conflict free.
constexpr int MLP_XPAD = 4;    // x tile rows: kpad + 4
constexpr int MLP_DHS = 20;    // transposed dh rows

enum MlpForm {
    MLP_F32,     // fp32 MFMA: mlp_fwd_kernel / mlp_bwd_kernel (fgc_mlp_f32.hip)
    MLP_SPLIT,   // fp32 storage, three-term bf16 operand splits on the bf16 matrix pipe (fgc_mlp_split.hip)
    MLP_BF16     // bf16-stored activations (fgc_mlp_bf16.hip)
};
struct MlpShape {
    int n, cin, hidden, cout;
    bool bf16;   // storage type of x / dx
};
// one packed operand: pack_many_kernel job `kind` writes `count` elements (a workgroup takes 1024) at byte `off` of the workspace
struct MlpOperand {
    int kind;        // PackKind; the W2 kinds read W2, every other W1
    size_t count;
    size_t off;
};

struct MlpFwdPlan {
    bool ok;             // the shape has a kernel
    MlpForm form;        // ... chosen with the alignment given,
    MlpForm shape_form;  // ... and by the shape alone: what fgc_conv_pack leaves in the workspace
    int ks;              // template selector: KG of mlp_fwd_kernel (0: generic), KS = cin / 32 of the other two
    int co;              // output columns carried in registers (3 or 4)
    int kpad;            // fp32 MFMA: input channels padded to the k group
    int gx;              // workgroups
    size_t smem;         // dynamic LDS bytes
    MlpOperand w1;       // the W1 operand, at the start of the workspace
    size_t bytes;
};
// workspace: [W1 operand][W1 in dx order | dx slabs][dW1 slabs][db1 slabs][dW2 slabs][db2 partials][W2 operand][reduce scratch]
//   (fp32 MFMA: dx slabs, no W2 operand; the other two forms: W1 in dx order, dx leaves its kernel complete)
struct MlpBwdPlan {
    bool ok;
    MlpForm form, shape_form;
    int mt, ctw, co;     // template selectors: MT = input-channel tiles of 16, CTW (fp32 MFMA: column tiles per wave), CO
    int kpad;            // fp32 MFMA: the kernel's k extent 16 * MT
    int slabs;           // parameter-gradient slabs (= row walkers)
    int dx_slabs;        // fp32 MFMA: dx slabs (= hidden slices); else 0
    int dx_gx;           // workgroups of the dx kernel (0: fp32 MFMA, one fused kernel)
    int gx, gy;          // grid of the parameter-gradient kernel (fp32 MFMA: of the fused kernel)
    size_t smem;         // dynamic LDS bytes of that kernel
    size_t wp, w1d, dW1, db1, dW2, db2, w2p, rtmp, bytes;   // byte offsets (w1d: W1 in dx order, or the dx slabs) and the total
    MlpOperand op[3];
    int nops;
};
// aligned: the 16-byte alignment the matrix-pipe forms need holds (fwd: x; bwd: x, dx, b1; every form needs it of the
// workspace, which the entry points check themselves).  The default plans for the shape alone.  Reads the options in force.
MlpFwdPlan plan_mlp_fwd(const MlpShape& s, bool aligned = true);
MlpBwdPlan plan_mlp_bwd(const MlpShape& s, bool aligned = true);

// the jobs that leave an MLP's operands in mlp_fwd_ws / mlp_bwd_ws as the plans lay them out; `totals[i]` = elements of job i.
// Returns the number of jobs written (<= 4), or -1 for a shape the entry points refuse.
int mlp_pack_jobs(const fgc_pack_extra* e, PackJob* jobs, size_t* totals);

struct MlpFwdArgs {
    const void* x;       // fp32 or bf16 rows
    const float *W1, *b1, *W2, *b2;
    float alpha;
    float *y, *abs_partial;
    char* ws;
};
struct MlpBwdArgs {
    const void* x;
    const float *dy, *W1, *b1, *W2;
    float alpha;
    void* dx;
    char* ws;            // slabs and operands at the plan's offsets
};
// the kernels of one family for a plan of that form (fgc_mlp_f32.hip, fgc_mlp_split.hip, fgc_mlp_bf16.hip)
int launch_mlp_fwd_f32(const MlpShape& s, const MlpFwdPlan& p, const MlpFwdArgs& a, hipStream_t st);
int launch_mlp_bwd_f32(const MlpShape& s, const MlpBwdPlan& p, const MlpBwdArgs& a, hipStream_t st);
int launch_mlp_fwd_split(const MlpShape& s, const MlpFwdPlan& p, const MlpFwdArgs& a, hipStream_t st);
int launch_mlp_bwd_split(const MlpShape& s, const MlpBwdPlan& p, const MlpBwdArgs& a, hipStream_t st);
int launch_mlp_fwd_bf16(const MlpShape& s, const MlpFwdPlan& p, const MlpFwdArgs& a, hipStream_t st);
int launch_mlp_bwd_bf16(const MlpShape& s, const MlpBwdPlan& p, const MlpBwdArgs& a, hipStream_t st);

}  // namespace fgc
