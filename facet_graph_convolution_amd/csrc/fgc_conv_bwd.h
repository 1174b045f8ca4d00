// The backward plan of one graph-convolution layer: everything that follows from (descriptor, options) - kernel form, partial-sum
// slots, packed operands, workspace layout - decided in ONE place (plan_bwd, fgc_conv_bwd.hip) and read by everything else.
#pragma once
#include "fgc_conv_w8.h"
#include "fgc_pack.h"

namespace fgc {

// which kernel computes the d-logits of the layer (K1 of fgc_conv_bwd.hip)
enum K1Form {
    K1_PAIR,     // pair graph given: pair_bwd_logits_kernel (fgc_conv_pair.hip)
    K1_NARROW,   // first layer, no input gradient wanted (io->dx0 == NULL): fgc_conv_narrow.hip; chosen per call (bwd_call)
    K1_BF16,     // conv_bwd_logits_bf16_kernel
    K1_DEEP,     // conv_bwd_logits_deep_kernel
    K1_MFMA,     // conv_bwd_logits_mfma_kernel
    K1_VALU      // conv_bwd_logits_kernel
};
struct PackedOperand {
    int kind;        // PackKind
    size_t count;    // elements the pack writes (a workgroup of pack_many_kernel takes 1024)
};

struct BwdPlan {
    bool pairs, narrow, bf16;   // pair form / a narrow first layer (cin <= 8) / FGC_CONV_BF16 storage
    ConvGeom g1, g2;            // K1 gathers x (cin wide); K2 gathers s (cout wide), GEMM N = cin
    int opad;                   // cout rounded up to 16
    K1Form k1;                  // of the tiled path (a narrow layer takes K1_NARROW per call)
    bool deep_ok;               // shape and options admit the deep-gather kernels (K1_DEEP; K1_BF16 needs it)
    bool k1_long, k1_half, k1_split;   // 17..24 edge slots / 16-node workgroups / dz GEMM on split bf16 operands
    bool fusable;               // the kernel form has the s = dy lrelu'(y) / deg prologue for this width (fuse_ds, given alignment)
    int k1_nodes;               // nodes per d-logits workgroup: the unit of the db and dc partial slots
    int n_dc;                   // dc partials
    int nb_db, rows_per_db;     // db partials, rows per partial of ds_db_kernel
    int nred, splitW;           // rows and slabs of the weight-gradient GEMM
    PackedOperand wq, wpt;      // what Wq / Wpt hold (wq.count == 0: the pair form has no d-logits operand)
    float* Wq;        // logits operand
    float* Wpt;       // data-gradient operand
    float* db_part;   // [nb_db][cout]
    float* dc_part;   // [n_dc][12]
    float* slab;      // gemm_tn partials of [dW0; du; dv]
    float* rtmp;      // scratch of the fixed-order reductions
    float* narrow_ws; // first-layer path (cin <= 8): z buffer, partial slabs (fgc_conv_narrow.hip); NULL unless `narrow`
    size_t bytes;
};
// base == NULL: sizes only.  Reads the options in force (call it inside the descriptor's FGC_OPT_SCOPE).
BwdPlan plan_bwd(const fgc_conv_desc* d, char* base);

// the packed backward operands of a layer as pack_many_kernel jobs (fgc_conv_pack.hip): returns the number of jobs written (<= 2)
int conv_bwd_pack_jobs(const fgc_conv_desc* d, const BwdPlan& w, PackJob* jobs, size_t* totals);

}  // namespace fgc
