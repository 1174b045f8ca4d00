// Operand packing: pack_many_kernel (every packed operand of several layers, and the step's other housekeeping, in one launch),
// the description of each conv operand as a job of it, and the whole-network entry point fgc_conv_pack.
#include "fgc_conv_bwd.h"
#include "fgc_conv_narrow.h"
#include "fgc_conv_pair.h"
#include "fgc_mlp.h"

namespace fgc {

__global__ __launch_bounds__(256) void pack_many_kernel(PackJobs J) {
    int q = 0;
#pragma unroll
    for (int t = 1; t < PACK_MAX_JOBS; ++t)
        if (t < J.njobs && (int)blockIdx.x >= J.job[t].block0) q = t;
    const PackJob& j = J.job[q];
    const int bid = blockIdx.x - j.block0;
    const int nb = (q + 1 < J.njobs ? J.job[q + 1].block0 : J.nblocks) - j.block0;
    if (j.kind >= PACK_ROTATE) {
        if (j.kind == PACK_ROTATE_LOGITS) rotate_logits_body(j.W0, j.dst, j.kdim, j.cin, j.aux, j.lg_u, j.lg_c, j.lg_v, j.lg_ag, bid, nb);
        else if (j.kind == PACK_ROTATE) rotate_rows_body(j.W0, j.dst, j.kdim, j.aux, bid, nb);
        else if (j.kind == PACK_MLP) mlp_pack_body(j.W0, j.dst, j.cin, j.kdim, j.ncols, bid, nb);
        else if (j.kind == PACK_MLP_SPLIT) mlp_pack_split_body(j.W0, (unsigned short*)j.dst, j.cin, j.ncols, bid, nb);
        else if (j.kind == PACK_MLP_BF16) mlp_pack_bf16_body(j.W0, (unsigned short*)j.dst, j.cin, j.ncols, bid, nb);
        else if (j.kind == PACK_MLP_W1DX_BF16) mlp_pack_w1dx_bf16_body(j.W0, (unsigned short*)j.dst, j.cin, j.ncols, bid, nb);
        else if (j.kind == PACK_MLP_W1DX_SPLIT) mlp_pack_w1dx_split_body(j.W0, (unsigned short*)j.dst, j.cin, j.ncols, bid, nb);
        else if (j.kind == PACK_MLP_W2_SPLIT) mlp_pack_w2_split_body(j.W0, (u32x4*)j.dst, j.ncols, j.cout, bid);
        else if (j.kind == PACK_LOGIT_SPLIT) pack_logit_weight_split_body(j.W0, (unsigned short*)j.dst, j.cin, j.cout, j.passes, bid, nb);
        else mlp_pack_w2_bf16_body(j.W0, (u32x4*)j.dst, j.ncols, j.cout, bid);
    } else if (j.kind == PACK_PLAIN_BF16) pack_plain_bf16_body(j.W0, (unsigned short*)j.dst, j.kdim, bid, nb);
    else if (j.kind == PACK_LOGIT_BF16) pack_logit_weight_bf16_body(j.W0, (unsigned short*)j.dst, j.cin, j.cout, j.passes, bid, nb);
    else if (j.kind >= PACK_FWD_BF16) pack_weight_bf16_body(j.W0, (unsigned short*)j.dst, j.cin, j.cout, j.kdim, j.ncols, j.npad, j.passes,
                                                j.kind - PACK_FWD_BF16, bid, nb);
    else if (j.kind == PACK_LOGIT) pack_logit_weight_body(j.W0, j.dst, j.cin, j.cout, j.opad, j.kc, j.kpass, j.passes, bid, nb);
    else pack_weight_body(j.W0, j.dst, j.cin, j.cout, j.kdim, j.ncols, j.npad, j.kc, j.kpass, j.passes, j.kind, bid, nb);
}

void PackBatch::add(const PackJob& j, size_t total) {
    if (J.njobs == PACK_MAX_JOBS) flush();
    PackJob& q = J.job[J.njobs++];
    q = j;
    q.block0 = J.nblocks;
    J.nblocks += cdiv((int)total, 1024);
}
void PackBatch::flush() {
    if (J.njobs == 0) return;
    FGC_LAUNCH("pack_many_kernel", st, pack_many_kernel, dim3(J.nblocks), dim3(256), 0, J);
    J.njobs = J.nblocks = 0;
}

int launch_pack_jobs(const PackJob* jobs, const size_t* totals, int n, const char* what, hipStream_t st) {
    PackBatch batch(st);
    for (int k = 0; k < n; ++k) batch.add(jobs[k], totals[k]);
    batch.flush();
    FGC_CHECK_LAUNCH(what);
    return FGC_OK;
}

// forward: the k-interleaved (fp32) or fragment-ordered (bf16) B operand of the aggregate-first GEMM; the pair form reads W0 in
// place (bf16 storage: a bf16 copy of it); a narrow first layer packs nothing
int conv_fwd_pack_jobs(const fgc_conv_desc* d, void* fwd_ws, PackJob* jobs, size_t* totals) {
    const int cin = d->c0 + d->c1, cout = d->cout;
    const bool bf16 = (d->flags & FGC_CONV_BF16) != 0;
    if (pairs_ok(d)) {
        if (!bf16) return 0;
        totals[0] = (size_t)FGC_M * cout * cin;
        jobs[0] = PackJob{d->W0, (float*)fwd_ws, PACK_PLAIN_BF16, cin, cout, (int)totals[0], 0, 0, 0, 0, 0, 0, 0};
        return 1;
    }
    if (narrow_supported(d)) return 0;
    const ConvGeom g = conv_geom(cin, cout);
    totals[0] = (size_t)g.passes * g.kpass * g.npad;
    jobs[0] = PackJob{d->W0, (float*)fwd_ws, bf16 ? PACK_FWD_BF16 : PACK_FWD, cin, cout, cin, cout, g.npad, g.kc, g.kpass, g.passes, 0, 0};
    return 1;
}

// backward: the d-logits operand Wq (none in the pair form) and the data-gradient operand Wpt, in the layouts the plan chose
int conv_bwd_pack_jobs(const fgc_conv_desc* d, const BwdPlan& w, PackJob* jobs, size_t* totals) {
    const int cin = d->c0 + d->c1, cout = d->cout;
    int n = 0;
    if (w.wq.count) {
        totals[n] = w.wq.count;
        jobs[n++] = PackJob{d->W0, w.Wq, w.wq.kind, cin, cout, 0, 0, 0, w.g1.kc, w.g1.kpass, w.g1.passes, w.opad, 0};
    }
    totals[n] = w.wpt.count;
    jobs[n++] = PackJob{d->W0, w.Wpt, w.wpt.kind, cin, cout, cout, cin, w.g2.npad, w.g2.kc, w.g2.kpass, w.g2.passes, 0, 0};
    return n;
}

}  // namespace fgc

using namespace fgc;

// ---------------------------------------------------------------------------------------------
// whole-network helpers: one launch where every layer used to bring its own
// ---------------------------------------------------------------------------------------------
extern "C" int fgc_conv_pack(const fgc_conv_desc* const* descs, const fgc_conv_bwd_io* const* ios, void* const* fwd_ws,
                             void* const* bwd_ws, int32_t count, const fgc_pack_extra* extra, void* stream) {
    FGC_CHECK_ARG((descs || count == 0) && count >= 0, "fgc_conv_pack: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    PackBatch batch(st);
    PackJob jobs[2];
    size_t totals[2];
    for (int i = 0; i < count; ++i) {
        const fgc_conv_desc* d = descs[i];
        FGC_OPT_SCOPE(d);      // (this layer's own option values, if its descriptor carries any)
        int rc = validate_conv_desc(d, "fgc_conv_pack");
        if (rc) return rc;
        if (fwd_ws && fwd_ws[i]) {
            FGC_CHECK_ARG((uintptr_t)fwd_ws[i] % 16 == 0 || narrow_supported(d) || pairs_ok(d), "fgc_conv_pack: workspace %d misaligned", i);
            const int nf = conv_fwd_pack_jobs(d, fwd_ws[i], jobs, totals);
            for (int k = 0; k < nf; ++k) batch.add(jobs[k], totals[k]);
        }
        const bool narrow_bwd = ios && ios[i] && ios[i]->dx0 == nullptr && narrow_supported(d);   // vector-ALU path: nothing to pack
        if (bwd_ws && bwd_ws[i] && !narrow_bwd) {
            FGC_CHECK_ARG((uintptr_t)bwd_ws[i] % 16 == 0, "fgc_conv_pack: workspace %d misaligned", i);
            const int nbw = conv_bwd_pack_jobs(d, plan_bwd(d, (char*)bwd_ws[i]), jobs, totals);
            for (int k = 0; k < nbw; ++k) batch.add(jobs[k], totals[k]);
        }
    }
    if (extra && extra->rot_x) {
        const int64_t nvec = (int64_t)extra->rot_rows * extra->rot_vecs;
        FGC_CHECK_ARG(extra->rot_y && extra->rot_R && extra->rot_rows > 0 && extra->rot_vecs > 0 && nvec < (1ll << 31),
                      "fgc_conv_pack: extra: bad rotation (rows=%lld vecs=%d)", (long long)extra->rot_rows, extra->rot_vecs);
        if (extra->rot_ag) {
            FGC_CHECK_ARG(extra->rot_u && extra->rot_c && extra->rot_v && extra->rot_vecs <= 2 && (uintptr_t)extra->rot_ag % 16 == 0,
                          "fgc_conv_pack: extra: the first layer's logit table needs u, c, v and at most 6 input channels");
            PackJob j{extra->rot_x, extra->rot_y, PACK_ROTATE_LOGITS, extra->rot_vecs, 0, (int)extra->rot_rows, 0, 0, 0, 0, 0, 0, 0, extra->rot_R,
                      extra->rot_u, extra->rot_c, extra->rot_v, extra->rot_ag};
            batch.add(j, (size_t)extra->rot_rows * 4);     // one row per thread
        } else {
            PackJob j{extra->rot_x, extra->rot_y, PACK_ROTATE, 0, 0, (int)nvec, 0, 0, 0, 0, 0, 0, 0, extra->rot_R};
            batch.add(j, (size_t)nvec * 2);     // two 3-vectors per thread-iteration share
        }
    }
    if (extra && extra->mlp_W1) {
        PackJob mj[4];
        size_t tot[4];
        const int nj = mlp_pack_jobs(extra, mj, tot);
        FGC_CHECK_ARG(nj >= 0, "fgc_conv_pack: extra: MLP shape cin=%d hidden=%d cout=%d n=%d not served%s", extra->mlp_cin,
                      extra->mlp_hidden, extra->mlp_cout, extra->mlp_n, extra->mlp_bf16 ? " (bf16)" : "");
        for (int i = 0; i < nj; ++i) batch.add(mj[i], tot[i]);
    }
    batch.flush();
    FGC_CHECK_LAUNCH("fgc_conv_pack");
    return FGC_OK;
}

