// Per-facet MLP cin -> hidden -> cout (replaces lrelu(custom_lin(x,1024)) -> custom_lin(.,3), model.py:763-769,937-941 of the
// reference) on the host: the plan (fgc_mlp.h), the pack jobs of its operands and the extern "C" entry points.  The kernels
// and their launch functions: fgc_mlp_f32.hip (fp32 MFMA), fgc_mlp_split.hip (fp32 through split bf16 operands),
// fgc_mlp_bf16.hip (bf16-stored activations).
#include <algorithm>
#include <cstdio>
#include <cstring>

#include "fgc_mlp.h"
#include "fgc_mlp_mb.h"

namespace fgc {

// ---- the plan -----------------------------------------------------------------------------------------------------------------
static bool mlp_f32_shape_ok(const MlpShape& s, int hidden_mult) {
    return s.cin > 0 && s.cin <= 128 && s.hidden > 0 && s.hidden % hidden_mult == 0 && s.cout > 0 && s.cout <= MLP_COUT_MAX;
}
static bool mlp_bf16_shape_ok(const MlpShape& s) {
    return (s.cin == 32 || s.cin == 64 || s.cin == 128) && s.hidden > 0 && s.hidden % 256 == 0 && s.cout > 0 && s.cout <= MLP_COUT_MAX;
}
// The form the shape and the options select.  The two 1024-wide products of the forward pass, and every one of the backward
// pass, run on the bf16 matrix pipe with three-term operand splits where the shape allows: fp32-equivalent results, the matrix
// time a sixth of the fp32 MFMA's.
static MlpForm fwd_shape_form(const MlpShape& s) {
    if (s.bf16) return MLP_BF16;
    return opt(OPT_NO_MLP_SPLIT) != 1 && (s.cin == 32 || s.cin == 64) && s.hidden % 256 == 0 && s.cout <= 4 ? MLP_SPLIT : MLP_F32;
}
static MlpForm bwd_shape_form(const MlpShape& s) {
    if (s.bf16) return MLP_BF16;
    return opt(OPT_NO_MLP_SPLIT) != 1 && opt(OPT_NO_MLP_BWD_SPLIT) != 1 && s.cin == 32 && s.hidden % 256 == 0 && s.cout <= 3 ? MLP_SPLIT
                                                                                                                          : MLP_F32;
}

static MlpFwdPlan fwd_layout(const MlpShape& s, MlpForm form) {
    MlpFwdPlan p{};
    p.form = p.shape_form = form;
    p.co = s.cout <= 3 ? 3 : 4;
    p.gx = cdiv(s.n, MLP_T);
    const size_t wide = (size_t)s.cin * s.hidden;
    if (form == MLP_F32) {
        p.ok = mlp_f32_shape_ok(s, 64);
        p.kpad = (s.cin + 15) / 16 * 16;
        p.ks = p.kpad == 16 ? 1 : (p.kpad == 32 ? 2 : 0);   // the next column tile's weight fragments prefetched (narrow inputs)
        p.smem = (size_t)(MLP_T * (p.kpad + MLP_XPAD) + 4 * MLP_T * 4 + 4) * 4;   // x tile, [4 waves][MLP_T][4] partial y, 4 sums
        p.w1 = MlpOperand{PACK_MLP, (size_t)p.kpad * s.hidden, 0};
        p.bytes = align_up(p.w1.count * sizeof(float), 256);
    } else {
        p.ok = form == MLP_BF16 ? mlp_bf16_shape_ok(s) : mlp_f32_shape_ok(s, 256);
        p.ks = s.cin / 32;
        p.w1 = MlpOperand{form == MLP_BF16 ? PACK_MLP_BF16 : PACK_MLP_SPLIT, wide, 0};
        p.bytes = align_up((form == MLP_BF16 ? 1 : 3) * wide * 2, 256);
    }
    return p;
}

static MlpBwdPlan bwd_layout(const MlpShape& s, MlpForm form) {
    MlpBwdPlan p{};
    p.form = p.shape_form = form;
    const size_t n = s.n, cin = s.cin, hidden = s.hidden, wide = cin * hidden;
    size_t w1_bytes, second_bytes, w2_bytes;
    if (form == MLP_F32) {
        // <MT, CTW> = <2,4> serves the 32-wide head of the network; <4,2> and <8,1> the 64/128-wide multi-scale heads
        // (model.py:894-899, 915-920), trading column width for the wider dx / dW1 accumulators.  The kernel's k extent is its
        // template width 16 * MT: narrower inputs are zero padded up to it.
        p.ok = mlp_f32_shape_ok(s, 256);
        p.ctw = s.cin <= 32 ? 4 : (s.cin <= 64 ? 2 : 1);
        p.mt = 8 / p.ctw;
        p.kpad = 16 * p.mt;
        p.co = s.cout <= 3 ? 3 : 4;
        const int ntiles = cdiv(s.n, BWD_T), hcw = 64 * p.ctw;
        p.slabs = p.gx = ntiles < 128 ? ntiles : 128;
        p.dx_slabs = p.gy = s.hidden / hcw;
        // x, dy, transposed dh per wave, dx partials (one tile per wave when MT <= 2), the workgroup's weight slice
        // [kpad/4][hcw+1][4], b1 [hcw], W2 [hcw][4]
        p.smem = (size_t)(BWD_T * (p.kpad + MLP_XPAD) + BWD_T * 4 + 4 * BWD_T * MLP_DHS + (p.ctw == 4 ? 4 : 1) * BWD_T * (p.kpad + MLP_XPAD) +
                          4 + (p.kpad / 4) * (hcw + 1) * 4 + hcw * 5) * 4;
        p.op[p.nops++] = MlpOperand{PACK_MLP, (size_t)p.kpad * hidden, 0};
        w1_bytes = (size_t)p.kpad * hidden * 4;
        second_bytes = (size_t)p.dx_slabs * n * cin * 4;
        w2_bytes = 0;
    } else {
        const bool bf = form == MLP_BF16;
        p.ok = bf ? mlp_bf16_shape_ok(s) && s.cin != 128 && s.cout <= 3 : mlp_f32_shape_ok(s, 256);   // (split: cin and the upper end of cout by bwd_shape_form)
        p.mt = s.cin / 16;
        p.co = 3;
        p.slabs = mb_gx(s.n);
        p.dx_gx = cdiv(cdiv(s.n, MB_T), MBB_WAVES);       // a wave per 32-row tile
        // bf16: a wave walks the tiles and owns 64 hidden columns; split: a workgroup walks, its four waves own 64 columns each
        p.gx = bf ? p.slabs / MBB_WAVES : p.slabs;
        p.gy = bf ? s.hidden / MBW_HCW : s.hidden / (MBB_WAVES * MBW_HCW);
        p.smem = bf ? mb_w_lds(s.cin) : (size_t)MBS_WG_LDS(s.cin);
        const size_t w2_frags = (size_t)(s.hidden >> 4) * (bf ? 32 : 64);      // 16-byte pieces the W2 pack writes, one per thread
        p.op[0] = MlpOperand{bf ? PACK_MLP_BF16 : PACK_MLP_SPLIT, wide, 0};
        p.op[1] = MlpOperand{bf ? PACK_MLP_W1DX_BF16 : PACK_MLP_W1DX_SPLIT, wide, 0};
        p.op[2] = MlpOperand{bf ? PACK_MLP_W2_BF16 : PACK_MLP_W2_SPLIT, (w2_frags + 255) / 256 * 1024, 0};
        p.nops = 3;
        w1_bytes = second_bytes = (bf ? 1 : 3) * wide * 2;
        w2_bytes = (size_t)(s.hidden >> 4) * 64 * 16;
    }
    // the workspace layout, written down once
    const size_t gx = p.slabs;
    size_t o = 0;
    auto take = [&o](size_t bytes) {
        const size_t at = o;
        o += align_up(bytes, 256);
        return at;
    };
    p.wp = take(w1_bytes);
    p.w1d = take(second_bytes);
    p.dW1 = take(gx * wide * 4);
    p.db1 = take(gx * hidden * 4);
    p.dW2 = take(gx * hidden * 4 * 4);
    p.db2 = take((size_t)1024 * 4 * 4);
    p.w2p = take(w2_bytes);
    p.rtmp = take((reduce_tmp_floats(1024, 4) + reduce_tmp_floats((int)gx, wide) + reduce_tmp_floats((int)gx, hidden * 5)) * 4 + 256);
    p.bytes = o;
    p.op[0].off = p.wp;
    p.op[1].off = p.w1d;
    p.op[2].off = p.w2p;
    return p;
}

MlpFwdPlan plan_mlp_fwd(const MlpShape& s, bool aligned) {
    const MlpForm shape_form = fwd_shape_form(s);
    // (misaligned fp32 rows: the fp32-MFMA kernel, which reads them element by element)
    MlpFwdPlan p = fwd_layout(s, shape_form == MLP_SPLIT && !aligned ? MLP_F32 : shape_form);
    p.shape_form = shape_form;
    return p;
}
MlpBwdPlan plan_mlp_bwd(const MlpShape& s, bool aligned) {
    const MlpForm shape_form = bwd_shape_form(s);
    MlpBwdPlan p = bwd_layout(s, shape_form == MLP_SPLIT && !aligned ? MLP_F32 : shape_form);
    p.shape_form = shape_form;
    return p;
}

// ---- the operands as jobs of pack_many_kernel ------------------------------------------------------------------------------------
static int operand_jobs(const MlpOperand* op, int nops, const MlpShape& s, const float* W1, const float* W2, char* ws, PackJob* jobs,
                        size_t* totals) {
    for (int i = 0; i < nops; ++i) {
        const bool w2 = op[i].kind == PACK_MLP_W2_BF16 || op[i].kind == PACK_MLP_W2_SPLIT;
        const int kdim = op[i].kind == PACK_MLP ? (int)(op[i].count / s.hidden) : 0;     // (the fp32 operand: kpad)
        jobs[i] = PackJob{w2 ? W2 : W1, (float*)(ws + op[i].off), op[i].kind, s.cin, s.cout, kdim, s.hidden, 0, 0, 0, 0, 0, 0};
        totals[i] = op[i].count;
    }
    return nops;
}
// fgc_conv_pack's view of the two workspaces: what the shape alone selects
int mlp_pack_jobs(const fgc_pack_extra* e, PackJob* jobs, size_t* totals) {
    const MlpShape s{e->mlp_n, e->mlp_cin, e->mlp_hidden, e->mlp_cout, e->mlp_bf16 != 0};
    int nj = 0;
    if (e->mlp_fwd_ws) {
        const MlpFwdPlan p = plan_mlp_fwd(s);
        if (!p.ok || (uintptr_t)e->mlp_fwd_ws % 16 != 0) return -1;
        nj += operand_jobs(&p.w1, 1, s, e->mlp_W1, e->mlp_W2, (char*)e->mlp_fwd_ws, jobs, totals);
    }
    if (e->mlp_bwd_ws) {
        const MlpBwdPlan p = plan_mlp_bwd(s);
        if (!p.ok) return -1;
        // (the W2 operand lies behind the slabs, whose size follows from n)
        if (p.form != MLP_F32 && (s.n <= 0 || !e->mlp_W2 || (uintptr_t)e->mlp_bwd_ws % 16 != 0)) return -1;
        nj += operand_jobs(p.op, p.nops, s, e->mlp_W1, e->mlp_W2, (char*)e->mlp_bwd_ws, jobs + nj, totals + nj);
    }
    return nj;
}

// which operand layouts the options in force select for the shape (include/fgc.h: fgc_mlp_layout_id), 1 ... 255
static int mlp_layout_id(const MlpShape& s) {
    if (s.bf16) return 1 | 8;     // (the bf16-storage kernels have one operand form)
    return 1 | (plan_mlp_fwd(s).form == MLP_SPLIT ? 2 : 0) | (plan_mlp_bwd(s).form == MLP_SPLIT ? 4 : 0);
}

// ---- what a call's pointers add to the plan: asked by the entry points and by fgc_mlp_forms alike ----------------------------------
// every kernel form reads its packed W1 out of the workspace in 16-byte pieces (and pack_many_kernel writes it so)
static bool mlp_ws_aligned(const void* ws) { return (uintptr_t)ws % 16 == 0; }
// the 16-byte alignment the split forms need beyond that (NULL counts as aligned); without it an fp32 call takes the fp32 MFMA,
// which reads rows and b1 element by element (the split dx kernel reads b1 in 16-byte pieces as well)
static bool mlp_fwd_call_aligned(const void* x) { return (uintptr_t)x % 16 == 0; }
static bool mlp_bwd_call_aligned(const void* x, const void* dx, const void* b1) {
    return (uintptr_t)x % 16 == 0 && (uintptr_t)dx % 16 == 0 && (uintptr_t)b1 % 16 == 0;
}

// ---- argument checks: one for the fp32 entry points, one for the bf16 ones ---------------------------------------------------------
// an FGC_MLP_PACKED call whose flags carry the layout the workspace was packed in (FGC_MLP_LAYOUT): refuse if the options moved
static int mlp_check_common(const char* who, const MlpShape& s, float alpha, int flags) {
    FGC_CHECK_ARG(alpha >= 0.f && alpha <= 1.f, "%s: alpha=%g outside [0,1] (the reference uses 0.1, model.py:846)", who, alpha);
    FGC_CHECK_ARG(!(flags & FGC_MLP_PACKED) || (flags >> 8) == 0 || (flags >> 8) == mlp_layout_id(s),
                  "%s: FGC_MLP_PACKED, but the operands were packed in layout %d and the options now select %d (an option "
                  "changed between fgc_conv_pack and this call)", who, flags >> 8, mlp_layout_id(s));
    return FGC_OK;
}
static int mlp_f32_check(const char* who, const MlpShape& s, int hidden_mult, float alpha, int flags) {
    FGC_CHECK_ARG(s.n > 0 && s.cin > 0 && s.cin <= 128, "%s: n=%d cin=%d (cin must be in [1,128])", who, s.n, s.cin);
    FGC_CHECK_ARG(s.hidden > 0 && s.hidden % hidden_mult == 0, "%s: hidden=%d must be a multiple of %d", who, s.hidden, hidden_mult);
    FGC_CHECK_ARG(s.cout > 0 && s.cout <= MLP_COUT_MAX, "%s: cout=%d outside [1,%d]", who, s.cout, MLP_COUT_MAX);
    return mlp_check_common(who, s, alpha, flags);
}
static int mlp_bf16_check(const char* who, const MlpShape& s, const void* x, float alpha, int flags) {
    FGC_CHECK_ARG(x && s.n > 0, "%s: null x / n=%d", who, s.n);
    FGC_CHECK_ARG(s.cin == 32 || s.cin == 64 || s.cin == 128, "%s: cin=%d (the bf16 MLP takes 32, 64 or 128 input channels)", who, s.cin);
    FGC_CHECK_ARG(s.hidden > 0 && s.hidden % 256 == 0, "%s: hidden=%d must be a multiple of 256", who, s.hidden);
    FGC_CHECK_ARG(s.cout > 0 && s.cout <= 4, "%s: cout=%d outside [1,4]", who, s.cout);
    FGC_CHECK_ARG(mlp_fwd_call_aligned(x), "%s: x needs 16-byte alignment", who);
    return mlp_check_common(who, s, alpha, flags);
}

// ---- what the four entry points do once their arguments are checked: pack if not FGC_MLP_PACKED, launch, reduce -----------------
static int mlp_fwd_run(const char* who, const MlpShape& s, const MlpFwdPlan& p, const MlpFwdArgs& a, int flags, hipStream_t st) {
    if (!(flags & FGC_MLP_PACKED)) {
        PackJob job;
        size_t total;
        operand_jobs(&p.w1, 1, s, a.W1, a.W2, a.ws, &job, &total);
        const int rc = launch_pack_jobs(&job, &total, 1, who, st);
        if (rc) return rc;
    }
    switch (p.form) {
        case MLP_F32: return launch_mlp_fwd_f32(s, p, a, st);
        case MLP_SPLIT: return launch_mlp_fwd_split(s, p, a, st);
        default: return launch_mlp_fwd_bf16(s, p, a, st);
    }
}
static int mlp_bwd_run(const char* who, const MlpShape& s, const MlpBwdPlan& p, const MlpBwdArgs& a, float* dW1, float* db1, float* dW2,
                       float* db2, int flags, hipStream_t st) {
    int rc;
    if (!(flags & FGC_MLP_PACKED)) {
        PackJob jobs[3];
        size_t totals[3];
        const int nj = operand_jobs(p.op, p.nops, s, a.W1, a.W2, a.ws, jobs, totals);
        if ((rc = launch_pack_jobs(jobs, totals, nj, who, st))) return rc;
    }
    switch (p.form) {
        case MLP_F32: rc = launch_mlp_bwd_f32(s, p, a, st); break;
        case MLP_SPLIT: rc = launch_mlp_bwd_split(s, p, a, st); break;
        default: rc = launch_mlp_bwd_bf16(s, p, a, st); break;
    }
    if (rc) return rc;
    // fixed-order reductions of the slabs, all of them in two launches (the fp32-MFMA kernel leaves dx in slabs as well)
    const int n = s.n, cin = s.cin, hidden = s.hidden, gx = p.slabs;
    RedJob jobs[5];
    int nj = 0;
    if (p.dx_slabs) jobs[nj++] = RedJob{(float*)(a.ws + p.w1d), (size_t)n * cin, p.dx_slabs, n * cin, cin, cin, (float*)a.dx};
    jobs[nj++] = RedJob{(float*)(a.ws + p.dW1), (size_t)cin * hidden, gx, cin * hidden, hidden, hidden, dW1};
    jobs[nj++] = RedJob{(float*)(a.ws + p.db1), (size_t)hidden, gx, hidden, hidden, hidden, db1};
    jobs[nj++] = RedJob{(float*)(a.ws + p.dW2), (size_t)hidden * 4, gx, hidden * 4, 4, s.cout, dW2};
    jobs[nj++] = RedJob{(float*)(a.ws + p.db2), (size_t)4, gx, 4, 4, s.cout, db2};
    if ((rc = reduce_jobs("reduce:mlp", jobs, nj, (float*)(a.ws + p.rtmp), st))) return rc;
    FGC_CHECK_LAUNCH(who);
    return FGC_OK;
}

}  // namespace fgc

using namespace fgc;

extern "C" int32_t fgc_mlp_layout_id(int32_t cin, int32_t hidden, int32_t cout, int32_t bf16) {
    return mlp_layout_id(MlpShape{1, cin, hidden, cout, bf16 != 0});
}

extern "C" int32_t fgc_mlp_num_partials(int32_t n) { return cdiv(n, MLP_T); }

// sizes only.  The fp32 entry points may fall back from the split form to the fp32 MFMA at call time (misaligned pointers), and
// the forward workspace is sized before the options are final: room for either form.
extern "C" size_t fgc_mlp_workspace_bytes(int32_t cin, int32_t hidden, int32_t cout) {
    const MlpShape s{1, cin, hidden, cout, false};
    return std::max(fwd_layout(s, MLP_F32).bytes, fwd_layout(s, MLP_SPLIT).bytes);
}
extern "C" size_t fgc_mlp_bwd_workspace_bytes(int32_t n, int32_t cin, int32_t hidden, int32_t cout) {
    const MlpShape s{n, cin, hidden, cout, false};
    return std::max(plan_mlp_bwd(s, true).bytes, plan_mlp_bwd(s, false).bytes);
}
extern "C" size_t fgc_mlp_bf16_workspace_bytes(int32_t cin, int32_t hidden, int32_t cout) {
    return plan_mlp_fwd(MlpShape{1, cin, hidden, cout, true}).bytes;
}
extern "C" size_t fgc_mlp_bwd_bf16_workspace_bytes(int32_t n, int32_t cin, int32_t hidden, int32_t cout) {
    return plan_mlp_bwd(MlpShape{n, cin, hidden, cout, true}).bytes;
}

extern "C" int fgc_mlp_fwd(const float* x, int32_t n, int32_t cin, int32_t hidden, int32_t cout, const float* W1,
                           const float* b1, const float* W2, const float* b2, float alpha, float* y,
                           float* abs_partial, int32_t flags, void* workspace, size_t workspace_bytes, void* stream) {
    const MlpShape s{n, cin, hidden, cout, false};
    FGC_CHECK_ARG(x && W1 && b1 && W2 && b2 && y, "fgc_mlp_fwd: null pointer");
    const int rc = mlp_f32_check("fgc_mlp_fwd", s, 64, alpha, flags);
    if (rc) return rc;
    FGC_CHECK_ARG(workspace && workspace_bytes >= fgc_mlp_workspace_bytes(cin, hidden, cout), "fgc_mlp_fwd: workspace too small");
    FGC_CHECK_ARG(mlp_ws_aligned(workspace), "fgc_mlp_fwd: workspace needs 16-byte alignment (the packed W1 is read in 16-byte pieces)");
    const MlpFwdPlan p = plan_mlp_fwd(s, mlp_fwd_call_aligned(x));
    // (the operands fgc_conv_pack leaves are the split planes whenever the SHAPE takes the split path)
    FGC_CHECK_ARG(!(flags & FGC_MLP_PACKED) || p.form == p.shape_form,
                  "fgc_mlp_fwd: FGC_MLP_PACKED needs 16-byte aligned x for this shape");
    return mlp_fwd_run("fgc_mlp_fwd", s, p, MlpFwdArgs{x, W1, b1, W2, b2, alpha, y, abs_partial, (char*)workspace}, flags,
                       (hipStream_t)stream);
}

extern "C" int fgc_mlp_bwd(const float* x, const float* dy, int32_t n, int32_t cin, int32_t hidden, int32_t cout,
                           const float* W1, const float* b1, const float* W2, float alpha, float* dx, float* dW1,
                           float* db1, float* dW2, float* db2, int32_t flags, void* workspace, size_t workspace_bytes,
                           void* stream) {
    const MlpShape s{n, cin, hidden, cout, false};
    FGC_CHECK_ARG(x && dy && W1 && b1 && W2 && dx && dW1 && db1 && dW2 && db2, "fgc_mlp_bwd: null pointer");
    const int rc = mlp_f32_check("fgc_mlp_bwd", s, 256, alpha, flags);
    if (rc) return rc;
    FGC_CHECK_ARG(workspace && workspace_bytes >= fgc_mlp_bwd_workspace_bytes(n, cin, hidden, cout),
                  "fgc_mlp_bwd: workspace too small (%zu < %zu)", workspace_bytes, fgc_mlp_bwd_workspace_bytes(n, cin, hidden, cout));
    FGC_CHECK_ARG(mlp_ws_aligned(workspace), "fgc_mlp_bwd: workspace needs 16-byte alignment (the packed W1 is read in 16-byte pieces)");
    const MlpBwdPlan p = plan_mlp_bwd(s, mlp_bwd_call_aligned(x, dx, b1));
    FGC_CHECK_ARG(!(flags & FGC_MLP_PACKED) || p.form == p.shape_form,
                  "fgc_mlp_bwd: FGC_MLP_PACKED needs 16-byte aligned x, dx and b1 for this shape");
    return mlp_bwd_run("fgc_mlp_bwd", s, p, MlpBwdArgs{x, dy, W1, b1, W2, alpha, dx, (char*)workspace}, dW1, db1, dW2, db2, flags,
                       (hipStream_t)stream);
}

extern "C" int fgc_mlp_fwd_bf16(const void* x, int32_t n, int32_t cin, int32_t hidden, int32_t cout, const float* W1,
                                const float* b1, const float* W2, const float* b2, float alpha, float* y,
                                float* abs_partial, int32_t flags, void* workspace, size_t workspace_bytes, void* stream) {
    const MlpShape s{n, cin, hidden, cout, true};
    const int rc = mlp_bf16_check("fgc_mlp_fwd_bf16", s, x, alpha, flags);
    if (rc) return rc;
    FGC_CHECK_ARG(W1 && b1 && W2 && b2 && y, "fgc_mlp_fwd_bf16: null pointer");
    const MlpFwdPlan p = plan_mlp_fwd(s);
    FGC_CHECK_ARG(workspace && workspace_bytes >= p.bytes && mlp_ws_aligned(workspace),
                  "fgc_mlp_fwd_bf16: workspace too small or misaligned");
    return mlp_fwd_run("fgc_mlp_fwd_bf16", s, p, MlpFwdArgs{x, W1, b1, W2, b2, alpha, y, abs_partial, (char*)workspace}, flags,
                       (hipStream_t)stream);
}

extern "C" int fgc_mlp_bwd_bf16(const void* x, const float* dy, int32_t n, int32_t cin, int32_t hidden, int32_t cout,
                                const float* W1, const float* b1, const float* W2, float alpha, void* dx, float* dW1,
                                float* db1, float* dW2, float* db2, int32_t flags, void* workspace, size_t workspace_bytes,
                                void* stream) {
    const MlpShape s{n, cin, hidden, cout, true};
    const int rc = mlp_bf16_check("fgc_mlp_bwd_bf16", s, x, alpha, flags);
    if (rc) return rc;
    FGC_CHECK_ARG(dy && W1 && b1 && W2 && dx && dW1 && db1 && dW2 && db2, "fgc_mlp_bwd_bf16: null pointer");
    const MlpBwdPlan p = plan_mlp_bwd(s);
    FGC_CHECK_ARG(p.ok, "fgc_mlp_bwd_bf16: cin=%d cout=%d (cin 32 or 64, cout <= 3)", cin, cout);
    FGC_CHECK_ARG(workspace && workspace_bytes >= p.bytes && mlp_ws_aligned(workspace),
                  "fgc_mlp_bwd_bf16: workspace too small or misaligned");
    return mlp_bwd_run("fgc_mlp_bwd_bf16", s, p, MlpBwdArgs{x, dy, W1, b1, W2, alpha, dx, (char*)workspace}, dW1, db1, dW2, db2, flags,
                       (hipStream_t)stream);
}

extern "C" int fgc_mlp_forms(int32_t n, int32_t cin, int32_t hidden, int32_t cout, int32_t bf16, const void* x, const void* dx,
                             const void* b1, const void* fwd_ws, const void* bwd_ws, char* buf, int32_t buf_bytes) {
    FGC_CHECK_ARG(buf && buf_bytes > 0, "fgc_mlp_forms: no buffer");
    int len = 0;
    bool full = false;
    auto put = [&](const char* key, const char* fmt, auto value) {
        char tmp[96];
        int k = snprintf(tmp, sizeof tmp, "%s%s=", len ? " " : "", key);
        k += snprintf(tmp + k, sizeof tmp - k, fmt, value);
        if (full || len + k + 1 > buf_bytes) { full = true; return; }
        memcpy(buf + len, tmp, (size_t)k + 1);
        len += k;
    };
    static const char* const names[] = {"f32", "split", "bf16"};
    buf[0] = 0;
    const MlpShape s{n, cin, hidden, cout, bf16 != 0};
    // the plans exactly as the entry points ask for them; `none` where the entry point returns before any launch (the bf16
    // forms have no kernel for rows that are not 16-byte aligned)
    const MlpFwdPlan f = plan_mlp_fwd(s, s.bf16 || mlp_fwd_call_aligned(x));
    const MlpBwdPlan b = plan_mlp_bwd(s, s.bf16 || mlp_bwd_call_aligned(x, dx, b1));
    const bool rows_ok = n > 0 && (!s.bf16 || mlp_fwd_call_aligned(x));
    put("fwd", "%s", f.ok && rows_ok && mlp_ws_aligned(fwd_ws) ? names[f.form] : "none");
    put("fwd_ks", "%d", f.ks);
    put("fwd_co", "%d", f.co);
    put("fwd_kpad", "%d", f.kpad);
    put("fwd_gx", "%d", f.gx);
    put("bwd", "%s", b.ok && rows_ok && mlp_ws_aligned(bwd_ws) ? names[b.form] : "none");
    put("bwd_mt", "%d", b.mt);
    put("bwd_ctw", "%d", b.ctw);
    put("bwd_co", "%d", b.co);
    put("bwd_slabs", "%d", b.slabs);
    put("bwd_dx_slabs", "%d", b.dx_slabs);
    put("bwd_dx_gx", "%d", b.dx_gx);
    put("bwd_gx", "%d", b.gx);
    put("bwd_gy", "%d", b.gy);
    put("fwd_shape", "%s", names[f.shape_form]);
    put("bwd_shape", "%s", names[b.shape_form]);
    put("layout", "%d", mlp_layout_id(s));
    FGC_CHECK_ARG(!full, "fgc_mlp_forms: buffer of %d bytes too small", buf_bytes);
    return len;
}
