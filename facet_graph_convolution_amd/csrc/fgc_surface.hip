// Closest point on a triangle list without a tree, and the two-sided point-to-surface loss built on it (build extensions;
// include/fgc.h: fgc_closest_point, fgc_surface_loss).  fgc_closest_point is to fgc_closest_point_tree what fgc_ray_cast is to
// fgc_ray_cast_tree: the same records (rc_record), the same per-pair function (cp_pair), every pair tested - for meshes that
// move every step, where two tree builds cost more than 1 000 samples save.
//
// The scan has fgc_ray_cast's launch shape (fgc_slabs.h):
//   rc_gather_kernel  the records of the mesh and every query's key = (+inf, -1).
//   cp_scan_kernel    64 points per workgroup, one per lane and the same in all four waves; the records are wave-uniform and
//                     come through scalar loads, the waves take the chunks of the workgroup's slab in turn.  Each lane keeps
//                     its smallest (dist2, face), the four waves merge through LDS, and the workgroup's result goes into the
//                     point's key with ONE 64-bit integer atomic min on (float bits of dist2) << 32 | face: dist2 >= 0 orders
//                     like its bits.  The minimum is exact, so it does not depend on the split into slabs.
//   cp_finish_kernel  key -> dist2_out, face_out, and (u, v) of the winner by cp_pair on the same record: the same bits.
// A record whose e1 and e2 are all +-0 takes no part, as in the tree (an invalid row, the padding, a collapsed triangle).
//
// The loss: two scans (the sampled rows of p0 against mesh 1, the sampled rows of p1 against mesh 0), one launch that turns
// every winner into gradient terms - one for a precision sample, three (the winning face's vertices) for a completeness
// sample - and the single-workgroup reduction of fgc_point_loss (fgc_points.h).  No atomics on floats.
//
// Contraction is off, every FMA is written out.  Device data is never trusted for addressing: the face of a key is bounded
// before its record is read, the vertex ids of a winning face before they become gradient rows.
#include "fgc_closest.h"
#include "fgc_points.h"
#include "fgc_slabs.h"

#pragma clang fp contract(off)

namespace fgc {

// whether a record takes part: not all six of e1, e2 are +-0 (wave-uniform where the record is)
__device__ __forceinline__ bool cp_takes_part(f32x4 e1, f32x4 e2) {
    return ((__float_as_uint(e1.x) | __float_as_uint(e1.y) | __float_as_uint(e1.z) | __float_as_uint(e2.x) |
             __float_as_uint(e2.y) | __float_as_uint(e2.z)) << 1) != 0u;
}

// grid (ceil(nq / 64), slabs)
__global__ __launch_bounds__(RC_THREADS) void cp_scan_kernel(const f32x4* __restrict__ rec, int nrec, int per_slab,
                                                             const float* __restrict__ points, int nq,
                                                             unsigned long long* __restrict__ keys) {
    __shared__ float part_d[RC_WAVES][RC_Q];
    __shared__ int part_f[RC_WAVES][RC_Q];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int i = blockIdx.x * RC_Q + lane;
    const bool live = i < nq;
    float q[3] = {0.f, 0.f, 0.f};
    if (live) q[0] = points[3 * (size_t)i], q[1] = points[3 * (size_t)i + 1], q[2] = points[3 * (size_t)i + 2];
    float best = __builtin_inff();
    int best_f = -1;
    // records [j0, j1) of this slab, whole chunks; faces in rising order, so the strict comparison keeps the smallest index
    // among equal dist2 (a NaN and +inf fail it)
    const int j0 = blockIdx.y * per_slab, j1 = min(nrec, j0 + per_slab);
    for (int j = j0 + wave * RC_CHUNK; j < j1; j += RC_WAVES * RC_CHUNK) {
        const f32x4* rb = rec + 3 * (size_t)j;      // wave-uniform: scalar loads
        f32x4 r[3 * RC_CHUNK];
#pragma unroll
        for (int k = 0; k < 3 * RC_CHUNK; ++k) r[k] = rb[k];
#pragma unroll
        for (int k = 0; k < RC_CHUNK; ++k) {
            if (!cp_takes_part(r[3 * k + 1], r[3 * k + 2])) continue;
            float u, v;
            const float d = cp_pair(q, r[3 * k], r[3 * k + 1], r[3 * k + 2], u, v);
            if (d < best) best = d, best_f = j + k;
        }
    }
    part_d[wave][lane] = best;
    part_f[wave][lane] = best_f;
    __syncthreads();
    if (wave != 0 || !live) return;
#pragma unroll
    for (int w = 1; w < RC_WAVES; ++w) {
        const float d = part_d[w][lane];
        const int f = part_f[w][lane];
        if (f >= 0 && (d < best || (d == best && f < best_f))) best = d, best_f = f;
    }
    if (best_f >= 0) atomicMin(keys + i, ((unsigned long long)__float_as_uint(best) << 32) | (unsigned)best_f);
}

// The winner of a key: its face (bounded by nf before it addresses anything; -1 for none) and dist2; with the point q also
// (u, v) and r = q - closest point from cp_pair_r on the winner's record.
__device__ __forceinline__ int cp_winner(unsigned long long key, int nf, float& dist2) {
    const int f = (int)(unsigned)(key & 0xFFFFFFFFull);
    dist2 = __builtin_inff();
    if ((unsigned)f >= (unsigned)nf) return -1;
    dist2 = __uint_as_float((unsigned)(key >> 32));
    return f;
}

__global__ __launch_bounds__(256) void cp_finish_kernel(const f32x4* __restrict__ rec, int nf,
                                                        const unsigned long long* __restrict__ keys,
                                                        const float* __restrict__ points, int nq,
                                                        float* __restrict__ dist2_out, int* __restrict__ face_out,
                                                        float* __restrict__ bary_out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq) return;
    float d2, u = 0.f, v = 0.f;
    const int f = cp_winner(keys[i], nf, d2);
    if (f >= 0 && bary_out) {
        const float q[3] = {points[3 * (size_t)i], points[3 * (size_t)i + 1], points[3 * (size_t)i + 2]};
        cp_pair(q, rec[3 * (size_t)f], rec[3 * (size_t)f + 1], rec[3 * (size_t)f + 2], u, v);
    }
    dist2_out[i] = d2;
    face_out[i] = f;
    if (bary_out) bary_out[2 * (size_t)i] = u, bary_out[2 * (size_t)i + 1] = v;
}

// One thread per sample.  t < ns0: precision of sample t, the point q0[t] = p0[i0[t]] against its winner on mesh 1 - ONE term
// at t on row i0[t]: scale r / d.  t >= ns0: completeness of sample s = t - ns0, the point q1[s] = p1[i1[s]] against its winner
// f on mesh 0 - THREE terms at ns0 + 3 s + k on rows faces0[f][k]: -w_k scale r / d with w = (1 - u - v, u, v); the value sits
// on the first of them.  val = d if d <= threshold else 0; the gradient is 0 for a masked term and at d = 0.  A sample index
// out of range (its gathered point is a NaN row, which no record wins), no winner, or a winning face whose vertex ids are
// not rows of p0: rows -1, value NaN.
__global__ __launch_bounds__(256) void surface_terms_kernel(int np0, const int* __restrict__ faces0, int nf0, int nf1,
                                                            const f32x4* __restrict__ rec0, const f32x4* __restrict__ rec1,
                                                            const float* __restrict__ q0, const float* __restrict__ q1,
                                                            const unsigned long long* __restrict__ keys0,
                                                            const unsigned long long* __restrict__ keys1,
                                                            const int* __restrict__ i0, int ns0, int ns1, float threshold,
                                                            int* __restrict__ rows, float4* __restrict__ terms) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= ns0 + ns1) return;
    const bool prec = t < ns0;
    const int s = prec ? t : t - ns0;
    const float* qp = (prec ? q0 : q1) + 3 * (size_t)s;
    const float q[3] = {qp[0], qp[1], qp[2]};
    float d2;
    const int f = cp_winner(prec ? keys0[s] : keys1[s], prec ? nf1 : nf0, d2);
    const f32x4* rec = prec ? rec1 : rec0;
    int id[3] = {-1, -1, -1};
    bool ok = f >= 0;
    if (ok && prec) {
        id[0] = i0[s];
        ok = (unsigned)id[0] < (unsigned)np0;
    } else if (ok) {
#pragma unroll
        for (int k = 0; k < 3; ++k) id[k] = faces0[3 * (size_t)f + k], ok = ok && (unsigned)id[k] < (unsigned)np0;
    }
    float4 g = make_float4(0.f, 0.f, 0.f, __builtin_nanf(""));
    float w[3] = {0.f, 0.f, 0.f};
    if (ok) {
        float u, v, r[3];
        cp_pair_r(q, rec[3 * (size_t)f], rec[3 * (size_t)f + 1], rec[3 * (size_t)f + 2], u, v, r);
        const float d = sqrtf(d2);
        const bool keep = d <= threshold;
        const float c = (keep && d > 0.f) ? (1000.0f / (float)(prec ? ns0 : ns1)) / d : 0.f;
        g = make_float4(r[0] * c, r[1] * c, r[2] * c, keep ? d : 0.f);
        w[0] = (1.f - u) - v, w[1] = u, w[2] = v;
    }
    if (prec) {
        rows[t] = ok ? id[0] : -1;
        terms[t] = g;
        return;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const size_t at = (size_t)ns0 + 3 * (size_t)s + k;
        rows[at] = ok ? id[k] : -1;
        terms[at] = make_float4(-(w[k] * g.x), -(w[k] * g.y), -(w[k] * g.z), k == 0 ? g.w : 0.f);
    }
}

// records + keys of nq points against the mesh, then the scan: what fgc_closest_point and each side of the loss enqueue
static void cp_enqueue(const float* verts, int nv, const int* faces, int nf, const float* points, int nq, const RcLayout& L,
                       void* ws, hipStream_t st) {
    f32x4* rec = (f32x4*)ws;
    unsigned long long* keys = (unsigned long long*)((char*)ws + L.keys);
    FGC_LAUNCH("rc_gather_kernel", st, rc_gather_kernel, dim3(cdiv(std::max(L.nrec, nq), 256)), dim3(256), 0, verts, nv, faces, nf,
               L.nrec, rec, keys, nq);
    FGC_LAUNCH("cp_scan_kernel", st, cp_scan_kernel, dim3(cdiv(nq, RC_Q), L.slabs), dim3(RC_THREADS), 0, (const f32x4*)rec, L.nrec,
               L.per_slab, points, nq, keys);
}

struct SurfaceLossWs {
    RcLayout s0, s1;      // the scan of the p0 samples against mesh 1, of the p1 samples against mesh 0
    size_t scan0, scan1, q0, q1, rows, terms, total;
};

static SurfaceLossWs surface_loss_layout(int nf0, int nf1, int ns0, int ns1) {
    SurfaceLossWs w;
    w.s0 = rc_layout(nf1, ns0);
    w.s1 = rc_layout(nf0, ns1);
    size_t o = 0;
    auto take = [&](size_t bytes) {
        const size_t at = o;
        o = align_up(o + bytes, 256);
        return at;
    };
    w.scan0 = take(w.s0.total);
    w.scan1 = take(w.s1.total);
    w.q0 = take((size_t)ns0 * 12);
    w.q1 = take((size_t)ns1 * 12);
    w.rows = take(((size_t)ns0 + 3 * (size_t)ns1) * 4);
    w.terms = take(((size_t)ns0 + 3 * (size_t)ns1) * 16);
    w.total = o;
    return w;
}

static bool surface_counts_ok(int64_t nf0, int64_t nf1, int64_t ns0, int64_t ns1) {
    return nf0 > 0 && nf1 > 0 && ns0 > 0 && ns1 > 0 && nf0 <= FGC_RAY_CAST_MAX_FACES && nf1 <= FGC_RAY_CAST_MAX_FACES &&
           ns0 + 3 * ns1 <= FGC_POINT_LOSS_MAX_SAMPLES;
}

}  // namespace fgc

using namespace fgc;

extern "C" size_t fgc_closest_point_workspace_bytes(int32_t nf, int32_t nq) { return fgc_ray_cast_workspace_bytes(nf, nq); }

extern "C" int fgc_closest_point(const float* verts, int32_t nv, const int32_t* faces, int32_t nf, const float* points,
                                 int32_t nq, float* dist2_out, int32_t* face_out, float* bary_out, void* workspace,
                                 size_t workspace_bytes, void* stream) {
    FGC_CHECK_ARG(verts && faces && points && dist2_out && face_out && workspace, "fgc_closest_point: null pointer");
    FGC_CHECK_ARG(nv > 0 && nf > 0 && nq > 0, "fgc_closest_point: nv=%d nf=%d nq=%d (all > 0)", nv, nf, nq);
    FGC_CHECK_ARG(nf <= FGC_RAY_CAST_MAX_FACES, "fgc_closest_point: nf=%d (at most %d)", nf, FGC_RAY_CAST_MAX_FACES);
    FGC_CHECK_ARG((uintptr_t)workspace % 16 == 0, "fgc_closest_point: workspace needs 16-byte alignment");
    const RcLayout L = rc_layout(nf, nq);
    FGC_CHECK_ARG(workspace_bytes >= L.total, "fgc_closest_point: workspace too small (%zu < %zu bytes)", workspace_bytes, L.total);
    hipStream_t st = (hipStream_t)stream;
    cp_enqueue(verts, nv, faces, nf, points, nq, L, workspace, st);
    FGC_LAUNCH("cp_finish_kernel", st, cp_finish_kernel, dim3(cdiv(nq, 256)), dim3(256), 0, (const f32x4*)workspace, nf,
               (const unsigned long long*)((char*)workspace + L.keys), points, nq, dist2_out, face_out, bary_out);
    FGC_CHECK_LAUNCH("fgc_closest_point");
    return FGC_OK;
}

extern "C" size_t fgc_surface_loss_workspace_bytes(int32_t nf0, int32_t nf1, int32_t ns0, int32_t ns1) {
    if (!surface_counts_ok(nf0, nf1, ns0, ns1)) return 0;
    return surface_loss_layout(nf0, nf1, ns0, ns1).total;
}

extern "C" int fgc_surface_loss(const float* p0, int32_t np0, const int32_t* faces0, int32_t nf0, const float* p1, int32_t np1,
                                const int32_t* faces1, int32_t nf1, const int32_t* i0, int32_t ns0, const int32_t* i1,
                                int32_t ns1, float threshold, float* loss, float* g_p0, void* workspace, size_t workspace_bytes,
                                void* stream) {
    FGC_CHECK_ARG(p0 && faces0 && p1 && faces1 && i0 && i1 && loss && workspace, "fgc_surface_loss: null pointer");
    FGC_CHECK_ARG(np0 > 0 && nf0 > 0 && np1 > 0 && nf1 > 0 && ns0 > 0 && ns1 > 0,
                  "fgc_surface_loss: np0=%d nf0=%d np1=%d nf1=%d ns0=%d ns1=%d (all > 0)", np0, nf0, np1, nf1, ns0, ns1);
    FGC_CHECK_ARG(nf0 <= FGC_RAY_CAST_MAX_FACES && nf1 <= FGC_RAY_CAST_MAX_FACES, "fgc_surface_loss: nf0=%d nf1=%d (at most %d)",
                  nf0, nf1, FGC_RAY_CAST_MAX_FACES);
    FGC_CHECK_ARG((int64_t)ns0 + 3 * (int64_t)ns1 <= FGC_POINT_LOSS_MAX_SAMPLES,
                  "fgc_surface_loss: ns0 + 3 ns1 = %lld terms (at most %d)", (long long)ns0 + 3 * (long long)ns1,
                  FGC_POINT_LOSS_MAX_SAMPLES);
    const SurfaceLossWs L = surface_loss_layout(nf0, nf1, ns0, ns1);
    FGC_CHECK_ARG(workspace_bytes >= L.total, "fgc_surface_loss: workspace too small (%zu < %zu bytes)", workspace_bytes, L.total);
    FGC_CHECK_ARG((uintptr_t)workspace % 256 == 0, "fgc_surface_loss: workspace needs 256-byte alignment");
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    float* q0 = (float*)(ws + L.q0);
    float* q1 = (float*)(ws + L.q1);
    int* rows = (int*)(ws + L.rows);
    float4* terms = (float4*)(ws + L.terms);
    point_gather(p0, np0, i0, ns0, q0, st);
    point_gather(p1, np1, i1, ns1, q1, st);
    cp_enqueue(p1, np1, faces1, nf1, q0, ns0, L.s0, ws + L.scan0, st);
    cp_enqueue(p0, np0, faces0, nf0, q1, ns1, L.s1, ws + L.scan1, st);
    FGC_LAUNCH("surface_terms_kernel", st, surface_terms_kernel, dim3(cdiv(ns0 + ns1, 256)), dim3(256), 0, np0, faces0, nf0, nf1,
               (const f32x4*)(ws + L.scan1), (const f32x4*)(ws + L.scan0), (const float*)q0, (const float*)q1,
               (const unsigned long long*)(ws + L.scan0 + L.s0.keys), (const unsigned long long*)(ws + L.scan1 + L.s1.keys), i0,
               ns0, ns1, threshold, rows, terms);
    if (g_p0 && hipMemsetAsync(g_p0, 0, (size_t)np0 * 12, st) != hipSuccess) {
        fgc::set_error("fgc_surface_loss: memset failed");
        return FGC_EHIP;
    }
    point_loss_finish(rows, terms, ns0, 3 * ns1, ns0, ns1, loss, g_p0, st);
    FGC_CHECK_LAUNCH("fgc_surface_loss");
    return FGC_OK;
}
