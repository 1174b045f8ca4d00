// Ray casting against a triangle list (build extension; include/fgc.h: fgc_ray_cast): for every ray o + t d the first
// triangle it meets, brute force over rays x triangles.  What a virtual depth scan is made of (utils.visible_vertices,
// utils.depth_image); run once per mesh at preparation time, never per training step.
//
// Three launches (the layout, the slab split and rc_gather_kernel live in fgc_slabs.h, shared with fgc_surface.hip):
//   rc_gather_kernel  one thread per record: rc_record of triangle f (zero records for a bad row and the padding behind nf).
//                     The same launch sets every ray's key to (+inf, -1).
//   rc_cast_kernel    64 rays per workgroup, one per lane and the same in all four waves (bl_filter_kernel's shape); the
//                     records are wave-uniform: chunks of RC_CHUNK come through scalar loads and reach the VALU from SGPRs,
//                     the waves take the chunks of the workgroup's slab in turn.  Each lane keeps its smallest (t, face),
//                     the four waves merge through LDS, and the workgroup's result goes into the ray's key with ONE 64-bit
//                     integer atomic min on (float bits of t) << 32 | face: t > t_min >= 0 orders like its bits, and equal
//                     t leave the smaller face.  The triangle list is split into slabs over blockIdx.y where the ray blocks
//                     alone do not fill the device; the minimum over (t, face) is exact, so it does not depend on the split.
//   rc_finish_kernel  one thread per ray: key -> t_out, face_out, and (u, v) of the winner evaluated again by the same
//                     function on the same record (the same bits the cast kernel compared).
//
// Per pair (rc_uvt, fgc_raycast.h): p = d x e2 (3 v_mul + 3 v_fma), det (v_mul + 2 v_fma), s = o - a (3 v_sub), s . p (v_mul + 2
// v_fma), u = (s . p) / det (the IEEE division: 11 instructions, one of them v_rcp_f32), the test of u (two v_cmp and a
// v_mov): 29 vector instructions in the gfx950 ISA.  A hit needs 0 <= u <= 1 (u + v <= 1 with v >= 0 implies it in rounded
// arithmetic too: rounding is monotonic), so everything else - qv = s x e1, v, t, two more divisions, 39 more instructions -
// sits behind a branch that a wave skips when none of its 64 rays passes; with small triangles that is nearly every pair.
// This is why there is no separate single-origin kernel: precomputing s, qv and e2 . qv per triangle would take 3 v_sub out
// of the 29 and nothing else, for a second record layout; a call with one origin runs this kernel with row 0 for every
// ray, the same bits.  (Built with -fno-slp-vectorize: Makefile; DESIGN.md 8e has the measurements.)
//
// Contraction is off, every FMA is written out.  Device data is never trusted for addressing: vertex ids are checked
// before a load, the face of a key before the record is read.
#include "fgc_slabs.h"

#pragma clang fp contract(off)

namespace fgc {

// grid (ceil(nq / 64), slabs)
__global__ __launch_bounds__(RC_THREADS) void rc_cast_kernel(const f32x4* __restrict__ rec, int nrec, int per_slab,
                                                             const float* __restrict__ origins, int n_origins,
                                                             const float* __restrict__ dirs, int nq, float t_min,
                                                             unsigned long long* __restrict__ keys) {
    __shared__ float part_t[RC_WAVES][RC_Q];
    __shared__ int part_f[RC_WAVES][RC_Q];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int q = blockIdx.x * RC_Q + lane;
    const bool live = q < nq;
    float o[3], d[3];
    rc_load_ray(origins, n_origins, dirs, q, live, o, d);
    float best_t = __builtin_inff();
    int best_f = -1;
    // records [j0, j1) of this slab, whole chunks (nrec and per_slab are multiples of RC_CHUNK); faces in rising order, so
    // the strict comparison keeps the smallest index among equal t
    const int j0 = blockIdx.y * per_slab, j1 = min(nrec, j0 + per_slab);
    for (int j = j0 + wave * RC_CHUNK; j < j1; j += RC_WAVES * RC_CHUNK) {
        const f32x4* rb = rec + 3 * (size_t)j;      // wave-uniform: scalar loads
        f32x4 r[3 * RC_CHUNK];
#pragma unroll
        for (int k = 0; k < 3 * RC_CHUNK; ++k) r[k] = rb[k];
#pragma unroll
        for (int k = 0; k < RC_CHUNK; ++k) {
            float u, v, t;
            if (rc_uvt(o, d, r[3 * k], r[3 * k + 1], r[3 * k + 2], t_min, u, v, t) && t < best_t) best_t = t, best_f = j + k;
        }
    }
    part_t[wave][lane] = best_t;
    part_f[wave][lane] = best_f;
    __syncthreads();
    if (wave != 0 || !live) return;
#pragma unroll
    for (int w = 1; w < RC_WAVES; ++w) {
        const float t = part_t[w][lane];
        const int f = part_f[w][lane];
        if (f >= 0 && (t < best_t || (t == best_t && f < best_f))) best_t = t, best_f = f;
    }
    if (best_f >= 0)
        atomicMin(keys + q, ((unsigned long long)__float_as_uint(best_t) << 32) | (unsigned)best_f);
}

__global__ __launch_bounds__(256) void rc_finish_kernel(const f32x4* __restrict__ rec, int nf,
                                                        const unsigned long long* __restrict__ keys,
                                                        const float* __restrict__ origins, int n_origins,
                                                        const float* __restrict__ dirs, int nq, float t_min,
                                                        float* __restrict__ t_out, int* __restrict__ face_out,
                                                        float* __restrict__ bary_out) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nq) return;
    const unsigned long long key = keys[q];
    const int f = (int)(unsigned)(key & 0xFFFFFFFFull);
    float t = __builtin_inff(), u = 0.f, v = 0.f;
    int face = -1;
    if ((unsigned)f < (unsigned)nf) {
        face = f;
        t = __uint_as_float((unsigned)(key >> 32));
        if (bary_out) {
            const size_t oo = n_origins == 1 ? 0 : 3 * (size_t)q;
            const float o[3] = {origins[oo], origins[oo + 1], origins[oo + 2]};
            const float d[3] = {dirs[3 * (size_t)q], dirs[3 * (size_t)q + 1], dirs[3 * (size_t)q + 2]};
            float t2;
            if (!rc_uvt(o, d, rec[3 * (size_t)f], rec[3 * (size_t)f + 1], rec[3 * (size_t)f + 2], t_min, u, v, t2)) u = v = 0.f;
        }
    }
    t_out[q] = t;
    face_out[q] = face;
    if (bary_out) bary_out[2 * (size_t)q] = u, bary_out[2 * (size_t)q + 1] = v;
}

}  // namespace fgc

using namespace fgc;

extern "C" size_t fgc_ray_cast_workspace_bytes(int32_t nf, int32_t nq) {
    if (nf <= 0 || nq <= 0 || nf > FGC_RAY_CAST_MAX_FACES) return 0;
    return rc_layout(nf, nq).total;
}

extern "C" int fgc_ray_cast(const float* verts, int32_t nv, const int32_t* faces, int32_t nf, const float* origins,
                            int32_t n_origins, const float* dirs, int32_t nq, float t_min, float* t_out, int32_t* face_out,
                            float* bary_out, void* workspace, size_t workspace_bytes, void* stream) {
    FGC_CHECK_ARG(verts && faces && origins && dirs && t_out && face_out && workspace, "fgc_ray_cast: null pointer");
    FGC_CHECK_ARG(nv > 0 && nf > 0 && nq > 0, "fgc_ray_cast: nv=%d nf=%d nq=%d (all > 0)", nv, nf, nq);
    FGC_CHECK_ARG(nf <= FGC_RAY_CAST_MAX_FACES, "fgc_ray_cast: nf=%d (at most %d)", nf, FGC_RAY_CAST_MAX_FACES);
    FGC_CHECK_ARG(n_origins == 1 || n_origins == nq, "fgc_ray_cast: n_origins=%d (1 or nq=%d)", n_origins, nq);
    FGC_CHECK_ARG(t_min >= 0.f && t_min < __builtin_inff(), "fgc_ray_cast: t_min=%g (>= 0 and finite)", (double)t_min);
    FGC_CHECK_ARG((uintptr_t)workspace % 16 == 0, "fgc_ray_cast: workspace needs 16-byte alignment");
    const RcLayout L = rc_layout(nf, nq);
    FGC_CHECK_ARG(workspace_bytes >= L.total, "fgc_ray_cast: workspace too small (%zu < %zu bytes)", workspace_bytes, L.total);
    hipStream_t st = (hipStream_t)stream;
    f32x4* rec = (f32x4*)workspace;
    unsigned long long* keys = (unsigned long long*)((char*)workspace + L.keys);
    FGC_LAUNCH("rc_gather_kernel", st, rc_gather_kernel, dim3(cdiv(std::max(L.nrec, nq), 256)), dim3(256), 0, verts, nv, faces, nf,
               L.nrec, rec, keys, nq);
    FGC_LAUNCH("rc_cast_kernel", st, rc_cast_kernel, dim3(cdiv(nq, RC_Q), L.slabs), dim3(RC_THREADS), 0, (const f32x4*)rec,
               L.nrec, L.per_slab, origins, n_origins, dirs, nq, t_min, keys);
    FGC_LAUNCH("rc_finish_kernel", st, rc_finish_kernel, dim3(cdiv(nq, 256)), dim3(256), 0, (const f32x4*)rec, nf,
               (const unsigned long long*)keys, origins, n_origins, dirs, nq, t_min, t_out, face_out, bary_out);
    FGC_CHECK_LAUNCH("fgc_ray_cast");
    return FGC_OK;
}
