// Ray casting through a bounding-box tree (build extension; include/fgc.h: fgc_ray_tree_build, fgc_ray_cast_tree): the first
// triangle every ray meets, as fgc_ray_cast finds it, at a cost that does not grow with rays x faces.  The per-pair
// arithmetic is rc_uvt of fgc_raycast.h, the function the brute-force kernel runs: what the tree finds is bit for bit what the
// full search finds, as long as the boxes do not cull the winner (DESIGN.md 8e.1 has the argument).
//
// The tree is implicit: a caller-given order of the triangles, cut into chunks of RC_CHUNK records (the leaves), and above
// them levels of fan-out 8.  Nothing in the buffer is a pointer or an index that addresses memory:
//   records   nrec x 3 float4, record j = (a, 0), (e1, 0), (e2, 0) of face order[j] (rc_record of fgc_raycast.h)
//   face_of   nrec x int32, order[j] (-1 behind nf)
//   nodes     node (L, k), L = 1 .. depth, k < n[L]: the boxes of its 8 children, 8 x (lo.xyz, hi.xyz) = 48 dwords, three
//             16-dword scalar loads like a chunk of records.  The children of (1, k) are the leaves 8k .. 8k + 7, those of
//             (L, k) the nodes (L - 1, 8k .. 8k + 7); a missing child is the empty box (+inf, -inf).  n[0] = leaves,
//             n[L] = ceil(n[L - 1] / 8), depth = the first L with n[L] = 1; level L starts at node noff[L].
//
// rt_leaf_kernel   one thread per leaf box (padding included): its four records, their face ids, and the exact min / max over
//                  the ORIGINAL vertices of its valid, finite faces.
// rt_level_kernel  one launch per level above, one thread per box: the union of its 8 children (min / max: exact).
// rt_cast_kernel   one wave of 64 rays per workgroup, one ray per lane, the walk the wave's (fgc_treewalk.h).  A lane takes
//                  part in a node only if ITS ray met that node and every node above it, tests a leaf's records only if
//                  its ray meets the leaf's box within [t_min, best_t] at that moment, and keeps the smallest (t, face_of)
//                  in full key order.  Children go in index order, so the leaves a lane tests, and in which order, are what
//                  its own ray would visit walking alone: the result of a ray does not depend on its neighbours, the launch
//                  or the order of the rays.
// The stack, the bounded pop, the node and leaf loads and the push are the steps of fgc_treewalk.h, which argues why a walk
// ends and stays in bounds; what is here is the ray's: the slab test, `entry <= best_t`, index order, rc_uvt.
#include "fgc_treewalk.h"         // the walk's steps, and through fgc_raytree.h the layout: RtShape, rt_layout, the RT_ constants

#pragma clang fp contract(off)

namespace fgc {

__device__ __forceinline__ bool rt_finite3(const float* p) {
    return fabsf(p[0]) < __builtin_inff() && fabsf(p[1]) < __builtin_inff() && fabsf(p[2]) < __builtin_inff();
}

// one thread per box of level 0, padding included (nbox = 8 n[1])
__global__ __launch_bounds__(256) void rt_leaf_kernel(const float* __restrict__ verts, int nv, const int* __restrict__ faces,
                                                      int nf, const int* __restrict__ order, int nleaf, int nbox,
                                                      f32x4* __restrict__ rec, int* __restrict__ face_of,
                                                      float* __restrict__ box) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nbox) return;
    float lo[3] = {__builtin_inff(), __builtin_inff(), __builtin_inff()};
    float hi[3] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
    if (i < nleaf) {
#pragma unroll
        for (int k = 0; k < RC_CHUNK; ++k) {
            const int j = RC_CHUNK * i + k;
            const int f = j < nf ? order[j] : -1;
            f32x4 r0, r1, r2;
            float v[3][3];
            if (rc_record(verts, nv, faces, nf, f, r0, r1, r2, v) && rt_finite3(v[0]) && rt_finite3(v[1]) && rt_finite3(v[2])) {
#pragma unroll
                for (int x = 0; x < 3; ++x) {
                    lo[x] = fminf(lo[x], fminf(v[0][x], fminf(v[1][x], v[2][x])));
                    hi[x] = fmaxf(hi[x], fmaxf(v[0][x], fmaxf(v[1][x], v[2][x])));
                }
            }
            rec[3 * (size_t)j] = r0, rec[3 * (size_t)j + 1] = r1, rec[3 * (size_t)j + 2] = r2;
            face_of[j] = f;
        }
    }
    float* b = box + 6 * (size_t)i;
    b[0] = lo[0], b[1] = lo[1], b[2] = lo[2], b[3] = hi[0], b[4] = hi[1], b[5] = hi[2];
}

// one thread per box of a level above the leaves, padding included: the union of children 8i .. 8i + 7 (all stored: the
// level below is padded to whole nodes)
__global__ __launch_bounds__(256) void rt_level_kernel(const float* __restrict__ child, int n, int nbox, float* __restrict__ box) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nbox) return;
    float lo[3] = {__builtin_inff(), __builtin_inff(), __builtin_inff()};
    float hi[3] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
    if (i < n) {
        const float* c = child + 6 * (size_t)RT_FAN * i;
#pragma unroll
        for (int k = 0; k < RT_FAN; ++k)
#pragma unroll
            for (int x = 0; x < 3; ++x) lo[x] = fminf(lo[x], c[6 * k + x]), hi[x] = fmaxf(hi[x], c[6 * k + 3 + x]);
    }
    float* b = box + 6 * (size_t)i;
    b[0] = lo[0], b[1] = lo[1], b[2] = lo[2], b[3] = hi[0], b[4] = hi[1], b[5] = hi[2];
}

// The slab test (include/fgc.h has the argument).  Per axis t1 = (lo - o) inv, t2 = (hi - o) inv, inv = 1 / d in IEEE; the
// nearer of the two is chosen by the sign of inv, never by comparing them, so a NaN (0 x inf: the ray lies in that plane)
// stays on its own side and fmaxf / fminf, which return the operand that is no NaN, drop it: that plane does not constrain.
// Returns the widened near end of the interval if [near', far'] is not empty and reaches t_min, a NaN otherwise; the lane
// meets the box iff that value <= best_t (false for a NaN).
__device__ __forceinline__ float rt_entry(const float (&o)[3], const float (&inv)[3], const bool (&neg)[3], const float* lo,
                                          const float* hi, float t_min) {
    float tn[3], tf[3];
#pragma unroll
    for (int x = 0; x < 3; ++x) {
        const float t1 = (lo[x] - o[x]) * inv[x], t2 = (hi[x] - o[x]) * inv[x];
        tn[x] = neg[x] ? t2 : t1;
        tf[x] = neg[x] ? t1 : t2;
    }
    const float near = fmaxf(fmaxf(tn[0], tn[1]), tn[2]);
    const float far = fminf(fminf(tf[0], tf[1]), tf[2]);
    const float nw = near - __builtin_fmaf(fabsf(near), RT_SLACK, RT_TINY);
    const float fw = far + __builtin_fmaf(fabsf(far), RT_SLACK, RT_TINY);
    return (nw <= fw && fw >= t_min) ? nw : __builtin_nanf("");
}

// grid ceil(nq / 64), 64 threads: one wave.  COUNT: the probe-only build (-DFGC_RT_COUNT) also writes, per ray, the pairs
// its lane tested and the boxes it tested.
template <bool COUNT>
__global__ __launch_bounds__(64) void rt_cast_kernel(const f32x4* __restrict__ rec, const int* __restrict__ face_of,
                                                     const f32x4* __restrict__ boxes, const RtShape S, unsigned nodes,
                                                     const float* __restrict__ origins, int n_origins,
                                                     const float* __restrict__ dirs, int nq, float t_min,
                                                     float* __restrict__ t_out, int* __restrict__ face_out,
                                                     float* __restrict__ bary_out, unsigned* __restrict__ count_out) {
    __shared__ RtWave W;
    const int lane = threadIdx.x;
    const int q = blockIdx.x * 64 + lane;
    const bool live = q < nq;
    float o[3], d[3];
    rc_load_ray(origins, n_origins, dirs, q, live, o, d);
    const float inv[3] = {1.f / d[0], 1.f / d[1], 1.f / d[2]};
    const bool neg[3] = {inv[0] < 0.f, inv[1] < 0.f, inv[2] < 0.f};
    float best_t = __builtin_inff(), best_u = 0.f, best_v = 0.f;
    int best_f = -1;
    unsigned n_pairs = 0, n_boxes = 0;
    const int depth = min(max(S.depth, 1), RT_MAX_LEVELS);

    int sp = rt_start(W, depth, live);
    for (unsigned it = 0; it < nodes && sp > 0; ++it) {
        int L, k;
        bool active;
        if (!rt_pop(W, sp, S, depth, L, k, active)) continue;
        float bx[RT_FAN * 6];
        rt_node(boxes, S, L, k, bx);
        float en[RT_FAN];
#pragma unroll
        for (int c = 0; c < RT_FAN; ++c) en[c] = active ? rt_entry(o, inv, neg, bx + 6 * c, bx + 6 * c + 3, t_min) : __builtin_nanf("");
        if (COUNT && active) n_boxes += RT_FAN;
        if (L > 1) {
            // push in falling order: child 0 is popped first
#pragma unroll
            for (int c = RT_FAN - 1; c >= 0; --c) rt_push(W, sp, L, RT_FAN * k + c, __ballot(en[c] <= best_t));
        } else {
#pragma unroll
            for (int c = 0; c < RT_FAN; ++c) W.ent[c][lane] = en[c];
#pragma unroll 1
            for (int c = 0; c < RT_FAN; ++c) {
                const int leaf = RT_FAN * k + c;
                if (leaf >= S.nleaf) break;
                const bool meet = W.ent[c][lane] <= best_t;          // best_t as it is NOW: earlier leaves have shrunk it
                if (__ballot(meet) == 0) continue;
                f32x4 r[3 * RC_CHUNK];
                int fid[RC_CHUNK];
                rt_leaf(rec, face_of, leaf, r, fid);
                if (meet) {
                    if (COUNT) n_pairs += RC_CHUNK;
#pragma unroll
                    for (int x = 0; x < RC_CHUNK; ++x) {
                        float u, v, t;
                        if (rc_uvt(o, d, r[3 * x], r[3 * x + 1], r[3 * x + 2], t_min, u, v, t) &&
                            (t < best_t || (t == best_t && fid[x] < best_f)))
                            best_t = t, best_f = fid[x], best_u = u, best_v = v;
                    }
                }
            }
        }
    }
    if (!live) return;
    t_out[q] = best_t;
    face_out[q] = best_f;
    if (bary_out) bary_out[2 * (size_t)q] = best_u, bary_out[2 * (size_t)q + 1] = best_v;
    if (COUNT && count_out) count_out[2 * (size_t)q] = n_pairs, count_out[2 * (size_t)q + 1] = n_boxes;
}

static int rt_cast(const char* what, const void* tree, size_t tree_bytes, int32_t nf, const float* origins, int32_t n_origins,
                   const float* dirs, int32_t nq, float t_min, float* t_out, int32_t* face_out, float* bary_out,
                   unsigned* count_out, void* stream) {
    FGC_CHECK_ARG(tree && origins && dirs && t_out && face_out, "%s: null pointer", what);
    FGC_CHECK_ARG(nf > 0 && nq > 0, "%s: nf=%d nq=%d (both > 0)", what, nf, nq);
    FGC_CHECK_ARG(nf <= FGC_RAY_CAST_MAX_FACES, "%s: nf=%d (at most %d)", what, nf, FGC_RAY_CAST_MAX_FACES);
    FGC_CHECK_ARG(n_origins == 1 || n_origins == nq, "%s: n_origins=%d (1 or nq=%d)", what, n_origins, nq);
    FGC_CHECK_ARG(t_min >= 0.f && t_min < __builtin_inff(), "%s: t_min=%g (>= 0 and finite)", what, (double)t_min);
    RtView T;
    if (int rc = rt_view(what, tree, tree_bytes, nf, T)) return rc;
    FGC_LAUNCH("rt_cast_kernel", (hipStream_t)stream, RT_COUNT_KERNEL(rt_cast_kernel, count_out), dim3(cdiv(nq, 64)), dim3(64), 0,
               T.rec, T.face_of, T.boxes, T.s, T.nodes, origins, n_origins, dirs, nq, t_min, t_out, face_out, bary_out, count_out);
    FGC_CHECK_LAUNCH(what);
    return FGC_OK;
}

}  // namespace fgc

using namespace fgc;

extern "C" size_t fgc_ray_tree_bytes(int32_t nf) {
    if (nf <= 0 || nf > FGC_RAY_CAST_MAX_FACES) return 0;
    return rt_layout(nf).total;
}

extern "C" int fgc_ray_tree_build(const float* verts, int32_t nv, const int32_t* faces, int32_t nf, const int32_t* order,
                                  void* tree, size_t tree_bytes, void* stream) {
    FGC_CHECK_ARG(verts && faces && order && tree, "fgc_ray_tree_build: null pointer");
    FGC_CHECK_ARG(nv > 0 && nf > 0, "fgc_ray_tree_build: nv=%d nf=%d (both > 0)", nv, nf);
    FGC_CHECK_ARG(nf <= FGC_RAY_CAST_MAX_FACES, "fgc_ray_tree_build: nf=%d (at most %d)", nf, FGC_RAY_CAST_MAX_FACES);
    RtView T;
    if (int rc = rt_view("fgc_ray_tree_build", tree, tree_bytes, nf, T)) return rc;
    hipStream_t st = (hipStream_t)stream;
    // the one place that writes a tree; the boxes of level L: the nodes of L + 1
    auto level = [&](int L) { return (float*)T.boxes + (size_t)T.s.noff[L + 1] * RT_FAN * 6; };
    const int nbox0 = RT_FAN * T.s.n[1];
    FGC_LAUNCH("rt_leaf_kernel", st, rt_leaf_kernel, dim3(cdiv(nbox0, 256)), dim3(256), 0, verts, nv, faces, nf, order, T.s.nleaf,
               nbox0, (f32x4*)T.rec, (int*)T.face_of, level(0));
    for (int L = 1; L < T.s.depth; ++L) {
        const int nbox = RT_FAN * T.s.n[L + 1];
        FGC_LAUNCH("rt_level_kernel", st, rt_level_kernel, dim3(cdiv(nbox, 256)), dim3(256), 0, (const float*)level(L - 1),
                   T.s.n[L], nbox, level(L));
    }
    FGC_CHECK_LAUNCH("fgc_ray_tree_build");
    return FGC_OK;
}

extern "C" int fgc_ray_cast_tree(const void* tree, size_t tree_bytes, int32_t nf, const float* origins, int32_t n_origins,
                                 const float* dirs, int32_t nq, float t_min, float* t_out, int32_t* face_out, float* bary_out,
                                 void* stream) {
    return rt_cast("fgc_ray_cast_tree", tree, tree_bytes, nf, origins, n_origins, dirs, nq, t_min, t_out, face_out, bary_out,
                   nullptr, stream);
}

#ifdef FGC_RT_COUNT
// probe-only build (tools/ray_cast_probe.py --tree): the same cast, plus count_out [nq,2] = (pairs, boxes) each ray's lane tested
extern "C" int fgc_ray_cast_tree_count(const void* tree, size_t tree_bytes, int32_t nf, const float* origins, int32_t n_origins,
                                       const float* dirs, int32_t nq, float t_min, float* t_out, int32_t* face_out,
                                       float* bary_out, uint32_t* count_out, void* stream) {
    FGC_CHECK_ARG(count_out, "fgc_ray_cast_tree_count: null pointer");
    return rt_cast("fgc_ray_cast_tree_count", tree, tree_bytes, nf, origins, n_origins, dirs, nq, t_min, t_out, face_out,
                   bary_out, count_out, stream);
}
#endif
