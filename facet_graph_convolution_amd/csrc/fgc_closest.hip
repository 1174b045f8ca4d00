// Closest point on a triangle mesh through the bounding-box tree of fgc_ray_tree_build (build extension; include/fgc.h:
// fgc_closest_point_tree): for every point the smallest (dist2, face) over all records, at a cost that does not grow with
// points x faces.  The per-pair arithmetic is cp_pair of fgc_closest.h whether a box was culled around the pair or not, and a
// box is skipped only if a lower bound that never exceeds the COMPUTED dist2 of a record inside it is > the lane's best: the
// tree returns bit for bit what FGC_CP_EXHAUSTIVE returns (include/fgc.h and DESIGN.md 8e.2 have the argument).
//
// cp_kernel   one wave of 64 points per workgroup, one point per lane, the walk of rt_cast_kernel (fgc_treewalk.h).  A lane
//             takes part in a child only while lower bound <= its best dist2.  The children of a node are visited
//             nearest-first by the wave's smallest (bound, distance to the middle of the box) over the lanes that take part
//             (the farthest is pushed first), after one greedy walk that gives every lane a finite best: a good bound early.
//             The order and the greedy walk change the time and, by the invariant above, not one bit.
// The stack, the bounded pop, the node and leaf loads and the push are the steps of fgc_treewalk.h, which argues why a walk
// ends and stays in bounds; what is here is the point's: cp_lower, the greedy mask, the wave's order, the skip, cp_pair.
#include "fgc_closest.h"
#include "fgc_treewalk.h"

#pragma clang fp contract(off)

namespace fgc {

constexpr float CP_ABS = 0x1p-18f;          // the absolute slack of a per-axis gap, in units of the largest coordinate

// The lower bound of dist2 over the records of a box (include/fgc.h has the argument).  Per axis the gap
// g = max(lo - q, q - hi, 0) is deflated by CP_ABS max(|lo|, |hi|, |q|) and clamped at 0; the sum of the squares is deflated
// relatively as the slab test does.  An empty box (+inf, -inf) or a NaN point gives a NaN: no comparison admits it.
// cen2: the squared distance from q to the middle of the box, which only ORDERS the visit (any value would do).
__device__ __forceinline__ float cp_lower(const float (&q)[3], const float* lo, const float* hi, float& cen2) {
    float s = 0.f;
    cen2 = 0.f;
#pragma unroll
    for (int x = 0; x < 3; ++x) {
        float g = lo[x] - q[x];          // comparisons, not fmaxf, which would drop a NaN: a NaN point must meet no box
        const float t = q[x] - hi[x];
        g = t > g ? t : g;
        g = g < 0.f ? 0.f : g;
        const float m = fmaxf(fmaxf(fabsf(lo[x]), fabsf(hi[x])), fabsf(q[x]));
        float gd = g - m * CP_ABS;          // inf - inf for the empty box: a NaN, and it stays one
        gd = gd < 0.f ? 0.f : gd;
        s = s + gd * gd;
        const float dc = q[x] - 0.5f * (lo[x] + hi[x]);
        cen2 = cen2 + dc * dc;
    }
    const float lb = s - __builtin_fmaf(s, RT_SLACK, RT_TINY);
    return lb < 0.f ? 0.f : lb;
}

// The smallest value of a wave, wave-uniform.  Four DPP steps inside every row of 16 lanes (swap neighbours, swap pairs,
// mirror the half rows, mirror the row: afterwards every lane holds its row's minimum), then one lane of each of the four
// rows is read into SGPRs.  All 64 lanes execute this: the walk's control flow is wave-uniform.
__device__ __forceinline__ unsigned cp_wave_min(unsigned x) {
    x = min(x, (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0xB1, 0xF, 0xF, false));           // quad_perm [1, 0, 3, 2]
    x = min(x, (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0x4E, 0xF, 0xF, false));           // quad_perm [2, 3, 0, 1]
    x = min(x, (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0x141, 0xF, 0xF, false));          // row_half_mirror
    x = min(x, (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0x140, 0xF, 0xF, false));          // row_mirror
    const unsigned a = (unsigned)__builtin_amdgcn_readlane((int)x, 0), b = (unsigned)__builtin_amdgcn_readlane((int)x, 16);
    const unsigned c = (unsigned)__builtin_amdgcn_readlane((int)x, 32), d = (unsigned)__builtin_amdgcn_readlane((int)x, 48);
    return min(min(a, b), min(c, d));
}

// grid ceil(nq / 64), 64 threads: one wave.  all: FGC_CP_EXHAUSTIVE, every bound counts as 0.  COUNT: the probe-only build
// (-DFGC_CP_COUNT) also writes, per point, the pairs its lane tested and the boxes it tested, and what its WAVE did: the nodes
// it popped and the leaves whose records it loaded.
template <bool COUNT>
__global__ __launch_bounds__(64) void cp_kernel(const f32x4* __restrict__ rec, const int* __restrict__ face_of,
                                                const f32x4* __restrict__ boxes, const RtShape S, unsigned nodes,
                                                const float* __restrict__ points, int nq, int all,
                                                float* __restrict__ dist2_out, int* __restrict__ face_out,
                                                float* __restrict__ bary_out, unsigned* __restrict__ count_out) {
    __shared__ RtWave W;
    const int lane = threadIdx.x;
    const int i = blockIdx.x * 64 + lane;
    const bool live = i < nq;
    // A lane beyond nq is left out of the root's ballot and stores nothing; it holds the LAST point all the same, so that it
    // cannot widen the wave's walk (with the origin there, the last wave of 500 000 points on a torus walked 8 864 leaves
    // towards the middle of the hole and set the kernel's time: 25.8 -> 3.0 ms).
    const size_t ip = (size_t)min(i, nq - 1);
    const float q[3] = {points[3 * ip], points[3 * ip + 1], points[3 * ip + 2]};
    float best = __builtin_inff(), best_u = 0.f, best_v = 0.f;
    int best_f = -1;
    unsigned n_pairs = 0, n_boxes = 0, w_nodes = 0, w_leaves = 0;
    const int depth = min(max(S.depth, 1), RT_MAX_LEVELS);

    // Two walks.  The first is greedy: in every node a lane follows only its OWN nearest child (the first among equals), down
    // to one leaf - the wave visits the union of those paths - and comes back with a finite best of its own neighbourhood.
    // The second is the search, with that bound from the start; without the first, a lane's best stays loose until the
    // wave's order reaches its corner of the tree.  Whatever the first walk finds is the result of a pair the search may
    // test again (the same bits): it changes the time only.  FGC_CP_EXHAUSTIVE runs the second walk alone.
#pragma unroll 1
    for (int pass = all ? 1 : 0; pass < 2; ++pass) {
        const bool greedy = pass == 0;
        int sp = rt_start(W, depth, live);
        for (unsigned it = 0; it < nodes && sp > 0; ++it) {
            int L, k;
            bool active;
            if (!rt_pop(W, sp, S, depth, L, k, active)) continue;
            float bx[RT_FAN * 6];
            rt_node(boxes, S, L, k, bx);
            const int nchild = S.n[L - 1];          // the boxes of the level below (the leaves for L = 1)
            if (COUNT && active) n_boxes += RT_FAN;
            if (COUNT) ++w_nodes;
            // the bounds, and per child the smallest over the lanes that take part: the order of the visit
            // Nearest by (bound, distance to the MIDDLE of the box): a point near the surface lies inside several boxes (bound 0
            // for all of them), among them the wide ones of leaves where the Morton order jumps, whose triangles are far away;
            // the middle tells them apart.
            unsigned key[RT_FAN], key2[RT_FAN];
            float lbv[RT_FAN], cen[RT_FAN];
            int mine = -1;          // the greedy walk: the lane's nearest child, the first among equals
            float near_lb = __builtin_inff(), near_cen = __builtin_inff();
#pragma unroll
            for (int c = 0; c < RT_FAN; ++c) {
                cen[c] = 0.f;
                lbv[c] = !active ? __builtin_nanf("") : all ? 0.f : cp_lower(q, bx + 6 * c, bx + 6 * c + 3, cen[c]);
                if (lbv[c] < near_lb || (lbv[c] == near_lb && cen[c] < near_cen)) near_lb = lbv[c], near_cen = cen[c], mine = c;
            }
#pragma unroll
            for (int c = 0; c < RT_FAN; ++c) {
                const float lb = (greedy && c != mine) ? __builtin_nanf("") : lbv[c];
                W.ent[c][lane] = lb;
                const bool in = lb <= best && lb < __builtin_inff();
                key[c] = cp_wave_min(in ? __float_as_uint(lb) : 0xFFFFFFFFu);
                key2[c] = cp_wave_min(in && __float_as_uint(lb) == key[c] ? __float_as_uint(cen[c]) : 0xFFFFFFFFu);
            }
            // rank of every child among the eight (wave-uniform, ties by index); ord holds child c at nibble rank(c)
            unsigned ord = 0;
#pragma unroll
            for (int c = 0; c < RT_FAN; ++c) {
                int rank = 0;
#pragma unroll
                for (int j = 0; j < RT_FAN; ++j)
                    rank += (key[j] < key[c] || (key[j] == key[c] && (key2[j] < key2[c] || (key2[j] == key2[c] && j < c)))) ? 1 : 0;
                ord |= (unsigned)c << (4 * rank);
            }
            if (L > 1) {
                // push the farthest first: the nearest is popped first
#pragma unroll 1
                for (int r = RT_FAN - 1; r >= 0; --r) {
                    const int c = (int)((ord >> (4 * r)) & 7u);
                    const int child = RT_FAN * k + c;
                    if (child >= nchild) continue;
                    const float lb = W.ent[c][lane];
                    rt_push(W, sp, L, child, __ballot(lb <= best && lb < __builtin_inff()));
                }
            } else {
#pragma unroll 1
                for (int r = 0; r < RT_FAN; ++r) {
                    const int c = (int)((ord >> (4 * r)) & 7u);
                    const int leaf = RT_FAN * k + c;
                    if (leaf >= nchild || leaf >= S.nleaf) continue;
                    const float lb = W.ent[c][lane];
                    const bool meet = lb <= best && lb < __builtin_inff();          // best as it is NOW: earlier leaves have shrunk it
                    if (__ballot(meet) == 0) continue;
                    if (COUNT) ++w_leaves;
                    f32x4 rr[3 * RC_CHUNK];
                    int fid[RC_CHUNK];
                    rt_leaf(rec, face_of, leaf, rr, fid);
#pragma unroll
                    for (int x = 0; x < RC_CHUNK; ++x) {
                        const f32x4 e1 = rr[3 * x + 1], e2 = rr[3 * x + 2];
                        // a triangle collapsed to a point - an invalid row, the padding - takes no part (wave-uniform)
                        // (the six are +-0 iff the OR of their bits without the signs is 0: scalar integer work)
                        if (((__float_as_uint(e1.x) | __float_as_uint(e1.y) | __float_as_uint(e1.z) | __float_as_uint(e2.x) |
                              __float_as_uint(e2.y) | __float_as_uint(e2.z)) << 1) == 0u) continue;
                        if (meet) {
                            if (COUNT) ++n_pairs;
                            float u, v;
                            const float d = cp_pair(q, rr[3 * x], e1, e2, u, v);
                            if (d < __builtin_inff() && (d < best || (d == best && fid[x] < best_f)))
                                best = d, best_f = fid[x], best_u = u, best_v = v;
                        }
                    }
                }
            }
        }
    }
    if (!live) return;
    dist2_out[i] = best;
    face_out[i] = best_f;
    if (bary_out) bary_out[2 * (size_t)i] = best_u, bary_out[2 * (size_t)i + 1] = best_v;
    if (COUNT && count_out) {
        count_out[4 * (size_t)i] = n_pairs, count_out[4 * (size_t)i + 1] = n_boxes;
        count_out[4 * (size_t)i + 2] = w_nodes, count_out[4 * (size_t)i + 3] = w_leaves;
    }
}

static int cp_query(const char* what, const void* tree, size_t tree_bytes, int32_t nf, const float* points, int32_t nq,
                    uint32_t flags, float* dist2_out, int32_t* face_out, float* bary_out, unsigned* count_out, void* stream) {
    FGC_CHECK_ARG(tree && points && dist2_out && face_out, "%s: null pointer", what);
    FGC_CHECK_ARG(nf > 0 && nq > 0, "%s: nf=%d nq=%d (both > 0)", what, nf, nq);
    FGC_CHECK_ARG(nf <= FGC_RAY_CAST_MAX_FACES, "%s: nf=%d (at most %d)", what, nf, FGC_RAY_CAST_MAX_FACES);
    FGC_CHECK_ARG((flags & ~FGC_CP_EXHAUSTIVE) == 0, "%s: unknown flags 0x%x", what, flags);
    RtView T;
    if (int rc = rt_view(what, tree, tree_bytes, nf, T)) return rc;
    FGC_LAUNCH("cp_kernel", (hipStream_t)stream, RT_COUNT_KERNEL(cp_kernel, count_out), dim3(cdiv(nq, 64)), dim3(64), 0, T.rec,
               T.face_of, T.boxes, T.s, T.nodes, points, nq, (int)(flags & FGC_CP_EXHAUSTIVE), dist2_out, face_out, bary_out, count_out);
    FGC_CHECK_LAUNCH(what);
    return FGC_OK;
}

}  // namespace fgc

using namespace fgc;

extern "C" int fgc_closest_point_tree(const void* tree, size_t tree_bytes, int32_t nf, const float* points, int32_t nq,
                                      uint32_t flags, float* dist2_out, int32_t* face_out, float* bary_out, void* stream) {
    return cp_query("fgc_closest_point_tree", tree, tree_bytes, nf, points, nq, flags, dist2_out, face_out, bary_out, nullptr,
                    stream);
}

#ifdef FGC_CP_COUNT
// probe-only build (tools/closest_probe.py): the same query, plus count_out [nq,4] = (pairs, boxes) each point's lane tested and
// (nodes popped, leaves loaded) of its wave
extern "C" int fgc_closest_point_tree_count(const void* tree, size_t tree_bytes, int32_t nf, const float* points, int32_t nq,
                                            uint32_t flags, float* dist2_out, int32_t* face_out, float* bary_out,
                                            uint32_t* count_out, void* stream) {
    FGC_CHECK_ARG(count_out, "fgc_closest_point_tree_count: null pointer");
    return cp_query("fgc_closest_point_tree_count", tree, tree_bytes, nf, points, nq, flags, dist2_out, face_out, bary_out,
                    count_out, stream);
}
#endif
