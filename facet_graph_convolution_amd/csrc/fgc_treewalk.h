// The steps that the two walks of a wave of 64 queries through the bounding-box tree of fgc_ray_tree_build share
// (fgc_raytree.h: the layout).  The ray cast (fgc_raytree.hip) and the closest-point query (fgc_closest.hip) keep a loop each,
// in which a lane decides what it is admitted to and in which order the children go; whatever touches the stack, a node or
// a leaf is here, once.  The stack of (node, ballot of the lanes admitted to it) lives in the wave's LDS and is popped into
// SGPRs, so boxes and records come through scalar loads and the control flow is wave-uniform.  What every walk rests on:
//   - No loop ends on device data: `for (it < nodes && sp > 0)` pops at most `nodes` times (a host-side count; a walk pushes
//     each node at most once), every loop inside a pop has RT_FAN or RC_CHUNK rounds.
//   - Every popped id is bounded before it addresses anything (rt_pop), the wave's own or not; a leaf by its caller.
//   - The stack holds at most 7 entries per level + 1 = RT_STACK, and rt_push writes nothing at sp >= RT_STACK.
//   - A dead lane takes part in no ballot: rt_start's mask is the ballot of `live`; every other mask is a ballot on an
//     entry value that the caller makes a NaN for a lane outside the popped mask (`active`).
#pragma once
#include "fgc_raytree.h"

namespace fgc {

// the wave's LDS, __shared__, one per workgroup of 64 threads (the order and the alignment are those the three arrays had)
struct RtWave {
    float ent[RT_FAN][64];                              // a leaf node's entry values, one row per child
    unsigned long long st_mask[RT_STACK];               // the lanes that were admitted to that node
    alignas(16) unsigned st_id[RT_STACK];               // (L << 28) | k
};

// the root on the stack; returns sp
__device__ __forceinline__ int rt_start(RtWave& W, int depth, bool live) {
    W.st_id[0] = (unsigned)depth << 28;
    W.st_mask[0] = __ballot(live);
    return 1;
}

// Pops into SGPRs: node (L, k) and whether this lane was admitted to it.  False for an id out of bounds (nothing to visit).
__device__ __forceinline__ bool rt_pop(const RtWave& W, int& sp, const RtShape& S, int depth, int& L, int& k, bool& active) {
    const unsigned* st_id = W.st_id;
    const unsigned long long* st_mask = W.st_mask;
    --sp;
    const unsigned long long mask_v = st_mask[sp];
    const unsigned id = __builtin_amdgcn_readfirstlane(st_id[sp]);
    const unsigned long long mask = ((unsigned long long)__builtin_amdgcn_readfirstlane((unsigned)(mask_v >> 32)) << 32) |
                                    __builtin_amdgcn_readfirstlane((unsigned)mask_v);
    L = (int)(id >> 28), k = (int)(id & 0x0FFFFFFFu);
    active = (mask >> threadIdx.x) & 1ull;
    return !(L < 1 || L > depth || k >= S.n[L]);
}

// the boxes of the 8 children of node (L, k), bounded by rt_pop: 12 f32x4 through scalar loads (wave-uniform address)
__device__ __forceinline__ void rt_node(const f32x4* __restrict__ boxes, const RtShape& S, int L, int k, float (&bx)[RT_FAN * 6]) {
    const f32x4* nb = boxes + (size_t)(S.noff[L] + (unsigned)k) * RT_NODE_F4;
    f32x4 b4[RT_NODE_F4];
#pragma unroll
    for (int x = 0; x < RT_NODE_F4; ++x) b4[x] = nb[x];
#pragma unroll
    for (int x = 0; x < RT_NODE_F4; ++x) bx[4 * x] = b4[x].x, bx[4 * x + 1] = b4[x].y, bx[4 * x + 2] = b4[x].z, bx[4 * x + 3] = b4[x].w;
}

// child `child` of a node of level L onto the stack, if some lane was admitted to it (m) and there is room
__device__ __forceinline__ void rt_push(RtWave& W, int& sp, int L, int child, unsigned long long m) {
    if (m != 0 && sp < RT_STACK) {
        W.st_id[sp] = ((unsigned)(L - 1) << 28) | (unsigned)child;
        W.st_mask[sp] = m;
        ++sp;
    }
}

// the RC_CHUNK records and face ids of leaf `leaf` (< nleaf: the caller's check) through scalar loads
__device__ __forceinline__ void rt_leaf(const f32x4* __restrict__ rec, const int* __restrict__ face_of, int leaf,
                                        f32x4 (&r)[3 * RC_CHUNK], int (&fid)[RC_CHUNK]) {
    const f32x4* rb = rec + 3 * (size_t)RC_CHUNK * leaf;
    const int* fb = face_of + (size_t)RC_CHUNK * leaf;
#pragma unroll
    for (int x = 0; x < 3 * RC_CHUNK; ++x) r[x] = rb[x];
#pragma unroll
    for (int x = 0; x < RC_CHUNK; ++x) fid[x] = fb[x];
}

// ---- the host's side ----
// A tree buffer as typed pointers (read-only: the builder alone casts the const away), the kernels' shape and the pop bound.
struct RtView {
    const f32x4 *rec, *boxes;
    const int* face_of;
    RtShape s;
    unsigned nodes;
};

// The alignment and size checks every entry point makes of (tree, tree_bytes), and the view.  nf within
// (0, FGC_RAY_CAST_MAX_FACES] is the caller's to have checked: rt_layout counts on it.
static inline int rt_view(const char* what, const void* tree, size_t tree_bytes, int32_t nf, RtView& v) {
    FGC_CHECK_ARG((uintptr_t)tree % 16 == 0, "%s: tree needs 16-byte alignment", what);
    const RtLayout T = rt_layout(nf);
    FGC_CHECK_ARG(tree_bytes >= T.total, "%s: tree too small (%zu < %zu bytes)", what, tree_bytes, T.total);
    const char* base = (const char*)tree;
    v = RtView{(const f32x4*)base, (const f32x4*)(base + T.boxes), (const int*)(base + T.face_of), T.s, T.nodes};
    return FGC_OK;
}

// kernel<true> where a probe-only build (-DFGC_RT_COUNT, -DFGC_CP_COUNT) was asked for counters; the library holds kernel<false>
#if defined(FGC_RT_COUNT) || defined(FGC_CP_COUNT)
#define RT_COUNT_KERNEL(kernel, count_out) ((count_out) ? kernel<true> : kernel<false>)
#else
#define RT_COUNT_KERNEL(kernel, count_out) kernel<false>
#endif

}  // namespace fgc
