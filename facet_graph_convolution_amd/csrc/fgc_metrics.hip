// Nearest neighbour over point sets (the distance scan of hausdorffOverSampled, utils.py:816-1006; exact distances of
// utils.mesh_distances).
//
// Tiled brute force.  A workgroup owns NQ_WG queries (QPL per lane, held as packed float2 pairs) and one contiguous slice
// of the candidates (blockIdx.y): the candidate split gives enough workgroups at any shape.  Candidates are wave-uniform:
// a chunk of CHUNK points (and their cells) is fetched with scalar loads and reaches the VALU from SGPRs.  Per candidate
// and pair of queries: 3 v_pk_add_f32 (differences), 3 v_pk_mul_f32 (squares), 2 v_pk_add_f32 ((dx^2 + dy^2) + dz^2, the
// reference's order), then per query v_cmp_lt + v_min + v_cndmask: 7 VALU instructions per pair.  Contraction is off in
// this file, so the squared distance is the correctly rounded fp32 value of that expression, as numpy computes it.
//
// Ties: a lane keeps the first strictly smaller candidate of its slice (lowest index in the slice); the slices merge in
// one 64-bit key per query, fp32 bits of d2 (non-negative, so its bits order like its value) above the index, with a
// global 64-bit atomicMin: the smallest d2, and among equal d2 the lowest index, whatever the split.
#include "fgc_common.h"

#pragma clang fp contract(off)

namespace fgc {

typedef float f2 __attribute__((ext_vector_type(2)));

constexpr int NN_THREADS = 256;
constexpr int NN_QPL = 4;                                // queries per lane (two packed pairs)
constexpr int NN_Q_WG = NN_THREADS * NN_QPL;             // queries per workgroup
constexpr int NN_CHUNK = 16;                             // candidates per scalar-load chunk
constexpr unsigned NN_CELL_STEP = (1u << 20) | (1u << 10) | 1u;   // a +1 step in every packed coordinate

// a candidate of packed cell pc is admissible for a query of packed cell qc iff every coordinate of pc - qc is 0 or 1
// (coordinates < 512 in 10-bit fields: the field differences lie in (-512, 512), so the packed difference determines them)
__device__ __forceinline__ bool nn_cell_ok(int qc, int pc) {
    const unsigned d = (unsigned)pc - (unsigned)qc;
    return (d & ~NN_CELL_STEP) == 0u;
}

template <bool MASKED>
__device__ __forceinline__ void nn_visit(const f2 (&qx)[NN_QPL / 2], const f2 (&qy)[NN_QPL / 2], const f2 (&qz)[NN_QPL / 2],
                                         const int (&qc)[NN_QPL], float (&best)[NN_QPL], int (&bi)[NN_QPL], float px,
                                         float py, float pz, int pc, int j) {
#pragma unroll
    for (int h = 0; h < NN_QPL / 2; ++h) {
        const f2 dx = qx[h] - px, dy = qy[h] - py, dz = qz[h] - pz;
        const f2 d2 = (dx * dx + dy * dy) + dz * dz;
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int q = 2 * h + e;
            const float v = e ? d2.y : d2.x;
            bool lt = v < best[q];
            if (MASKED) lt = lt && nn_cell_ok(qc[q], pc);
            bi[q] = lt ? j : bi[q];
            best[q] = lt ? v : best[q];
        }
    }
}

template <bool MASKED>
__global__ __launch_bounds__(NN_THREADS) void nn_scan_kernel(const float* __restrict__ q, int nq, const float* __restrict__ p,
                                                             int np, const int* __restrict__ q_cell,
                                                             const int* __restrict__ p_cell, int per_split,
                                                             unsigned long long* __restrict__ keys) {
    const int q0 = blockIdx.x * NN_Q_WG + threadIdx.x;
    f2 qx[NN_QPL / 2], qy[NN_QPL / 2], qz[NN_QPL / 2];
    int qc[NN_QPL];
    float best[NN_QPL];
    int bi[NN_QPL];
#pragma unroll
    for (int k = 0; k < NN_QPL; ++k) {
        const int i = q0 + k * NN_THREADS;
        const bool in = i < nq;
        const float x = in ? q[3 * (size_t)i] : 0.f, y = in ? q[3 * (size_t)i + 1] : 0.f, z = in ? q[3 * (size_t)i + 2] : 0.f;
        if (k & 1) {
            qx[k / 2].y = x;
            qy[k / 2].y = y;
            qz[k / 2].y = z;
        } else {
            qx[k / 2].x = x;
            qy[k / 2].x = y;
            qz[k / 2].x = z;
        }
        // out-of-range queries and queries in no cell never accept a candidate: their keys stay "none"
        qc[k] = MASKED ? (in ? q_cell[i] : -1) : 0;
        best[k] = __builtin_inff();
        bi[k] = -1;
    }
    const int j0 = blockIdx.y * per_split;
    const int j1 = min(np, j0 + per_split);
    int j = j0;
    for (; j + NN_CHUNK <= j1; j += NN_CHUNK) {
        const float* pb = p + 3 * (size_t)j;     // wave-uniform: s_load_dwordx16 x 3
        float c[3 * NN_CHUNK];
#pragma unroll
        for (int t = 0; t < 3 * NN_CHUNK; ++t) c[t] = pb[t];
        int cc[NN_CHUNK];
#pragma unroll
        for (int t = 0; t < NN_CHUNK; ++t) cc[t] = MASKED ? p_cell[j + t] : 0;
#pragma unroll
        for (int t = 0; t < NN_CHUNK; ++t)
            nn_visit<MASKED>(qx, qy, qz, qc, best, bi, c[3 * t], c[3 * t + 1], c[3 * t + 2], cc[t], j + t);
    }
    for (; j < j1; ++j) {
        const float* pb = p + 3 * (size_t)j;
        nn_visit<MASKED>(qx, qy, qz, qc, best, bi, pb[0], pb[1], pb[2], MASKED ? p_cell[j] : 0, j);
    }
#pragma unroll
    for (int k = 0; k < NN_QPL; ++k) {
        const int i = q0 + k * NN_THREADS;
        bool take = i < nq && bi[k] >= 0;
        if (MASKED) take = take && qc[k] >= 0;
        if (take) {
            const unsigned long long key =
                ((unsigned long long)__float_as_uint(best[k]) << 32) | (unsigned long long)(unsigned)bi[k];
            atomicMin(keys + i, key);
        }
    }
}

// key -> (sqrt(d2), index); "none" (all ones) -> (+inf, -1).  The square root is taken in double and rounded once to
// fp32: the correctly rounded fp32 square root, as numpy's float32 sqrt.
__global__ __launch_bounds__(256) void nn_finalize_kernel(const unsigned long long* __restrict__ keys, int nq,
                                                          float* __restrict__ dist, int* __restrict__ idx) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq) return;
    const unsigned long long k = keys[i];
    if (k == ~0ull) {
        dist[i] = __builtin_inff();
        idx[i] = -1;
    } else {
        dist[i] = (float)sqrt((double)__uint_as_float((unsigned)(k >> 32)));
        idx[i] = (int)(unsigned)(k & 0xffffffffu);
    }
}

}  // namespace fgc

using namespace fgc;

extern "C" size_t fgc_nn_workspace_bytes(int32_t nq, int32_t np) {
    (void)np;
    return nq > 0 ? (size_t)nq * sizeof(unsigned long long) : 0;
}

extern "C" int fgc_nn_query(const float* q, int32_t nq, const float* p, int32_t np, const int32_t* q_cell,
                            const int32_t* p_cell, float* dist, int32_t* idx, void* workspace, size_t workspace_bytes,
                            void* stream) {
    FGC_CHECK_ARG(q && p && dist && idx && workspace, "fgc_nn_query: null pointer");
    FGC_CHECK_ARG(nq > 0 && np > 0, "fgc_nn_query: nq=%d np=%d (both > 0)", nq, np);
    FGC_CHECK_ARG((q_cell == nullptr) == (p_cell == nullptr), "fgc_nn_query: q_cell and p_cell must be both NULL or both given");
    FGC_CHECK_ARG(workspace_bytes >= fgc_nn_workspace_bytes(nq, np), "fgc_nn_query: workspace too small (%zu < %zu bytes)",
                  workspace_bytes, fgc_nn_workspace_bytes(nq, np));
    FGC_CHECK_ARG((uintptr_t)workspace % 8 == 0, "fgc_nn_query: workspace needs 8-byte alignment");
    hipStream_t st = (hipStream_t)stream;
    unsigned long long* keys = (unsigned long long*)workspace;
    if (hipMemsetAsync(keys, 0xff, (size_t)nq * sizeof(unsigned long long), st) != hipSuccess) {
        fgc::set_error("fgc_nn_query: memset failed");
        return FGC_EHIP;
    }
    // candidate split: about 4096 workgroups in all (16 per CU), slices of at least 256 candidates, multiples of the chunk
    const int qblocks = cdiv(nq, NN_Q_WG);
    int splits = cdiv(4096, qblocks);
    splits = min(splits, max(1, np / 256));
    splits = max(splits, 1);
    const int per_split = cdiv(cdiv(np, splits), NN_CHUNK) * NN_CHUNK;
    splits = cdiv(np, per_split);
    if (q_cell)
        FGC_LAUNCH("nn_scan_kernel_masked", st, nn_scan_kernel<true>, dim3(qblocks, splits), dim3(NN_THREADS), 0, q, nq, p, np,
                   q_cell, p_cell, per_split, keys);
    else
        FGC_LAUNCH("nn_scan_kernel", st, nn_scan_kernel<false>, dim3(qblocks, splits), dim3(NN_THREADS), 0, q, nq, p, np,
                   q_cell, p_cell, per_split, keys);
    FGC_LAUNCH("nn_finalize_kernel", st, nn_finalize_kernel, dim3(cdiv(nq, 256)), dim3(256), 0, keys, nq, dist, idx);
    FGC_CHECK_LAUNCH("fgc_nn_query");
    return FGC_OK;
}
