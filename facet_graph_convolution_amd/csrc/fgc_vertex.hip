// Vertex update from denoised face normals (replaces update_position2, train.py:1467-1557).
//
// One thread per vertex and iteration: walk the vertex' edge slots, fetch the edge record [v1, v2, f1, f2] (one
// 16-byte load), the other endpoint's position and the two face normals, accumulate
//     n_f1 (n_f1 . d) + n_f2 (n_f2 . d),   d = x_other - x_i
// in slot order, x_i += lambda * sum.  Jacobi: every vertex reads the previous iterate, so the iterations ping-pong
// between two buffers and are enqueued back to back on the caller's stream.  Pure gather/stream work: the per-vertex
// footprint is 80 B of slots + 16 B per edge + 12 B per endpoint / normal, HBM- (in practice L2-) bound.
#include "fgc_common.h"

namespace fgc {

// the edge-slot walk of vertex i at (xi0, xi1, xi2): per used slot, in slot order, add(u0, u1, u2) with u = n_f1 (n_f1 . d) +
// n_f2 (n_f2 . d).  The one copy of this loop: both single-scale kernels accumulate through it.
template <class Add>
__device__ __forceinline__ void edge_walk(int i, float xi0, float xi1, float xi2, const float* __restrict__ x, int nv,
                                          const float* __restrict__ nrm, int nf, const int4* __restrict__ emap, int ne,
                                          const int* __restrict__ vemap, int max_edges, Add&& add) {
    const int* slots = vemap + (size_t)i * max_edges;
    for (int s = 0; s < max_edges; ++s) {
        const int e = slots[s];
        if (e < 0 || e >= ne) continue;           // unused slot: the reference adds exact zeros (train.py:1479,1539)
        const int4 em = emap[e];
        const int j = em.x == i ? em.y : em.x;    // the endpoint that is i itself contributes zero (train.py:1523-1526)
        if (j < 0 || j >= nv) continue;
        const float d0 = x[3 * (size_t)j] - xi0, d1 = x[3 * (size_t)j + 1] - xi1, d2 = x[3 * (size_t)j + 2] - xi2;
        float u0 = 0.f, u1 = 0.f, u2 = 0.f;
        if (em.z >= 0 && em.z < nf) {
            const float n0 = nrm[3 * (size_t)em.z], n1 = nrm[3 * (size_t)em.z + 1], n2 = nrm[3 * (size_t)em.z + 2];
            const float dp = (d0 * n0 + d1 * n1) + d2 * n2;
            u0 = n0 * dp;
            u1 = n1 * dp;
            u2 = n2 * dp;
        }
        if (em.w >= 0 && em.w < nf) {              // boundary edges have f2 = -1: zero normal in the reference
            const float n0 = nrm[3 * (size_t)em.w], n1 = nrm[3 * (size_t)em.w + 1], n2 = nrm[3 * (size_t)em.w + 2];
            const float dp = (d0 * n0 + d1 * n1) + d2 * n2;
            u0 += n0 * dp;
            u1 += n1 * dp;
            u2 += n2 * dp;
        }
        add(u0, u1, u2);
    }
}

__global__ __launch_bounds__(256) void vertex_update_kernel(const float* __restrict__ x, float* __restrict__ xo, int nv,
                                                            const float* __restrict__ nrm, int nf,
                                                            const int4* __restrict__ emap, int ne,
                                                            const int* __restrict__ vemap, int max_edges,
                                                            float lambda) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nv) return;
    const float xi0 = x[3 * (size_t)i], xi1 = x[3 * (size_t)i + 1], xi2 = x[3 * (size_t)i + 2];
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
    edge_walk(i, xi0, xi1, xi2, x, nv, nrm, nf, emap, ne, vemap, max_edges, [&](float u0, float u1, float u2) {
        a0 += u0;
        a1 += u1;
        a2 += u2;
    });
    xo[3 * (size_t)i] = xi0 + lambda * a0;
    xo[3 * (size_t)i + 1] = xi1 + lambda * a1;
    xo[3 * (size_t)i + 2] = xi2 + lambda * a2;
}

// The same walk with every contribution projected onto the vertex' own direction d_i (update_position_with_depth,
// train.py:1561-1665: a vertex of a depth scan moves along its viewing ray only).  The state of a vertex is ONE scalar,
// t_i = the signed step along d_i accumulated so far: t_i += lambda * sum_s (u_s . d_i) in slot order, and the position is
// always rebuilt from the INPUT position, x_i = fma(t_i, d_i, x0_i) - never previous iterate + step, so a vertex stays
// within one rounding of its ray whatever the iteration count.  d is used as given (unit or not): sum (u . d) d.
// x: the previous iterate (x0 itself in the first iteration, `first`: t is not read then); t is private to its thread and
// updated in place; dstride: 3, or 0 for one direction shared by every vertex.
__global__ __launch_bounds__(256) void vertex_update_dir_kernel(const float* __restrict__ x0, const float* __restrict__ x,
                                                                float* __restrict__ xo, float* __restrict__ t,
                                                                float* __restrict__ t_out, int nv,
                                                                const float* __restrict__ nrm, int nf,
                                                                const int4* __restrict__ emap, int ne,
                                                                const int* __restrict__ vemap, int max_edges,
                                                                const float* __restrict__ dirs, int dstride, float lambda,
                                                                int first) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nv) return;
    const float xi0 = x[3 * (size_t)i], xi1 = x[3 * (size_t)i + 1], xi2 = x[3 * (size_t)i + 2];
    const float* dir = dirs + (size_t)i * dstride;
    const float e0 = dir[0], e1 = dir[1], e2 = dir[2];
    float acc = 0.f;
    edge_walk(i, xi0, xi1, xi2, x, nv, nrm, nf, emap, ne, vemap, max_edges,
              [&](float u0, float u1, float u2) { acc += (u0 * e0 + u1 * e1) + u2 * e2; });
    const float ti = (first ? 0.f : t[i]) + lambda * acc;
    t[i] = ti;
    if (t_out) t_out[i] = ti;
    xo[3 * (size_t)i] = fmaf(ti, e0, x0[3 * (size_t)i]);
    xo[3 * (size_t)i + 1] = fmaf(ti, e1, x0[3 * (size_t)i + 1]);
    xo[3 * (size_t)i + 2] = fmaf(ti, e2, x0[3 * (size_t)i + 2]);
}

// ---------------------------------------------------------------------------------------------
// multi-scale vertex update (update_position_MS, train.py:1668-1798)
// ---------------------------------------------------------------------------------------------
// node centres of the finest level: barycentre of the face's vertices; -1 corners read a zero vertex (train.py:1779-1787)
__global__ __launch_bounds__(256) void face_centers_kernel(const float* __restrict__ x, int nv,
                                                           const int* __restrict__ faces, int n0,
                                                           float* __restrict__ fpos) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= n0) return;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        const int v = faces[3 * (size_t)f + t];
        if (v >= 0 && v < nv) {
            s0 += x[3 * (size_t)v];
            s1 += x[3 * (size_t)v + 1];
            s2 += x[3 * (size_t)v + 2];
        }
    }
    fpos[3 * (size_t)f] = s0 / 3.0f;
    fpos[3 * (size_t)f + 1] = s1 / 3.0f;
    fpos[3 * (size_t)f + 2] = s2 / 3.0f;
}

// model.py:792-814 with steps = 2: thread = (output row, channel); the zero test is on whole rows, so a thread reads
// all c channels of its four input rows for the flags (c is 3 here)
__global__ __launch_bounds__(256) void pool4_avg_iz_kernel(const float* __restrict__ x, int nout, int c,
                                                           float* __restrict__ y) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= nout * c) return;
    const int r = idx / c, ch = idx % c;
    const float* base = x + (size_t)r * 4 * c;
    bool z[4];
    float v[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        bool all0 = true;
        for (int k = 0; k < c; ++k) all0 = all0 && (base[q * c + k] == 0.f);
        z[q] = all0;
        v[q] = base[q * c + ch];
    }
    // first round: pairs (0,1) and (2,3); a zero row takes its partner's values
    const float a0 = z[0] ? v[1] : v[0], a1 = z[1] ? v[0] : v[1];
    const float b0 = z[2] ? v[3] : v[2], b1 = z[3] ? v[2] : v[3];
    const float m0 = (a0 + a1) / 2.0f, m1 = (b0 + b1) / 2.0f;
    // the mean of a pair is a zero ROW only if both inputs were zero rows... or cancel exactly in every channel: the
    // reference tests the pooled values themselves, so do the same test on them
    bool zm0 = true, zm1 = true;
    for (int k = 0; k < c; ++k) {
        const float p0 = z[0] ? base[c + k] : base[k], p1 = z[1] ? base[k] : base[c + k];
        const float q0 = z[2] ? base[3 * c + k] : base[2 * c + k], q1 = z[3] ? base[2 * c + k] : base[3 * c + k];
        zm0 = zm0 && ((p0 + p1) / 2.0f == 0.f);
        zm1 = zm1 && ((q0 + q1) / 2.0f == 0.f);
    }
    const float c0 = zm0 ? m1 : m0, c1 = zm1 ? m0 : m1;
    y[idx] = (c0 + c1) / 2.0f;
}

// the face-slot walk of vertex v at (x0, x1, x2), level `shift`: a = sum_k n (n . (c - x_v)) over the vertex' slots in slot
// order; returns lam = 1 / #faces(v).  The one copy of this loop: both multi-scale kernels step through it.
__device__ __forceinline__ float ms_walk(int v, float x0, float x1, float x2, const int* __restrict__ vfaces, int k_v,
                                         int shift, const float* __restrict__ nrm, const float* __restrict__ fpos,
                                         int nnodes, float& a0, float& a1, float& a2) {
    a0 = a1 = a2 = 0.f;
    int numf = 0;
    for (int k = 0; k < k_v; ++k) {
        const int f = vfaces[(size_t)v * k_v + k];
        if (f < 0) continue;                      // -1 stays -1 under the floor division, i.e. the zero-normal fake node
        ++numf;
        const int node = f >> shift;
        if (node >= nnodes) continue;
        const float n0 = nrm[3 * (size_t)node], n1 = nrm[3 * (size_t)node + 1], n2 = nrm[3 * (size_t)node + 2];
        const float e0 = fpos[3 * (size_t)node] - x0, e1 = fpos[3 * (size_t)node + 1] - x1,
                    e2 = fpos[3 * (size_t)node + 2] - x2;
        const float w = (n0 * e0 + n1 * e1) + n2 * e2;
        a0 += w * n0;
        a1 += w * n1;
        a2 += w * n2;
    }
    // a vertex without faces keeps its position (the reference computes 0 * (1/0) = NaN there)
    return numf > 0 ? 1.0f / (float)numf : 0.f;
}

// one Jacobi iteration at one scale: x_v += (1/#faces(v)) sum_k n (n . (c - x_v)) over the vertex' face slots
__global__ __launch_bounds__(256) void vertex_update_ms_kernel(const float* __restrict__ x, float* __restrict__ xo,
                                                               int nv, const int* __restrict__ vfaces, int k_v,
                                                               int shift, const float* __restrict__ nrm,
                                                               const float* __restrict__ fpos, int nnodes) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= nv) return;
    const float x0 = x[3 * (size_t)v], x1 = x[3 * (size_t)v + 1], x2 = x[3 * (size_t)v + 2];
    float a0, a1, a2;
    const float lm = ms_walk(v, x0, x1, x2, vfaces, k_v, shift, nrm, fpos, nnodes, a0, a1, a2);
    xo[3 * (size_t)v] = x0 + lm * a0;
    xo[3 * (size_t)v + 1] = x1 + lm * a1;
    xo[3 * (size_t)v + 2] = x2 + lm * a2;
}

// ---------------------------------------------------------------------------------------------
// adjoint of the multi-scale vertex update (trainAccuracyNet back-propagates through update_position_MS, train.py:767-776)
// ---------------------------------------------------------------------------------------------
// One forward iteration at level s (shift = 2s): x'_v = x_v + lam_v sum_k n_j (n_j . (c_j - x_v)), j = v_faces[v,k] >> shift,
// c = P_s(C(x)).  With gbar = dL/dx' and a_v = lam_v gbar_v, summed over the slot pairs (v,k) that point to node j:
// A_j = sum a_v, S_j = sum (a_v x_v^T + x_v a_v^T).  Then
//   dL/dx_v = gbar_v - sum_k n_j (n_j . a_v) + [C^T P_s^T dL/dc]_v,  dL/dc_j = n_j (n_j . A_j),
//   dL/dn_j += (A_j . n_j) c_j + (n_j . c_j) A_j - S_j n_j.
// Every sum runs over a fixed list in a fixed order (the inverse tables below, built once per mesh), one thread per
// output row: no atomics, the result is the same bits from run to run and under hipGraph replay.

// lam_v = 1 / #valid slots, exactly as vertex_update_ms_kernel computes it (0 for a vertex without faces)
__global__ __launch_bounds__(256) void vertex_lambda_kernel(const int* __restrict__ vfaces, int k_v, int nv,
                                                            float* __restrict__ lam) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= nv) return;
    int numf = 0;
    for (int k = 0; k < k_v; ++k) numf += vfaces[(size_t)v * k_v + k] >= 0;
    lam[v] = numf > 0 ? 1.0f / (float)numf : 0.f;
}

// one thread per node j of level s: A_j and S_j over the slot entries of the fine faces [j 4^s, (j+1) 4^s) (a contiguous
// segment of the slot inverse), then dL/dc_j (written) and dL/dn_j (accumulated over the iterations of the level)
__global__ __launch_bounds__(256) void vertex_ms_bwd_node_kernel(const float* __restrict__ g, const float* __restrict__ x,
                                                                 const float* __restrict__ lam,
                                                                 const int* __restrict__ slot_ptr,
                                                                 const int* __restrict__ slot_vert, int shift, int nnodes,
                                                                 const float* __restrict__ nrm,
                                                                 const float* __restrict__ c, float* __restrict__ gc,
                                                                 float* __restrict__ gn) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nnodes) return;
    const int lo = slot_ptr[(size_t)j << shift], hi = slot_ptr[(size_t)(j + 1) << shift];
    float A0 = 0.f, A1 = 0.f, A2 = 0.f;
    float S00 = 0.f, S11 = 0.f, S22 = 0.f, S01 = 0.f, S02 = 0.f, S12 = 0.f;
    for (int e = lo; e < hi; ++e) {
        const int v = slot_vert[e];
        const float l = lam[v];
        const float a0 = l * g[3 * (size_t)v], a1 = l * g[3 * (size_t)v + 1], a2 = l * g[3 * (size_t)v + 2];
        const float x0 = x[3 * (size_t)v], x1 = x[3 * (size_t)v + 1], x2 = x[3 * (size_t)v + 2];
        A0 += a0;
        A1 += a1;
        A2 += a2;
        S00 += 2.f * a0 * x0;
        S11 += 2.f * a1 * x1;
        S22 += 2.f * a2 * x2;
        S01 += a0 * x1 + a1 * x0;
        S02 += a0 * x2 + a2 * x0;
        S12 += a1 * x2 + a2 * x1;
    }
    const float n0 = nrm[3 * (size_t)j], n1 = nrm[3 * (size_t)j + 1], n2 = nrm[3 * (size_t)j + 2];
    const float c0 = c[3 * (size_t)j], c1 = c[3 * (size_t)j + 1], c2 = c[3 * (size_t)j + 2];
    const float an = (A0 * n0 + A1 * n1) + A2 * n2;
    const float cn = (c0 * n0 + c1 * n1) + c2 * n2;
    gc[3 * (size_t)j] = an * n0;
    gc[3 * (size_t)j + 1] = an * n1;
    gc[3 * (size_t)j + 2] = an * n2;
    gn[3 * (size_t)j] += an * c0 + cn * A0 - ((S00 * n0 + S01 * n1) + S02 * n2);
    gn[3 * (size_t)j + 1] += an * c1 + cn * A1 - ((S01 * n0 + S11 * n1) + S12 * n2);
    gn[3 * (size_t)j + 2] += an * c2 + cn * A2 - ((S02 * n0 + S12 * n1) + S22 * n2);
}

// adjoint of pool4_avg_iz_kernel (c = 3): one thread per output row re-derives the forward's zero-row choices from the
// same input values (x [4n,3]) and routes dy to the four input rows it read; every input row has one reader: plain writes
__global__ __launch_bounds__(256) void pool4_avg_iz_bwd_kernel(const float* __restrict__ x, int nout,
                                                               const float* __restrict__ dy, float* __restrict__ dx) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nout) return;
    const float* base = x + (size_t)r * 12;
    bool z[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) z[q] = base[3 * q] == 0.f && base[3 * q + 1] == 0.f && base[3 * q + 2] == 0.f;
    bool zm0 = true, zm1 = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float p0 = z[0] ? base[3 + k] : base[k], p1 = z[1] ? base[k] : base[3 + k];
        const float q0 = z[2] ? base[9 + k] : base[6 + k], q1 = z[3] ? base[6 + k] : base[9 + k];
        zm0 = zm0 && ((p0 + p1) / 2.0f == 0.f);
        zm1 = zm1 && ((q0 + q1) / 2.0f == 0.f);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float gcc = dy[3 * (size_t)r + k] * 0.5f;                       // y = (c0 + c1) / 2
        const float gm0 = (zm0 ? 0.f : gcc) + (zm1 ? gcc : 0.f);               // c0 = zm0 ? m1 : m0, c1 = zm1 ? m0 : m1
        const float gm1 = (zm0 ? gcc : 0.f) + (zm1 ? 0.f : gcc);
        const float ga = gm0 * 0.5f, gb = gm1 * 0.5f;                          // m = (a0 + a1) / 2
        // a0 = z0 ? v1 : v0, a1 = z1 ? v0 : v1 (and b likewise over rows 2, 3)
        dx[(size_t)r * 12 + k] = (z[0] ? 0.f : ga) + (z[1] ? ga : 0.f);
        dx[(size_t)r * 12 + 3 + k] = (z[0] ? ga : 0.f) + (z[1] ? 0.f : ga);
        dx[(size_t)r * 12 + 6 + k] = (z[2] ? 0.f : gb) + (z[3] ? gb : 0.f);
        dx[(size_t)r * 12 + 9 + k] = (z[2] ? gb : 0.f) + (z[3] ? 0.f : gb);
    }
}

// one vertex of the adjoint: the direct term over the vertex' own slots on a = lam_v x (the gradient as it enters the step),
// then the barycentre adjoint over its face incidence; the identity term is g itself
__device__ __forceinline__ void ms_bwd_vertex_row(int v, float g0, float g1, float g2, float a0, float a1, float a2,
                                                  const int* __restrict__ vfaces, int k_v, int shift,
                                                  const float* __restrict__ nrm, int nnodes,
                                                  const int* __restrict__ inc_ptr, const int* __restrict__ inc_face,
                                                  const float* __restrict__ gfp0, float* __restrict__ go) {
    float d0 = 0.f, d1 = 0.f, d2 = 0.f;
    for (int k = 0; k < k_v; ++k) {
        const int f = vfaces[(size_t)v * k_v + k];
        if (f < 0) continue;
        const int node = f >> shift;
        if (node >= nnodes) continue;
        const float n0 = nrm[3 * (size_t)node], n1 = nrm[3 * (size_t)node + 1], n2 = nrm[3 * (size_t)node + 2];
        const float w = (n0 * a0 + n1 * a1) + n2 * a2;
        d0 += w * n0;
        d1 += w * n1;
        d2 += w * n2;
    }
    float b0 = 0.f, b1 = 0.f, b2 = 0.f;
    const int lo = inc_ptr[v], hi = inc_ptr[v + 1];
    for (int e = lo; e < hi; ++e) {
        const int f = inc_face[e];
        b0 += gfp0[3 * (size_t)f];
        b1 += gfp0[3 * (size_t)f + 1];
        b2 += gfp0[3 * (size_t)f + 2];
    }
    go[3 * (size_t)v] = (g0 - d0) + b0 / 3.0f;
    go[3 * (size_t)v + 1] = (g1 - d1) + b1 / 3.0f;
    go[3 * (size_t)v + 2] = (g2 - d2) + b2 / 3.0f;
}

// one thread per vertex: the direct term over the vertex' own slots, then the barycentre adjoint over its face incidence
__global__ __launch_bounds__(256) void vertex_ms_bwd_vertex_kernel(const float* __restrict__ g, int nv,
                                                                   const float* __restrict__ lam,
                                                                   const int* __restrict__ vfaces, int k_v, int shift,
                                                                   const float* __restrict__ nrm, int nnodes,
                                                                   const int* __restrict__ inc_ptr,
                                                                   const int* __restrict__ inc_face,
                                                                   const float* __restrict__ gfp0,
                                                                   float* __restrict__ go) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= nv) return;
    const float l = lam[v];
    const float g0 = g[3 * (size_t)v], g1 = g[3 * (size_t)v + 1], g2 = g[3 * (size_t)v + 2];
    ms_bwd_vertex_row(v, g0, g1, g2, l * g0, l * g1, l * g2, vfaces, k_v, shift, nrm, nnodes, inc_ptr, inc_face, gfp0, go);
}

__global__ void sub3_kernel(const float* a, const float* b, int n, float* o) {   // o may alias b
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) o[i] = a[i] - b[i];
}

// ---------------------------------------------------------------------------------------------
// the multi-scale update along a per-vertex direction (a build extension: the reference constrains the single-scale
// update only) and its adjoint
// ---------------------------------------------------------------------------------------------
// vertex_update_ms_kernel's walk, the step delta_v = lam_v sum_k n (n . (c - x_v)) projected onto the vertex' own direction
// d_v.  As in vertex_update_dir_kernel the state of a vertex is ONE scalar, t_v += delta_v . d_v, private to its thread
// and zeroed by the host before the first iteration, and the position is rebuilt from the INPUT position x0, x_v = fma(t_v,
// d_v, x0_v).  x: the previous iterate (where the centres came from); dstride: 3, or 0 for one direction shared by all.
__global__ __launch_bounds__(256) void vertex_update_ms_dir_kernel(const float* __restrict__ x0,
                                                                   const float* __restrict__ x, float* __restrict__ xo,
                                                                   float* __restrict__ t, int nv,
                                                                   const int* __restrict__ vfaces, int k_v, int shift,
                                                                   const float* __restrict__ nrm,
                                                                   const float* __restrict__ fpos, int nnodes,
                                                                   const float* __restrict__ dirs, int dstride) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= nv) return;
    const float p0 = x[3 * (size_t)v], p1 = x[3 * (size_t)v + 1], p2 = x[3 * (size_t)v + 2];   // the current iterate
    float a0, a1, a2;      // (a vertex without faces: lm = 0, t stays where it is)
    const float lm = ms_walk(v, p0, p1, p2, vfaces, k_v, shift, nrm, fpos, nnodes, a0, a1, a2);
    const float* dir = dirs + (size_t)v * dstride;
    const float d0 = dir[0], d1 = dir[1], d2 = dir[2];
    const float tv = t[v] + (((lm * a0) * d0 + (lm * a1) * d1) + (lm * a2) * d2);
    t[v] = tv;
    xo[3 * (size_t)v] = fmaf(tv, d0, x0[3 * (size_t)v]);
    xo[3 * (size_t)v + 1] = fmaf(tv, d1, x0[3 * (size_t)v + 1]);
    xo[3 * (size_t)v + 2] = fmaf(tv, d2, x0[3 * (size_t)v + 2]);
}

// gp_v = d_v (d_v . g_v): the incoming gradient as the projected step sees it
__global__ __launch_bounds__(256) void project_rows_kernel(const float* __restrict__ g, int nv,
                                                           const float* __restrict__ dirs, int dstride,
                                                           float* __restrict__ gp) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= nv) return;
    const float* dir = dirs + (size_t)v * dstride;
    const float d0 = dir[0], d1 = dir[1], d2 = dir[2];
    const float s = (d0 * g[3 * (size_t)v] + d1 * g[3 * (size_t)v + 1]) + d2 * g[3 * (size_t)v + 2];
    gp[3 * (size_t)v] = s * d0;
    gp[3 * (size_t)v + 1] = s * d1;
    gp[3 * (size_t)v + 2] = s * d2;
}

// vertex_ms_bwd_vertex_kernel with the projected gradient gp in the direct term; the identity term keeps g itself
__global__ __launch_bounds__(256) void vertex_ms_dir_bwd_vertex_kernel(const float* __restrict__ g,
                                                                       const float* __restrict__ gp, int nv,
                                                                       const float* __restrict__ lam,
                                                                       const int* __restrict__ vfaces, int k_v, int shift,
                                                                       const float* __restrict__ nrm, int nnodes,
                                                                       const int* __restrict__ inc_ptr,
                                                                       const int* __restrict__ inc_face,
                                                                       const float* __restrict__ gfp0,
                                                                       float* __restrict__ go) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= nv) return;
    const float l = lam[v];
    ms_bwd_vertex_row(v, g[3 * (size_t)v], g[3 * (size_t)v + 1], g[3 * (size_t)v + 2], l * gp[3 * (size_t)v],
                      l * gp[3 * (size_t)v + 1], l * gp[3 * (size_t)v + 2], vfaces, k_v, shift, nrm, nnodes, inc_ptr, inc_face,
                      gfp0, go);
}

}  // namespace fgc

using namespace fgc;

extern "C" int fgc_face_centers(const float* x, int32_t nv, const int32_t* faces, int32_t n0, float* fpos, void* stream) {
    FGC_CHECK_ARG(x && faces && fpos && nv > 0 && n0 > 0, "fgc_face_centers: bad arguments");
    FGC_LAUNCH("face_centers_kernel", (hipStream_t)stream, face_centers_kernel, dim3(cdiv(n0, 256)), dim3(256), 0, x, nv,
               faces, n0, fpos);
    FGC_CHECK_LAUNCH("fgc_face_centers");
    return FGC_OK;
}

extern "C" int fgc_pool4_avg_iz(const float* x, int32_t n, int32_t c, float* y, void* stream) {
    FGC_CHECK_ARG(x && y && n > 0 && n % 4 == 0 && c > 0, "fgc_pool4_avg_iz: n=%d (multiple of 4) c=%d", n, c);
    const int total = (n / 4) * c;
    FGC_LAUNCH("pool4_avg_iz_kernel", (hipStream_t)stream, pool4_avg_iz_kernel, dim3(cdiv(total, 256)), dim3(256), 0, x,
               n / 4, c, y);
    FGC_CHECK_LAUNCH("fgc_pool4_avg_iz");
    return FGC_OK;
}

extern "C" int fgc_vertex_update(const float* x, float* x_out, float* tmp, int32_t nv, const float* normals, int32_t nf,
                                 const int32_t* e_map, int32_t ne, const int32_t* v_e_map, int32_t max_edges,
                                 int32_t iters, float lambda, void* stream) {
    FGC_CHECK_ARG(x && x_out && tmp && normals && e_map && v_e_map, "fgc_vertex_update: null pointer");
    FGC_CHECK_ARG(nv > 0 && nf > 0 && ne >= 0 && max_edges > 0 && iters >= 0,
                  "fgc_vertex_update: nv=%d nf=%d ne=%d max_edges=%d iters=%d", nv, nf, ne, max_edges, iters);
    FGC_CHECK_ARG(x != x_out && x != tmp && x_out != tmp, "fgc_vertex_update: x, x_out and tmp must be distinct");
    FGC_CHECK_ARG((uintptr_t)e_map % 16 == 0, "fgc_vertex_update: e_map needs 16-byte alignment");
    hipStream_t st = (hipStream_t)stream;
    if (iters == 0) {
        if (hipMemcpyAsync(x_out, x, (size_t)nv * 12, hipMemcpyDeviceToDevice, st) != hipSuccess) {
            fgc::set_error("fgc_vertex_update: copy failed");
            return FGC_EHIP;
        }
        return FGC_OK;
    }
    const float* src = x;
    for (int it = 0; it < iters; ++it) {
        float* dst = ((iters - 1 - it) & 1) ? tmp : x_out;   // the last iteration lands in x_out
        FGC_LAUNCH("vertex_update_kernel", st, vertex_update_kernel, dim3(cdiv(nv, 256)), dim3(256), 0, src, dst, nv,
                   normals, nf, reinterpret_cast<const int4*>(e_map), ne, v_e_map, max_edges, lambda);
        src = dst;
    }
    FGC_CHECK_LAUNCH("fgc_vertex_update");
    return FGC_OK;
}

extern "C" size_t fgc_vertex_update_dir_workspace_floats(int32_t nv) {
    return nv > 0 ? 4 * (size_t)nv : 0;      // one ping-pong position buffer [nv,3] and t [nv]
}

extern "C" int fgc_vertex_update_dir(const float* x, float* x_out, float* t_out, float* ws, size_t ws_floats, int32_t nv,
                                     const float* normals, int32_t nf, const int32_t* e_map, int32_t ne,
                                     const int32_t* v_e_map, int32_t max_edges, const float* dirs, int32_t n_dirs,
                                     int32_t iters, float lambda, void* stream) {
    FGC_CHECK_ARG(x && x_out && ws && normals && v_e_map && dirs && (e_map || ne == 0),
                  "fgc_vertex_update_dir: null pointer");
    FGC_CHECK_ARG(nv > 0 && nf > 0 && ne >= 0 && max_edges > 0 && iters >= 0,
                  "fgc_vertex_update_dir: nv=%d nf=%d ne=%d max_edges=%d iters=%d", nv, nf, ne, max_edges, iters);
    FGC_CHECK_ARG(n_dirs == 1 || n_dirs == nv, "fgc_vertex_update_dir: n_dirs=%d (1, or nv=%d)", n_dirs, nv);
    const size_t need = fgc_vertex_update_dir_workspace_floats(nv);
    FGC_CHECK_ARG(ws_floats >= need, "fgc_vertex_update_dir: workspace too small (%zu < %zu floats)", ws_floats, need);
    FGC_CHECK_ARG(x != x_out && (x + 3 * (size_t)nv <= ws || x >= ws + need) &&
                      (x_out + 3 * (size_t)nv <= ws || x_out >= ws + need),
                  "fgc_vertex_update_dir: x, x_out and the workspace must be distinct");
    FGC_CHECK_ARG(!t_out || (t_out != x && t_out != x_out && (t_out + nv <= ws || t_out >= ws + need)),
                  "fgc_vertex_update_dir: t_out must be a buffer of its own");
    FGC_CHECK_ARG((uintptr_t)e_map % 16 == 0, "fgc_vertex_update_dir: e_map needs 16-byte alignment");
    hipStream_t st = (hipStream_t)stream;
    if (iters == 0) {
        if (hipMemcpyAsync(x_out, x, (size_t)nv * 12, hipMemcpyDeviceToDevice, st) != hipSuccess ||
            (t_out && hipMemsetAsync(t_out, 0, (size_t)nv * 4, st) != hipSuccess)) {
            fgc::set_error("fgc_vertex_update_dir: copy failed");
            return FGC_EHIP;
        }
        return FGC_OK;
    }
    float* tmp = ws;
    float* t = ws + 3 * (size_t)nv;
    const float* src = x;
    for (int it = 0; it < iters; ++it) {
        const bool last = it == iters - 1;
        float* dst = ((iters - 1 - it) & 1) ? tmp : x_out;   // the last iteration lands in x_out
        FGC_LAUNCH("vertex_update_dir_kernel", st, vertex_update_dir_kernel, dim3(cdiv(nv, 256)), dim3(256), 0, x, src, dst,
                   t, last ? t_out : (float*)nullptr, nv, normals, nf, reinterpret_cast<const int4*>(e_map), ne, v_e_map,
                   max_edges, dirs, n_dirs == 1 ? 0 : 3, lambda, it == 0 ? 1 : 0);
        src = dst;
    }
    FGC_CHECK_LAUNCH("fgc_vertex_update_dir");
    return FGC_OK;
}

// ---------------------------------------------------------------------------------------------
// the multi-scale update, free or along a per-vertex direction: host side
// ---------------------------------------------------------------------------------------------
// the three levels as the drivers index them by scale: normals, node centres (3 (n0 + n0/4 + n0/16) floats at `centres`,
// inside the caller's scratch) and node counts
struct MsLevels {
    const float* nrm[3];
    float* fps[3];
    int nn[3];
};

static MsLevels ms_levels(const float* normals0, const float* normals1, const float* normals2, int n0, float* centres) {
    const int n1 = n0 / 4, n2 = n0 / 16;
    return {{normals0, normals1, normals2}, {centres, centres + 3 * (size_t)n0, centres + 3 * ((size_t)n0 + n1)}, {n0, n1, n2}};
}

// the node centres of levels 0 .. scale from the positions x: the barycentres, then one 4:1 pooling per coarser level.  The
// one copy of this sequence: every iteration, forward and adjoint, gets its centres here.
static void ms_centres(hipStream_t st, const float* x, int nv, const int32_t* faces, const MsLevels& L, int scale) {
    FGC_LAUNCH("face_centers_kernel", st, face_centers_kernel, dim3(cdiv(L.nn[0], 256)), dim3(256), 0, x, nv, faces, L.nn[0],
               L.fps[0]);
    for (int l = 1; l <= scale; ++l)
        FGC_LAUNCH("pool4_avg_iz_kernel", st, pool4_avg_iz_kernel, dim3(cdiv(L.nn[l] * 3, 256)), dim3(256), 0, L.fps[l - 1],
                   L.nn[l], 3, L.fps[l]);
}

static bool ms_apart(const float* p, size_t n, const float* q, size_t m) {   // [p, p+n) and [q, q+m) do not meet
    return p + n <= q || q + m <= p;
}

extern "C" size_t fgc_vertex_update_ms_dir_scratch_floats(int32_t nv, int32_t n0) {
    if (nv <= 0 || n0 <= 0) return 0;
    // t [nv], the node centres of the three levels, two ping-pong position buffers (the trajectory form: the first two)
    return (size_t)nv * 7 + 3 * ((size_t)n0 + n0 / 4 + n0 / 16);
}

// The four forward entry points in one body, so that they cannot drift apart: free (dirs == NULL) or along dirs, the plain
// form (traj == NULL: ping-pong buffers in the scratch, the result copied to x_out, dx_out optional) or the trajectory form
// (every iteration writes its own slot of traj; x_out and dx_out are NULL).  The first iteration of the plain form reads
// the caller's x in place.  Scratch: two position buffers (plain form), t [nv] (along dirs), the centres of the three levels.
// fn: the entry point's name, for the messages; the wrappers have checked dirs / x_out / traj, whichever is theirs.
static int ms_fwd_impl(const char* fn, const float* x, float* x_out, int32_t nv, const int32_t* faces, int32_t n0,
                       const int32_t* v_faces, int32_t k_v, const float* normals0, const float* normals1,
                       const float* normals2, const int32_t* iters, const float* dirs, int32_t n_dirs, float* traj,
                       size_t traj_floats, float* t_out, float* dx_out, float* scratch, size_t scratch_floats, void* stream) {
    FGC_CHECK_ARG(x && faces && v_faces && normals0 && normals1 && normals2 && iters && scratch, "%s: null pointer", fn);
    FGC_CHECK_ARG(nv > 0 && n0 > 0 && n0 % 16 == 0 && k_v > 0, "%s: nv=%d n0=%d (multiple of 16) k_v=%d", fn, nv, n0, k_v);
    FGC_CHECK_ARG(!dirs || n_dirs == 1 || n_dirs == nv, "%s: n_dirs=%d (1, or nv=%d)", fn, n_dirs, nv);
    FGC_CHECK_ARG(iters[0] >= 0 && iters[1] >= 0 && iters[2] >= 0, "%s: negative iteration count", fn);
    const size_t nx = 3 * (size_t)nv;
    const size_t ncentres = 3 * ((size_t)n0 + n0 / 4 + n0 / 16);
    float* out = traj ? traj : x_out;
    const size_t nout = traj ? ((size_t)iters[0] + iters[1] + iters[2] + 1) * nx : nx;
    FGC_CHECK_ARG(!traj || traj_floats >= nout, "%s: traj too small (%zu < %zu floats)", fn, traj_floats, nout);
    const size_t need = ncentres + (dirs ? (size_t)nv : 0) + (traj ? 0 : 2 * nx);
    FGC_CHECK_ARG(scratch_floats >= need, "%s: scratch too small (%zu < %zu floats)", fn, scratch_floats, need);
    FGC_CHECK_ARG(ms_apart(x, nx, out, nout) && ms_apart(x, nx, scratch, need) && ms_apart(out, nout, scratch, need),
                  "%s: x, %s and the scratch must be distinct", fn, traj ? "traj" : "x_out");
    FGC_CHECK_ARG(!dx_out || (ms_apart(dx_out, 3 * nx, x, nx) && ms_apart(dx_out, 3 * nx, out, nout) &&
                              ms_apart(dx_out, 3 * nx, scratch, need) && (!t_out || ms_apart(dx_out, 3 * nx, t_out, nv))),
                  "%s: dx_out must be a buffer of its own", fn);
    FGC_CHECK_ARG(!t_out || (ms_apart(t_out, nv, x, nx) && ms_apart(t_out, nv, out, nout) && ms_apart(t_out, nv, scratch, need)),
                  "%s: t_out must be a buffer of its own", fn);
    hipStream_t st = (hipStream_t)stream;
    // the buffers that copies and the memset touch come first, in whole rows: they keep the scratch's alignment
    float* xa = scratch;                              // (plain form only)
    float* xb = xa + nx;
    float* t = traj ? scratch : xb + nx;              // (along dirs only)
    const MsLevels L = ms_levels(normals0, normals1, normals2, n0, dirs ? t + nv : t);
    if (dirs && hipMemsetAsync(t, 0, (size_t)nv * 4, st) != hipSuccess) {
        fgc::set_error("%s: memset failed", fn);
        return FGC_EHIP;
    }
    if (traj && hipMemcpyAsync(traj, x, nx * 4, hipMemcpyDeviceToDevice, st) != hipSuccess) {
        fgc::set_error("%s: copy failed", fn);
        return FGC_EHIP;
    }
    const float* cur = traj ? traj : x;      // x0 is the caller's x through all three stages
    float* nxt = traj ? traj + nx : xa;
    for (int stage = 0; stage < 3; ++stage) {
        const int scale = 2 - stage;                 // coarse to fine (train.py:1687)
        float* start = dx_out ? dx_out + (size_t)stage * nx : nullptr;
        // remember where this stage started: dx = x_end - x_start (train.py:1763)
        if (start && hipMemcpyAsync(start, cur, nx * 4, hipMemcpyDeviceToDevice, st) != hipSuccess) {
            fgc::set_error("%s: copy failed", fn);
            return FGC_EHIP;
        }
        for (int it = 0; it < iters[stage]; ++it) {
            ms_centres(st, cur, nv, faces, L, scale);
            if (dirs)
                FGC_LAUNCH("vertex_update_ms_dir_kernel", st, vertex_update_ms_dir_kernel, dim3(cdiv(nv, 256)), dim3(256), 0, x,
                           cur, nxt, t, nv, v_faces, k_v, 2 * scale, L.nrm[scale], L.fps[scale], L.nn[scale], dirs,
                           n_dirs == 1 ? 0 : 3);
            else
                FGC_LAUNCH("vertex_update_ms_kernel", st, vertex_update_ms_kernel, dim3(cdiv(nv, 256)), dim3(256), 0, cur, nxt,
                           nv, v_faces, k_v, 2 * scale, L.nrm[scale], L.fps[scale], L.nn[scale]);
            cur = nxt;
            nxt = traj ? nxt + nx : (nxt == xa ? xb : xa);
        }
        if (start)
            FGC_LAUNCH("sub3_kernel", st, sub3_kernel, dim3(cdiv(nv * 3, 256)), dim3(256), 0, cur, start, nv * 3, start);
    }
    if ((x_out && hipMemcpyAsync(x_out, cur, nx * 4, hipMemcpyDeviceToDevice, st) != hipSuccess) ||
        (t_out && hipMemcpyAsync(t_out, t, (size_t)nv * 4, hipMemcpyDeviceToDevice, st) != hipSuccess)) {
        fgc::set_error("%s: copy failed", fn);
        return FGC_EHIP;
    }
    FGC_CHECK_LAUNCH(fn);
    return FGC_OK;
}

extern "C" int fgc_vertex_update_ms(const float* x, float* x_out, int32_t nv, const int32_t* faces, int32_t n0,
                                    const int32_t* v_faces, int32_t k_v, const float* normals0, const float* normals1,
                                    const float* normals2, const int32_t* iters, float* dx_out, float* scratch,
                                    size_t scratch_floats, void* stream) {
    FGC_CHECK_ARG(x_out, "fgc_vertex_update_ms: null pointer");
    return ms_fwd_impl("fgc_vertex_update_ms", x, x_out, nv, faces, n0, v_faces, k_v, normals0, normals1, normals2, iters,
                       nullptr, 0, nullptr, 0, nullptr, dx_out, scratch, scratch_floats, stream);
}

// the trajectory form: the same launches with the same arguments, every iteration writing its own slot of traj (slot 0 = x,
// slot t + 1 = the output of iteration t) instead of a ping-pong buffer
extern "C" int fgc_vertex_update_ms_traj(const float* x, int32_t nv, const int32_t* faces, int32_t n0,
                                         const int32_t* v_faces, int32_t k_v, const float* normals0,
                                         const float* normals1, const float* normals2, const int32_t* iters,
                                         float* traj, size_t traj_floats, float* scratch, size_t scratch_floats,
                                         void* stream) {
    FGC_CHECK_ARG(traj, "fgc_vertex_update_ms_traj: null pointer");
    return ms_fwd_impl("fgc_vertex_update_ms_traj", x, nullptr, nv, faces, n0, v_faces, k_v, normals0, normals1, normals2,
                       iters, nullptr, 0, traj, traj_floats, nullptr, nullptr, scratch, scratch_floats, stream);
}

extern "C" int fgc_vertex_update_ms_dir(const float* x, float* x_out, int32_t nv, const int32_t* faces, int32_t n0,
                                        const int32_t* v_faces, int32_t k_v, const float* normals0, const float* normals1,
                                        const float* normals2, const int32_t* iters, const float* dirs, int32_t n_dirs,
                                        float* t_out, float* dx_out, float* scratch, size_t scratch_floats, void* stream) {
    FGC_CHECK_ARG(x_out && dirs, "fgc_vertex_update_ms_dir: null pointer");
    return ms_fwd_impl("fgc_vertex_update_ms_dir", x, x_out, nv, faces, n0, v_faces, k_v, normals0, normals1, normals2, iters,
                       dirs, n_dirs, nullptr, 0, t_out, dx_out, scratch, scratch_floats, stream);
}

extern "C" int fgc_vertex_update_ms_dir_traj(const float* x, int32_t nv, const int32_t* faces, int32_t n0,
                                             const int32_t* v_faces, int32_t k_v, const float* normals0,
                                             const float* normals1, const float* normals2, const int32_t* iters,
                                             const float* dirs, int32_t n_dirs, float* traj, size_t traj_floats,
                                             float* t_out, float* scratch, size_t scratch_floats, void* stream) {
    FGC_CHECK_ARG(traj && dirs, "fgc_vertex_update_ms_dir_traj: null pointer");
    return ms_fwd_impl("fgc_vertex_update_ms_dir_traj", x, nullptr, nv, faces, n0, v_faces, k_v, normals0, normals1,
                       normals2, iters, dirs, n_dirs, traj, traj_floats, t_out, nullptr, scratch, scratch_floats, stream);
}

extern "C" size_t fgc_vertex_update_ms_bwd_workspace_floats(int32_t nv, int32_t n0) {
    if (nv <= 0 || n0 <= 0) return 0;
    const size_t nodes = (size_t)n0 + n0 / 4 + n0 / 16;
    return (size_t)nv * 7 + 6 * nodes;      // lam, two gradient buffers; centres and their gradients of the three levels
}

extern "C" size_t fgc_vertex_update_ms_dir_bwd_workspace_floats(int32_t nv, int32_t n0) {
    if (nv <= 0 || n0 <= 0) return 0;
    return fgc_vertex_update_ms_bwd_workspace_floats(nv, n0) + 3 * (size_t)nv;      // and the projected gradient
}

// The adjoint of the multi-scale update, free (dirs == NULL: fgc_vertex_update_ms_bwd) or along dirs
// (fgc_vertex_update_ms_dir_bwd): one body, so the two cannot drift apart.  Along dirs every iteration first writes the
// projected gradient gp (3 nv more workspace floats, behind the two gradient buffers); the node kernel then reads gp in the
// place of g, and the vertex kernel takes both.  fn: the entry point's name, for the messages.
static int ms_bwd_impl(const char* fn, const float* traj, size_t traj_floats, int32_t nv, const int32_t* faces, int32_t n0,
                       const int32_t* v_faces, int32_t k_v, const float* normals0, const float* normals1,
                       const float* normals2, const int32_t* iters, const float* dirs, int32_t n_dirs,
                       const int32_t* slot_ptr, const int32_t* slot_vert, const int32_t* inc_ptr, const int32_t* inc_face,
                       const float* g_out, float* g_x, float* g_n0, float* g_n1, float* g_n2, float* workspace,
                       size_t workspace_floats, void* stream) {
    FGC_CHECK_ARG(traj && faces && v_faces && normals0 && normals1 && normals2 && iters && slot_ptr && slot_vert &&
                      inc_ptr && inc_face && g_out && g_x && g_n0 && g_n1 && g_n2 && workspace,
                  "%s: null pointer", fn);
    FGC_CHECK_ARG(nv > 0 && n0 > 0 && n0 % 16 == 0 && k_v > 0, "%s: nv=%d n0=%d (multiple of 16) k_v=%d", fn, nv, n0, k_v);
    FGC_CHECK_ARG(!dirs || n_dirs == 1 || n_dirs == nv, "%s: n_dirs=%d (1, or nv=%d)", fn, n_dirs, nv);
    FGC_CHECK_ARG(iters[0] >= 0 && iters[1] >= 0 && iters[2] >= 0, "%s: negative iteration count", fn);
    const size_t need = dirs ? fgc_vertex_update_ms_dir_bwd_workspace_floats(nv, n0)
                             : fgc_vertex_update_ms_bwd_workspace_floats(nv, n0);
    FGC_CHECK_ARG(workspace_floats >= need, "%s: workspace too small (%zu < %zu floats)", fn, workspace_floats, need);
    const size_t need_traj = ((size_t)iters[0] + iters[1] + iters[2] + 1) * 3 * (size_t)nv;
    FGC_CHECK_ARG(traj_floats >= need_traj, "%s: traj too small (%zu < %zu floats)", fn, traj_floats, need_traj);
    FGC_CHECK_ARG(g_out != g_x, "%s: g_out and g_x must be distinct", fn);
    const int dstride = n_dirs == 1 ? 0 : 3;
    hipStream_t st = (hipStream_t)stream;
    float* lam = workspace;
    float* ga = lam + nv;
    float* gb = ga + 3 * (size_t)nv;
    float* gp = gb + 3 * (size_t)nv;                      // (along dirs only)
    const MsLevels L = ms_levels(normals0, normals1, normals2, n0, dirs ? gp + 3 * (size_t)nv : gp);
    float* gc0 = L.fps[2] + 3 * (size_t)L.nn[2];          // the centres' gradients, laid out like the centres behind them
    float* gcs[3] = {gc0, gc0 + 3 * (size_t)L.nn[0], gc0 + 3 * ((size_t)L.nn[0] + L.nn[1])};
    float* gns[3] = {g_n0, g_n1, g_n2};
    for (int s = 0; s < 3; ++s)
        if (hipMemsetAsync(gns[s], 0, (size_t)L.nn[s] * 12, st) != hipSuccess) {
            fgc::set_error("%s: memset failed", fn);
            return FGC_EHIP;
        }
    if (hipMemcpyAsync(ga, g_out, (size_t)nv * 12, hipMemcpyDeviceToDevice, st) != hipSuccess) {
        fgc::set_error("%s: copy failed", fn);
        return FGC_EHIP;
    }
    FGC_LAUNCH("vertex_lambda_kernel", st, vertex_lambda_kernel, dim3(cdiv(nv, 256)), dim3(256), 0, v_faces, k_v, nv, lam);
    size_t t = (size_t)iters[0] + iters[1] + iters[2];
    float* cur = ga;     // dL/d x_{t+1}
    float* nxt = gb;
    for (int stage = 2; stage >= 0; --stage) {
        const int scale = 2 - stage, nn = L.nn[scale];
        for (int it = 0; it < iters[stage]; ++it) {
            --t;
            const float* xt = traj + t * 3 * (size_t)nv;
            // the centres the forward iteration read, recomputed by the forward's own kernels from x_t
            ms_centres(st, xt, nv, faces, L, scale);
            if (dirs)
                FGC_LAUNCH("project_rows_kernel", st, project_rows_kernel, dim3(cdiv(nv, 256)), dim3(256), 0, cur, nv, dirs,
                           dstride, gp);
            FGC_LAUNCH("vertex_ms_bwd_node_kernel", st, vertex_ms_bwd_node_kernel, dim3(cdiv(nn, 256)), dim3(256), 0,
                       dirs ? gp : cur, xt, lam, slot_ptr, slot_vert, 2 * scale, nn, L.nrm[scale], L.fps[scale], gcs[scale],
                       gns[scale]);
            for (int l = scale; l >= 1; --l)
                FGC_LAUNCH("pool4_avg_iz_bwd_kernel", st, pool4_avg_iz_bwd_kernel, dim3(cdiv(L.nn[l], 256)), dim3(256), 0,
                           L.fps[l - 1], L.nn[l], gcs[l], gcs[l - 1]);
            if (dirs)
                FGC_LAUNCH("vertex_ms_dir_bwd_vertex_kernel", st, vertex_ms_dir_bwd_vertex_kernel, dim3(cdiv(nv, 256)),
                           dim3(256), 0, cur, gp, nv, lam, v_faces, k_v, 2 * scale, L.nrm[scale], nn, inc_ptr, inc_face, gc0, nxt);
            else
                FGC_LAUNCH("vertex_ms_bwd_vertex_kernel", st, vertex_ms_bwd_vertex_kernel, dim3(cdiv(nv, 256)), dim3(256), 0,
                           cur, nv, lam, v_faces, k_v, 2 * scale, L.nrm[scale], nn, inc_ptr, inc_face, gc0, nxt);
            float* tmp = cur;
            cur = nxt;
            nxt = tmp;
        }
    }
    if (hipMemcpyAsync(g_x, cur, (size_t)nv * 12, hipMemcpyDeviceToDevice, st) != hipSuccess) {
        fgc::set_error("%s: copy failed", fn);
        return FGC_EHIP;
    }
    FGC_CHECK_LAUNCH(fn);
    return FGC_OK;
}

extern "C" int fgc_vertex_update_ms_bwd(const float* traj, size_t traj_floats, int32_t nv, const int32_t* faces, int32_t n0,
                                        const int32_t* v_faces, int32_t k_v, const float* normals0,
                                        const float* normals1, const float* normals2, const int32_t* iters,
                                        const int32_t* slot_ptr, const int32_t* slot_vert, const int32_t* inc_ptr,
                                        const int32_t* inc_face, const float* g_out, float* g_x, float* g_n0,
                                        float* g_n1, float* g_n2, float* workspace, size_t workspace_floats,
                                        void* stream) {
    return ms_bwd_impl("fgc_vertex_update_ms_bwd", traj, traj_floats, nv, faces, n0, v_faces, k_v, normals0, normals1,
                       normals2, iters, nullptr, 0, slot_ptr, slot_vert, inc_ptr, inc_face, g_out, g_x, g_n0, g_n1, g_n2,
                       workspace, workspace_floats, stream);
}

extern "C" int fgc_vertex_update_ms_dir_bwd(const float* traj, size_t traj_floats, int32_t nv, const int32_t* faces,
                                            int32_t n0, const int32_t* v_faces, int32_t k_v, const float* normals0,
                                            const float* normals1, const float* normals2, const int32_t* iters,
                                            const float* dirs, int32_t n_dirs, const int32_t* slot_ptr,
                                            const int32_t* slot_vert, const int32_t* inc_ptr, const int32_t* inc_face,
                                            const float* g_out, float* g_x, float* g_n0, float* g_n1, float* g_n2,
                                            float* workspace, size_t workspace_floats, void* stream) {
    FGC_CHECK_ARG(dirs, "fgc_vertex_update_ms_dir_bwd: null pointer");
    return ms_bwd_impl("fgc_vertex_update_ms_dir_bwd", traj, traj_floats, nv, faces, n0, v_faces, k_v, normals0, normals1,
                       normals2, iters, dirs, n_dirs, slot_ptr, slot_vert, inc_ptr, inc_face, g_out, g_x, g_n0, g_n1, g_n2,
                       workspace, workspace_floats, stream);
}
