// Point-set loss of trainAccuracyNet (fullLoss, train.py:1373-1424), forward and gradient.
//
// The two nearest-point scans are fgc_nn_query (exact, ties to the lowest index).  Then one launch turns every sample into
// a term (its P0 row, its masked distance, its gradient on that row) and one single-workgroup launch sums the loss and
// reduces the terms that share a P0 row: a term is summed by the first term of its row, in term order.  No atomics: the
// loss and the gradient are the same bits from run to run and under hipGraph replay.
#include "fgc_points.h"

extern "C" int fgc_nn_query(const float* q, int32_t nq, const float* p, int32_t np, const int32_t* q_cell,
                            const int32_t* p_cell, float* dist, int32_t* idx, void* workspace, size_t workspace_bytes,
                            void* stream);
extern "C" size_t fgc_nn_workspace_bytes(int32_t nq, int32_t np);

namespace fgc {

constexpr int PL_THREADS = 1024;

// q[i] = p[ind[i]]; an index out of [0, np) gives a NaN row (its scan finds nothing and the loss turns NaN)
__global__ __launch_bounds__(256) void point_gather_kernel(const float* __restrict__ p, int np, const int* __restrict__ ind,
                                                           int n, float* __restrict__ q) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int r = ind[i];
    const bool ok = r >= 0 && r < np;
#pragma unroll
    for (int k = 0; k < 3; ++k) q[3 * (size_t)i + k] = ok ? p[3 * (size_t)r + k] : __builtin_nanf("");
}

// term t < ns0: precision of sample t (row i0[t] of P0 against its nearest P1 point); t >= ns0: completeness of sample
// t - ns0 (its nearest P0 row against row i1 of P1).  val = d if d <= threshold else 0; grad = scale (P0 - P1) / d on the P0
// row, 0 for a masked term and at d = 0.  A sample whose scan found nothing gets row -1 and val NaN.
__global__ __launch_bounds__(256) void point_loss_terms_kernel(const float* __restrict__ p0, int np0,
                                                               const float* __restrict__ p1, int np1,
                                                               const int* __restrict__ i0, int ns0,
                                                               const int* __restrict__ i1, int ns1,
                                                               const float* __restrict__ dist0, const int* __restrict__ idx0,
                                                               const float* __restrict__ dist1, const int* __restrict__ idx1,
                                                               float threshold, int* __restrict__ rows,
                                                               float4* __restrict__ terms) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= ns0 + ns1) return;
    int r, m;
    float d, scale;
    if (t < ns0) {
        r = i0[t];
        m = idx0[t];
        d = dist0[t];
        scale = 1000.0f / (float)ns0;
    } else {
        r = idx1[t - ns0];
        m = i1[t - ns0];
        d = dist1[t - ns0];
        scale = 1000.0f / (float)ns1;
    }
    if (r < 0 || r >= np0 || m < 0 || m >= np1) {
        rows[t] = -1;
        terms[t] = make_float4(0.f, 0.f, 0.f, __builtin_nanf(""));
        return;
    }
    const bool keep = d <= threshold;
    const float w = (keep && d > 0.f) ? scale / d : 0.f;
    rows[t] = r;
    terms[t] = make_float4((p0[3 * (size_t)r] - p1[3 * (size_t)m]) * w, (p0[3 * (size_t)r + 1] - p1[3 * (size_t)m + 1]) * w,
                           (p0[3 * (size_t)r + 2] - p1[3 * (size_t)m + 2]) * w, keep ? d : 0.f);
}

// one workgroup: loss = 1000 (sum of the first nt0 values / n0 + sum of the other nt1 / n1), both sums in a fixed tree order;
// gradient rows written by the first term of each row (g must be zero on entry).  fgc_point_loss has one term per sample
// (nt = n); fgc_surface_loss three per completeness sample, the value on the first of them.
__global__ __launch_bounds__(PL_THREADS) void point_loss_finish_kernel(const int* __restrict__ rows,
                                                                       const float4* __restrict__ terms, int nt0, int nt1,
                                                                       int n0, int n1, float* __restrict__ loss,
                                                                       float* __restrict__ g) {
    __shared__ float s0[PL_THREADS], s1[PL_THREADS];
    const int tid = threadIdx.x;
    const int nt = nt0 + nt1;
    float a0 = 0.f, a1 = 0.f;
    for (int t = tid; t < nt; t += PL_THREADS) {
        if (t < nt0)
            a0 += terms[t].w;
        else
            a1 += terms[t].w;
    }
    s0[tid] = a0;
    s1[tid] = a1;
    __syncthreads();
    for (int h = PL_THREADS / 2; h > 0; h >>= 1) {
        if (tid < h) {
            s0[tid] += s0[tid + h];
            s1[tid] += s1[tid + h];
        }
        __syncthreads();
    }
    if (tid == 0) loss[0] = 1000.0f * (s0[0] / (float)n0 + s1[0] / (float)n1);
    if (!g) return;
    for (int t = tid; t < nt; t += PL_THREADS) {
        const int r = rows[t];
        if (r < 0) continue;
        bool first = true;
        for (int u = 0; u < t && first; ++u) first = rows[u] != r;
        if (!first) continue;
        float gx = 0.f, gy = 0.f, gz = 0.f;
        for (int u = t; u < nt; ++u) {
            if (rows[u] != r) continue;
            const float4 e = terms[u];
            gx += e.x;
            gy += e.y;
            gz += e.z;
        }
        g[3 * (size_t)r] = gx;
        g[3 * (size_t)r + 1] = gy;
        g[3 * (size_t)r + 2] = gz;
    }
}

void point_gather(const float* p, int np, const int* ind, int n, float* q, hipStream_t st) {
    FGC_LAUNCH("point_gather_kernel", st, point_gather_kernel, dim3(cdiv(n, 256)), dim3(256), 0, p, np, ind, n, q);
}

void point_loss_finish(const int* rows, const float4* terms, int nt0, int nt1, int n0, int n1, float* loss, float* g,
                       hipStream_t st) {
    FGC_LAUNCH("point_loss_finish_kernel", st, point_loss_finish_kernel, dim3(1), dim3(PL_THREADS), 0, rows, terms, nt0, nt1,
               n0, n1, loss, g);
}

}  // namespace fgc

using namespace fgc;

namespace {
struct PointLossWs {
    size_t nn, q0, q1, d0, x0, d1, x1, rows, terms, total;
};

PointLossWs point_loss_layout(int32_t np0, int32_t np1, int32_t ns0, int32_t ns1) {
    PointLossWs w;
    size_t o = 0;
    auto take = [&](size_t bytes) {
        const size_t at = o;
        o = align_up(o + bytes, 256);
        return at;
    };
    w.nn = take(std::max(fgc_nn_workspace_bytes(ns0, np1), fgc_nn_workspace_bytes(ns1, np0)));
    w.q0 = take((size_t)ns0 * 12);
    w.q1 = take((size_t)ns1 * 12);
    w.d0 = take((size_t)ns0 * 4);
    w.x0 = take((size_t)ns0 * 4);
    w.d1 = take((size_t)ns1 * 4);
    w.x1 = take((size_t)ns1 * 4);
    w.rows = take(((size_t)ns0 + ns1) * 4);
    w.terms = take(((size_t)ns0 + ns1) * 16);
    w.total = o;
    return w;
}
}  // namespace

extern "C" size_t fgc_point_loss_workspace_bytes(int32_t np0, int32_t np1, int32_t ns0, int32_t ns1) {
    if (np0 <= 0 || np1 <= 0 || ns0 <= 0 || ns1 <= 0) return 0;
    return point_loss_layout(np0, np1, ns0, ns1).total;
}

extern "C" int fgc_point_loss(const float* p0, int32_t np0, const float* p1, int32_t np1, const int32_t* i0, int32_t ns0,
                              const int32_t* i1, int32_t ns1, float threshold, float* loss, float* g_p0, void* workspace,
                              size_t workspace_bytes, void* stream) {
    FGC_CHECK_ARG(p0 && p1 && i0 && i1 && loss && workspace, "fgc_point_loss: null pointer");
    FGC_CHECK_ARG(np0 > 0 && np1 > 0 && ns0 > 0 && ns1 > 0, "fgc_point_loss: np0=%d np1=%d ns0=%d ns1=%d (all > 0)", np0, np1,
                  ns0, ns1);
    FGC_CHECK_ARG((int64_t)ns0 + ns1 <= FGC_POINT_LOSS_MAX_SAMPLES, "fgc_point_loss: ns0 + ns1 = %lld samples (at most %d)",
                  (long long)ns0 + ns1, FGC_POINT_LOSS_MAX_SAMPLES);
    const PointLossWs L = point_loss_layout(np0, np1, ns0, ns1);
    FGC_CHECK_ARG(workspace_bytes >= L.total, "fgc_point_loss: workspace too small (%zu < %zu bytes)", workspace_bytes, L.total);
    FGC_CHECK_ARG((uintptr_t)workspace % 256 == 0, "fgc_point_loss: workspace needs 256-byte alignment");
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    float* q0 = (float*)(ws + L.q0);
    float* q1 = (float*)(ws + L.q1);
    float* d0 = (float*)(ws + L.d0);
    int* x0 = (int*)(ws + L.x0);
    float* d1 = (float*)(ws + L.d1);
    int* x1 = (int*)(ws + L.x1);
    int* rows = (int*)(ws + L.rows);
    float4* terms = (float4*)(ws + L.terms);
    const size_t nnb = L.q0 - L.nn;
    point_gather(p0, np0, i0, ns0, q0, st);
    point_gather(p1, np1, i1, ns1, q1, st);
    int rc = fgc_nn_query(q0, ns0, p1, np1, nullptr, nullptr, d0, x0, ws + L.nn, nnb, stream);
    if (rc != FGC_OK) return rc;
    rc = fgc_nn_query(q1, ns1, p0, np0, nullptr, nullptr, d1, x1, ws + L.nn, nnb, stream);
    if (rc != FGC_OK) return rc;
    FGC_LAUNCH("point_loss_terms_kernel", st, point_loss_terms_kernel, dim3(cdiv(ns0 + ns1, 256)), dim3(256), 0, p0, np0, p1,
               np1, i0, ns0, i1, ns1, d0, x0, d1, x1, threshold, rows, terms);
    if (g_p0 && hipMemsetAsync(g_p0, 0, (size_t)np0 * 12, st) != hipSuccess) {
        fgc::set_error("fgc_point_loss: memset failed");
        return FGC_EHIP;
    }
    point_loss_finish(rows, terms, ns0, ns1, ns0, ns1, loss, g_p0, st);
    FGC_CHECK_LAUNCH("fgc_point_loss");
    return FGC_OK;
}
