// Dense face-normal loss of trainDoubleLossNet (faceNormalsLoss over ALL rows of head 0, train.py:1101, 1272-1294),
// forward and gradient.
//
// One workgroup per DL_ROWS rows, one row per thread: the ground-truth row is rotated in registers (rot3, the bits
// fgc_rotate_rows writes), a row whose rotated ground truth has an L1 norm <= 1e-3 is a fake node, and the angle is the
// one angular_loss_fwd_kernel computes (same expressions, same compiler flags).  Each workgroup leaves one partial
// {sum of angles, real rows}; a one-workgroup launch sums them in a fixed order into the loss.  The backward launch
// re-derives the real-row count from the partials in every workgroup (the same order again) and ADDS each row's gradient
// into g_fn: each row has one writer, so there are no atomics and no memset, and the result is the same bits from run to
// run and under hipGraph replay.
#include <math.h>

#include "fgc_common.h"
#include "fgc_pack.h"

namespace fgc {

constexpr int DL_ROWS = 256;     // rows per workgroup (= threads)

__device__ __forceinline__ float dl_block_sum(float v, float* red /* >= 4 floats LDS */) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    __syncthreads();
    if (lane == 0) red[wave] = v;
    __syncthreads();
    float t = 0.f;
#pragma unroll
    for (int w = 0; w < DL_ROWS / 64; ++w) t += red[w];
    return t;
}

// row r: the rotated ground truth g and the cosine dt with fn; false for a fake row
__device__ __forceinline__ bool dl_row(const float* __restrict__ fn, const float* __restrict__ gt,
                                       const float (&rm)[9], bool rot, int r, float (&g)[3], float& dt) {
    const float a = gt[3 * (size_t)r], b = gt[3 * (size_t)r + 1], c = gt[3 * (size_t)r + 2];
    if (rot) {
        rot3(rm, a, b, c, g[0], g[1], g[2]);
    } else {
        g[0] = a;
        g[1] = b;
        g[2] = c;
    }
    const float f0 = fn[3 * (size_t)r], f1 = fn[3 * (size_t)r + 1], f2 = fn[3 * (size_t)r + 2];
    dt = f0 * g[0] + f1 * g[1] + f2 * g[2];
    return !((fabsf(g[0]) + fabsf(g[1]) + fabsf(g[2])) <= 10e-4f);
}

__device__ __forceinline__ void dl_load_R(const float* __restrict__ Rd, float (&rm)[9]) {
#pragma unroll
    for (int i = 0; i < 9; ++i) rm[i] = Rd ? Rd[i] : 0.f;
}

// the real-row count (and the angle sum) over all partials, in one fixed order: every caller gets the same bits
__device__ __forceinline__ void dl_sum_partials(const float* __restrict__ part, int nblk, float* red, float& lsum,
                                                float& rsum) {
    float l = 0.f, c = 0.f;
    for (int i = threadIdx.x; i < nblk; i += DL_ROWS) {
        l += part[2 * i];
        c += part[2 * i + 1];
    }
    lsum = dl_block_sum(l, red);
    rsum = dl_block_sum(c, red);
}

__global__ __launch_bounds__(DL_ROWS) void dense_loss_partial_kernel(const float* __restrict__ fn,
                                                                     const float* __restrict__ gt,
                                                                     const float* __restrict__ Rd, int n,
                                                                     float* __restrict__ part) {
    __shared__ float red[DL_ROWS / 64];
    const float close = 0.9999999f;
    float rm[9];
    dl_load_R(Rd, rm);
    const int r = blockIdx.x * DL_ROWS + threadIdx.x;
    float lsum = 0.f, rsum = 0.f;
    if (r < n) {
        float g[3], dt;
        if (dl_row(fn, gt, rm, Rd != nullptr, r, g, dt)) {
            lsum = 180.f * acosf(fminf(fmaxf(dt, -close), close)) / 3.14159265358979323846f;
            rsum = 1.f;
        }
    }
    lsum = dl_block_sum(lsum, red);
    rsum = dl_block_sum(rsum, red);
    if (threadIdx.x == 0) {
        part[2 * blockIdx.x] = lsum;
        part[2 * blockIdx.x + 1] = rsum;
    }
}

// one workgroup: loss_out = {sum of angles / real rows, real rows}; total[0] = add[0] + loss when both are given
__global__ __launch_bounds__(DL_ROWS) void dense_loss_finish_kernel(const float* __restrict__ part, int nblk,
                                                                    float* __restrict__ loss_out,
                                                                    const float* __restrict__ add,
                                                                    float* __restrict__ total) {
    __shared__ float red[DL_ROWS / 64];
    float lsum, rsum;
    dl_sum_partials(part, nblk, red, lsum, rsum);
    if (threadIdx.x == 0) {
        const float loss = lsum / rsum;      // (no real row: 0 / 0, as the reference's)
        loss_out[0] = loss;
        loss_out[1] = rsum;
        if (total) total[0] = add[0] + loss;
    }
}

// g_fn[r] += dloss k (R gt_r),  k = -(180/pi) / sqrt(1 - dt^2) / nreal,  for real rows strictly inside the clip
// (tf.minimum / maximum pass no gradient outside it; angular_loss_bwd_kernel's arithmetic)
__global__ __launch_bounds__(DL_ROWS) void dense_loss_bwd_kernel(const float* __restrict__ fn,
                                                                 const float* __restrict__ gt,
                                                                 const float* __restrict__ Rd, int n,
                                                                 const float* __restrict__ part, int nblk, float dloss,
                                                                 float* __restrict__ g_fn) {
    __shared__ float red[DL_ROWS / 64];
    const float close = 0.9999999f;
    float rm[9];
    dl_load_R(Rd, rm);
    float lsum, nreal;
    dl_sum_partials(part, nblk, red, lsum, nreal);
    const int r = blockIdx.x * DL_ROWS + threadIdx.x;
    if (r >= n) return;
    float g[3], dt;
    if (!dl_row(fn, gt, rm, Rd != nullptr, r, g, dt)) return;
    if (dt > close || dt < -close) return;
    const float k = -(180.f / 3.14159265358979323846f) / sqrtf(1.f - dt * dt) * dloss / nreal;
#pragma unroll
    for (int c = 0; c < 3; ++c) g_fn[3 * (size_t)r + c] += k * g[c];
}

}  // namespace fgc

using namespace fgc;

extern "C" size_t fgc_dense_normals_loss_scratch_floats(int32_t n) {
    if (n <= 0) return 0;
    return 2 * (size_t)cdiv(n, DL_ROWS);
}

extern "C" int fgc_dense_normals_loss_fwd(const float* fn, const float* gt, const float* R, int32_t n, float* loss_out,
                                          const float* add, float* total, float* scratch, size_t scratch_floats,
                                          void* stream) {
    FGC_CHECK_ARG(fn && gt && loss_out && scratch, "fgc_dense_normals_loss_fwd: null pointer");
    FGC_CHECK_ARG(n > 0, "fgc_dense_normals_loss_fwd: n=%d (> 0)", n);
    FGC_CHECK_ARG((add == nullptr) == (total == nullptr), "fgc_dense_normals_loss_fwd: add and total go together");
    const size_t need = fgc_dense_normals_loss_scratch_floats(n);
    FGC_CHECK_ARG(scratch_floats >= need, "fgc_dense_normals_loss_fwd: scratch too small (%zu < %zu floats)",
                  scratch_floats, need);
    hipStream_t st = (hipStream_t)stream;
    const int nblk = cdiv(n, DL_ROWS);
    FGC_LAUNCH("dense_loss_partial_kernel", st, dense_loss_partial_kernel, dim3(nblk), dim3(DL_ROWS), 0, fn, gt, R, n,
               scratch);
    FGC_LAUNCH("dense_loss_finish_kernel", st, dense_loss_finish_kernel, dim3(1), dim3(DL_ROWS), 0, scratch, nblk,
               loss_out, add, total);
    FGC_CHECK_LAUNCH("fgc_dense_normals_loss_fwd");
    return FGC_OK;
}

extern "C" int fgc_dense_normals_loss_bwd(const float* fn, const float* gt, const float* R, int32_t n,
                                          const float* scratch, size_t scratch_floats, float dloss, float* g_fn,
                                          void* stream) {
    FGC_CHECK_ARG(fn && gt && scratch && g_fn, "fgc_dense_normals_loss_bwd: null pointer");
    FGC_CHECK_ARG(n > 0, "fgc_dense_normals_loss_bwd: n=%d (> 0)", n);
    const size_t need = fgc_dense_normals_loss_scratch_floats(n);
    FGC_CHECK_ARG(scratch_floats >= need, "fgc_dense_normals_loss_bwd: scratch too small (%zu < %zu floats)",
                  scratch_floats, need);
    FGC_CHECK_ARG(g_fn != fn, "fgc_dense_normals_loss_bwd: g_fn and fn must be distinct");
    hipStream_t st = (hipStream_t)stream;
    const int nblk = cdiv(n, DL_ROWS);
    FGC_LAUNCH("dense_loss_bwd_kernel", st, dense_loss_bwd_kernel, dim3(nblk), dim3(DL_ROWS), 0, fn, gt, R, n, scratch,
               nblk, dloss, g_fn);
    FGC_CHECK_LAUNCH("fgc_dense_normals_loss_bwd");
    return FGC_OK;
}
