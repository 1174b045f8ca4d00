// Per-facet MLP cin -> hidden -> cout with bf16-STORED activations (FGC_CONV_BF16 companion of fgc_mlp_f32.hip; the
// reference is fp32 only: model.py:763-769,937-941, train.py:409-427).
//
// x (and dx in backward) are bf16 tensors; W1, b1, W2, b2 and every gradient of them stay fp32 (master weights).  The
// matrix products with the 1024-wide hidden layer run on v_mfma_f32_16x16x32_bf16 with fp32 accumulation; bias, leaky
// ReLU, the forward 1024 -> 3 layer and every sum over nodes stay fp32 on the vector ALU / in the accumulators.  In the
// backward pass the two K = 3 / N = 3 products of that layer ride on the matrix pipe too (g = dy W2^T with hi + lo
// operand pairs, dW2 = hact^T dy with hact rounded to bf16 and dy as a hi + lo pair): they were a third of the vector
// work of kernels that the vector ALU bounds.  The hidden activation is never stored (recomputed in backward), exactly
// as in the fp32 kernels.  (Fragment layouts and tile constants: fgc_mlp_mb.h.)
#include "fgc_mlp.h"
#include "fgc_mlp_mb.h"

namespace fgc {

// (operand packs of the backward pass: fgc_pack.h)
__device__ __forceinline__ u32x4 mb_w2_frag(const u32x4* __restrict__ W2p, int ct, int lane) {
    const u32x4 v = W2p[ct * 32 + (lane & 31)];
    return lane < 32 ? v : u32x4{0u, 0u, 0u, 0u};
}
// A fragment of that product from a lane's dy row (o = 0..2)
__device__ __forceinline__ u32x4 mb_dy_frag(float d0, float d1, float d2, int lq) {
    const unsigned h01 = f2_to_bf2(d0, d1), h2x = f2_to_bf2(d2, 0.f);
    const f32x2c f01 = bf2_to_f2(h01), f2x = bf2_to_f2(h2x);
    const unsigned l01 = f2_to_bf2(d0 - f01[0], d1 - f01[1]), l2x = f2_to_bf2(d2 - f2x[0], 0.f);
    // lq 0: {hi0 hi1 | hi2 lo0 | lo1 lo2 | 0}    lq 1: {hi0 hi1 | hi2 0 | 0 | 0}
    const unsigned w1 = lq == 0 ? ((h2x & 0xFFFFu) | (l01 << 16)) : (h2x & 0xFFFFu);
    const unsigned w2 = lq == 0 ? ((l01 >> 16) | (l2x << 16)) : 0u;
    return lq < 2 ? u32x4{h01, w1, w2, 0u} : u32x4{0u, 0u, 0u, 0u};
}

// ---------------------------------------------------------------------------------------------
// forward.  A workgroup = 64 rows; wave w computes the hidden column tiles w, w+4, ... for all four 16-row tiles and folds
// them into the second layer on the spot.  The x fragments (16 bytes per lane, k-step and row tile) come straight from
// global memory once and stay in registers.  KS = cin / 32.
// ---------------------------------------------------------------------------------------------
template <int KS, int CO>
__global__ __launch_bounds__(MB_THREADS, 4) void mlp_fwd_bf16_kernel(const unsigned short* __restrict__ x, int n, int hidden,
                                                                     int cout, const u32x4* __restrict__ Wp16,
                                                                     const float* __restrict__ b1,
                                                                     const float* __restrict__ W2,
                                                                     const float* __restrict__ b2, float alpha,
                                                                     float* __restrict__ y, float* __restrict__ abs_partial) {
    __shared__ float ypart[4 * MB_FWD_T * 4];
    __shared__ float red[4];
    constexpr int CIN = KS * 32;
    const int row0 = blockIdx.x * MB_FWD_T;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, lr = lane & 15, lq = lane >> 4;
    const int nct = hidden >> 4;
    u32x4 a[MB_FWD_RT][KS];
#pragma unroll
    for (int r = 0; r < MB_FWD_RT; ++r) {
        const int row = min(row0 + r * 16 + lr, n - 1);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
            a[r][ks] = *reinterpret_cast<const u32x4*>(x + (size_t)row * CIN + ks * 32 + 8 * lq);
    }
    float yp[MB_FWD_RT][4][CO];
#pragma unroll
    for (int r = 0; r < MB_FWD_RT; ++r)
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int o = 0; o < CO; ++o) yp[r][t][o] = 0.f;

    u32x4 bnext[KS];
    float bbn = 0.f, w2n[CO];
    auto fetch_weights = [&](int ct) {   // (clamped: always a valid load)
        ct = min(ct, nct - 1);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) bnext[ks] = Wp16[((size_t)ks * nct + ct) * 64 + lane];
        bbn = b1[ct * 16 + lr];
#pragma unroll
        for (int o = 0; o < CO; ++o) w2n[o] = W2[(size_t)(ct * 16 + lr) * cout + min(o, cout - 1)];
    };
    fetch_weights(wave);
    for (int ct = wave; ct < nct; ct += 4) {
        u32x4 bcur[KS];
        float w2[CO];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) bcur[ks] = bnext[ks];
        const float bb = bbn;
#pragma unroll
        for (int o = 0; o < CO; ++o) w2[o] = o < cout ? w2n[o] : 0.f;
        fetch_weights(ct + 4);
        f32x4 h[MB_FWD_RT];
#pragma unroll
        for (int r = 0; r < MB_FWD_RT; ++r) h[r] = f32x4{bb, bb, bb, bb};   // the bias rides in the accumulator
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
#pragma unroll
            for (int r = 0; r < MB_FWD_RT; ++r)
                h[r] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a[r][ks]),
                                                              __builtin_bit_cast(bf16x8, bcur[ks]), h[r], 0, 0, 0);
#pragma unroll
        for (int r = 0; r < MB_FWD_RT; ++r)
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                float v = h[r][t];
                v = lrelu01(v, alpha);    // leaky ReLU for 0 <= alpha <= 1 (checked by the host)
#pragma unroll
                for (int o = 0; o < CO; ++o) yp[r][t][o] = fmaf(v, w2[o], yp[r][t][o]);
            }
    }
    // reduce over the 16 column lanes, then over the four waves (fixed order)
#pragma unroll
    for (int r = 0; r < MB_FWD_RT; ++r)
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int o = 0; o < CO; ++o) {
                float v = yp[r][t][o];
                FGC_ROW16_SUM(v);
                yp[r][t][o] = v;
            }
    if (lr == 0) {
#pragma unroll
        for (int r = 0; r < MB_FWD_RT; ++r)
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int o = 0; o < CO; ++o) ypart[(wave * MB_FWD_T + r * 16 + lq * 4 + t) * 4 + o] = yp[r][t][o];
    }
    __syncthreads();
    float asum = 0.f;
    for (int t = threadIdx.x; t < MB_FWD_T * cout; t += MB_THREADS) {
        const int r = t / cout, o = t % cout;
        const int row = row0 + r;
        if (row < n) {
            float v = b2[o];
            v += ypart[(0 * MB_FWD_T + r) * 4 + o];
            v += ypart[(1 * MB_FWD_T + r) * 4 + o];
            v += ypart[(2 * MB_FWD_T + r) * 4 + o];
            v += ypart[(3 * MB_FWD_T + r) * 4 + o];
            y[(size_t)row * cout + o] = v;
            asum += fabsf(v);
        }
    }
    if (abs_partial) {
        for (int off = 32; off > 0; off >>= 1) asum += __shfl_xor(asum, off);
        if (lane == 0) red[wave] = asum;
        __syncthreads();
        if (threadIdx.x == 0) abs_partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
    }
}

// ---------------------------------------------------------------------------------------------
// backward = two kernels, because the two big products want opposite loop orders and the bf16 MFMA makes recomputing
// the hidden layer nearly free (a fused kernel with the fp32 kernel's structure kept ~200 registers of partial sums
// alive and spilled; giving the waves of a workgroup the same rows cost three barriers per 32-row tile):
//   mlp_bwd_dx_bf16_kernel   row major: a wave owns 32 rows and walks ALL hidden columns, 32 at a time:
//        h^T = W1^T x^T + b1 and g^T = W2 dy^T (MFMA, operands swapped), dh = g * lrelu'(h) (vector ALU, fp32),
//        dx += dh W1^T (MFMA; the transposed C layout of dh IS the A layout, no LDS).  dx leaves as bf16, complete: no
//        partial slabs.
//   mlp_bwd_w_bf16_kernel    column major: a wave owns 64 hidden columns (blockIdx.y) and walks its share of the
//        32-row tiles with dW1 / db1 / dW2 partial sums in registers:
//        dW1 += x^T dh: K = the 32 rows of the tile, ONE MFMA per (16 input channels, 16 hidden columns); B = dh
//        straight out of the registers (k order: row tile, then 4*lq + reg), A = x^T out of a wave-private LDS tile
//        read in that same k order.  One fp32 slab per wave, summed in fixed order by reduce_jobs.
// No barrier inside either loop: nothing is shared between the waves of a workgroup except read-only weights.
// MT = cin / 16.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void mb_load_rows(const unsigned short* __restrict__ x, const float* __restrict__ dy, int n,
                                             int cout, int row0, int cin, int lane, u32x4* ax /* [MB_RT][KS] */, int ks_n,
                                             float* dyw) {
    const int lr = lane & 15, lq = lane >> 4;
#pragma unroll
    for (int r = 0; r < MB_RT; ++r) {
        const int row = row0 + r * 16 + lr;
        for (int ks = 0; ks < ks_n; ++ks) {
            const u32x4 v = *reinterpret_cast<const u32x4*>(x + (size_t)min(row, n - 1) * cin + ks * 32 + 8 * lq);
            ax[r * ks_n + ks] = row < n ? v : u32x4{0u, 0u, 0u, 0u};
        }
    }
    // dy rows of the tile into the wave's LDS tile [32][4]: lane l < 32 owns row l
    const int rr = row0 + (lane & 31);
    f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int o = 0; o < 4; ++o) {
        const float g = dy[(size_t)min(rr, n - 1) * cout + min(o, cout - 1)];
        v[o] = (rr < n && o < cout) ? g : 0.f;
    }
    if (lane < 32) *reinterpret_cast<f32x4*>(dyw + lane * 4) = v;
}

template <int MT>
__global__ __launch_bounds__(MBB_THREADS, MT <= 2 ? 3 : 2) void mlp_bwd_dx_bf16_kernel(
    const unsigned short* __restrict__ x, const float* __restrict__ dy, int n, int hidden, int cout,
    const u32x4* __restrict__ Wp16, const u32x4* __restrict__ W1d /* mlp_pack_w1dx_bf16_kernel */,
    const float* __restrict__ b1, const u32x4* __restrict__ W2p /* mlp_pack_w2_bf16_kernel */, float alpha,
    unsigned short* __restrict__ dx) {
    constexpr int CIN = MT * 16;
    constexpr int KS = CIN / 32;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, lr = lane & 15, lq = lane >> 4;
    const int nct = hidden >> 4;
    const int tile = blockIdx.x * MBB_WAVES + wave;
    const int row0 = tile * MB_T;
    if (row0 >= n) return;                    // (whole wave; nothing below is shared between waves)
    u32x4 ax[MB_RT * KS], gA[MB_RT];
#pragma unroll
    for (int r = 0; r < MB_RT; ++r) {
        const int row = row0 + r * 16 + lr;
        const size_t rc = (size_t)min(row, n - 1);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const u32x4 v = *reinterpret_cast<const u32x4*>(x + rc * CIN + ks * 32 + 8 * lq);
            ax[r * KS + ks] = row < n ? v : u32x4{0u, 0u, 0u, 0u};
        }
        // this lane's dy row as the A fragment of g = dy W2^T (rows past n: zero, so their dh is zero)
        float d[3];
#pragma unroll
        for (int o = 0; o < 3; ++o) d[o] = (row < n && o < cout) ? dy[rc * cout + min(o, cout - 1)] : 0.f;
        gA[r] = mb_dy_frag(d[0], d[1], d[2], lq);
    }
    f32x4 dxacc[MB_RT][MT];
#pragma unroll
    for (int r = 0; r < MB_RT; ++r)
#pragma unroll
        for (int m = 0; m < MT; ++m) dxacc[r][m] = f32x4{0.f, 0.f, 0.f, 0.f};

    // weights of one pair of column tiles (W1 fragments, b1, W2 fragments, W1 rows for the dx product): clamped, so that the
    // pair after the last is a valid (unused) load; fetched one pair ahead.
    // The two products that make dh are computed TRANSPOSED (operands swapped: h^T = W1^T x^T, g^T = W2 dy^T): in the C
    // layout a lane then holds ONE row (its lr) and the hidden columns 4*lq + t of a tile - with the two tiles of a pair,
    // eight k values of the A operand of dx += dh W1^T, straight out of the registers.  k slot j = c2*4 + t of lane group
    // lq stands for hidden column c2*16 + 4*lq + t; the W1 rows (B operand) are loaded in that same order.  No LDS.
    struct PairW {
        u32x4 bw[2][KS];
        f32x4 bb[2];
        u32x4 bg[2];
        u32x4 bt[MT];
    };
    auto fetch = [&](int pp, PairW& w) {
        pp = min(pp, (nct >> 1) - 1);
#pragma unroll
        for (int c2 = 0; c2 < 2; ++c2) {
            const int ct = pp * 2 + c2;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) w.bw[c2][ks] = Wp16[((size_t)ks * nct + ct) * 64 + lane];
            w.bb[c2] = *reinterpret_cast<const f32x4*>(b1 + ct * 16 + 4 * lq);
            w.bg[c2] = mb_w2_frag(W2p, ct, lane);
        }
#pragma unroll
        for (int m = 0; m < MT; ++m) w.bt[m] = W1d[((size_t)pp * MT + m) * 64 + lane];
    };
    auto pair = [&](const PairW& w) {
        f32x4 d[2][MB_RT];
#pragma unroll
        for (int c2 = 0; c2 < 2; ++c2) {
            f32x4 h[MB_RT], g[MB_RT];
#pragma unroll
            for (int r = 0; r < MB_RT; ++r) h[r] = w.bb[c2];
#pragma unroll
            for (int ks = 0; ks < KS; ++ks)
#pragma unroll
                for (int r = 0; r < MB_RT; ++r)
                    h[r] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, w.bw[c2][ks]),
                                                                  __builtin_bit_cast(bf16x8, ax[r * KS + ks]), h[r], 0, 0, 0);
#pragma unroll
            for (int r = 0; r < MB_RT; ++r)
                g[r] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, w.bg[c2]), __builtin_bit_cast(bf16x8, gA[r]),
                                                              f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
#pragma unroll
            for (int r = 0; r < MB_RT; ++r)
#pragma unroll
                for (int t = 0; t < 4; ++t) d[c2][r][t] = g[r][t] * lrelu01_slope(h[r][t], alpha);
        }
#pragma unroll
        for (int r = 0; r < MB_RT; ++r) {
            const u32x4 ad = u32x4{f2_to_bf2(d[0][r][0], d[0][r][1]), f2_to_bf2(d[0][r][2], d[0][r][3]),
                                   f2_to_bf2(d[1][r][0], d[1][r][1]), f2_to_bf2(d[1][r][2], d[1][r][3])};
#pragma unroll
            for (int m = 0; m < MT; ++m)
                dxacc[r][m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, ad), __builtin_bit_cast(bf16x8, w.bt[m]),
                                                                     dxacc[r][m], 0, 0, 0);
        }
    };
    // cout > 3 (a fourth output column) is folded in by a second sweep below: the network's heads have three
    PairW wa, wb;
    const int npairs = nct >> 1;
    fetch(0, wa);
    // sched_barrier: keep the program order "request the next pair, then work on this one" (left alone the scheduler sinks
    // every request to the end of the iteration and waits for all of them at the top of the next: no load ever overlaps
    // a product)
#pragma unroll 1
    for (int pp = 0; pp < npairs; pp += 2) {
        fetch(pp + 1, wb);
        __builtin_amdgcn_sched_barrier(0);
        pair(wa);
        __builtin_amdgcn_sched_barrier(0);
        fetch(pp + 2, wa);
        __builtin_amdgcn_sched_barrier(0);
        pair(wb);                 // (hidden % 256 == 0: the pair count is even; a conditional here lets the compiler sink
                                  //  the loads of wb into the branch, next to their use)
        __builtin_amdgcn_sched_barrier(0);
    }
    // C layout: column = input channel lr of tile m, rows 4*lq + t
#pragma unroll
    for (int r = 0; r < MB_RT; ++r)
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int row = row0 + r * 16 + lq * 4 + t;
            if (row < n) {
#pragma unroll
                for (int m = 0; m < MT; ++m) dx[(size_t)row * CIN + m * 16 + lr] = f_to_bf(dxacc[r][m][t]);
            }
        }
}

template <int MT, int CO>
__global__ __launch_bounds__(MBB_THREADS, 2) void mlp_bwd_w_bf16_kernel(
    const unsigned short* __restrict__ x, const float* __restrict__ dy, int n, int hidden, int cout,
    const u32x4* __restrict__ Wp16, const float* __restrict__ b1, const u32x4* __restrict__ W2p, float alpha,
    float* __restrict__ dW1_slab /* [walkers][cin][hidden] */, float* __restrict__ db1_slab /* [walkers][hidden] */,
    float* __restrict__ dW2_slab /* [walkers][hidden][4] */, float* __restrict__ db2_slab /* [walkers][4] */) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    constexpr int CIN = MT * 16;
    constexpr int KS = CIN / 32;
    constexpr int XTS = MB_T * 2 + 8;         // bytes per row (= input channel) of a wave's transposed x tile
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, lr = lane & 15, lq = lane >> 4;
    char* xT = smem_raw + wave * (CIN * XTS + MB_T * 16);
    float* dyw = reinterpret_cast<float*>(xT + CIN * XTS);
    unsigned short* xT16 = reinterpret_cast<unsigned short*>(xT);
    const int hc0 = blockIdx.y * MBW_HCW;
    const int nct = hidden >> 4;
    const int ntiles = (n + MB_T - 1) / MB_T;
    const int walker = blockIdx.x * MBB_WAVES + wave, nwalkers = gridDim.x * MBB_WAVES;

    u32x4 bw[MBW_CT][KS], bg[MBW_CT];
    float bb[MBW_CT];
#pragma unroll
    for (int c = 0; c < MBW_CT; ++c) {
        const int ct = (hc0 >> 4) + c;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) bw[c][ks] = Wp16[((size_t)ks * nct + ct) * 64 + lane];
        bb[c] = b1[ct * 16 + lr];
        bg[c] = mb_w2_frag(W2p, ct, lane);
    }
    // dW1acc: C layout of x^T dh (column = hidden column lr, row = input channel 4*lq + t of tile m)
    // dW2acc: C layout of hact^T dy (column = output o = lr, row = hidden column 4*lq + t of tile c): lanes lr < cout count
    f32x4 dW1acc[MBW_CT][MT], dW2acc[MBW_CT];
    float db1acc[MBW_CT], db2acc = 0.f;
#pragma unroll
    for (int c = 0; c < MBW_CT; ++c) {
        db1acc[c] = 0.f;
        dW2acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int m = 0; m < MT; ++m) dW1acc[c][m] = f32x4{0.f, 0.f, 0.f, 0.f};
    }

#pragma unroll 1
    for (int tile = walker; tile < ntiles; tile += nwalkers) {
        const int row0 = tile * MB_T;
        u32x4 ax[MB_RT * KS];
        mb_load_rows(x, dy, n, cout, row0, CIN, lane, ax, KS, dyw);
        // x^T of the tile for the dW1 product
#pragma unroll
        for (int r = 0; r < MB_RT; ++r)
#pragma unroll
            for (int ks = 0; ks < KS; ++ks)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int c = ks * 32 + 8 * lq + 2 * e;
                    xT16[(c * XTS) / 2 + r * 16 + lr] = (unsigned short)(ax[r * KS + ks][e] & 0xFFFFu);
                    xT16[((c + 1) * XTS) / 2 + r * 16 + lr] = (unsigned short)(ax[r * KS + ks][e] >> 16);
                }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        // dy of the tile in the two operand layouts it is needed in:
        //   gA[r]    A of g = dy W2^T: this lane's row r*16 + lr (mb_dy_frag)
        //   dyh/dyl  B of dW2 += hact^T dy: lane (o = lr, lq), k slot j <-> row (j >> 2) * 16 + 4*lq + (j & 3) - the row
        //            order in which a lane holds its hidden column in the C layout - as bf16 hi and lo parts
        u32x4 gA[MB_RT], dyh, dyl;
#pragma unroll
        for (int r = 0; r < MB_RT; ++r) {
            const f32x4 d = *reinterpret_cast<const f32x4*>(dyw + (r * 16 + lr) * 4);
            gA[r] = mb_dy_frag(d[0], d[1], d[2], lq);
        }
        {
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float d = dyw[((j >> 2) * 16 + 4 * lq + (j & 3)) * 4 + (lr & 3)];
                v[j] = lr < CO ? d : 0.f;
            }
            if (blockIdx.y == 0) db2acc += ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
            unsigned hh[4], ll[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                hh[q] = f2_to_bf2(v[2 * q], v[2 * q + 1]);
                const f32x2c f = bf2_to_f2(hh[q]);
                ll[q] = f2_to_bf2(v[2 * q] - f[0], v[2 * q + 1] - f[1]);
            }
            dyh = u32x4{hh[0], hh[1], hh[2], hh[3]};
            dyl = u32x4{ll[0], ll[1], ll[2], ll[3]};
        }
        u32x4 af[MT];
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            const char* row = xT + (m * 16 + lr) * XTS;
            const u32x2 lo = *reinterpret_cast<const u32x2*>(row + lq * 8);          // rows 4*lq .. +3
            const u32x2 hi = *reinterpret_cast<const u32x2*>(row + 32 + lq * 8);     // rows 16 + 4*lq .. +3
            af[m] = u32x4{lo[0], lo[1], hi[0], hi[1]};
        }
#pragma unroll
        for (int c = 0; c < MBW_CT; ++c) {
            __builtin_amdgcn_sched_barrier(0);    // one column tile at a time
            f32x4 h[MB_RT], g[MB_RT];
#pragma unroll
            for (int r = 0; r < MB_RT; ++r) h[r] = f32x4{bb[c], bb[c], bb[c], bb[c]};
#pragma unroll
            for (int ks = 0; ks < KS; ++ks)
#pragma unroll
                for (int r = 0; r < MB_RT; ++r)
                    h[r] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, ax[r * KS + ks]),
                                                                  __builtin_bit_cast(bf16x8, bw[c][ks]), h[r], 0, 0, 0);
#pragma unroll
            for (int r = 0; r < MB_RT; ++r)
                g[r] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, gA[r]), __builtin_bit_cast(bf16x8, bg[c]),
                                                              f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
            // lrelu(pre) = pre * lrelu'(pre): one multiply instead of a multiply and a max
            f32x4 ha[MB_RT];
#pragma unroll
            for (int r = 0; r < MB_RT; ++r)
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const float slope = lrelu01_slope(h[r][t], alpha);
                    ha[r][t] = h[r][t] * slope;
                    g[r][t] *= slope;
                    db1acc[c] += g[r][t];
                }
            // k = r*16 + 4*lq + t: element j of the fragments is (r = j >> 2, t = j & 3)
            const u32x4 bf = u32x4{f2_to_bf2(g[0][0], g[0][1]), f2_to_bf2(g[0][2], g[0][3]), f2_to_bf2(g[1][0], g[1][1]),
                                   f2_to_bf2(g[1][2], g[1][3])};
            const u32x4 hf = u32x4{f2_to_bf2(ha[0][0], ha[0][1]), f2_to_bf2(ha[0][2], ha[0][3]), f2_to_bf2(ha[1][0], ha[1][1]),
                                   f2_to_bf2(ha[1][2], ha[1][3])};
#pragma unroll
            for (int m = 0; m < MT; ++m)
                dW1acc[c][m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, af[m]), __builtin_bit_cast(bf16x8, bf),
                                                                      dW1acc[c][m], 0, 0, 0);
            // dW2 += hact^T dy (smaller term first)
            dW2acc[c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, hf), __builtin_bit_cast(bf16x8, dyl),
                                                               dW2acc[c], 0, 0, 0);
            dW2acc[c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, hf), __builtin_bit_cast(bf16x8, dyh),
                                                               dW2acc[c], 0, 0, 0);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   // the next tile overwrites the LDS tiles
    }
    // parameter-gradient slabs of this wave (slab index = its walker id)
    if (blockIdx.y == 0) {   // db2[o]: lanes (lr = o, lq) hold the sums of their rows
        float v = db2acc;
        v += __shfl_xor(v, 16);
        v += __shfl_xor(v, 32);
        if (lq == 0 && lr < 4) db2_slab[walker * 4 + lr] = lr < CO ? v : 0.f;
    }
#pragma unroll
    for (int c = 0; c < MBW_CT; ++c) {
        const int col = hc0 + c * 16 + lr;
        // dW1acc C layout: column = lr (hidden column), row = 4*lq + t (input channel within tile m)
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int t = 0; t < 4; ++t)
                dW1_slab[((size_t)walker * CIN + m * 16 + lq * 4 + t) * hidden + col] = dW1acc[c][m][t];
        float v = db1acc[c];
        v += __shfl_xor(v, 16);
        v += __shfl_xor(v, 32);
        if (lq == 0) db1_slab[(size_t)walker * hidden + col] = v;
        // dW2acc C layout: column = lr (output o), row = 4*lq + t (hidden column within tile c)
        if (lr < 4) {
#pragma unroll
            for (int t = 0; t < 4; ++t)
                dW2_slab[((size_t)walker * hidden + hc0 + c * 16 + lq * 4 + t) * 4 + lr] = lr < CO ? dW2acc[c][t] : 0.f;
        }
    }
}

}  // namespace fgc

namespace fgc {

template <int KS, int CO>
static int fwd_bf16(const MlpShape& s, const MlpFwdPlan& p, const MlpFwdArgs& a, hipStream_t st) {
    return launch_kernel<mlp_fwd_bf16_kernel<KS, CO>>(LaunchCfg{"mlp_fwd_kernel", "fgc_mlp_fwd_bf16", st, p.gx, MB_THREADS, 0},
                                                      (const unsigned short*)a.x, s.n, s.hidden, s.cout, (const u32x4*)(a.ws + p.w1.off),
                                                      a.b1, a.W2, a.b2, a.alpha, a.y, a.abs_partial);
}
int launch_mlp_fwd_bf16(const MlpShape& s, const MlpFwdPlan& p, const MlpFwdArgs& a, hipStream_t st) {
    switch (p.ks) {
        case 1: return p.co == 3 ? fwd_bf16<1, 3>(s, p, a, st) : fwd_bf16<1, 4>(s, p, a, st);
        case 2: return p.co == 3 ? fwd_bf16<2, 3>(s, p, a, st) : fwd_bf16<2, 4>(s, p, a, st);
        default: return p.co == 3 ? fwd_bf16<4, 3>(s, p, a, st) : fwd_bf16<4, 4>(s, p, a, st);
    }
}

template <int MT>
static int bwd_bf16(const MlpShape& s, const MlpBwdPlan& p, const MlpBwdArgs& a, hipStream_t st) {
    const unsigned short* x = (const unsigned short*)a.x;
    const u32x4 *Wp16 = (const u32x4*)(a.ws + p.wp), *W1d = (const u32x4*)(a.ws + p.w1d), *W2p = (const u32x4*)(a.ws + p.w2p);
    int rc = launch_kernel<mlp_bwd_dx_bf16_kernel<MT>>(LaunchCfg{"mlp_bwd_kernel<dx>", "fgc_mlp_bwd_bf16", st, p.dx_gx, MBB_THREADS, 0}, x,
                                                       a.dy, s.n, s.hidden, s.cout, Wp16, W1d, a.b1, W2p, a.alpha, (unsigned short*)a.dx);
    if (rc) return rc;
    return launch_kernel<mlp_bwd_w_bf16_kernel<MT, 3>>(LaunchCfg{"mlp_bwd_kernel<w>", "fgc_mlp_bwd_bf16", st, p.gx, MBB_THREADS, p.smem, p.gy},
                                                       x, a.dy, s.n, s.hidden, s.cout, Wp16, a.b1, W2p, a.alpha, (float*)(a.ws + p.dW1),
                                                       (float*)(a.ws + p.db1), (float*)(a.ws + p.dW2), (float*)(a.ws + p.db2));
}
int launch_mlp_bwd_bf16(const MlpShape& s, const MlpBwdPlan& p, const MlpBwdArgs& a, hipStream_t st) {
    return p.mt == 2 ? bwd_bf16<2>(s, p, a, st) : bwd_bf16<4>(s, p, a, st);
}

}  // namespace fgc
