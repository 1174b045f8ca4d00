// Per-facet MLP cin -> hidden -> cout of the fp32 network on the bf16 matrix pipe: fp32 activations in and out, every operand
// of a 1024-wide product a three-term bf16 split.  The kernels have the structure of the bf16-storage ones (fgc_mlp_bf16.hip).
// ---------------------------------------------------------------------------------------------
// fp32 operands on the bf16 matrix pipe (the fp32 network's MLP).  v_mfma_f32_16x16x4_f32 runs at the vector FMA rate and
// shares the SIMD with the vector ALU; the bf16 pipe is 16 times faster and runs beside it.  An
// fp32 value is split into three bf16 terms v = v0 + v1 + v2 (v0 = bf16(v), v1 = bf16(v - v0), v2 = bf16(v - v0 - v1): 3 x 8
// significand bits >= the 24 of fp32, same exponent range), and a product a b is the six bf16 MFMAs a0 b2 + a2 b0 + a1 b1 +
// a0 b1 + a1 b0 + a0 b0 accumulated in fp32, smallest terms first.  Each bf16 x bf16 product is exact in fp32; the three
// terms left out (a1 b2, a2 b1, a2 b2) are below 2^-25 of the product: the result differs from the fp32-MFMA kernel's by
// summation order only (tests/test_gpu_ops.py compares the two).  FGC_NO_MLP_SPLIT=1 keeps the fp32 MFMA kernels.
// ---------------------------------------------------------------------------------------------
#include "fgc_mlp.h"
#include "fgc_mlp_mb.h"
#include "fgc_split.h"

namespace fgc {

// forward: the bf16 kernel's structure (a workgroup = 64 rows, wave w walks the hidden column tiles w, w + 4, ...); x is
// fp32 and is split once per workgroup, the weights come split from mlp_pack_split_body.
template <int KS, int CO>
__global__ __launch_bounds__(MB_THREADS, 2) void mlp_fwd_split_kernel(const float* __restrict__ x, int n, int hidden, int cout,
                                                                      const u32x4* __restrict__ Wp16,
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
    const size_t plane = (size_t)KS * nct * 64;            // u32x4 per plane
    u32x4 a[MB_FWD_RT][KS][3];
#pragma unroll
    for (int r = 0; r < MB_FWD_RT; ++r) {
        const int row = min(row0 + r * 16 + lr, n - 1);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const f32x4* src = reinterpret_cast<const f32x4*>(x + (size_t)row * CIN + ks * 32 + 8 * lq);
            u32x2 lo[3], hi[3];
            split3(src[0], lo[0], lo[1], lo[2]);
            split3(src[1], hi[0], hi[1], hi[2]);
#pragma unroll
            for (int p = 0; p < 3; ++p) a[r][ks][p] = u32x4{lo[p][0], lo[p][1], hi[p][0], hi[p][1]};
        }
    }
    float yp[MB_FWD_RT][4][CO];
#pragma unroll
    for (int r = 0; r < MB_FWD_RT; ++r)
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int o = 0; o < CO; ++o) yp[r][t][o] = 0.f;

    u32x4 bnext[KS][3];
    float bbn = 0.f, w2n[CO];
    auto fetch_weights = [&](int ct) {   // (clamped: always a valid load)
        ct = min(ct, nct - 1);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
#pragma unroll
            for (int p = 0; p < 3; ++p) bnext[ks][p] = Wp16[p * plane + ((size_t)ks * nct + ct) * 64 + lane];
        bbn = b1[ct * 16 + lr];
#pragma unroll
        for (int o = 0; o < CO; ++o) w2n[o] = W2[(size_t)(ct * 16 + lr) * cout + min(o, cout - 1)];
    };
    fetch_weights(wave);
    for (int ct = wave; ct < nct; ct += 4) {
        u32x4 bcur[KS][3];
        float w2[CO];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
#pragma unroll
            for (int p = 0; p < 3; ++p) bcur[ks][p] = bnext[ks][p];
        const float bb = bbn;
#pragma unroll
        for (int o = 0; o < CO; ++o) w2[o] = o < cout ? w2n[o] : 0.f;
        fetch_weights(ct + 4);
        f32x4 h[MB_FWD_RT];
#pragma unroll
        // (the bias rides in the accumulator: the small terms of the split product then lose what lies below the last place of
        //  max(|b1|, |x W1|) - below the last place of the result; one vector add per hidden activation less)
        for (int r = 0; r < MB_FWD_RT; ++r) h[r] = f32x4{bb, bb, bb, bb};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
#pragma unroll
            for (int r = 0; r < MB_FWD_RT; ++r) h[r] = mfma_split(a[r][ks], bcur[ks], h[r]);
#pragma unroll
        for (int r = 0; r < MB_FWD_RT; ++r)
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                float v = h[r][t];
                v = lrelu01(v, alpha);
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
// The fp32 network's MLP BACKWARD on the bf16 matrix pipe.  mlp_bwd_kernel (fgc_mlp_f32.hip) spends 61 % of its SIMD
// cycles in v_mfma_f32_16x16x4_f32, which run at the vector FMA rate and keep the vector ALU from issuing (DESIGN.md
// section 3.1).  Here the two backward kernels of fgc_mlp_bf16.hip - the structure whose loop orders fit the two big products -
// take fp32 x and write fp32 dx, and every operand of a 1024-wide product is a three-term bf16 split (fgc_split.h): x once per row
// tile, W1 at pack time, dh = g * lrelu'(h) in registers right where it is produced (4.5 vector instructions per hidden
// activation against the 64 multiply-adds it then feeds).  g = dy W2^T (K = 3) is ONE MFMA whose 32 k slots hold the six
// significant term pairs of its three products (split_k3_frag); dW2 = hact^T dy and db2 stay fp32 on the vector ALU (three
// FMAs per hidden activation - cheaper than splitting hact).  The bias starts in the accumulator of the recomputed hidden
// layer (one vector add per activation less): the small terms of the split product are then added to a sum that already
// holds b1 - they lose what lies below the last place of max(|b1|, |x W1|), which is below the last place of the result.  Same results as the fp32-MFMA kernel up to summation order
// (tests/test_gpu_ops.py holds both against float64 at the same bound).  FGC_NO_MLP_BWD_SPLIT=1 keeps mlp_bwd_kernel.
// ---------------------------------------------------------------------------------------------
typedef short mbs_s16x4 __attribute__((ext_vector_type(4)));
// A fragment of x^T (rows = input channels col0 .. col0 + 15, k = the tile's rows in the order a lane holds its hidden
// column in the C layout: element j <-> row (j >> 2) * 16 + 4*lq + (j & 3)) out of a row-major plane, by two transposed reads
__device__ __forceinline__ u32x4 mbs_xT_frag(const char* plane, int stride, int col0, int lq, int lr) {
    const char* a = plane + (4 * lq + (lr >> 2)) * stride + (col0 + 4 * (lr & 3)) * 2;
    const mbs_s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) mbs_s16x4*)a);
    const mbs_s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) mbs_s16x4*)(a + 16 * stride));
    const u32x2 l2 = __builtin_bit_cast(u32x2, lo), h2 = __builtin_bit_cast(u32x2, hi);
    return u32x4{l2[0], l2[1], h2[0], h2[1]};
}
__device__ __forceinline__ float keep_if(float v, bool c) { return __uint_as_float(__float_as_uint(v) & (c ? ~0u : 0u)); }
__device__ __forceinline__ f32x4 keep_if(const f32x4& v, bool c) {
    return f32x4{keep_if(v[0], c), keep_if(v[1], c), keep_if(v[2], c), keep_if(v[3], c)};
}

// The weights of a pair of column tiles - 6 KS W1 fragments for h, 2 W2 operands for g, 3 MT W1 fragments for dx: 14 KB at
// cin = 32 - are the same for every wave: the workgroup stages them in LDS ONCE per pair (each thread moves four 16-byte
// pieces, requested one pair ahead through registers) and its four waves read them from there.  Loading them per wave, as
// the bf16 kernel does with a third of the bytes, kept the texture-address path busy with 2 GB per launch and the
// double-buffered fragments took 128 registers.  One barrier per pair.
template <int MT>
__global__ __launch_bounds__(MBB_THREADS, 3) void mlp_bwd_dx_split_kernel(
    const float* __restrict__ x, const float* __restrict__ dy, int n, int hidden, int cout,
    const u32x4* __restrict__ Wp16 /* mlp_pack_split_body: three planes */, const u32x4* __restrict__ W1d /* mlp_pack_w1dx_split_body */,
    const float* __restrict__ b1, const u32x4* __restrict__ W2s /* mlp_pack_w2_split_body */, float alpha, float* __restrict__ dx) {
    constexpr int CIN = MT * 16;
    constexpr int KS = CIN / 32;
    constexpr int NF = 6 * KS + 2 + 3 * MT;     // fragments per pair: bw[c2][ks][p], bg[c2], bt[m][p]
    constexpr int NI = (NF * 64 + MBB_THREADS - 1) / MBB_THREADS;   // 16-byte pieces per thread
    __shared__ u32x4 wl[2][NI * MBB_THREADS];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, lr = lane & 15, lq = lane >> 4;
    const int nct = hidden >> 4;
    const int tile = blockIdx.x * MBB_WAVES + wave;
    const int row0 = tile * MB_T;               // (a wave past the last row keeps walking: the barriers are the workgroup's)
    const size_t wplane = (size_t)KS * nct * 64;               // u32x4 per plane of Wp16
    const size_t dplane = (size_t)(nct >> 1) * MT * 64;        // ... of W1d
    // this thread's pieces of a pair: source of pair 0 and the step from pair to pair (in u32x4)
    const u32x4* src[NI];
    int step[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int item = threadIdx.x + i * MBB_THREADS, f = min(item >> 6, NF - 1), l = item & 63;
        if (f < 6 * KS) {
            const int c2 = f / (3 * KS), ks = (f / 3) % KS, p = f % 3;
            src[i] = Wp16 + p * wplane + ((size_t)ks * nct + c2) * 64 + l;
            step[i] = 128;
        } else if (f < 6 * KS + 2) {
            src[i] = W2s + (f - 6 * KS) * 64 + l;
            step[i] = 128;
        } else {
            const int g = f - 6 * KS - 2, m = g / 3, p = g % 3;
            src[i] = W1d + p * dplane + (size_t)m * 64 + l;
            step[i] = MT * 64;
        }
    }
    u32x4 ax[MB_RT][KS][3], gA[MB_RT];
#pragma unroll
    for (int r = 0; r < MB_RT; ++r) {
        const int row = row0 + r * 16 + lr;
        const size_t rc = (size_t)min(row, n - 1);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const f32x4* s4 = reinterpret_cast<const f32x4*>(x + rc * CIN + ks * 32 + 8 * lq);
            // (unconditional loads from the clamped row, zeroed by a bit mask: no load under an exec mask)
            split3_frag(keep_if(s4[0], row < n), keep_if(s4[1], row < n), ax[r][ks]);
        }
        float d[3];
#pragma unroll
        for (int o = 0; o < 3; ++o) d[o] = keep_if(dy[rc * cout + min(o, cout - 1)], row < n && o < cout);
        gA[r] = split_k3_frag(d, lq, 0);      // rows past n: zero, so their dh is zero
    }
    f32x4 dxacc[MB_RT][MT], dxlo[MB_RT][MT];      // (large and small terms apart: mfma_split2)
#pragma unroll
    for (int r = 0; r < MB_RT; ++r)
#pragma unroll
        for (int m = 0; m < MT; ++m) dxacc[r][m] = dxlo[r][m] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int npairs = nct >> 1;
    u32x4 stage[NI];
    f32x4 bbn[2];
    auto request = [&](int pp) {               // (clamped: the request behind the last pair is a valid, unused load)
        pp = min(pp, npairs - 1);
#pragma unroll
        for (int i = 0; i < NI; ++i) stage[i] = src[i][(size_t)pp * step[i]];
#pragma unroll
        for (int c2 = 0; c2 < 2; ++c2) bbn[c2] = *reinterpret_cast<const f32x4*>(b1 + (pp * 2 + c2) * 16 + 4 * lq);
    };
    auto park = [&](int buf) {
#pragma unroll
        for (int i = 0; i < NI; ++i) wl[buf][threadIdx.x + i * MBB_THREADS] = stage[i];
    };
    request(0);
    park(0);
    __syncthreads();
    // as mlp_bwd_dx_bf16_kernel: both products that make dh are computed transposed, so that dh leaves the accumulators in
    // the A layout of dx += dh W1^T
#pragma unroll 1
    for (int pp = 0; pp < npairs; ++pp) {
        const u32x4* w = wl[pp & 1] + lane;
        const f32x4 bb[2] = {bbn[0], bbn[1]};
        request(pp + 1);
        __builtin_amdgcn_sched_barrier(0);
        f32x4 d[2][MB_RT];
#pragma unroll
        for (int c2 = 0; c2 < 2; ++c2) {
            f32x4 h[MB_RT], g[MB_RT];
#pragma unroll
            for (int r = 0; r < MB_RT; ++r) h[r] = bb[c2];     // (the bias rides in the accumulator: below)
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                const u32x4 bw[3] = {w[((c2 * KS + ks) * 3 + 0) * 64], w[((c2 * KS + ks) * 3 + 1) * 64], w[((c2 * KS + ks) * 3 + 2) * 64]};
#pragma unroll
                for (int r = 0; r < MB_RT; ++r) h[r] = mfma_split(bw, ax[r][ks], h[r]);
            }
            const u32x4 bg = w[(6 * KS + c2) * 64];
#pragma unroll
            for (int r = 0; r < MB_RT; ++r)
                g[r] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, bg), __builtin_bit_cast(bf16x8, gA[r]),
                                                              f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
#pragma unroll
            for (int r = 0; r < MB_RT; ++r)
#pragma unroll
                for (int t = 0; t < 4; ++t) d[c2][r][t] = g[r][t] * lrelu01_slope(h[r][t], alpha);
        }
        u32x4 ad[MB_RT][3];
#pragma unroll
        for (int r = 0; r < MB_RT; ++r) split3_frag(d[0][r], d[1][r], ad[r]);
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            const u32x4 bt[3] = {w[(6 * KS + 2 + m * 3 + 0) * 64], w[(6 * KS + 2 + m * 3 + 1) * 64], w[(6 * KS + 2 + m * 3 + 2) * 64]};
#pragma unroll
            for (int r = 0; r < MB_RT; ++r) mfma_split2(ad[r], bt, dxacc[r][m], dxlo[r][m]);
        }
        __builtin_amdgcn_sched_barrier(0);
        park((pp + 1) & 1);                   // (buffer (pp + 1) & 1 was last read in iteration pp - 1, before its barrier)
        __syncthreads();
    }
    // C layout: column = input channel lr of tile m, rows 4*lq + t
#pragma unroll
    for (int r = 0; r < MB_RT; ++r)
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int row = row0 + r * 16 + lq * 4 + t;
            if (row < n) {
#pragma unroll
                for (int m = 0; m < MT; ++m) dx[(size_t)row * CIN + m * 16 + lr] = dxacc[r][m][t] + dxlo[r][m][t];
            }
        }
}

// Parameter gradients.  A WORKGROUP walks the 32-row tiles; its four waves own 64 hidden columns each (256 per workgroup,
// blockIdx.y picks the quarter of the hidden layer) and share everything that belongs to the rows: the tile's x split into
// three planes, dy, and the dy operand of the g product are staged in LDS once per workgroup - each wave splits a
// quarter of the rows - one tile ahead (requested before the current tile's products, parked behind them, one barrier per
// tile).  The first version gave every wave its own tiles: 16 column slices each split the same x and built the same dy
// operand (270 of its 700 vector instructions per tile) and waited for its own loads at the top of every tile.
//   LDS: 2 x { x [32 rows][plane 0 | plane 1 | plane 2 | pad] bf16, dy [32][4] fp32, dy operand [32][3 lane groups] } +
//   per wave its W1 fragments [c][ks][plane][lane] (they do not change over the walk; as registers they were 48 of 256).
// all nine dwords of the dy operand of one row (split_k3_frag, side 0): lane group lq takes dwords 4 lq .. 4 lq + 3
__device__ __forceinline__ void split_k3_row(const float (&v)[3], unsigned (&w)[9]) {
    unsigned short p[3][3];
#pragma unroll
    for (int o = 0; o < 3; ++o) split3_scalar(v[o], p[o]);
    constexpr int PD[6] = {0, 0, 1, 1, 0, 2};
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        const int s0 = 2 * i, s1 = 2 * i + 1;
        w[i] = (unsigned)p[s0 % 3][PD[s0 / 3]] | ((unsigned)p[s1 % 3][PD[s1 / 3]] << 16);
    }
}

template <int MT>
__global__ __launch_bounds__(MBB_THREADS, 2) void mlp_bwd_w_split_kernel(
    const float* __restrict__ x, const float* __restrict__ dy, int n, int hidden, int cout,
    const u32x4* __restrict__ Wp16, const float* __restrict__ b1, const u32x4* __restrict__ W2s, float alpha,
    float* __restrict__ dW1_slab /* [walkers][cin][hidden] */, float* __restrict__ db1_slab /* [walkers][hidden] */,
    float* __restrict__ dW2_slab /* [walkers][hidden][4] */, float* __restrict__ db2_slab /* [walkers][4] */) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    constexpr int CIN = MT * 16;
    constexpr int KS = CIN / 32;
    static_assert(KS == 1, "staging below moves one 16-byte piece of a 32-channel row per lane");
    constexpr int XTS = MBS_XTS(CIN);         // row stride of the x tile, == 32 bytes mod 64 (conflict-free transposed reads)
    constexpr int XPL = CIN * 2;              // byte offset of a plane within a row
    constexpr int TILE = MBS_TILE_LDS(CIN);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, lr = lane & 15, lq = lane >> 4;
    const int hc0 = blockIdx.y * (MBB_WAVES * MBW_HCW) + wave * MBW_HCW;
    const int nct = hidden >> 4;
    const int ntiles = (n + MB_T - 1) / MB_T;
    const int walker = blockIdx.x, nwalkers = gridDim.x;
    const size_t wplane = (size_t)KS * nct * 64;

    // the wave's weights do not change over its walk: W1 fragments (three planes: 48 registers - affordable since the file is
    // compiled without the SLP vectoriser, which had the kernel at 226 registers; in LDS they were 12 reads per tile), b1 and
    // the W2 operand
    u32x4 bw[MBW_CT][KS][3], bg[MBW_CT];
    float bb[MBW_CT];
#pragma unroll
    for (int c = 0; c < MBW_CT; ++c) {
        const int ct = (hc0 >> 4) + c;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
#pragma unroll
            for (int p = 0; p < 3; ++p) bw[c][ks][p] = Wp16[p * wplane + ((size_t)ks * nct + ct) * 64 + lane];
        bb[c] = b1[ct * 16 + lr];
        bg[c] = W2s[ct * 64 + lane];
    }
    // dW1acc: C layout of x^T dh (column = hidden column lr, row = input channel 4*lq + t of tile m)
    // dW2acc[c][o], db1acc[c]: this lane's hidden column lr of tile c, summed over the rows the lane holds (its lq)
    f32x4 dW1acc[MBW_CT][MT];
    float dW2acc[MBW_CT][3], db1acc[MBW_CT], db2acc[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < MBW_CT; ++c) {
        db1acc[c] = 0.f;
#pragma unroll
        for (int o = 0; o < 3; ++o) dW2acc[c][o] = 0.f;
#pragma unroll
        for (int m = 0; m < MT; ++m) dW1acc[c][m] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    // staging share of this lane: row 8 wave + (lane >> 3) of the tile, channels 4 (lane & 7) .. + 3; its dy row if lane < 8
    const int srow = wave * 8 + (lane >> 3), sch = (lane & 7) * 4, drow = wave * 8 + (lane & 7);
    f32x4 sx;
    float sd[3];
    auto request = [&](int tile) {             // (clamped rows: always valid loads; rows past n are zeroed by bit masks)
        const int row = tile * MB_T + srow, rd = tile * MB_T + drow;
        sx = keep_if(*reinterpret_cast<const f32x4*>(x + (size_t)min(row, n - 1) * CIN + sch), row < n);
#pragma unroll
        for (int o = 0; o < 3; ++o) sd[o] = keep_if(dy[(size_t)min(rd, n - 1) * cout + min(o, cout - 1)], rd < n && o < cout);
    };
    auto park = [&](int buf) {
        char* t = smem_raw + buf * TILE;
        u32x2 pl[3];
        split3(sx, pl[0], pl[1], pl[2]);
#pragma unroll
        for (int p = 0; p < 3; ++p) *reinterpret_cast<u32x2*>(t + srow * XTS + p * XPL + sch * 2) = pl[p];
        unsigned w9[9];
        split_k3_row(sd, w9);
        {   // (no `lane < 8`: the eight lanes that share a dy row store the same bytes - a branch here, with every accumulator
            //  live across it, made the register allocator spill 129 of them)
            *reinterpret_cast<f32x4*>(t + MB_T * XTS + drow * 16) = f32x4{sd[0], sd[1], sd[2], 0.f};
            u32x4* fr = reinterpret_cast<u32x4*>(t + MB_T * XTS + MB_T * 16 + drow * 48);
            fr[0] = u32x4{w9[0], w9[1], w9[2], w9[3]};
            fr[1] = u32x4{w9[4], w9[5], w9[6], w9[7]};
            fr[2] = u32x4{w9[8], 0u, 0u, 0u};
        }
    };
    const int my_tiles = walker < ntiles ? (ntiles - walker + nwalkers - 1) / nwalkers : 0;
    if (my_tiles > 0) {
        request(walker);
        park(0);
    }
    __syncthreads();
#pragma unroll 1
    for (int it = 0; it < my_tiles; ++it) {
        const int tile = walker + it * nwalkers;
        const char* t = smem_raw + (it & 1) * TILE;
        const float* dyw = reinterpret_cast<const float*>(t + MB_T * XTS);
        request(min(tile + nwalkers, ntiles - 1));      // (the tile behind the last: a valid load, parked and never read)
        __builtin_amdgcn_sched_barrier(0);
        // gA[r] = the A operand of g = dy W2^T (this lane's row r*16 + lr; lane groups 0-2 carry slots, group 3 zeros)
        u32x4 gA[MB_RT];
#pragma unroll
        for (int r = 0; r < MB_RT; ++r) {
            const u32x4 f = *reinterpret_cast<const u32x4*>(t + MB_T * XTS + MB_T * 16 + (r * 16 + lr) * 48 + min(lq, 2) * 16);
            const unsigned keep = lq < 3 ? ~0u : 0u;
            gA[r] = u32x4{f[0] & keep, f[1] & keep, f[2] & keep, f[3] & keep};
        }
        u32x4 ax[MB_RT][KS][3];       // x fragments: row r*16 + lr, channels ks*32 + 8*lq .. + 7, plane by plane (once per tile)
#pragma unroll
        for (int r = 0; r < MB_RT; ++r)
#pragma unroll
            for (int ks = 0; ks < KS; ++ks)
#pragma unroll
                for (int p = 0; p < 3; ++p)
                    ax[r][ks][p] = *reinterpret_cast<const u32x4*>(t + (r * 16 + lr) * XTS + p * XPL + (ks * 32 + 8 * lq) * 2);
        u32x4 af[MT][3];              // x^T fragments of the channel tiles (transposed reads, once per tile)
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int p = 0; p < 3; ++p) af[m][p] = mbs_xT_frag(t + p * XPL, XTS, m * 16, lq, lr);
        if (blockIdx.y == 0 && wave == 0 && lr == 0) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const f32x4 d = *reinterpret_cast<const f32x4*>(dyw + ((j >> 2) * 16 + 4 * lq + (j & 3)) * 4);
#pragma unroll
                for (int o = 0; o < 3; ++o) db2acc[o] += d[o];
            }
        }
#pragma unroll
        for (int c = 0; c < MBW_CT; ++c) {
            __builtin_amdgcn_sched_barrier(0);    // one column tile at a time
            asm volatile("" ::: "memory");        // (and its LDS operands re-read: kept from the previous column tile - the
                                                  //  addresses are the same - they would be 60 registers held across the loop)
            f32x4 h[MB_RT], g[MB_RT];
#pragma unroll
            for (int r = 0; r < MB_RT; ++r) h[r] = f32x4{bb[c], bb[c], bb[c], bb[c]};   // (the bias rides in the accumulator)
#pragma unroll
            for (int ks = 0; ks < KS; ++ks)
#pragma unroll
                for (int r = 0; r < MB_RT; ++r) h[r] = mfma_split(ax[r][ks], bw[c][ks], h[r]);
#pragma unroll
            for (int r = 0; r < MB_RT; ++r)
                g[r] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, gA[r]), __builtin_bit_cast(bf16x8, bg[c]),
                                                              f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);    // (phases kept apart: hoisted together their operands do not fit 256 registers)
#pragma unroll
            for (int r = 0; r < MB_RT; ++r)
#pragma unroll
                for (int t4 = 0; t4 < 4; ++t4) {
                    // (the row's dy: re-read per column tile, four addresses per wave - cheaper than 24 registers held)
                    const f32x4 dyv = *reinterpret_cast<const f32x4*>(dyw + (r * 16 + 4 * lq + t4) * 4);
                    const float pre = h[r][t4];
                    const float slope = lrelu01_slope(pre, alpha);
                    const float ha = pre * slope;            // lrelu(pre) = pre * lrelu'(pre)
                    g[r][t4] *= slope;
                    db1acc[c] += g[r][t4];
#pragma unroll
                    for (int o = 0; o < 3; ++o) dW2acc[c][o] = fmaf(ha, dyv[o], dW2acc[c][o]);
                }
            // k = r*16 + 4*lq + t: element j of the B fragment of dW1 += x^T dh is (r = j >> 2, t = j & 3)
            u32x4 bf[3];
            split3_frag(g[0], g[1], bf);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                dW1acc[c][m] = mfma_split(af[m], bf, dW1acc[c][m]);
                // (volatile statements keep their order: this column tile's last product comes before the next one's first
                //  LDS read; left free, the compiler runs two column tiles' phases side by side and spills the accumulators)
                asm volatile("" : "+v"(dW1acc[c][m])::"memory");
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        park((it + 1) & 1);                   // (that buffer was last read in iteration it - 1, before its barrier)
        __syncthreads();
    }
    // parameter-gradient slabs of this wave (slab index = the workgroup's walker id)
    if (blockIdx.y == 0 && wave == 0) {   // db2[o]: lanes (lr = 0, lq) hold the sums of their rows
#pragma unroll
        for (int o = 0; o < 3; ++o) {
            float v = db2acc[o];
            v += __shfl_xor(v, 16);
            v += __shfl_xor(v, 32);
            if (lane == 0) db2_slab[walker * 4 + o] = o < cout ? v : 0.f;
        }
        if (lane == 0) db2_slab[walker * 4 + 3] = 0.f;
    }
#pragma unroll
    for (int c = 0; c < MBW_CT; ++c) {
        const int col = hc0 + c * 16 + lr;
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int t4 = 0; t4 < 4; ++t4)
                dW1_slab[((size_t)walker * CIN + m * 16 + lq * 4 + t4) * hidden + col] = dW1acc[c][m][t4];
        float v = db1acc[c];
        v += __shfl_xor(v, 16);
        v += __shfl_xor(v, 32);
        if (lq == 0) db1_slab[(size_t)walker * hidden + col] = v;
        float w3[3];
#pragma unroll
        for (int o = 0; o < 3; ++o) {
            float u = dW2acc[c][o];
            u += __shfl_xor(u, 16);
            u += __shfl_xor(u, 32);
            w3[o] = o < cout ? u : 0.f;
        }
        if (lq == 0) *reinterpret_cast<f32x4*>(dW2_slab + ((size_t)walker * hidden + col) * 4) = f32x4{w3[0], w3[1], w3[2], 0.f};
    }
}

}  // namespace fgc

namespace fgc {

template <int KS, int CO>
static int fwd_split(const MlpShape& s, const MlpFwdPlan& p, const MlpFwdArgs& a, hipStream_t st) {
    return launch_kernel<mlp_fwd_split_kernel<KS, CO>>(LaunchCfg{"mlp_fwd_kernel", "fgc_mlp_fwd (split operands)", st, p.gx, MB_THREADS, 0},
                                                       (const float*)a.x, s.n, s.hidden, s.cout, (const u32x4*)(a.ws + p.w1.off), a.b1,
                                                       a.W2, a.b2, a.alpha, a.y, a.abs_partial);
}
int launch_mlp_fwd_split(const MlpShape& s, const MlpFwdPlan& p, const MlpFwdArgs& a, hipStream_t st) {
    switch (p.ks) {
        case 1: return p.co == 3 ? fwd_split<1, 3>(s, p, a, st) : fwd_split<1, 4>(s, p, a, st);
        default: return p.co == 3 ? fwd_split<2, 3>(s, p, a, st) : fwd_split<2, 4>(s, p, a, st);
    }
}

int launch_mlp_bwd_split(const MlpShape& s, const MlpBwdPlan& p, const MlpBwdArgs& a, hipStream_t st) {
    constexpr int MT = 2;                      // cin == 32 (the plan takes this form for no other width)
    const float* x = (const float*)a.x;
    const u32x4 *Wp16 = (const u32x4*)(a.ws + p.wp), *W1d = (const u32x4*)(a.ws + p.w1d), *W2s = (const u32x4*)(a.ws + p.w2p);
    int rc = launch_kernel<mlp_bwd_dx_split_kernel<MT>>(
        LaunchCfg{"mlp_bwd_kernel<dx>", "fgc_mlp_bwd (split operands)", st, p.dx_gx, MBB_THREADS, 0}, x, a.dy, s.n, s.hidden, s.cout,
        Wp16, W1d, a.b1, W2s, a.alpha, (float*)a.dx);
    if (rc) return rc;
    return launch_kernel<mlp_bwd_w_split_kernel<MT>>(
        LaunchCfg{"mlp_bwd_kernel<w>", "fgc_mlp_bwd (split operands)", st, p.gx, MBB_THREADS, p.smem, p.gy}, x, a.dy, s.n, s.hidden,
        s.cout, Wp16, a.b1, W2s, a.alpha, (float*)(a.ws + p.dW1), (float*)(a.ws + p.db1), (float*)(a.ws + p.dW2),
        (float*)(a.ws + p.db2));
}

}  // namespace fgc
