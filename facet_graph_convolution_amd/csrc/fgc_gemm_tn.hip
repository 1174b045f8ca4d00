// The weight-gradient GEMMs of the graph convolution (K3 of fgc_conv_bwd.hip; also the narrow first layer's, fgc_conv_narrow.hip):
// the four kernels, their grouped forms, and the host code that chooses between them.
#include <algorithm>

#include "fgc_gemm_tn.h"

namespace fgc {


// ---------------------------------------------------------------------------------------------
// K3: C[P,Q] = sum_rows A[row,P] * X[row >> shift, Q]   (X = [x0 | x1]); f32 MFMA with K = rows.
// Both operands are row-major with the reduction index as the slow dimension, so a lane's 16-byte load of
// A[row, p0+4*lr .. +3] holds the SAME k (row) for 4 different output rows: MFMA number e takes element e,
// i.e. MFMA e owns output rows p0 + 4*i + e (i = MFMA row index).  One dwordx4 of A and one of X per lane feed
// 16 MFMAs (a 64 x 64 tile per wave, 4 rows of K per step); no LDS staging, no barrier in the loop.
// grid (P tiles * Q tiles, row splits); the 4 waves of a workgroup interleave the k-steps of their split and are
// summed through LDS in a fixed order; partials go to slab[split][P][Q], reduced by reduce_jobs.
// ---------------------------------------------------------------------------------------------
template <bool VEC4>
__device__ __forceinline__ void tn_load(const float* __restrict__ A, int lda, int P, const float* __restrict__ x0,
                                        const float* __restrict__ x1, int c0, int c1, int shift, int row, bool valid,
                                        int pbase, int qbase, f32x4& a, f32x4& b) {
    a = f32x4{0.f, 0.f, 0.f, 0.f};
    b = f32x4{0.f, 0.f, 0.f, 0.f};
    if (!valid) return;
    const int Q = c0 + c1;
    const size_t sr = (size_t)(row >> shift);
    if (VEC4) {
        if (pbase < P) a = *reinterpret_cast<const f32x4*>(A + (size_t)row * lda + pbase);
        if (qbase < c0) b = *reinterpret_cast<const f32x4*>(x0 + sr * c0 + qbase);
        else if (qbase < Q) b = *reinterpret_cast<const f32x4*>(x1 + sr * c1 + (qbase - c0));
    } else {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            if (pbase + t < P) a[t] = A[(size_t)row * lda + pbase + t];
            const int q = qbase + t;
            if (q < c0) b[t] = x0[sr * c0 + q];
            else if (q < Q) b[t] = x1[sr * c1 + (q - c0)];
        }
    }
}

// Workgroup -> (output tile, node-range split) of the weight-gradient GEMMs.  Workgroups are dealt round-robin over the
// 8 XCDs, each with a private L2.  With the plain (tile, split) grid the tiles of one split - which read the SAME rows of r
// and x - land on different XCDs and every L2 fetches those rows from HBM again (dconv2: x came in ten times).  Here all
// tiles of a split run on one XCD, next to each other in dispatch order: the rows are fetched once and the other tiles
// hit in L2.  The grid is padded to 8 * ceil(splits / 8) splits; workgroups of a padding split return at once.
// Same work per (tile, split), same slabs, same sums: results are unchanged bit for bit.
__device__ __forceinline__ bool tn_block(int ntiles, int nsplits, int& tile, int& split, int vblock = -1) {
    // (vblock: the workgroup's index within ITS job of a grouped launch; jobs start at multiples of 8, so vblock & 7 is
    //  still the XCD the hardware dealt this workgroup to)
    const int L = vblock >= 0 ? vblock : (int)blockIdx.x, xcd = L & 7, idx = L >> 3;
    tile = idx % ntiles;
    split = (idx / ntiles) * 8 + xcd;
    return split < nsplits;
}

__device__ __forceinline__ int tn_job_of(const TnJobs& J) {
    int q = 0;
#pragma unroll
    for (int t = 1; t < TN_MAX_JOBS; ++t)
        if (t < J.njobs && (int)blockIdx.x >= J.job[t].block0) q = t;
    return q;
}

template <bool VEC4>
__global__ __launch_bounds__(256) void gemm_tn_kernel(const float* __restrict__ A, int lda, int P,
                                                      const float* __restrict__ x0, const float* __restrict__ x1,
                                                      int c0, int c1, int shift, int rows, int rows_per_split,
                                                      float* __restrict__ slab) {
    __shared__ float red[4][64][65];
    const int Q = c0 + c1;
    const int npt = (P + 63) >> 6;
    int tile_id, split_id;
    if (!tn_block(npt * ((Q + 63) >> 6), (rows + rows_per_split - 1) / rows_per_split, tile_id, split_id)) return;
    const int pt = tile_id % npt, qt = tile_id / npt;
    const int p0 = pt * 64, q0 = qt * 64;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lr = lane & 15, lq = lane >> 4;
    const int r_begin = split_id * rows_per_split;
    const int r_end = min(rows, r_begin + rows_per_split);
    const int nsteps = (r_end - r_begin + 3) >> 2;
    const int pbase = p0 + 4 * lr, qbase = q0 + 4 * lr;
    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    // two operand register sets with fixed roles (unrolled by 2, no copies of in-flight loads)
    f32x4 a0, b0, a1, b1;
    auto ld = [&](int step, f32x4& a, f32x4& b) {
        const int row = r_begin + 4 * step + lq;
        tn_load<VEC4>(A, lda, P, x0, x1, c0, c1, shift, row, step < nsteps && row < r_end, pbase, qbase, a, b);
    };
    auto mm = [&](const f32x4& a, const f32x4& b) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[j], acc[i][j], 0, 0, 0);
    };
    ld(wave, a0, b0);
    ld(wave + 4, a1, b1);
    for (int s = wave; s < nsteps; s += 8) {
        mm(a0, b0);
        ld(s + 8, a0, b0);
        if (s + 4 < nsteps) mm(a1, b1);
        ld(s + 12, a1, b1);
    }
    // C layout of acc[i][j]: column index lr -> q = 4*lr + j ; row index lq*4+reg -> p = 4*(lq*4+reg) + i
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int t = 0; t < 4; ++t) red[wave][4 * (lq * 4 + t) + i][4 * lr + j] = acc[i][j][t];
    __syncthreads();
    float* out = slab + (size_t)split_id * P * Q;
    for (int t = tid; t < 64 * 64; t += 256) {
        const int pp = t >> 6, qq = t & 63;
        if (p0 + pp < P && q0 + qq < Q)
            out[(size_t)(p0 + pp) * Q + q0 + qq] = (red[0][pp][qq] + red[1][pp][qq]) + (red[2][pp][qq] + red[3][pp][qq]);
    }
}

// Streaming form of gemm_tn_kernel for 16-byte aligned operands whose widths are multiples of 4 (every layer but
// conv1).  Same tiling, same summation order, bit-identical results; what differs is how memory is asked for:
//   * loads are UNCONDITIONAL (row and column indices clamped into the operands, out-of-range rows zeroed by a
//     select on the A fragment): no exec-masked branch around a load, so hipcc counts its s_waitcnt instead of
//     draining everything with vmcnt(0) in front of every MFMA group;
//   * four operand register sets with fixed roles (loop unrolled by 4): each load has three MFMA groups = 48
//     matrix instructions to land;
//   * the 4-wave sum goes through 2 x 16 KB of LDS instead of 4, so four workgroups are resident per CU.
// NJ = 4: 64 x 64 output tile (lane lr owns columns 4*lr .. 4*lr+3); NJ = 2: 64 x 32 for operands only 32 wide (columns
// 2*lr, 2*lr+1: half the MFMAs instead of multiplying clamped duplicates)
// BF: both operands are bf16 tensors (FGC_CONV_BF16); they are widened on load and multiplied on the fp32 MFMA: the
// products are exact and the sum over the nodes stays an fp32 chain, as in the fp32 network
template <int NJ, bool BF>
__device__ __forceinline__ void tn_stream_body(const float* __restrict__ A, int lda, int P, const float* __restrict__ x0,
                                               const float* __restrict__ x1, int c0, int c1, int shift, int rows,
                                               int rows_per_split, float* __restrict__ slab, int vblock,
                                               float (*red)[64][65]) {
    const int Q = c0 + c1;
    const int npt = (P + 63) >> 6;
    int tile_id, split_id;
    if (!tn_block(npt * ((Q + 16 * NJ - 1) / (16 * NJ)), (rows + rows_per_split - 1) / rows_per_split, tile_id, split_id, vblock))
        return;
    const int pt = tile_id % npt, qt = tile_id / npt;
    const int p0 = pt * 64, q0 = qt * (16 * NJ);
    const int tid = threadIdx.x, lane = tid & 63, lr = lane & 15, lq = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r_begin = split_id * rows_per_split;
    const int r_end = min(rows, r_begin + rows_per_split);
    const int nsteps = (r_end - r_begin + 3) >> 2;
    // column quads of this lane, clamped into the operands (results of clamped columns are never stored)
    const int pc = min(p0 + 4 * lr, P - 4);
    const int qc = min(q0 + NJ * lr, Q - NJ);
    const float* bsrc = BF ? reinterpret_cast<const float*>(reinterpret_cast<const unsigned short*>(qc < c0 ? x0 : x1) +
                                                            (qc < c0 ? qc : qc - c0))
                           : (qc < c0 ? x0 + qc : x1 + (qc - c0));
    const int bld = qc < c0 ? c0 : c1;
    f32x4 acc[4][NJ];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    // A load only requests memory; the zeroing of out-of-range rows happens where the fragment is consumed (a select
    // right behind the load would make the compiler wait for it on the spot)
    auto ld = [&](int step, f32x4& a, f32x4& b, int& row) {
        row = r_begin + 4 * step + lq;
        const int rc = min(row, r_end - 1);
        if constexpr (BF) {
            const unsigned short* A16 = reinterpret_cast<const unsigned short*>(A);
            const unsigned short* b16 = reinterpret_cast<const unsigned short*>(bsrc);
            a = bf4_to_f4(*reinterpret_cast<const u32x2*>(A16 + (size_t)rc * lda + pc));
            if constexpr (NJ == 4) {
                b = bf4_to_f4(*reinterpret_cast<const u32x2*>(b16 + (size_t)(rc >> shift) * bld));
            } else {
                const f32x2c b2 = bf2_to_f2(*reinterpret_cast<const unsigned*>(b16 + (size_t)(rc >> shift) * bld));
                b = f32x4{b2[0], b2[1], 0.f, 0.f};
            }
            return;
        }
        a = *reinterpret_cast<const f32x4*>(A + (size_t)rc * lda + pc);
        if constexpr (NJ == 4) {
            b = *reinterpret_cast<const f32x4*>(bsrc + (size_t)(rc >> shift) * bld);
        } else {
            const f32x2c b2 = *reinterpret_cast<const f32x2c*>(bsrc + (size_t)(rc >> shift) * bld);
            b = f32x4{b2[0], b2[1], 0.f, 0.f};
        }
    };
    auto mm = [&](f32x4 a, const f32x4& b, int row) {
        if (row >= r_end) a = f32x4{0.f, 0.f, 0.f, 0.f};   // a select, not a branch
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < NJ; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[j], acc[i][j], 0, 0, 0);
    };
    f32x4 a0, b0, a1, b1, a2, b2, a3, b3;
    int r0, r1, r2, r3;
    ld(wave, a0, b0, r0);
    ld(wave + 4, a1, b1, r1);
    ld(wave + 8, a2, b2, r2);
    ld(wave + 12, a3, b3, r3);
    // sched_barrier: keep the program order "16 MFMAs, then the refill of the set they consumed" (left alone the
    // scheduler sinks every refill to just in front of its use and the prefetch distance collapses to zero)
#define FGC_TN_STEP(A_, B_, R_, NEXT_)          \
    mm(A_, B_, R_);                             \
    __builtin_amdgcn_sched_barrier(0);          \
    ld(NEXT_, A_, B_, R_);                      \
    __builtin_amdgcn_sched_barrier(0);
    for (int s = wave; s < nsteps; s += 16) {   // steps past the end load a clamped row and multiply by zero
        FGC_TN_STEP(a0, b0, r0, s + 16)
        FGC_TN_STEP(a1, b1, r1, s + 20)
        FGC_TN_STEP(a2, b2, r2, s + 24)
        FGC_TN_STEP(a3, b3, r3, s + 28)
    }
#undef FGC_TN_STEP
    // (w0 + w1) + (w2 + w3), as gemm_tn_kernel sums them.  C layout of acc[i][j]: column lr -> q = 4*lr + j,
    // row lq*4+reg -> p = 4*(lq*4+reg) + i
    auto put = [&](int slot) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < NJ; ++j)
#pragma unroll
                for (int t = 0; t < 4; ++t) red[slot][4 * (lq * 4 + t) + i][NJ * lr + j] = acc[i][j][t];
    };
    auto add = [&](int slot) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < NJ; ++j)
#pragma unroll
                for (int t = 0; t < 4; ++t) acc[i][j][t] += red[slot][4 * (lq * 4 + t) + i][NJ * lr + j];
    };
    if (wave == 1) put(0);
    if (wave == 3) put(1);
    __syncthreads();
    if (wave == 0) add(0);
    if (wave == 2) add(1);
    __syncthreads();
    if (wave == 0) put(0);
    if (wave == 2) put(1);
    __syncthreads();
    float* out = slab + (size_t)split_id * P * Q;
    for (int t = tid; t < 64 * 16 * NJ; t += 256) {
        const int pp = t / (16 * NJ), qq = t % (16 * NJ);
        if (p0 + pp < P && q0 + qq < Q) out[(size_t)(p0 + pp) * Q + q0 + qq] = red[0][pp][qq] + red[1][pp][qq];
    }
}

// Direct form of the fp32 streaming body: the same tiles, k-step order, operand sets and sums, with the address and tail work
// taken off the vector ALU (v_mfma_f32_16x16x4_f32 and VALU instructions do not co-issue: every vector instruction in the loop
// costs a SIMD 4 cycles next to the 32 of an MFMA).
//   * A goes through a buffer descriptor that starts at the split's first row and ends at its last: a row past r_end comes
//     back as zeros from the range check, so the clamp of the row and the select on the fragment are gone.  The lane's byte
//     offset is computed once and advances by the constant 16 rows per load (all four operand sets share one running
//     offset: consecutive loads of a wave are always four k-steps apart).
//   * X goes through one descriptor per HALF tile of 32 columns (lane lr owns columns 2*lr, 2*lr + 1 of each half: b[2h],
//     b[2h + 1]), from the split's first row to the operand's end.  A half lies in one source whenever c0 % 32 == 0 (or there
//     is one source), so the descriptor is wave-uniform even in a tile that the concat boundary cuts; rows past r_end read
//     the rows that follow (finite, times the zero of A) or zeros past the operand's end (0 * 0): + 0 either way, as the
//     clamped row gives in tn_stream_body.  Which column a lane holds does not enter an element's sum: same bits.
//   * the sum over the four waves goes through LDS in the accumulators' own layout (element (i, j) of lane l at
//     ((i * NJ + j) * 64 + l) as an f32x4: ds_write_b128 / ds_read_b128 at constant offsets), (w0 + w1) + (w2 + w3) as
//     before, and wave 0 stores the tile from registers, two columns per store.
// Offsets are 32 bits relative to the split's first row; tn_direct_ok is the (wave-uniform) test that they fit, that a
// k-step's 16 rows advance X by whole rows and that no half tile straddles the sources.  Where it fails the workgroup runs
// tn_stream_body.
__device__ __forceinline__ bool tn_direct_ok(int lda, int c0, int c1, int shift, int rows_per_split) {
    // (a wave requests at most 4 * 28 + 3 rows past the end of its split)
    return (c1 == 0 || (c0 & 31) == 0) && shift <= 4 &&
           (long long)(rows_per_split + 160) * max(lda, max(c0, c1)) < (1ll << 29);   // (and P * Q: a weight matrix)
}

template <int NJ>
__device__ __forceinline__ void tn_direct_body(const float* __restrict__ A, int lda, int P, const float* __restrict__ x0,
                                               const float* __restrict__ x1, int c0, int c1, int shift, int rows,
                                               int rows_per_split, float* __restrict__ slab, int vblock, f32x4* red) {
    constexpr int NH = NJ / 2;   // half tiles of 32 columns
    const int Q = c0 + c1;
    const int npt = (P + 63) >> 6;
    int tile_id, split_id;
    if (!tn_block(npt * ((Q + 16 * NJ - 1) / (16 * NJ)), (rows + rows_per_split - 1) / rows_per_split, tile_id, split_id, vblock))
        return;
    const int pt = tile_id % npt, qt = tile_id / npt;
    const int p0 = pt * 64, q0 = qt * (16 * NJ);
    const int tid = threadIdx.x, lane = tid & 63, lr = lane & 15, lq = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r_begin = split_id * rows_per_split;
    const int r_end = min(rows, r_begin + rows_per_split);
    const int nsteps = (r_end - r_begin + 3) >> 2;
    const int row0 = 4 * wave + lq;   // this lane's row of the wave's first k-step, from r_begin
    // column quad / pairs of this lane, clamped into the operands (results of clamped columns are never stored)
    const int pc = min(p0 + 4 * lr, P - 4);
    const __amdgpu_buffer_rsrc_t a_rs = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(A + (size_t)r_begin * lda), 0, (r_end - r_begin) * lda * 4, 0x00020000);
    unsigned ao = (unsigned)(row0 * lda + pc) * 4u;
    const unsigned astep = 16u * (unsigned)lda * 4u;
    const int xr0 = r_begin >> shift, xrows = ((rows - 1) >> shift) + 1;   // X: first row of the split, rows of the operand
    const int xrow0 = ((r_begin + row0) >> shift) - xr0;
    __amdgpu_buffer_rsrc_t b_rs[NH];
    unsigned bo[NH], bstep[NH];
#pragma unroll
    for (int h = 0; h < NH; ++h) {
        const int hs = q0 + 32 * h;
        const bool first = hs < c0 || c1 == 0;
        const int ld = first ? c0 : c1;
        const size_t bytes = (size_t)(xrows - xr0) * ld * 4;
        b_rs[h] = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>((first ? x0 : x1) + (size_t)xr0 * ld), 0,
                                                    (int)(unsigned)std::min<size_t>(bytes, 0xffffffffu), 0x00020000);
        bo[h] = (unsigned)(xrow0 * ld + min(hs + 2 * lr, Q - 2) - (first ? 0 : c0)) * 4u;
        bstep[h] = (unsigned)((16 >> shift) * ld) * 4u;
    }
    f32x4 acc[4][NJ];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    struct Set {
        f32x4 a;
        f32x2c b[NH];
    };
    // (the empty asm pins the running offset in its register: left alone, loop strength reduction turns each into four
    //  induction variables plus a base and the loop pays 21 vector instructions for what takes 12)
    auto ld = [&](Set& s) {   // the wave's next k-step
        s.a = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(a_rs, ao, 0, 0));
        ao += astep;
        asm volatile("" : "+v"(ao));
#pragma unroll
        for (int h = 0; h < NH; ++h) {
            s.b[h] = __builtin_bit_cast(f32x2c, __builtin_amdgcn_raw_buffer_load_b64(b_rs[h], bo[h], 0, 0));
            bo[h] += bstep[h];
            asm volatile("" : "+v"(bo[h]));
        }
    };
    auto mm = [&](const Set& s) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < NJ; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(s.a[i], s.b[j >> 1][j & 1], acc[i][j], 0, 0, 0);
    };
    // sched_barrier: keep the program order "16 MFMAs, then the refill of the set they consumed" (see tn_stream_body), and
    // the first four requests in the order of the refills: s_waitcnt counts from the older of the two histories that meet
    // at the loop's head
    if (wave < nsteps) {   // (a split shorter than four k-steps leaves waves without one)
        Set s0, s1, s2, s3;
        ld(s0);
        __builtin_amdgcn_sched_barrier(0);
        ld(s1);
        __builtin_amdgcn_sched_barrier(0);
        ld(s2);
        __builtin_amdgcn_sched_barrier(0);
        ld(s3);
        __builtin_amdgcn_sched_barrier(0);
#define FGC_TN_STEP(S_)                         \
    mm(S_);                                     \
    __builtin_amdgcn_sched_barrier(0);          \
    ld(S_);                                     \
    __builtin_amdgcn_sched_barrier(0);
        int s = wave;
        do {   // steps past the end multiply zeros
            FGC_TN_STEP(s0)
            FGC_TN_STEP(s1)
            FGC_TN_STEP(s2)
            FGC_TN_STEP(s3)
            s += 16;
        } while (s < nsteps);
    }
#undef FGC_TN_STEP
    // (w0 + w1) + (w2 + w3), as gemm_tn_kernel sums them; a lane only ever meets its own slots
    auto put = [&](int slot) {
#pragma unroll
        for (int e = 0; e < 4 * NJ; ++e) red[(slot * 4 * NJ + e) * 64 + lane] = acc[e / NJ][e % NJ];
    };
    auto add = [&](int slot) {
#pragma unroll
        for (int e = 0; e < 4 * NJ; ++e) acc[e / NJ][e % NJ] += red[(slot * 4 * NJ + e) * 64 + lane];
    };
    if (wave == 1) put(0);
    if (wave == 3) put(1);
    __syncthreads();
    if (wave == 0) add(0);
    if (wave == 2) {
        add(1);
        put(1);
    }
    __syncthreads();
    if (wave != 0) return;
    add(1);
    // C layout of acc[i][j]: column lr of half j >> 1 -> q = 32 * (j >> 1) + 2 * lr + (j & 1), row lq*4+reg -> p = 4*(lq*4+reg) + i.
    // The slab tile goes out through a descriptor of exactly this split's [P, Q]: rows >= P fall to its range check, lanes
    // whose columns are >= Q (whole pairs: Q is even) get an offset that no addition brings back into range.
    const __amdgpu_buffer_rsrc_t c_rs =
        __builtin_amdgcn_make_buffer_rsrc(slab + (size_t)split_id * P * Q, 0, P * Q * 4, 0x00020000);
#pragma unroll
    for (int h = 0; h < NH; ++h) {
        const int q = q0 + 32 * h + 2 * lr;
        const unsigned co = q < Q ? (unsigned)((p0 + 16 * lq) * Q + q) * 4u : 0x80000000u;
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int i = 0; i < 4; ++i)
                __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, f32x2c{acc[i][2 * h][t], acc[i][2 * h + 1][t]}), c_rs,
                                                      co + (unsigned)((4 * t + i) * Q) * 4u, 0, 0);
    }
}

// (the LDS of the 4-wave sum: 2 x 16 KB; tn_stream_body pads its rows, hence the 65)
template <int NJ, bool BF>
__device__ __forceinline__ void tn_stream_any(const float* __restrict__ A, int lda, int P, const float* __restrict__ x0,
                                              const float* __restrict__ x1, int c0, int c1, int shift, int rows,
                                              int rows_per_split, float* __restrict__ slab, int vblock) {
    __shared__ __attribute__((aligned(16))) float red[2][64][65];
    if constexpr (!BF) {
        if (tn_direct_ok(lda, c0, c1, shift, rows_per_split)) {
            tn_direct_body<NJ>(A, lda, P, x0, x1, c0, c1, shift, rows, rows_per_split, slab, vblock,
                               reinterpret_cast<f32x4*>(&red[0][0][0]));
            return;
        }
    }
    tn_stream_body<NJ, BF>(A, lda, P, x0, x1, c0, c1, shift, rows, rows_per_split, slab, vblock, red);
}
template <int NJ, bool BF = false>
__global__ __launch_bounds__(256, 4) void gemm_tn_stream_kernel(const float* __restrict__ A, int lda, int P,
                                                                const float* __restrict__ x0,
                                                                const float* __restrict__ x1, int c0, int c1, int shift,
                                                                int rows, int rows_per_split, float* __restrict__ slab) {
    tn_stream_any<NJ, BF>(A, lda, P, x0, x1, c0, c1, shift, rows, rows_per_split, slab, -1);
}
template <int NJ, bool BF = false>
__global__ __launch_bounds__(256, 4) void gemm_tn_stream_group_kernel(TnJobs J) {
    const TnArgs& a = J.job[tn_job_of(J)];
    tn_stream_any<NJ, BF>((const float*)a.A, a.lda, a.P, (const float*)a.x0, (const float*)a.x1, a.c0, a.c1, a.shift, a.rows,
                          a.rps, a.slab, (int)blockIdx.x - a.block0);
}

// ---------------------------------------------------------------------------------------------
// K3 for bf16-stored operands ON the bf16 matrix cores (FGC_CONV_BF16).  C[P,Q] = sum_rows A[row,P] * X[row >> shift, Q]
// reduces over the rows, the slow index of both operands, while a v_mfma_f32_16x16x32_bf16 fragment wants 8 consecutive k
// of ONE output row / column in a lane.  The transposition is done by the LDS read: a chunk of 32 rows of A (up to 320
// columns) and of X (QT * 16 columns) is staged row-major, as it lies in memory (16-byte pieces, coalesced), and read back
// with ds_read_b64_tr_b16: per 16-lane group a 4 row x 16 column block comes back column-major, lane i holding column i
// of the four rows.  Two such reads (rows 4*lq .. +3 and 16 + 4*lq .. +3) are a whole fragment; A and X use the same row
// order, so the permuted k is consistent.  Row strides == 32 bytes mod 256, an odd multiple of 32: the eight rows a
// 32-lane half touches land on eight disjoint 32-byte bank spans.  Wave w owns row tiles 5w .. 5w+4 of the product
// (columns of A) and all column tiles: 18 transposed reads per 20 MFMAs.  The kernel streams: what bounds it is how fast
// the rows of r arrive, so the next chunk travels through registers under the current one.  fp32 accumulators; slabs and
// their fixed-order sum as for the fp32 kernels.
// ---------------------------------------------------------------------------------------------
constexpr int TNB_THREADS = 256;
constexpr int TNB_AS = TNB_PC * 2 + 32;   // LDS row strides in bytes
typedef short s16x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ u32x4 tnb_frag(const char* tile, int stride, int col0, int lq, int lr) {
    // block rows 4*lq + q (then 16 + 4*lq + q), columns col0 + 4*p .. +3 for lane 4*q + p of the group
    const char* a = tile + (4 * lq + (lr >> 2)) * stride + (col0 + 4 * (lr & 3)) * 2;
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)a);
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(a + 16 * stride));
    const u32x2 l2 = __builtin_bit_cast(u32x2, lo), h2 = __builtin_bit_cast(u32x2, hi);
    return u32x4{l2[0], l2[1], h2[0], h2[1]};
}

template <int QT>
__device__ __forceinline__ void tn_bf16_body(const unsigned short* __restrict__ A, int lda, int P,
                                             const unsigned short* __restrict__ x0, const unsigned short* __restrict__ x1, int c0,
                                             int c1, int shift, int rows, int rows_per_split, float* __restrict__ slab,
                                             int vblock) {
    constexpr int QC = QT * 16;
    constexpr int XS = QC * 2 + 32;
    constexpr int APC = TNB_PC / 8;                                  // 16-byte pieces per row of the A chunk
    constexpr int NA = 32 * APC / TNB_THREADS;                       // pieces per thread: 5
    static_assert(32 * APC % TNB_THREADS == 0 && 32 * (QC / 8) <= TNB_THREADS, "staging shape");
    __shared__ __attribute__((aligned(16))) char As[2][32 * TNB_AS];
    __shared__ __attribute__((aligned(16))) char Xs[2][32 * XS];
    const int Q = c0 + c1;
    const int npc = (P + TNB_PC - 1) / TNB_PC;
    int tile_id, split_id;
    if (!tn_block(npc * (Q / QC), (rows + rows_per_split - 1) / rows_per_split, tile_id, split_id, vblock)) return;
    const int pc = tile_id % npc, qc = tile_id / npc;
    const int p0 = pc * TNB_PC, q0 = qc * QC;
    const int pw = min(P - p0, TNB_PC);                              // valid columns of A here (a multiple of 8)
    const int tid = threadIdx.x, lane = tid & 63, lr = lane & 15, lq = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r_begin = split_id * rows_per_split;
    const int r_end = min(rows, r_begin + rows_per_split);
    const int nchunks = (r_end - r_begin + 31) >> 5;

    u32x4 ra[NA], rx;
    const int xrow = min(tid, 32 * (QC / 8) - 1) / (QC / 8), xcol = (min(tid, 32 * (QC / 8) - 1) % (QC / 8)) * 8;
    const int qcol = q0 + xcol;
    const bool x_first = qcol < c0;
    const unsigned short* xsrc = x_first ? x0 : x1;
    const int xld = x_first ? c0 : c1;
    const int xoff = min(x_first ? qcol : qcol - c0, xld - 8);
    auto fetch = [&](int ch) {
        const int rb = r_begin + ch * 32;
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            const int t = tid + i * TNB_THREADS;
            const int row = min(rb + t / APC, r_end - 1);
            const int col = p0 + min((t % APC) * 8, pw - 8);
            ra[i] = *reinterpret_cast<const u32x4*>(A + (size_t)row * lda + col);
        }
        rx = *reinterpret_cast<const u32x4*>(xsrc + (size_t)(min(rb + xrow, r_end - 1) >> shift) * xld + xoff);
    };
    auto stage = [&](int ch, int buf) {
        const int rb = r_begin + ch * 32;
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            const int t = tid + i * TNB_THREADS;
            const int r = t / APC, c = (t % APC) * 8;
            const bool ok = rb + r < r_end && c < pw;
            *reinterpret_cast<u32x4*>(&As[buf][r * TNB_AS + c * 2]) = ok ? ra[i] : u32x4{0u, 0u, 0u, 0u};
        }
        if (tid < 32 * (QC / 8)) {
            const bool ok = rb + xrow < r_end && qcol < Q;
            *reinterpret_cast<u32x4*>(&Xs[buf][xrow * XS + xcol * 2]) = ok ? rx : u32x4{0u, 0u, 0u, 0u};
        }
    };
    f32x4 acc[5][QT];
#pragma unroll
    for (int i = 0; i < 5; ++i)
#pragma unroll
        for (int j = 0; j < QT; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    if (nchunks > 0) {
        fetch(0);
        stage(0, 0);
    }
    __syncthreads();
    for (int ch = 0; ch < nchunks; ++ch) {
        const int buf = ch & 1;
        if (ch + 1 < nchunks) fetch(ch + 1);
        u32x4 af[5], bq[QT];
#pragma unroll
        for (int i = 0; i < 5; ++i) af[i] = tnb_frag(As[buf], TNB_AS, (wave * 5 + i) * 16, lq, lr);
#pragma unroll
        for (int j = 0; j < QT; ++j) bq[j] = tnb_frag(Xs[buf], XS, j * 16, lq, lr);
#pragma unroll
        for (int i = 0; i < 5; ++i)
#pragma unroll
            for (int j = 0; j < QT; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, af[i]), __builtin_bit_cast(bf16x8, bq[j]),
                                                                   acc[i][j], 0, 0, 0);
        if (ch + 1 < nchunks) stage(ch + 1, buf ^ 1);     // (the other buffer: its readers finished before the last barrier)
        __syncthreads();
    }
    // C layout: column = lr -> q, row = 4*lq + reg -> p
    float* out = slab + (size_t)split_id * P * Q;
#pragma unroll
    for (int i = 0; i < 5; ++i)
#pragma unroll
        for (int j = 0; j < QT; ++j)
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int pp = p0 + (wave * 5 + i) * 16 + lq * 4 + t, qq = q0 + j * 16 + lr;
                if (pp < p0 + pw && qq < Q) out[(size_t)pp * Q + qq] = acc[i][j][t];
            }
}
template <int QT>
__global__ __launch_bounds__(TNB_THREADS, 2) void gemm_tn_bf16_kernel(const unsigned short* __restrict__ A, int lda, int P,
                                                                      const unsigned short* __restrict__ x0,
                                                                      const unsigned short* __restrict__ x1, int c0, int c1,
                                                                      int shift, int rows, int rows_per_split,
                                                                      float* __restrict__ slab) {
    tn_bf16_body<QT>(A, lda, P, x0, x1, c0, c1, shift, rows, rows_per_split, slab, -1);
}
template <int QT>
__global__ __launch_bounds__(TNB_THREADS, 2) void gemm_tn_bf16_group_kernel(TnJobs J) {
    const TnArgs& a = J.job[tn_job_of(J)];
    tn_bf16_body<QT>((const unsigned short*)a.A, a.lda, a.P, (const unsigned short*)a.x0, (const unsigned short*)a.x1, a.c0, a.c1,
                     a.shift, a.rows, a.rps, a.slab, (int)blockIdx.x - a.block0);
}

bool tn_bf16_ok(int P, int c0, int c1) {
    if (opt(OPT_NO_TNBF16) == 1) return false;
    const int Q = c0 + c1;
    return P % 8 == 0 && c0 % 8 == 0 && c1 % 8 == 0 && Q % 32 == 0 && (c1 == 0 || c0 % 16 == 0) && c0 >= 8 && (c1 == 0 || c1 >= 8);
}

int launch_gemm_tn_stream(const char* tag, const float* A, int lda, int P, const float* x0, int c0, int rows,
                          int rows_per_split, int nsplits, float* slab, hipStream_t st) {
    if (c0 <= 32 && c0 % 2 == 0) {
        const dim3 grid = tn_grid(cdiv(P, 64), nsplits);
        FGC_LAUNCH(tag, st, gemm_tn_stream_kernel<2>, grid, dim3(256), 0, A, lda, P, x0, (const float*)nullptr, c0, 0, 0, rows,
                   rows_per_split, slab);
    } else {
        const dim3 grid = tn_grid(cdiv(P, 64) * cdiv(c0, 64), nsplits);
        FGC_LAUNCH(tag, st, gemm_tn_stream_kernel<4>, grid, dim3(256), 0, A, lda, P, x0, (const float*)nullptr, c0, 0, 0, rows,
                   rows_per_split, slab);
    }
    FGC_CHECK_LAUNCH("gemm_tn_stream_kernel");
    return FGC_OK;
}

int tn_rows_per_slab(int n, int splits) { return cdiv(cdiv(n, splits), 4) * 4; }

// A split count near `desired` (at most `maxs`) whose EFFECTIVE number of slabs is a multiple of 8: tn_block gives every
// XCD the slabs s = xcd, xcd + 8, ...; with 27 slabs two XCDs would work through four of them and six through three.
int tn_balanced_splits(int desired, int maxs, int rows) {
    desired = std::max(1, std::min(desired, maxs));
    for (int delta = 0; delta < 24; ++delta)
        for (int sgn = 1; sgn >= -1; sgn -= 2) {
            const int s = desired + sgn * delta;
            if (s >= 8 && s <= maxs && cdiv(rows, tn_rows_per_slab(rows, s)) % 8 == 0) return s;
        }
    return desired;
}

// An XCD has 32 CUs x 4 resident workgroups of these kernels = 128 slots and is given tiles x (slabs / 8) workgroups: the
// slab count fills a whole number of slots per CU exactly once (a count just above a multiple of 32 leaves a few CUs with one
// workgroup more than the rest, and the launch waits for them).
int tn_splits(int P, int Q, int rows) {
    const int tiles = cdiv(P, 64) * cdiv(Q, 64);
    // Two workgroups per CU (64 slots per XCD), not the four that fit: the kernel is bound by the matrix pipe and by HBM,
    // which eight waves per CU keep as busy as sixteen, and every workgroup less is a 16 KB slab less to write and to sum
    // (measured over 32 ... 256 slots: 64 is the minimum of the step, 2.192 -> 2.179 ms; the GEMMs 1-2 us faster each, the
    // sums 17 -> 12 us per launch).  Layers with more than 32 output tiles (the 128 -> 128 layer of the coarsest level)
    // would get one slab per XCD that way and keep 128 slots (32 -> 39 us otherwise).  FGC_TN_SLOTS: developer knob.
    const int slots = (int)opt(OPT_TN_SLOTS);
    int per = slots / tiles;
    if (per < 2) per = std::max(1, 2 * slots / tiles);
    return tn_balanced_splits(8 * per, cdiv(rows, 128), rows);
}

// rows x [PL columns of A] against [c0 + c1 columns of x0 | x1]
TnPlan tn_plan_of(bool bf16, bool vec4, bool stream_ok, const void* A, int PL, const void* x0, const void* x1, int c0, int c1,
                         int shift, int rows, int rps, float* slab, int lda) {
    TnPlan pl;
    const int cin = c0 + c1, ns = cdiv(rows, rps);
    pl.a = TnArgs{A, x0, x1, slab, lda ? lda : PL, PL, c0, c1, shift, rows, rps, 0};   // (lda: row stride of A, >= its PL columns)
    pl.nsplits = ns;
    if (bf16 && tn_bf16_ok(PL, c0, c1)) {
        pl.variant = cin % 64 == 0 ? TN_BF16_4 : TN_BF16_2;
        pl.ntiles = cdiv(PL, TNB_PC) * (cin % 64 == 0 ? cin / 64 : cin / 32);
    } else if (bf16 && cin <= 32 && c1 == 0) {
        pl.variant = TN_STREAM2_BF;
        pl.ntiles = cdiv(PL, 64);
    } else if (bf16) {
        pl.variant = TN_STREAM4_BF;
        pl.ntiles = cdiv(PL, 64) * cdiv(cin, 64);
    } else if (stream_ok && cin <= 32 && c1 == 0 && cin % 2 == 0) {
        pl.variant = TN_STREAM2;
        pl.ntiles = cdiv(PL, 64);
    } else if (stream_ok) {
        pl.variant = TN_STREAM4;
        pl.ntiles = cdiv(PL, 64) * cdiv(cin, 64);
    } else {
        pl.variant = vec4 ? TN_PLAIN_V4 : TN_PLAIN;
        pl.ntiles = cdiv(PL, 64) * cdiv(cin, 64);
    }
    return pl;
}
int tn_launch_one(const TnPlan& pl, const char* tag, hipStream_t st) {
    const TnArgs& a = pl.a;
    const dim3 grid = tn_grid(pl.ntiles, pl.nsplits);
    const float *A = (const float*)a.A, *x0 = (const float*)a.x0, *x1 = (const float*)a.x1;
    const unsigned short *A16 = (const unsigned short*)a.A, *h0 = (const unsigned short*)a.x0, *h1 = (const unsigned short*)a.x1;
    switch (pl.variant) {
        case TN_BF16_4: FGC_LAUNCH(tag, st, (gemm_tn_bf16_kernel<4>), grid, dim3(TNB_THREADS), 0, A16, a.lda, a.P, h0, h1, a.c0, a.c1, a.shift, a.rows, a.rps, a.slab); break;
        case TN_BF16_2: FGC_LAUNCH(tag, st, (gemm_tn_bf16_kernel<2>), grid, dim3(TNB_THREADS), 0, A16, a.lda, a.P, h0, h1, a.c0, a.c1, a.shift, a.rows, a.rps, a.slab); break;
        case TN_STREAM2_BF: FGC_LAUNCH(tag, st, (gemm_tn_stream_kernel<2, true>), grid, dim3(256), 0, A, a.lda, a.P, x0, x1, a.c0, a.c1, a.shift, a.rows, a.rps, a.slab); break;
        case TN_STREAM4_BF: FGC_LAUNCH(tag, st, (gemm_tn_stream_kernel<4, true>), grid, dim3(256), 0, A, a.lda, a.P, x0, x1, a.c0, a.c1, a.shift, a.rows, a.rps, a.slab); break;
        case TN_STREAM2: FGC_LAUNCH(tag, st, gemm_tn_stream_kernel<2>, grid, dim3(256), 0, A, a.lda, a.P, x0, x1, a.c0, a.c1, a.shift, a.rows, a.rps, a.slab); break;
        case TN_STREAM4: FGC_LAUNCH(tag, st, gemm_tn_stream_kernel<4>, grid, dim3(256), 0, A, a.lda, a.P, x0, x1, a.c0, a.c1, a.shift, a.rows, a.rps, a.slab); break;
        case TN_PLAIN_V4: FGC_LAUNCH(tag, st, (gemm_tn_kernel<true>), grid, dim3(256), 0, A, a.lda, a.P, x0, x1, a.c0, a.c1, a.shift, a.rows, a.rps, a.slab); break;
        default: FGC_LAUNCH(tag, st, (gemm_tn_kernel<false>), grid, dim3(256), 0, A, a.lda, a.P, x0, x1, a.c0, a.c1, a.shift, a.rows, a.rps, a.slab); break;
    }
    FGC_CHECK_LAUNCH("fgc_conv_bwd/dW");
    return FGC_OK;
}
// jobs of one variant in one launch (block ranges in job order; every tn_grid is a multiple of 8 workgroups)
int tn_launch_group(int variant, TnJobs& J, int nblocks, const char* tag, hipStream_t st) {
    if (J.njobs == 0) return FGC_OK;
    switch (variant) {
        case TN_BF16_4: FGC_LAUNCH(tag, st, (gemm_tn_bf16_group_kernel<4>), dim3(nblocks), dim3(TNB_THREADS), 0, J); break;
        case TN_BF16_2: FGC_LAUNCH(tag, st, (gemm_tn_bf16_group_kernel<2>), dim3(nblocks), dim3(TNB_THREADS), 0, J); break;
        case TN_STREAM2_BF: FGC_LAUNCH(tag, st, (gemm_tn_stream_group_kernel<2, true>), dim3(nblocks), dim3(256), 0, J); break;
        case TN_STREAM4_BF: FGC_LAUNCH(tag, st, (gemm_tn_stream_group_kernel<4, true>), dim3(nblocks), dim3(256), 0, J); break;
        case TN_STREAM2: FGC_LAUNCH(tag, st, (gemm_tn_stream_group_kernel<2>), dim3(nblocks), dim3(256), 0, J); break;
        default: FGC_LAUNCH(tag, st, (gemm_tn_stream_group_kernel<4>), dim3(nblocks), dim3(256), 0, J); break;
    }
    FGC_CHECK_LAUNCH("fgc_conv_bwd_reduce/dW");
    J.njobs = 0;
    return FGC_OK;
}

}  // namespace fgc
