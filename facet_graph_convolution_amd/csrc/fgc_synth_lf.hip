// Low-frequency noise synthesis (build extension; include/fgc.h: fgc_synth_noise_lf): on top of the per-vertex white draw
// of fgc_synth_noise every vertex is pushed along its clean normal by a smooth field, a sum of K Gaussian bumps centred on
// randomly chosen clean vertices.  Two launches:
//   lf_table_kernel   one thread per bump: Philox draw, centre gathered, {x, y, z, a_k} (16 bytes) into the scratch
//   lf_field_kernel   one vertex per lane (the vertex sets of fgc_synth_noise's workgroups: the same bounding-box
//                     partials), the bump table wave-uniform: chunks of LF_CHUNK bumps come through scalar loads and
//                     reach the VALU from SGPRs (the idiom of fgc_nn_query, fgc_metrics.hip).  Per pair: 3 v_sub, v_mul + 2 v_fma (the
//                     squared distance), v_mul (by -log2 e / 2 w^2), v_exp_f32, v_fma: 8 VALU instructions (the
//                     issue-rate floor; 11 slots if the transcendental costs four - DESIGN.md 8d.3).
// K is split into slices over blockIdx.y where the vertex blocks alone do not fill the device.  A slice's workgroup writes
// its partial sums to the scratch; the workgroup that arrives LAST at the vertex block's counter (an integer atomic, set
// to zero by the table launch) adds the slices in slice order, so the fp32 sum has one order per (nv, K): no
// floating-point atomics, the same bits eager or replayed.
//
// Contraction is off as in fgc_synth.hip (the white displacement keeps that file's roundings); the fused operations of
// the field are explicit fmaf.
#include "fgc_common.h"
#include "fgc_synth.h"
#pragma clang fp contract(off)      // (and -ffp-contract=off for the file: Makefile)

namespace fgc {

constexpr int LF_CHUNK = 16;            // bumps per scalar-load chunk: 64 dwords of SGPRs
constexpr int LF_TARGET_WGS = 2048;     // workgroups that fill the device: 256 CUs x 8 of 256 threads
constexpr int LF_MIN_SLICE = 256;       // bumps a slice has at least (the last-arriver sum costs one load per slice)

// The scratch, in floats: [box partials 6 G, padded to 16 bytes | table 4 K | slice sums slices x nv | counters G],
// G = synth_blocks(nv).  The slicing depends on (nv, K) alone.
struct LfLayout {
    int slices, per_slice;
    size_t table, part, counters, total;
};

static LfLayout lf_layout(int nv, int n_bumps) {
    LfLayout l;
    const int nblk = synth_blocks(nv);
    int slices = std::min(cdiv(LF_TARGET_WGS, nblk), std::max(1, n_bumps / LF_MIN_SLICE));
    l.per_slice = cdiv(cdiv(n_bumps, slices), LF_CHUNK) * LF_CHUNK;
    l.slices = cdiv(n_bumps, l.per_slice);
    l.table = align_up(6 * (size_t)nblk, 4);
    l.part = l.table + 4 * (size_t)n_bumps;
    l.counters = l.part + (l.slices > 1 ? (size_t)l.slices * (size_t)nv : 0);
    l.total = l.counters + (size_t)nblk;
    return l;
}

__global__ __launch_bounds__(SY_THREADS) void lf_table_kernel(const float* __restrict__ v, int nv,
                                                              const uint32_t* __restrict__ ctl,
                                                              const uint32_t* __restrict__ lf_ctl, int n_bumps,
                                                              NoiseKey key, f32x4* __restrict__ table,
                                                              int* __restrict__ counters, int n_counters) {
    const NoiseCtl c0 = load_noise_ctl(ctl);
    const uint32_t word = lf_ctl[0];
    if (!c0.on || word == 0) return;      // (uniform over the launch)
    const int k = blockIdx.x * SY_THREADS + threadIdx.x;
    if (k < n_counters) counters[k] = 0;
    if (k >= n_bumps) return;
    const float A = __uint_as_float(word & 0x7FFFFFFFu);
    uint32_t c[4] = {(uint32_t)k, c0.step_lo, c0.step_hi, key.stream_id | 0x80000000u};
    philox4x32_10(c, key.seed_lo, key.seed_hi);
    const size_t o = 3 * (size_t)mulhi32(c[0], (uint32_t)nv);      // (< nv: in bounds)
    float z, unused;
    box_muller(c[2], c[3], &z, &unused);
    table[k] = f32x4{v[o], v[o + 1], v[o + 2], A * z};
}

__device__ __forceinline__ float lf_pair(float s, float px, float py, float pz, float bx, float by, float bz, float a,
                                         float scale) {
    const float dx = px - bx, dy = py - by, dz = pz - bz;
    const float d2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
    return fmaf(a, __builtin_amdgcn_exp2f(d2 * scale), s);      // (argument <= 0; far bumps flush to 0)
}

// grid (synth_blocks(nv), slices).  part [slices, nv]: the slices' partial sums (slices > 1 only).
__global__ __launch_bounds__(SY_THREADS) void lf_field_kernel(const float* __restrict__ v, const float* __restrict__ vn,
                                                              const float* __restrict__ wn, int nv,
                                                              const uint32_t* __restrict__ ctl,
                                                              const uint32_t* __restrict__ lf_ctl, int n_bumps,
                                                              int per_slice, NoiseKey key,
                                                              const float* __restrict__ table, float* part, int* counters,
                                                              float* __restrict__ v_out, float* __restrict__ partials) {
    __shared__ float red[SY_THREADS / 64][6];
    __shared__ int arrived;
    const NoiseCtl c = load_noise_ctl(ctl);
    if (!c.on) return;
    const bool lf_on = lf_ctl[0] != 0;
    const int slices = lf_on ? (int)gridDim.y : 1;
    if ((int)blockIdx.y >= slices) return;      // bumps off: the launch is fgc_synth_noise's
    const float w = __uint_as_float(lf_ctl[1]);
    const float scale = -1.44269504088896341f / (2.0f * w * w);
    const int stride = gridDim.x * SY_THREADS;
    const int j0 = blockIdx.y * per_slice, j1 = lf_on ? min(n_bumps, j0 + per_slice) : j0;
    Box3 box;

    // the epilogue of vertex i with the field value s: white step, bump displacement, v_out, box
    auto finish = [&](int i, float s) {
        float q[3];
        synth_white_vertex(v, wn, i, c, key, q);
        if (lf_on)      // (off: the white vertex bit for bit, a -0.0 included)
#pragma unroll
            for (int t = 0; t < 3; ++t) q[t] = q[t] + vn[3 * (size_t)i + t] * s;
        store_vertex(v_out, i, q, box);
    };

    // (the loop is uniform and the lanes past nv predicated: the table addresses stay provably wave-uniform)
    for (int base = blockIdx.x * SY_THREADS; base < nv; base += stride) {
        const int i = base + (int)threadIdx.x;
        const bool in = i < nv;
        const size_t o = 3 * (size_t)(in ? i : 0);
        const float px = v[o], py = v[o + 1], pz = v[o + 2];
        float s = 0.f;
        int j = j0;
        for (; j + LF_CHUNK <= j1; j += LF_CHUNK) {
            const float* tb = table + 4 * (size_t)j;      // wave-uniform: s_load_dwordx16 x 4
            float c[4 * LF_CHUNK];
#pragma unroll
            for (int t = 0; t < 4 * LF_CHUNK; ++t) c[t] = tb[t];
#pragma unroll
            for (int t = 0; t < LF_CHUNK; ++t) s = lf_pair(s, px, py, pz, c[4 * t], c[4 * t + 1], c[4 * t + 2], c[4 * t + 3], scale);
        }
        for (; j < j1; ++j) {
            const float* tb = table + 4 * (size_t)j;
            s = lf_pair(s, px, py, pz, tb[0], tb[1], tb[2], tb[3], scale);
        }
        if (!in) continue;
        if (slices == 1)
            finish(i, s);
        else
            part[(size_t)blockIdx.y * nv + i] = s;
    }

    if (slices > 1) {
        // the last of the vertex block's slices to arrive adds them up
        __threadfence();
        __syncthreads();
        if (threadIdx.x == 0) arrived = atomicAdd(counters + blockIdx.x, 1);
        __syncthreads();
        if (arrived != slices - 1) return;
        __threadfence();
        for (int i = blockIdx.x * SY_THREADS + threadIdx.x; i < nv; i += stride) {
            float s = part[i];
            for (int y = 1; y < slices; ++y) s = s + part[(size_t)y * nv + i];
            finish(i, s);
        }
    }
    store_block_box(box, red, partials);
}

}  // namespace fgc

using namespace fgc;

extern "C" size_t fgc_synth_lf_scratch_floats(int32_t nv, int32_t n_bumps) {
    if (nv <= 0 || n_bumps <= 0 || n_bumps > FGC_SYNTH_LF_MAX_BUMPS) return 0;
    return lf_layout(nv, n_bumps).total;
}

extern "C" int fgc_synth_noise_lf(const float* v, const float* vnormals, const float* white_normals, int32_t nv,
                                  const uint32_t* ctl, const uint32_t* lf_ctl, int32_t n_bumps, uint64_t seed,
                                  uint32_t stream_id, float* v_out, float* scratch, size_t scratch_floats, void* stream) {
    if (int rc = check_noise_args("fgc_synth_noise_lf", v && vnormals && ctl && lf_ctl && v_out && scratch,
                                  " (the bumps need the vertex normals)", nv, v, v_out, scratch_floats,
                                  fgc_synth_lf_scratch_floats(nv, n_bumps)))      // (0 for a count the next line refuses)
        return rc;
    FGC_CHECK_ARG(n_bumps >= 1 && n_bumps <= FGC_SYNTH_LF_MAX_BUMPS, "fgc_synth_noise_lf: n_bumps=%d (1 ... %d)", n_bumps,
                  FGC_SYNTH_LF_MAX_BUMPS);
    FGC_CHECK_ARG(stream_id < 0x80000000u, "fgc_synth_noise_lf: stream_id=%u (below 2^31: the top bit marks the bump counters)",
                  stream_id);
    FGC_CHECK_ARG(((uintptr_t)scratch & 15) == 0, "fgc_synth_noise_lf: scratch must be 16-byte aligned");
    const LfLayout lay = lf_layout(nv, n_bumps);
    hipStream_t st = (hipStream_t)stream;
    const NoiseKey key = noise_key(seed, stream_id);
    const int nblk = synth_blocks(nv);
    float* table = scratch + lay.table;
    int* counters = reinterpret_cast<int*>(scratch + lay.counters);
    FGC_LAUNCH("lf_table_kernel", st, lf_table_kernel, dim3(cdiv(std::max(n_bumps, nblk), SY_THREADS)), dim3(SY_THREADS), 0, v,
               nv, ctl, lf_ctl, n_bumps, key, reinterpret_cast<f32x4*>(table), counters, nblk);
    FGC_LAUNCH("lf_field_kernel", st, lf_field_kernel, dim3(nblk, lay.slices), dim3(SY_THREADS), 0, v, vnormals,
               white_normals, nv, ctl, lf_ctl, n_bumps, lay.per_slice, key, (const float*)table,
               scratch + lay.part, counters, v_out, scratch);
    FGC_CHECK_LAUNCH("fgc_synth_noise_lf");
    return FGC_OK;
}
