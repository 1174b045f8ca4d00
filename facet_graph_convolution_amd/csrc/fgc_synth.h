// Per-vertex noise draw of fgc_synth_noise (include/fgc.h): Philox4x32-10, Box-Muller, displacement.  Device code; the
// published known answers of the generator are checked ON the device through fgc_philox_words (tests/test_gpu_synth.py).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "fgc_common.h"

#define FGC_HD __device__ __forceinline__

namespace fgc {

FGC_HD uint32_t mulhi32(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a * (uint64_t)b) >> 32); }

// Philox4x32-10 (Salmon et al., SC'11): ten rounds, the key bumped between rounds.  c: counter in, random words out.
FGC_HD void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = mulhi32(0xD2511F53u, c[0]), lo0 = 0xD2511F53u * c[0];
        const uint32_t hi1 = mulhi32(0xCD9E8D57u, c[2]), lo1 = 0xCD9E8D57u * c[2];
        const uint32_t n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
        c[0] = n0;
        c[1] = lo1;
        c[2] = n2;
        c[3] = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
}

// Two standard normals of two random words.  u = (n + 0.5) 2^-24 with n = x >> 8 lies strictly between 0 and 1 but needs 25
// bits: it is exact in fp32 only for n < 2^23.  In the upper half 1 - u = ((2^24 - 1 - n) + 0.5) 2^-24 is exact instead, so
// ln u is taken as log1p(-(1 - u)) and the angle 2 pi u as -2 pi (1 - u): a u next to 1 (where a rounded u would lose all of
// r = sqrt(-2 ln u)) keeps fp32 relative accuracy.  The angle is never formed: sin / cos of pi (2 w) come from sinpif /
// cospif on the exact 2 w, so a cosine next to 0 keeps its RELATIVE accuracy too - with the angle rounded to fp32 (2e-7
// absolute) a draw whose direction (z0, z1, z2) is short turns by 2e-7 r1 / |z|: 1e-5 and more for |z| < 0.05.
FGC_HD float philox_half(uint32_t n, bool upper) { return ((float)(upper ? 0xFFFFFFu - n : n) + 0.5f) * 0x1p-24f; }

FGC_HD void box_muller(uint32_t x0, uint32_t x1, float* z0, float* z1) {
    const uint32_t n0 = x0 >> 8, n1 = x1 >> 8;
    const bool up0 = n0 >= (1u << 23), up1 = n1 >= (1u << 23);
    const float w0 = philox_half(n0, up0);
    const float r = sqrtf(-2.0f * (up0 ? log1pf(-w0) : logf(w0)));
    const float t = 2.0f * philox_half(n1, up1);
    const float s = sinpif(t);
    *z0 = r * cospif(t);
    *z1 = r * (up1 ? -s : s);
}

// The displaced vertex i: along nrm[0..2] (along_normal), otherwise along the random unit vector (z0, z1, z2) / |.|;
// the length is sigma z3.  sigma == 0 returns the vertex itself, bit for bit (also a -0.0 coordinate).
FGC_HD void synth_displace(uint32_t i, uint32_t step_lo, uint32_t step_hi, uint32_t stream_id, uint32_t seed_lo,
                           uint32_t seed_hi, float sigma, const float v[3], bool along_normal, const float nrm[3],
                           float out[3]) {
    uint32_t c[4] = {i, step_lo, step_hi, stream_id};
    philox4x32_10(c, seed_lo, seed_hi);
    float z0, z1, z2, z3;
    box_muller(c[0], c[1], &z0, &z1);
    box_muller(c[2], c[3], &z2, &z3);
    const float inv = 1.0f / sqrtf(z0 * z0 + z1 * z1 + z2 * z2);
    const float d[3] = {along_normal ? nrm[0] : z0 * inv, along_normal ? nrm[1] : z1 * inv, along_normal ? nrm[2] : z2 * inv};
    const float len = sigma * z3;
    for (int t = 0; t < 3; ++t) out[t] = sigma == 0.0f ? v[t] : v[t] + d[t] * len;
}

// The depth-sensor model of fgc_synth_noise_sensor (include/fgc.h has the definition): vertex i displaced along its viewing
// ray d by a Gaussian whose sigma grows with the range r = |v - cam| (power 0, 1, 2 of r / r_ref), then - q > 0 - put on the
// lattice of a sensor that reports r = 1 / (k q).  z3 is synth_displace's: the same counter, key and pair of words.
// power 0 with q == 0 is synth_displace(along_normal) bit for bit; q == 0 with sigma == 0 returns the vertex itself.
// Every operation is one rounded IEEE operation (the file compiles with contraction off; / and sqrtf are the accurate
// ones): the fmaf below are the definition's.
FGC_HD void synth_displace_sensor(uint32_t i, uint32_t step_lo, uint32_t step_hi, uint32_t stream_id, uint32_t seed_lo,
                                  uint32_t seed_hi, float sigma, uint32_t power, float r_ref, float q, const float cam[3],
                                  const float v[3], const float d[3], float out[3]) {
    uint32_t c[4] = {i, step_lo, step_hi, stream_id};
    philox4x32_10(c, seed_lo, seed_hi);
    float z2, z3;
    box_muller(c[2], c[3], &z2, &z3);
    const float w[3] = {v[0] - cam[0], v[1] - cam[1], v[2] - cam[2]};
    const float r = sqrtf(fmaf(w[2], w[2], fmaf(w[1], w[1], w[0] * w[0])));
    const float rho = r / r_ref;
    float s = sigma;
    if (power >= 1) s = sigma * rho;
    if (power == 2) s = s * rho;
    float len = s * z3;
    bool keep = sigma == 0.0f;
    if (q > 0.0f) {
        float rt = r + len;
        if (!(rt > 0.0f)) rt = r;      // the noise carried the sample through the sensor (or r itself is 0)
        const float k = fminf(fmaxf(rintf(1.0f / (rt * q)), 1.0f), 16777216.0f);
        len = 1.0f / (k * q) - r;
        keep = false;
    }
    for (int t = 0; t < 3; ++t) out[t] = keep ? v[t] : v[t] + d[t] * len;
}

// What a sensor_ctl of fgc_synth_noise_sensor must hold to be ON: the on flag, power 0 ... 2, r_ref a positive normal
// float, q zero or a positive normal float.  Anything else is OFF - plain noise along the rays - never a non-finite vertex.
FGC_HD bool sensor_words_valid(uint32_t w0, float r_ref, float q) {
    const bool on = (w0 & 0x80000000u) != 0 && (w0 & 0x7FFFFFFFu) <= 2u;
    const bool ref_ok = r_ref >= 0x1p-126f && r_ref <= 3.402823466e+38f;
    const bool q_ok = q == 0.0f || (q >= 0x1p-126f && q <= 3.402823466e+38f);
    return on && ref_ok && q_ok;
}

// ---- what the noise launches share (fgc_synth.hip, fgc_synth_lf.hip): launch shape, control words, the per-vertex white
// step and the workgroup's bounding box - one copy of each ----
constexpr int SY_THREADS = 256;
constexpr int SY_MAX_BLOCKS = 1024;      // vertex blocks of a launch = bounding-box partials the feature kernel re-reduces

static inline int synth_blocks(int nv) { return std::min(cdiv(nv, SY_THREADS), SY_MAX_BLOCKS); }

// The Philox key of a launch, by value: seed -> (lo, hi) and the stream id.
struct NoiseKey {
    uint32_t seed_lo, seed_hi, stream_id;
};

static inline NoiseKey noise_key(uint64_t seed, uint32_t stream_id) {
    return NoiseKey{(uint32_t)(seed & 0xFFFFFFFFu), (uint32_t)(seed >> 32), stream_id};
}

// What every noise entry point checks, under the entry point's name `who`: no null pointer (`pointers`: all of its own are
// set; null_note: what it adds to that message), nv > 0, an output of its own, a scratch of `need` floats.
static inline int check_noise_args(const char* who, bool pointers, const char* null_note, int nv, const float* v,
                                   const float* v_out, size_t scratch_floats, size_t need) {
    FGC_CHECK_ARG(pointers, "%s: null pointer%s", who, null_note);
    FGC_CHECK_ARG(nv > 0, "%s: nv=%d (> 0)", who, nv);
    FGC_CHECK_ARG(v_out != v, "%s: v_out and v must be distinct (the clean vertices are kept)", who);
    FGC_CHECK_ARG(scratch_floats >= need, "%s: scratch too small (%zu < %zu floats)", who, scratch_floats, need);
    return FGC_OK;
}

// ctl (device) of every noise launch: {step low, step high, sigma word}; sigma word 0 = off (the launch reads and writes
// nothing more), otherwise bit 31 is the on flag and the low 31 bits are the float bits of sigma >= 0.
struct NoiseCtl {
    bool on;      // (uniform over the launch: `if (!c.on) return;` is no divergence)
    float sigma;
    uint32_t step_lo, step_hi;
};

FGC_HD NoiseCtl load_noise_ctl(const uint32_t* __restrict__ ctl) {
    const uint32_t word = ctl[2];
    return NoiseCtl{word != 0, __uint_as_float(word & 0x7FFFFFFFu), ctl[0], ctl[1]};
}

// The white step of vertex i: q = v[i] displaced by synth_displace along dir[i] (dir == nullptr: a random direction).
FGC_HD void synth_white_vertex(const float* __restrict__ v, const float* __restrict__ dir, int i, const NoiseCtl& c,
                               const NoiseKey& key, float q[3]) {
    const size_t o = 3 * (size_t)i;
    const float p[3] = {v[o], v[o + 1], v[o + 2]};
    float nrm[3] = {0.f, 0.f, 0.f};
    if (dir) {
        nrm[0] = dir[o];
        nrm[1] = dir[o + 1];
        nrm[2] = dir[o + 2];
    }
    synth_displace((uint32_t)i, c.step_lo, c.step_hi, key.stream_id, key.seed_lo, key.seed_hi, c.sigma, p, dir != nullptr, nrm,
                   q);
}

// A thread's share of a bounding box: empty, grown point by point, reduced over the workgroup.
struct Box3 {
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};

    FGC_HD void add(const float lo[3], const float hi[3]) {
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            mn[t] = fminf(mn[t], lo[t]);
            mx[t] = fmaxf(mx[t], hi[t]);
        }
    }
};

// v_out[i] = q, folded into the thread's box.
FGC_HD void store_vertex(float* __restrict__ v_out, int i, const float q[3], Box3& box) {
    const size_t o = 3 * (size_t)i;
#pragma unroll
    for (int t = 0; t < 3; ++t) v_out[o + t] = q[t];
    box.add(q, q);
}

// min over mn[0..2] / max over mx[0..2] of the workgroup's threads; the result in every thread.  min / max are exact:
// the order of the reduction is free.
FGC_HD void block_minmax(Box3& box, float (*red)[6]) {
    float* mn = box.mn;
    float* mx = box.mx;
#pragma unroll
    for (int t = 0; t < 3; ++t)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            mn[t] = fminf(mn[t], __shfl_xor(mn[t], off, 64));
            mx[t] = fmaxf(mx[t], __shfl_xor(mx[t], off, 64));
        }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            red[wave][t] = mn[t];
            red[wave][3 + t] = mx[t];
        }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        mn[t] = red[0][t];
        mx[t] = red[0][3 + t];
#pragma unroll
        for (int w = 1; w < SY_THREADS / 64; ++w) {
            mn[t] = fminf(mn[t], red[w][t]);
            mx[t] = fmaxf(mx[t], red[w][3 + t]);
        }
    }
}

// The epilogue of a launch that made vertices: the workgroup's box into partials[6 * blockIdx.x ..] = {min xyz, max xyz}.
FGC_HD void store_block_box(Box3& box, float (*red)[6], float* __restrict__ partials) {
    block_minmax(box, red);
    if (threadIdx.x == 0) {
        float* dst = partials + 6 * (size_t)blockIdx.x;
#pragma unroll
        for (int t = 0; t < 3; ++t) {      // (constant indices: the arrays stay in registers)
            dst[t] = box.mn[t];
            dst[3 + t] = box.mx[t];
        }
    }
}

// The bounding-box diagonal the input rows and the point sets are divided by: every workgroup reduces the n_partials boxes
// of a noise launch (at most SY_MAX_BLOCKS x 24 bytes, from the L2) - with gt_box, six floats, the union with that box - and
// takes the diagonal in double from the fp32 extents, then rounds it to fp32 (what numpy's float32 / python float divides
// by: utils.py:1271-1280, utils.normalizePointSets).  Contraction is off in the files that call it.
FGC_HD float box_diagonal(const float* __restrict__ partials, int n_partials, const float* __restrict__ gt_box,
                          float (*red)[6]) {
    Box3 box;
    for (int j = threadIdx.x; j < n_partials; j += SY_THREADS) box.add(partials + 6 * j, partials + 6 * j + 3);
    if (gt_box && threadIdx.x == 0) box.add(gt_box, gt_box + 3);
    block_minmax(box, red);
    double diag2 = 0.0;
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        const double e = (double)(box.mx[t] - box.mn[t]);
        diag2 += e * e;
    }
    return (float)sqrt(diag2);
}

}  // namespace fgc
