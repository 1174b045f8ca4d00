// Noise synthesis for training from clean meshes (build extension; include/fgc.h: fgc_synth_noise,
// fgc_face_features_rows): per step, every vertex of a clean mesh is displaced by a counter-based Gaussian draw and the
// six input channels of every node row are rebuilt from the displaced vertices, bit for bit as the host routine
// fgc_face_features computes them.  Plain bandwidth work: one thread per vertex, one thread per node row.
// fgc_point_sets_prepare: the displaced vertices and the ground-truth vertices divided by the bounding-box diagonal of
// their union and rotated, for the point-set loss - one thread per 3-vector.
//
// The features must carry the host routine's roundings: no fused multiply-add anywhere in this file but the explicit
// fmaf of rot3 (fgc_pack.h), which are the rotation's definition.
#include <algorithm>
#include <cmath>

#include "fgc_common.h"
#include "fgc_pack.h"
#include "fgc_synth.h"
#pragma clang fp contract(off)      // (and -ffp-contract=off for the file: Makefile)

namespace fgc {

// What the depth-sensor instantiation of synth_noise_kernel takes on top.  ctl (device): {FGC_SYNTH_ON | power, float bits of
// r_ref, float bits of q, 0}; words that are off or out of range (sensor_words_valid) give plain noise along the rays, the
// bits of the white instantiation.  The camera comes by value: it is fixed per bound mesh, and a captured launch keeps it.
struct SensorArgs {
    const uint32_t* ctl;
    float cam[3];
};

// One thread per vertex (grid-stride above SY_MAX_BLOCKS workgroups): v_out = v + direction * length, and the workgroup's
// bounding box of v_out into partials[6 * blockIdx.x ..].  White (fgc_synth_noise): length sigma z3 along dir, or - dir ==
// nullptr - along a random direction.  SENSOR (fgc_synth_noise_sensor; fgc_synth.h: synth_displace_sensor): the model's
// length along the viewing rays dir; the same vertex sets per workgroup, so the same partials.
template <bool SENSOR>
__global__ __launch_bounds__(SY_THREADS) void synth_noise_kernel(const float* __restrict__ v, const float* __restrict__ dir,
                                                                 int nv, const uint32_t* __restrict__ ctl, SensorArgs sensor,
                                                                 NoiseKey key, float* __restrict__ v_out,
                                                                 float* __restrict__ partials) {
    __shared__ float red[SY_THREADS / 64][6];
    const NoiseCtl c = load_noise_ctl(ctl);
    if (!c.on) return;
    uint32_t power = 0;
    float r_ref = 1.0f, qs = 0.0f;
    if (SENSOR) {
        const uint32_t w0 = sensor.ctl[0];
        const float r = __uint_as_float(sensor.ctl[1]), q = __uint_as_float(sensor.ctl[2]);
        if (sensor_words_valid(w0, r, q)) {
            power = w0 & 0x7FFFFFFFu;
            r_ref = r;
            qs = q;
        }
    }
    Box3 box;
    for (int i = blockIdx.x * SY_THREADS + threadIdx.x; i < nv; i += gridDim.x * SY_THREADS) {
        float q[3];
        if (SENSOR) {
            const size_t o = 3 * (size_t)i;
            const float p[3] = {v[o], v[o + 1], v[o + 2]};
            const float d[3] = {dir[o], dir[o + 1], dir[o + 2]};
            synth_displace_sensor((uint32_t)i, c.step_lo, c.step_hi, key.stream_id, key.seed_lo, key.seed_hi, c.sigma, power,
                                  r_ref, qs, sensor.cam, p, d, q);
        } else {
            synth_white_vertex(v, dir, i, c, key, q);
        }
        store_vertex(v_out, i, q, box);
    }
    store_block_box(box, red, partials);
}

// The raw generator, for the known-answer test: out[4 i ..] = Philox4x32-10 of counter (first + i, step, stream_id).
__global__ __launch_bounds__(SY_THREADS) void philox_words_kernel(uint32_t first, int n, uint32_t step_lo, uint32_t step_hi,
                                                                  NoiseKey key, uint32_t* __restrict__ out) {
    const int i = blockIdx.x * SY_THREADS + threadIdx.x;
    if (i >= n) return;
    uint32_t c[4] = {first + (uint32_t)i, step_lo, step_hi, key.stream_id};
    philox4x32_10(c, key.seed_lo, key.seed_hi);
    *reinterpret_cast<u32x4*>(out + 4 * (size_t)i) = u32x4{c[0], c[1], c[2], c[3]};
}

// The same partials of vertices as they are (fgc_face_features_rows on vertices no fgc_synth_noise has produced).
__global__ __launch_bounds__(SY_THREADS) void synth_bbox_kernel(const float* __restrict__ v, int nv,
                                                                const uint32_t* __restrict__ ctl,
                                                                float* __restrict__ partials) {
    __shared__ float red[SY_THREADS / 64][6];
    if (ctl && ctl[2] == 0) return;
    Box3 box;
    for (int i = blockIdx.x * SY_THREADS + threadIdx.x; i < nv; i += gridDim.x * SY_THREADS) {
        const float* q = v + 3 * (size_t)i;
        box.add(q, q);
    }
    store_block_box(box, red, partials);
}

// One thread per node row: x[i] = [unit normal | barycentre / bounding-box diagonal] of face faces_rows[i] on the
// vertices v, in fgc_face_features's arithmetic (fgc_prep.hip).  Every workgroup first reduces the n_partials
// bounding-box partials (at most SY_MAX_BLOCKS x 24 bytes, from the L2) to the diagonal: no launch of its own for that.
// A row with a negative or out-of-range vertex id is a fake node: six zeros, nothing dereferenced.
__global__ __launch_bounds__(SY_THREADS) void face_features_rows_kernel(const float* __restrict__ v, int nv,
                                                                        const int32_t* __restrict__ faces, int n,
                                                                        const uint32_t* __restrict__ ctl,
                                                                        const float* __restrict__ partials, int n_partials,
                                                                        float* __restrict__ x) {
    __shared__ float red[SY_THREADS / 64][6];
    if (ctl && ctl[2] == 0) return;
    const float diag = box_diagonal(partials, n_partials, nullptr, red);
    const int i = blockIdx.x * SY_THREADS + threadIdx.x;
    if (i >= n) return;
    const int a = faces[3 * (size_t)i], b = faces[3 * (size_t)i + 1], c = faces[3 * (size_t)i + 2];
    float row[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (a >= 0 && b >= 0 && c >= 0 && a < nv && b < nv && c < nv) {
        const float* p0 = v + 3 * (size_t)a;
        const float* p1 = v + 3 * (size_t)b;
        const float* p2 = v + 3 * (size_t)c;
        float q0[3], q1[3], q2[3], e1[3], e2[3];
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            q0[t] = p0[t];
            q1[t] = p1[t];
            q2[t] = p2[t];
            e1[t] = q1[t] - q0[t];
            e2[t] = q2[t] - q0[t];
        }
        // np.cross on float32: every multiply and subtract rounded on its own (contraction is off for this file)
        float nr[3];
        nr[0] = e1[1] * e2[2] - e1[2] * e2[1];
        nr[1] = e1[2] * e2[0] - e1[0] * e2[2];
        nr[2] = e1[0] * e2[1] - e1[1] * e2[0];
#pragma unroll
        for (int it = 0; it < 2; ++it) {      // utils.normalize = normalizeOnce twice, eps 1e-8 added to the norm
            const float ss = (nr[0] * nr[0] + nr[1] * nr[1]) + nr[2] * nr[2];
            const float inv = 1.0f / (sqrtf(ss) + 0.00000001f);
#pragma unroll
            for (int t = 0; t < 3; ++t) nr[t] = nr[t] * inv;
        }
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            row[t] = nr[t];
            row[3 + t] = ((q0[t] / diag + q1[t] / diag) + q2[t] / diag) / 3.0f;
        }
    }
    f32x2c* dst = reinterpret_cast<f32x2c*>(x + 6 * (size_t)i);      // (24-byte rows: 8-byte aligned)
    dst[0] = f32x2c{row[0], row[1]};
    dst[1] = f32x2c{row[2], row[3]};
    dst[2] = f32x2c{row[4], row[5]};
}

// One thread per 3-vector of the two point sets (the nv vectors of v, then the ngt of gt; no stride: a workgroup's 256
// vectors): out = R (p / diag), diag the bounding-box diagonal of the UNION of the two sets - utils.normalizePointSets
// followed by rotate_rows_kernel, bit for bit.  Every workgroup first reduces the n_partials boxes of v (the noise
// launch's, or synth_bbox_kernel's: at most SY_MAX_BLOCKS x 24 bytes, from the L2) together with the box of gt (gt_box:
// six floats, made once per mesh) to the diagonal, as face_features_rows_kernel does: no launch of its own for that.
// The coordinates are DIVIDED (numpy divides; a multiply by the reciprocal differs in the last bit).  R == nullptr: no
// rotation.
__global__ __launch_bounds__(SY_THREADS) void point_sets_prepare_kernel(const float* __restrict__ v, int nv,
                                                                        const float* __restrict__ gt, int ngt,
                                                                        const float* __restrict__ gt_box,
                                                                        const float* __restrict__ partials, int n_partials,
                                                                        const float* __restrict__ Rd,
                                                                        float* __restrict__ v_out, float* __restrict__ gt_out) {
    __shared__ float red[SY_THREADS / 64][6];
    const float diag = box_diagonal(partials, n_partials, gt_box, red);
    const int64_t i = (int64_t)blockIdx.x * SY_THREADS + threadIdx.x;
    if (i >= (int64_t)nv + ngt) return;
    const bool first = i < nv;
    const size_t o = 3 * (size_t)(first ? i : i - nv);
    const float* __restrict__ src = first ? v : gt;
    float* __restrict__ dst = first ? v_out : gt_out;
    const float a = src[o] / diag, b = src[o + 1] / diag, c = src[o + 2] / diag;
    if (Rd) {
        float r[9];
#pragma unroll
        for (int t = 0; t < 9; ++t) r[t] = Rd[t];
        rot3(r, a, b, c, dst[o], dst[o + 1], dst[o + 2]);
    } else {
        dst[o] = a;
        dst[o + 1] = b;
        dst[o + 2] = c;
    }
}

}  // namespace fgc

using namespace fgc;

extern "C" size_t fgc_synth_scratch_floats(int32_t nv) {
    if (nv <= 0) return 0;
    return 6 * (size_t)synth_blocks(nv);
}

extern "C" int fgc_synth_noise(const float* v, const float* vnormals, int32_t nv, const uint32_t* ctl, uint64_t seed,
                               uint32_t stream_id, float* v_out, float* scratch, size_t scratch_floats, void* stream) {
    if (int rc = check_noise_args("fgc_synth_noise", v && ctl && v_out && scratch, "", nv, v, v_out, scratch_floats,
                                  fgc_synth_scratch_floats(nv)))
        return rc;
    hipStream_t st = (hipStream_t)stream;
    FGC_LAUNCH("synth_noise_kernel", st, synth_noise_kernel<false>, dim3(synth_blocks(nv)), dim3(SY_THREADS), 0, v, vnormals,
               nv, ctl, SensorArgs{}, noise_key(seed, stream_id), v_out, scratch);
    FGC_CHECK_LAUNCH("fgc_synth_noise");
    return FGC_OK;
}

extern "C" int fgc_synth_noise_sensor(const float* v, const float* dirs, int32_t nv, const uint32_t* ctl,
                                      const uint32_t* sensor_ctl, const float* camera, uint64_t seed, uint32_t stream_id,
                                      float* v_out, float* scratch, size_t scratch_floats, void* stream) {
    if (int rc = check_noise_args("fgc_synth_noise_sensor", v && dirs && ctl && sensor_ctl && camera && v_out && scratch,
                                  " (the model needs the table of rays and the camera)", nv, v, v_out, scratch_floats,
                                  fgc_synth_scratch_floats(nv)))
        return rc;
    FGC_CHECK_ARG(std::isfinite(camera[0]) && std::isfinite(camera[1]) && std::isfinite(camera[2]),
                  "fgc_synth_noise_sensor: the camera must be three finite numbers");
    hipStream_t st = (hipStream_t)stream;
    FGC_LAUNCH("synth_noise_sensor_kernel", st, synth_noise_kernel<true>, dim3(synth_blocks(nv)), dim3(SY_THREADS), 0, v, dirs,
               nv, ctl, SensorArgs{sensor_ctl, {camera[0], camera[1], camera[2]}}, noise_key(seed, stream_id), v_out, scratch);
    FGC_CHECK_LAUNCH("fgc_synth_noise_sensor");
    return FGC_OK;
}

extern "C" int fgc_philox_words(uint32_t first, int32_t n, uint64_t step, uint64_t seed, uint32_t stream_id, uint32_t* out,
                                void* stream) {
    FGC_CHECK_ARG(out && n > 0, "fgc_philox_words: out=%p, n=%d", (void*)out, n);
    FGC_CHECK_ARG(((uintptr_t)out & 15) == 0, "fgc_philox_words: out must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    FGC_LAUNCH("philox_words_kernel", st, philox_words_kernel, dim3(cdiv(n, SY_THREADS)), dim3(SY_THREADS), 0, first, n,
               (uint32_t)(step & 0xFFFFFFFFu), (uint32_t)(step >> 32), noise_key(seed, stream_id), out);
    FGC_CHECK_LAUNCH("fgc_philox_words");
    return FGC_OK;
}

extern "C" int fgc_face_features_rows(const float* v, int32_t nv, const int32_t* faces_rows, int32_t n, const uint32_t* ctl,
                                      int32_t have_bbox, float* x, float* scratch, size_t scratch_floats, void* stream) {
    FGC_CHECK_ARG(v && faces_rows && x && scratch, "fgc_face_features_rows: null pointer");
    FGC_CHECK_ARG(nv > 0 && n > 0, "fgc_face_features_rows: nv=%d, n=%d (> 0)", nv, n);
    FGC_CHECK_ARG(((uintptr_t)x & 7) == 0, "fgc_face_features_rows: x must be 8-byte aligned");
    const size_t need = fgc_synth_scratch_floats(nv);
    FGC_CHECK_ARG(scratch_floats >= need, "fgc_face_features_rows: scratch too small (%zu < %zu floats)", scratch_floats,
                  need);
    hipStream_t st = (hipStream_t)stream;
    const int nblk = synth_blocks(nv);
    if (!have_bbox)
        FGC_LAUNCH("synth_bbox_kernel", st, synth_bbox_kernel, dim3(nblk), dim3(SY_THREADS), 0, v, nv, ctl, scratch);
    FGC_LAUNCH("face_features_rows_kernel", st, face_features_rows_kernel, dim3(cdiv(n, SY_THREADS)), dim3(SY_THREADS), 0,
               v, nv, faces_rows, n, ctl, (const float*)scratch, nblk, x);
    FGC_CHECK_LAUNCH("fgc_face_features_rows");
    return FGC_OK;
}

extern "C" int fgc_point_sets_prepare(const float* v, int32_t nv, const float* gt, int32_t ngt, const float* gt_box,
                                      const float* R, int32_t have_bbox, float* v_out, float* gt_out, float* scratch,
                                      size_t scratch_floats, void* stream) {
    FGC_CHECK_ARG(v && gt && gt_box && v_out && gt_out && scratch, "fgc_point_sets_prepare: null pointer");
    FGC_CHECK_ARG(nv > 0 && ngt > 0, "fgc_point_sets_prepare: nv=%d, ngt=%d (> 0)", nv, ngt);
    FGC_CHECK_ARG(v_out != v && gt_out != gt && v_out != gt_out, "fgc_point_sets_prepare: the outputs must be buffers of their own");
    const size_t need = fgc_synth_scratch_floats(nv);
    FGC_CHECK_ARG(scratch_floats >= need, "fgc_point_sets_prepare: scratch too small (%zu < %zu floats)", scratch_floats,
                  need);
    hipStream_t st = (hipStream_t)stream;
    const int nblk = synth_blocks(nv);
    if (!have_bbox)
        FGC_LAUNCH("synth_bbox_kernel", st, synth_bbox_kernel, dim3(nblk), dim3(SY_THREADS), 0, v, nv,
                   (const uint32_t*)nullptr, scratch);
    const int64_t total = (int64_t)nv + ngt;
    FGC_LAUNCH("point_sets_prepare_kernel", st, point_sets_prepare_kernel, dim3((unsigned)((total + SY_THREADS - 1) / SY_THREADS)),
               dim3(SY_THREADS), 0, v, nv, gt, ngt, gt_box, (const float*)scratch, nblk, R, v_out, gt_out);
    FGC_CHECK_LAUNCH("fgc_point_sets_prepare");
    return FGC_OK;
}
