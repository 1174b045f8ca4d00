// What the ray casts share (include/fgc.h: fgc_ray_cast, fgc_ray_cast_tree): ONE definition each of a face's record, a lane's
// ray and the per-pair arithmetic, for the brute-force kernels (fgc_raycast.hip) and the tree kernels (fgc_raytree.hip), so
// that a pair tested by either gives the same bits.  Contraction is off, every FMA is written out.
#pragma once
#include "fgc_common.h"

#pragma clang fp contract(off)

namespace fgc {

constexpr int RC_CHUNK = 4;            // records per scalar-load chunk: 48 dwords of SGPRs

// a . b = fma(a_z, b_z, fma(a_y, b_y, a_x b_x))
__device__ __forceinline__ float rc_dot(float ax, float ay, float az, float bx, float by, float bz) {
    return __builtin_fmaf(az, bz, __builtin_fmaf(ay, by, ax * bx));
}
// one component of a x b: fma(a1, b2, -(a2 b1))
__device__ __forceinline__ float rc_det2(float a1, float b2, float a2, float b1) { return __builtin_fmaf(a1, b2, -(a2 * b1)); }

// Moeller-Trumbore as include/fgc.h spells it.  Returns whether (u, v, t) is a hit of a ray with t > t_min; u, v, t are
// written only as far as they were needed (all three when the result is true).
__device__ __forceinline__ bool rc_uvt(const float (&o)[3], const float (&d)[3], f32x4 a, f32x4 e1, f32x4 e2, float t_min,
                                       float& u, float& v, float& t) {
    const float px = rc_det2(d[1], e2.z, d[2], e2.y), py = rc_det2(d[2], e2.x, d[0], e2.z), pz = rc_det2(d[0], e2.y, d[1], e2.x);
    const float det = rc_dot(e1.x, e1.y, e1.z, px, py, pz);
    const float sx = o[0] - a.x, sy = o[1] - a.y, sz = o[2] - a.z;
    u = rc_dot(sx, sy, sz, px, py, pz) / det;
    if (!(u >= 0.f && u <= 1.f)) return false;      // (det == 0: u is an infinity or a NaN)
    const float qx = rc_det2(sy, e1.z, sz, e1.y), qy = rc_det2(sz, e1.x, sx, e1.z), qz = rc_det2(sx, e1.y, sy, e1.x);
    v = rc_dot(d[0], d[1], d[2], qx, qy, qz) / det;
    t = rc_dot(e2.x, e2.y, e2.z, qx, qy, qz) / det;
    return v >= 0.f && u + v <= 1.f && t > t_min && t < __builtin_inff();
}

// Face f as a record: (a, 0), (e1 = b - a, 0), (e2 = c - a, 0), and its three vertices in v.  An f outside [0, nf) (the
// padding) or a row with a vertex id outside [0, nv) gives the zero record (det = 0: it can never hit) and false; nothing is
// loaded through an id that was not bounded.  v is written only where true is returned.  A caller that does not read v
// pays nothing: the values are the loads the record needs anyway.
__device__ __forceinline__ bool rc_record(const float* __restrict__ verts, int nv, const int* __restrict__ faces, int nf, int f,
                                          f32x4& r0, f32x4& r1, f32x4& r2, float (&v)[3][3]) {
    r0 = r1 = r2 = f32x4{0.f, 0.f, 0.f, 0.f};
    if ((unsigned)f >= (unsigned)nf) return false;
    const int id[3] = {faces[3 * (size_t)f], faces[3 * (size_t)f + 1], faces[3 * (size_t)f + 2]};
    if (!((unsigned)id[0] < (unsigned)nv && (unsigned)id[1] < (unsigned)nv && (unsigned)id[2] < (unsigned)nv)) return false;
#pragma unroll
    for (int k = 0; k < 3; ++k) v[k][0] = verts[3 * (size_t)id[k]], v[k][1] = verts[3 * (size_t)id[k] + 1], v[k][2] = verts[3 * (size_t)id[k] + 2];
    r0 = f32x4{v[0][0], v[0][1], v[0][2], 0.f};
    r1 = f32x4{v[1][0] - v[0][0], v[1][1] - v[0][1], v[1][2] - v[0][2], 0.f};
    r2 = f32x4{v[2][0] - v[0][0], v[2][1] - v[0][1], v[2][2] - v[0][2], 0.f};
    return true;
}

// Ray q of a cast with one origin row or one per ray.  A dead lane's ray is o = d = 0: det = 0, never a hit.
__device__ __forceinline__ void rc_load_ray(const float* __restrict__ origins, int n_origins, const float* __restrict__ dirs,
                                            int q, bool live, float (&o)[3], float (&d)[3]) {
    o[0] = o[1] = o[2] = d[0] = d[1] = d[2] = 0.f;
    if (!live) return;
    const size_t oo = n_origins == 1 ? 0 : 3 * (size_t)q;
    o[0] = origins[oo], o[1] = origins[oo + 1], o[2] = origins[oo + 2];
    d[0] = dirs[3 * (size_t)q], d[1] = dirs[3 * (size_t)q + 1], d[2] = dirs[3 * (size_t)q + 2];
}

}  // namespace fgc
