// The per-pair arithmetic of the ray casts (include/fgc.h: fgc_ray_cast, fgc_ray_cast_tree): ONE definition, shared by the
// brute-force kernels (fgc_raycast.hip) and the tree kernels (fgc_raytree.hip), so that a pair tested by either gives the
// same bits.  Contraction is off, every FMA is written out.
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

}  // namespace fgc
