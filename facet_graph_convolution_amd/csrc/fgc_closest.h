// The per-pair arithmetic of the closest-point query (include/fgc.h: fgc_closest_point_tree): ONE definition, run on every
// pair whether the boxes culled around it or not (FGC_CP_EXHAUSTIVE), so that a pair gives the same bits either way.
// Contraction is off, every FMA is written out; the dot product is rc_dot of fgc_raycast.h.
#pragma once
#include "fgc_raycast.h"

#pragma clang fp contract(off)

namespace fgc {

// Closest point of the triangle of record (a, e1, e2) to q, by the region walk of Ericson, Real-Time Collision Detection
// 5.1.5, as include/fgc.h spells it: the first region that applies wins.  Returns dist2 = r . r with
// r = q - a - u e1 - v e2 and writes (u, v); a NaN (a collinear triangle that reaches the last region with 0 x inf, a
// non-finite coordinate) is returned as it is: every comparison with it is false, so it never wins.
// In the last region (u, v) is clamped to u in [0, 1], v in [0, 1 - u] by comparisons that leave a NaN alone: whatever the
// rounding of va, vb, vc did, the point a + u e1 + v e2 lies on the triangle, which is what the culling bound rests on.
// cp_pair_r also hands out r (what the surface loss differentiates); cp_pair is the same arithmetic without it.
__device__ __forceinline__ float cp_pair_r(const float (&q)[3], f32x4 a, f32x4 e1, f32x4 e2, float& u, float& v, float (&r)[3]) {
    const float apx = q[0] - a.x, apy = q[1] - a.y, apz = q[2] - a.z;
    const float d1 = rc_dot(e1.x, e1.y, e1.z, apx, apy, apz), d2 = rc_dot(e2.x, e2.y, e2.z, apx, apy, apz);
    const float bpx = apx - e1.x, bpy = apy - e1.y, bpz = apz - e1.z;
    const float d3 = rc_dot(e1.x, e1.y, e1.z, bpx, bpy, bpz), d4 = rc_dot(e2.x, e2.y, e2.z, bpx, bpy, bpz);
    const float cpx = apx - e2.x, cpy = apy - e2.y, cpz = apz - e2.z;
    const float d5 = rc_dot(e1.x, e1.y, e1.z, cpx, cpy, cpz), d6 = rc_dot(e2.x, e2.y, e2.z, cpx, cpy, cpz);
    const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    const float d43 = d4 - d3, d56 = d5 - d6;
    if (d1 <= 0.f && d2 <= 0.f) {
        u = 0.f, v = 0.f;
    } else if (d3 >= 0.f && d4 <= d3) {
        u = 1.f, v = 0.f;
    } else if (vc <= 0.f && d1 >= 0.f && d3 <= 0.f) {
        u = d1 / (d1 - d3), v = 0.f;
    } else if (d6 >= 0.f && d5 <= d6) {
        u = 0.f, v = 1.f;
    } else if (vb <= 0.f && d2 >= 0.f && d6 <= 0.f) {
        u = 0.f, v = d2 / (d2 - d6);
    } else if (va <= 0.f && d43 >= 0.f && d56 >= 0.f) {
        const float w = d43 / (d43 + d56);
        u = 1.f - w, v = w;
    } else {
        const float den = 1.f / ((va + vb) + vc);
        u = vb * den, v = vc * den;
        u = u < 0.f ? 0.f : u;
        u = u > 1.f ? 1.f : u;
        const float rest = 1.f - u;
        v = v < 0.f ? 0.f : v;
        v = v > rest ? rest : v;
    }
    const float rx = __builtin_fmaf(-v, e2.x, __builtin_fmaf(-u, e1.x, apx));
    const float ry = __builtin_fmaf(-v, e2.y, __builtin_fmaf(-u, e1.y, apy));
    const float rz = __builtin_fmaf(-v, e2.z, __builtin_fmaf(-u, e1.z, apz));
    r[0] = rx, r[1] = ry, r[2] = rz;
    return rc_dot(rx, ry, rz, rx, ry, rz);
}
__device__ __forceinline__ float cp_pair(const float (&q)[3], f32x4 a, f32x4 e1, f32x4 e2, float& u, float& v) {
    float r[3];
    return cp_pair_r(q, a, e1, e2, u, v, r);
}

}  // namespace fgc
