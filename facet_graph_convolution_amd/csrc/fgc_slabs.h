// What the brute-force scans share (fgc_raycast.hip: fgc_ray_cast; fgc_surface.hip: fgc_closest_point, fgc_surface_loss): ONE
// definition of the launch shape - 64 queries per workgroup, the records split into slabs over blockIdx.y - of the workspace
// (records, then one 64-bit key per query) and of the launch that fills both.
#pragma once
#include "fgc_raycast.h"

namespace fgc {

constexpr int RC_THREADS = 256;
constexpr int RC_WAVES = RC_THREADS / 64;
constexpr int RC_Q = 64;               // rays per workgroup: one per lane, the same in every wave
constexpr int RC_TARGET_WGS = 2048;    // workgroups that fill the device: 256 CUs x 8 of 256 threads
constexpr int RC_MIN_SLAB = 1024;      // records a slab has at least (a slab costs one atomic per ray)
constexpr unsigned long long RC_MISS = 0x7F800000FFFFFFFFull;      // (+inf, face -1)

struct RcLayout {
    int nrec;            // records: nf rounded up to whole chunks
    int slabs, per_slab;
    size_t keys, total;
};

// the slab split depends on (nf, nq) alone
static RcLayout rc_layout(int nf, int nq) {
    RcLayout l;
    l.nrec = cdiv(nf, RC_CHUNK) * RC_CHUNK;
    const int slabs = std::min(cdiv(RC_TARGET_WGS, cdiv(nq, RC_Q)), std::max(1, nf / RC_MIN_SLAB));
    l.per_slab = cdiv(cdiv(nf, slabs), RC_CHUNK * RC_WAVES) * (RC_CHUNK * RC_WAVES);
    l.slabs = cdiv(nf, l.per_slab);
    l.keys = align_up((size_t)l.nrec * 3 * sizeof(f32x4), 16);
    l.total = l.keys + align_up((size_t)nq * sizeof(unsigned long long), 16);
    return l;
}

static __global__ __launch_bounds__(256) void rc_gather_kernel(const float* __restrict__ verts, int nv, const int* __restrict__ faces,
                                                        int nf, int nrec, f32x4* __restrict__ rec,
                                                        unsigned long long* __restrict__ keys, int nq) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < nq) keys[j] = RC_MISS;
    if (j >= nrec) return;
    f32x4 r0, r1, r2;
    float v[3][3];
    rc_record(verts, nv, faces, nf, j, r0, r1, r2, v);
    rec[3 * (size_t)j] = r0, rec[3 * (size_t)j + 1] = r1, rec[3 * (size_t)j + 2] = r2;
}

}  // namespace fgc
