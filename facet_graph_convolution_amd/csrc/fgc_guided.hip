// Guidance normals of guided normal filtering (include/fgc.h: fgc_guided_normals; a build extension).
//
//   H(k) = Phi(k) R(k), M(k) = sum of A_a N_a over the patch P(k) = ring[k];  G_i = normalize(M(argmin of H over ring[i]))
//
// Two launches.  gd_patch_kernel writes {M, H} of every face as one float4.  The work per face is small and irregular (a
// ring of about 13 faces, all pairs of them for Phi, three membership tests per member for E), so a face takes one DPP row
// of 16 lanes, four faces per wave: every lane holds one member a of the ring (index, normal, its three edge neighbours)
// and a second copy b of the row's members (index, normal, area) goes round the row one lane at a time (row_ror:15, a
// rotation to the left).  After 16 steps every lane has met every member: |N_a - N_b|^2 feeds the running maximum for Phi
// (the square root is taken once, at the end: it is monotone), a member b that is one of a's edge neighbours with a < b
// is an edge of E(k) and adds sqrt(|N_a - N_b|^2) to the lane's sum and maximum, and lane 0, which meets the members in
// slot order, adds A_b N_b to M - the order the definition asks for.  The row's maxima and its sum merge by the usual four
// DPP steps.  Empty slots (and indices outside [0, n)) carry the face's own normal, area 0 and index -1: they change no
// maximum, add zero to M and match no edge.
// Rings above 16 (fan vertices, irregular meshes) take the SAME body in rounds: the row's members in chunks of 16, chunk
// ca on the lanes against chunk cb going round, all nch x nch blocks (nch = chunks up to the row's last valid slot, <= 4);
// M is summed in the ca = 0 round, where lane 0 meets chunk after chunk in slot order.  Built this way and not as a looped
// form chosen per face: it is the one code path that the common ring (nch = 1: one block, exactly the 16 steps above) takes
// as well, so the rare case is not a second kernel to keep exact, and the trip counts are uniform per row, which is all a
// row operation needs.
// gd_pick_kernel: one lane per face reads H of its ring (at most ld values) and M of the winner.
//
// Device data is never trusted for addressing: ring entries are checked before they index, fe entries are only compared.
#include "fgc_common.h"

#pragma clang fp contract(off)

namespace fgc {

constexpr int GD_THREADS = 256;
constexpr int GD_ROW = 16;

// one lane to the left inside each row of 16: lane l takes the value of lane (l + 1) & 15
__device__ __forceinline__ float gd_next(float v) { return fgc_dpp_c<0x12F>(v); }
__device__ __forceinline__ int gd_next(int v) { return __builtin_amdgcn_update_dpp(0, v, 0x12F, 0xF, 0xF, true); }
// maximum over each row of 16 lanes, in every lane (the steps of FGC_ROW16_SUM)
__device__ __forceinline__ float gd_row_max(float v) {
    v = fmaxf(v, fgc_dpp_c<0xB1>(v));
    v = fmaxf(v, fgc_dpp_c<0x4E>(v));
    v = fmaxf(v, fgc_dpp_c<0x141>(v));
    return fmaxf(v, fgc_dpp_c<0x140>(v));
}
__device__ __forceinline__ int gd_row_max(int v) {
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, true));
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xF, 0xF, true));
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x141, 0xF, 0xF, true));
    return max(v, __builtin_amdgcn_update_dpp(0, v, 0x140, 0xF, 0xF, true));
}

__global__ __launch_bounds__(GD_THREADS) void gd_patch_kernel(const float* __restrict__ nrm, const float* __restrict__ area,
                                                              int n, const int* __restrict__ ring, int ld,
                                                              const int* __restrict__ fe, f32x4* __restrict__ mh) {
    const int face = blockIdx.x * (GD_THREADS / GD_ROW) + (threadIdx.x >> 4);
    const int l = threadIdx.x & (GD_ROW - 1);
    if (face >= n) return;                                  // whole rows leave: the row operations below stay inside a row
    const int* rg = ring + (size_t)face * ld;
    const float sx = nrm[3 * (size_t)face], sy = nrm[3 * (size_t)face + 1], sz = nrm[3 * (size_t)face + 2];
    // chunks up to the row's last valid slot
    int last = -1;
    for (int s = l; s < ld; s += GD_ROW)
        if ((unsigned)rg[s] < (unsigned)n) last = s;
    const int nch = (gd_row_max(last) + GD_ROW) / GD_ROW;   // 0 .. 4, the same in the whole row

    float phi2 = 0.f, esum = 0.f, emax = 0.f, m0 = 0.f, m1 = 0.f, m2 = 0.f;
    for (int ca = 0; ca < nch; ++ca) {
        const int sa = ca * GD_ROW + l;
        const int ia = sa < ld ? rg[sa] : -1;
        float ax = sx, ay = sy, az = sz;
        int e0 = -2, e1 = -2, e2 = -2;                      // -2 matches no member: an empty lane is index -1
        if ((unsigned)ia < (unsigned)n) {
            ax = nrm[3 * (size_t)ia], ay = nrm[3 * (size_t)ia + 1], az = nrm[3 * (size_t)ia + 2];
            const int f0 = fe[3 * (size_t)ia], f1 = fe[3 * (size_t)ia + 1], f2 = fe[3 * (size_t)ia + 2];
            e0 = f0 > ia ? f0 : -2, e1 = f1 > ia ? f1 : -2, e2 = f2 > ia ? f2 : -2;   // every edge once: from its lower face
        }
        for (int cb = 0; cb < nch; ++cb) {
            const int sb = cb * GD_ROW + l;
            int ib = sb < ld ? rg[sb] : -1;
            float bx = sx, by = sy, bz = sz, ba = 0.f;
            if ((unsigned)ib < (unsigned)n) {
                bx = nrm[3 * (size_t)ib], by = nrm[3 * (size_t)ib + 1], bz = nrm[3 * (size_t)ib + 2];
                ba = area[ib];
            } else {
                ib = -1;
            }
#pragma unroll
            for (int r = 0; r < GD_ROW; ++r) {
                const float dx = ax - bx, dy = ay - by, dz = az - bz;
                const float d2 = __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));
                phi2 = fmaxf(phi2, d2);
                const float phi = __builtin_sqrtf(d2);
                if (ib == e0) esum += phi, emax = fmaxf(emax, phi);
                if (ib == e1) esum += phi, emax = fmaxf(emax, phi);
                if (ib == e2) esum += phi, emax = fmaxf(emax, phi);
                if (ca == 0) {
                    const float px = ba * bx, py = ba * by, pz = ba * bz;
                    m0 += px, m1 += py, m2 += pz;
                }
                ib = gd_next(ib), bx = gd_next(bx), by = gd_next(by), bz = gd_next(bz), ba = gd_next(ba);
            }
        }
    }
    phi2 = gd_row_max(phi2);
    emax = gd_row_max(emax);
    FGC_ROW16_SUM(esum);
    if (l == 0) {
        const float h = __builtin_sqrtf(phi2) * (emax / (0.000000001f + esum));
        mh[face] = f32x4{m0, m1, m2, h};
    }
}

__global__ __launch_bounds__(GD_THREADS) void gd_pick_kernel(const f32x4* __restrict__ mh, int n, const int* __restrict__ ring,
                                                             int ld, float* __restrict__ guide, int* __restrict__ pick_out,
                                                             float* __restrict__ h_out) {
    const int i = blockIdx.x * GD_THREADS + threadIdx.x;
    if (i >= n) return;
    const int4* rg = reinterpret_cast<const int4*>(ring + (size_t)i * ld);
    int best = -1;
    float hb = 0.f;
    for (int s = 0; s < ld / 4; ++s) {
        const int4 r4 = rg[s];
        const int ks[4] = {r4.x, r4.y, r4.z, r4.w};
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int k = ks[t];
            if ((unsigned)k >= (unsigned)n) continue;
            const float h = mh[k].w;
            if (best < 0 || h < hb) best = k, hb = h;      // strictly smaller: the first slot wins a tie
        }
    }
    float v[3] = {0.f, 0.f, 0.f};
    if (best >= 0) {
        const f32x4 m = mh[best];
        v[0] = m.x, v[1] = m.y, v[2] = m.z;
    }
    // utils.normalize: x * (1 / (|x| + 1e-8)), twice
#pragma unroll
    for (int twice = 0; twice < 2; ++twice) {
        const float inv = 1.0f / (__builtin_sqrtf((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]) + 0.00000001f);
        v[0] *= inv, v[1] *= inv, v[2] *= inv;
    }
    guide[3 * (size_t)i] = v[0], guide[3 * (size_t)i + 1] = v[1], guide[3 * (size_t)i + 2] = v[2];
    if (pick_out) pick_out[i] = best;
    if (h_out) h_out[i] = mh[i].w;
}

}  // namespace fgc

using namespace fgc;

static bool gd_shape_ok(int32_t n, int32_t ld) {
    return n > 0 && n <= (1 << 27) && ld >= 4 && ld <= FGC_GUIDED_MAX_RING && ld % 4 == 0;
}

extern "C" size_t fgc_guided_workspace_bytes(int32_t n, int32_t ld) {
    return gd_shape_ok(n, ld) ? (size_t)n * sizeof(f32x4) : 0;
}

extern "C" int fgc_guided_normals(const float* normals, const float* areas, int32_t n, const int32_t* ring, int32_t ld,
                                  const int32_t* fe, float* guide_out, int32_t* pick_out, float* h_out, void* workspace,
                                  size_t workspace_bytes, void* stream) {
    FGC_CHECK_ARG(normals && areas && ring && fe && guide_out && workspace, "fgc_guided_normals: null pointer");
    FGC_CHECK_ARG(gd_shape_ok(n, ld), "fgc_guided_normals: n=%d ld=%d (n in 1 .. 2^27, ld a multiple of 4 in 4 .. %d)", n, ld,
                  FGC_GUIDED_MAX_RING);
    FGC_CHECK_ARG(workspace_bytes >= (size_t)n * sizeof(f32x4), "fgc_guided_normals: workspace too small (%zu < %zu bytes)",
                  workspace_bytes, (size_t)n * sizeof(f32x4));
    FGC_CHECK_ARG((uintptr_t)workspace % 16 == 0 && (uintptr_t)ring % 16 == 0,
                  "fgc_guided_normals: workspace and ring need 16-byte alignment");
    hipStream_t st = (hipStream_t)stream;
    f32x4* mh = (f32x4*)workspace;
    FGC_LAUNCH("gd_patch_kernel", st, gd_patch_kernel, dim3(cdiv(n, GD_THREADS / GD_ROW)), dim3(GD_THREADS), 0, normals, areas, n,
               ring, ld, fe, mh);
    FGC_LAUNCH("gd_pick_kernel", st, gd_pick_kernel, dim3(cdiv(n, GD_THREADS)), dim3(GD_THREADS), 0, mh, n, ring, ld, guide_out,
               pick_out, h_out);
    FGC_CHECK_LAUNCH("fgc_guided_normals");
    return FGC_OK;
}
