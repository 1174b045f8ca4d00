// Bilateral normal filter over a list of triangles (utils.bilateralFilter / utils.FND, utils.py:2344-2496):
//
//   out[i, p] = normalize( sum over j in window(i) of a_j exp(-|c_i - c_j|^2 / (2 ss^2)) exp(-|n_i - n_j|^2 / (2 sr^2)) n_j )
//
// for P = S x R pairs (ss, sr) at once, window(i) = the 3 x 3 x 3 block of cells around face i's cell.
//
// Three launches and a memset.  bl_gather_kernel puts the faces into cell order as two float4 per face, (c, a) and (n, 0).
// bl_tasks_kernel (one workgroup) turns the range table into a list of tasks (cell, 64-query chunk of that cell).
// bl_filter_kernel runs one task per workgroup of four waves.  All four waves hold the SAME 64 queries, one per lane; the
// window is at most 9 contiguous candidate ranges (the cells along z are adjacent in the flattened grid), cut into chunks
// of BL_CHUNK candidates that the waves take in turn (a range's last chunk is filled up with zero-area candidates).
// Candidates are wave-uniform: a chunk comes through scalar loads and reaches the VALU from SGPRs.  Per pair of faces:
// 3 subtractions, 1 multiply and 2 FMAs for each of |dc|^2 and |dn|^2 (12), then per sigma_s a multiply, v_exp_f32 and
// the multiply by the area, per sigma_r a multiply and v_exp_f32, per (s, r) one multiply and three FMAs (the compiler
// packs two of them into a v_pk_fma_f32): 20 vector instructions, two of them transcendental, for P = 1.
// The four partial sums of a query merge through LDS in wave order, so a row's sum has one fixed order whatever the
// launch: deterministic, and the same order and the same per-pair arithmetic (contraction is off, every FMA is written
// out) in every instantiation, so a multi-pair call equals the single-pair calls bit for bit.
//
// sigma_r = -1 ("no range term") runs as a zero factor: exp2(|dn|^2 * 0) = 1 exactly.
//
// The guided form (fgc_bilateral_filter_guided, a build extension; GUIDED = true in the templates below) takes the range term
// on a guidance normal g instead of n: a third float4 plane (g, 0) behind the two, three more query registers, the same loop
// in the same order; the unguided instantiations are the code they were.
//
// Device data is never trusted for addressing: ranges are clamped to [0, n], face indices are checked before a store.
#include "fgc_common.h"

#pragma clang fp contract(off)

namespace fgc {

constexpr int BL_THREADS = 256;
constexpr int BL_WAVES = BL_THREADS / 64;
constexpr int BL_Q = 64;          // queries per task: one per lane, the same in every wave
constexpr int BL_CHUNK = 8;       // candidates per scalar-load chunk (16 dwords x 4)
constexpr int BL_FLUSH = 32;      // chunks between two flushes of a wave's running sums into its totals
constexpr int BL_MAX_S = 4;       // sigma_s per launch
constexpr int BL_MAX_R = 3;       // sigma_r per launch
constexpr int BL_TASK_THREADS = 1024;

struct BlParams {
    float ks[BL_MAX_S];   // -log2(e) / (2 sigma_s^2)
    float kr[BL_MAX_R];   // -log2(e) / (2 sigma_r^2), 0 for sigma_r = -1
    int col[BL_MAX_S];    // first output column of (s, r = 0)
};

__device__ __forceinline__ int bl_clamp(int v, int lo, int hi) { return min(max(v, lo), hi); }

// GUIDED: a third plane behind the two of every candidate, cand[2 (n + BL_CHUNK) + j] = (g, 0), the guidance normal
template <bool GUIDED>
__global__ __launch_bounds__(256) void bl_gather_kernel(const float* __restrict__ c, const float* __restrict__ nrm,
                                                        const float* __restrict__ a, const float* __restrict__ guide,
                                                        const int* __restrict__ order, int n, f32x4* __restrict__ cand) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n + BL_CHUNK) return;
    const int f = j < n ? order[j] : -1;      // the last BL_CHUNK entries are padding: zero candidates
    f32x4 v0 = {0.f, 0.f, 0.f, 0.f}, v1 = {0.f, 0.f, 0.f, 0.f};
    if ((unsigned)f < (unsigned)n) {
        v0 = f32x4{c[3 * (size_t)f], c[3 * (size_t)f + 1], c[3 * (size_t)f + 2], a[f]};
        v1 = f32x4{nrm[3 * (size_t)f], nrm[3 * (size_t)f + 1], nrm[3 * (size_t)f + 2], 0.f};
    }
    cand[2 * (size_t)j] = v0;
    cand[2 * (size_t)j + 1] = v1;
    if constexpr (GUIDED) {
        f32x4 v2 = {0.f, 0.f, 0.f, 0.f};
        if ((unsigned)f < (unsigned)n) v2 = f32x4{guide[3 * (size_t)f], guide[3 * (size_t)f + 1], guide[3 * (size_t)f + 2], 0.f};
        cand[2 * ((size_t)n + BL_CHUNK) + j] = v2;
    }
}

// tasks[t] = (cell, chunk) for every 64-query chunk of every occupied cell, in cell order; *ntasks = their number
__global__ __launch_bounds__(BL_TASK_THREADS) void bl_tasks_kernel(const int* __restrict__ cell_ptr, int cells, int n,
                                                                   int2* __restrict__ tasks, int max_tasks,
                                                                   int* __restrict__ ntasks) {
    __shared__ int scan[BL_TASK_THREADS];
    const int t = threadIdx.x;
    const int per = (cells + BL_TASK_THREADS - 1) / BL_TASK_THREADS;
    const int c0 = min(cells, t * per), c1 = min(cells, c0 + per);
    int mine = 0;
    for (int c = c0; c < c1; ++c) {
        const int b = bl_clamp(cell_ptr[c], 0, n), e = bl_clamp(cell_ptr[c + 1], b, n);
        mine += (e - b + BL_Q - 1) / BL_Q;
    }
    scan[t] = mine;
    __syncthreads();
    for (int d = 1; d < BL_TASK_THREADS; d <<= 1) {
        const int v = t >= d ? scan[t - d] : 0;
        __syncthreads();
        scan[t] += v;
        __syncthreads();
    }
    int pos = scan[t] - mine;
    if (t == BL_TASK_THREADS - 1) *ntasks = min(scan[t], max_tasks);
    for (int c = c0; c < c1; ++c) {
        const int b = bl_clamp(cell_ptr[c], 0, n), e = bl_clamp(cell_ptr[c + 1], b, n);
        const int k = (e - b + BL_Q - 1) / BL_Q;
        for (int q = 0; q < k; ++q, ++pos)
            if (pos < max_tasks) tasks[pos] = make_int2(c, q);
    }
}

// GUIDED: the range term is taken on the guidance normals (q[6 .. 8] against g), everything else is the same body
template <int S, int R, bool GUIDED>
__device__ __forceinline__ void bl_visit(const float (&q)[GUIDED ? 9 : 6], float (&acc)[S * R][3], const BlParams& prm,
                                         f32x4 c0, f32x4 c1, f32x4 g) {
    const float dx = q[0] - c0.x, dy = q[1] - c0.y, dz = q[2] - c0.z;
    const float d2 = __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));
    const float ex = q[GUIDED ? 6 : 3] - (GUIDED ? g.x : c1.x), ey = q[GUIDED ? 7 : 4] - (GUIDED ? g.y : c1.y),
                ez = q[GUIDED ? 8 : 5] - (GUIDED ? g.z : c1.z);
    const float e2 = __builtin_fmaf(ez, ez, __builtin_fmaf(ey, ey, ex * ex));
    float ws[S], wr[R];
#pragma unroll
    for (int s = 0; s < S; ++s) ws[s] = __builtin_amdgcn_exp2f(d2 * prm.ks[s]) * c0.w;
#pragma unroll
    for (int r = 0; r < R; ++r) wr[r] = __builtin_amdgcn_exp2f(e2 * prm.kr[r]);
#pragma unroll
    for (int s = 0; s < S; ++s)
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const float w = ws[s] * wr[r];
            acc[s * R + r][0] = __builtin_fmaf(w, c1.x, acc[s * R + r][0]);
            acc[s * R + r][1] = __builtin_fmaf(w, c1.y, acc[s * R + r][1]);
            acc[s * R + r][2] = __builtin_fmaf(w, c1.z, acc[s * R + r][2]);
        }
}

template <int S, int R, bool GUIDED>
__global__ __launch_bounds__(BL_THREADS) void bl_filter_kernel(const f32x4* __restrict__ cand, const int* __restrict__ order,
                                                               const int* __restrict__ cell_ptr,
                                                               const int2* __restrict__ tasks,
                                                               const int* __restrict__ ntasks, int n, int sx, int sy, int sz,
                                                               BlParams prm, float* __restrict__ out, int ld) {
    constexpr int P = S * R;
    __shared__ float part[BL_WAVES][3 * P][BL_Q];
    if ((int)blockIdx.x >= *ntasks) return;
    const int2 task = tasks[blockIdx.x];
    const int cell = bl_clamp(task.x, 0, sx * sy * sz - 1);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int qb = bl_clamp(cell_ptr[cell], 0, n), qe = bl_clamp(cell_ptr[cell + 1], qb, n);
    const int qi = qb + task.y * BL_Q + lane;
    const bool live = qi >= qb && qi < qe;
    float q[GUIDED ? 9 : 6] = {};
    if (live) {
        const f32x4 v0 = cand[2 * (size_t)qi], v1 = cand[2 * (size_t)qi + 1];
        q[0] = v0.x, q[1] = v0.y, q[2] = v0.z, q[3] = v1.x, q[4] = v1.y, q[5] = v1.z;
        if constexpr (GUIDED) {
            const f32x4 v2 = cand[2 * ((size_t)n + BL_CHUNK) + qi];
            q[6] = v2.x, q[7] = v2.y, q[8] = v2.z;
        }
    }
    // two levels: acc takes the candidates one by one and is added to sum (and cleared) every BL_FLUSH chunks, so that no
    // chain of additions is longer than 8 BL_FLUSH + (a wave's candidates) / (8 BL_FLUSH) whatever the window holds
    float acc[P][3], sum[P][3];
#pragma unroll
    for (int p = 0; p < P; ++p) acc[p][0] = acc[p][1] = acc[p][2] = sum[p][0] = sum[p][1] = sum[p][2] = 0.f;
    int since = 0;

    const int ck = cell % sz, cj = (cell / sz) % sy, ci = cell / (sz * sy);
    const int k0 = max(ck - 1, 0), k1 = min(ck + 1, sz - 1);
    for (int ii = max(ci - 1, 0); ii <= min(ci + 1, sx - 1); ++ii)
        for (int jj = max(cj - 1, 0); jj <= min(cj + 1, sy - 1); ++jj) {
            const int row = (ii * sy + jj) * sz;
            const int r0 = bl_clamp(cell_ptr[row + k0], 0, n), r1 = bl_clamp(cell_ptr[row + k1 + 1], r0, n);
            for (int j = r0 + wave * BL_CHUNK; j < r1; j += BL_WAVES * BL_CHUNK) {
                // wave-uniform: scalar loads.  Always a whole chunk (the buffer ends in BL_CHUNK zero entries); what lies past
                // the range is replaced by a zero candidate (area 0: no weight) on the scalar unit
                // (GUIDED: 12 dwords a candidate, so the chunk comes in two halves - a whole one would not fit the SGPRs)
                const f32x4* cb = cand + 2 * (size_t)j;
                const int m = r1 - j;
                constexpr int SUB = GUIDED ? BL_CHUNK / 2 : BL_CHUNK;
#pragma unroll
                for (int h = 0; h < BL_CHUNK; h += SUB) {
                    f32x4 c[2 * SUB], g[SUB];
#pragma unroll
                    for (int t = 0; t < 2 * SUB; ++t) c[t] = cb[2 * h + t];
#pragma unroll
                    for (int t = 0; t < SUB; ++t) g[t] = GUIDED ? cand[2 * ((size_t)n + BL_CHUNK) + j + h + t] : c[0];
#pragma unroll
                    for (int t = 0; t < SUB; ++t) {
                        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
                        bl_visit<S, R, GUIDED>(q, acc, prm, h + t < m ? c[2 * t] : zero, h + t < m ? c[2 * t + 1] : zero,
                                               h + t < m ? g[t] : zero);
                        if (P >= 6) __builtin_amdgcn_sched_barrier(0);   // many pairs: one candidate's weights live at a time
                    }
                }
                if (++since == BL_FLUSH) {
                    since = 0;
#pragma unroll
                    for (int p = 0; p < P; ++p)
#pragma unroll
                        for (int d = 0; d < 3; ++d) sum[p][d] += acc[p][d], acc[p][d] = 0.f;
                }
            }
        }

#pragma unroll
    for (int p = 0; p < P; ++p)
#pragma unroll
        for (int d = 0; d < 3; ++d) part[wave][3 * p + d][lane] = sum[p][d] + acc[p][d];
    __syncthreads();
    const int f = live ? order[qi] : -1;
    if ((unsigned)f >= (unsigned)n) return;
    // pair p of this query: waves 0..3 in order, then utils.normalize (x * (1 / (|x| + 1e-8)), twice)
    for (int p = wave; p < P; p += BL_WAVES) {
        float v[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            float s = part[0][3 * p + d][lane];
#pragma unroll
            for (int w = 1; w < BL_WAVES; ++w) s += part[w][3 * p + d][lane];
            v[d] = s;
        }
#pragma unroll
        for (int twice = 0; twice < 2; ++twice) {
            const float inv = 1.0f / (__builtin_sqrtf((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]) + 0.00000001f);
            v[0] *= inv, v[1] *= inv, v[2] *= inv;
        }
        const int s = p / R, r = p % R;
        float* o = out + (size_t)f * ld + prm.col[s] + 3 * r;
        o[0] = v[0], o[1] = v[1], o[2] = v[2];
    }
}

struct BlLayout {
    size_t cand, tasks, ntasks, total;
    int max_tasks;
};

// planes: float4 per candidate, 2 for the plain filter, 3 for the guided one (the tables follow the planes)
static BlLayout bl_layout(int n, long long cells, int planes) {
    BlLayout L;
    L.max_tasks = (int)(n / BL_Q + (cells < n ? cells : (long long)n) + 1);
    L.cand = 0;
    L.tasks = align_up(((size_t)n + BL_CHUNK) * planes * sizeof(f32x4), 16);
    L.ntasks = L.tasks + align_up((size_t)L.max_tasks * sizeof(int2), 16);
    L.total = L.ntasks + 16;
    return L;
}

template <int S, bool GUIDED>
static void bl_launch_r(int R, hipStream_t st, int grid, const f32x4* cand, const int* order, const int* ptr,
                        const int2* tasks, const int* ntasks, int n, int sx, int sy, int sz, const BlParams& prm, float* out,
                        int ld) {
#define BL_CASE(RR)                                                                                                    \
    case RR:                                                                                                           \
        FGC_LAUNCH(GUIDED ? "bl_filter_guided_kernel" : "bl_filter_kernel", st, (bl_filter_kernel<S, RR, GUIDED>),     \
                   dim3(grid), dim3(BL_THREADS), 0, cand, order, ptr, tasks, ntasks, n, sx, sy, sz, prm, out, ld);     \
        break;
    switch (R) {
        BL_CASE(1)
        BL_CASE(2)
        BL_CASE(3)
    }
#undef BL_CASE
}

// both entry points: guide == NULL is the plain filter (two planes, the launches and the arithmetic it always had)
template <bool GUIDED>
static int bl_run(const char* what, const float* centres, const float* normals, const float* areas, const float* guide,
                  int32_t n, const int32_t* cell_order, const int32_t* cell_ptr, int32_t sx, int32_t sy, int32_t sz,
                  const float* sigma_s, int32_t S, const float* sigma_r, int32_t R, float* out, void* workspace,
                  size_t workspace_bytes, void* stream) {
    FGC_CHECK_ARG(centres && normals && areas && cell_order && cell_ptr && sigma_s && sigma_r && out && workspace &&
                      (guide || !GUIDED),
                  "%s: null pointer", what);
    FGC_CHECK_ARG(n > 0, "%s: n=%d (> 0)", what, n);
    FGC_CHECK_ARG(S >= 1 && R >= 1 && (long long)S * R <= 65536, "%s: S=%d R=%d (both >= 1)", what, S, R);
    FGC_CHECK_ARG(sx >= 1 && sy >= 1 && sz >= 1 && sx <= FGC_BILATERAL_MAX_SLICES && sy <= FGC_BILATERAL_MAX_SLICES &&
                      sz <= FGC_BILATERAL_MAX_SLICES,
                  "%s: grid %d x %d x %d (1 .. %d per axis)", what, sx, sy, sz, FGC_BILATERAL_MAX_SLICES);
    for (int s = 0; s < S; ++s)
        FGC_CHECK_ARG(sigma_s[s] > 0.f && sigma_s[s] < __builtin_inff(), "%s: sigma_s[%d]=%g (> 0)", what, s,
                      (double)sigma_s[s]);
    for (int r = 0; r < R; ++r)
        FGC_CHECK_ARG((sigma_r[r] > 0.f && sigma_r[r] < __builtin_inff()) || sigma_r[r] == -1.f,
                      "%s: sigma_r[%d]=%g (> 0, or -1 for no range term)", what, r, (double)sigma_r[r]);
    const BlLayout L = bl_layout(n, (long long)sx * sy * sz, GUIDED ? 3 : 2);
    // one size for both forms (fgc_bilateral_workspace_bytes): the plain one leaves the room of the third plane unused
    const size_t need = bl_layout(n, (long long)sx * sy * sz, 3).total;
    FGC_CHECK_ARG(workspace_bytes >= need, "%s: workspace too small (%zu < %zu bytes)", what, workspace_bytes, need);
    FGC_CHECK_ARG((uintptr_t)workspace % 16 == 0, "%s: workspace needs 16-byte alignment", what);
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    f32x4* cand = (f32x4*)(ws + L.cand);
    int2* tasks = (int2*)(ws + L.tasks);
    int* ntasks = (int*)(ws + L.ntasks);
    const int ld = 3 * S * R;
    // rows of faces in no cell stay zero
    if (hipMemsetAsync(out, 0, (size_t)n * ld * sizeof(float), st) != hipSuccess) {
        fgc::set_error("%s: memset failed", what);
        return FGC_EHIP;
    }
    FGC_LAUNCH("bl_gather_kernel", st, bl_gather_kernel<GUIDED>, dim3(cdiv(n + BL_CHUNK, 256)), dim3(256), 0, centres, normals,
               areas, guide, cell_order, n, cand);
    FGC_LAUNCH("bl_tasks_kernel", st, bl_tasks_kernel, dim3(1), dim3(BL_TASK_THREADS), 0, cell_ptr, sx * sy * sz, n, tasks,
               L.max_tasks, ntasks);
    const double log2e = 1.4426950408889634;
    for (int s0 = 0; s0 < S; s0 += BL_MAX_S)
        for (int r0 = 0; r0 < R; r0 += BL_MAX_R) {
            const int ts = min(BL_MAX_S, S - s0), tr = min(BL_MAX_R, R - r0);
            BlParams prm = {};
            for (int s = 0; s < ts; ++s) {
                prm.ks[s] = (float)(-log2e / (2.0 * (double)sigma_s[s0 + s] * (double)sigma_s[s0 + s]));
                prm.col[s] = 3 * ((s0 + s) * R + r0);
            }
            for (int r = 0; r < tr; ++r)
                prm.kr[r] = sigma_r[r0 + r] == -1.f
                                ? 0.f
                                : (float)(-log2e / (2.0 * (double)sigma_r[r0 + r] * (double)sigma_r[r0 + r]));
            switch (ts) {
                case 1: bl_launch_r<1, GUIDED>(tr, st, L.max_tasks, cand, cell_order, cell_ptr, tasks, ntasks, n, sx, sy, sz, prm, out, ld); break;
                case 2: bl_launch_r<2, GUIDED>(tr, st, L.max_tasks, cand, cell_order, cell_ptr, tasks, ntasks, n, sx, sy, sz, prm, out, ld); break;
                case 3: bl_launch_r<3, GUIDED>(tr, st, L.max_tasks, cand, cell_order, cell_ptr, tasks, ntasks, n, sx, sy, sz, prm, out, ld); break;
                default: bl_launch_r<4, GUIDED>(tr, st, L.max_tasks, cand, cell_order, cell_ptr, tasks, ntasks, n, sx, sy, sz, prm, out, ld); break;
            }
        }
    FGC_CHECK_LAUNCH(what);
    return FGC_OK;
}

}  // namespace fgc

using namespace fgc;

// room for the guided form's third plane: one size serves both entry points
extern "C" size_t fgc_bilateral_workspace_bytes(int32_t n, int32_t sx, int32_t sy, int32_t sz) {
    if (n <= 0 || sx < 1 || sy < 1 || sz < 1 || sx > FGC_BILATERAL_MAX_SLICES || sy > FGC_BILATERAL_MAX_SLICES ||
        sz > FGC_BILATERAL_MAX_SLICES)
        return 0;
    return bl_layout(n, (long long)sx * sy * sz, 3).total;
}

extern "C" int fgc_bilateral_filter(const float* centres, const float* normals, const float* areas, int32_t n,
                                    const int32_t* cell_order, const int32_t* cell_ptr, int32_t sx, int32_t sy, int32_t sz,
                                    const float* sigma_s, int32_t S, const float* sigma_r, int32_t R, float* out,
                                    void* workspace, size_t workspace_bytes, void* stream) {
    return bl_run<false>("fgc_bilateral_filter", centres, normals, areas, nullptr, n, cell_order, cell_ptr, sx, sy, sz, sigma_s,
                         S, sigma_r, R, out, workspace, workspace_bytes, stream);
}

extern "C" int fgc_bilateral_filter_guided(const float* centres, const float* normals, const float* areas, int32_t n,
                                           const int32_t* cell_order, const int32_t* cell_ptr, int32_t sx, int32_t sy,
                                           int32_t sz, const float* sigma_s, int32_t S, const float* sigma_r, int32_t R,
                                           const float* guide, float* out, void* workspace, size_t workspace_bytes,
                                           void* stream) {
    return bl_run<true>("fgc_bilateral_filter_guided", centres, normals, areas, guide, n, cell_order, cell_ptr, sx, sy, sz,
                        sigma_s, S, sigma_r, R, out, workspace, workspace_bytes, stream);
}
