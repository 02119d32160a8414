/* bgk_assign.hip -- permutation reduction (distribution/sampling/_mcmc/permutation.py:38-73): for every sample the m <= 64 identical
 * particles are relabelled onto the reference configuration by a linear sum assignment on the squared distances
 *
 *     C[i][j] = sum_k (xref[i, k] - x[b, j, k])^2          (f32: difference, square, sum over k = 0 .. d-1, every op rounded)
 *
 * solved by shortest augmenting paths with potentials (Jonker-Volgenant / "Hungarian with potentials", O(m^3)): rows are added one at
 * a time, each by a Dijkstra search over the columns on the reduced costs C[i][j] - u[i] - v[j] and an augmentation along the path found.
 *
 * Mapping.  A group of W lanes per sample (W = 64: one wavefront per sample; BGK_ASSIGN_PACK builds 32- and 16-lane groups for m <= 32 /
 * m <= 16, see DESIGN.md "Permutation reduction"), four waves per workgroup.  Lane j of a group owns COLUMN j: its particle's
 * coordinates, v[j], minv[j], way[j], the used bit -- and what belongs to the ROW currently assigned to the column: the row index p[j],
 * that row's potential u[p[j]] and its reference position.  Row-side values of the search (the row at the head of the path, its
 * potential and position) are group-uniform and come out of the owning lane by v_readlane (W = 64) / ds_bpermute (W < 64); the
 * augmentation moves (p, u, position) from lane to lane along the path.  So there is no cost matrix, no u[] array and no LDS in the
 * solver: LDS holds the index list and a particle bitmap for the row copy only.
 * A Dijkstra step is one group-wide minimum (DPP: quad_perm, row_half_mirror, row_mirror, row_bcast15 / 31), a ballot of the lanes
 * that hold it and a count of trailing zeros: ties go to the lowest column, so the permutation is a function of the sample alone.
 *
 * Precision.  The costs are f32 (above); the potentials u, v, the running minima and the step lengths are f64, so the solver finds the
 * optimum of the f32 cost matrix itself: with f32 potentials their rounding, accumulated over a long path, decided near-ties the other
 * way in 2 % of 64-particle 1-d samples at large noise (host restatement of this algorithm against scipy on the same f32 costs; none
 * of 1500 with f64).  f64 adds, compares and minima are full rate on this device; a DPP move or lane read of an f64 is two.
 *
 * Trip bounds.  The row loop runs m times, the search and the unwinding at most m times each, by loop counters; no exit depends on a
 * floating-point comparison coming true: the search picks an unused column in every step whatever the values are (a NaN counts as
 * +inf, and among nothing but +inf the lowest unused column is taken), so it meets a free column after at most (rows assigned + 1)
 * steps; way[] points from a column to one that was used earlier, so the unwinding cannot cycle.  Samples with a non-finite coordinate
 * (among their identical particles or the reference's) never enter the solver: identity, status 1.  Finite inputs whose squares
 * overflow give some valid permutation. */
#include "bgk_common.h"

#ifndef BGK_ASSIGN_PACK
#define BGK_ASSIGN_PACK 1      /* 0: one sample per wavefront for every m (the A/B build of DESIGN.md "Permutation reduction") */
#endif

namespace {

constexpr int ASG_MAX_M = 64;
constexpr int ASG_MAX_ROW = 4096;          /* n d */
constexpr int ASG_WAVES = 4;
constexpr int ASG_THREADS = ASG_WAVES * BGK_WAVE;

struct AsgIndex {
    int32_t v[ASG_MAX_M];
};

/* one DPP move of x; lanes the control or the row mask leaves out receive `old` */
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float asg_dpp(float old, float x) {
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(old), __float_as_int(x), CTRL, ROW_MASK, 0xF, false));
}
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double asg_dpp(double old, double x) {
    const int lo = __builtin_amdgcn_update_dpp(__double2loint(old), __double2loint(x), CTRL, ROW_MASK, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp(__double2hiint(old), __double2hiint(x), CTRL, ROW_MASK, 0xF, false);
    return __hiloint2double(hi, lo);
}

/* value of lane (base + j) of the group; j is group-uniform and in [0, W) */
template <int W>
__device__ __forceinline__ int asg_get(int v, int j, int base) {
    if (W == BGK_WAVE) return __builtin_amdgcn_readlane(v, __builtin_amdgcn_readfirstlane(j));
    return __shfl(v, base + j, BGK_WAVE);
}
template <int W>
__device__ __forceinline__ float asg_get(float v, int j, int base) {
    return __int_as_float(asg_get<W>(__float_as_int(v), j, base));
}
template <int W>
__device__ __forceinline__ double asg_get(double v, int j, int base) {
    return __hiloint2double(asg_get<W>(__double2hiint(v), j, base), asg_get<W>(__double2loint(v), j, base));
}

/* the group's last lane holds the reduction of the 16-lane rows' butterflies; hand it to every lane */
template <int W, typename T>
__device__ __forceinline__ T asg_last(T x, int base) {
    if (W == 16) return x;
    return asg_get<W>(x, W - 1, base);
}

/* minimum over the group's W lanes, in every lane */
template <int W>
__device__ __forceinline__ double asg_min(double x, int base) {
    x = fmin(x, asg_dpp<0xB1, 0xF>(x, x));         /* quad_perm [1, 0, 3, 2] */
    x = fmin(x, asg_dpp<0x4E, 0xF>(x, x));         /* quad_perm [2, 3, 0, 1] */
    x = fmin(x, asg_dpp<0x141, 0xF>(x, x));        /* row_half_mirror */
    x = fmin(x, asg_dpp<0x140, 0xF>(x, x));        /* row_mirror: every lane of a 16-lane row holds the row's */
    if (W >= 32) x = fmin(x, asg_dpp<0x142, 0xA>(x, x));       /* row_bcast15 into rows 1 and 3 */
    if (W >= 64) x = fmin(x, asg_dpp<0x143, 0xC>(x, x));       /* row_bcast31 into rows 2 and 3 */
    return asg_last<W>(x, base);
}

/* sum over the group's W lanes in that fixed order, in every lane */
template <int W>
__device__ __forceinline__ float asg_sum(float x, int base) {
    x = x + asg_dpp<0xB1, 0xF>(0.0f, x);
    x = x + asg_dpp<0x4E, 0xF>(0.0f, x);
    x = x + asg_dpp<0x141, 0xF>(0.0f, x);
    x = x + asg_dpp<0x140, 0xF>(0.0f, x);
    if (W >= 32) x = x + asg_dpp<0x142, 0xA>(0.0f, x);
    if (W >= 64) x = x + asg_dpp<0x143, 0xC>(0.0f, x);
    return asg_last<W>(x, base);
}

/* the group's W ballot bits, bit j = lane base + j */
template <int W>
__device__ __forceinline__ unsigned long long asg_ballot(bool pred, int base) {
    const unsigned long long all = __ballot(pred);
    if (W == BGK_WAVE) return all;
    return (all >> base) & ((1ull << W) - 1ull);
}

template <int D>
__device__ __forceinline__ float asg_cost(const float (&r)[D], const float (&c)[D]) {
    float s = 0.0f;
#pragma unroll
    for (int k = 0; k < D; ++k) {
        const float t = r[k] - c[k];
        s = k ? s + t * t : t * t;
    }
    return s;
}

template <int D, int W>
__global__ __launch_bounds__(ASG_THREADS) void assign_kernel(const float* __restrict__ x, int64_t ldx, int64_t B, int n,
                                                             const float* __restrict__ xref, const AsgIndex idx, int m,
                                                             float* __restrict__ y, int64_t ldy, int32_t* __restrict__ perm,
                                                             float* __restrict__ cost, int32_t* __restrict__ status,
                                                             int32_t* __restrict__ permuted) {
    __shared__ uint32_t s_ident[ASG_MAX_ROW / 32];         /* bit q: particle q is one of the identical ones */
    __shared__ int32_t s_idx[ASG_MAX_M];
    const int t = threadIdx.x;
    if (t < ASG_MAX_ROW / 32) s_ident[t] = 0u;
    if (t < ASG_MAX_M) s_idx[t] = t < m ? idx.v[t] : 0;
    __syncthreads();
    if (t < m) atomicOr(&s_ident[s_idx[t] >> 5], 1u << (s_idx[t] & 31));
    __syncthreads();

    constexpr int G = BGK_WAVE / W;                        /* samples per wavefront */
    constexpr float INF = __builtin_inff();
    constexpr double DINF = __builtin_inf();
    const int lane = t & (BGK_WAVE - 1), jl = lane & (W - 1), base = lane - jl;
    const int64_t b0 = ((int64_t)blockIdx.x * ASG_WAVES + t / BGK_WAVE) * G;
    if (b0 >= B) return;                                   /* the whole wavefront (no barrier below) */
    const int64_t b = b0 + lane / W;
    const bool sample = b < B;
    const bool col = sample && jl < m;
    const int mine = col ? s_idx[jl] : 0;                  /* particle of column jl = particle of row jl */
    float cx[D], xr[D];
#pragma unroll
    for (int k = 0; k < D; ++k) {
        cx[k] = col ? x[b * ldx + (int64_t)mine * D + k] : 0.0f;
        xr[k] = col ? xref[mine * D + k] : 0.0f;
    }
    bool finite = true;
#pragma unroll
    for (int k = 0; k < D; ++k) finite = finite && __builtin_fabsf(cx[k]) < INF && __builtin_fabsf(xr[k]) < INF;
    const bool bad = asg_ballot<W>(col && !finite, base) != 0ull;
    const bool live = sample && !bad;                      /* group-uniform */

    /* what lane jl holds of the row assigned to its column */
    int p = bad && col ? jl : -1;
    double ua = 0.0, v = 0.0;
    float ax[D];
#pragma unroll
    for (int k = 0; k < D; ++k) ax[k] = bad ? xr[k] : 0.0f;

    if (__any(live)) {
        for (int i = 0; i < m; ++i) {
            float ri[D], r0[D];                            /* position of row i; of the row at the head of the path */
#pragma unroll
            for (int k = 0; k < D; ++k) r0[k] = ri[k] = asg_get<W>(xr[k], i, base);
            double ucur = 0.0, u0 = 0.0;                   /* u[i]; u of the row at the head of the path */
            double minv = DINF;
            int way = -1, j0 = -1;                         /* -1: the start (row i is not in a column yet) */
            bool used = false, searching = live;
            for (int step = 0; step < m; ++step) {
                if (!__any(searching)) break;
                const bool open = col && !used;
                const double cur = (double)asg_cost<D>(r0, cx) - u0 - v;
                if (searching && open && cur < minv) { minv = cur; way = j0; }
                const double val = (open && minv == minv) ? minv : DINF;
                const double delta = asg_min<W>(val, base);
                /* the open columns that hold the minimum: at least one while the group searches (+inf == +inf); a group of a packed
                 * wavefront that has finished may have none */
                const unsigned long long cand = asg_ballot<W>(open && val == delta, base);
                const int j1 = cand ? __builtin_ctzll(cand) : 0;
                if (searching) {
                    if (used) { ua += delta; v -= delta; }
                    else if (col) minv -= delta;
                    ucur += delta;
                    if (jl == j1) used = true;
                    j0 = j1;
                }
                const int pj = asg_get<W>(p, j1, base);
                const double uj = asg_get<W>(ua, j1, base);
#pragma unroll
                for (int k = 0; k < D; ++k) {
                    const float a = asg_get<W>(ax[k], j1, base);
                    if (searching && pj >= 0) r0[k] = a;
                }
                if (searching && pj >= 0) u0 = uj;
                if (pj < 0) searching = false;                                  /* column j0 is free: the path ends there */
            }
            /* augment: column j0 takes the row of way[j0], that column the row of its own predecessor, .., the start's takes row i */
            bool unwinding = live;
            for (int step = 0; step < m; ++step) {
                if (!__any(unwinding)) break;
                const int jc = j0 < 0 ? 0 : j0;
                const int j1 = asg_get<W>(way, jc, base);
                const int js = j1 < 0 ? 0 : j1;
                const int np = asg_get<W>(p, js, base);
                const double nu = asg_get<W>(ua, js, base);
                float na[D];
#pragma unroll
                for (int k = 0; k < D; ++k) na[k] = asg_get<W>(ax[k], js, base);
                if (unwinding && jl == j0) {
                    p = j1 < 0 ? i : np;
                    ua = j1 < 0 ? ucur : nu;
#pragma unroll
                    for (int k = 0; k < D; ++k) ax[k] = j1 < 0 ? ri[k] : na[k];
                }
                if (j1 < 0) unwinding = false;
                if (unwinding) j0 = j1;
            }
        }
    }

    const bool placed = col && (unsigned)p < (unsigned)m;                       /* (every column, after m rows) */
    const bool moved = asg_ballot<W>(col && p != jl, base) != 0ull;
    const float total = asg_sum<W>(placed ? asg_cost<D>(ax, cx) : 0.0f, base);
    if (sample && jl == 0) {
        if (cost) cost[b] = total;
        if (status) status[b] = bad ? 1 : 0;
        if (permuted) permuted[b] = moved ? 1 : 0;
    }
    if (perm && placed) perm[b * m + p] = jl;
    if (y && sample) {
        const int nd = n * D;
        for (int c = jl; c < nd; c += W) {
            const int q = c / D;
            if (!((s_ident[q >> 5] >> (q & 31)) & 1u)) y[b * ldy + c] = x[b * ldx + c];
        }
        if (placed) {
            const int64_t dst = b * ldy + (int64_t)s_idx[p] * D;
#pragma unroll
            for (int k = 0; k < D; ++k) y[dst + k] = cx[k];
        }
    }
}

template <int D>
void assign_launch(const float* x, int64_t ldx, int64_t B, int n, const float* xref, const AsgIndex& idx, int m, float* y, int64_t ldy,
                   int32_t* perm, float* cost, int32_t* status, int32_t* permuted, hipStream_t st) {
    const int W = !BGK_ASSIGN_PACK ? 64 : (m <= 16 ? 16 : (m <= 32 ? 32 : 64));
    const int64_t per_block = (int64_t)ASG_WAVES * (BGK_WAVE / W);
    const dim3 grid((unsigned)((B + per_block - 1) / per_block)), block(ASG_THREADS);
    if (W == 16)
        hipLaunchKernelGGL((assign_kernel<D, 16>), grid, block, 0, st, x, ldx, B, n, xref, idx, m, y, ldy, perm, cost, status, permuted);
    else if (W == 32)
        hipLaunchKernelGGL((assign_kernel<D, 32>), grid, block, 0, st, x, ldx, B, n, xref, idx, m, y, ldy, perm, cost, status, permuted);
    else
        hipLaunchKernelGGL((assign_kernel<D, 64>), grid, block, 0, st, x, ldx, B, n, xref, idx, m, y, ldy, perm, cost, status, permuted);
}

}  // namespace

extern "C" int bgk_assign_particles(const float* x, int64_t ldx, int64_t B, int32_t n, int32_t d, const float* xref,
                                    const int32_t* identical_host, int32_t m, float* y, int64_t ldy, int32_t* perm, float* cost,
                                    int32_t* status, int32_t* permuted, void* stream) {
    BGK_CHECK_ARG(x && xref && identical_host, "bgk_assign_particles: null pointer (x, xref, identical_host)");
    BGK_CHECK_ARG(B >= 0 && B <= ((int64_t)1 << 31), "bgk_assign_particles: bad batch size %lld", (long long)B);
    BGK_CHECK_ARG(m >= 1 && m <= ASG_MAX_M, "bgk_assign_particles: m = %d identical particles (1 .. %d)", (int)m, ASG_MAX_M);
    BGK_CHECK_ARG(d >= 1 && d <= 3, "bgk_assign_particles: d = %d dimensions (1 .. 3)", (int)d);
    BGK_CHECK_ARG(n >= m && (int64_t)n * d <= ASG_MAX_ROW, "bgk_assign_particles: n = %d particles (m .. %d / d)", (int)n, ASG_MAX_ROW);
    AsgIndex idx;
    for (int i = 0; i < ASG_MAX_M; ++i) idx.v[i] = 0;
    for (int i = 0; i < m; ++i) {
        const int32_t q = identical_host[i];
        BGK_CHECK_ARG(q >= 0 && q < n && (i == 0 || q > identical_host[i - 1]),
                      "bgk_assign_particles: identical[%d] = %d (indices must be strictly increasing and in [0, %d))", i, (int)q, (int)n);
        idx.v[i] = q;
    }
    const int64_t nd = (int64_t)n * d;
    BGK_CHECK_ARG(ldx >= nd && (!y || ldy >= nd), "bgk_assign_particles: a row stride is below n d = %lld", (long long)nd);
    BGK_CHECK_ARG(((uintptr_t)x | (uintptr_t)xref | (uintptr_t)y | (uintptr_t)perm | (uintptr_t)cost | (uintptr_t)status |
                   (uintptr_t)permuted) % 4 == 0, "bgk_assign_particles: a pointer is not aligned to 4 bytes");
    if (B == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    if (d == 1) assign_launch<1>(x, ldx, B, n, xref, idx, m, y, ldy, perm, cost, status, permuted, st);
    else if (d == 2) assign_launch<2>(x, ldx, B, n, xref, idx, m, y, ldy, perm, cost, status, permuted, st);
    else assign_launch<3>(x, ldx, B, n, xref, idx, m, y, ldy, perm, cost, status, permuted, st);
    return bgk_launch_status("bgk_assign_particles");
}
