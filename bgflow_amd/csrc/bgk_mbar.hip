/* bgk_mbar.hip -- binless WHAM / MBAR over K harmonic umbrella windows on one scalar reaction coordinate (what
 * distribution/sampling/_mcmc/umbrella_sampling.py:182-228 hands to pyemma.thermo.estimate_umbrella_sampling) as a deterministic
 * two-stage reduction whose second stage also advances the self-consistent iteration, so that one iteration
 *
 *     D_n  = log sum_l N_l exp(f_l - b_l(r_n)),   b_l(r) = kappa_l (r - m_l)^2          for every sample n of every window
 *     W_nk = N_k exp(f_k - b_k(r_n) - D_n)                                              0 <= W_nk <= 1 by construction
 *     S_k  = sum_n W_nk
 *     f_k <- f_k - (log S_k - log N_k), then all f shifted so that f_0 = 0;   err = max_k |f_k_new - f_k_old|
 *
 * is two launches and no host read.  The bias is formed from r_n on the fly: no [K, N] array exists anywhere.
 * Roofline: an iteration reads the N samples once (4 or 8 B each; L2 / Infinity-Cache resident after the first pass) and spends 2 K N f64
 * exponentials (K per sample for D_n, K per sample for the W_nk), i.e. it is bound by the f64 vector rate, not by bytes: at K = 32,
 * N = 2^20 that is 6.7e7 exponentials per iteration.
 *
 * Stage 1 (mbar_partial_kernel): block b takes one slice of bgk_reduce.h of the pooled samples (head, 16-byte pieces, tail).  The block
 * holds c_l = log N_l + f_l, kappa_l, m_l in LDS (every lane reads the same l at the same time: broadcast reads) and walks its slice in
 * tiles of MBAR_TILE samples.  Per tile, (A) each thread forms D_n of its samples in two passes over l (the maximum of a_l = c_l - b_l(r_n),
 * then sum exp(a_l - max)) and leaves r_n, D_n in LDS; (B) the waves split the windows (wave w takes k = w, w + 4, ...), the lanes stride
 * over the tile's samples, merge in the lane order of bgk_reduce.h, and lane 0 adds the tile's sum to the block's S_k in LDS (only this wave
 * touches that k).  One S_k per block and window goes to partial[n_blocks, K].  No atomics and no per-thread array of K accumulators.
 * Stage 2 (mbar_advance_kernel, ONE workgroup): thread k adds the block partials of window k in block order (16 loads in flight; read one by
 * one, each waiting for the add before it, the 512 partials cost as much as stage 1 at K = 32), forms the new f_k, the shift by the new f_0
 * goes through LDS, err is merged with a maximum that keeps a NaN (lanes, then the waves in order), thread 0 advances the record.  The
 * record protocol is bgk_reduce.h's: steps enqueued past the end cost two empty launches each.
 *
 * NaN / infinity: a NaN sample gives a NaN D_n, a NaN S_k for every k, a NaN err: status 3.  An infinite sample gives a_l = -inf for
 * every l and exp(-inf - -inf) = NaN: status 3 as well.
 *
 * The iteration is restated in torch ops by bgflow_amd/umbrella.py::_mbar_torch; the two must stay the same, step for step. */
#include "bgk_reduce.h"

namespace {

enum { PH_ITERATE = 0, PH_DONE = 1 };
/* the record, BGK_MBAR_RECORD_DOUBLES doubles (include/bgflow_amd.h) */
enum { R_PHASE = BGK_R_PHASE, R_STATUS = BGK_R_STATUS, R_N_ITER, R_ERR, R_K, R_N, R_PAD0, R_PAD1, R_COUNT };
static_assert(R_COUNT == BGK_MBAR_RECORD_DOUBLES, "record layout");

constexpr int MBAR_THREADS = 256;
constexpr int MBAR_WAVES = MBAR_THREADS / BGK_WAVE;
constexpr int MBAR_MAX_BLOCKS = 512;
constexpr int MBAR_MAX_K = 256;
constexpr int MBAR_TILE = 1024;             /* samples per tile: a multiple of both piece widths */
constexpr int MBAR_SLOTS = MBAR_TILE + 4;   /* + the scalar head (at most 3 elements), which rides with the first tile */

/* the window table in LDS */
struct Windows {
    double c[MBAR_MAX_K];        /* log N_l + f_l */
    double kappa[MBAR_MAX_K];
    double m[MBAR_MAX_K];
};

__device__ __forceinline__ void windows_load(Windows& w, const double* __restrict__ table, const double* __restrict__ f, int K) {
    for (int l = threadIdx.x; l < K; l += blockDim.x) {
        w.m[l] = table[3 * l];
        w.kappa[l] = table[3 * l + 1];
        w.c[l] = table[3 * l + 2] + f[l];
    }
}

/* D = log sum_l exp(c_l - kappa_l (r - m_l)^2): the maximum first (it keeps a NaN -- fmax would drop it), then the sum */
__device__ __forceinline__ double mbar_log_denominator(const Windows& w, int K, double r) {
    double mx = -__builtin_inf();
    for (int l = 0; l < K; ++l) {
        const double d = r - w.m[l];
        const double a = w.c[l] - w.kappa[l] * (d * d);
        mx = bgk_nan_max(mx, a);
    }
    double s = 0.0;
    for (int l = 0; l < K; ++l) {
        const double d = r - w.m[l];
        s += exp((w.c[l] - w.kappa[l] * (d * d)) - mx);
    }
    return mx + log(s);
}

template <typename T>
__global__ __launch_bounds__(MBAR_THREADS) void mbar_partial_kernel(const T* __restrict__ rc, int64_t n, int64_t per,
                                                                    const double* __restrict__ table, int K, const double* __restrict__ f,
                                                                    const double* __restrict__ record, double* __restrict__ partial) {
    __shared__ Windows w;
    __shared__ double s_sum[MBAR_MAX_K];
    __shared__ double s_r[MBAR_SLOTS], s_d[MBAR_SLOTS];
    if (bgk_solver_phase(record) == PH_DONE) return;
    const int t = threadIdx.x;
    windows_load(w, table, f, K);
    for (int k = t; k < K; k += MBAR_THREADS) s_sum[k] = 0.0;
    const int64_t blk = blockIdx.x;
    const BgkSlice<T> sl(rc, n, per, blk);
    constexpr int N = BgkPiece<T>::N;
    const int wave = t / BGK_WAVE, lane = t & (BGK_WAVE - 1);
    __syncthreads();
    for (int64_t c0 = 0; c0 == 0 || c0 < sl.body; c0 += MBAR_TILE) {
        /* (A) r_n and D_n of the tile's samples into LDS: slot e holds body element c0 + e; the head follows the first tile's body */
        const int clen = (int)((sl.body - c0) < MBAR_TILE ? (sl.body - c0) : MBAR_TILE);
        const int npiece = clen / N;
        const auto put = [&](int e, double r) { s_r[e] = r; s_d[e] = mbar_log_denominator(w, K, r); };
        for (int v = t; v < npiece; v += MBAR_THREADS) {
            double r[N];
            bgk_piece_unpack(sl.pv[c0 / N + v], r);
#pragma unroll
            for (int i = 0; i < N; ++i) put(N * v + i, r[i]);
        }
        const int done = npiece * N;
        if (t < clen - done) put(done + t, (double)sl.p[sl.head + c0 + done + t]);
        const int extra = c0 == 0 ? (int)sl.head : 0;
        if (t < extra) put(clen + t, (double)sl.p[t]);
        const int cnt = clen + extra;            /* <= MBAR_SLOTS */
        __syncthreads();
        /* (B) wave w: S_k of the tile for k = w, w + 4, ... */
        for (int k = wave; k < K; k += MBAR_WAVES) {
            const double ck = w.c[k], kk = w.kappa[k], mk = w.m[k];
            double acc = 0.0;
            for (int e = lane; e < cnt; e += BGK_WAVE) {
                const double d = s_r[e] - mk;
                acc += exp((ck - kk * (d * d)) - s_d[e]);
            }
            bgk_wave_reduce(acc, [](double& a, double b) { a += b; });
            if (lane == 0) s_sum[k] += acc;
        }
        __syncthreads();
    }
    for (int k = t; k < K; k += MBAR_THREADS) partial[blk * K + k] = s_sum[k];
}

__global__ __launch_bounds__(MBAR_THREADS) void mbar_advance_kernel(const double* __restrict__ partial, int nb, const double* __restrict__ table,
                                                                    int K, int64_t n, int max_iter, double tolerance, double* __restrict__ f,
                                                                    double* __restrict__ record) {
    __shared__ double s_f0;
    __shared__ double s_err[MBAR_WAVES];
    if (bgk_solver_phase(record) == PH_DONE) return;
    const int k = threadIdx.x;                  /* K <= MBAR_THREADS: one thread per window */
    double f_old = 0.0, f_new = 0.0;
    if (k < K) {
        /* block order, 16 loads in flight: the adds wait on each other, the loads need not */
        constexpr int AHEAD = 16;
        const double* src = partial + k;
        double S = 0.0;
        int b = 0;
        for (; b + AHEAD <= nb; b += AHEAD) {
            double v[AHEAD];
#pragma unroll
            for (int i = 0; i < AHEAD; ++i) v[i] = src[(int64_t)(b + i) * K];
#pragma unroll
            for (int i = 0; i < AHEAD; ++i) S += v[i];
        }
        for (; b < nb; ++b) S += src[(int64_t)b * K];
        f_old = f[k];
        f_new = f_old - (log(S) - table[3 * k + 2]);
        if (k == 0) s_f0 = f_new;
    }
    __syncthreads();
    double err = 0.0;                            /* threads past K take no part: |.| >= 0 */
    if (k < K) {
        f_new -= s_f0;
        f[k] = f_new;
        err = __builtin_fabs(f_new - f_old);
    }
    bgk_wave_reduce(err, [](double& a, double b) { a = bgk_nan_max(a, b); });      /* a NaN stays */
    if ((k & (BGK_WAVE - 1)) == 0) s_err[k / BGK_WAVE] = err;
    __syncthreads();
    if (k != 0) return;
    for (int wv = 1; wv < MBAR_WAVES; ++wv) err = bgk_nan_max(err, s_err[wv]);
    double* r = record;
    const double n_iter = r[R_N_ITER] + 1.0;
    r[R_N_ITER] = n_iter;
    r[R_ERR] = err;
    r[R_K] = (double)K;
    r[R_N] = (double)n;
    const int status = err != err ? BGK_ST_NAN : err <= tolerance ? BGK_ST_CONVERGED : n_iter >= (double)max_iter ? BGK_ST_BUDGET : -1;
    if (status >= 0) bgk_solver_finish(r, status, PH_DONE);
}

template <typename T>
__global__ __launch_bounds__(MBAR_THREADS) void mbar_log_weights_kernel(const T* __restrict__ rc, int64_t n, const double* __restrict__ table,
                                                                        int K, const double* __restrict__ f, double* __restrict__ out) {
    __shared__ Windows w;
    windows_load(w, table, f, K);
    __syncthreads();
    const int64_t stride = (int64_t)gridDim.x * MBAR_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * MBAR_THREADS + threadIdx.x; i < n; i += stride) out[i] = -mbar_log_denominator(w, K, (double)rc[i]);
}

/* the checks both entries share; 0 or the error code, text in bgk_last_error */
int mbar_check_common(const char* who, const void* rc, int64_t n, int32_t dtype, const double* table, int32_t K) {
    BGK_CHECK_ARG(n > 0 && K > 0, "%s: bad sizes (n = %lld samples, K = %d windows)", who, (long long)n, (int)K);
    BGK_CHECK_DTYPE(who, dtype);
    BGK_CHECK_ALIGNED(who, bgk_aligned(bgk_dtype_size(dtype), rc) && bgk_aligned(8, table));
    if (K > MBAR_MAX_K) {
        bgk_set_error("%s: K = %d windows is outside the envelope (1 .. %d)", who, (int)K, MBAR_MAX_K);
        return BGK_EUNSUPPORTED;
    }
    BGK_CHECK_ARG(n >= K, "%s: n = %lld samples for K = %d windows (every window holds at least one)", who, (long long)n, (int)K);
    return 0;
}

}  // namespace

extern "C" int bgk_mbar_solve_steps(const void* rc, int64_t n, int32_t dtype, const double* table, int32_t K, int32_t n_blocks, double* partial,
                                    double* f, double* record, int32_t maximum_iterations, double tolerance, int32_t n_steps, void* stream) {
    BGK_CHECK_ARG(rc && table && partial && f && record, "bgk_mbar_solve_steps: null pointer");
    const int bad = mbar_check_common("bgk_mbar_solve_steps", rc, n, dtype, table, K);
    if (bad) return bad;
    BGK_CHECK_ALIGNED("bgk_mbar_solve_steps", bgk_aligned(8, partial, f, record));
    BGK_CHECK_ARG(n_blocks > 0 && n_blocks <= MBAR_MAX_BLOCKS, "bgk_mbar_solve_steps: n_blocks must be in 1 .. %d", MBAR_MAX_BLOCKS);
    BGK_CHECK_ARG(maximum_iterations > 0, "bgk_mbar_solve_steps: maximum_iterations must be positive");
    BGK_CHECK_ARG(tolerance >= 0.0, "bgk_mbar_solve_steps: the tolerance must be a number >= 0");
    BGK_CHECK_ARG(n_steps >= 0, "bgk_mbar_solve_steps: negative n_steps");
    if (n_steps == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const int64_t per = bgk_slice_per(n, n_blocks);
    bgk_dtype_dispatch(dtype, [&](auto elem) {
        typedef decltype(elem) T;
        for (int i = 0; i < n_steps; ++i) {
            hipLaunchKernelGGL(mbar_partial_kernel<T>, dim3(n_blocks), dim3(MBAR_THREADS), 0, st, (const T*)rc, n, per, table, (int)K,
                               (const double*)f, (const double*)record, partial);
            hipLaunchKernelGGL(mbar_advance_kernel, dim3(1), dim3(MBAR_THREADS), 0, st, (const double*)partial, (int)n_blocks, table, (int)K, n,
                               (int)maximum_iterations, tolerance, f, record);
        }
    });
    return bgk_launch_status("bgk_mbar_solve_steps");
}

extern "C" int bgk_mbar_log_weights(const void* rc, int64_t n, int32_t dtype, const double* table, int32_t K, const double* f, double* out,
                                    void* stream) {
    BGK_CHECK_ARG(rc && table && f && out, "bgk_mbar_log_weights: null pointer");
    const int bad = mbar_check_common("bgk_mbar_log_weights", rc, n, dtype, table, K);
    if (bad) return bad;
    BGK_CHECK_ALIGNED("bgk_mbar_log_weights", bgk_aligned(8, f, out));
    hipStream_t st = (hipStream_t)stream;
    const int64_t want = (n + MBAR_THREADS - 1) / MBAR_THREADS;
    const int grid = (int)(want < 65536 ? want : 65536);
    bgk_dtype_dispatch(dtype, [&](auto elem) {
        typedef decltype(elem) T;
        hipLaunchKernelGGL(mbar_log_weights_kernel<T>, dim3(grid), dim3(MBAR_THREADS), 0, st, (const T*)rc, n, table, K, f, out);
    });
    return bgk_launch_status("bgk_mbar_log_weights");
}
