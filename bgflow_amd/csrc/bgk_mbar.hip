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
 * Stage 1 (mbar_partial_kernel): block b takes a fixed contiguous slice of the pooled samples (a multiple of 4 elements, so every slice
 * keeps the array's 16-byte phase), read as in bar_partial_kernel: a scalar head up to the first 16-byte boundary, 16-byte pieces (4 x f32
 * / 2 x f64; piece v belongs to thread v mod 256), a scalar tail.  The block holds c_l = log N_l + f_l, kappa_l, m_l in LDS (every lane
 * reads the same l at the same time: broadcast reads) and walks its slice in tiles of MBAR_TILE samples.  Per tile, (A) each thread forms
 * D_n of its samples in two passes over l (the maximum of a_l = c_l - b_l(r_n), then sum exp(a_l - max)) and leaves r_n, D_n in LDS;
 * (B) the waves split the windows (wave w takes k = w, w + 4, ...), the lanes stride over the tile's samples, merge by shuffles in the
 * fixed order 32 .. 1, and lane 0 adds the tile's sum to the block's S_k in LDS (only this wave touches that k).  One S_k per block and
 * window goes to partial[n_blocks, K].  No atomics and no per-thread array of K accumulators.
 * Stage 2 (mbar_advance_kernel, ONE workgroup): thread k adds the block partials of window k in block order (16 loads in flight; read one
 * by one, each waiting for the add before it, the 512 partials cost as much as stage 1 at K = 32), forms the new f_k, the
 * shift by the new f_0 goes through LDS, err is merged with a maximum that keeps a NaN (shuffles 32 .. 1, then the waves in order), thread
 * 0 advances the record.  Both stages return at once when the record's phase is DONE, so steps enqueued past the end cost two empty
 * launches each.  Nothing waits on another block: the order between stages is stream order.
 *
 * NaN / infinity: a NaN sample gives a NaN D_n, a NaN S_k for every k, a NaN err: status 3.  An infinite sample gives a_l = -inf for
 * every l and exp(-inf - -inf) = NaN: status 3 as well.
 *
 * The iteration is restated in torch ops by bgflow_amd/umbrella.py::_mbar_torch; the two must stay the same, step for step. */
#include "bgk_common.h"

namespace {

enum { PH_ITERATE = 0, PH_DONE = 1 };
enum { ST_CONVERGED = 0, ST_BUDGET = 1, ST_NAN = 3 };
/* the record, BGK_MBAR_RECORD_DOUBLES doubles (include/bgflow_amd.h) */
enum { R_PHASE = 0, R_STATUS, R_N_ITER, R_ERR, R_K, R_N, R_PAD0, R_PAD1, R_COUNT };
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
        mx = (a > mx || a != a) ? a : mx;
    }
    double s = 0.0;
    for (int l = 0; l < K; ++l) {
        const double d = r - w.m[l];
        s += exp((w.c[l] - w.kappa[l] * (d * d)) - mx);
    }
    return mx + log(s);
}

template <typename T> struct Piece;
template <> struct Piece<float> { typedef float4 type; static constexpr int N = 4; };
template <> struct Piece<double> { typedef double2 type; static constexpr int N = 2; };

__device__ __forceinline__ void piece_unpack(const float4& v, double* r) { r[0] = (double)v.x; r[1] = (double)v.y; r[2] = (double)v.z; r[3] = (double)v.w; }
__device__ __forceinline__ void piece_unpack(const double2& v, double* r) { r[0] = v.x; r[1] = v.y; }

template <typename T>
__global__ __launch_bounds__(MBAR_THREADS) void mbar_partial_kernel(const T* __restrict__ rc, int64_t n, int64_t per,
                                                                    const double* __restrict__ table, int K, const double* __restrict__ f,
                                                                    const double* __restrict__ record, double* __restrict__ partial) {
    __shared__ Windows w;
    __shared__ double s_sum[MBAR_MAX_K];
    __shared__ double s_r[MBAR_SLOTS], s_d[MBAR_SLOTS];
    if ((int)record[R_PHASE] == PH_DONE) return;
    const int t = threadIdx.x;
    windows_load(w, table, f, K);
    for (int k = t; k < K; k += MBAR_THREADS) s_sum[k] = 0.0;
    const int64_t blk = blockIdx.x;
    const int64_t i0 = blk * per < n ? blk * per : n;
    const int64_t i1 = (i0 + per) < n ? (i0 + per) : n;
    const T* p = rc + i0;
    const int64_t len = i1 - i0;
    constexpr int N = Piece<T>::N;
    /* scalar head up to the first 16-byte boundary */
    int64_t head = (int64_t)(((16u - (unsigned)((uintptr_t)p & 15u)) & 15u) / sizeof(T));
    head = head < len ? head : len;
    const int64_t body = len - head;           /* 16-byte pieces, then a scalar tail of fewer than N elements in the last tile */
    const typename Piece<T>::type* pv = reinterpret_cast<const typename Piece<T>::type*>(p + head);
    const int wave = t / BGK_WAVE, lane = t & (BGK_WAVE - 1);
    __syncthreads();
    for (int64_t c0 = 0; c0 == 0 || c0 < body; c0 += MBAR_TILE) {
        /* (A) r_n and D_n of the tile's samples into LDS: slot e holds body element c0 + e; the head follows the first tile's body */
        const int clen = (int)((body - c0) < MBAR_TILE ? (body - c0) : MBAR_TILE);
        const int npiece = clen / N;
        for (int v = t; v < npiece; v += MBAR_THREADS) {
            double r[N];
            piece_unpack(pv[c0 / N + v], r);
#pragma unroll
            for (int i = 0; i < N; ++i) {
                s_r[N * v + i] = r[i];
                s_d[N * v + i] = mbar_log_denominator(w, K, r[i]);
            }
        }
        const int done = npiece * N;
        if (t < clen - done) {
            const double r = (double)p[head + c0 + done + t];
            s_r[done + t] = r;
            s_d[done + t] = mbar_log_denominator(w, K, r);
        }
        const int extra = c0 == 0 ? (int)head : 0;
        if (t < extra) {
            const double r = (double)p[t];
            s_r[clen + t] = r;
            s_d[clen + t] = mbar_log_denominator(w, K, r);
        }
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
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, BGK_WAVE);
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
    if ((int)record[R_PHASE] == PH_DONE) return;
    const int k = threadIdx.x;                   /* K <= MBAR_THREADS: one thread per window */
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
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double o = __shfl_down(err, off, BGK_WAVE);
        err = (o > err || o != o) ? o : err;     /* a NaN stays */
    }
    if ((k & (BGK_WAVE - 1)) == 0) s_err[k / BGK_WAVE] = err;
    __syncthreads();
    if (k != 0) return;
    for (int wv = 1; wv < MBAR_WAVES; ++wv) {
        const double o = s_err[wv];
        err = (o > err || o != o) ? o : err;
    }
    double* r = record;
    const double n_iter = r[R_N_ITER] + 1.0;
    r[R_N_ITER] = n_iter;
    r[R_ERR] = err;
    r[R_K] = (double)K;
    r[R_N] = (double)n;
    if (err != err) { r[R_STATUS] = (double)ST_NAN; r[R_PHASE] = (double)PH_DONE; }
    else if (err <= tolerance) { r[R_STATUS] = (double)ST_CONVERGED; r[R_PHASE] = (double)PH_DONE; }
    else if (n_iter >= (double)max_iter) { r[R_STATUS] = (double)ST_BUDGET; r[R_PHASE] = (double)PH_DONE; }
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

template <typename T>
void mbar_enqueue(const void* rc, int64_t n, const double* table, int K, int nb, double* partial, double* f, double* record, int max_iter,
                  double tolerance, int n_steps, hipStream_t st) {
    const int64_t per = ((n + nb - 1) / nb + 3) / 4 * 4;
    for (int i = 0; i < n_steps; ++i) {
        hipLaunchKernelGGL(mbar_partial_kernel<T>, dim3(nb), dim3(MBAR_THREADS), 0, st, (const T*)rc, n, per, table, K, (const double*)f,
                           (const double*)record, partial);
        hipLaunchKernelGGL(mbar_advance_kernel, dim3(1), dim3(MBAR_THREADS), 0, st, (const double*)partial, nb, table, K, n, max_iter,
                           tolerance, f, record);
    }
}

/* the checks both entries share; 0 or the error code, text in bgk_last_error */
int mbar_check_common(const char* who, const void* rc, int64_t n, int32_t dtype, const double* table, int32_t K) {
    BGK_CHECK_ARG(n > 0 && K > 0, "%s: bad sizes (n = %lld samples, K = %d windows)", who, (long long)n, (int)K);
    BGK_CHECK_ARG(dtype == BGK_MBAR_F32 || dtype == BGK_MBAR_F64, "%s: dtype code %d (0 = f32, 1 = f64)", who, (int)dtype);
    const uintptr_t elem = dtype == BGK_MBAR_F32 ? 4 : 8;
    BGK_CHECK_ARG((uintptr_t)rc % elem == 0 && (uintptr_t)table % 8 == 0, "%s: a pointer is not aligned to its element size", who);
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
    BGK_CHECK_ARG((uintptr_t)partial % 8 == 0 && (uintptr_t)f % 8 == 0 && (uintptr_t)record % 8 == 0,
                  "bgk_mbar_solve_steps: a pointer is not aligned to its element size");
    BGK_CHECK_ARG(n_blocks > 0 && n_blocks <= MBAR_MAX_BLOCKS, "bgk_mbar_solve_steps: n_blocks must be in 1 .. %d", MBAR_MAX_BLOCKS);
    BGK_CHECK_ARG(maximum_iterations > 0, "bgk_mbar_solve_steps: maximum_iterations must be positive");
    BGK_CHECK_ARG(tolerance >= 0.0, "bgk_mbar_solve_steps: the tolerance must be a number >= 0");
    BGK_CHECK_ARG(n_steps >= 0, "bgk_mbar_solve_steps: negative n_steps");
    if (n_steps == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    if (dtype == BGK_MBAR_F32)
        mbar_enqueue<float>(rc, n, table, K, n_blocks, partial, f, record, maximum_iterations, tolerance, n_steps, st);
    else
        mbar_enqueue<double>(rc, n, table, K, n_blocks, partial, f, record, maximum_iterations, tolerance, n_steps, st);
    return bgk_launch_status("bgk_mbar_solve_steps");
}

extern "C" int bgk_mbar_log_weights(const void* rc, int64_t n, int32_t dtype, const double* table, int32_t K, const double* f, double* out,
                                    void* stream) {
    BGK_CHECK_ARG(rc && table && f && out, "bgk_mbar_log_weights: null pointer");
    const int bad = mbar_check_common("bgk_mbar_log_weights", rc, n, dtype, table, K);
    if (bad) return bad;
    BGK_CHECK_ARG((uintptr_t)f % 8 == 0 && (uintptr_t)out % 8 == 0, "bgk_mbar_log_weights: a pointer is not aligned to its element size");
    hipStream_t st = (hipStream_t)stream;
    const int64_t want = (n + MBAR_THREADS - 1) / MBAR_THREADS;
    const int grid = (int)(want < 65536 ? want : 65536);
    if (dtype == BGK_MBAR_F32)
        hipLaunchKernelGGL(mbar_log_weights_kernel<float>, dim3(grid), dim3(MBAR_THREADS), 0, st, (const float*)rc, n, table, K, f, out);
    else
        hipLaunchKernelGGL(mbar_log_weights_kernel<double>, dim3(grid), dim3(MBAR_THREADS), 0, st, (const double*)rc, n, table, K, f, out);
    return bgk_launch_status("bgk_mbar_log_weights");
}
