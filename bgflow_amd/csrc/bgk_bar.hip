/* bgk_bar.hip -- the Bennett acceptance ratio (utils/free_energy.py:104-197) as a deterministic two-stage reduction whose second
 * stage also advances the root finder, so that one evaluation of
 *
 *     f(D) = log sum_i fermi(M + wF_i - D) - log sum_j fermi(wR_j + D - M),   fermi(a) = 1 / (1 + e^a),   M = log(nF / nR)
 *
 * is two launches and no host read (the reference: ~30 torch ops per evaluation and two scalar reads per iteration of its loop).
 * Roofline: every evaluation reads both work arrays once (4 or 8 B per element, L2 / Infinity-Cache resident after the first pass at the
 * sizes in question) and spends three f64 transcendentals per element; at 2^20 elements a stage-1 launch is of the order of its
 * own launch latency, so the solve is bound by 2 launches x (5 .. 25) evaluations, not by bytes or flops.
 *
 * Stage 1 (bar_partial_kernel): blocks [0, nbf) take the forward work, [nbf, nbf + nbr) the reverse work, each one slice of bgk_reduce.h
 * (head, 16-byte pieces, tail; piece v belongs to thread v mod 256).  Per element, in f64: a = w + c with c = M - D (forward) or D - M
 * (reverse), D read from the device record; lf = -softplus(a) = -(max(a, 0) + log1p(exp(-|a|))) = log fermi(a); the thread keeps the online
 * log-sum-exp triple (m, s1 = sum e^(lf - m), s2 = sum e^(2 (lf - m))) under one running maximum m.  While the record's phase is BOUNDS the
 * element is lf = -w instead (s2 is carried along, unused): the one-sided exponential averages.  Lanes, then waves, merge in the orders of
 * bgk_reduce.h; one triple per block.  No atomics; the partition and every merge order are fixed by (pointer alignment, n, block counts).
 * Stage 2 (bar_advance_kernel, ONE workgroup): thread t merges a fixed run of block triples of its array (t < 128 forward, else reverse) in
 * block order, waves merge as in stage 1, thread 0 forms log sum F, log sum F^2, log sum R, log sum R^2 and advances the solver's state in
 * the record, including the D the next stage 1 reads.  The record protocol is bgk_reduce.h's: steps enqueued past the end cost two empty
 * launches each.
 *
 * NaN / infinity: torch.logsumexp's.  The running maximum keeps a NaN (bgk_nan_above) and a NaN maximum poisons s1; an element equal to the
 * maximum counts e^0 = 1 without forming inf - inf, so all -inf gives -inf and a +inf gives +inf; inf - inf inside a is a NaN that reaches
 * f.
 *
 * The state machine (phases BOUNDS -> F_UPPER <-> F_LOWER -> ITERATE -> DONE) is restated in torch ops by
 * bgflow_amd/free_energy.py::_solve_torch; the two must stay the same, step for step. */
#include "bgk_reduce.h"

namespace {

enum { PH_BOUNDS = 0, PH_F_UPPER = 1, PH_F_LOWER = 2, PH_ITERATE = 3, PH_DONE = 4 };
/* the record, BGK_BAR_RECORD_DOUBLES doubles (include/bgflow_amd.h) */
enum { R_PHASE = BGK_R_PHASE, R_STATUS = BGK_R_STATUS, R_UPPER, R_LOWER, R_F_UPPER, R_F_LOWER, R_DELTA, R_DELTA_OLD, R_N_EVAL, R_N_EXPAND, R_N_ITER,
       R_L1F, R_L2F, R_L1R, R_L2R, R_RESIDUAL, R_RESULT, R_UNCERTAINTY, R_COUNT };
static_assert(R_COUNT == BGK_BAR_RECORD_DOUBLES, "record layout");

constexpr int BAR_THREADS = 256;
constexpr int BAR_MAX_BLOCKS = 512;        /* per array */

struct Lse {
    double m, s1, s2;
};

__device__ __forceinline__ Lse lse_empty() { return Lse{-__builtin_inf(), 0.0, 0.0}; }
__device__ __forceinline__ Lse lse_one(double v) { return Lse{v, 1.0, 1.0}; }        /* one element: e^0 and e^(2 0) under its own maximum */

/* a <- a merged with b (a first); b.m above a.m: a new maximum (or a NaN: it stays), and a.m = -inf gives sc = 0 */
__device__ __forceinline__ void lse_merge(Lse& a, const Lse& b) {
    if (bgk_nan_above(b.m, a.m)) {
        const double sc = exp(a.m - b.m);
        a.s1 = a.s1 * sc + b.s1;
        a.s2 = a.s2 * (sc * sc) + b.s2;
        a.m = b.m;
    } else {
        const double sc = (b.m == a.m) ? 1.0 : exp(b.m - a.m);
        a.s1 = a.s1 + b.s1 * sc;
        a.s2 = a.s2 + b.s2 * (sc * sc);
    }
}

__device__ __forceinline__ Lse bgk_shfl_down(const Lse& a, int off) { return Lse{::bgk_shfl_down(a.m, off), ::bgk_shfl_down(a.s1, off), ::bgk_shfl_down(a.s2, off)}; }

/* log fermi(w + c), or -w for the one-sided bounds */
__device__ __forceinline__ double bar_element(double w, double c, bool bounds) {
    if (bounds) return -w;
    const double a = w + c;
    const double p = a > 0.0 ? a : 0.0;
    return -(p + log1p(exp(-__builtin_fabs(a))));        /* a NaN: p = 0, the log1p term is NaN */
}

template <typename T>
__global__ __launch_bounds__(BAR_THREADS) void bar_partial_kernel(const T* __restrict__ wf, int64_t nf, const T* __restrict__ wr, int64_t nr,
                                                                  int nbf, int64_t per_f, int64_t per_r, double log_ratio,
                                                                  const double* __restrict__ record, double* __restrict__ partial) {
    __shared__ double s[3][BAR_THREADS / BGK_WAVE];
    const int phase = bgk_solver_phase(record);
    if (phase == PH_DONE) return;
    const bool bounds = phase == PH_BOUNDS;
    const double delta = record[R_DELTA];
    const int t = threadIdx.x;
    const bool fwd = (int)blockIdx.x < nbf;
    const int64_t blk = fwd ? blockIdx.x : (int64_t)blockIdx.x - nbf;
    const int64_t n = fwd ? nf : nr, per = fwd ? per_f : per_r;
    const double c = fwd ? log_ratio - delta : delta - log_ratio;
    const BgkSlice<T> sl(fwd ? wf : wr, n, per, blk);
    constexpr int N = BgkPiece<T>::N;
    Lse acc = lse_empty();
    if (t < sl.head) lse_merge(acc, lse_one(bar_element((double)sl.p[t], c, bounds)));
    const int64_t npiece = sl.body / N;
    for (int64_t v = t; v < npiece; v += BAR_THREADS)
        bgk_piece_each(sl.pv[v], [&](double w) { lse_merge(acc, lse_one(bar_element(w, c, bounds))); });
    const int64_t done = sl.head + npiece * N;
    if (t < sl.len - done) lse_merge(acc, lse_one(bar_element((double)sl.p[done + t], c, bounds)));
    bgk_wave_reduce(acc, lse_merge);
    const int wave = t / BGK_WAVE;
    if ((t & (BGK_WAVE - 1)) == 0) { s[0][wave] = acc.m; s[1][wave] = acc.s1; s[2][wave] = acc.s2; }
    __syncthreads();
    if (t == 0) {
        Lse r = Lse{s[0][0], s[1][0], s[2][0]};
        for (int w = 1; w < BAR_THREADS / BGK_WAVE; ++w) lse_merge(r, Lse{s[0][w], s[1][w], s[2][w]});
        double* out = partial + 3 * (int64_t)blockIdx.x;
        out[0] = r.m; out[1] = r.s1; out[2] = r.s2;
    }
}

__device__ __forceinline__ double bar_clamp(double x) { return x < 0.1 ? 0.1 : (x > 1e10 ? 1e10 : x); }      /* a NaN stays */

__device__ __forceinline__ void bar_finish(double* r, int status, double delta, double residual, double nrat) {
    const bool number = status == BGK_ST_CONVERGED || status == BGK_ST_BUDGET;
    const double nan = __builtin_nan("");
    const double var = exp(r[R_L2F] - 2.0 * r[R_L1F]) + exp(r[R_L2R] - 2.0 * r[R_L1R]) - nrat;
    r[R_RESULT] = number ? delta : nan;
    r[R_UNCERTAINTY] = number ? __builtin_sqrt(var) : nan;
    r[R_RESIDUAL] = number ? residual : nan;
    bgk_solver_finish(r, status, PH_DONE);
}

__global__ __launch_bounds__(BAR_THREADS) void bar_advance_kernel(const double* __restrict__ partial, int nbf, int nbr, double log_nf,
                                                                  double log_nr, double nrat, int max_iter, double rtol,
                                                                  double* __restrict__ record) {
    __shared__ double s[3][BAR_THREADS / BGK_WAVE];
    const int phase = bgk_solver_phase(record);
    if (phase == PH_DONE) return;
    const int t = threadIdx.x;
    constexpr int HALF = BAR_THREADS / 2;
    const bool fwd = t < HALF;
    const int j = fwd ? t : t - HALF;
    const int nb = fwd ? nbf : nbr;
    const int run = (nb + HALF - 1) / HALF;
    const int b0 = j * run < nb ? j * run : nb, b1 = (b0 + run) < nb ? (b0 + run) : nb;
    const double* src = partial + 3 * (int64_t)(fwd ? 0 : nbf);
    Lse acc = lse_empty();
    for (int b = b0; b < b1; ++b) lse_merge(acc, Lse{src[3 * b], src[3 * b + 1], src[3 * b + 2]});
    bgk_wave_reduce(acc, lse_merge);
    const int wave = t / BGK_WAVE;
    if ((t & (BGK_WAVE - 1)) == 0) { s[0][wave] = acc.m; s[1][wave] = acc.s1; s[2][wave] = acc.s2; }
    __syncthreads();
    if (t != 0) return;
    Lse F = Lse{s[0][0], s[1][0], s[2][0]}, R = Lse{s[0][2], s[1][2], s[2][2]};
    lse_merge(F, Lse{s[0][1], s[1][1], s[2][1]});
    lse_merge(R, Lse{s[0][3], s[1][3], s[2][3]});
    const double l1f = F.m + log(F.s1), l1r = R.m + log(R.s1);
    double* r = record;
    if (phase == PH_BOUNDS) {              /* upper = -(LSE(-wF) - log nF), lower = LSE(-wR) - log nR  (:125-138) */
        const double upper = -(l1f - log_nf), lower = l1r - log_nr;
        r[R_UPPER] = upper; r[R_LOWER] = lower;
        r[R_DELTA] = upper;
        r[R_PHASE] = (double)PH_F_UPPER;
        return;
    }
    const double f = l1f - l1r;
    r[R_L1F] = l1f; r[R_L2F] = 2.0 * F.m + log(F.s2);
    r[R_L1R] = l1r; r[R_L2R] = 2.0 * R.m + log(R.s2);
    r[R_RESIDUAL] = f;
    r[R_N_EVAL] += 1.0;
    double upper = r[R_UPPER], lower = r[R_LOWER], f_upper = r[R_F_UPPER], f_lower = r[R_F_LOWER];
    if (phase == PH_F_UPPER) {
        r[R_F_UPPER] = f;
        r[R_DELTA] = lower;
        r[R_PHASE] = (double)PH_F_LOWER;
        return;
    }
    if (phase == PH_F_LOWER) {
        f_lower = f;
        r[R_F_LOWER] = f;
        if (f_upper * f_lower > 0.0) {     /* no sign change: widen the bracket (:142-147) */
            if (r[R_N_EXPAND] >= (double)max_iter) { bar_finish(r, BGK_ST_NO_ROOT, 0.0, 0.0, nrat); return; }
            const double average = (upper + lower) / 2.0;
            upper = upper - bar_clamp(__builtin_fabs(upper - average));
            lower = lower + bar_clamp(__builtin_fabs(lower - average));
            r[R_UPPER] = upper; r[R_LOWER] = lower;
            r[R_N_EXPAND] += 1.0;
            r[R_DELTA] = upper;
            r[R_PHASE] = (double)PH_F_UPPER;
            return;
        }
        r[R_DELTA_OLD] = __builtin_inf();
        r[R_DELTA] = upper - f_upper * (upper - lower) / (f_upper - f_lower);
        r[R_PHASE] = (double)PH_ITERATE;
        return;
    }
    /* PH_ITERATE: false position (:151-161) */
    const double delta = r[R_DELTA], delta_old = r[R_DELTA_OLD];
    if (f_upper * f < 0.0) { lower = delta; f_lower = f; }
    else if (f_lower * f <= 0.0) { upper = delta; f_upper = f; }
    else { bar_finish(r, BGK_ST_NAN, 0.0, 0.0, nrat); return; }
    r[R_UPPER] = upper; r[R_LOWER] = lower; r[R_F_UPPER] = f_upper; r[R_F_LOWER] = f_lower;
    const double n_iter = r[R_N_ITER] + 1.0;
    r[R_N_ITER] = n_iter;
    if (f == 0.0 || delta == delta_old || __builtin_fabs(delta - delta_old) <= rtol * __builtin_fabs(delta)) {
        bar_finish(r, BGK_ST_CONVERGED, delta, f, nrat);
        return;
    }
    if (n_iter >= (double)max_iter) { bar_finish(r, BGK_ST_BUDGET, delta, f, nrat); return; }
    r[R_DELTA_OLD] = delta;
    r[R_DELTA] = upper - f_upper * (upper - lower) / (f_upper - f_lower);
}

}  // namespace

extern "C" int bgk_bar_solve_steps(const void* forward_work, int64_t n_forward, const void* reverse_work, int64_t n_reverse, int32_t dtype,
                                   int32_t nblk_forward, int32_t nblk_reverse, double* partial, double* record,
                                   int32_t maximum_iterations, double relative_tolerance, int32_t n_steps, void* stream) {
    BGK_CHECK_ARG(forward_work && reverse_work && partial && record, "bgk_bar_solve_steps: null pointer");
    BGK_CHECK_ARG(n_forward > 0 && n_reverse > 0, "bgk_bar_solve_steps: bad sizes (both work arrays need at least one value)");
    BGK_CHECK_DTYPE("bgk_bar_solve_steps", dtype);
    BGK_CHECK_ALIGNED("bgk_bar_solve_steps", bgk_aligned(bgk_dtype_size(dtype), forward_work, reverse_work) && bgk_aligned(8, partial, record));
    BGK_CHECK_ARG(nblk_forward > 0 && nblk_forward <= BAR_MAX_BLOCKS && nblk_reverse > 0 && nblk_reverse <= BAR_MAX_BLOCKS,
                  "bgk_bar_solve_steps: block counts must be in 1 .. %d", BAR_MAX_BLOCKS);
    BGK_CHECK_ARG(maximum_iterations > 0, "bgk_bar_solve_steps: maximum_iterations must be positive");
    BGK_CHECK_ARG(n_steps >= 0, "bgk_bar_solve_steps: negative n_steps");
    if (n_steps == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const int nbf = nblk_forward, nbr = nblk_reverse;
    const int64_t per_f = bgk_slice_per(n_forward, nbf), per_r = bgk_slice_per(n_reverse, nbr);
    const double dnf = (double)n_forward, dnr = (double)n_reverse;
    const double log_ratio = log(dnf / dnr), log_nf = log(dnf), log_nr = log(dnr), nrat = (dnf + dnr) / (dnf * dnr);
    bgk_dtype_dispatch(dtype, [&](auto elem) {
        typedef decltype(elem) T;
        for (int i = 0; i < n_steps; ++i) {
            hipLaunchKernelGGL(bar_partial_kernel<T>, dim3(nbf + nbr), dim3(BAR_THREADS), 0, st, (const T*)forward_work, n_forward,
                               (const T*)reverse_work, n_reverse, nbf, per_f, per_r, log_ratio, (const double*)record, partial);
            hipLaunchKernelGGL(bar_advance_kernel, dim3(1), dim3(BAR_THREADS), 0, st, (const double*)partial, nbf, nbr, log_nf, log_nr, nrat,
                               (int)maximum_iterations, relative_tolerance, record);
        }
    });
    return bgk_launch_status("bgk_bar_solve_steps");
}
