/* bgk_kdyn.hip -- the equivariant kernel dynamics of a particle system x [B, n d] and its fixed-step integration
 *   KernelDynamics.forward (bgflow/nn/flow/dynamics/kernel_dynamic.py:59-116, utils/rbf_kernels.py:134-144, utils/geometry.py:5-48, 93-111):
 *     r_ij = x_i - x_j, d_ij = sqrt(|r_ij|^2 + 1e-6), g_k = exp(-(d - mu_k)^2 exp(nlg_k)^2), s = sum_k g_k, dg_k = -2 (d - mu_k) exp(nlg_k)^2 g_k
 *     kern_k = g_k / (1e-6 + s),  dkern_k = dg_k / (1e-6 + s) - g_k sum(dg) / (1e-6 + s^2)         (the reference's second denominator)
 *     F = sum_k kern_k w_k + c,  dF = sum_k dkern_k w_k;  force_i = sum_{j != i} r_ij F_ij;  divergence = sum_i sum_{j != i} (d_ij dF_ij + n_dims F_ij)
 *   with the time contraction w_k = sum_o W_ko tau_o, c = sum_k importance_k^2 w_k + sum_o b_o tau_o, tau the normalised radial basis
 *   functions of the scalar t -- uniform over the batch, formed by the 64 lanes of every workgroup from the raw parameter tensors (lane k:
 *   w_k; c by a butterfly over the wave: a fixed order) before the pair loop: no extra launch, no host read.
 * By linearity only four sums over k are needed per pair: s, sd = sum dg, A = sum g_k w_k, Bq = sum dg_k w_k:
 *     F = A / (1e-6 + s) + c,  dF = Bq / (1e-6 + s) - A sd / (1e-6 + s^2).
 * The reference materialises [B, n, n - 1, d] distance vectors and [B, n, n - 1, K] kernels and derivatives per evaluation; here a sample is
 * read once, and a whole RK4 / Euler integration (4 Nt or Nt evaluations) keeps the sample's state in LDS: x is read once, y and dlogp are
 * written once.
 *
 * Like bgk_pair.hip, by the rules of bgk_pair_tile.h: one wave per workgroup, a tile of rows staged coalesced through LDS at the odd row
 * stride S, ONE LANE PER SAMPLE, the unordered pairs i < j in ascending order (F_ij = F_ji: half the exponentials of an ordered-pair loop), the contribution to
 * particle i in registers over the j loop and the one to particle j read-modify-written in the lane's own LDS row: no atomics, deterministic.
 * The divergence adds the terms of one i in f32 and the row sums in f64.  exp is the accurate one (dkern is a difference of close terms); when
 * every g_k underflows, s = 0 and A = Bq = 0 give F = c, dF = 0 -- no 0 / 0.
 *
 * Backward of one evaluation (given g_forces, g_div): per unordered pair, with a0 = (gf_i - gf_j) . r, a = a0 + 2 g_div n_dims, b = 2 g_div d:
 *     g_c += a;  g_w[k] += a kern_k + b dkern_k;  v = (gf_i - gf_j) F + (a0 F' + 2 g_div G') r / d,  g_x_i += v, g_x_j -= v
 *   F' = Bq P - A sd P^2 (the derivative of F as computed, P = 1 / (1e-6 + s)), G = d dF + n_dims F, G' = dF + d dF' + n_dims F',
 *   dF' = C P - Bq sd P^2 - (Bq sd + A sdd) Q + 2 A sd^2 s Q^2  (Q = 1 / (1e-6 + s^2), sdd = sum ddg, C = sum ddg_k w_k,
 *   ddg_k = -2 gamma2_k g_k - 2 (d - mu_k) gamma2_k dg_k): derivatives of the formulas above, not of the true divergence.
 *   g_k of a pair is kept in a lane-private LDS row between the pass that forms the sums and the pass that adds to g_w (no second exp).
 *   g_w / g_c: per lane (LDS row / register) over the block's tiles, summed over the lanes in a fixed order into partial [grid, K + 1], finished
 *   in f64 in a fixed order by kdyn_finish_kernel.
 *
 * Envelope: bgk_pair_tile.h's, and K <= 64, O <= 16.  Dynamic LDS <= 63,488 B (64 KiB less the static tables); rows per tile =
 * min(64, 63,488 / bytes per row), lanes beyond the rows only stage, store and take part in the time contraction:
 *   eval       2 S floats per row             n d = 192: 1,544 B, 41 rows      LJ13 (S = 39): 312 B, 64 rows
 *   backward   3 S + 2 (K | 1) floats         n d = 192, K = 64: 2,836 B, 22 rows
 *   integrate  4 S floats (x, stage input, force, RK4 sum)   n d = 192: 3,088 B, 20 rows;  LJ13: 624 B, 64 rows (39,936 B) */
#include "bgk_common.h"
#include "bgk_pair_tile.h"

namespace {

constexpr int KD_MAX_K = 64, KD_MAX_O = 16;
constexpr int KD_LDS_DYNAMIC = 63488;
constexpr int KD_MAX_BWD_GRID = 1024;

/* the per-kernel table of a launch: three float rows (768 B), not float4 (1,024 B) -- with the 64 B of tau the integration's LJ13 tile
 * (39,936 B dynamic) then stays below 40 KiB in all, so that four workgroups fit the 160 KiB of a CU */
struct KdPar { float mu[KD_MAX_K], g2[KD_MAX_K], w[KD_MAX_K]; };

struct KdArgs {
    const float* x; int64_t B;
    int n, nd, K, O, rows; uint32_t magic;
    const float *mus, *nlg, *W, *bias, *imp, *mus_t, *nlg_t;
    double t;
    float* forces; float* div;                                                   /* eval */
    const float* g_forces; const float* g_div; float* g_x; float* partial;      /* backward */
    double t_max; int n_steps, method, inverse; float* y; float* dlogp;         /* integrate */
};

/* all 64 lanes: s_par = (mu_k, exp(nlg_k)^2, w_k(t)) for k < K; returns c(t) in every lane.  Barriers inside: the callers reach it
 * in uniform control flow. */
__device__ float kd_contract(const KdArgs& a, float t, KdPar& s_par, float* s_tau) {
    const int tid = threadIdx.x;
    __syncthreads();                                    /* the readers of the previous tables are done */
    if (tid < a.O) {
        float g = 1.0f;
        if (a.mus_t) {
            const float u = t - a.mus_t[tid], ig = expf(a.nlg_t[tid]);
            g = expf(-(u * u) * (ig * ig));
        }
        s_tau[tid] = g;
    }
    __syncthreads();
    float st = 0.0f;
    for (int o = 0; o < a.O; ++o) st += s_tau[o];
    const float den = 1e-6f + st;
    float w = 0.0f, cterm = 0.0f;
    if (tid < a.K) {
        for (int o = 0; o < a.O; ++o) w += a.W[tid * a.O + o] * (a.mus_t ? s_tau[o] / den : 1.0f);
        const float ig = expf(a.nlg[tid]), im = a.imp[tid];
        s_par.mu[tid] = a.mus[tid]; s_par.g2[tid] = ig * ig; s_par.w[tid] = w;
        cterm = (im * im) * w;
    }
    if (tid < a.O) cterm += a.bias[tid] * (a.mus_t ? s_tau[tid] / den : 1.0f);
    for (int off = 32; off >= 1; off >>= 1) cterm += __shfl_xor(cterm, off, 64);
    __syncthreads();
    return cterm;
}

/* forces of the lane's row xr into fr (LDS, the lane's own row), divergence returned */
template <int D, bool DIV>
__device__ __forceinline__ float kd_eval_row(const float* xr, float* fr, int n, int K, const KdPar& s_par, float c) {
    for (int q = 0; q < n * D; ++q) fr[q] = 0.0f;
    double dv = 0.0;
    for (int i = 0; i + 1 < n; ++i) {
        float xi[D], fi[D];
#pragma unroll
        for (int k = 0; k < D; ++k) { xi[k] = xr[i * D + k]; fi[k] = 0.0f; }
        float drow = 0.0f;
        for (int j = i + 1; j < n; ++j) {
            float r[D], d2 = 0.0f;
#pragma unroll
            for (int k = 0; k < D; ++k) { r[k] = xi[k] - xr[j * D + k]; d2 += r[k] * r[k]; }
            const float d = __builtin_sqrtf(d2 + 1e-6f);
            float s = 0.0f, sd = 0.0f, A = 0.0f, Bq = 0.0f;
            for (int k = 0; k < K; ++k) {
                const float3 p = make_float3(s_par.mu[k], s_par.g2[k], s_par.w[k]);
                const float u = d - p.x;
                const float g = expf(-(u * u) * p.y);
                s += g; A += g * p.z;
                if (DIV) { const float dg = ((-2.0f * u) * p.y) * g; sd += dg; Bq += dg * p.z; }
            }
            const float P = 1.0f / (1e-6f + s);
            const float F = A * P + c;
            if (DIV) {
                const float Q = 1.0f / (1e-6f + s * s);
                const float dF = Bq * P - (A * sd) * Q;
                drow += d * dF + (float)D * F;
            }
#pragma unroll
            for (int k = 0; k < D; ++k) { const float v = r[k] * F; fi[k] += v; fr[j * D + k] -= v; }
        }
#pragma unroll
        for (int k = 0; k < D; ++k) fr[i * D + k] += fi[k];
        dv += (double)drow;
    }
    return (float)(2.0 * dv);
}

template <int D>
__global__ __launch_bounds__(BGK_TILE_THREADS) void kdyn_eval_kernel(KdArgs a) {
    extern __shared__ float s_mem[];
    __shared__ KdPar s_par;
    __shared__ float s_tau[KD_MAX_O];
    const int tid = threadIdx.x, S = a.nd | 1;
    float* s_x = s_mem;
    float* s_f = s_mem + a.rows * S;
    const float c = kd_contract(a, (float)a.t, s_par, s_tau);
    const int64_t n_tiles = (a.B + a.rows - 1) / a.rows;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t b0 = tile * a.rows;
        const int rows = (int)((a.B - b0) < a.rows ? (a.B - b0) : a.rows);
        tile_stage(a.x, b0, rows, a.nd, a.magic, s_x);
        __syncthreads();
        if (tid < rows) {
            if (a.div) a.div[b0 + tid] = kd_eval_row<D, true>(s_x + tid * S, s_f + tid * S, a.n, a.K, s_par, c);
            else kd_eval_row<D, false>(s_x + tid * S, s_f + tid * S, a.n, a.K, s_par, c);
        }
        __syncthreads();
        tile_store(a.forces, b0, rows, a.nd, a.magic, s_f);
        __syncthreads();
    }
}

template <int D>
__global__ __launch_bounds__(BGK_TILE_THREADS) void kdyn_integrate_kernel(KdArgs a) {
    extern __shared__ float s_mem[];
    __shared__ KdPar s_par;
    __shared__ float s_tau[KD_MAX_O];
    const int tid = threadIdx.x, S = a.nd | 1, nd = a.nd;
    float* xr = s_mem + tid * S;                        /* the state */
    float* xs = s_mem + (a.rows + tid) * S;             /* the input of stages 2..4 */
    float* fr = s_mem + (2 * a.rows + tid) * S;         /* a stage's forces */
    float* ac = s_mem + (3 * a.rows + tid) * S;         /* k1 + 2 k2 + 2 k3 + k4 */
    const double h = a.t_max / (double)a.n_steps;
    const float hf = (float)h, hh = (float)(0.5 * h), h6 = (float)(h / 6.0), sg = a.inverse ? -1.0f : 1.0f;
    const int n_stages = a.method == 0 ? 4 : 1;
    const int64_t n_tiles = (a.B + a.rows - 1) / a.rows;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t b0 = tile * a.rows;
        const int rows = (int)((a.B - b0) < a.rows ? (a.B - b0) : a.rows);
        tile_stage(a.x, b0, rows, nd, a.magic, s_mem);
        float lp = 0.0f, lacc = 0.0f;
        for (int step = 0; step < a.n_steps; ++step) {
            for (int st = 0; st < n_stages; ++st) {
                const double ts = (double)step * h + (st == 0 ? 0.0 : (st == 3 ? h : 0.5 * h));
                const float c = kd_contract(a, (float)(a.inverse ? a.t_max - ts : ts), s_par, s_tau);   /* its barriers also order the staging */
                if (tid < rows) {
                    const float dv = sg * kd_eval_row<D, true>(st == 0 ? xr : xs, fr, a.n, a.K, s_par, c);
                    if (a.method != 0) {
                        for (int q = 0; q < nd; ++q) xr[q] += hf * (sg * fr[q]);
                        lp += hf * dv;
                    } else if (st == 0) {
                        for (int q = 0; q < nd; ++q) { const float f = sg * fr[q]; ac[q] = f; xs[q] = xr[q] + hh * f; }
                        lacc = dv;
                    } else if (st < 3) {
                        const float hs = st == 1 ? hh : hf;
                        for (int q = 0; q < nd; ++q) { const float f = sg * fr[q]; ac[q] += 2.0f * f; xs[q] = xr[q] + hs * f; }
                        lacc += 2.0f * dv;
                    } else {
                        for (int q = 0; q < nd; ++q) xr[q] += h6 * (ac[q] + sg * fr[q]);
                        lp += h6 * (lacc + dv);
                    }
                }
            }
        }
        if (tid < rows) a.dlogp[b0 + tid] = lp;
        __syncthreads();
        tile_store(a.y, b0, rows, nd, a.magic, s_mem);
        __syncthreads();
    }
}

template <int D>
__global__ __launch_bounds__(BGK_TILE_THREADS) void kdyn_eval_bwd_kernel(KdArgs a) {
    extern __shared__ float s_mem[];
    __shared__ KdPar s_par;
    __shared__ float s_tau[KD_MAX_O];
    __shared__ float s_red[BGK_TILE_THREADS];
    const int tid = threadIdx.x, S = a.nd | 1, K = a.K, KS = a.K | 1, n = a.n;
    float* s_x = s_mem;
    float* s_gf = s_x + a.rows * S;
    float* s_gx = s_gf + a.rows * S;
    float* s_gw = s_gx + a.rows * S;                    /* [rows][KS] the lane's sum of g_w over its samples */
    float* s_gk = s_gw + a.rows * KS;                   /* [rows][KS] g_k of the pair at hand */
    const float c = kd_contract(a, (float)a.t, s_par, s_tau);
    if (tid < a.rows) for (int k = 0; k < K; ++k) s_gw[tid * KS + k] = 0.0f;
    double gc = 0.0;
    const int64_t n_tiles = (a.B + a.rows - 1) / a.rows;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t b0 = tile * a.rows;
        const int rows = (int)((a.B - b0) < a.rows ? (a.B - b0) : a.rows);
        tile_stage(a.x, b0, rows, a.nd, a.magic, s_x);
        tile_stage(a.g_forces, b0, rows, a.nd, a.magic, s_gf);
        __syncthreads();
        if (tid < rows) {
            const float* xr = s_x + tid * S;
            const float* gf = s_gf + tid * S;
            float* gx = s_gx + tid * S;
            float* gw = s_gw + tid * KS;
            float* gk = s_gk + tid * KS;
            const float gd2 = a.g_div ? 2.0f * a.g_div[b0 + tid] : 0.0f;
            for (int q = 0; q < n * D; ++q) gx[q] = 0.0f;
            for (int i = 0; i + 1 < n; ++i) {
                float xi[D], gfi[D], gi[D];
#pragma unroll
                for (int k = 0; k < D; ++k) { xi[k] = xr[i * D + k]; gfi[k] = gf[i * D + k]; gi[k] = 0.0f; }
                float crow = 0.0f;
                for (int j = i + 1; j < n; ++j) {
                    float r[D], dg_[D], d2 = 0.0f, a0 = 0.0f;
#pragma unroll
                    for (int k = 0; k < D; ++k) {
                        r[k] = xi[k] - xr[j * D + k]; d2 += r[k] * r[k];
                        dg_[k] = gfi[k] - gf[j * D + k]; a0 += dg_[k] * r[k];
                    }
                    const float d = __builtin_sqrtf(d2 + 1e-6f);
                    float s = 0.0f, sd = 0.0f, sdd = 0.0f, A = 0.0f, Bq = 0.0f, C = 0.0f;
                    for (int k = 0; k < K; ++k) {
                        const float3 p = make_float3(s_par.mu[k], s_par.g2[k], s_par.w[k]);
                        const float u = d - p.x, m2 = (-2.0f * u) * p.y;
                        const float g = expf(-(u * u) * p.y);
                        const float dg = m2 * g, ddg = (-2.0f * p.y) * g + m2 * dg;
                        gk[k] = g;
                        s += g; sd += dg; sdd += ddg; A += g * p.z; Bq += dg * p.z; C += ddg * p.z;
                    }
                    const float P = 1.0f / (1e-6f + s), Q = 1.0f / (1e-6f + s * s);
                    const float F = A * P + c;
                    const float Fp = Bq * P - ((A * sd) * P) * P;
                    const float dF = Bq * P - (A * sd) * Q;
                    const float dFp = C * P - ((Bq * sd) * P) * P - (Bq * sd + A * sdd) * Q + (((2.0f * A) * (sd * sd)) * s) * (Q * Q);
                    const float Gp = dF + d * dFp + (float)D * Fp;
                    const float aa = a0 + gd2 * (float)D, bb = gd2 * d;
                    crow += aa;
                    const float m = (a0 * Fp + gd2 * Gp) / d;
#pragma unroll
                    for (int k = 0; k < D; ++k) { const float v = dg_[k] * F + m * r[k]; gi[k] += v; gx[j * D + k] -= v; }
                    const float c1 = aa * P - (bb * sd) * Q, c2 = bb * P;
                    for (int k = 0; k < K; ++k) {
                        const float3 p = make_float3(s_par.mu[k], s_par.g2[k], s_par.w[k]);
                        gw[k] += gk[k] * (c1 + c2 * ((-2.0f * (d - p.x)) * p.y));
                    }
                }
#pragma unroll
                for (int k = 0; k < D; ++k) gx[i * D + k] += gi[k];
                gc += (double)crow;
            }
        }
        __syncthreads();
        tile_store(a.g_x, b0, rows, a.nd, a.magic, s_gx);
        __syncthreads();
    }
    /* block partials in a fixed order over the lanes */
    s_red[tid] = (float)gc;
    __syncthreads();
    float* out = a.partial + (int64_t)blockIdx.x * (K + 1);
    if (tid < K) {
        float v = 0.0f;
        for (int l = 0; l < a.rows; ++l) v += s_gw[l * KS + tid];
        out[tid] = v;
    }
    if (tid == BGK_TILE_THREADS - 1) {
        float v = 0.0f;
        for (int l = 0; l < BGK_TILE_THREADS; ++l) v += s_red[l];
        out[K] = v;
    }
}

/* out[k] = sum over the blocks' partials [nblk, K + 1] in f64, a fixed order: block k of the grid, 64 strided sums, then lane 0 */
__global__ __launch_bounds__(BGK_TILE_THREADS) void kdyn_finish_kernel(const float* partial, int nblk, int K1, float* out) {
    __shared__ double s_sum[BGK_TILE_THREADS];
    const int k = blockIdx.x;
    double v = 0.0;
    for (int b = threadIdx.x; b < nblk; b += BGK_TILE_THREADS) v += (double)partial[(int64_t)b * K1 + k];
    s_sum[threadIdx.x] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int l = 0; l < BGK_TILE_THREADS; ++l) t += s_sum[l];
        out[k] = (float)t;
    }
}

struct BgkKdynCall {
    const char* what;
    const float* x; int64_t B; int32_t n_particles, n_dims, n_kernels, n_out;
    const float *mus, *neg_log_gammas, *weights, *bias, *importance, *mus_time, *neg_log_gammas_time;
    int floats_per_row;                                 /* of dynamic LDS */
};

int kd_common(const BgkKdynCall& c, KdArgs* a) {
    BGK_CHECK_ARG(c.B >= 0, "%s: bad batch size", c.what);
    if (!(c.n_particles >= 2 && c.n_particles <= BGK_TILE_MAX_N && c.n_dims >= 1 && c.n_dims <= BGK_TILE_MAX_D && c.n_kernels >= 1 &&
          c.n_kernels <= KD_MAX_K && c.n_out >= 1 && c.n_out <= KD_MAX_O)) {
        bgk_set_error("%s: %d particles in %d dimensions with %d distance and %d time kernels are outside the kernel's envelope "
                      "(2..%d particles, 1..%d dimensions, 1..%d and 1..%d kernels)", c.what, c.n_particles, c.n_dims, c.n_kernels, c.n_out,
                      BGK_TILE_MAX_N, BGK_TILE_MAX_D, KD_MAX_K, KD_MAX_O);
        return BGK_EUNSUPPORTED;
    }
    BGK_CHECK_ARG(c.mus && c.neg_log_gammas && c.weights && c.bias && c.importance, "%s: null parameter tensor", c.what);
    BGK_CHECK_ARG((c.mus_time != nullptr) == (c.neg_log_gammas_time != nullptr), "%s: mus_time and neg_log_gammas_time go together", c.what);
    BGK_CHECK_ARG(c.mus_time || c.n_out == 1, "%s: without time kernels n_out is 1", c.what);
    a->x = c.x; a->B = c.B; a->n = c.n_particles; a->nd = c.n_particles * c.n_dims; a->K = c.n_kernels; a->O = c.n_out;
    a->magic = tile_magic(a->nd);
    a->mus = c.mus; a->nlg = c.neg_log_gammas; a->W = c.weights; a->bias = c.bias; a->imp = c.importance;
    a->mus_t = c.mus_time; a->nlg_t = c.neg_log_gammas_time;
    a->rows = rows_within(KD_LDS_DYNAMIC, c.floats_per_row * (int)sizeof(float));
    return 0;
}

}  // namespace

extern "C" int bgk_kdyn_eval(const float* x, int64_t B, int32_t n_particles, int32_t n_dims, int32_t n_kernels, int32_t n_out,
                             const float* mus, const float* neg_log_gammas, const float* weights, const float* bias,
                             const float* importance, const float* mus_time, const float* neg_log_gammas_time, double t,
                             float* forces, float* divergence, void* stream) {
    BgkKdynCall c{"bgk_kdyn_eval", x, B, n_particles, n_dims, n_kernels, n_out, mus, neg_log_gammas, weights, bias, importance,
                  mus_time, neg_log_gammas_time, 2 * ((n_particles * n_dims) | 1)};
    KdArgs a{};
    const int st = kd_common(c, &a);
    if (st) return st;
    if (B == 0) return 0;
    BGK_CHECK_ARG(x && forces, "bgk_kdyn_eval: null tensor");
    a.t = t; a.forces = forces; a.div = divergence;
    const size_t lds = (size_t)a.rows * c.floats_per_row * sizeof(float);
    tile_dispatch_d(n_dims, [&](auto D) { tile_launch(kdyn_eval_kernel<D()>, tile_grid(B, a.rows), lds, (hipStream_t)stream, a); });
    return bgk_launch_status(c.what);
}

extern "C" int bgk_kdyn_eval_backward(const float* x, int64_t B, int32_t n_particles, int32_t n_dims, int32_t n_kernels, int32_t n_out,
                                      const float* mus, const float* neg_log_gammas, const float* weights, const float* bias,
                                      const float* importance, const float* mus_time, const float* neg_log_gammas_time, double t,
                                      const float* g_forces, const float* g_div, float* g_x, float* partial, int32_t nblk,
                                      float* g_wc, void* stream) {
    BgkKdynCall c{"bgk_kdyn_eval_backward", x, B, n_particles, n_dims, n_kernels, n_out, mus, neg_log_gammas, weights, bias, importance,
                  mus_time, neg_log_gammas_time, 3 * ((n_particles * n_dims) | 1) + 2 * (n_kernels | 1)};
    KdArgs a{};
    const int st = kd_common(c, &a);
    if (st) return st;
    BGK_CHECK_ARG(g_wc && partial && nblk >= 1, "bgk_kdyn_eval_backward: need g_wc [n_kernels + 1] and a [nblk, n_kernels + 1] workspace");
    hipStream_t s = (hipStream_t)stream;
    if (B == 0) {
        hipError_t e = hipMemsetAsync(g_wc, 0, (size_t)(n_kernels + 1) * sizeof(float), s);
        return e == hipSuccess ? 0 : (int)e;
    }
    BGK_CHECK_ARG(x && g_forces && g_x, "bgk_kdyn_eval_backward: null tensor");
    a.t = t; a.g_forces = g_forces; a.g_div = g_div; a.g_x = g_x; a.partial = partial;
    const size_t lds = (size_t)a.rows * c.floats_per_row * sizeof(float);
    const int grid = tile_grid(B, a.rows, nblk < KD_MAX_BWD_GRID ? nblk : KD_MAX_BWD_GRID);
    tile_dispatch_d(n_dims, [&](auto D) { tile_launch(kdyn_eval_bwd_kernel<D()>, grid, lds, s, a); });
    const int st2 = bgk_launch_status(c.what);
    if (st2) return st2;
    hipLaunchKernelGGL(kdyn_finish_kernel, dim3(n_kernels + 1), dim3(BGK_TILE_THREADS), 0, s, partial, grid, n_kernels + 1, g_wc);
    return bgk_launch_status(c.what);
}

extern "C" int bgk_kdyn_integrate(const float* x, int64_t B, int32_t n_particles, int32_t n_dims, int32_t n_kernels, int32_t n_out,
                                  const float* mus, const float* neg_log_gammas, const float* weights, const float* bias,
                                  const float* importance, const float* mus_time, const float* neg_log_gammas_time, double t_max,
                                  int32_t n_steps, int32_t method, int32_t inverse, float* y, float* dlogp, void* stream) {
    BgkKdynCall c{"bgk_kdyn_integrate", x, B, n_particles, n_dims, n_kernels, n_out, mus, neg_log_gammas, weights, bias, importance,
                  mus_time, neg_log_gammas_time, 4 * ((n_particles * n_dims) | 1)};
    KdArgs a{};
    const int st = kd_common(c, &a);
    if (st) return st;
    BGK_CHECK_ARG(n_steps >= 1 && (method == 0 || method == 1), "bgk_kdyn_integrate: n_steps %d, method %d (0 RK4, 1 Euler)", n_steps, method);
    if (B == 0) return 0;
    BGK_CHECK_ARG(x && y && dlogp, "bgk_kdyn_integrate: null tensor");
    a.t_max = t_max; a.n_steps = n_steps; a.method = method; a.inverse = inverse != 0; a.y = y; a.dlogp = dlogp;
    const size_t lds = (size_t)a.rows * c.floats_per_row * sizeof(float);
    tile_dispatch_d(n_dims, [&](auto D) { tile_launch(kdyn_integrate_kernel<D()>, tile_grid(B, a.rows), lds, (hipStream_t)stream, a); });
    return bgk_launch_status(c.what);
}
