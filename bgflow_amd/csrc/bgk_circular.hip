/* bgk_circular.hip -- the circular bump-mixture bijection of [0, 1] (bgflow/nn/flow/circular.py: _cdf_transform, about 40 torch ops
 * per call, and _bisect, that chain once per step) as ONE launch forward, ONE launch inverse and ONE launch backward.
 *
 * Raw conditioner outputs: mu_raw, log_sigma, log_weight [B, K D] (k major; row pitch `param_pitch`, 0 = one row shared by the batch),
 * log_eps [B, D] (row pitch `eps_pitch`, 0 likewise).  Per element (b, j) and component k, in f32:
 *   mu = 0.5 sin(mu_raw) + 0.5    sigma = 1 + exp(log_sigma)    e = exp(log_weight - max_k log_weight), w = e / sum_k e
 *   eps = 1 / (1 + exp(-log_eps)),  1 - eps = exp(-log_eps) / (1 + exp(-log_eps))
 *   u = y - mu;  hi = mu > 0.5;  wrapped = hi ? u < -0.5 : u > 0.5;  s = wrapped ? (hi ? u + 1 : u - 1) : u;  off = wrapped != hi
 *   s0 = hi ? 1 - mu : -mu
 *   bump(z): z clamped to [0, 1]; a = z^3, b = (1 - z)^3; cdf = a / (a + b); pdf = 3 (z (1 - z) / (a + b))^2;
 *            pdf' = 6 z (1 - z) (1 - 2 z) / (a + b)^3                                   (a + b lies in [1/4, 1])
 *   c, p, p' = bump(sigma s + 0.5);  c0, p0 = bump(sigma s0 + 0.5)
 *   F = (sum_k e ((c - c0) + off)) / sum_k e     f = (sum_k e sigma p) / sum_k e     f' = (sum_k e sigma^2 p') / sum_k e   (ascending k)
 *   out = F (1 - eps) + y eps     L = log(f (1 - eps) + eps)     dlogp[b] = sum_j L (ascending j)
 * The wrap and the offset are ONE decision taken from u: a y within rounding of the seam mu -+ 0.5 gets either (c = 1, off = 0) or
 * (c = 0, off = 1), never neither -- the reference's strict `x > mu - 0.5` next to torch.min's first-of-equals loses a component's whole
 * weight there (DESIGN.md "Circular bump mixture", deviation 2).  The clamp of z keeps log_sigma = 40 finite (deviation 1).
 *
 * Layout (after bgk_affine.hip): a 256-thread workgroup owns a tile of consecutive rows, about 2048 elements; the elements (r, j) of
 * the tile are one flat stream, so the loads of [k D + j] are coalesced across j.  L goes through LDS and ONE lane per row adds it in
 * ascending j: deterministic, no float atomics, a row's result independent of the batch.  Forward: a max pass over log_weight, then
 * one pass over k.  No per-thread array is indexed at run time.
 *
 * Inverse: (e, mu, sigma) of the element's K components and C0 = sum_k e c0 are formed once and kept in LDS laid out [k][thread]
 * (conflict-free; 256 threads up to K = 16, 128 above: at most 48 KB); exactly 25 halvings of [0, 1] follow -- a fixed trip count, no
 * global memory, no sin / exp inside -- comparing ((sum_k e (c + off) - C0) / sum_k e) (1 - eps) + x eps with the target; x is the
 * midpoint of the last bracket.  The closing evaluation at x is circ_totals, the forward's own function, on the LDS copy: dlogp = -sum_j L
 * at the returned x.  Targets outside [-1e-6, 1 + 1e-6] are counted into bad_count (an integer atomic add, the convention of bgk_colmap).
 *
 * Backward (one kernel, `inverse` flag; no LDS): pass 1 over k forms F, f, f'; with f_tot = f (1 - eps) + eps
 *   forward:  go = g_out, gl = g_dlogp[b];   g_y = go f_tot + gl (1 - eps) f' / f_tot
 *   inverse (at the saved x, outputs x and -sum_j L(x); implicit-function theorem):  G = g_x - g_dlogp[b] (1 - eps) f' / f_tot;
 *             g_y = G / f_tot,  go = -G / f_tot,  gl = -g_dlogp[b]
 * and pass 2 over k writes the gradients of the four RAW tensors from (go, gl):  gF = go (1 - eps), gf = gl (1 - eps) / f_tot,
 *   A_k = gF ((c - c0) + off) + gf sigma p                      g_log_weight = w (A_k - (gF F + gf f))
 *   g_mu = w (gF sigma (p0 - p) - gf sigma^2 p')                g_mu_raw = g_mu 0.5 cos(mu_raw)
 *   g_sigma = w (gF (p s - p0 s0) + gf (p + sigma p' s))        g_log_sigma = g_sigma exp(log_sigma)
 *   g_log_eps = (go (y - F) + gl (1 - f) / f_tot) eps (1 - eps)
 * The gradient at y == mu is the smooth derivative (s = u has derivative 1 there; the reference's comes from abs'(0) = 0). */
#include "bgk_common.h"

namespace {

constexpr int CB_THREADS = 256;
constexpr int CB_TILE = 2048;          /* elements of a tile: 8 per thread */
constexpr int CB_HALVINGS = 25;
constexpr int CB_MAX_GRID = 4096;

/* LEVEL 0: cdf; 1: + pdf; 2: + the derivative of the pdf */
template <int LEVEL>
__device__ __forceinline__ void circ_bump(float z, float& c, float& p, float& dp) {
    z = z < 0.0f ? 0.0f : (z > 1.0f ? 1.0f : z);
    const float zc = 1.0f - z;
    const float a = z * z * z, b = zc * zc * zc, d = a + b;
    const float r = bgk_rcp_refined(d);
    c = bgk_div_r(a, d, r);
    if constexpr (LEVEL >= 1) {
        const float qr = (z * zc) * r;
        p = 3.0f * (qr * qr);
        if constexpr (LEVEL >= 2) dp = 6.0f * (qr * (zc - z)) * (r * r);
    }
}

/* the component at mu against the point y: cdf c, offset off, pdf p, its derivative dp (all in z), the signed distance s */
template <int LEVEL>
__device__ __forceinline__ void circ_term(float y, float mu, float sigma, float& c, float& off, float& p, float& dp, float& s) {
    const float u = y - mu;
    const bool hi = mu > 0.5f;
    const bool wrapped = hi ? (u < -0.5f) : (u > 0.5f);
    s = wrapped ? (hi ? u + 1.0f : u - 1.0f) : u;
    off = (wrapped != hi) ? 1.0f : 0.0f;
    circ_bump<LEVEL>(sigma * s + 0.5f, c, p, dp);
}

/* the same component at y = 0 */
template <int LEVEL>
__device__ __forceinline__ void circ_origin(float mu, float sigma, float& c0, float& p0, float& s0) {
    float unused = 0.0f;
    s0 = mu > 0.5f ? 1.0f - mu : -mu;
    circ_bump<(LEVEL > 1 ? 1 : LEVEL)>(sigma * s0 + 0.5f, c0, p0, unused);
}

__device__ __forceinline__ void circ_eps(float log_eps, float& eps, float& ome) {
    const float t = bgk_expf(-log_eps);
    eps = 1.0f / (1.0f + t);
    ome = t * eps;
}

/* F, f (LEVEL >= 1), f' (LEVEL >= 2) and sum_k e of one element; param(k, e, mu, sigma) supplies component k -- from the raw tensors
 * in global memory (forward, backward) or from the LDS copy (the inverse's closing evaluation): the same sequence of operations */
template <int LEVEL, typename P>
__device__ __forceinline__ void circ_totals(float y, int K, P param, float& F, float& f, float& fp, float& S) {
    float sa = 0.0f, Fa = 0.0f, fa = 0.0f, fpa = 0.0f;
    for (int k = 0; k < K; ++k) {
        float e, mu, sigma;
        param(k, e, mu, sigma);
        float c, off, p = 0.0f, dp = 0.0f, s, c0, p0 = 0.0f, s0;
        circ_term<LEVEL>(y, mu, sigma, c, off, p, dp, s);
        circ_origin<0>(mu, sigma, c0, p0, s0);
        sa += e;
        Fa += e * ((c - c0) + off);
        if constexpr (LEVEL >= 1) fa += e * (sigma * p);
        if constexpr (LEVEL >= 2) fpa += e * (sigma * (sigma * dp));
    }
    S = sa;
    F = Fa / sa;
    f = fa / sa;
    fp = fpa / sa;
}

__device__ __forceinline__ float circ_max(const float* __restrict__ pw, int K, int D) {
    float m = pw[0];
    for (int k = 1; k < K; ++k) { const float v = pw[k * D]; m = v > m ? v : m; }
    return m;
}

struct CircArgs {
    const float* y; const float* mu_raw; const float* log_sigma; const float* log_weight; const float* log_eps;
    int64_t pp, pe, B; int K, D, TS;
    float* out; float* dlogp; int32_t* bad;
};

/* dlogp[b0 + r] = sign * sum_j s_l[r D + j], ascending j, one lane per row */
__device__ __forceinline__ void circ_row_sums(const float* s_l, int rows, int D, int64_t b0, float* dlogp, int tid, int nthreads) {
    for (int r = tid; r < rows; r += nthreads) {
        float acc = 0.0f;
        for (int j = 0; j < D; ++j) acc += s_l[r * D + j];
        dlogp[b0 + r] = acc;
    }
}

__global__ __launch_bounds__(CB_THREADS) void circular_forward_kernel(CircArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* s_l = smem;                       /* [TS][D] per-element log-density */
    const int K = a.K, D = a.D, TS = a.TS, tid = threadIdx.x;
    const int64_t n_tiles = (a.B + TS - 1) / TS;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t b0 = tile * TS;
        const int rows = (int)((a.B - b0) < TS ? (a.B - b0) : TS);
        const int n = rows * D;
        for (int i = tid; i < n; i += CB_THREADS) {
            const int r = i / D, j = i - r * D;
            const int64_t b = b0 + r;
            const float y = a.y[b * D + j];
            const float* pm = a.mu_raw + b * a.pp + j;
            const float* ps = a.log_sigma + b * a.pp + j;
            const float* pw = a.log_weight + b * a.pp + j;
            const float m = circ_max(pw, K, D);
            float F, f, fp, S;
            circ_totals<1>(y, K, [&](int k, float& e, float& mu, float& sigma) {
                e = bgk_expf(pw[k * D] - m);
                mu = 0.5f * sinf(pm[k * D]) + 0.5f;
                sigma = 1.0f + bgk_expf(ps[k * D]);
            }, F, f, fp, S);
            float eps, ome;
            circ_eps(a.log_eps[b * a.pe + j], eps, ome);
            a.out[b * D + j] = F * ome + y * eps;
            s_l[i] = bgk_logf(f * ome + eps);
        }
        __syncthreads();
        circ_row_sums(s_l, rows, D, b0, a.dlogp, tid, CB_THREADS);
        __syncthreads();                     /* the next tile overwrites s_l */
    }
}

template <int THREADS>
__global__ __launch_bounds__(THREADS) void circular_inverse_kernel(CircArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int K = a.K, D = a.D, TS = a.TS, tid = threadIdx.x;
    float* s_l = smem;                       /* [TS][D] */
    float* s_e = smem + TS * D;              /* [K][THREADS] each: this thread's element, slot k at [k * THREADS + tid] */
    float* s_mu = s_e + K * THREADS;
    float* s_sg = s_mu + K * THREADS;
    const int64_t n_tiles = (a.B + TS - 1) / TS;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t b0 = tile * TS;
        const int rows = (int)((a.B - b0) < TS ? (a.B - b0) : TS);
        const int n = rows * D;
        for (int i = tid; i < n; i += THREADS) {
            const int r = i / D, j = i - r * D;
            const int64_t b = b0 + r;
            const float t = a.y[b * D + j];
            if (a.bad && !(t >= -1e-6f && t <= 1.0f + 1e-6f)) atomicAdd(a.bad, 1);
            const float* pm = a.mu_raw + b * a.pp + j;
            const float* ps = a.log_sigma + b * a.pp + j;
            const float* pw = a.log_weight + b * a.pp + j;
            const float m = circ_max(pw, K, D);
            float S = 0.0f, C0 = 0.0f;
            for (int k = 0; k < K; ++k) {
                const float e = bgk_expf(pw[k * D] - m);
                const float mu = 0.5f * sinf(pm[k * D]) + 0.5f;
                const float sigma = 1.0f + bgk_expf(ps[k * D]);
                float c0, p0, s0;
                circ_origin<0>(mu, sigma, c0, p0, s0);
                s_e[k * THREADS + tid] = e; s_mu[k * THREADS + tid] = mu; s_sg[k * THREADS + tid] = sigma;
                S += e;
                C0 += e * c0;
            }
            float eps, ome;
            circ_eps(a.log_eps[b * a.pe + j], eps, ome);
            const float scale = ome / S;
            float lo = 0.0f, hi = 1.0f;
#pragma unroll 1
            for (int it = 0; it < CB_HALVINGS; ++it) {
                const float mid = 0.5f * (lo + hi);
                float acc = 0.0f;
                for (int k = 0; k < K; ++k) {
                    float c, off, p, dp, s;
                    circ_term<0>(mid, s_mu[k * THREADS + tid], s_sg[k * THREADS + tid], c, off, p, dp, s);
                    acc += s_e[k * THREADS + tid] * (c + off);
                }
                const bool above = (acc - C0) * scale + mid * eps > t;
                hi = above ? mid : hi;
                lo = above ? lo : mid;
            }
            const float x = 0.5f * (lo + hi);
            float F, f, fp;
            circ_totals<1>(x, K, [&](int k, float& e, float& mu, float& sigma) {
                e = s_e[k * THREADS + tid]; mu = s_mu[k * THREADS + tid]; sigma = s_sg[k * THREADS + tid];
            }, F, f, fp, S);
            a.out[b * D + j] = x;
            s_l[i] = -bgk_logf(f * ome + eps);
        }
        __syncthreads();
        circ_row_sums(s_l, rows, D, b0, a.dlogp, tid, THREADS);
        __syncthreads();
    }
}

struct CircBwdArgs {
    const float* y; const float* mu_raw; const float* log_sigma; const float* log_weight; const float* log_eps;
    int64_t pp, pe, B; int K, D, inverse;
    const float* g_out; const float* g_dlogp;
    float* g_y; float* g_mu; float* g_ls; float* g_lw; float* g_le;
};

__global__ __launch_bounds__(CB_THREADS) void circular_backward_kernel(CircBwdArgs a) {
    const int K = a.K, D = a.D;
    const int64_t total = a.B * D, KD = (int64_t)K * D;
    for (int64_t idx = (int64_t)blockIdx.x * CB_THREADS + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * CB_THREADS) {
        const int64_t b = idx / D;
        const int j = (int)(idx - b * D);
        const float y = a.y[idx];
        const float* pm = a.mu_raw + b * a.pp + j;
        const float* ps = a.log_sigma + b * a.pp + j;
        const float* pw = a.log_weight + b * a.pp + j;
        const float m = circ_max(pw, K, D);
        float F, f, fp, S;
        circ_totals<2>(y, K, [&](int k, float& e, float& mu, float& sigma) {
            e = bgk_expf(pw[k * D] - m);
            mu = 0.5f * sinf(pm[k * D]) + 0.5f;
            sigma = 1.0f + bgk_expf(ps[k * D]);
        }, F, f, fp, S);
        float eps, ome;
        circ_eps(a.log_eps[b * a.pe + j], eps, ome);
        const float ftot = f * ome + eps;
        const float dLdx = ome * fp / ftot;              /* d log f_tot / dx */
        float go, gl, gy;
        if (!a.inverse) {
            go = a.g_out[idx]; gl = a.g_dlogp[b];
            gy = go * ftot + gl * dLdx;
        } else {                                         /* outputs x and -sum_j L(x): G = g_x - g_dlogp dL/dx */
            const float G = a.g_out[idx] - a.g_dlogp[b] * dLdx;
            gy = G / ftot;
            go = -gy; gl = -a.g_dlogp[b];
        }
        a.g_y[idx] = gy;
        const float gF = go * ome, gf = gl * ome / ftot;
        a.g_le[idx] = (go * (y - F) + gl * (1.0f - f) / ftot) * (eps * ome);
        const float base = gF * F + gf * f;
        float* om = a.g_mu + b * KD + j;
        float* os = a.g_ls + b * KD + j;
        float* ow = a.g_lw + b * KD + j;
        for (int k = 0; k < K; ++k) {
            const float raw = pm[k * D];
            const float w = bgk_expf(pw[k * D] - m) / S;
            const float mu = 0.5f * sinf(raw) + 0.5f;
            const float es = bgk_expf(ps[k * D]);
            const float sigma = 1.0f + es;
            float c, off, p, dp, s, c0, p0, s0;
            circ_term<2>(y, mu, sigma, c, off, p, dp, s);
            circ_origin<1>(mu, sigma, c0, p0, s0);
            const float sdp = sigma * dp;
            const float A = gF * ((c - c0) + off) + gf * (sigma * p);
            ow[k * D] = w * (A - base);
            const float g_mu = w * (gF * (sigma * (p0 - p)) - gf * (sigma * sdp));
            om[k * D] = g_mu * (0.5f * cosf(raw));
            const float g_sg = w * (gF * (p * s - p0 * s0) + gf * (p + sdp * s));
            os[k * D] = g_sg * es;
        }
    }
}

int circ_check(const char* who, int64_t B, int32_t K, int32_t d, int64_t pp, int64_t pe) {
    BGK_CHECK_ARG(B >= 0, "%s: bad batch size %lld", who, (long long)B);
    if (K < 1 || K > BGK_CIRCULAR_MAX_COMPONENTS || d < 1 || d > BGK_CIRCULAR_MAX_WIDTH) {
        bgk_set_error("%s: (components, width) = (%d, %d) outside 1..%d x 1..%d", who, K, d, BGK_CIRCULAR_MAX_COMPONENTS, BGK_CIRCULAR_MAX_WIDTH);
        return BGK_EUNSUPPORTED;
    }
    BGK_CHECK_ARG((pp == 0 || pp >= (int64_t)K * d) && (pe == 0 || pe >= d), "%s: a row pitch is 0 (shared) or at least the row", who);
    return 0;
}

}  // namespace

extern "C" int bgk_circular_bump_transform(const float* y, const float* mu_raw, const float* log_sigma, const float* log_weight,
                                           int64_t param_pitch, const float* log_eps, int64_t eps_pitch, int64_t B,
                                           int32_t n_components, int32_t d, int32_t inverse, float* out, float* dlogp,
                                           int32_t* bad_count, void* stream) {
    const int st = circ_check("bgk_circular_bump_transform", B, n_components, d, param_pitch, eps_pitch);
    if (st) return st;
    if (B == 0) return 0;
    BGK_CHECK_ARG(y && mu_raw && log_sigma && log_weight && log_eps && out && dlogp, "bgk_circular_bump_transform: null pointer");
    CircArgs a{y, mu_raw, log_sigma, log_weight, log_eps, param_pitch, eps_pitch, B, n_components, d, 0, out, dlogp, inverse ? bad_count : nullptr};
    a.TS = CB_TILE / d < 1 ? 1 : CB_TILE / d;
    const int64_t n_tiles = (B + a.TS - 1) / a.TS;
    const int grid = (int)(n_tiles < CB_MAX_GRID ? n_tiles : CB_MAX_GRID);
    const size_t tile_bytes = sizeof(float) * (size_t)a.TS * d;
    hipStream_t s = (hipStream_t)stream;
    if (!inverse) {
        hipLaunchKernelGGL(circular_forward_kernel, dim3(grid), dim3(CB_THREADS), tile_bytes, s, a);
    } else if (n_components <= 16) {
        hipLaunchKernelGGL(circular_inverse_kernel<256>, dim3(grid), dim3(256), tile_bytes + sizeof(float) * 3 * n_components * 256, s, a);
    } else {
        hipLaunchKernelGGL(circular_inverse_kernel<128>, dim3(grid), dim3(128), tile_bytes + sizeof(float) * 3 * n_components * 128, s, a);
    }
    return bgk_launch_status("bgk_circular_bump_transform");
}

extern "C" int bgk_circular_bump_backward(const float* point, const float* mu_raw, const float* log_sigma, const float* log_weight,
                                          int64_t param_pitch, const float* log_eps, int64_t eps_pitch, int64_t B,
                                          int32_t n_components, int32_t d, int32_t inverse, const float* g_out, const float* g_dlogp,
                                          float* g_point, float* g_mu_raw, float* g_log_sigma, float* g_log_weight, float* g_log_eps,
                                          void* stream) {
    const int st = circ_check("bgk_circular_bump_backward", B, n_components, d, param_pitch, eps_pitch);
    if (st) return st;
    if (B == 0) return 0;
    BGK_CHECK_ARG(point && mu_raw && log_sigma && log_weight && log_eps && g_out && g_dlogp && g_point && g_mu_raw && g_log_sigma &&
                  g_log_weight && g_log_eps, "bgk_circular_bump_backward: null pointer");
    CircBwdArgs a{point, mu_raw, log_sigma, log_weight, log_eps, param_pitch, eps_pitch, B, n_components, d, inverse,
                  g_out, g_dlogp, g_point, g_mu_raw, g_log_sigma, g_log_weight, g_log_eps};
    const int64_t n_blocks = (B * d + CB_THREADS - 1) / CB_THREADS;
    const int grid = (int)(n_blocks < 4 * CB_MAX_GRID ? n_blocks : 4 * CB_MAX_GRID);
    hipLaunchKernelGGL(circular_backward_kernel, dim3(grid), dim3(CB_THREADS), 0, (hipStream_t)stream, a);
    return bgk_launch_status("bgk_circular_bump_backward");
}
