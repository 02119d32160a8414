/* bgk_mixture.hip -- a mixture of diagonal normals as ONE launch (bgflow/distribution/mixture.py:41-47: the stack of the K component
 * energies [B, 1, K] and the logsumexp over it, K energy evaluations per call and the same again under autograd).
 *
 * Tables (device, built by bgflow_amd/mixture.py): mu [K, d], h [K, d] (inverse variances, 1 without `cov`), logz [K]
 * (d / 2 log 2 pi + 1/2 sum log_diag); logw [K]: the live output of log_softmax.  Per row, in f32:
 *   q_k = sum_j (x_j - mu_kj)^2 h_kj              ascending j, the product folded into the sum by one fma
 *   a_k = (logw_k - logz_k) - 0.5 q_k
 *   m   = max_k a_k (a NaN is kept),  s = sum_k exp(a_k - m) in ascending k,  u = -(m + log s) / T
 *   r_k = exp(a_k - m) / s                         the responsibility (backward; m and s formed again from the row, never from u)
 * exp / log are the fixed sequences of bgk_detmath.h; exp's clamp at -80 would turn an argument of -inf into e^-80, so an argument below
 * -80 gives exactly 0: a component of weight zero contributes nothing and gets responsibility 0.  Only the difference form of q: the
 * expansion |x|^2 - 2 x.mu + |mu|^2 (and with it any matrix-core form) cancels to nothing in f32 for rows far from the means.
 * A row's result depends on that row alone -- not on B, its position in the batch or the grid; a NaN in a row stays in that row.
 *
 * Layout: a tile of 64 rows is staged coalesced into LDS (odd stride: lane = row reads conflict-free); the four waves of the workgroup
 * share the tile, wave w takes the components k = w, w + 4, ..: k is the outer loop, j the inner one, mu / h are read at wave-uniform
 * addresses (scalar loads).  The a_k meet in LDS ([K][64]); the maximum over four partial maxima is exact in any order, the exps are
 * again spread over the waves, and ONE lane per row adds them in ascending k.  50.9 KB of LDS at (K, d) = (64, 128): three workgroups
 * per CU.  A wave takes its components two at a time (every x_j read once for both; each sum the same sequence of operations).  Backward:
 * the forward's phases again up to m and s (every thread of a row adds the K exps itself), r_k = exp(a_k - m) / s, then wave w forms the columns [4 w, 4 w + 4), [4 w + 16, ..), .. of g_x = (g / T) sum_k r_k (x_j - mu_kj) h_kj
 * (ascending k) in place of the staged tile, which leaves as coalesced stores.  g_logw[k] = -(1 / T) sum_b g_b r_bk in f64: lanes merged
 * by the fixed shuffle tree of bgk_reduce.h, tiles added in the order the block walks them, block partials merged in a fixed order by a
 * second launch -- no float atomics.  A row whose upstream gradient is exactly 0 (a sample the KL form dropped) contributes exactly 0
 * to g_x and g_logw, whatever the row holds.
 *
 * bgk_mixture_sample: row b draws the numbers bgk_philox_fields writes for the fields [uniform 1, normal d] at the same (seed, offset,
 * row0); the uniform picks the first k whose running sum of exp(logw) (f32, ascending k) exceeds it, the last component of positive
 * weight catching what rounding leaves; x_j = mu_kj + n_j / sqrt(h_kj); the mixture energy of the sample (T = 1, the arithmetic
 * above) and the component come out of the same launch.  One wave per 64-row tile. */
#include "bgk_reduce.h"
#include "bgk_philox.h"

namespace {

constexpr int MX_WAVES = 4;
constexpr int MX_THREADS = MX_WAVES * 64;
constexpr int MX_ROWS = 64;
constexpr int MX_MAX_GRID = 2048;

__device__ __forceinline__ float mix_exp(float t) { return t < -80.0f ? 0.0f : bgk_expf(t); }

/* q_k of the row at xrow (LDS) for the component whose table rows are mk / hk (wave-uniform addresses) */
__device__ __forceinline__ float mix_q(const float* xrow, const float* __restrict__ mk, const float* __restrict__ hk, int d) {
    float q = 0.0f;
#pragma unroll 4
    for (int j = 0; j < d; ++j) {
        const float t = xrow[j] - mk[j];
        q = __builtin_fmaf(t * t, hk[j], q);
    }
    return q;
}

/* q of TWO components for the same row: every x_j is read once; each sum is the sequence of mix_q, bit for bit */
__device__ __forceinline__ void mix_q2(const float* xrow, const float* __restrict__ m0, const float* __restrict__ h0,
                                       const float* __restrict__ m1, const float* __restrict__ h1, int d, float& q0, float& q1) {
    float a = 0.0f, b = 0.0f;
#pragma unroll 4
    for (int j = 0; j < d; ++j) {
        const float x = xrow[j];
        const float t0 = x - m0[j], t1 = x - m1[j];
        a = __builtin_fmaf(t0 * t0, h0[j], a);
        b = __builtin_fmaf(t1 * t1, h1[j], b);
    }
    q0 = a; q1 = b;
}

/* f(k, q_k) for the components k = wave, wave + 4, .. of this wave, two at a time */
template <typename F>
__device__ __forceinline__ void mix_each_q(const float* xrow, const float* __restrict__ mu, const float* __restrict__ h, int K, int d, int wave, F f) {
    for (int k = wave; k < K; k += 2 * MX_WAVES) {
        const int k1 = k + MX_WAVES;
        if (k1 < K) {
            float q0, q1;
            mix_q2(xrow, mu + (size_t)k * d, h + (size_t)k * d, mu + (size_t)k1 * d, h + (size_t)k1 * d, d, q0, q1);
            f(k, q0);
            f(k1, q1);
        } else {
            f(k, mix_q(xrow, mu + (size_t)k * d, h + (size_t)k * d, d));
        }
    }
}

/* u of a row from its a_k: sum of the K exps (already formed, [K][64] in LDS) in ascending k */
__device__ __forceinline__ float mix_u(const float* s_e, int K, int lane, float m, float temperature) {
    float s = 0.0f;
    for (int k = 0; k < K; ++k) s += s_e[k * MX_ROWS + lane];
    const float lse = m + bgk_logf(s);
    return (s != s || m != m) ? __builtin_nanf("") : -lse / temperature;
}

/* rows [b0, b0 + rows) of x -> s_x [64][S], coalesced */
__device__ __forceinline__ void mix_stage(const float* __restrict__ x, int64_t ldx, int64_t b0, int rows, int d, uint32_t magic, int S,
                                          float* s_x, int tid, int nthreads) {
    for (int i = tid; i < rows * d; i += nthreads) {
        const int r = d == 1 ? i : (int)__umulhi((unsigned)i, magic), c = i - r * d;      /* (2^32 / 1 has no 32-bit magic) */
        s_x[r * S + c] = x[(b0 + r) * ldx + c];
    }
}

struct MixArgs {
    const float* x; int64_t ldx, B; int K, d; uint32_t magic; float temperature;
    float* u; float* neg_e;                                     /* neg_e [B, K] = -E_k(x), or NULL */
    const float* dlogp; int drop_nonfinite; float* partial;     /* partial [gridDim.x][2] or NULL */
};

__global__ __launch_bounds__(MX_THREADS) void mixture_energy_kernel(MixArgs a, const float* __restrict__ mu, const float* __restrict__ h,
                                                                    const float* __restrict__ logz, const float* __restrict__ logw) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int K = a.K, d = a.d, S = d | 1;
    float* s_x = smem;                            /* [64][S] */
    float* s_a = s_x + MX_ROWS * S;               /* [K][64] */
    float* s_m = s_a + K * MX_ROWS;               /* [4][64] partial maxima */
    float* s_red = s_m + MX_WAVES * MX_ROWS;      /* [2][64] */
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t n_tiles = (a.B + MX_ROWS - 1) / MX_ROWS;
    float bsum = 0.0f, bcnt = 0.0f;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t b0 = tile * MX_ROWS;
        const int rows = (int)((a.B - b0) < MX_ROWS ? (a.B - b0) : MX_ROWS);
        mix_stage(a.x, a.ldx, b0, rows, d, a.magic, S, s_x, tid, MX_THREADS);
        __syncthreads();
        float pmax = -__builtin_inff();
        mix_each_q(s_x + lane * S, mu, h, K, d, wave, [&](int k, float q) {
            const float lz = logz[k];
            const float av = (logw[k] - lz) - 0.5f * q;
            s_a[k * MX_ROWS + lane] = av;
            if (a.neg_e && lane < rows) a.neg_e[(b0 + lane) * K + k] = -(0.5f * q + lz);
            pmax = bgk_nan_max(pmax, av);
        });
        s_m[wave * MX_ROWS + lane] = pmax;
        __syncthreads();
        float m = s_m[lane];
#pragma unroll
        for (int w = 1; w < MX_WAVES; ++w) m = bgk_nan_max(m, s_m[w * MX_ROWS + lane]);
        for (int k = wave; k < K; k += MX_WAVES) s_a[k * MX_ROWS + lane] = mix_exp(s_a[k * MX_ROWS + lane] - m);
        __syncthreads();
        if (wave == 0 && lane < rows) {
            const float u = mix_u(s_a, K, lane, m, a.temperature);
            a.u[b0 + lane] = u;
            if (a.partial) {
                const float loss = u - a.dlogp[b0 + lane];
                const bool ok = !a.drop_nonfinite || __builtin_isfinite(loss);
                bsum += ok ? loss : 0.0f;
                bcnt += ok ? 1.0f : 0.0f;
            }
        }
        /* the next tile's staging writes s_x only (every wave is past its last read of it); s_a and s_m are written again after the
         * barrier that follows the staging, which wave 0 reaches after its sums */
    }
    if (a.partial) {                   /* block partial: fixed order over the 64 row lanes */
        if (wave == 0) { s_red[lane] = bsum; s_red[MX_ROWS + lane] = bcnt; }
        __syncthreads();
        if (tid == 0) {
            float s = 0.0f, c = 0.0f;
            for (int i = 0; i < MX_ROWS; ++i) { s += s_red[i]; c += s_red[MX_ROWS + i]; }
            a.partial[2 * blockIdx.x] = s; a.partial[2 * blockIdx.x + 1] = c;
        }
    }
}

struct MixBwdArgs {
    const float* x; int64_t ldx, B; int K, d; uint32_t magic; float temperature;
    const float* u;                      /* [B]: the energies the forward wrote (read by the loss-sum form's mask only) */
    const float* g_u;                    /* [B] upstream gradient, or NULL: then g_scalar[0] for the samples the loss-sum form kept */
    const float* g_scalar; const float* dlogp; int drop_nonfinite; float* g_dlogp;
    float* g_x; int64_t ldg;             /* may be NULL */
    double* wpartial;                    /* [gridDim.x][K] sums of g_b r_bk, or NULL */
};

__global__ __launch_bounds__(MX_THREADS) void mixture_energy_bwd_kernel(MixBwdArgs a, const float* __restrict__ mu, const float* __restrict__ h,
                                                                        const float* __restrict__ logz, const float* __restrict__ logw) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int K = a.K, d = a.d, S = d | 1;
    double* s_gw = reinterpret_cast<double*>(smem);      /* [64] (K used): the block's running sums */
    float* s_x = smem + 2 * 64;                          /* [64][S] */
    float* s_a = s_x + MX_ROWS * S;                      /* [K][64] */
    float* s_g = s_a + K * MX_ROWS;                      /* [64] upstream gradient of the row (0 beyond the tile) */
    float* s_m = s_g + MX_ROWS;                          /* [4][64] partial maxima */
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t n_tiles = (a.B + MX_ROWS - 1) / MX_ROWS;
    const float gs = a.g_scalar ? a.g_scalar[0] : 0.0f;
    if (tid < 64) s_gw[tid] = 0.0;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t b0 = tile * MX_ROWS;
        const int rows = (int)((a.B - b0) < MX_ROWS ? (a.B - b0) : MX_ROWS);
        mix_stage(a.x, a.ldx, b0, rows, d, a.magic, S, s_x, tid, MX_THREADS);
        if (wave == 0) {
            float g = 0.0f;
            if (lane < rows) {
                if (a.g_u) g = a.g_u[b0 + lane];
                else g = (!a.drop_nonfinite || __builtin_isfinite(a.u[b0 + lane] - a.dlogp[b0 + lane])) ? gs : 0.0f;
                if (a.g_dlogp) a.g_dlogp[b0 + lane] = -g;
            }
            s_g[lane] = g;
        }
        __syncthreads();
        /* the forward's a_k, m and s again, from the row itself: the responsibilities are r_k = exp(a_k - m) / s.  (T u of the saved energy
         * is NOT the log-sum-exp: u = fl(-lse / T) loses up to an ulp of lse, an absolute error in the exponent -- a factor e^1024 for a
         * row with lse ~ 1e10.) */
        const float g = s_g[lane];
        float pmax = -__builtin_inff();
        mix_each_q(s_x + lane * S, mu, h, K, d, wave, [&](int k, float q) {
            const float av = (logw[k] - logz[k]) - 0.5f * q;
            s_a[k * MX_ROWS + lane] = av;
            pmax = bgk_nan_max(pmax, av);
        });
        s_m[wave * MX_ROWS + lane] = pmax;
        __syncthreads();
        float m = s_m[lane];
#pragma unroll
        for (int w = 1; w < MX_WAVES; ++w) m = bgk_nan_max(m, s_m[w * MX_ROWS + lane]);
        for (int k = wave; k < K; k += MX_WAVES) s_a[k * MX_ROWS + lane] = mix_exp(s_a[k * MX_ROWS + lane] - m);
        __syncthreads();
        float ssum = 0.0f;                          /* every thread of the row adds the K exps in ascending k: the forward's s, bit for bit */
        for (int k = 0; k < K; ++k) ssum += s_a[k * MX_ROWS + lane];
        __syncthreads();                            /* all sums are formed before any exp is replaced by its responsibility */
        for (int k = wave; k < K; k += MX_WAVES) {
            const float r = g == 0.0f ? 0.0f : s_a[k * MX_ROWS + lane] / ssum;
            s_a[k * MX_ROWS + lane] = r;
            if (a.wpartial) {
                double v = (double)(g * r);
                bgk_wave_reduce(v, [](double& acc, double o) { acc += o; });
                if (lane == 0) s_gw[k] += v;         /* k belongs to this wave alone */
            }
        }
        __syncthreads();
        if (a.g_x) {
            const float scale = g / a.temperature;
            /* wave w takes the whole chunks of columns [4 w, 4 w + 4), [4 w + 16, ..), ..: r_k is read once per four columns, mu / h in
             * 16-byte pieces; every column's sum runs over k in ascending order.  A thread alone reads and writes its slots of s_x. */
            float* xr = s_x + lane * S;
            const int d4 = d & ~3;
            const bool z = g == 0.0f;
            for (int j0 = 4 * wave; j0 < d4; j0 += 4 * MX_WAVES) {
                const float x0 = xr[j0], x1 = xr[j0 + 1], x2 = xr[j0 + 2], x3 = xr[j0 + 3];
                float c0 = 0.0f, c1 = 0.0f, c2 = 0.0f, c3 = 0.0f;
                for (int k = 0; k < K; ++k) {
                    const float r = s_a[k * MX_ROWS + lane];
                    const float* mk = mu + (size_t)k * d + j0;
                    const float* hk = h + (size_t)k * d + j0;
                    c0 = __builtin_fmaf(r * (x0 - mk[0]), hk[0], c0);
                    c1 = __builtin_fmaf(r * (x1 - mk[1]), hk[1], c1);
                    c2 = __builtin_fmaf(r * (x2 - mk[2]), hk[2], c2);
                    c3 = __builtin_fmaf(r * (x3 - mk[3]), hk[3], c3);
                }
                xr[j0] = z ? 0.0f : scale * c0; xr[j0 + 1] = z ? 0.0f : scale * c1;
                xr[j0 + 2] = z ? 0.0f : scale * c2; xr[j0 + 3] = z ? 0.0f : scale * c3;
            }
            const int jt = d4 + wave;               /* the up to three columns past the last whole chunk: one per wave */
            if (jt < d) {
                const float xj = xr[jt];
                float acc = 0.0f;
                for (int k = 0; k < K; ++k) {
                    const float t = xj - mu[(size_t)k * d + jt];
                    acc = __builtin_fmaf(s_a[k * MX_ROWS + lane] * t, h[(size_t)k * d + jt], acc);
                }
                xr[jt] = z ? 0.0f : scale * acc;
            }
            __syncthreads();
            for (int i = tid; i < rows * d; i += MX_THREADS) {
                const int r = d == 1 ? i : (int)__umulhi((unsigned)i, a.magic), c = i - r * d;
                a.g_x[(b0 + r) * a.ldg + c] = s_x[r * S + c];
            }
        }
        __syncthreads();              /* the next tile's staging overwrites s_x and s_g */
    }
    if (a.wpartial) {
        __syncthreads();
        if (tid < K) a.wpartial[(size_t)blockIdx.x * K + tid] = s_gw[tid];
    }
}

/* g_logw[k] = -(sum over the blocks' partials) / T: block k of the grid; lane t adds the partials t, t + 64, .. in ascending order,
 * lane 0 then the 64 lane sums in ascending order */
__global__ __launch_bounds__(64) void mixture_logw_merge_kernel(const double* wpartial, int nblk, int K, double temperature, float* g_logw) {
    __shared__ double s_s[64];
    const int k = blockIdx.x;
    double s = 0.0;
    for (int i = threadIdx.x; i < nblk; i += 64) s += wpartial[(size_t)i * K + k];
    s_s[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int i = 0; i < 64; ++i) t += s_s[i];
        g_logw[k] = (float)(-t / temperature);
    }
}

struct MixSampleArgs {
    float* x; int64_t ldx, B, row0; int K, d; uint32_t magic;
    uint32_t seed_lo, seed_hi, offset;
    int32_t* assign; float* energy;
};

__global__ __launch_bounds__(64) void mixture_sample_kernel(MixSampleArgs a, const float* __restrict__ mu, const float* __restrict__ h,
                                                            const float* __restrict__ logz, const float* __restrict__ logw) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int K = a.K, d = a.d, S = d | 1;
    float* s_x = smem;                            /* [64][S] */
    float* s_a = s_x + MX_ROWS * S;               /* [K][64] */
    const int lane = threadIdx.x;
    const int64_t b0 = (int64_t)blockIdx.x * MX_ROWS;
    if (b0 >= a.B) return;
    const int rows = (int)((a.B - b0) < MX_ROWS ? (a.B - b0) : MX_ROWS);
    const uint64_t grow = (uint64_t)(a.row0 + b0 + lane);
    const uint32_t r_lo = (uint32_t)grow, r_hi = (uint32_t)(grow >> 32);
    uint32_t o[4];
    philox4x32_10(r_lo, r_hi, 0u, a.offset, a.seed_lo, a.seed_hi, o);           /* field 0: the uniform, column 0 */
    const float uu = u01(o[0]);
    int kk = -1, last = 0;
    float cum = 0.0f;
    for (int k = 0; k < K; ++k) {
        const float w = mix_exp(logw[k]);
        cum += w;
        last = w > 0.0f ? k : last;
        kk = (kk < 0 && cum > uu) ? k : kk;
    }
    kk = kk < 0 ? last : kk;
    const float* mk = mu + (size_t)kk * d;
    const float* hk = h + (size_t)kk * d;
    float* row = s_x + lane * S;
    for (int cb = 0; 4 * cb < d; ++cb) {
        philox4x32_10(r_lo, r_hi, (1u << 20) | (uint32_t)cb, a.offset, a.seed_lo, a.seed_hi, o);      /* field 1: the d normals */
        float v[4];
        philox_normal4(o, v);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int col = 4 * cb + q;
            if (col < d) row[col] = mk[col] + v[q] / __builtin_sqrtf(hk[col]);
        }
    }
    /* the mixture energy of the sample at T = 1: the arithmetic of mixture_energy_kernel, every component on this lane */
    float m = -__builtin_inff();
    for (int k = 0; k < K; ++k) {
        const float q = mix_q(row, mu + (size_t)k * d, h + (size_t)k * d, d);
        const float av = (logw[k] - logz[k]) - 0.5f * q;
        s_a[k * MX_ROWS + lane] = av;
        m = bgk_nan_max(m, av);
    }
    for (int k = 0; k < K; ++k) s_a[k * MX_ROWS + lane] = mix_exp(s_a[k * MX_ROWS + lane] - m);
    if (lane < rows) {
        if (a.energy) a.energy[b0 + lane] = mix_u(s_a, K, lane, m, 1.0f);
        if (a.assign) a.assign[b0 + lane] = kk;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    for (int i = lane; i < rows * d; i += 64) {
        const int r = d == 1 ? i : (int)__umulhi((unsigned)i, a.magic), c = i - r * d;
        a.x[(b0 + r) * a.ldx + c] = s_x[r * S + c];
    }
}

int mix_check(const char* who, int64_t B, int32_t K, int32_t d, const float* mu, const float* h, const float* logz, const float* logw) {
    BGK_CHECK_ARG(B >= 0 && mu && h && logz && logw, "%s: bad arguments", who);
    if (K < 1 || K > BGK_MIXTURE_MAX_COMPONENTS || d < 1 || d > BGK_MIXTURE_MAX_WIDTH) {
        bgk_set_error("%s: (components, width) = (%d, %d) outside 1..%d x 1..%d", who, K, d, BGK_MIXTURE_MAX_COMPONENTS, BGK_MIXTURE_MAX_WIDTH);
        return BGK_EUNSUPPORTED;
    }
    return 0;
}

uint32_t mix_magic(int d) { return (uint32_t)(((1ull << 32) + (uint64_t)d - 1) / (uint64_t)d); }

int mix_grid(int64_t B, int cap) {
    const int64_t n_tiles = (B + MX_ROWS - 1) / MX_ROWS;
    return (int)(n_tiles < cap ? n_tiles : cap);
}

}  // namespace

extern "C" int bgk_mixture_energy(const float* x, int64_t ldx, int64_t B, int32_t n_components, int32_t d,
                                  const float* mu, const float* h, const float* logz, const float* logw, double temperature,
                                  float* u, float* neg_e, const float* dlogp, int32_t drop_nonfinite, float* partial, int32_t nblk,
                                  double* loss_sums, void* stream) {
    const int st = mix_check("bgk_mixture_energy", B, n_components, d, mu, h, logz, logw);
    if (st) return st;
    BGK_CHECK_ARG(temperature > 0.0 && (B == 0 || (x && u && ldx >= d)), "bgk_mixture_energy: bad arguments");
    BGK_CHECK_ARG(!loss_sums || (dlogp && partial && nblk >= 1), "bgk_mixture_energy: the loss sums need dlogp and a [nblk, 2] workspace");
    hipStream_t s = (hipStream_t)stream;
    if (B == 0) {
        if (loss_sums) { hipError_t e = hipMemsetAsync(loss_sums, 0, 2 * sizeof(double), s); if (e != hipSuccess) return (int)e; }
        return 0;
    }
    MixArgs a{};
    a.x = x; a.ldx = ldx; a.B = B; a.K = n_components; a.d = d; a.magic = mix_magic(d); a.temperature = (float)temperature;
    a.u = u; a.neg_e = neg_e; a.dlogp = loss_sums ? dlogp : nullptr; a.drop_nonfinite = drop_nonfinite; a.partial = loss_sums ? partial : nullptr;
    int grid = mix_grid(B, MX_MAX_GRID);
    if (loss_sums && grid > nblk) grid = nblk;
    const size_t shmem = sizeof(float) * ((size_t)MX_ROWS * (d | 1) + (size_t)n_components * MX_ROWS + (MX_WAVES + 2) * MX_ROWS);
    hipLaunchKernelGGL(mixture_energy_kernel, dim3(grid), dim3(MX_THREADS), shmem, s, a, mu, h, logz, logw);
    if (loss_sums) return bgk_loss_partial_reduce(partial, grid, loss_sums, stream);
    return bgk_launch_status("bgk_mixture_energy");
}

extern "C" int bgk_mixture_energy_backward(const float* x, int64_t ldx, int64_t B, int32_t n_components, int32_t d,
                                           const float* mu, const float* h, const float* logz, const float* logw, double temperature,
                                           const float* u, const float* g_u, const float* g_scalar, const float* dlogp,
                                           int32_t drop_nonfinite, float* g_dlogp, float* g_x, int64_t ldg,
                                           float* g_logw, double* wpartial, int32_t nblk, void* stream) {
    const int st = mix_check("bgk_mixture_energy_backward", B, n_components, d, mu, h, logz, logw);
    if (st) return st;
    BGK_CHECK_ARG(temperature > 0.0 && (B == 0 || (x && u && ldx >= d)) && (!g_x || ldg >= d), "bgk_mixture_energy_backward: bad arguments");
    BGK_CHECK_ARG(B == 0 || g_u || (g_scalar && dlogp), "bgk_mixture_energy_backward: need g_u [B] or (g_scalar, dlogp)");
    BGK_CHECK_ARG(!g_logw || (wpartial && nblk >= 1), "bgk_mixture_energy_backward: g_logw needs a [nblk, n_components] f64 workspace");
    hipStream_t s = (hipStream_t)stream;
    if (B == 0) {
        if (g_logw) { hipError_t e = hipMemsetAsync(g_logw, 0, n_components * sizeof(float), s); if (e != hipSuccess) return (int)e; }
        return 0;
    }
    MixBwdArgs a{};
    a.x = x; a.ldx = ldx; a.B = B; a.K = n_components; a.d = d; a.magic = mix_magic(d); a.temperature = (float)temperature;
    a.u = u; a.g_u = g_u; a.g_scalar = g_scalar; a.dlogp = dlogp; a.drop_nonfinite = drop_nonfinite; a.g_dlogp = g_dlogp;
    a.g_x = g_x; a.ldg = ldg; a.wpartial = g_logw ? wpartial : nullptr;
    int grid = mix_grid(B, MX_MAX_GRID);
    if (g_logw && grid > nblk) grid = nblk;
    const size_t shmem = sizeof(float) * (2 * 64 + (size_t)MX_ROWS * (d | 1) + (size_t)n_components * MX_ROWS + (1 + MX_WAVES) * MX_ROWS);
    hipLaunchKernelGGL(mixture_energy_bwd_kernel, dim3(grid), dim3(MX_THREADS), shmem, s, a, mu, h, logz, logw);
    if (g_logw) hipLaunchKernelGGL(mixture_logw_merge_kernel, dim3(n_components), dim3(64), 0, s, wpartial, grid, n_components, temperature, g_logw);
    return bgk_launch_status("bgk_mixture_energy_backward");
}

extern "C" int bgk_mixture_sample(uint64_t seed, uint32_t offset, int64_t row0, int64_t B, int32_t n_components, int32_t d,
                                  const float* mu, const float* h, const float* logz, const float* logw,
                                  float* x, int64_t ldx, int32_t* assign, float* energy, void* stream) {
    const int st = mix_check("bgk_mixture_sample", B, n_components, d, mu, h, logz, logw);
    if (st) return st;
    if (B == 0) return 0;
    BGK_CHECK_ARG(x && ldx >= d && row0 >= 0, "bgk_mixture_sample: bad arguments");
    const int64_t n_tiles = (B + MX_ROWS - 1) / MX_ROWS;
    BGK_CHECK_ARG(n_tiles < (int64_t)0x7fffffff, "bgk_mixture_sample: batch too large for one launch");
    MixSampleArgs a{};
    a.x = x; a.ldx = ldx; a.B = B; a.row0 = row0; a.K = n_components; a.d = d; a.magic = mix_magic(d);
    a.seed_lo = (uint32_t)seed; a.seed_hi = (uint32_t)(seed >> 32); a.offset = offset; a.assign = assign; a.energy = energy;
    const size_t shmem = sizeof(float) * ((size_t)MX_ROWS * (d | 1) + (size_t)n_components * MX_ROWS);
    hipLaunchKernelGGL(mixture_sample_kernel, dim3((unsigned)n_tiles), dim3(64), shmem, (hipStream_t)stream, a, mu, h, logz, logw);
    return bgk_launch_status("bgk_mixture_sample");
}
