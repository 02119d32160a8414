/* bgk_clip.hip -- gradient clipping and the energy cut of robust reverse-KL training as launches of their own (the forms folded into the
 * target-energy kernels are in bgk_energy.hip; the arithmetic both share is bgk_clip.h):
 *   bgk_clip_gradient   ClipGradient.clip_tensor (bgflow/utils/train.py:107-118) of a [B, D] gradient: NaN -> 0, groups of norm_dim
 *                       consecutive elements of a row scaled by min(clip / |group|_2, 1); norm_dim = -1: one norm over the whole tensor
 *   bgk_linlogcut       linlogcut (train.py:60-62) of a vector, or its derivative times an upstream gradient -- LinLogCutEnergy
 *                       (bgflow/distribution/energy/clipped.py:25-27) around a delegate that is not described by kernel fields
 * HBM-bound: 8 B per element.  No atomics, every sum in a fixed order: two runs give the same bits. */
#include "bgk_clip.h"

namespace {

constexpr int NC_THREADS = 256;

/* norm_dim in {1, 2, 4}, D a multiple of 4, 16-byte aligned rows: a lane owns one float4 = whole groups */
__global__ __launch_bounds__(NC_THREADS) void clip_quads_kernel(const float* g, int64_t ldg, int64_t B, int D, float clip, int nd,
                                                                 float* out, int64_t ldo) {
    const int q = D >> 2;
    const int64_t total = B * q;
    for (int64_t i = (int64_t)blockIdx.x * NC_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * NC_THREADS) {
        const int64_t r = i / q;
        const int c = (int)(i - r * q) * 4;
        const float4 v = *reinterpret_cast<const float4*>(g + r * ldg + c);
        *reinterpret_cast<float4*>(out + r * ldo + c) = bgk_clip_quad(v, nd, clip);
    }
}

/* any norm_dim that divides D: a lane owns one group at a time (two passes over its nd elements; the second hits the cache) */
__global__ __launch_bounds__(NC_THREADS) void clip_groups_kernel(const float* g, int64_t ldg, int64_t B, int D, float clip, int nd,
                                                                  float* out, int64_t ldo) {
    const int gpr = D / nd;
    const int64_t total = B * gpr;
    for (int64_t i = (int64_t)blockIdx.x * NC_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * NC_THREADS) {
        const int64_t r = i / gpr;
        const int c0 = (int)(i - r * gpr) * nd;
        const float* src = g + r * ldg + c0;
        if (nd == 1) { out[r * ldo + c0] = bgk_clip_value(bgk_clip_clean(src[0]), clip); continue; }
        float ss = 0.0f;
        for (int j = 0; j < nd; ++j) { const float v = bgk_clip_clean(src[j]); ss += v * v; }
        const float f = bgk_clip_factor(ss, clip);
        float* dst = out + r * ldo + c0;
        for (int j = 0; j < nd; ++j) dst[j] = bgk_clip_clean(src[j]) * f;      /* (in place: a group is read and written by one lane) */
    }
}

/* fixed-order sum of the 256 lane values of a block (LDS tree), valid in lane 0 */
__device__ __forceinline__ double block_sum(double v, double* s) {
    s[threadIdx.x] = v;
    __syncthreads();
    for (int off = NC_THREADS / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) s[threadIdx.x] += s[threadIdx.x + off];
        __syncthreads();
    }
    return s[0];
}

/* norm_dim = -1, first launch: partial[block] = sum of squares (double) of the cleaned values the block owns */
__global__ __launch_bounds__(NC_THREADS) void clip_sumsq_kernel(const float* g, int64_t ldg, int64_t B, int D, double* partial) {
    __shared__ double s[NC_THREADS];
    const int64_t total = B * D;
    double acc = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * NC_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * NC_THREADS) {
        const int64_t r = i / D;
        const double v = (double)bgk_clip_clean(g[r * ldg + (i - r * D)]);
        acc += v * v;
    }
    const double t = block_sum(acc, s);
    if (threadIdx.x == 0) partial[blockIdx.x] = t;
}

/* second launch: every block adds the partials in the same fixed order and scales its elements.  The reference forms the norm in f32: a
 * sum of squares beyond FLT_MAX is inf there and the factor clip / inf = 0 -- kept (a tensor with an inf entry comes out all zero). */
__global__ __launch_bounds__(NC_THREADS) void clip_scale_all_kernel(const float* g, int64_t ldg, int64_t B, int D, double clip,
                                                                     const double* partial, int nblk, float* out, int64_t ldo, double* norm_out) {
    __shared__ double s[NC_THREADS];
    double acc = 0.0;
    for (int i = threadIdx.x; i < nblk; i += NC_THREADS) acc += partial[i];
    const double ss = block_sum(acc, s);
    double fd = ss > (double)BGK_FLT_MAX ? 0.0 : clip / sqrt(ss);
    fd = fd < 1.0 ? fd : (fd != fd ? fd : 1.0);
    const float f = (float)fd;
    if (blockIdx.x == 0 && threadIdx.x == 0 && norm_out) norm_out[0] = sqrt(ss);
    const int64_t total = B * D;
    for (int64_t i = (int64_t)blockIdx.x * NC_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * NC_THREADS) {
        const int64_t r = i / D;
        const int64_t c = i - r * D;
        out[r * ldo + c] = bgk_clip_clean(g[r * ldg + c]) * f;
    }
}

__global__ __launch_bounds__(NC_THREADS) void linlogcut_kernel(const float* v, const float* g, int64_t n, float high, float max_val, float* out) {
    for (int64_t i = (int64_t)blockIdx.x * NC_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * NC_THREADS)
        out[i] = g ? g[i] * bgk_linlogcut_grad(v[i], high, max_val) : bgk_linlogcut(v[i], high, max_val);
}

int grid_for(int64_t work, int cap) {
    const int64_t nb = (work + NC_THREADS - 1) / NC_THREADS;
    return (int)(nb < cap ? (nb < 1 ? 1 : nb) : cap);
}

}  // namespace

extern "C" int bgk_clip_gradient(const float* g, int64_t ldg, int64_t B, int32_t D, double clip, int32_t norm_dim,
                                 float* out, int64_t ldo, double* workspace, int32_t nblk, void* stream) {
    BGK_CHECK_ARG(B >= 0 && D >= 1, "bgk_clip_gradient: bad sizes (B %lld, D %d)", (long long)B, D);
    BGK_CHECK_ARG(norm_dim == -1 || (norm_dim >= 1 && D % norm_dim == 0),
                  "bgk_clip_gradient: norm_dim %d is neither -1 nor a divisor of the row width %d (groups do not straddle rows)", norm_dim, D);
    BGK_CHECK_ARG(clip == clip && clip >= 0.0, "bgk_clip_gradient: clip must be a non-negative number");
    if (B == 0) return 0;
    BGK_CHECK_ARG(g && out && ldg >= D && ldo >= D, "bgk_clip_gradient: null pointer / row stride below the width");
    hipStream_t s = (hipStream_t)stream;
    if (norm_dim == -1) {
        BGK_CHECK_ARG(workspace && nblk >= 1, "bgk_clip_gradient: norm_dim -1 needs a workspace of nblk + 1 doubles");
        const int grid = grid_for(B * D, nblk < 1024 ? nblk : 1024);
        hipLaunchKernelGGL(clip_sumsq_kernel, dim3(grid), dim3(NC_THREADS), 0, s, g, ldg, B, D, workspace);
        hipLaunchKernelGGL(clip_scale_all_kernel, dim3(grid_for(B * D, 2048)), dim3(NC_THREADS), 0, s, g, ldg, B, D, clip,
                           (const double*)workspace, grid, out, ldo, workspace + nblk);
        return bgk_launch_status("bgk_clip_gradient");
    }
    const auto al = [](const void* p, int64_t ld) { return ((uintptr_t)p & 15) == 0 && ld % 4 == 0; };
    if (D % 4 == 0 && (norm_dim == 1 || norm_dim == 2 || norm_dim == 4) && al(g, ldg) && al(out, ldo))
        hipLaunchKernelGGL(clip_quads_kernel, dim3(grid_for(B * (D / 4), 4096)), dim3(NC_THREADS), 0, s, g, ldg, B, D, (float)clip, norm_dim, out, ldo);
    else
        hipLaunchKernelGGL(clip_groups_kernel, dim3(grid_for(B * (D / norm_dim), 4096)), dim3(NC_THREADS), 0, s, g, ldg, B, D, (float)clip,
                           norm_dim, out, ldo);
    return bgk_launch_status("bgk_clip_gradient");
}

extern "C" int bgk_linlogcut(const float* v, const float* g, int64_t n, double high, double max_val, float* out, void* stream) {
    BGK_CHECK_ARG(n >= 0 && high == high && max_val == max_val, "bgk_linlogcut: bad arguments");
    if (n == 0) return 0;
    BGK_CHECK_ARG(v && out, "bgk_linlogcut: null pointer");
    hipLaunchKernelGGL(linlogcut_kernel, dim3(grid_for(n, 2048)), dim3(NC_THREADS), 0, (hipStream_t)stream, v, g, n, (float)high, (float)max_val, out);
    return bgk_launch_status("bgk_linlogcut");
}
