/* bgk_optim.hip -- optimizer step of the training loop on the flat parameter / gradient bucket:
 *   bgk_grad_nan_flag   flag[0] = 1 if any gradient is NaN (the reference KLTrainer skips the optimizer step in that case,
 *                       nn/training/trainers.py:198-201 -- there with a host round trip per parameter tensor)
 *   bgk_adam_step       torch.optim.Adam's update (bias-corrected first / second moments, eps outside the square root, optional
 *                       L2 weight decay) over ONE contiguous bucket, skipped on the device when flag[0] != 0; counts skipped steps
 *   bgk_grad_norm_flag  the same scan that also gives the f64 sum of squares of the bucket (fixed-order block partials, then one
 *                       block): the total 2-norm torch.nn.utils.clip_grad_norm_ forms over ~100 parameter views; a non-finite sum sets
 *                       the flag as well
 *   bgk_adam_step_clipped  bgk_adam_step on coef * g, coef = min(1, max_norm / (sqrt(sumsq) + 1e-6)) formed on the device
 *                       (clip_grad_norm_ with norm_type = 2 without its host read; the bucket itself stays unscaled)
 * One launch each instead of torch's per-tensor-list multi-tensor kernels + the NaN scans; HBM-bound: 4 x 4 B read + 3 x 4 B
 * written per parameter (1.07 M parameters for cfg 3: microseconds). */
#include "bgk_common.h"

namespace {

__global__ __launch_bounds__(256) void nan_flag_kernel(const float* g, int64_t n, int32_t* flag) {
    int bad = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) bad |= (g[i] != g[i]);
    if (__builtin_amdgcn_ballot_w64(bad != 0) && (threadIdx.x & 63) == 0) atomicOr(flag, 1);
}

struct AdamArgs {
    float* p; const float* g; float* m; float* v; int64_t n;
    float lr, beta1, beta2, eps, weight_decay;
    int64_t step;                                                  /* number of bgk_adam_step calls so far, this one included */
    const int32_t* flag; int32_t* skipped;
    const double* sumsq; float max_norm;                          /* sumsq != NULL: the gradient is scaled by the norm-clip coefficient */
};

/* partial[block] = sum of squares (double) of the block's elements, lanes and blocks in a fixed order; flag |= any NaN */
__global__ __launch_bounds__(256) void norm_flag_kernel(const float* g, int64_t n, int32_t* flag, double* partial) {
    __shared__ double s[256];
    int bad = 0;
    double acc = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const float v = g[i];
        bad |= (v != v);
        acc += (double)v * (double)v;
    }
    if (__builtin_amdgcn_ballot_w64(bad != 0) && (threadIdx.x & 63) == 0) atomicOr(flag, 1);
    s[threadIdx.x] = acc;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) s[threadIdx.x] += s[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[blockIdx.x] = s[0];
}

__global__ __launch_bounds__(256) void norm_reduce_kernel(const double* partial, int nblk, double* sumsq, int32_t* flag) {
    __shared__ double s[256];
    double acc = 0.0;
    for (int i = threadIdx.x; i < nblk; i += 256) acc += partial[i];
    s[threadIdx.x] = acc;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) s[threadIdx.x] += s[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        sumsq[0] = s[0];
        if (!(s[0] <= 1.7976931348623157e308)) atomicOr(flag, 1);      /* inf (an inf gradient) or NaN: the step is skipped */
    }
}

/* Adam's time step is `step - skipped[0]`: the skip count is read on the device, so an update skipped for a NaN gradient does not
 * advance the bias corrections 1 - beta^t (the reference does not call optim.step() at all in that case, trainers.py:198-201)
 * and the host never has to know whether a step was skipped.  Races: the skip path only writes `skipped`, the update path
 * only reads it. */
__global__ __launch_bounds__(256) void adam_kernel(AdamArgs a) {
    if (a.flag && a.flag[0] != 0) {
        if (blockIdx.x == 0 && threadIdx.x == 0 && a.skipped) atomicAdd(a.skipped, 1);
        return;
    }
    __shared__ float s_bc[2];
    if (threadIdx.x == 0) {
        const double t = (double)(a.step - (a.skipped ? (int64_t)a.skipped[0] : 0));
        s_bc[0] = (float)(1.0 - pow((double)a.beta1, t));               /* bc1 = 1 - beta1^t */
        s_bc[1] = (float)sqrt(1.0 - pow((double)a.beta2, t)); /* sqrt(1 - beta2^t) */
    }
    __syncthreads();
    const float step_size = a.lr / s_bc[0], bc2_sqrt = s_bc[1];
    float coef = 1.0f;
    if (a.sumsq) {
        const double c = (double)a.max_norm / (sqrt(a.sumsq[0]) + 1e-6);
        coef = (float)(c < 1.0 ? c : 1.0);
    }
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * 256) {
        float g = a.g[i];
        if (a.sumsq) g = g * coef;
        const float p = a.p[i];
        if (a.weight_decay != 0.0f) g = g + a.weight_decay * p;
        const float m = a.beta1 * a.m[i] + (1.0f - a.beta1) * g;
        const float v = a.beta2 * a.v[i] + (1.0f - a.beta2) * (g * g);
        a.m[i] = m; a.v[i] = v;
        const float denom = __builtin_sqrtf(v) / bc2_sqrt + a.eps;
        a.p[i] = p - step_size * (m / denom);
    }
}

}  // namespace

extern "C" int bgk_grad_nan_flag(const float* g, int64_t n, int32_t* flag, void* stream) {
    BGK_CHECK_ARG(g && flag && n >= 0, "bgk_grad_nan_flag: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(flag, 0, sizeof(int32_t), st);
    if (e != hipSuccess) { bgk_set_error("bgk_grad_nan_flag: %s", hipGetErrorString(e)); return (int)e; }
    if (n == 0) return 0;
    const int64_t nb = (n + 255) / 256;
    hipLaunchKernelGGL(nan_flag_kernel, dim3((unsigned)(nb < 2048 ? nb : 2048)), dim3(256), 0, st, g, n, flag);
    return bgk_launch_status("bgk_grad_nan_flag");
}

extern "C" int bgk_grad_norm_flag(const float* g, int64_t n, int32_t* flag, double* partial, int32_t nblk, double* sumsq, void* stream) {
    BGK_CHECK_ARG(g && flag && partial && sumsq && n >= 0 && nblk >= 1, "bgk_grad_norm_flag: bad arguments (null pointer / no partial workspace)");
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(flag, 0, sizeof(int32_t), st);
    if (e == hipSuccess && n == 0) e = hipMemsetAsync(sumsq, 0, sizeof(double), st);
    if (e != hipSuccess) { bgk_set_error("bgk_grad_norm_flag: %s", hipGetErrorString(e)); return (int)e; }
    if (n == 0) return 0;
    const int64_t nb = (n + 255) / 256;
    const int cap = nblk < 1024 ? nblk : 1024;
    const int grid = (int)(nb < cap ? nb : cap);
    hipLaunchKernelGGL(norm_flag_kernel, dim3(grid), dim3(256), 0, st, g, n, flag, partial);
    hipLaunchKernelGGL(norm_reduce_kernel, dim3(1), dim3(256), 0, st, (const double*)partial, grid, sumsq, flag);
    return bgk_launch_status("bgk_grad_norm_flag");
}

static int adam_launch(const char* what, float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                       float weight_decay, int64_t step, const int32_t* skip_flag, int32_t* skipped_count, const double* sumsq, float max_norm,
                       void* stream) {
    BGK_CHECK_ARG(p && g && m && v && n >= 0 && step >= 1, "%s: bad arguments", what);
    if (n == 0) return 0;
    AdamArgs a{p, g, m, v, n, lr, beta1, beta2, eps, weight_decay, step, skip_flag, skipped_count, sumsq, max_norm};
    const int64_t nb = (n + 255) / 256;
    hipLaunchKernelGGL(adam_kernel, dim3((unsigned)(nb < 4096 ? nb : 4096)), dim3(256), 0, (hipStream_t)stream, a);
    return bgk_launch_status(what);
}

extern "C" int bgk_adam_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                             float weight_decay, int64_t step, const int32_t* skip_flag, int32_t* skipped_count, void* stream) {
    return adam_launch("bgk_adam_step", p, g, m, v, n, lr, beta1, beta2, eps, weight_decay, step, skip_flag, skipped_count, nullptr, 0.0f, stream);
}

extern "C" int bgk_adam_step_clipped(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                                     float weight_decay, int64_t step, const int32_t* skip_flag, int32_t* skipped_count,
                                     const double* grad_sumsq, float max_norm, void* stream) {
    BGK_CHECK_ARG(grad_sumsq && max_norm == max_norm && max_norm >= 0.0f, "bgk_adam_step_clipped: needs the gradient's sum of squares and a max_norm >= 0");
    return adam_launch("bgk_adam_step_clipped", p, g, m, v, n, lr, beta1, beta2, eps, weight_decay, step, skip_flag, skipped_count, grad_sumsq,
                       max_norm, stream);
}
