/* bgk_moments.hip -- per-column count / mean / unbiased std / min / max of a tall row-major f32 matrix in ONE pass over it:
 * replaces `values.min/max/mean/std(axis=0)` of `factory/icmarginals.py:126-157` (four passes per IC field in the reference,
 * over data sets of 1e5 .. 1e7 frames).  Roofline: HBM, 4 B per element read once.
 *
 * Arithmetic: f64 shifted sums S1 = sum(x - K), S2 = sum((x - K)^2) with K a value of the column itself (the first one the
 * accumulating thread sees), so |x - K| is of the size of the column's spread and nothing is lost to cancellation at
 * 0.1 +- 0.003 over 1e7 rows (or 1000 +- 0.001).  Two accumulators with different K are merged exactly by shifting one onto the
 * other's K (d = Kb - Ka: S1 += S1b + nb d, S2 += S2b + 2 d S1b + nb d^2).  No raw sum of squares anywhere.
 * Determinism: fixed rows -> block partition, fixed rows -> thread mapping, every merge in a fixed order, no atomics.
 *
 * Stage 1 (moments_partial_kernel): lanes run over the FLAT element index of a tile of R = 256 / P whole rows, so a wave reads
 * consecutive addresses (ldx == P) and every thread keeps ONE column for the whole block (the tile advances by whole rows): its
 * six values live in registers; the R threads of a column are merged in row-group order through LDS at the end of the block.
 * Columns beyond 256 are taken 256 at a time (one row segment of 1 KiB per step).
 * Stage 2 (moments_merge_kernel): the block partials of a column, 16 segments per column merged in block order, then the 16
 * segment results in segment order, then onto the caller's running state [P, 6] = {n, K, S1, S2, min, max} under the STATE's K;
 * min / max are merged, never overwritten -- a data set larger than memory is reduced chunk by chunk.
 * Finalize (moments_finalize_kernel): mean = K + S1 / n, var = (S2 - S1^2 / n) / (n - 1) clamped at 0 (n = 1: 0 / 0 = NaN as
 * torch.std; a constant column has S1 = S2 = 0 exactly).  A NaN in the data reaches S1, S2, min and max of its column only.
 */
#include "bgk_reduce.h"

namespace {

struct Mom {
    double n, K, S1, S2, mn, mx;
};

/* a <- a merged with b, under a's K (b's when a is empty) */
__device__ __forceinline__ void mom_merge(Mom& a, const Mom& b) {
    if (b.n == 0.0) return;
    if (a.n == 0.0) { a = b; return; }
    const double d = b.K - a.K;
    a.S2 = a.S2 + (b.S2 + (2.0 * d * b.S1 + b.n * d * d));
    a.S1 = a.S1 + (b.S1 + b.n * d);
    a.n += b.n;
    a.mn = bgk_nan_min(a.mn, b.mn);         /* min / max keep a NaN once seen */
    a.mx = bgk_nan_max(a.mx, b.mx);
}

__device__ __forceinline__ Mom mom_load(const double* p) { return Mom{p[0], p[1], p[2], p[3], p[4], p[5]}; }
__device__ __forceinline__ void mom_store(double* p, const Mom& m) {
    p[0] = m.n; p[1] = m.K; p[2] = m.S1; p[3] = m.S2; p[4] = m.mn; p[5] = m.mx;
}

struct Acc {
    double K, S1, S2;
    float mn, mx;
    __device__ __forceinline__ void add(float v) {
        const double d = (double)v - K;
        S1 += d;
        S2 = __builtin_fma(d, d, S2);
        mn = bgk_nan_min(mn, v);
        mx = bgk_nan_max(mx, v);
    }
};

__global__ __launch_bounds__(256) void moments_partial_kernel(const float* __restrict__ x, int64_t ldx, int64_t B, int P,
                                                              int64_t rows_per_block, double* __restrict__ partial) {
    __shared__ double s[6][256];
    const int t = threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
    const int64_t r1 = (r0 + rows_per_block) < B ? (r0 + rows_per_block) : B;
    for (int c0 = 0; c0 < P; c0 += 256) {
        const int Pw = (P - c0) < 256 ? (P - c0) : 256;     /* columns of this tile */
        const int R = 256 / Pw;                             /* whole rows per step */
        const int rr = t / Pw, c = c0 + (t - rr * Pw);
        Acc a = {0.0, 0.0, 0.0, 0.0f, 0.0f};
        int64_t n = 0;
        if (rr < R) {
            const float* px = x + c;
            int64_t row = r0 + rr;
            if (row < r1) {                                 /* the thread's first value is its K */
                const float v = px[row * ldx];
                a.K = (double)v; a.mn = v; a.mx = v;
                n = 1;
                row += R;
            }
            for (; row + 3 * (int64_t)R < r1; row += 4 * (int64_t)R) {
                const float v0 = px[row * ldx];
                const float v1 = px[(row + R) * ldx];
                const float v2 = px[(row + 2 * (int64_t)R) * ldx];
                const float v3 = px[(row + 3 * (int64_t)R) * ldx];
                a.add(v0); a.add(v1); a.add(v2); a.add(v3);
                n += 4;
            }
            for (; row < r1; row += R) { a.add(px[row * ldx]); ++n; }
        }
        s[0][t] = (double)n; s[1][t] = a.K; s[2][t] = a.S1; s[3][t] = a.S2; s[4][t] = (double)a.mn; s[5][t] = (double)a.mx;
        __syncthreads();
        if (t < Pw) {                                       /* row groups 0 .. R-1 of column c, in that order */
            Mom m = {s[0][t], s[1][t], s[2][t], s[3][t], s[4][t], s[5][t]};
            for (int g = 1; g < R; ++g) {
                const int u = g * Pw + t;
                mom_merge(m, Mom{s[0][u], s[1][u], s[2][u], s[3][u], s[4][u], s[5][u]});
            }
            mom_store(partial + ((int64_t)blockIdx.x * P + c) * 6, m);
        }
        __syncthreads();
    }
}

/* 16 columns x 16 block segments per workgroup */
__global__ __launch_bounds__(256) void moments_merge_kernel(const double* __restrict__ partial, int nblk, int P, double* __restrict__ state) {
    __shared__ double s[6][256];
    const int t = threadIdx.x;
    const int cl = t & 15, seg = t >> 4;
    const int col = blockIdx.x * 16 + cl;
    const int per = (nblk + 15) / 16;
    const int b0 = seg * per, b1 = (b0 + per) < nblk ? (b0 + per) : nblk;
    Mom m = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (col < P)
        for (int b = b0; b < b1; ++b) mom_merge(m, mom_load(partial + ((int64_t)b * P + col) * 6));
    s[0][t] = m.n; s[1][t] = m.K; s[2][t] = m.S1; s[3][t] = m.S2; s[4][t] = m.mn; s[5][t] = m.mx;
    __syncthreads();
    if (seg == 0 && col < P) {
        Mom st = mom_load(state + (int64_t)col * 6);        /* the running state keeps its K */
        for (int g = 0; g < 16; ++g) {
            const int u = g * 16 + cl;
            mom_merge(st, Mom{s[0][u], s[1][u], s[2][u], s[3][u], s[4][u], s[5][u]});
        }
        mom_store(state + (int64_t)col * 6, st);
    }
}

/* out [5, P]: count, mean, std (divisor n - 1), min, max */
__global__ __launch_bounds__(256) void moments_finalize_kernel(const double* __restrict__ state, int P, double* __restrict__ out) {
    const int col = blockIdx.x * 256 + threadIdx.x;
    if (col >= P) return;
    const Mom m = mom_load(state + (int64_t)col * 6);
    const double mean_shift = m.S1 / m.n;
    double var = (m.S2 - m.S1 * mean_shift) / (m.n - 1.0);
    var = var < 0.0 ? 0.0 : var;                            /* (a NaN stays a NaN) */
    out[col] = m.n;
    out[(int64_t)P + col] = m.K + mean_shift;
    out[2 * (int64_t)P + col] = __builtin_sqrt(var);
    out[3 * (int64_t)P + col] = m.mn;
    out[4 * (int64_t)P + col] = m.mx;
}

}  // namespace

extern "C" int bgk_column_moments_update(const float* x, int64_t ldx, int64_t B, int32_t P, double* partial, int32_t nblk,
                                         double* state, void* stream) {
    if (B == 0) return 0;       /* nothing to merge: the state stays as it is (x has no storage) */
    BGK_CHECK_ARG(x && partial && state, "bgk_column_moments_update: null pointer");
    BGK_CHECK_ARG(B > 0 && P > 0 && nblk > 0 && ldx >= P, "bgk_column_moments_update: bad sizes");
    hipStream_t st = (hipStream_t)stream;
    const int64_t rpb = (B + nblk - 1) / nblk;
    hipLaunchKernelGGL(moments_partial_kernel, dim3(nblk), dim3(256), 0, st, x, ldx, B, (int)P, rpb > 0 ? rpb : 1, partial);
    hipLaunchKernelGGL(moments_merge_kernel, dim3((P + 15) / 16), dim3(256), 0, st, partial, (int)nblk, (int)P, state);
    return bgk_launch_status("bgk_column_moments_update");
}

extern "C" int bgk_column_moments_finalize(const double* state, int32_t P, int64_t n_rows, double* out, void* stream) {
    BGK_CHECK_ARG(n_rows > 0, "bgk_column_moments_finalize: no rows were accumulated (n = 0): the statistics are undefined");
    BGK_CHECK_ARG(state && out, "bgk_column_moments_finalize: null pointer");
    BGK_CHECK_ARG(P > 0, "bgk_column_moments_finalize: bad sizes");
    hipLaunchKernelGGL(moments_finalize_kernel, dim3((P + 255) / 256), dim3(256), 0, (hipStream_t)stream, state, (int)P, out);
    return bgk_launch_status("bgk_column_moments_finalize");
}
