/* bgk_langevin.hip -- Brownian and Langevin dynamics with the path-probability ratio dW on a particle-system target, a whole run of steps
 * in one launch.  BrownianFlow._forward and LangevinFlow._forward (bgflow/nn/flow/stochastic/langevin.py:32-45, 86-118) on the targets of
 * bgk_pair.hip (kind 0 Lennard-Jones, 1 multi-double-well, 2 mean-free normal), f = -d e / d x at temperature 1, h = stepsize:
 *   Brownian   y = x + h f(x) + sqrt(2 h) w,  w_ = (x - y - h f(y)) / sqrt(2 h),  dW += 0.5 sum (w^2 - w_^2)
 *   Langevin   vh = v1 + c1 (f(q1) - gm v1 + fac1 w1),  q2 = q1 + h vh,  v2 = c2 (vh + c1 (f(q2) + fac1 w2)),
 *              w1_ = w2 - fac2 v2,  w2_ = w1 - fac2 v1,  dW += 0.5 sum (w1^2 + w2^2 - w1_^2 - w2_^2)
 *              gm = gamma mass, c1 = h / (2 mass), c2 = 1 / (1 + gamma h / 2), fac1 = sqrt(4 gm kT / h), fac2 = sqrt(gm h / kT)
 * In stock ops a step is a randn (two), two force calls (autograd through the energy) and about ten elementwise ops and reductions over a
 * state of n d <= 192 floats per sample; here the state never leaves LDS between the first and the last step.
 *
 * Like bgk_mcmc.hip: one wave per workgroup, ONE LANE PER SAMPLE, a tile of rows staged coalesced through LDS with the odd row stride
 * S = (n d) | 1 (lane r reads word r S + k: distinct banks within a 32-lane group), the steps in lockstep across the wave, the final q / v
 * as coalesced tile stores, no atomics, a fixed summation order.  The scalars (h, sqrt(2 h), c1, ...) are formed in f64 on the host and
 * rounded to f32 once, as torch does with a python number that meets an f32 tensor.
 *
 * Force: bgk_pair_row_gradient of bgk_pair_terms.h -- the code of pair_energy_bwd_kernel -- into the lane's own row of a force tile; the
 * kernel uses its negative.  f(y) of step k is f(x) of step k + 1 (the evaluation is deterministic: the same bits), so a step costs ONE
 * force evaluation, plus one at the start of the launch; the two force tiles swap roles after every step.
 *
 * Arithmetic: the elementwise terms in f32 in the reference's order of operations -- w_ from the rounded x - y, not from the algebraic
 * simplification -- the row sum of the (w^2 - w_^2) terms of a step and the running dW in f64, rounded once at the end (accumulate != 0
 * then adds to dW in f32).  Non-finite values propagate as in the reference.
 *
 * LDS tiles of rows x S floats (all lanes address the same tile at the same time, so the tiles simply follow one another):
 *   Brownian  A: x, overwritten elementwise by x - y    B: y    Fa: d e / d x (x), overwritten by w    Fb: d e / d x (y)
 *             after the step (A, B) and (Fa, Fb) swap roles
 *   Langevin  Q: q1 -> q2 in place    V: v1 -> vh -> v2    F: d e / d x (q1), overwritten by w1    G: d e / d x (q2)    T: w2_
 *             after the step F and G swap roles
 * Dynamic LDS <= 63,488 B: rows per tile = the most (<= 64) with (4 or 5) rows S 4 B within it; lanes beyond the rows only stage and store:
 *                 n d = 192 (S = 193)       LJ13, n d = 39 (S = 39)     DW4, n d = 8 (S = 9)
 *   Brownian      20 rows, 61,760 B         64 rows, 39,936 B           64 rows,  9,216 B
 *   Langevin      16 rows, 61,760 B         64 rows, 49,920 B           64 rows, 11,520 B
 *
 * Random numbers: explicit (w1 and, for Langevin, w2 [n_steps, B, n d], read by the sample's lane) or drawn in the kernel from
 * Philox4x32-10 in the counter layout of bgk_philox.h: counter = (global row low, high, field << 20 | 4-column block, offset + step),
 * field 0 = w / w1, field 1 = w2 (n d Box-Muller normals each).  The stream is a pure function of (seed, step, global row, column): the
 * same bits whatever the tiling, the grid, row0 sharding or the split of a run into launches, and the bits bgk_philox_fields writes for
 * (seed, offset + step) with fields [normal n d, normal n d].
 *
 * Envelope 2 <= n <= 64, 1 <= d <= 3. */
#include "bgk_common.h"
#include "bgk_pair_terms.h"
#include "bgk_philox.h"

namespace {

constexpr int LG_THREADS = 64;
constexpr int LG_MAX_N = 64, LG_MAX_D = 3;
constexpr int LG_LDS_DYNAMIC = 63488;
constexpr int LG_MAX_GRID = 256 * 16;

struct LgArgs {
    float* q; float* v; int64_t B, row0;
    int n, nd, rows; uint32_t magic;
    float p0, p1, p2, p3, osc;
    float h, sq2h, c1, c2, gm, fac1, fac2; int n_steps;
    const float* w1; const float* w2;
    uint32_t seed_lo, seed_hi, offset;
    float* dW; int accumulate;
};

/* the four normals of columns 4 cb .. 4 cb + 3 of a field: the explicit row (columns beyond n d: 0) or the Philox block */
__device__ __forceinline__ void lg_normal4(const float* row, int nd, int cb, uint32_t r_lo, uint32_t r_hi, uint32_t field, uint32_t off,
                                           uint32_t k0, uint32_t k1, float (&w)[4]) {
    if (row) {
#pragma unroll
        for (int j = 0; j < 4; ++j) w[j] = 4 * cb + j < nd ? row[4 * cb + j] : 0.0f;
    } else {
        uint32_t o[4];
        philox4x32_10(r_lo, r_hi, (field << 20) | (uint32_t)cb, off, k0, k1, o);
        philox_normal4(o, w);
    }
}

template <int D, int KIND, bool LANGEVIN>
__global__ __launch_bounds__(LG_THREADS) void pair_langevin_kernel(LgArgs a) {
    extern __shared__ float s_mem[];
    const int tid = threadIdx.x, n = a.n, nd = a.nd, S = a.nd | 1;
    const int T = a.rows * S;                                          /* words of one tile */
    const float rm2 = a.p1 * a.p1, c12 = -12.0f * a.p0 / rm2;
    const int64_t n_tiles = (a.B + a.rows - 1) / a.rows;
    for (int64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const int64_t b0 = t * a.rows;
        const int rows = (int)((a.B - b0) < a.rows ? (a.B - b0) : a.rows);
        for (int i = tid; i < rows * nd; i += LG_THREADS) {
            const int r = (int)__umulhi((unsigned)i, a.magic), c = i - r * nd;
            s_mem[r * S + c] = a.q[(b0 + r) * nd + c];
            if (LANGEVIN) s_mem[T + r * S + c] = a.v[(b0 + r) * nd + c];
        }
        __syncthreads();
        const bool active = tid < rows;
        const int64_t b = b0 + (active ? tid : 0);
        const uint64_t grow = (uint64_t)(a.row0 + b);
        const uint32_t r_lo = (uint32_t)grow, r_hi = (uint32_t)(grow >> 32);
        /* tile offsets, uniform over the wave.  Brownian: A, B, Fa, Fb; Langevin: Q (0), V (T), F, G, and T at 4 T */
        int ox = 0, oy = T, of = 2 * T, og = 3 * T;
        double dw = 0.0;
        if (active)
            bgk_pair_row_gradient<D, KIND>(s_mem + ox + tid * S, s_mem + of + tid * S, n, a.p0, a.p1, a.p3, rm2, c12, a.osc);
        for (int step = 0; step < a.n_steps; ++step) {
            if (active) {
                const uint32_t off = a.offset + (uint32_t)step;
                const float* n1 = a.w1 ? a.w1 + ((int64_t)step * a.B + b) * nd : nullptr;
                const float* n2 = a.w2 ? a.w2 + ((int64_t)step * a.B + b) * nd : nullptr;
                float* gf = s_mem + of + tid * S;                      /* d e / d x at the step's start; then w / w1 */
                float* gg = s_mem + og + tid * S;                      /* d e / d x at the step's end */
                double sum = 0.0;
                if (!LANGEVIN) {
                    float* xa = s_mem + ox + tid * S;
                    float* xb = s_mem + oy + tid * S;
                    for (int cb = 0; 4 * cb < nd; ++cb) {
                        float w[4];
                        lg_normal4(n1, nd, cb, r_lo, r_hi, 0u, off, a.seed_lo, a.seed_hi, w);
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const int c = 4 * cb + j;
                            if (c < nd) {
                                const float x = xa[c];
                                const float y = x + a.h * (-gf[c]) + a.sq2h * w[j];
                                xb[c] = y; xa[c] = x - y; gf[c] = w[j];
                            }
                        }
                    }
                    bgk_pair_row_gradient<D, KIND>(xb, gg, n, a.p0, a.p1, a.p3, rm2, c12, a.osc);
                    for (int c = 0; c < nd; ++c) {
                        const float wb = (xa[c] - a.h * (-gg[c])) / a.sq2h, w = gf[c];
                        sum += (double)(w * w - wb * wb);
                    }
                } else {
                    float* qr = s_mem + tid * S;
                    float* vr = s_mem + T + tid * S;
                    float* tr = s_mem + 4 * T + tid * S;
                    for (int cb = 0; 4 * cb < nd; ++cb) {
                        float w[4];
                        lg_normal4(n1, nd, cb, r_lo, r_hi, 0u, off, a.seed_lo, a.seed_hi, w);
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const int c = 4 * cb + j;
                            if (c < nd) {
                                const float v1 = vr[c];
                                const float vh = v1 + a.c1 * ((-gf[c]) - a.gm * v1 + a.fac1 * w[j]);
                                qr[c] = qr[c] + a.h * vh;
                                vr[c] = vh; gf[c] = w[j]; tr[c] = w[j] - a.fac2 * v1;
                            }
                        }
                    }
                    bgk_pair_row_gradient<D, KIND>(qr, gg, n, a.p0, a.p1, a.p3, rm2, c12, a.osc);
                    for (int cb = 0; 4 * cb < nd; ++cb) {
                        float w[4];
                        lg_normal4(n2, nd, cb, r_lo, r_hi, 1u, off, a.seed_lo, a.seed_hi, w);
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const int c = 4 * cb + j;
                            if (c < nd) {
                                const float v2 = a.c2 * (vr[c] + a.c1 * ((-gg[c]) + a.fac1 * w[j]));
                                const float w1b = w[j] - a.fac2 * v2, w1 = gf[c], w2b = tr[c];
                                sum += (double)(w1 * w1 + w[j] * w[j] - w1b * w1b - w2b * w2b);
                                vr[c] = v2;
                            }
                        }
                    }
                }
                dw += 0.5 * sum;
            }
            if (!LANGEVIN) { const int sx = ox; ox = oy; oy = sx; }
            const int sf = of; of = og; og = sf;
        }
        __syncthreads();
        for (int i = tid; i < rows * nd; i += LG_THREADS) {
            const int r = (int)__umulhi((unsigned)i, a.magic), c = i - r * nd;
            a.q[(b0 + r) * nd + c] = s_mem[ox + r * S + c];
            if (LANGEVIN) a.v[(b0 + r) * nd + c] = s_mem[T + r * S + c];
        }
        if (active) a.dW[b] = a.accumulate ? a.dW[b] + (float)dw : (float)dw;
        __syncthreads();
    }
}

template <int KIND, bool LANGEVIN>
void launch_langevin_d(int d, int grid, size_t lds, hipStream_t s, const LgArgs& a) {
    if (d == 1) hipLaunchKernelGGL((pair_langevin_kernel<1, KIND, LANGEVIN>), dim3(grid), dim3(LG_THREADS), lds, s, a);
    else if (d == 2) hipLaunchKernelGGL((pair_langevin_kernel<2, KIND, LANGEVIN>), dim3(grid), dim3(LG_THREADS), lds, s, a);
    else hipLaunchKernelGGL((pair_langevin_kernel<3, KIND, LANGEVIN>), dim3(grid), dim3(LG_THREADS), lds, s, a);
}

template <int KIND>
void launch_langevin(bool langevin, int d, int grid, size_t lds, hipStream_t s, const LgArgs& a) {
    if (langevin) launch_langevin_d<KIND, true>(d, grid, lds, s, a);
    else launch_langevin_d<KIND, false>(d, grid, lds, s, a);
}

}  // namespace

extern "C" int bgk_pair_langevin(float* q, float* v, int64_t B, int32_t n_particles, int32_t n_dims, int32_t kind,
                                 double p0, double p1, double p2, double p3, double osc_scale,
                                 double stepsize, double mass, double gamma, double kT, int32_t n_steps,
                                 const float* w1, const float* w2, uint64_t seed, uint32_t offset, int64_t row0,
                                 float* dW, int32_t accumulate, void* stream) {
    BGK_CHECK_ARG(B >= 0 && row0 >= 0 && n_steps >= 0, "bgk_pair_langevin: bad batch size / row0 / n_steps");
    BGK_CHECK_ARG(kind >= 0 && kind <= 2, "bgk_pair_langevin: kind %d (0 Lennard-Jones, 1 multi-double-well, 2 mean-free normal)", kind);
    if (!(n_particles >= 2 && n_particles <= LG_MAX_N && n_dims >= 1 && n_dims <= LG_MAX_D)) {
        bgk_set_error("bgk_pair_langevin: %d particles in %d dimensions are outside the kernel's envelope (2..%d particles, 1..%d dimensions)",
                      n_particles, n_dims, LG_MAX_N, LG_MAX_D);
        return BGK_EUNSUPPORTED;
    }
    BGK_CHECK_ARG(stepsize > 0.0 && stepsize < INFINITY, "bgk_pair_langevin: the step size must be positive and finite");
    BGK_CHECK_ARG(mass > 0.0 && gamma >= 0.0 && kT > 0.0, "bgk_pair_langevin: mass and kT must be positive, gamma not negative");
    BGK_CHECK_ARG(!w2 || (w1 && v), "bgk_pair_langevin: w2 goes with w1 and with velocities");
    BGK_CHECK_ARG(!(v && w1) || w2, "bgk_pair_langevin: with velocities w1 and w2 go together");
    if (B == 0) return 0;
    BGK_CHECK_ARG(q && dW, "bgk_pair_langevin: null tensor");
    const bool langevin = v != nullptr;
    LgArgs a{};
    a.q = q; a.v = v; a.B = B; a.row0 = row0; a.n = n_particles; a.nd = n_particles * n_dims;
    a.magic = (uint32_t)(((1ull << 32) + (uint64_t)a.nd - 1) / (uint64_t)a.nd);
    const int S = a.nd | 1, tiles = langevin ? 5 : 4;
    int rows = LG_THREADS;
    while (tiles * rows * S * (int)sizeof(float) > LG_LDS_DYNAMIC) --rows;
    a.rows = rows;
    a.p0 = (float)p0; a.p1 = (float)p1; a.p2 = (float)p2; a.p3 = (float)p3; a.osc = (float)osc_scale;
    const double gm = gamma * mass;
    a.h = (float)stepsize; a.sq2h = (float)sqrt(2.0 * stepsize);
    a.c1 = (float)(stepsize / (2.0 * mass)); a.c2 = (float)(1.0 / (1.0 + gamma * stepsize / 2.0)); a.gm = (float)gm;
    a.fac1 = (float)sqrt(4.0 * gm * kT / stepsize); a.fac2 = (float)sqrt(gm * stepsize / kT);
    a.n_steps = n_steps; a.w1 = w1; a.w2 = w2;
    a.seed_lo = (uint32_t)seed; a.seed_hi = (uint32_t)(seed >> 32); a.offset = offset;
    a.dW = dW; a.accumulate = accumulate != 0;
    const size_t lds = (size_t)tiles * rows * S * sizeof(float);
    const int64_t n_tiles = (B + rows - 1) / rows;
    const int grid = (int)(n_tiles < LG_MAX_GRID ? n_tiles : LG_MAX_GRID);
    hipStream_t s = (hipStream_t)stream;
    if (kind == 0) launch_langevin<0>(langevin, n_dims, grid, lds, s, a);
    else if (kind == 1) launch_langevin<1>(langevin, n_dims, grid, lds, s, a);
    else launch_langevin<2>(langevin, n_dims, grid, lds, s, a);
    return bgk_launch_status("bgk_pair_langevin");
}
