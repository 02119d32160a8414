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
 * Like bgk_mcmc.hip, by the rules of bgk_pair_tile.h: one wave per workgroup, ONE LANE PER SAMPLE, a tile of rows staged coalesced through
 * LDS at the odd row stride S, the steps in lockstep across the wave, the final q / v as coalesced tile stores, no atomics, a fixed
 * summation order.  The scalars (h, sqrt(2 h), c1, ...) are formed in f64 on the host and
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
 * Backward (training through the layers; stochastic.py's _BrownianFn / _LangevinFn).  The forward with the template flag RECORD also
 * stores the tile after every step, coalesced (traj_q / traj_v [n_steps, B, n d]); q, v, dW are the non-recording launch's bits.
 * pair_langevin_bwd_kernel sweeps a recorded segment in reverse for the loss L with d L / d dW[b] = gamma, same lane mapping and tiles
 * of stride S, a fixed order, no atomics; H = d^2 e / d x^2 through bgk_pair_row_hvp of bgk_pair_terms.h.  Three running vectors per
 * sample live in LDS over the sweep and in gq, gv, carry [B, n d] between launches (last segment first):
 *   Brownian   w_k_ = (x_k - x_(k+1) + h g_(k+1)) / r, r = sqrt(2 h);  a_k = -gamma w_k_ / r, a_(-1) = a_K = 0;
 *              L_k = L_(k+1) + a_k - a_(k-1) - h H(x_k) (L_(k+1) - a_(k-1)),  L_K = g_y - a_(K-1) + h H(x_K) a_(K-1)
 *              kept as gq = L_(k+1) + a_k, carry = L_(k+1) (start: g_y, 0).  State k: g_k (one gradient) for a_(k-1), u = carry - a_(k-1),
 *              H(x_k) u (one product), L_k = (gq - a_(k-1)) - h H u, carry = L_k, gq = L_k + a_(k-1).  No noise is needed.
 *   Langevin   per step in reverse, b1 = w2 - fac2 v_(k+1), b2 = w1 - fac2 v_k:  Lv += gamma fac2 b1,  p = c2 Lv,  Lq -= c1 H(q_(k+1)) p,
 *              Lvh = p + h Lq,  Lv_k = (1 - c1 gm) Lvh + gamma fac2 b2,  Lq_k = Lq - c1 H(q_k) Lvh.  The two products at one state are
 *              one, with the vector c1 (Lvh_k + p_(k-1)); gq = Lq, gv = Lv, carry = Lvh (start: g_q, g_v, 0).  State j: Lv += ..b1 and p of
 *              step j - 1, carry = c1 (carry + p), Lq -= H(q_j) carry, then Lvh, Lv of step j - 1.  The noise: w1 / w2, or Philox as the
 *              forward drew it.
 * A launch handles the states n_steps .. 1 of its segment (0: the state before it, j > 0: frame j - 1) and, for the run's first
 * segment, state 0; every state by one launch, with the same operations whatever the split: the gradients do not depend on it.
 * Tiles (5 for either): X the state q_j (Langevin: then v_(j-1));  Y x_(j-1) / v_j, then H u;  GQ;  GV (Brownian: g_j, then a_(j-1));
 * GC the carry = the product's vector.  States are staged coalesced per state (barriers around them, uniform over the wave).
 * Rows per tile = the most (<= 64) with 5 rows S 4 B within the dynamic LDS:
 *                 n d = 192 (S = 193)       LJ13, n d = 39 (S = 39)     DW4, n d = 8 (S = 9)
 *   backward      16 rows, 61,760 B         64 rows, 49,920 B           64 rows, 11,520 B
 *
 * Envelope: bgk_pair_tile.h. */
#include "bgk_common.h"
#include "bgk_pair_terms.h"
#include "bgk_philox.h"

namespace {

constexpr int LG_LDS_DYNAMIC = 63488;

struct LgArgs {
    float* q; float* v; int64_t B, row0;
    BgkPairTarget t; int rows;
    float h, sq2h, c1, c2, gm, fac1, fac2; int n_steps;
    const float* w1; const float* w2;
    uint32_t seed_lo, seed_hi, offset;
    float* dW; int accumulate;
    float* traj_q; float* traj_v;                      /* RECORD: the state after every step [n_steps, B, n d] */
};

template <int D, int KIND, bool LANGEVIN, bool RECORD>
__global__ __launch_bounds__(BGK_TILE_THREADS) void pair_langevin_kernel(LgArgs a) {
    extern __shared__ float s_mem[];
    const int tid = threadIdx.x, nd = a.t.nd, S = nd | 1;
    const int T = a.rows * S;                                          /* words of one tile */
    const int64_t n_tiles = (a.B + a.rows - 1) / a.rows;
    for (int64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const int64_t b0 = t * a.rows;
        const int rows = (int)((a.B - b0) < a.rows ? (a.B - b0) : a.rows);
        for (int i = tid; i < rows * nd; i += BGK_TILE_THREADS) {     /* tile_stage of q and v in one pass: one row split for both */
            const int r = (int)__umulhi((unsigned)i, a.t.magic), c = i - r * nd;
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
        if (active) bgk_pair_row_gradient<D, KIND>(s_mem + ox + tid * S, s_mem + of + tid * S, a.t);
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
                        philox_field_normal4(n1, nd, cb, r_lo, r_hi, 0u, off, a.seed_lo, a.seed_hi, w);
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
                    bgk_pair_row_gradient<D, KIND>(xb, gg, a.t);
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
                        philox_field_normal4(n1, nd, cb, r_lo, r_hi, 0u, off, a.seed_lo, a.seed_hi, w);
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
                    bgk_pair_row_gradient<D, KIND>(qr, gg, a.t);
                    for (int cb = 0; 4 * cb < nd; ++cb) {
                        float w[4];
                        philox_field_normal4(n2, nd, cb, r_lo, r_hi, 1u, off, a.seed_lo, a.seed_hi, w);
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
            if (RECORD) {                                              /* the state after the step, as coalesced tile stores */
                __syncthreads();
                const int64_t f0 = ((int64_t)step * a.B + b0) * nd;
                const int oq = LANGEVIN ? 0 : oy;
                for (int i = tid; i < rows * nd; i += BGK_TILE_THREADS) {
                    const int r = (int)__umulhi((unsigned)i, a.t.magic), c = i - r * nd;
                    a.traj_q[f0 + i] = s_mem[oq + r * S + c];
                    if (LANGEVIN) a.traj_v[f0 + i] = s_mem[T + r * S + c];
                }
                __syncthreads();
            }
            if (!LANGEVIN) { const int sx = ox; ox = oy; oy = sx; }
            const int sf = of; of = og; og = sf;
        }
        __syncthreads();
        for (int i = tid; i < rows * nd; i += BGK_TILE_THREADS) {     /* tile_store of q and v in one pass */
            const int r = (int)__umulhi((unsigned)i, a.t.magic), c = i - r * nd;
            a.q[(b0 + r) * nd + c] = s_mem[ox + r * S + c];
            if (LANGEVIN) a.v[(b0 + r) * nd + c] = s_mem[T + r * S + c];
        }
        if (active) a.dW[b] = a.accumulate ? a.dW[b] + (float)dw : (float)dw;
        __syncthreads();
    }
}

/* ---- the adjoint sweep over a recorded segment (header: "Backward") ---- */
struct LbArgs {
    const float* q0; const float* v0; const float* traj_q; const float* traj_v; int64_t B, row0;
    BgkPairTarget t; int rows;
    float h, sq2h, c1, c2, omg, fac2; int n_steps;
    const float* w1; const float* w2;
    uint32_t seed_lo, seed_hi, offset;
    const float* g_dW; float* gq; float* gv; float* carry; int first;
};

template <int D, int KIND, bool LANGEVIN>
__global__ __launch_bounds__(BGK_TILE_THREADS) void pair_langevin_bwd_kernel(LbArgs a) {
    extern __shared__ float s_mem[];
    const int tid = threadIdx.x, nd = a.t.nd, S = nd | 1;
    const int T = a.rows * S;
    const uint32_t magic = a.t.magic;
    const int64_t n_tiles = (a.B + a.rows - 1) / a.rows;
    const int64_t frame = a.B * (int64_t)nd;
    float* s_x = s_mem;                 /* the state q_j; Langevin: then v_(j-1) */
    float* s_y = s_mem + T;             /* Brownian x_(j-1), Langevin v_j; then H u */
    float* s_gq = s_mem + 2 * T;
    float* s_gv = s_mem + 3 * T;        /* Langevin: the velocity adjoint; Brownian: g_j, then a_(j-1) */
    float* s_gc = s_mem + 4 * T;        /* the carry; the vector of the Hessian product */
    for (int64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const int64_t b0 = t * a.rows;
        const int rows = (int)((a.B - b0) < a.rows ? (a.B - b0) : a.rows);
        tile_stage(a.gq, b0, rows, nd, magic, s_gq);
        tile_stage(a.carry, b0, rows, nd, magic, s_gc);
        if (LANGEVIN) tile_stage(a.gv, b0, rows, nd, magic, s_gv);
        const bool active = tid < rows;
        const int64_t b = b0 + (active ? tid : 0);
        const uint64_t grow = (uint64_t)(a.row0 + b);
        const uint32_t r_lo = (uint32_t)grow, r_hi = (uint32_t)(grow >> 32);
        const float gamma = a.g_dW[b], gf2 = gamma * a.fac2;
        float* xr = s_x + tid * S;
        float* yr = s_y + tid * S;
        float* gq = s_gq + tid * S;
        float* gv = s_gv + tid * S;
        float* gc = s_gc + tid * S;
        for (int j = a.n_steps; j >= (a.first ? 0 : 1); --j) {       /* state j of the segment: 0 the state before it, j > 0 frame j - 1 */
            __syncthreads();
            tile_stage(j > 0 ? a.traj_q + (int64_t)(j - 1) * frame : a.q0, b0, rows, nd, magic, s_x);
            if (j > 0) {
                if (LANGEVIN) tile_stage(a.traj_v + (int64_t)(j - 1) * frame, b0, rows, nd, magic, s_y);
                else tile_stage(j > 1 ? a.traj_q + (int64_t)(j - 2) * frame : a.q0, b0, rows, nd, magic, s_y);
            }
            __syncthreads();
            const uint32_t off = a.offset + (uint32_t)(j - 1);         /* the step that led to state j */
            const float* n1 = (a.w1 && j > 0) ? a.w1 + ((int64_t)(j - 1) * a.B + b) * nd : nullptr;
            const float* n2 = (a.w2 && j > 0) ? a.w2 + ((int64_t)(j - 1) * a.B + b) * nd : nullptr;
            if (active) {
                if (!LANGEVIN) {
                    if (j > 0) {
                        bgk_pair_row_gradient<D, KIND>(xr, gv, a.t);
                        for (int c = 0; c < nd; ++c) {
                            const float wb = ((yr[c] - xr[c]) - a.h * (-gv[c])) / a.sq2h;     /* the forward's w_ of step j - 1 */
                            const float am = -(gamma * wb) / a.sq2h;                          /* a_(j-1) */
                            gv[c] = am; gc[c] = gc[c] - am;
                        }
                    }
                    bgk_pair_row_hvp<D, KIND, false>(xr, gc, nullptr, yr, a.t);
                    for (int c = 0; c < nd; ++c) {
                        const float am = j > 0 ? gv[c] : 0.0f;
                        const float lam = (gq[c] - am) - a.h * yr[c];
                        gc[c] = lam; gq[c] = lam + am;
                    }
                } else {
                    if (j > 0) {
                        for (int cb = 0; 4 * cb < nd; ++cb) {
                            float w[4];
                            philox_field_normal4(n2, nd, cb, r_lo, r_hi, 1u, off, a.seed_lo, a.seed_hi, w);
#pragma unroll
                            for (int k = 0; k < 4; ++k) {
                                const int c = 4 * cb + k;
                                if (c < nd) {
                                    const float lv = gv[c] + gf2 * (w[k] - a.fac2 * yr[c]);
                                    gv[c] = lv; gc[c] = a.c1 * (gc[c] + a.c2 * lv);
                                }
                            }
                        }
                    } else {
                        for (int c = 0; c < nd; ++c) gc[c] = a.c1 * gc[c];
                    }
                    bgk_pair_row_hvp<D, KIND, false>(xr, gc, nullptr, yr, a.t);
                    for (int c = 0; c < nd; ++c) gq[c] -= yr[c];
                }
            }
            if (LANGEVIN && j > 0) {
                __syncthreads();
                tile_stage(j > 1 ? a.traj_v + (int64_t)(j - 2) * frame : a.v0, b0, rows, nd, magic, s_x);
                __syncthreads();
                if (active) {
                    for (int cb = 0; 4 * cb < nd; ++cb) {
                        float w[4];
                        philox_field_normal4(n1, nd, cb, r_lo, r_hi, 0u, off, a.seed_lo, a.seed_hi, w);
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            const int c = 4 * cb + k;
                            if (c < nd) {
                                const float vh = a.c2 * gv[c] + a.h * gq[c];
                                gc[c] = vh; gv[c] = a.omg * vh + gf2 * (w[k] - a.fac2 * xr[c]);
                            }
                        }
                    }
                }
            }
        }
        __syncthreads();
        tile_store(a.gq, b0, rows, nd, magic, s_gq);
        tile_store(a.carry, b0, rows, nd, magic, s_gc);
        if (LANGEVIN) tile_store(a.gv, b0, rows, nd, magic, s_gv);
        __syncthreads();
    }
}

/* what the three entries share, in their order: the target as the entry names it (bgk_pair_spec), the integrator and the noise */
struct BgkLangevinCall {
    BgkPairSpec spec;
    int64_t B;
    double stepsize, mass, gamma, kT; int32_t n_steps;
    const float* w1; const float* w2; uint64_t seed; uint32_t offset; int64_t row0;
    void* stream;
};

/* the checks every entry shares; fills *t */
int langevin_check(const BgkLangevinCall& c, bool langevin, BgkPairTarget* t) {
    const char* what = c.spec.what;
    BGK_CHECK_ARG(c.B >= 0 && c.row0 >= 0 && c.n_steps >= 0, "%s: bad batch size / row0 / n_steps", what);
    const int st = bgk_pair_target(c.spec, t);
    if (st) return st;
    BGK_CHECK_ARG(c.stepsize > 0.0 && c.stepsize < INFINITY, "%s: the step size must be positive and finite", what);
    BGK_CHECK_ARG(c.mass > 0.0 && c.gamma >= 0.0 && c.kT > 0.0, "%s: mass and kT must be positive, gamma not negative", what);
    BGK_CHECK_ARG(!c.w2 || (c.w1 && langevin), "%s: w2 goes with w1 and with velocities", what);
    BGK_CHECK_ARG(!(langevin && c.w1) || c.w2, "%s: with velocities w1 and w2 go together", what);
    return 0;
}

/* v: Langevin, else Brownian; traj_q (traj_v): the recording kernel */
int langevin_forward(const BgkLangevinCall& c, float* q, float* v, float* dW, int32_t accumulate, float* traj_q, float* traj_v) {
    const char* what = c.spec.what;
    const bool langevin = v != nullptr, record = traj_q != nullptr;
    LgArgs a{};
    const int st = langevin_check(c, langevin, &a.t);
    if (st) return st;
    if (c.B == 0) return 0;
    BGK_CHECK_ARG(q && dW, "%s: null tensor", what);
    a.q = q; a.v = v; a.B = c.B; a.row0 = c.row0;
    const int bytes_per_row = (langevin ? 5 : 4) * (a.t.nd | 1) * (int)sizeof(float);
    a.rows = rows_within(LG_LDS_DYNAMIC, bytes_per_row);
    const double gm = c.gamma * c.mass;
    a.h = (float)c.stepsize; a.sq2h = (float)sqrt(2.0 * c.stepsize);
    a.c1 = (float)(c.stepsize / (2.0 * c.mass)); a.c2 = (float)(1.0 / (1.0 + c.gamma * c.stepsize / 2.0)); a.gm = (float)gm;
    a.fac1 = (float)sqrt(4.0 * gm * c.kT / c.stepsize); a.fac2 = (float)sqrt(gm * c.stepsize / c.kT);
    a.n_steps = c.n_steps; a.w1 = c.w1; a.w2 = c.w2;
    a.seed_lo = (uint32_t)c.seed; a.seed_hi = (uint32_t)(c.seed >> 32); a.offset = c.offset;
    a.dW = dW; a.accumulate = accumulate != 0;
    a.traj_q = traj_q; a.traj_v = traj_v;
    const size_t lds = (size_t)a.rows * bytes_per_row;
    const int grid = tile_grid(c.B, a.rows);
    hipStream_t s = (hipStream_t)c.stream;
    tile_dispatch<false>(c.spec.kind, c.spec.n_dims, [&](auto D, auto K) {
        if (langevin && record) tile_launch(pair_langevin_kernel<D(), K(), true, true>, grid, lds, s, a);
        else if (langevin) tile_launch(pair_langevin_kernel<D(), K(), true, false>, grid, lds, s, a);
        else if (record) tile_launch(pair_langevin_kernel<D(), K(), false, true>, grid, lds, s, a);
        else tile_launch(pair_langevin_kernel<D(), K(), false, false>, grid, lds, s, a);
    });
    return bgk_launch_status(what);
}

}  // namespace

extern "C" int bgk_pair_langevin(float* q, float* v, int64_t B, int32_t n_particles, int32_t n_dims, int32_t kind,
                                 double p0, double p1, double p2, double p3, double osc_scale,
                                 double stepsize, double mass, double gamma, double kT, int32_t n_steps,
                                 const float* w1, const float* w2, uint64_t seed, uint32_t offset, int64_t row0,
                                 float* dW, int32_t accumulate, void* stream) {
    const BgkPairSpec spec = bgk_pair_spec("bgk_pair_langevin", n_particles, n_dims, kind, p0, p1, p2, p3, osc_scale);
    return langevin_forward({spec, B, stepsize, mass, gamma, kT, n_steps, w1, w2, seed, offset, row0, stream}, q, v, dW, accumulate,
                            nullptr, nullptr);
}

extern "C" int bgk_pair_langevin_record(float* q, float* v, int64_t B, int32_t n_particles, int32_t n_dims, int32_t kind,
                                        double p0, double p1, double p2, double p3, double osc_scale,
                                        double stepsize, double mass, double gamma, double kT, int32_t n_steps,
                                        const float* w1, const float* w2, uint64_t seed, uint32_t offset, int64_t row0,
                                        float* dW, int32_t accumulate, float* traj_q, float* traj_v, void* stream) {
    BGK_CHECK_ARG(B == 0 || (traj_q && (traj_v != nullptr) == (v != nullptr)),
                  "bgk_pair_langevin_record: traj_q [n_steps, B, n d], and traj_v exactly with velocities");
    const BgkPairSpec spec = bgk_pair_spec("bgk_pair_langevin_record", n_particles, n_dims, kind, p0, p1, p2, p3, osc_scale);
    return langevin_forward({spec, B, stepsize, mass, gamma, kT, n_steps, w1, w2, seed, offset, row0, stream}, q, v, dW, accumulate,
                            traj_q, traj_v);
}

extern "C" int bgk_pair_langevin_backward(const float* q0, const float* v0, const float* traj_q, const float* traj_v, int64_t B,
                                          int32_t n_particles, int32_t n_dims, int32_t kind,
                                          double p0, double p1, double p2, double p3, double osc_scale,
                                          double stepsize, double mass, double gamma, double kT, int32_t n_steps,
                                          const float* w1, const float* w2, uint64_t seed, uint32_t offset, int64_t row0,
                                          const float* g_dW, float* gq, float* gv, float* carry, int32_t first, void* stream) {
    const char* what = "bgk_pair_langevin_backward";
    const BgkLangevinCall c{bgk_pair_spec(what, n_particles, n_dims, kind, p0, p1, p2, p3, osc_scale), B, stepsize, mass, gamma, kT, n_steps,
                            w1, w2, seed, offset, row0, stream};
    const bool langevin = v0 != nullptr;
    LbArgs a{};
    const int st = langevin_check(c, langevin, &a.t);
    if (st) return st;
    if (B == 0) return 0;
    BGK_CHECK_ARG(q0 && g_dW && gq && carry && (traj_q || n_steps == 0), "%s: null tensor", what);
    BGK_CHECK_ARG(langevin ? ((traj_v || n_steps == 0) && gv) : (!traj_v && !gv), "%s: traj_v and gv exactly with velocities", what);
    a.q0 = q0; a.v0 = v0; a.traj_q = traj_q; a.traj_v = traj_v; a.B = B; a.row0 = row0;
    const int bytes_per_row = 5 * (a.t.nd | 1) * (int)sizeof(float);
    a.rows = rows_within(LG_LDS_DYNAMIC, bytes_per_row);
    const double c1 = stepsize / (2.0 * mass), gm = gamma * mass;
    a.h = (float)stepsize; a.sq2h = (float)sqrt(2.0 * stepsize);
    a.c1 = (float)c1; a.c2 = (float)(1.0 / (1.0 + gamma * stepsize / 2.0)); a.omg = (float)(1.0 - c1 * gm);
    a.fac2 = (float)sqrt(gm * stepsize / kT);
    a.n_steps = n_steps; a.w1 = w1; a.w2 = w2;
    a.seed_lo = (uint32_t)seed; a.seed_hi = (uint32_t)(seed >> 32); a.offset = offset;
    a.g_dW = g_dW; a.gq = gq; a.gv = gv; a.carry = carry; a.first = first != 0;
    const size_t lds = (size_t)a.rows * bytes_per_row;
    const int grid = tile_grid(B, a.rows);
    hipStream_t s = (hipStream_t)stream;
    tile_dispatch<false>(kind, n_dims, [&](auto D, auto K) {
        if (langevin) tile_launch(pair_langevin_bwd_kernel<D(), K(), true>, grid, lds, s, a);
        else tile_launch(pair_langevin_bwd_kernel<D(), K(), false>, grid, lds, s, a);
    });
    return bgk_launch_status(what);
}
