/* bgk_anneal.hip -- annealed switching between two particle-system targets: Metropolis chains whose energy moves from target A to
 * target B along a schedule, with the nonequilibrium work of every chain, a whole protocol in one launch.  The producer of the forward /
 * reverse work that bgk_bar.hip consumes, and annealed importance sampling (the log weight of a chain is -work).
 *
 * Definitions (the same in bgflow_amd/annealing.py, whose general path restates them in torch ops):
 *   ends          two energies A and B over the same rows x [B, n d], at the positive temperatures T_A and T_B
 *   schedule      lambdas = [l_0, ..., l_M], each in [0, 1], M >= 1; need not be monotone
 *   coefficients  stage m has cA_m = (1 - l_m) / T_A and cB_m = l_m / T_B, formed on the host in f64 and rounded to f32 once: the
 *                 device table `schedule` of f32 pairs (cA_m, cB_m), m = 0 .. M
 *   reduced energy  u_m(x) = cA_m e_A(x) + cB_m e_B(x) in f32 (two products, one sum); e_A, e_B: the raw f32 energies the lane carries,
 *                 bit for bit what bgk_pair_energy / bgk_box_energy return for the row at temperature 1.  A coefficient that is exactly 0
 *                 drops its term: 0 inf would be a NaN and freeze the chain
 *   protocol      global steps s = 0 .. M K - 1, K steps per stage, stage m = s / K + 1.  At the first step of a stage, first
 *                   W += (cA_m - cA_{m-1}) e_A + (cB_m - cB_{m-1}) e_B
 *                 of the CURRENT state, in f64 from the f32 operands (a difference that is exactly 0 drops its term, as above); then the
 *                 Metropolis step at u_m:  x' = x + noise_std xi_s,  accept iff -(u_m(x') - u_m(x)) >= log r_s  (false for a NaN on either
 *                 side, as in bgk_mcmc.hip).  Steps are taken at every stage, the last included
 *   results       the final state, work [B] (f64), e_A and e_B of the final state, n_accepted per chain
 *
 * By the rules of bgk_pair_tile.h, and in the pattern of pair_mcmc_kernel (bgk_mcmc.hip, unchanged): one wave per workgroup, ONE LANE PER
 * CHAIN, two LDS tiles A and B at the odd row stride, the second one a multiple of 32 words behind the first; a lane's current row is in
 * one, its proposal goes into the other, accepting is a per-lane flip.  Rows move through tile_stage and a per-row tile flag.  The tile
 * height is bgk_mcmc.hip's: 64 rows up to the 63,488-byte budget, 41 rows at n d = 192.  The argument record holds two BgkPairTargets; a
 * lane keeps cur, e_a, e_b, the f64 W and acc; every proposal evaluates bgk_row_energy<D, KIND_A> and bgk_row_energy<D, KIND_B> on the
 * proposal row.
 *
 * Random numbers: explicit -- noise [M K, B, n d] and uniforms [M K, B], row s -- or Philox4x32-10 in bgk_mcmc.hip's counter layout:
 * (global chain row0 + b, field 0 << 20 | 4-column block for the normals / 1 << 20 for the uniform, offset + s).  A pure function of
 * (seed, s, row0 + b, column).
 *
 * A launch runs the global steps [step_begin, step_end).  work, e_a, e_b and n_accepted are carried in memory between launches
 * (e_valid: read e_a / e_b instead of computing them; accumulate: continue work and n_accepted): the same bits however a protocol is
 * split, inside a stage included -- the increment belongs to the stage's first step, whichever launch runs it.
 *
 * Dispatch: ALL ordered pairs (KIND_A, KIND_B) are instantiated -- 3 x 3 pair kinds x 3 dimensions, 2 x 2 box kinds -- so the host
 * never swaps the ends or mirrors the table.  Plain C++ and vector stores only. */
#include "bgk_common.h"
#include "bgk_pair_terms.h"
#include "bgk_philox.h"

namespace {

constexpr int AN_LDS_DYNAMIC = 63488;

struct AnArgs {
    float* x; int64_t B, row0;
    BgkPairTarget ta, tb; int rows, tile_b;             /* tile_b: word offset of the second tile, a multiple of 32 */
    const float* schedule; int stage_steps, step_begin, step_end;
    float noise_std;
    const float* noise; const float* uniforms;
    uint32_t seed_lo, seed_hi, offset;
    float* e_a; float* e_b; int e_valid;
    double* work; int* n_accepted; int accumulate;
};

/* c_a e_a + c_b e_b; a coefficient that is exactly 0 drops its term */
__device__ __forceinline__ float an_reduced(float c_a, float c_b, float e_a, float e_b) {
    const float u_a = c_a != 0.0f ? c_a * e_a : 0.0f, u_b = c_b != 0.0f ? c_b * e_b : 0.0f;
    return u_a + u_b;
}

template <int D, int KIND_A, int KIND_B>
__global__ __launch_bounds__(BGK_TILE_THREADS) void pair_anneal_kernel(AnArgs a) {
    extern __shared__ float s_mem[];
    __shared__ int s_sel[BGK_TILE_THREADS];             /* which tile holds row r's current state */
    const int tid = threadIdx.x, nd = a.ta.nd, S = nd | 1;
    const int64_t n_tiles = (a.B + a.rows - 1) / a.rows;
    for (int64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const int64_t b0 = t * a.rows;
        const int rows = (int)((a.B - b0) < a.rows ? (a.B - b0) : a.rows);
        tile_stage(a.x, b0, rows, nd, a.ta.magic, s_mem);
        __syncthreads();
        const bool active = tid < rows;
        const int64_t b = b0 + (active ? tid : 0);
        const uint64_t grow = (uint64_t)(a.row0 + b);
        const uint32_t r_lo = (uint32_t)grow, r_hi = (uint32_t)(grow >> 32);
        int cur = 0, acc = 0;
        float e_a = 0.0f, e_b = 0.0f;
        double W = 0.0;
        if (active) {
            e_a = a.e_valid ? a.e_a[b] : (float)bgk_row_energy<D, KIND_A>(s_mem + tid * S, a.ta);
            e_b = a.e_valid ? a.e_b[b] : (float)bgk_row_energy<D, KIND_B>(s_mem + tid * S, a.tb);
            W = a.accumulate ? a.work[b] : 0.0;
        }
        int m = a.step_begin / a.stage_steps + 1, in_stage = a.step_begin - (m - 1) * a.stage_steps;
        for (int s = a.step_begin; s < a.step_end; ++s) {
            const float c_a = a.schedule[2 * m], c_b = a.schedule[2 * m + 1];       /* wave-uniform */
            if (active) {
                if (in_stage == 0) {                    /* the stage's first step: the work of switching the current state to it */
                    const double d_a = (double)c_a - (double)a.schedule[2 * m - 2], d_b = (double)c_b - (double)a.schedule[2 * m - 1];
                    const double w_a = d_a != 0.0 ? d_a * (double)e_a : 0.0, w_b = d_b != 0.0 ? d_b * (double)e_b : 0.0;
                    W += w_a + w_b;
                }
                const float* xc = s_mem + (cur ? a.tile_b : 0) + tid * S;
                float* xp = s_mem + (cur ? 0 : a.tile_b) + tid * S;
                float r;
                if (a.noise) {
                    const float* ns = a.noise + ((int64_t)s * a.B + b) * nd;
                    for (int c = 0; c < nd; ++c) xp[c] = xc[c] + a.noise_std * ns[c];
                    r = a.uniforms[(int64_t)s * a.B + b];
                } else {
                    const uint32_t off = a.offset + (uint32_t)s;
                    uint32_t o[4];
                    for (int cb = 0; 4 * cb < nd; ++cb) {
                        philox4x32_10(r_lo, r_hi, (uint32_t)cb, off, a.seed_lo, a.seed_hi, o);
                        float v[4];
                        philox_normal4(o, v);
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const int c = 4 * cb + q;
                            if (c < nd) xp[c] = xc[c] + a.noise_std * v[q];
                        }
                    }
                    philox4x32_10(r_lo, r_hi, 1u << 20, off, a.seed_lo, a.seed_hi, o);
                    r = u01(o[0]);
                }
                const float p_a = (float)bgk_row_energy<D, KIND_A>(xp, a.ta);       /* at temperature 1: the calls of pair_energy_kernel */
                const float p_b = (float)bgk_row_energy<D, KIND_B>(xp, a.tb);
                const float u = an_reduced(c_a, c_b, e_a, e_b), up = an_reduced(c_a, c_b, p_a, p_b);
                const bool accept = -(up - u) >= bgk_logf(r);                       /* false for a NaN on either side */
                cur = accept ? cur ^ 1 : cur;
                e_a = accept ? p_a : e_a;
                e_b = accept ? p_b : e_b;
                acc += accept ? 1 : 0;
            }
            if (++in_stage == a.stage_steps) { in_stage = 0; ++m; }
        }
        s_sel[tid] = cur;
        __syncthreads();
        for (int i = tid; i < rows * nd; i += BGK_TILE_THREADS) {       /* tile_store of every row's CURRENT state */
            const int r = (int)__umulhi((unsigned)i, a.ta.magic), c = i - r * nd;
            a.x[b0 * nd + i] = s_mem[(s_sel[r] ? a.tile_b : 0) + r * S + c];
        }
        if (active) {
            a.e_a[b] = e_a; a.e_b[b] = e_b; a.work[b] = W;
            if (a.n_accepted) a.n_accepted[b] = a.accumulate ? a.n_accepted[b] + acc : acc;
        }
        __syncthreads();
    }
}

/* one call of either entry: the two ends as the entry names them, then the entries' common arguments in order */
struct BgkAnnealCall {
    BgkPairSpec a, b;
    float* x; int64_t B;
    const float* schedule; int32_t n_stages, stage_steps, step_begin, step_end;
    double noise_std; const float* noise; const float* uniforms;
    uint64_t seed; uint32_t offset; int64_t row0;
    float* e_a; float* e_b; int32_t e_valid; double* work; int32_t* n_accepted; int32_t accumulate;
    void* stream;
};

template <int D, int KIND_A>
void anneal_launch_b(int kind_b, int grid, size_t lds, hipStream_t s, const AnArgs& a) {
    if constexpr (KIND_A >= 3) {
        if (kind_b == 3) tile_launch(pair_anneal_kernel<2, KIND_A, 3>, grid, lds, s, a);
        else tile_launch(pair_anneal_kernel<2, KIND_A, 4>, grid, lds, s, a);
    } else {
        if (kind_b == 0) tile_launch(pair_anneal_kernel<D, KIND_A, 0>, grid, lds, s, a);
        else if (kind_b == 1) tile_launch(pair_anneal_kernel<D, KIND_A, 1>, grid, lds, s, a);
        else tile_launch(pair_anneal_kernel<D, KIND_A, 2>, grid, lds, s, a);
    }
}

int anneal_run(const BgkAnnealCall& c) {
    const char* what = c.a.what;
    AnArgs a{};
    BGK_CHECK_ARG(c.B >= 0 && c.row0 >= 0, "%s: bad batch size / row0", what);
    int st = bgk_pair_target(c.a, &a.ta);
    if (st) return st;
    st = bgk_pair_target(c.b, &a.tb);
    if (st) return st;
    BGK_CHECK_ARG(c.a.n_particles == c.b.n_particles && c.a.n_dims == c.b.n_dims, "%s: both ends must have the same particles and dimensions", what);
    BGK_CHECK_ARG(c.n_stages >= 1 && c.stage_steps >= 1, "%s: n_stages %d / n_steps %d (at least 1)", what, c.n_stages, c.stage_steps);
    BGK_CHECK_ARG((int64_t)c.n_stages * c.stage_steps <= 0x7fffffff, "%s: n_stages * n_steps overflows", what);
    BGK_CHECK_ARG(c.step_begin >= 0 && c.step_begin <= c.step_end && c.step_end <= c.n_stages * c.stage_steps,
                  "%s: steps [%d, %d) of %d", what, c.step_begin, c.step_end, c.n_stages * c.stage_steps);
    BGK_CHECK_ARG(c.noise_std >= 0.0, "%s: noise_std must not be negative", what);
    BGK_CHECK_ARG((c.noise != nullptr) == (c.uniforms != nullptr), "%s: noise and uniforms go together", what);
    if (c.B == 0 || c.step_begin == c.step_end) return 0;
    BGK_CHECK_ARG(c.x && c.e_a && c.e_b && c.work && c.schedule, "%s: null tensor", what);
    const int S = a.ta.nd | 1;
    int rows = rows_within(AN_LDS_DYNAMIC, 2 * S * (int)sizeof(float));
    while ((((rows * S + 31) & ~31) + rows * S) * (int)sizeof(float) > AN_LDS_DYNAMIC) --rows;     /* the second tile starts at round32 */
    a.x = c.x; a.B = c.B; a.row0 = c.row0;
    a.rows = rows; a.tile_b = (rows * S + 31) & ~31;
    a.schedule = c.schedule; a.stage_steps = c.stage_steps; a.step_begin = c.step_begin; a.step_end = c.step_end;
    a.noise_std = (float)c.noise_std; a.noise = c.noise; a.uniforms = c.uniforms;
    a.seed_lo = (uint32_t)c.seed; a.seed_hi = (uint32_t)(c.seed >> 32); a.offset = c.offset;
    a.e_a = c.e_a; a.e_b = c.e_b; a.e_valid = c.e_valid != 0;
    a.work = c.work; a.n_accepted = c.n_accepted; a.accumulate = c.accumulate != 0;
    const size_t lds = (size_t)(a.tile_b + rows * S) * sizeof(float);
    const int grid = tile_grid(c.B, rows);
    hipStream_t s = (hipStream_t)c.stream;
    const int kind_b = c.b.kind;
    tile_dispatch<true>(c.a.kind, c.a.n_dims, [&](auto D, auto K) { anneal_launch_b<D(), K()>(kind_b, grid, lds, s, a); });
    return bgk_launch_status(what);
}

}  // namespace

extern "C" int bgk_pair_anneal(float* x, int64_t B, int32_t n_particles, int32_t n_dims,
                               int32_t kind_a, double a0, double a1, double a2, double a3, double osc_scale_a,
                               int32_t kind_b, double b0, double b1, double b2, double b3, double osc_scale_b,
                               const float* schedule, int32_t n_stages, int32_t n_steps, int32_t step_begin, int32_t step_end,
                               double noise_std, const float* noise, const float* uniforms,
                               uint64_t seed, uint32_t offset, int64_t row0,
                               float* e_a, float* e_b, int32_t e_valid, double* work, int32_t* n_accepted, int32_t accumulate, void* stream) {
    return anneal_run({bgk_pair_spec("bgk_pair_anneal", n_particles, n_dims, kind_a, a0, a1, a2, a3, osc_scale_a),
                       bgk_pair_spec("bgk_pair_anneal", n_particles, n_dims, kind_b, b0, b1, b2, b3, osc_scale_b), x, B,
                       schedule, n_stages, n_steps, step_begin, step_end, noise_std, noise, uniforms, seed, offset, row0,
                       e_a, e_b, e_valid, work, n_accepted, accumulate, stream});
}

/* the particle box (kinds 3 / 4 of bgk_pair_terms.h) at both ends, each with its own parameter array; two dimensions */
extern "C" int bgk_box_anneal(float* x, int64_t B, int32_t n_particles,
                              int32_t kind_a, const float* params_a, int32_t n_params_a,
                              int32_t kind_b, const float* params_b, int32_t n_params_b,
                              const float* schedule, int32_t n_stages, int32_t n_steps, int32_t step_begin, int32_t step_end,
                              double noise_std, const float* noise, const float* uniforms,
                              uint64_t seed, uint32_t offset, int64_t row0,
                              float* e_a, float* e_b, int32_t e_valid, double* work, int32_t* n_accepted, int32_t accumulate, void* stream) {
    return anneal_run({bgk_box_spec("bgk_box_anneal", n_particles, kind_a, params_a, n_params_a),
                       bgk_box_spec("bgk_box_anneal", n_particles, kind_b, params_b, n_params_b), x, B,
                       schedule, n_stages, n_steps, step_begin, step_end, noise_std, noise, uniforms, seed, offset, row0,
                       e_a, e_b, e_valid, work, n_accepted, accumulate, stream});
}
