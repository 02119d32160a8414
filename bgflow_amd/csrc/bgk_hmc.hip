/* bgk_hmc.hip -- Hamiltonian Monte Carlo chains on a particle-system target, a whole run of steps in one launch
 *   MCMCStep._step (bgflow/distribution/sampling/mcmc.py:86-122) and metropolis_accept (mcmc.py:192-222) with a Hamiltonian proposal; the
 *   reference has HMC only as an OpenMM integrator (HamiltonianMCPathProbabilityIntegrator, nn/flow/stochastic/snf_openmm.py).  Per step,
 *   with h = step_size, m = mass, L = n_leapfrog, f(x) = -(d e / d x) / T, xi ~ N(0, 1)^{n d}, r ~ U(0, 1):
 *     p0 = sqrt(m) xi,  p = p0 + (h / 2) f(x),  then L times:  x' = x' + (h / m) p,  p = p + c f(x')  (c = h; h / 2 after the last drift)
 *     accept iff -(e(x') - e(x)) / T - (K(p) - K(p0)) >= log r,  K(p) = |p|^2 / (2 m)
 *   on the targets of bgk_pair.hip (kind 0 Lennard-Jones, 1 multi-double-well, 2 mean-free normal; through bgk_box_hmc kind 3 / 4, the
 *   particle box).  L = 1 is the Metropolis-adjusted Langevin algorithm.  In stock ops a step is L autograd force calls (an energy and
 *   a backward launch each), about 4 L elementwise launches, two energy calls and the accept chain, over a state of n d <= 192 floats per
 *   chain; here state, momentum and both gradients never leave LDS between recorded frames.
 *
 * By the rules of bgk_pair_tile.h, like bgk_mcmc.hip: one wave per workgroup, ONE LANE PER CHAIN, a tile of rows staged coalesced through
 * LDS at the odd row stride S, the steps in lockstep across the wave (the accept flag only selects), no atomics, a fixed summation order,
 * workgroups walk several tiles.  Five LDS tiles of rows x S floats: positions A and B, gradients GA and GB, the momentum P.  A lane's
 * current state and d e / d x at it sit in one (position, gradient) pair; the trajectory is integrated in the other pair, starting from a
 * copy of the current row, and accepting is the per-lane flip of which pair is which -- no copy, and the gradient at the current state
 * is carried: a step costs exactly L gradient evaluations and one energy evaluation, plus one gradient at the start of a launch.
 * Layout: A, GA, P, then (B, GB) from the next multiple of 32 words, so lanes whose current rows sit in different pairs still hit
 * distinct banks.  A recorded frame leaves as one coalesced tile store through a per-row pair flag in LDS.
 *
 * Arithmetic (the library is built with -ffp-contract=off): energy and gradient are bgk_row_energy / bgk_row_gradient of
 * bgk_pair_terms.h -- the calls of pair_energy_kernel and its backward -- so e is, bit for bit, what bgk_pair_energy / bgk_box_energy
 * return for the row at temperature 1.  The energies of kinds 0..2 do not change when all particles move together, so the exact gradient
 * sums to zero over the particles; the f32 one does not: where a chain's centroid has drifted (the momenta are not mean-free), osc (x_i -
 * xbar) carries the rounding of xbar as an error common to all particles, which would push the centroid on at every kick.  The kernel
 * takes the mean over the particles out of the gradient per dimension (f32, particles in ascending order) before it is used or
 * carried, as the reference's autograd gradient of 0.5 sum |x - xbar|^2 does -- where there is an oscillator term (osc != 0): the pair
 * terms alone add v to one particle and -v to the other, nothing common.  The box kinds 3 / 4 have walls and keep their gradient.
 * h / 2, h, h / m and sqrt(m) are formed in f64 on the host and rounded to f32 once; 1 / T per lane in f32; the kinetic energies are f64
 * sums of f32 squares times 1 / (2 m), rounded once.  The decision is made in f32 in the order of pair_mcmc_kernel plus the kinetic
 * term; min(0, .) is dropped as there.  A proposal whose energy, kinetic energy or any coordinate is NaN or +-inf is rejected by the
 * comparison itself (0 * x' of every coordinate and 0 * e(x') are added to the left side: 0, or NaN): a trajectory that blows up
 * leaves the chain where it was, and finite.
 *
 * Random numbers: explicit (noise [n_steps, B, n d] = xi and uniforms [n_steps, B], read by the chain's lane) or Philox4x32-10 in the
 * chain kernel's counter layout (bgk_philox.h): counter = (global chain low, high, field << 20 | 4-column block, offset + step), field
 * 0 = the n d normals, field 1 / block 0 / word 0 = the uniform, the chain index row0 + b.  The stream is a pure function of (seed,
 * step, global chain, column) -- the same bits whatever the tiling, the grid, row0 sharding or the split of a run into launches -- and
 * the bits bgk_philox_fields writes for (seed, offset + step) with fields [normal n d, uniform 1].
 *
 * Envelope: bgk_pair_tile.h.  Dynamic LDS <= 63,488 B: rows per tile = the most (<= 64) with (round32(3 rows S) + 2 rows S) 4 B within
 * it; lanes beyond the rows only stage and store:
 *   n d = 192 (S = 193): 16 rows, 61,824 B       LJ13 (S = 39): 64 rows, 49,920 B       DW4 (S = 9): 64 rows, 11,520 B
 *   the particle box of 38 particles (S = 77): 41 rows, 63,144 B       of 64 particles (S = 129): 24 rows, 62,016 B */
#include "bgk_common.h"
#include "bgk_pair_terms.h"
#include "bgk_philox.h"

namespace {

constexpr int HM_LDS_DYNAMIC = 63488;

struct HmArgs {
    float* x; int64_t B, row0;
    BgkPairTarget t; int rows, tile_b;                  /* tile_b: word offset of the second (position, gradient) pair, a multiple of 32 */
    float* e; int e_valid;
    float temperature; const float* temperatures;
    float h, hh, hm, sqrt_m; double inv_2m;             /* h, h / 2, h / m, sqrt(m): rounded once; 1 / (2 m) */
    int n_leapfrog, n_steps;
    const float* noise; const float* uniforms;
    uint32_t seed_lo, seed_hi, offset;
    float* traj; float* traj_e; int traj_every;
    int* n_accepted; int accumulate;
};

/* tile_store of every row's CURRENT state: s_sel[r] says which pair holds it; dst: the tile's first row in contiguous rows */
__device__ __forceinline__ void hm_store_current(const HmArgs& a, float* dst, int rows, const int* s_sel, const float* s_mem) {
    const int nd = a.t.nd, S = nd | 1;
    for (int i = threadIdx.x; i < rows * nd; i += BGK_TILE_THREADS) {
        const int r = (int)__umulhi((unsigned)i, a.t.magic), c = i - r * nd;
        dst[i] = s_mem[(s_sel[r] ? a.tile_b : 0) + r * S + c];
    }
}

/* d e / d x of the row for the kicks: bgk_row_gradient, and for the kinds 0..2 with an oscillator term its mean over the particles taken
 * out per dimension (header, "Arithmetic"); gw is the lane's own row of a gradient tile */
template <int D, int KIND>
__device__ __forceinline__ void hm_gradient(const float* xr, float* gw, const BgkPairTarget& tg) {
    bgk_row_gradient<D, KIND>(xr, gw, tg);
    if (KIND <= 2 && tg.osc != 0.0f) {                  /* uniform over the wave */
        const float inv_n = 1.0f / (float)tg.n;
#pragma unroll
        for (int k = 0; k < D; ++k) {
            float s = 0.0f;
            for (int i = 0; i < tg.n; ++i) s += gw[i * D + k];
            const float mean = s * inv_n;
            for (int i = 0; i < tg.n; ++i) gw[i * D + k] -= mean;
        }
    }
}

template <int D, int KIND>
__global__ __launch_bounds__(BGK_TILE_THREADS) void pair_hmc_kernel(HmArgs a) {
    extern __shared__ float s_mem[];
    __shared__ int s_sel[BGK_TILE_THREADS];             /* which pair holds row r's current state */
    const int tid = threadIdx.x, nd = a.t.nd, S = nd | 1;
    const int T = a.rows * S;                           /* words of one tile: a pair is (position at 0, gradient at T) */
    const int64_t n_tiles = (a.B + a.rows - 1) / a.rows;
    for (int64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const int64_t b0 = t * a.rows;
        const int rows = (int)((a.B - b0) < a.rows ? (a.B - b0) : a.rows);
        tile_stage(a.x, b0, rows, nd, a.t.magic, s_mem);
        __syncthreads();
        const bool active = tid < rows;
        const int64_t b = b0 + (active ? tid : 0);
        const uint64_t grow = (uint64_t)(a.row0 + b);
        const uint32_t r_lo = (uint32_t)grow, r_hi = (uint32_t)(grow >> 32);
        float* pr = s_mem + 2 * T + tid * S;            /* the momentum row (active lanes only: tid < rows) */
        int cur = 0, acc = 0;
        float e = 0.0f, temp = 1.0f, inv_t = 1.0f;
        if (active) {
            temp = a.temperatures ? a.temperatures[b] : a.temperature;
            inv_t = 1.0f / temp;
            e = a.e_valid ? a.e[b] : (float)bgk_row_energy<D, KIND>(s_mem + tid * S, a.t);
            hm_gradient<D, KIND>(s_mem + tid * S, s_mem + T + tid * S, a.t);
        }
        int frame = 0, since = 0;
        for (int step = 0; step < a.n_steps; ++step) {
            if (active) {
                const float* xc = s_mem + (cur ? a.tile_b : 0) + tid * S;
                const float* gc = xc + T;
                float* xt = s_mem + (cur ? 0 : a.tile_b) + tid * S;
                float* gt = xt + T;
                float r;
                double k0 = 0.0;
                if (a.noise) {
                    const float* ns = a.noise + ((int64_t)step * a.B + b) * nd;
                    for (int c = 0; c < nd; ++c) {
                        const float p0 = a.sqrt_m * ns[c];
                        k0 += (double)(p0 * p0);
                        pr[c] = p0 + a.hh * ((-gc[c]) * inv_t);
                        xt[c] = xc[c];
                    }
                    r = a.uniforms[(int64_t)step * a.B + b];
                } else {
                    const uint32_t off = a.offset + (uint32_t)step;
                    uint32_t o[4];
                    for (int cb = 0; 4 * cb < nd; ++cb) {
                        philox4x32_10(r_lo, r_hi, (uint32_t)cb, off, a.seed_lo, a.seed_hi, o);
                        float v[4];
                        philox_normal4(o, v);
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const int c = 4 * cb + q;
                            if (c < nd) {
                                const float p0 = a.sqrt_m * v[q];
                                k0 += (double)(p0 * p0);
                                pr[c] = p0 + a.hh * ((-gc[c]) * inv_t);
                                xt[c] = xc[c];
                            }
                        }
                    }
                    philox4x32_10(r_lo, r_hi, 1u << 20, off, a.seed_lo, a.seed_hi, o);
                    r = u01(o[0]);
                }
                for (int l = 0; l < a.n_leapfrog; ++l) {                /* uniform over the wave */
                    for (int c = 0; c < nd; ++c) xt[c] = xt[c] + a.hm * pr[c];
                    hm_gradient<D, KIND>(xt, gt, a.t);
                    const float kick = l + 1 < a.n_leapfrog ? a.h : a.hh;
                    for (int c = 0; c < nd; ++c) pr[c] = pr[c] + kick * ((-gt[c]) * inv_t);
                }
                double k1 = 0.0;
                float xz = 0.0f;                                        /* 0, or NaN if a coordinate is not finite */
                for (int c = 0; c < nd; ++c) {
                    const float p = pr[c];
                    k1 += (double)(p * p);
                    xz += 0.0f * xt[c];
                }
                const float kin0 = (float)(k0 * a.inv_2m), kin1 = (float)(k1 * a.inv_2m);
                const float ep = (float)bgk_row_energy<D, KIND>(xt, a.t);      /* at temperature 1: the call of pair_energy_kernel */
                xz += 0.0f * ep;                                        /* ... or if the energy is +-inf */
                const bool accept = (-(ep - e) / temp - (kin1 - kin0)) + xz >= bgk_logf(r);     /* false for a NaN on either side */
                cur = accept ? cur ^ 1 : cur;
                e = accept ? ep : e;
                acc += accept ? 1 : 0;
            }
            if (a.traj && ++since == a.traj_every) {    /* uniform over the wave */
                since = 0;
                s_sel[tid] = cur;
                __syncthreads();
                hm_store_current(a, a.traj + ((int64_t)frame * a.B + b0) * nd, rows, s_sel, s_mem);
                if (active && a.traj_e) a.traj_e[(int64_t)frame * a.B + b] = e;
                ++frame;
                __syncthreads();                        /* the next trajectories overwrite rows this store reads */
            }
        }
        s_sel[tid] = cur;
        __syncthreads();
        hm_store_current(a, a.x + b0 * nd, rows, s_sel, s_mem);
        if (active) {
            a.e[b] = e;
            if (a.n_accepted) a.n_accepted[b] = a.accumulate ? a.n_accepted[b] + acc : acc;
        }
        __syncthreads();
    }
}

/* one call of either entry: the target as the entry names it (bgk_pair_spec / bgk_box_spec), then the entries' common arguments in order */
struct BgkHmcCall {
    BgkPairSpec spec;
    float* x; int64_t B;
    float* e; int32_t e_valid; double temperature; const float* temperatures;
    double step_size; int32_t n_leapfrog; double mass; int32_t n_steps; const float* noise; const float* uniforms;
    uint64_t seed; uint32_t offset; int64_t row0;
    float* traj; float* traj_e; int32_t traj_every; int32_t* n_accepted; int32_t accumulate;
    void* stream;
};

int hmc_run(const BgkHmcCall& c) {
    const char* what = c.spec.what;
    HmArgs a{};
    BGK_CHECK_ARG(c.B >= 0 && c.row0 >= 0 && c.n_steps >= 0, "%s: bad batch size / row0 / n_steps", what);
    const int st = bgk_pair_target(c.spec, &a.t);
    if (st) return st;
    BGK_CHECK_ARG(c.temperatures || c.temperature > 0.0, "%s: the temperature must be positive", what);
    BGK_CHECK_ARG(c.step_size > 0.0 && c.step_size < INFINITY, "%s: the step size must be positive and finite", what);
    BGK_CHECK_ARG(c.mass > 0.0 && c.mass < INFINITY, "%s: the mass must be positive and finite", what);
    BGK_CHECK_ARG(c.n_leapfrog >= 1, "%s: n_leapfrog %d (at least 1)", what, c.n_leapfrog);
    BGK_CHECK_ARG((c.noise != nullptr) == (c.uniforms != nullptr), "%s: noise and uniforms go together", what);
    BGK_CHECK_ARG(!c.traj_e || c.traj, "%s: traj_e without traj", what);
    BGK_CHECK_ARG(!c.traj || c.traj_every >= 1, "%s: traj_every %d", what, c.traj_every);
    if (c.B == 0) return 0;
    BGK_CHECK_ARG(c.x && c.e, "%s: null tensor", what);
    const int S = a.t.nd | 1;
    int rows = rows_within(HM_LDS_DYNAMIC, 5 * S * (int)sizeof(float));
    while ((((3 * rows * S + 31) & ~31) + 2 * rows * S) * (int)sizeof(float) > HM_LDS_DYNAMIC) --rows;     /* the second pair starts at round32 */
    a.x = c.x; a.B = c.B; a.row0 = c.row0;
    a.rows = rows; a.tile_b = (3 * rows * S + 31) & ~31;
    a.e = c.e; a.e_valid = c.e_valid != 0; a.temperature = (float)c.temperature; a.temperatures = c.temperatures;
    a.h = (float)c.step_size; a.hh = (float)(c.step_size / 2.0); a.hm = (float)(c.step_size / c.mass); a.sqrt_m = (float)sqrt(c.mass);
    a.inv_2m = 1.0 / (2.0 * c.mass);
    a.n_leapfrog = c.n_leapfrog; a.n_steps = c.n_steps; a.noise = c.noise; a.uniforms = c.uniforms;
    a.seed_lo = (uint32_t)c.seed; a.seed_hi = (uint32_t)(c.seed >> 32); a.offset = c.offset;
    a.traj = c.traj; a.traj_e = c.traj_e; a.traj_every = c.traj_every; a.n_accepted = c.n_accepted; a.accumulate = c.accumulate != 0;
    const size_t lds = (size_t)(a.tile_b + 2 * rows * S) * sizeof(float);
    const int grid = tile_grid(c.B, rows);
    hipStream_t s = (hipStream_t)c.stream;
    tile_dispatch<true>(c.spec.kind, c.spec.n_dims, [&](auto D, auto K) { tile_launch(pair_hmc_kernel<D(), K()>, grid, lds, s, a); });
    return bgk_launch_status(what);
}

}  // namespace

extern "C" int bgk_pair_hmc(float* x, int64_t B, int32_t n_particles, int32_t n_dims, int32_t kind,
                            double p0, double p1, double p2, double p3, double osc_scale,
                            float* e, int32_t e_valid, double temperature, const float* temperatures,
                            double step_size, int32_t n_leapfrog, double mass, int32_t n_steps, const float* noise, const float* uniforms,
                            uint64_t seed, uint32_t offset, int64_t row0,
                            float* traj, float* traj_e, int32_t traj_every, int32_t* n_accepted, int32_t accumulate, void* stream) {
    return hmc_run({bgk_pair_spec("bgk_pair_hmc", n_particles, n_dims, kind, p0, p1, p2, p3, osc_scale), x, B,
                    e, e_valid, temperature, temperatures, step_size, n_leapfrog, mass, n_steps, noise, uniforms, seed, offset, row0,
                    traj, traj_e, traj_every, n_accepted, accumulate, stream});
}

/* the particle box (kinds 3 / 4 of bgk_pair_terms.h) in the same kernel; two dimensions */
extern "C" int bgk_box_hmc(float* x, int64_t B, int32_t n_particles, int32_t kind, const float* params, int32_t n_params,
                           float* e, int32_t e_valid, double temperature, const float* temperatures,
                           double step_size, int32_t n_leapfrog, double mass, int32_t n_steps, const float* noise, const float* uniforms,
                           uint64_t seed, uint32_t offset, int64_t row0,
                           float* traj, float* traj_e, int32_t traj_every, int32_t* n_accepted, int32_t accumulate, void* stream) {
    return hmc_run({bgk_box_spec("bgk_box_hmc", n_particles, kind, params, n_params), x, B,
                    e, e_valid, temperature, temperatures, step_size, n_leapfrog, mass, n_steps, noise, uniforms, seed, offset, row0,
                    traj, traj_e, traj_every, n_accepted, accumulate, stream});
}
