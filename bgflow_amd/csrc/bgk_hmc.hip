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
 * A chain kernel by the rules of bgk_chain.h (sides, banks, budget, numbers, accept, carried, frames), with 3 + 2 tiles, a fixed summation
 * order: positions A and B, gradients GA and GB, the momentum P, laid out A, GA, P, then (B, GB).  A lane's current state and
 * d e / d x at it sit in one (position, gradient) pair; the trajectory is integrated in the other pair, starting from a
 * copy of the current row, and the gradient at the current state is carried with the flip: a step costs exactly L gradient evaluations
 * and one energy evaluation, plus one gradient at the start of a launch.  noise holds xi.
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
 * term.  A proposal whose kinetic energy or any coordinate is NaN or +-inf is rejected like one whose energy is
 * (0 * x' of every coordinate and 0 * e(x') are added to the left side: 0, or NaN): a trajectory that blows up
 * leaves the chain where it was, and finite.
 *
 * Tile heights (rows, dynamic LDS):
 *   n d = 192 (S = 193): 16 rows, 61,824 B       LJ13 (S = 39): 64 rows, 49,920 B       DW4 (S = 9): 64 rows, 11,520 B
 *   the particle box of 38 particles (S = 77): 41 rows, 63,144 B       of 64 particles (S = 129): 24 rows, 62,016 B */
#include "bgk_chain.h"
#include "bgk_pair_terms.h"

namespace {

struct HmArgs {
    BgkPairTarget t;                                    /* ahead of c: the other order reloads more spilled scalars in the leapfrog, */
    ChainArgs c;                                        /* measured 1 % (L = 1) to 2 % (L = 10) slower at n d = 192 */
    float* e; int e_valid;
    float temperature; const float* temperatures;
    float h, hh, hm, sqrt_m; double inv_2m;             /* h, h / 2, h / m, sqrt(m): rounded once; 1 / (2 m) */
    int n_leapfrog, n_steps;
};

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
    const int tid = threadIdx.x, nd = a.c.nd, S = nd | 1;
    const int T = a.c.rows * S;                         /* words of one tile: a pair is (position at 0, gradient at T) */
    const int64_t n_tiles = chain_n_tiles(a.c);
    for (int64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        ChainLane l = chain_tile_begin(a.c, t, s_mem);
        const bool active = l.active;
        const int64_t b = l.b;
        float* pr = s_mem + 2 * T + tid * S;            /* the momentum row (active lanes only: tid < rows) */
        int cur = 0, acc = 0;
        float e = 0.0f, temp = 1.0f, inv_t = 1.0f;
        if (active) {
            temp = a.temperatures ? a.temperatures[b] : a.temperature;
            inv_t = 1.0f / temp;
            e = a.e_valid ? a.e[b] : (float)bgk_row_energy<D, KIND>(s_mem + tid * S, a.t);
            hm_gradient<D, KIND>(s_mem + tid * S, s_mem + T + tid * S, a.t);
        }
        for (int step = 0; step < a.n_steps; ++step) {
            if (active) {
                const float* xc = s_mem + (cur ? a.c.tile_b : 0) + tid * S;
                const float* gc = xc + T;
                float* xt = s_mem + (cur ? 0 : a.c.tile_b) + tid * S;
                float* gt = xt + T;
                double k0 = 0.0;
                const float r = chain_draws(a.c, l, step, [&](int c, float xi) {
                    const float p0 = a.sqrt_m * xi;
                    k0 += (double)(p0 * p0);
                    pr[c] = p0 + a.hh * ((-gc[c]) * inv_t);
                    xt[c] = xc[c];
                });
                for (int lf = 0; lf < a.n_leapfrog; ++lf) {             /* uniform over the wave */
                    for (int c = 0; c < nd; ++c) xt[c] = xt[c] + a.hm * pr[c];
                    hm_gradient<D, KIND>(xt, gt, a.t);
                    const float kick = lf + 1 < a.n_leapfrog ? a.h : a.hh;
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
                const bool accept = (-(ep - e) / temp - (kin1 - kin0)) + xz >= bgk_logf(r);
                cur = accept ? cur ^ 1 : cur;
                e = accept ? ep : e;
                acc += accept ? 1 : 0;
            }
            chain_record(a.c, l, cur, e, s_sel, s_mem);
        }
        chain_tile_end(a.c, l, cur, acc, s_sel, s_mem, [&] { a.e[b] = e; });
    }
}

/* one call of either entry: the target as the entry names it (bgk_pair_spec / bgk_box_spec), then the entries' arguments: the chain
 * kernels' common ones, the Hamiltonian step's and the stream */
struct BgkHmcCall {
    BgkPairSpec spec;
    ChainCall chain;
    float* e; int32_t e_valid; double temperature; const float* temperatures;
    double step_size; int32_t n_leapfrog; double mass; int32_t n_steps;
    void* stream;
};

int hmc_run(const BgkHmcCall& c) {
    const char* what = c.spec.what;
    HmArgs a{};
    int st = chain_check_batch(what, c.chain, c.n_steps);
    if (!st) st = bgk_pair_target(c.spec, &a.t);
    if (!st) st = chain_check(what, c.chain, c.temperatures || c.temperature > 0.0);
    if (st) return st;
    BGK_CHECK_ARG(c.step_size > 0.0 && c.step_size < INFINITY, "%s: the step size must be positive and finite", what);
    BGK_CHECK_ARG(c.mass > 0.0 && c.mass < INFINITY, "%s: the mass must be positive and finite", what);
    BGK_CHECK_ARG(c.n_leapfrog >= 1, "%s: n_leapfrog %d (at least 1)", what, c.n_leapfrog);
    if (c.chain.B == 0) return 0;
    BGK_CHECK_ARG(c.chain.x && c.e, "%s: null tensor", what);
    const ChainLayout lay = chain_layout(c.chain.B, a.t.nd, 3, 2);
    a.c = chain_args(c.chain, a.t.nd, a.t.magic, lay);
    a.e = c.e; a.e_valid = c.e_valid != 0; a.temperature = (float)c.temperature; a.temperatures = c.temperatures;
    a.h = (float)c.step_size; a.hh = (float)(c.step_size / 2.0); a.hm = (float)(c.step_size / c.mass); a.sqrt_m = (float)sqrt(c.mass);
    a.inv_2m = 1.0 / (2.0 * c.mass);
    a.n_leapfrog = c.n_leapfrog; a.n_steps = c.n_steps;
    hipStream_t s = (hipStream_t)c.stream;
    tile_dispatch<true>(c.spec.kind, c.spec.n_dims, [&](auto D, auto K) { tile_launch(pair_hmc_kernel<D(), K()>, lay.grid, lay.lds, s, a); });
    return bgk_launch_status(what);
}

}  // namespace

extern "C" int bgk_pair_hmc(float* x, int64_t B, int32_t n_particles, int32_t n_dims, int32_t kind,
                            double p0, double p1, double p2, double p3, double osc_scale,
                            float* e, int32_t e_valid, double temperature, const float* temperatures,
                            double step_size, int32_t n_leapfrog, double mass, int32_t n_steps, const float* noise, const float* uniforms,
                            uint64_t seed, uint32_t offset, int64_t row0,
                            float* traj, float* traj_e, int32_t traj_every, int32_t* n_accepted, int32_t accumulate, void* stream) {
    return hmc_run({bgk_pair_spec("bgk_pair_hmc", n_particles, n_dims, kind, p0, p1, p2, p3, osc_scale),
                    {x, B, noise, uniforms, seed, offset, row0, traj, traj_e, traj_every, n_accepted, accumulate},
                    e, e_valid, temperature, temperatures, step_size, n_leapfrog, mass, n_steps, stream});
}

/* the particle box (kinds 3 / 4 of bgk_pair_terms.h) in the same kernel; two dimensions */
extern "C" int bgk_box_hmc(float* x, int64_t B, int32_t n_particles, int32_t kind, const float* params, int32_t n_params,
                           float* e, int32_t e_valid, double temperature, const float* temperatures,
                           double step_size, int32_t n_leapfrog, double mass, int32_t n_steps, const float* noise, const float* uniforms,
                           uint64_t seed, uint32_t offset, int64_t row0,
                           float* traj, float* traj_e, int32_t traj_every, int32_t* n_accepted, int32_t accumulate, void* stream) {
    return hmc_run({bgk_box_spec("bgk_box_hmc", n_particles, kind, params, n_params),
                    {x, B, noise, uniforms, seed, offset, row0, traj, traj_e, traj_every, n_accepted, accumulate},
                    e, e_valid, temperature, temperatures, step_size, n_leapfrog, mass, n_steps, stream});
}
