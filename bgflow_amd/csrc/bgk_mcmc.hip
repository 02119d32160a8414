/* bgk_mcmc.hip -- Metropolis chains on a particle-system target, a whole run of steps in one launch
 *   MCMCStep._step with a GaussianProposal (bgflow/distribution/sampling/mcmc.py:29-46, 86-122) and metropolis_accept (mcmc.py:192-222):
 *     x' = x + noise_std eps,  accept iff min(0, -(e(x') - e(x)) / T) >= log r,  eps ~ N(0, 1)^{n d}, r ~ U(0, 1)
 *   on the targets of bgk_pair.hip (kind 0 Lennard-Jones, 1 multi-double-well, 2 mean-free normal; through bgk_box_mcmc kind 3 / 4, the
 *   particle box).  In stock ops one step is about a dozen
 *   launches (randn_like, add, the energy's op chain, rand_like, log, min, compare, two where) over a state of n d <= 192 floats per chain;
 *   here the state of a chain never leaves LDS between recorded frames.
 *
 * A chain kernel by the rules of bgk_chain.h (sides, banks, budget, numbers, accept, carried, frames), with 1 + 1 tiles: a lane's current
 * row is in one, its proposal is written into the other.
 *
 * Energy: bgk_row_energy of bgk_pair_terms.h -- the call of pair_energy_kernel, so e is, bit for bit, what bgk_pair_energy returns for
 * the row at temperature 1.
 *
 * Tile heights (rows, dynamic LDS):
 *   n d = 192 (S = 193): 41 rows, 63,396 B       LJ13 (S = 39): 64 rows, 19,968 B       DW4 (S = 9): 64 rows, 4,608 B
 *   the particle box of 38 particles (S = 77): 64 rows, 39,424 B       of 64 particles (S = 129): 61 rows, 62,964 B
 *
 * Replica exchange (EXCHANGE = true; entries bgk_pair_remc / bgk_box_remc; ReplicaExchangeMetropolisGauss.run,
 * distribution/sampling/_mcmc/metropolis.py:172-188): the B chains are L ladders of K temperatures, ladder-major -- chain b is slot
 * b % K of ladder b / K -- and a tile holds whole ladders (rows = the plain kernel's rounded down to a multiple of K), so a ladder is K
 * neighbouring lanes.  After the Metropolis part of every exchange_every-th step the pairs of slots (k, k + 1), k = parity (mod 2), try
 *   c = -(e[k+1] - e[k]) (1 / T[k+1] - 1 / T[k]),  exchange iff -log r > c   (f32; false for a NaN on either side),
 * r the number of the pair's LOWER slot: row j of exchange_uniforms for the j-th exchange of the launch, or Philox field 2 at the step's
 * offset.  The parity flips after every attempt.  An exchange moves
 * no data: the lane keeps `row`, the LDS row that holds its state (both tiles), next to `cur`, and two lanes swap (row, cur, e, walker) by
 * wave shuffles; the rows of a tile stay a permutation of its rows, so the banks stay distinct.  Temperatures, n_accepted and n_exchanged
 * (counted at the lower slot) belong to the slot.  The exchange condition is uniform over the wave and every lane executes the shuffles.
 * A frame due at the same step is recorded BEFORE the exchange.  Tile heights: floor(rows / K) K, e.g. K = 5: 40 rows at n d = 192. */
#include "bgk_chain.h"
#include "bgk_pair_terms.h"

namespace {

struct McArgs {
    ChainArgs c;
    BgkPairTarget t;
    float* e; int e_valid;
    float temperature; const float* temperatures;
    float noise_std; int n_steps;
    /* replica exchange (EXCHANGE kernels only) */
    int n_replicas, ex_every, ex_phase, ex_parity;
    const float* ex_uniforms; int* n_exchanged; int* walkers;
};

/* v of this lane after the exchanges of a step: the upper neighbour's if this lane exchanges upwards, the lower one's if downwards */
template <class T>
__device__ __forceinline__ T mc_exchanged(T v, bool up, bool down) {
    const T above = __shfl_down(v, 1), below = __shfl_up(v, 1);
    return up ? above : (down ? below : v);
}

template <int D, int KIND, bool EXCHANGE>
__global__ __launch_bounds__(BGK_TILE_THREADS) void pair_mcmc_kernel(McArgs a) {
    extern __shared__ float s_mem[];
    __shared__ int s_sel[BGK_TILE_THREADS];             /* which tile holds row r's current state */
    const int tid = threadIdx.x, S = a.c.nd | 1;
    const int64_t n_tiles = chain_n_tiles(a.c);
    for (int64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        ChainLane l = chain_tile_begin(a.c, t, s_mem);
        const bool active = l.active;
        const int64_t b = l.b;
        int cur = 0, acc = 0;
        float e = 0.0f, temp = 1.0f;
        if (active) {
            temp = a.temperatures ? a.temperatures[b] : a.temperature;
            e = a.e_valid ? a.e[b] : (float)bgk_row_energy<D, KIND>(s_mem + tid * S, a.t);
        }
        /* EXCHANGE: row = the LDS row of this slot's state; slot = tid % K (tiles start at multiples of K); d_beta = 1 / T of the slot
         * above minus this slot's; ex_since / parity / n_ex: the schedule, the same for every tile */
        int row = tid, slot = 0, walker = 0, exch = 0, ex_since = 0, parity = 0, n_ex = 0;
        float d_beta = 0.0f;
        if constexpr (EXCHANGE) {
            slot = tid % a.n_replicas;
            walker = (active && a.walkers) ? a.walkers[b] : slot;
            const float beta = 1.0f / temp;
            d_beta = __shfl_down(beta, 1) - beta;
            ex_since = a.ex_phase; parity = a.ex_parity;
        }
        for (int step = 0; step < a.n_steps; ++step) {
            if (active) {
                const int lrow = EXCHANGE ? row : tid;
                const float* xc = s_mem + (cur ? a.c.tile_b : 0) + lrow * S;
                float* xp = s_mem + (cur ? 0 : a.c.tile_b) + lrow * S;
                const float r = chain_draws(a.c, l, step, [&](int c, float v) { xp[c] = xc[c] + a.noise_std * v; });
                const float ep = (float)bgk_row_energy<D, KIND>(xp, a.t);      /* at temperature 1: the call of pair_energy_kernel */
                const bool accept = -(ep - e) / temp >= bgk_logf(r);
                cur = accept ? cur ^ 1 : cur;
                e = accept ? ep : e;
                acc += accept ? 1 : 0;
            }
            chain_record<EXCHANGE>(a.c, l, EXCHANGE ? (cur | (row << 1)) : cur, e, s_sel, s_mem);
            if constexpr (EXCHANGE) {
                if (++ex_since == a.ex_every) {         /* uniform over the wave; every lane runs the shuffles */
                    ex_since = 0;
                    const bool lower = active && (slot & 1) == parity && slot + 1 < a.n_replicas;      /* its upper slot is active too */
                    const float e_up = __shfl_down(e, 1);
                    bool up = false;
                    if (lower) {
                        const float r = philox_field_uniform(a.c.noise ? a.ex_uniforms + ((int64_t)n_ex * a.c.B + b) : nullptr, l.r_lo, l.r_hi,
                                                             2u, a.c.offset + (uint32_t)step, a.c.seed_lo, a.c.seed_hi);
                        const float c = -(e_up - e) * d_beta;
                        up = -bgk_logf(r) > c;          /* false for a NaN on either side */
                    }
                    const bool down = __shfl_up((int)up, 1) != 0 && slot >= 1 && ((slot - 1) & 1) == parity;
                    e = mc_exchanged(e, up, down);
                    cur = mc_exchanged(cur, up, down);
                    row = mc_exchanged(row, up, down);
                    walker = mc_exchanged(walker, up, down);
                    /* from here a lane reads and writes the LDS rows its partner wrote: ordered because the workgroup is ONE wave,
                     * whose LDS accesses execute in issue order; the fence keeps the compiler from moving accesses across the exchange */
                    static_assert(BGK_TILE_THREADS == 64, "the exchange relies on one wave per workgroup: more waves need a barrier here");
                    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    exch += up ? 1 : 0;
                    parity ^= 1;
                    ++n_ex;
                }
            }
        }
        chain_tile_end<EXCHANGE>(a.c, l, EXCHANGE ? (cur | (row << 1)) : cur, acc, s_sel, s_mem, [&] {
            a.e[b] = e;
            if constexpr (EXCHANGE) {
                if (a.n_exchanged) a.n_exchanged[b] = a.c.accumulate ? a.n_exchanged[b] + exch : exch;
                if (a.walkers) a.walkers[b] = walker;
            }
        });
    }
}

/* one call of either entry: the target as the entry names it (bgk_pair_spec / bgk_box_spec), then the entries' arguments: the chain
 * kernels' common ones, the Metropolis step's and the stream */
struct BgkMcmcCall {
    BgkPairSpec spec;
    ChainCall chain;
    float* e; int32_t e_valid; double temperature; const float* temperatures;
    double noise_std; int32_t n_steps;
    void* stream;
    /* replica exchange (the *_remc entries; n_replicas = 0: the plain kernel) */
    int32_t n_replicas, exchange_every, exchange_phase, exchange_parity;
    const float* exchange_uniforms; int32_t* n_exchanged; int32_t* walkers;
};

int mcmc_run(const BgkMcmcCall& c) {
    const char* what = c.spec.what;
    McArgs a{};
    int st = chain_check_batch(what, c.chain, c.n_steps);
    if (!st) st = bgk_pair_target(c.spec, &a.t);
    if (!st) st = chain_check(what, c.chain, c.temperatures || c.temperature > 0.0);
    if (st) return st;
    BGK_CHECK_ARG(c.noise_std >= 0.0, "%s: noise_std must not be negative", what);
    const bool exchange = c.n_replicas != 0;
    if (exchange) {
        BGK_CHECK_ARG(c.n_replicas >= 2, "%s: n_replicas %d (at least 2)", what, c.n_replicas);
        BGK_CHECK_ARG(c.exchange_every >= 1 && c.exchange_phase >= 0 && c.exchange_phase < c.exchange_every,
                      "%s: exchange_every %d / exchange_phase %d (0 <= phase < every)", what, c.exchange_every, c.exchange_phase);
        BGK_CHECK_ARG(c.exchange_parity == 0 || c.exchange_parity == 1, "%s: exchange_parity %d", what, c.exchange_parity);
        BGK_CHECK_ARG(c.chain.B % c.n_replicas == 0 && c.chain.row0 % c.n_replicas == 0,
                      "%s: the batch size and row0 must be multiples of n_replicas", what);
        const int64_t n_exchanges = ((int64_t)c.exchange_phase + c.n_steps) / c.exchange_every;
        BGK_CHECK_ARG(n_exchanges == 0 || (c.chain.noise != nullptr) == (c.exchange_uniforms != nullptr),
                      "%s: noise, uniforms and exchange_uniforms go together", what);
    }
    ChainLayout lay = chain_layout(c.chain.B, a.t.nd, 1, 1);
    if (exchange) {                                         /* the envelope of K, whatever the batch (an empty one included) */
        if (c.n_replicas > lay.rows) {
            bgk_set_error("%s: %d replicas are more than the %d rows of a tile of this target", what, c.n_replicas, lay.rows);
            return BGK_EUNSUPPORTED;
        }
        lay = chain_layout(c.chain.B, a.t.nd, 1, 1, lay.rows / c.n_replicas * c.n_replicas);      /* a tile holds whole ladders */
    }
    if (c.chain.B == 0) return 0;
    BGK_CHECK_ARG(c.chain.x && c.e, "%s: null tensor", what);
    BGK_CHECK_ARG(!exchange || c.temperatures, "%s: replica exchange needs temperatures [B]", what);
    a.c = chain_args(c.chain, a.t.nd, a.t.magic, lay);
    a.e = c.e; a.e_valid = c.e_valid != 0; a.temperature = (float)c.temperature; a.temperatures = c.temperatures;
    a.noise_std = (float)c.noise_std; a.n_steps = c.n_steps;
    hipStream_t s = (hipStream_t)c.stream;
    if (exchange) {
        a.n_replicas = c.n_replicas; a.ex_every = c.exchange_every; a.ex_phase = c.exchange_phase; a.ex_parity = c.exchange_parity;
        a.ex_uniforms = c.exchange_uniforms; a.n_exchanged = c.n_exchanged; a.walkers = c.walkers;
        tile_dispatch<true>(c.spec.kind, c.spec.n_dims, [&](auto D, auto K) { tile_launch(pair_mcmc_kernel<D(), K(), true>, lay.grid, lay.lds, s, a); });
    } else {
        tile_dispatch<true>(c.spec.kind, c.spec.n_dims, [&](auto D, auto K) { tile_launch(pair_mcmc_kernel<D(), K(), false>, lay.grid, lay.lds, s, a); });
    }
    return bgk_launch_status(what);
}

}  // namespace

extern "C" int bgk_pair_mcmc(float* x, int64_t B, int32_t n_particles, int32_t n_dims, int32_t kind,
                             double p0, double p1, double p2, double p3, double osc_scale,
                             float* e, int32_t e_valid, double temperature, const float* temperatures,
                             double noise_std, int32_t n_steps, const float* noise, const float* uniforms,
                             uint64_t seed, uint32_t offset, int64_t row0,
                             float* traj, float* traj_e, int32_t traj_every, int32_t* n_accepted, int32_t accumulate, void* stream) {
    return mcmc_run({bgk_pair_spec("bgk_pair_mcmc", n_particles, n_dims, kind, p0, p1, p2, p3, osc_scale),
                     {x, B, noise, uniforms, seed, offset, row0, traj, traj_e, traj_every, n_accepted, accumulate},
                     e, e_valid, temperature, temperatures, noise_std, n_steps, stream});
}

/* the particle box (kinds 3 / 4 of bgk_pair_terms.h) in the same chain kernel: MCMCStep._step (mcmc.py:86-122) over
 * RepulsiveParticles._energy / HarmonicParticles._energy (distribution/energy/particles.py:272-277, 376-381); two dimensions */
extern "C" int bgk_box_mcmc(float* x, int64_t B, int32_t n_particles, int32_t kind, const float* params, int32_t n_params,
                            float* e, int32_t e_valid, double temperature, const float* temperatures,
                            double noise_std, int32_t n_steps, const float* noise, const float* uniforms,
                            uint64_t seed, uint32_t offset, int64_t row0,
                            float* traj, float* traj_e, int32_t traj_every, int32_t* n_accepted, int32_t accumulate, void* stream) {
    return mcmc_run({bgk_box_spec("bgk_box_mcmc", n_particles, kind, params, n_params),
                     {x, B, noise, uniforms, seed, offset, row0, traj, traj_e, traj_every, n_accepted, accumulate},
                     e, e_valid, temperature, temperatures, noise_std, n_steps, stream});
}

/* replica exchange inside the chain kernel (the head comment's last part): the arguments of the *_mcmc entry, then the exchange's */
extern "C" int bgk_pair_remc(float* x, int64_t B, int32_t n_particles, int32_t n_dims, int32_t kind,
                             double p0, double p1, double p2, double p3, double osc_scale,
                             float* e, int32_t e_valid, double temperature, const float* temperatures,
                             double noise_std, int32_t n_steps, const float* noise, const float* uniforms,
                             uint64_t seed, uint32_t offset, int64_t row0,
                             float* traj, float* traj_e, int32_t traj_every, int32_t* n_accepted, int32_t accumulate, void* stream,
                             int32_t n_replicas, int32_t exchange_every, int32_t exchange_phase, int32_t exchange_parity,
                             const float* exchange_uniforms, int32_t* n_exchanged, int32_t* walkers) {
    if (n_replicas == 0) n_replicas = -1;               /* 0 means "the plain kernel" inside mcmc_run: refused here like any K < 2 */
    return mcmc_run({bgk_pair_spec("bgk_pair_remc", n_particles, n_dims, kind, p0, p1, p2, p3, osc_scale),
                     {x, B, noise, uniforms, seed, offset, row0, traj, traj_e, traj_every, n_accepted, accumulate},
                     e, e_valid, temperature, temperatures, noise_std, n_steps, stream,
                     n_replicas, exchange_every, exchange_phase, exchange_parity, exchange_uniforms, n_exchanged, walkers});
}

extern "C" int bgk_box_remc(float* x, int64_t B, int32_t n_particles, int32_t kind, const float* params, int32_t n_params,
                            float* e, int32_t e_valid, double temperature, const float* temperatures,
                            double noise_std, int32_t n_steps, const float* noise, const float* uniforms,
                            uint64_t seed, uint32_t offset, int64_t row0,
                            float* traj, float* traj_e, int32_t traj_every, int32_t* n_accepted, int32_t accumulate, void* stream,
                            int32_t n_replicas, int32_t exchange_every, int32_t exchange_phase, int32_t exchange_parity,
                            const float* exchange_uniforms, int32_t* n_exchanged, int32_t* walkers) {
    if (n_replicas == 0) n_replicas = -1;
    return mcmc_run({bgk_box_spec("bgk_box_remc", n_particles, kind, params, n_params),
                     {x, B, noise, uniforms, seed, offset, row0, traj, traj_e, traj_every, n_accepted, accumulate},
                     e, e_valid, temperature, temperatures, noise_std, n_steps, stream,
                     n_replicas, exchange_every, exchange_phase, exchange_parity, exchange_uniforms, n_exchanged, walkers});
}
