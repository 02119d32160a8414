/* bgk_chain.h -- what the chain kernels share: bgk_mcmc.hip (Metropolis, replica exchange), bgk_hmc.hip (Hamiltonian Monte Carlo) and
 * bgk_anneal.hip (annealed switching).  Each runs a whole sequence of accept / reject steps of many chains in one launch, by the rules of
 * bgk_pair_tile.h: one wave per workgroup, ONE LANE PER CHAIN, a tile of rows staged coalesced through LDS at the odd row stride S, the
 * steps in lockstep across the wave (the accept flag only selects), no atomics, workgroups walk several tiles.  Here are the common
 * argument record, the host's checks and layout, the lane's identity for a tile, the step's random numbers, the frame record and the
 * final store.  The energy, and what a step does with it, is the kernel's own: nothing here knows a target.
 *
 * The rules, stated here once:
 *   sides      a lane's state has two SIDES in LDS, of `first` and `second` tiles of rows x S floats (Metropolis and annealing 1 + 1: the
 *              row; HMC 3 + 2: position, gradient, and the momentum with the first side).  The current state is in one side, the step's
 *              candidate is built in the other, and accepting is the per-lane flip of `cur` -- no copy.
 *   banks      the second side starts at tile_b, the next multiple of 32 words, so lanes whose current rows sit in different sides still
 *              hit distinct banks.
 *   budget     dynamic LDS <= 63,488 B: rows per tile = the most (<= 64) with (round32(first rows S) + second rows S) 4 B within it
 *              (chain_layout; the kernels' headers have the tables of heights).  Lanes beyond the rows only stage and store.
 *   numbers    explicit (noise [n_steps, B, n d] and uniforms [n_steps, B], read by the chain's lane) or drawn in the kernel from
 *              Philox4x32-10 in the counter layout of bgk_philox.h: counter = (global chain row0 + b low, high, field << 20 | 4-column
 *              block, offset + step); field 0 = the n d normals (Box-Muller), field 1 / block 0 / word 0 = the accept uniform, field 2
 *              likewise = the exchange uniform (bgk_mcmc.hip).  The stream is a pure function of (seed, step, global chain, column): the
 *              same bits whatever the tiling, the grid, row0 sharding or the split of a run into launches, and the bits
 *              bgk_philox_fields writes for (seed, offset + step) with fields [normal n d, uniform 1].
 *   accept     `left side >= log r` in f32: false for a NaN on either side, so a candidate whose energy is NaN or +inf is rejected by the
 *              comparison itself, as in the reference.  Its min(0, .) is dropped: log r < 0, so v and min(0, v) decide alike.
 *   carried    between launches x, the energies (e_valid: read, not computed) and, with accumulate, n_accepted are carried in memory: the
 *              same bits however a run is split into launches.
 *   frames     a recorded frame, like the final state, leaves as one coalesced tile store of every row's CURRENT side through a per-row
 *              flag in LDS (s_sel), between two barriers: the next candidates overwrite rows the store reads. */
#ifndef BGK_CHAIN_H
#define BGK_CHAIN_H

#include "bgk_pair_tile.h"
#include "bgk_philox.h"

constexpr int BGK_CHAIN_LDS_DYNAMIC = 63488;

/* the common part of a chain kernel's argument record, by value inside McArgs / HmArgs / AnArgs */
struct ChainArgs {
    float* x; int64_t B, row0;
    int nd; uint32_t magic; int rows, tile_b;           /* magic: i / nd by multiply-high; tile_b: word offset of the second side */
    const float* noise; const float* uniforms;
    uint32_t seed_lo, seed_hi, offset;
    int* n_accepted; int accumulate;
    float* traj; float* traj_e; int traj_every;        /* the optional frame record */
};

/* the same as the C entries name it, in their order */
struct ChainCall {
    float* x; int64_t B;
    const float* noise; const float* uniforms; uint64_t seed; uint32_t offset; int64_t row0;
    float* traj; float* traj_e; int32_t traj_every; int32_t* n_accepted; int32_t accumulate;
};

/* ---- host ------------------------------------------------------------------------------------------------------------------------- */

/* the entries' first check, before the target's own */
inline int chain_check_batch(const char* what, const ChainCall& c, int32_t n_steps) {
    BGK_CHECK_ARG(c.B >= 0 && c.row0 >= 0 && n_steps >= 0, "%s: bad batch size / row0 / n_steps", what);
    return 0;
}

/* ... and the shared ones after it */
inline int chain_check(const char* what, const ChainCall& c, bool temperature_positive) {
    BGK_CHECK_ARG(temperature_positive, "%s: the temperature must be positive", what);
    BGK_CHECK_ARG((c.noise != nullptr) == (c.uniforms != nullptr), "%s: noise and uniforms go together", what);
    BGK_CHECK_ARG(!c.traj_e || c.traj, "%s: traj_e without traj", what);
    BGK_CHECK_ARG(!c.traj || c.traj_every >= 1, "%s: traj_every %d", what, c.traj_every);
    return 0;
}

struct ChainLayout { int rows, tile_b; size_t lds; int grid; };

/* tiles of B chains of nd floats with `first` + `second` tiles per side: the most rows within the budget, or `rows` of them (the
 * caller's smaller height) */
inline ChainLayout chain_layout(int64_t B, int nd, int first, int second, int rows = 0) {
    const int S = nd | 1;
    const auto round32 = [](int words) { return (words + 31) & ~31; };
    if (rows == 0) {
        rows = rows_within(BGK_CHAIN_LDS_DYNAMIC, (first + second) * S * (int)sizeof(float));
        while ((round32(first * rows * S) + second * rows * S) * (int)sizeof(float) > BGK_CHAIN_LDS_DYNAMIC) --rows;
    }
    const int tile_b = round32(first * rows * S);
    return {rows, tile_b, (size_t)(tile_b + second * rows * S) * sizeof(float), tile_grid(B, rows)};
}

inline ChainArgs chain_args(const ChainCall& c, int nd, uint32_t magic, const ChainLayout& l) {
    return {c.x, c.B, c.row0, nd, magic, l.rows, l.tile_b, c.noise, c.uniforms, (uint32_t)c.seed, (uint32_t)(c.seed >> 32), c.offset,
            c.n_accepted, c.accumulate != 0, c.traj, c.traj_e, c.traj_every};
}

/* ---- device ----------------------------------------------------------------------------------------------------------------------- */

/* a lane's identity for a tile (b: its chain, the tile's first for an inactive lane; r_lo, r_hi: the global chain row0 + b) and the
 * tile's frame counter */
struct ChainLane {
    int64_t b0, b; int rows; bool active;
    uint32_t r_lo, r_hi;
    int frame, since;
};

__device__ __forceinline__ int64_t chain_n_tiles(const ChainArgs& a) { return (a.B + a.rows - 1) / a.rows; }

/* stages tile t into the first tile of s_mem, with the barrier */
__device__ __forceinline__ ChainLane chain_tile_begin(const ChainArgs& a, int64_t t, float* s_mem) {
    ChainLane l;
    l.b0 = t * a.rows;
    l.rows = (int)((a.B - l.b0) < a.rows ? (a.B - l.b0) : a.rows);
    tile_stage(a.x, l.b0, l.rows, a.nd, a.magic, s_mem);
    __syncthreads();
    l.active = (int)threadIdx.x < l.rows;
    l.b = l.b0 + (l.active ? (int)threadIdx.x : 0);
    const uint64_t grow = (uint64_t)(a.row0 + l.b);
    l.r_lo = (uint32_t)grow; l.r_hi = (uint32_t)(grow >> 32);
    l.frame = 0; l.since = 0;
    return l;
}

/* the numbers of step `step` (the Philox offset's and the explicit row's index) for an active lane: per_column(c, normal) for the
 * columns c = 0 .. n d - 1 in ascending order, then the accept uniform.  The explicit row is read column by column, outside the 4-column
 * blocks of bgk_philox.h's draw, and r has one exit: either other form costs the exchange kernels a VGPR and with it an occupancy step */
template <class F>
__device__ __forceinline__ float chain_draws(const ChainArgs& a, const ChainLane& l, int step, F per_column) {
    float r;
    if (a.noise) {
        const float* ns = a.noise + ((int64_t)step * a.B + l.b) * a.nd;
        for (int c = 0; c < a.nd; ++c) per_column(c, ns[c]);
        r = a.uniforms[(int64_t)step * a.B + l.b];
    } else {
        const uint32_t off = a.offset + (uint32_t)step;
        for (int cb = 0; 4 * cb < a.nd; ++cb) {
            float v[4];
            philox_field_normal4(nullptr, a.nd, cb, l.r_lo, l.r_hi, 0u, off, a.seed_lo, a.seed_hi, v);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int c = 4 * cb + q;
                if (c < a.nd) per_column(c, v[q]);
            }
        }
        r = philox_field_uniform(nullptr, l.r_lo, l.r_hi, 1u, off, a.seed_lo, a.seed_hi);
    }
    return r;
}

/* tile_store of every row's CURRENT state: s_sel[r] says which side holds it (ROWSEL, the exchange: bit 0, and the bits above which LDS
 * row holds slot r's state); dst: the tile's first row in contiguous rows */
template <bool ROWSEL>
__device__ __forceinline__ void chain_store_current(const ChainArgs& a, float* dst, int rows, const int* s_sel, const float* s_mem) {
    const int nd = a.nd, S = nd | 1;
    for (int i = threadIdx.x; i < rows * nd; i += BGK_TILE_THREADS) {
        const int r = (int)__umulhi((unsigned)i, a.magic), c = i - r * nd;
        const int sel = s_sel[r];
        dst[i] = s_mem[((ROWSEL ? sel & 1 : sel) ? a.tile_b : 0) + (ROWSEL ? sel >> 1 : r) * S + c];
    }
}

/* after a step, every lane: the frame if one is due (uniform over the wave).  sel: cur, or cur | row << 1 with ROWSEL */
template <bool ROWSEL = false>
__device__ __forceinline__ void chain_record(const ChainArgs& a, ChainLane& l, int sel, float e, int* s_sel, const float* s_mem) {
    if (a.traj && ++l.since == a.traj_every) {
        l.since = 0;
        s_sel[threadIdx.x] = sel;
        __syncthreads();
        chain_store_current<ROWSEL>(a, a.traj + ((int64_t)l.frame * a.B + l.b0) * a.nd, l.rows, s_sel, s_mem);
        if (l.active && a.traj_e) a.traj_e[(int64_t)l.frame * a.B + l.b] = e;
        ++l.frame;
        __syncthreads();                                /* the next candidates overwrite rows this store reads */
    }
}

/* after the last step, every lane: the tile's final state into x and, for an active lane, the kernel's own results (store_own()) and the
 * accepted steps, in one block (stores of the kernel's own elsewhere cost the exchange kernels an occupancy step); then the barrier before
 * the next tile is staged */
template <bool ROWSEL = false, class F>
__device__ __forceinline__ void chain_tile_end(const ChainArgs& a, const ChainLane& l, int sel, int acc, int* s_sel, const float* s_mem,
                                               F store_own) {
    s_sel[threadIdx.x] = sel;
    __syncthreads();
    chain_store_current<ROWSEL>(a, a.x + l.b0 * a.nd, l.rows, s_sel, s_mem);
    if (l.active) {
        store_own();
        if (a.n_accepted) a.n_accepted[l.b] = a.accumulate ? a.n_accepted[l.b] + acc : acc;
    }
    __syncthreads();
}

#endif
