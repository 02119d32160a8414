/* bgk_pair_tile.h -- what the particle-system kernels share: bgk_pair.hip (energy / backward / hvp), the chain kernels of bgk_chain.h (bgk_mcmc.hip, bgk_hmc.hip, bgk_anneal.hip),
 * bgk_langevin.hip (Brownian / Langevin forward, record, adjoint) and bgk_kdyn.hip (kernel dynamics).  The formulas of the targets are in
 * bgk_pair_terms.h; here are the target's parameter record, the walk over tiles of rows and the choice of a kernel instantiation.
 *
 * The rules, stated here once:
 *   envelope   x [B, n d]: 2 <= n <= 64 particles in 1 <= d <= 3 dimensions, i.e. n d <= 192.
 *   lanes      one wave of 64 per workgroup, ONE LANE PER SAMPLE (row): rows of a tile <= 64, pairs in the fixed ascending (i, j) order, no
 *              atomics -- deterministic.  Lanes beyond a tile's rows only stage and store.  A workgroup walks the tiles
 *              blockIdx.x, blockIdx.x + gridDim.x, ...; the grid is the number of tiles, at most 256 CUs x 16.
 *   stride     a tile's rows lie in LDS at the odd stride S = (n d) | 1 <= 193: lane r reads word r S + k, distinct banks.
 *   staging    all 64 lanes move a tile between memory and LDS coalesced: element i of the tile is row r = i / (n d), column
 *              c = i - r n d, and the division is a multiply-high by magic = ceil(2^32 / (n d)), exact for i < 64 * 192.
 *   rows       where a kernel keeps several tiles per row, a tile has the most rows (<= 64) whose bytes fit the kernel's LDS budget
 *              (rows_within; the budgets and the tables of the resulting heights are in the kernels' own headers). */
#ifndef BGK_PAIR_TILE_H
#define BGK_PAIR_TILE_H

#include <type_traits>

#include "bgk_common.h"

constexpr int BGK_TILE_THREADS = 64;                    /* one wave: rows of a tile <= lanes */
constexpr int BGK_TILE_MAX_N = 64, BGK_TILE_MAX_D = 3;
constexpr int BGK_TILE_MAX_GRID = 256 * 16;

/* ---- the target --------------------------------------------------------------------------------------------------------------------- */

/* the parameters of KIND 3 / 4 (the particle box; formulas: bgk_pair_terms.h) */
struct BgkBoxParams {
    float eps, rm2, spring, rc, rc2;
    float dimer_k, dimer_slope, dimer_a, dimer_b, dimer_dmid;
    float box_half, box_k;
};

/* the host array of the bgk_box_* entries (include/bgflow_amd.h): [eps, rm^2, rc, rc^2, spring_constant, dimer_slope, dimer_a, dimer_b,
 * dimer_dmid, dimer_k, box_halfsize, box_k]; the caller forms the squares in double, so that they are rounded once */
constexpr int BGK_BOX_N_PARAMS = 12;
inline void bgk_box_params_from_host(const float* h, BgkBoxParams* p) {
    p->eps = h[0]; p->rm2 = h[1]; p->rc = h[2]; p->rc2 = h[3]; p->spring = h[4];
    p->dimer_slope = h[5]; p->dimer_a = h[6]; p->dimer_b = h[7]; p->dimer_dmid = h[8]; p->dimer_k = h[9];
    p->box_half = h[10]; p->box_k = h[11];
}

/* a particle-system target, by value inside the kernels' argument records (wave-uniform): kind 0..2 read p0..p3 and osc, kind 3 / 4 box
 * (bgk_pair_terms.h says which parameter is which) */
struct BgkPairTarget {
    int n, nd; uint32_t magic;                          /* nd = n d; magic: i / nd by multiply-high (tile_stage) */
    float p0, p1, p2, p3, osc;
    BgkBoxParams box;
};

/* the target as a C entry names it: the bgk_pair_* entries give (n_dims, kind 0..2, p0..p3, osc_scale), the bgk_box_* entries
 * (kind 3 / 4, a host parameter array), two dimensions */
struct BgkPairSpec {
    const char* what;                                   /* the entry's name, for its messages */
    int32_t n_particles, n_dims, kind;
    double p0, p1, p2, p3, osc_scale;
    const float* box_params; int32_t n_box_params; int32_t is_box;
};

inline BgkPairSpec bgk_pair_spec(const char* what, int32_t n_particles, int32_t n_dims, int32_t kind, double p0, double p1, double p2,
                                 double p3, double osc_scale) {
    return BgkPairSpec{what, n_particles, n_dims, kind, p0, p1, p2, p3, osc_scale, nullptr, 0, 0};
}

inline BgkPairSpec bgk_box_spec(const char* what, int32_t n_particles, int32_t kind, const float* params, int32_t n_params) {
    return BgkPairSpec{what, n_particles, 2, kind, 0.0, 0.0, 0.0, 0.0, 0.0, params, n_params, 1};
}

inline uint32_t tile_magic(int nd) { return (uint32_t)(((1ull << 32) + (uint64_t)nd - 1) / (uint64_t)nd); }

/* checks the kind, then the envelope, and fills *t (the doubles rounded to f32 once); 0, BGK_EINVAL or BGK_EUNSUPPORTED */
inline int bgk_pair_target(const BgkPairSpec& c, BgkPairTarget* t) {
    if (c.is_box) {
        BGK_CHECK_ARG(c.kind == 3 || c.kind == 4, "%s: kind %d (3 repulsive particles, 4 harmonic particles)", c.what, c.kind);
        BGK_CHECK_ARG(c.box_params && c.n_box_params == BGK_BOX_N_PARAMS, "%s: params must be %d floats (see bgflow_amd.h)", c.what,
                      BGK_BOX_N_PARAMS);
    } else {
        BGK_CHECK_ARG(c.kind >= 0 && c.kind <= 2, "%s: kind %d (0 Lennard-Jones, 1 multi-double-well, 2 mean-free normal)", c.what, c.kind);
    }
    if (!(c.n_particles >= 2 && c.n_particles <= BGK_TILE_MAX_N && c.n_dims >= 1 && c.n_dims <= BGK_TILE_MAX_D)) {
        bgk_set_error("%s: %d particles in %d dimensions are outside the kernel's envelope (2..%d particles, 1..%d dimensions)", c.what,
                      c.n_particles, c.n_dims, BGK_TILE_MAX_N, BGK_TILE_MAX_D);
        return BGK_EUNSUPPORTED;
    }
    t->n = c.n_particles; t->nd = c.n_particles * c.n_dims; t->magic = tile_magic(t->nd);
    t->p0 = (float)c.p0; t->p1 = (float)c.p1; t->p2 = (float)c.p2; t->p3 = (float)c.p3; t->osc = (float)c.osc_scale;
    if (c.is_box) bgk_box_params_from_host(c.box_params, &t->box);
    return 0;
}

/* ---- the tile walk ------------------------------------------------------------------------------------------------------------------ */

/* the most rows (<= 64) of bytes_per_row that fit budget_bytes of LDS */
inline int rows_within(int budget_bytes, int bytes_per_row) {
    const int rows = budget_bytes / bytes_per_row;
    return rows < BGK_TILE_THREADS ? rows : BGK_TILE_THREADS;
}

/* workgroups for B rows in tiles of `rows` */
inline int tile_grid(int64_t B, int rows, int cap = BGK_TILE_MAX_GRID) {
    const int64_t n_tiles = (B + rows - 1) / rows;
    return (int)(n_tiles < cap ? n_tiles : cap);
}

/* rows [b0, b0 + rows) of the contiguous src [B, nd] into the tile (row stride (nd | 1)), every lane of the wave; no barrier.  The rows
 * are one run of src: element i of the tile is word b0 nd + i */
__device__ __forceinline__ void tile_stage(const float* src, int64_t b0, int rows, int nd, uint32_t magic, float* tile) {
    const int S = nd | 1;
    for (int i = threadIdx.x; i < rows * nd; i += BGK_TILE_THREADS) {
        const int r = (int)__umulhi((unsigned)i, magic), c = i - r * nd;
        tile[r * S + c] = src[b0 * nd + i];
    }
}

/* the same from rows of stride ld >= nd (bgk_pair.hip's x) */
__device__ __forceinline__ void tile_stage_ld(const float* src, int64_t ld, int64_t b0, int rows, int nd, uint32_t magic, float* tile) {
    const int S = nd | 1;
    for (int i = threadIdx.x; i < rows * nd; i += BGK_TILE_THREADS) {
        const int r = (int)__umulhi((unsigned)i, magic), c = i - r * nd;
        tile[r * S + c] = src[(b0 + r) * ld + c];
    }
}

/* the tile into rows [b0, b0 + rows) of the contiguous dst [B, nd], every lane of the wave; no barrier */
__device__ __forceinline__ void tile_store(float* dst, int64_t b0, int rows, int nd, uint32_t magic, const float* tile) {
    const int S = nd | 1;
    for (int i = threadIdx.x; i < rows * nd; i += BGK_TILE_THREADS) {
        const int r = (int)__umulhi((unsigned)i, magic), c = i - r * nd;
        dst[b0 * nd + i] = tile[r * S + c];
    }
}

/* ---- the choice of an instantiation --------------------------------------------------------------------------------------------------- */

template <int V> using bgk_int = std::integral_constant<int, V>;

/* f(bgk_int<D>) for d = 1..3 (checked by the caller) */
template <class F>
void tile_dispatch_d(int d, F f) {
    if (d == 1) f(bgk_int<1>{});
    else if (d == 2) f(bgk_int<2>{});
    else f(bgk_int<3>{});
}

/* f(bgk_int<D>, bgk_int<KIND>) for (d = 1..3) x (kind = 0..2) and, for the kernels that have a box form (BOX), (2, 3) and (2, 4); kind
 * and d as bgk_pair_target has checked them */
template <bool BOX, class F>
void tile_dispatch(int kind, int d, F f) {
    if constexpr (BOX) {
        if (kind == 3) return f(bgk_int<2>{}, bgk_int<3>{});
        if (kind == 4) return f(bgk_int<2>{}, bgk_int<4>{});
    }
    if (kind == 0) tile_dispatch_d(d, [&](auto D) { f(D, bgk_int<0>{}); });
    else if (kind == 1) tile_dispatch_d(d, [&](auto D) { f(D, bgk_int<1>{}); });
    else tile_dispatch_d(d, [&](auto D) { f(D, bgk_int<2>{}); });
}

/* one wave per workgroup */
template <class Kernel, class Args>
void tile_launch(Kernel kernel, int grid, size_t lds, hipStream_t s, const Args& a) {
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(BGK_TILE_THREADS), lds, s, a);
}

#endif
