/* bgk_pair.hip -- the many-particle targets and their prior: energies over ONE tensor x [B, n d] of n particles in d dimensions
 *   kind 0  LennardJonesPotential (bgflow/distribution/energy/lennard_jones.py:9-64, utils/geometry.py:93-111):
 *           eps sum_{i<j} [(rm / r_ij)^12 - 2 (rm / r_ij)^6],  r_ij^2 = |x_i - x_j|^2 + 1e-6 (the eps inside the root)
 *           + osc_scale 0.5 sum_i |x_i - xbar|^2 (the `oscillator`; osc_scale = 0: none), xbar the sample's centroid
 *   kind 1  MultiDoubleWellPotential (energy/multi_double_well_potential.py:37-43, utils/geometry.py:134-139):
 *           sum_{i<j} [a (d_ij - off)^4 + b (d_ij - off)^2 + c],  d_ij = |x_i - x_j| (no eps)
 *   kind 2  MeanFreeNormalDistribution (distribution/normal.py:267-283): osc_scale 0.5 sum_i |x_i - xbar|^2, osc_scale = 1 / std^2
 *   kind 3 / 4  the particle box, RepulsiveParticles / HarmonicParticles (distribution/energy/particles.py:51-381), d = 2, through the
 *           bgk_box_* entries at the end of this file only: a pair term over i < j except the dimer's (0, 1), the dimer's terms and the
 *           walls' (formulas: bgk_pair_terms.h); parameters in BgkPairTarget::box; no hvp kernel
 * u = e / T.  The reference forms the [B, n, n, d] tensor of distance vectors (or the [B, n, n] cdist matrix) and reads it back
 * several times; here a sample is read once: roofline HBM, 4 (n d + 1) B per sample forward, 4 (2 n d + 1) B backward.
 *
 * Like bgk_energy.hip, by the rules of bgk_pair_tile.h (tiles of rows staged through LDS at the odd stride S, one lane per sample, a fixed
 * pair order).  A lane adds the terms
 * of one i in f32 and the n - 1 row sums (and the centroid term) in f64, so the summation error stays below the rounding of the terms.
 * The backward accumulates d e / d x of a sample in the lane's OWN row of a second LDS tile (g_i in registers over the j loop, g_j
 * read-modify-write: no atomics), then all lanes store the tile coalesced, scaled by g_row / T.  At d_ij = 0 the double-well pair
 * gradient is 0 (torch.cdist's backward), the Lennard-Jones one whatever the f32 arithmetic gives (r_ij = 1e-3).
 * Optional epilogue as in energy_fields_kernel: block partials [sum (u - dlogp), n kept] finished by bgk_loss_partial_reduce; the
 * backward's loss-sum form (g_u == NULL) then also writes g_dlogp.
 *
 * Envelope (bgk_pair_tile.h): n d <= 192, S <= 193.  Dynamic LDS below 64 KiB:
 *   forward   64 rows:  64 x 193 x 4 B = 49,408 B at n d = 192 (three workgroups per CU; LJ13: 64 x 39 x 4 = 9,984 B)
 *   backward  x tile + gradient tile + 64 row scales: 64 rows while 2 x 64 x S x 4 + 256 <= 65,536 B (S <= 127: 65,280 B),
 *             else 32 rows: 2 x 32 x 193 x 4 + 256 = 49,664 B at n d = 192 (lanes 32..63 only stage and store).
 *   hvp       tiles x, u, g, Hu: the most rows (<= 64) with 4 rows S 4 B <= 65,536 B: 21 rows, 64,848 B at n d = 192; 64 rows at S <= 64
 *             (LJ13: 39,936 B).  g and Hu = (d^2 e / d x^2) u of a sample in one pass over its pairs (bgk_pair_row_hvp).
 *   the particle box of 38 particles (S = 77): forward 19,712 B, backward 39,680 B at 64 rows; 64 particles (S = 129): 33,024 B and
 *             33,280 B at 32 rows */
#include "bgk_common.h"
#include "bgk_pair_terms.h"

namespace {

constexpr int PR_LDS_LIMIT = 65536;

struct PairArgs {
    const float* x; int64_t ldx; int64_t B;
    BgkPairTarget t; int rows;                          /* rows per tile */
    float inv_t;
    float* u; const float* dlogp; int drop_nonfinite; float* partial;                     /* forward (+ loss partials [gridDim.x][2]) */
    const float* g_u; const float* g_scalar; float* g_dlogp; float* g_x; int64_t ldg;     /* backward */
    const float* vec; float* hu;                                                          /* Hessian-vector product (contiguous rows) */
};

template <int D, int KIND>
__global__ __launch_bounds__(BGK_TILE_THREADS) void pair_energy_kernel(PairArgs a) {
    extern __shared__ float s_x[];
    __shared__ float s_red[2 * BGK_TILE_THREADS];
    const int tid = threadIdx.x, S = a.t.nd | 1;
    const int64_t n_tiles = (a.B + a.rows - 1) / a.rows;
    float bsum = 0.0f, bcnt = 0.0f;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t b0 = tile * a.rows;
        const int rows = (int)((a.B - b0) < a.rows ? (a.B - b0) : a.rows);
        tile_stage_ld(a.x, a.ldx, b0, rows, a.t.nd, a.t.magic, s_x);
        __syncthreads();
        if (tid < rows) {
            const double e = bgk_row_energy<D, KIND>(s_x + tid * S, a.t);                              /* bgk_pair_terms.h */
            const float u = (float)e * a.inv_t;
            a.u[b0 + tid] = u;
            if (a.partial) {
                const float loss = u - a.dlogp[b0 + tid];
                const bool ok = !a.drop_nonfinite || __builtin_isfinite(loss);
                bsum += ok ? loss : 0.0f;
                bcnt += ok ? 1.0f : 0.0f;
            }
        }
        __syncthreads();
    }
    if (a.partial) {                   /* block partial: fixed order over the 64 row lanes */
        s_red[tid] = bsum; s_red[BGK_TILE_THREADS + tid] = bcnt;
        __syncthreads();
        if (tid == 0) {
            float s = 0.0f, c = 0.0f;
            for (int i = 0; i < BGK_TILE_THREADS; ++i) { s += s_red[i]; c += s_red[BGK_TILE_THREADS + i]; }
            a.partial[2 * blockIdx.x] = s; a.partial[2 * blockIdx.x + 1] = c;
        }
    }
}

template <int D, int KIND>
__global__ __launch_bounds__(BGK_TILE_THREADS) void pair_energy_bwd_kernel(PairArgs a) {
    extern __shared__ float s_mem[];
    const int tid = threadIdx.x, nd = a.t.nd, S = nd | 1;
    float* s_x = s_mem;
    float* s_g = s_mem + a.rows * S;
    float* s_scale = s_g + a.rows * S;                  /* [BGK_TILE_THREADS] g_row / T of the tile's rows */
    const int64_t n_tiles = (a.B + a.rows - 1) / a.rows;
    const float gs = a.g_scalar ? a.g_scalar[0] : 0.0f;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t b0 = tile * a.rows;
        const int rows = (int)((a.B - b0) < a.rows ? (a.B - b0) : a.rows);
        tile_stage_ld(a.x, a.ldx, b0, rows, nd, a.t.magic, s_x);
        __syncthreads();
        if (tid < rows) {
            const int64_t b = b0 + tid;
            float gr;
            if (a.g_u) gr = a.g_u[b];
            else gr = (!a.drop_nonfinite || __builtin_isfinite(a.u[b] - a.dlogp[b])) ? gs : 0.0f;
            if (a.g_dlogp) a.g_dlogp[b] = -gr;          /* d(sum_i (u_i - dlogp_i)) / d dlogp_i = -1 for the kept samples */
            s_scale[tid] = gr * a.inv_t;
            bgk_row_gradient<D, KIND>(s_x + tid * S, s_g + tid * S, a.t);                                            /* bgk_pair_terms.h */
        }
        __syncthreads();
        for (int i = tid; i < rows * nd; i += BGK_TILE_THREADS) {    /* tile_store, scaled by the row's g / T */
            const int r = (int)__umulhi((unsigned)i, a.t.magic), c = i - r * nd;
            a.g_x[(b0 + r) * a.ldg + c] = s_g[r * S + c] * s_scale[r];
        }
        __syncthreads();
    }
}

/* g = (d e / d x)(x) / T and Hu = (d^2 e / d x^2)(x) u / T of every row: tiles x, u, g, Hu; bgk_pair_row_hvp of bgk_pair_terms.h */
template <int D, int KIND>
__global__ __launch_bounds__(BGK_TILE_THREADS) void pair_energy_hvp_kernel(PairArgs a) {
    extern __shared__ float s_mem[];
    const int tid = threadIdx.x, nd = a.t.nd, S = nd | 1, T = a.rows * S;
    float* s_x = s_mem;
    const int64_t n_tiles = (a.B + a.rows - 1) / a.rows;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t b0 = tile * a.rows;
        const int rows = (int)((a.B - b0) < a.rows ? (a.B - b0) : a.rows);
        tile_stage_ld(a.x, a.ldx, b0, rows, nd, a.t.magic, s_x);
        tile_stage(a.vec, b0, rows, nd, a.t.magic, s_mem + T);
        __syncthreads();
        if (tid < rows)
            bgk_pair_row_hvp<D, KIND>(s_x + tid * S, s_mem + T + tid * S, s_mem + 2 * T + tid * S, s_mem + 3 * T + tid * S, a.t);
        __syncthreads();
        for (int i = tid; i < rows * nd; i += BGK_TILE_THREADS) {    /* tile_store of two tiles, scaled by 1 / T */
            const int r = (int)__umulhi((unsigned)i, a.t.magic), c = i - r * nd;
            if (a.g_x) a.g_x[(b0 + r) * nd + c] = s_mem[2 * T + r * S + c] * a.inv_t;
            a.hu[(b0 + r) * nd + c] = s_mem[3 * T + r * S + c] * a.inv_t;
        }
        __syncthreads();
    }
}

/* the head every entry of this file shares: the target as the entry names it (bgk_pair_spec / bgk_box_spec), the rows, the temperature */
struct BgkPairCall {
    BgkPairSpec spec;
    const float* x; int64_t ldx; int64_t B; double temperature; void* stream;
};

int pair_common(const BgkPairCall& c, PairArgs* a) {
    BGK_CHECK_ARG(c.B >= 0 && c.temperature > 0.0, "%s: bad batch size / temperature", c.spec.what);
    const int st = bgk_pair_target(c.spec, &a->t);
    if (st) return st;
    a->x = c.x; a->ldx = c.ldx; a->B = c.B;
    a->inv_t = (float)(1.0 / c.temperature);
    return 0;
}

/* loss_sums != NULL: also the KL loss sums, over dlogp, through the [nblk, 2] workspace `partial` */
int pair_forward(const BgkPairCall& c, float* u, const float* dlogp, int32_t drop_nonfinite, float* partial, int32_t nblk, double* loss_sums) {
    const char* what = c.spec.what;
    PairArgs a{};
    const int st = pair_common(c, &a);
    if (st) return st;
    BGK_CHECK_ARG(!loss_sums || (dlogp && partial && nblk >= 1), "%s: the loss sums need dlogp and a [nblk, 2] workspace", what);
    hipStream_t s = (hipStream_t)c.stream;
    if (c.B == 0) {             /* an empty batch (its tensors have no storage: null pointers): the loss sums are zero */
        if (loss_sums) { hipError_t e = hipMemsetAsync(loss_sums, 0, 2 * sizeof(double), s); if (e != hipSuccess) return (int)e; }
        return 0;
    }
    BGK_CHECK_ARG(c.x && u && c.ldx >= a.t.nd, "%s: null tensor / row stride", what);
    a.rows = BGK_TILE_THREADS;
    a.u = u; a.drop_nonfinite = drop_nonfinite;
    if (loss_sums) { a.dlogp = dlogp; a.partial = partial; }
    const size_t lds = (size_t)a.rows * (a.t.nd | 1) * sizeof(float);
    int grid = tile_grid(c.B, a.rows);
    if (loss_sums && grid > nblk) grid = nblk;
    tile_dispatch<true>(c.spec.kind, c.spec.n_dims, [&](auto D, auto K) { tile_launch(pair_energy_kernel<D(), K()>, grid, lds, s, a); });
    const int st2 = bgk_launch_status(what);
    if (st2 || !loss_sums) return st2;
    return bgk_loss_partial_reduce(partial, grid, loss_sums, c.stream);
}

/* g_u [B], or the loss-sum form (g_scalar, u_saved, dlogp, drop_nonfinite) that also writes g_dlogp */
int pair_backward(const BgkPairCall& c, const float* g_u, const float* g_scalar, const float* u_saved, const float* dlogp,
                  int32_t drop_nonfinite, float* g_dlogp, float* g_x, int64_t ldg) {
    const char* what = c.spec.what;
    PairArgs a{};
    const int st = pair_common(c, &a);
    if (st) return st;
    BGK_CHECK_ARG(g_u || (g_scalar && u_saved && dlogp), "%s: need g_u [B] or (g_scalar, u, dlogp)", what);
    if (c.B == 0) return 0;
    BGK_CHECK_ARG(c.x && g_x && c.ldx >= a.t.nd && ldg >= a.t.nd, "%s: null tensor / row stride", what);
    const int S = a.t.nd | 1;
    const int bytes_at_64 = (2 * BGK_TILE_THREADS * S + BGK_TILE_THREADS) * (int)sizeof(float);     /* x tile, gradient tile, row scales */
    a.rows = bytes_at_64 <= PR_LDS_LIMIT ? BGK_TILE_THREADS : BGK_TILE_THREADS / 2;
    a.u = const_cast<float*>(u_saved); a.dlogp = dlogp; a.drop_nonfinite = drop_nonfinite;
    a.g_u = g_u; a.g_scalar = g_scalar; a.g_dlogp = g_dlogp; a.g_x = g_x; a.ldg = ldg;
    const size_t lds = ((size_t)2 * a.rows * S + BGK_TILE_THREADS) * sizeof(float);
    const int grid = tile_grid(c.B, a.rows);
    hipStream_t s = (hipStream_t)c.stream;
    tile_dispatch<true>(c.spec.kind, c.spec.n_dims, [&](auto D, auto K) { tile_launch(pair_energy_bwd_kernel<D(), K()>, grid, lds, s, a); });
    return bgk_launch_status(what);
}

int pair_hvp(const BgkPairCall& c, const float* vec, float* g_out, float* hu) {
    const char* what = c.spec.what;
    PairArgs a{};
    const int st = pair_common(c, &a);
    if (st) return st;
    if (c.B == 0) return 0;
    BGK_CHECK_ARG(c.x && vec && hu && c.ldx >= a.t.nd, "%s: null tensor / row stride", what);
    const int bytes_per_row = 4 * (a.t.nd | 1) * (int)sizeof(float);
    a.rows = rows_within(PR_LDS_LIMIT, bytes_per_row);
    a.vec = vec; a.hu = hu; a.g_x = g_out;
    const size_t lds = (size_t)a.rows * bytes_per_row;
    const int grid = tile_grid(c.B, a.rows);
    hipStream_t s = (hipStream_t)c.stream;
    tile_dispatch<false>(c.spec.kind, c.spec.n_dims, [&](auto D, auto K) { tile_launch(pair_energy_hvp_kernel<D(), K()>, grid, lds, s, a); });
    return bgk_launch_status(what);
}

}  // namespace

extern "C" int bgk_pair_energy(const float* x, int64_t ldx, int64_t B, int32_t n_particles, int32_t n_dims, int32_t kind,
                               double p0, double p1, double p2, double p3, double osc_scale, double temperature,
                               float* u, void* stream) {
    const BgkPairSpec spec = bgk_pair_spec("bgk_pair_energy", n_particles, n_dims, kind, p0, p1, p2, p3, osc_scale);
    return pair_forward({spec, x, ldx, B, temperature, stream}, u, nullptr, 0, nullptr, 0, nullptr);
}

extern "C" int bgk_pair_energy_kl_sums(const float* x, int64_t ldx, int64_t B, int32_t n_particles, int32_t n_dims, int32_t kind,
                                       double p0, double p1, double p2, double p3, double osc_scale, double temperature,
                                       float* u, const float* dlogp, int32_t drop_nonfinite, float* partial, int32_t nblk,
                                       double* loss_sums, void* stream) {
    BGK_CHECK_ARG(loss_sums, "bgk_pair_energy_kl_sums: loss_sums is NULL");
    const BgkPairSpec spec = bgk_pair_spec("bgk_pair_energy_kl_sums", n_particles, n_dims, kind, p0, p1, p2, p3, osc_scale);
    return pair_forward({spec, x, ldx, B, temperature, stream}, u, dlogp, drop_nonfinite, partial, nblk, loss_sums);
}

extern "C" int bgk_pair_energy_backward(const float* x, int64_t ldx, int64_t B, int32_t n_particles, int32_t n_dims, int32_t kind,
                                        double p0, double p1, double p2, double p3, double osc_scale, double temperature,
                                        const float* g_u, const float* g_scalar, const float* u, const float* dlogp,
                                        int32_t drop_nonfinite, float* g_dlogp, float* g_x, int64_t ldg, void* stream) {
    const BgkPairSpec spec = bgk_pair_spec("bgk_pair_energy_backward", n_particles, n_dims, kind, p0, p1, p2, p3, osc_scale);
    return pair_backward({spec, x, ldx, B, temperature, stream}, g_u, g_scalar, u, dlogp, drop_nonfinite, g_dlogp, g_x, ldg);
}

extern "C" int bgk_pair_energy_hvp(const float* x, int64_t ldx, int64_t B, int32_t n_particles, int32_t n_dims, int32_t kind,
                                   double p0, double p1, double p2, double p3, double osc_scale, double temperature,
                                   const float* u, float* g_out, float* hu_out, void* stream) {
    const BgkPairSpec spec = bgk_pair_spec("bgk_pair_energy_hvp", n_particles, n_dims, kind, p0, p1, p2, p3, osc_scale);
    return pair_hvp({spec, x, ldx, B, temperature, stream}, u, g_out, hu_out);
}

/* The particle box (kinds 3 / 4 of bgk_pair_terms.h) on the same kernels: RepulsiveParticles._energy / HarmonicParticles._energy
 * (bgflow/distribution/energy/particles.py:99-123, 191-210, 235-254, 272-277, 354-381) and, backward, what autograd makes of them (for the
 * repulsive kind also force(), particles.py:161-189, 212-233, 256-270, 324-327).  Two dimensions; params: BGK_BOX_N_PARAMS host floats. */
extern "C" int bgk_box_energy(const float* x, int64_t ldx, int64_t B, int32_t n_particles, int32_t kind, const float* params,
                              int32_t n_params, double temperature, float* u, void* stream) {
    const BgkPairSpec spec = bgk_box_spec("bgk_box_energy", n_particles, kind, params, n_params);
    return pair_forward({spec, x, ldx, B, temperature, stream}, u, nullptr, 0, nullptr, 0, nullptr);
}

extern "C" int bgk_box_energy_kl_sums(const float* x, int64_t ldx, int64_t B, int32_t n_particles, int32_t kind, const float* params,
                                      int32_t n_params, double temperature, float* u, const float* dlogp, int32_t drop_nonfinite,
                                      float* partial, int32_t nblk, double* loss_sums, void* stream) {
    BGK_CHECK_ARG(loss_sums, "bgk_box_energy_kl_sums: loss_sums is NULL");
    const BgkPairSpec spec = bgk_box_spec("bgk_box_energy_kl_sums", n_particles, kind, params, n_params);
    return pair_forward({spec, x, ldx, B, temperature, stream}, u, dlogp, drop_nonfinite, partial, nblk, loss_sums);
}

extern "C" int bgk_box_energy_backward(const float* x, int64_t ldx, int64_t B, int32_t n_particles, int32_t kind, const float* params,
                                       int32_t n_params, double temperature, const float* g_u, const float* g_scalar, const float* u,
                                       const float* dlogp, int32_t drop_nonfinite, float* g_dlogp, float* g_x, int64_t ldg,
                                       void* stream) {
    const BgkPairSpec spec = bgk_box_spec("bgk_box_energy_backward", n_particles, kind, params, n_params);
    return pair_backward({spec, x, ldx, B, temperature, stream}, g_u, g_scalar, u, dlogp, drop_nonfinite, g_dlogp, g_x, ldg);
}
