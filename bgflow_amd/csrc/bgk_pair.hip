/* bgk_pair.hip -- the many-particle targets and their prior: energies over ONE tensor x [B, n d] of n particles in d dimensions
 *   kind 0  LennardJonesPotential (bgflow/distribution/energy/lennard_jones.py:9-64, utils/geometry.py:93-111):
 *           eps sum_{i<j} [(rm / r_ij)^12 - 2 (rm / r_ij)^6],  r_ij^2 = |x_i - x_j|^2 + 1e-6 (the eps inside the root)
 *           + osc_scale 0.5 sum_i |x_i - xbar|^2 (the `oscillator`; osc_scale = 0: none), xbar the sample's centroid
 *   kind 1  MultiDoubleWellPotential (energy/multi_double_well_potential.py:37-43, utils/geometry.py:134-139):
 *           sum_{i<j} [a (d_ij - off)^4 + b (d_ij - off)^2 + c],  d_ij = |x_i - x_j| (no eps)
 *   kind 2  MeanFreeNormalDistribution (distribution/normal.py:267-283): osc_scale 0.5 sum_i |x_i - xbar|^2, osc_scale = 1 / std^2
 *   kind 3 / 4  the particle box, RepulsiveParticles / HarmonicParticles (distribution/energy/particles.py:51-381), d = 2, through the
 *           bgk_box_* entries at the end of this file only: a pair term over i < j except the dimer's (0, 1), the dimer's terms and the
 *           walls' (formulas: bgk_pair_terms.h); parameters in PairArgs::box; no hvp kernel
 * u = e / T.  The reference forms the [B, n, n, d] tensor of distance vectors (or the [B, n, n] cdist matrix) and reads it back
 * several times; here a sample is read once: roofline HBM, 4 (n d + 1) B per sample forward, 4 (2 n d + 1) B backward.
 *
 * Like bgk_energy.hip: a tile of rows is staged coalesced through LDS with an odd row stride S = (n d) | 1 (lane r reads word
 * r S + k: 64 distinct banks), one lane per sample, pairs in the fixed ascending (i, j) order -- deterministic.  A lane adds the terms
 * of one i in f32 and the n - 1 row sums (and the centroid term) in f64, so the summation error stays below the rounding of the terms.
 * The backward accumulates d e / d x of a sample in the lane's OWN row of a second LDS tile (g_i in registers over the j loop, g_j
 * read-modify-write: no atomics), then all lanes store the tile coalesced, scaled by g_row / T.  At d_ij = 0 the double-well pair
 * gradient is 0 (torch.cdist's backward), the Lennard-Jones one whatever the f32 arithmetic gives (r_ij = 1e-3).
 * Optional epilogue as in energy_fields_kernel: block partials [sum (u - dlogp), n kept] finished by bgk_loss_partial_reduce; the
 * backward's loss-sum form (g_u == NULL) then also writes g_dlogp.
 *
 * Envelope 2 <= n <= 64, 1 <= d <= 3, i.e. n d <= 192, S <= 193.  One wave per workgroup, dynamic LDS below 64 KiB:
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

constexpr int PR_THREADS = 64;        /* one wave: rows of a tile <= lanes */
constexpr int PR_MAX_N = 64, PR_MAX_D = 3;
constexpr int PR_LDS_LIMIT = 65536;

struct PairArgs {
    const float* x; int64_t ldx; int64_t B;
    int n, nd, rows; uint32_t magic;                    /* rows per tile; magic: i / nd by multiply-high for i < 64 * 192 */
    float p0, p1, p2, p3, osc, inv_t;
    BgkBoxParams box;                                   /* kinds 3 / 4 (the particle box) */
    float* u; const float* dlogp; int drop_nonfinite; float* partial;                     /* forward (+ loss partials [gridDim.x][2]) */
    const float* g_u; const float* g_scalar; float* g_dlogp; float* g_x; int64_t ldg;     /* backward */
    const float* vec; float* hu;                                                          /* Hessian-vector product (contiguous rows) */
};

/* stage rows [b0, b0 + rows) of x into s_x (row stride S), every lane of the wave */
__device__ __forceinline__ void stage_rows(const PairArgs& a, int64_t b0, int rows, int S, float* s_x) {
    for (int i = threadIdx.x; i < rows * a.nd; i += PR_THREADS) {
        const int r = (int)__umulhi((unsigned)i, a.magic), c = i - r * a.nd;
        s_x[r * S + c] = a.x[(b0 + r) * a.ldx + c];
    }
}

template <int D, int KIND>
__global__ __launch_bounds__(PR_THREADS) void pair_energy_kernel(PairArgs a) {
    extern __shared__ float s_x[];
    __shared__ float s_red[2 * PR_THREADS];
    const int tid = threadIdx.x, n = a.n, S = a.nd | 1;
    const int64_t n_tiles = (a.B + a.rows - 1) / a.rows;
    const float rm2 = a.p1 * a.p1;
    float bsum = 0.0f, bcnt = 0.0f;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t b0 = tile * a.rows;
        const int rows = (int)((a.B - b0) < a.rows ? (a.B - b0) : a.rows);
        stage_rows(a, b0, rows, S, s_x);
        __syncthreads();
        if (tid < rows) {
            const float* xr = s_x + tid * S;
            double e;                                                                                   /* bgk_pair_terms.h */
            if constexpr (KIND >= 3) e = bgk_box_row_energy<KIND>(xr, n, a.box);
            else e = bgk_pair_row_energy<D, KIND>(xr, n, a.p0, a.p1, a.p2, a.p3, rm2, a.osc);
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
        s_red[tid] = bsum; s_red[PR_THREADS + tid] = bcnt;
        __syncthreads();
        if (tid == 0) {
            float s = 0.0f, c = 0.0f;
            for (int i = 0; i < PR_THREADS; ++i) { s += s_red[i]; c += s_red[PR_THREADS + i]; }
            a.partial[2 * blockIdx.x] = s; a.partial[2 * blockIdx.x + 1] = c;
        }
    }
}

template <int D, int KIND>
__global__ __launch_bounds__(PR_THREADS) void pair_energy_bwd_kernel(PairArgs a) {
    extern __shared__ float s_mem[];
    const int tid = threadIdx.x, n = a.n, S = a.nd | 1;
    float* s_x = s_mem;
    float* s_g = s_mem + a.rows * S;
    float* s_scale = s_g + a.rows * S;                  /* [PR_THREADS] g_row / T of the tile's rows */
    const int64_t n_tiles = (a.B + a.rows - 1) / a.rows;
    const float gs = a.g_scalar ? a.g_scalar[0] : 0.0f;
    const float rm2 = a.p1 * a.p1, c12 = -12.0f * a.p0 / rm2;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t b0 = tile * a.rows;
        const int rows = (int)((a.B - b0) < a.rows ? (a.B - b0) : a.rows);
        stage_rows(a, b0, rows, S, s_x);
        __syncthreads();
        if (tid < rows) {
            const int64_t b = b0 + tid;
            float gr;
            if (a.g_u) gr = a.g_u[b];
            else gr = (!a.drop_nonfinite || __builtin_isfinite(a.u[b] - a.dlogp[b])) ? gs : 0.0f;
            if (a.g_dlogp) a.g_dlogp[b] = -gr;          /* d(sum_i (u_i - dlogp_i)) / d dlogp_i = -1 for the kept samples */
            s_scale[tid] = gr * a.inv_t;
            if constexpr (KIND >= 3) bgk_box_row_gradient<KIND>(s_x + tid * S, s_g + tid * S, n, a.box);              /* bgk_pair_terms.h */
            else bgk_pair_row_gradient<D, KIND>(s_x + tid * S, s_g + tid * S, n, a.p0, a.p1, a.p3, rm2, c12, a.osc);
        }
        __syncthreads();
        for (int i = tid; i < rows * a.nd; i += PR_THREADS) {
            const int r = (int)__umulhi((unsigned)i, a.magic), c = i - r * a.nd;
            a.g_x[(b0 + r) * a.ldg + c] = s_g[r * S + c] * s_scale[r];
        }
        __syncthreads();
    }
}

/* g = (d e / d x)(x) / T and Hu = (d^2 e / d x^2)(x) u / T of every row: tiles x, u, g, Hu; bgk_pair_row_hvp of bgk_pair_terms.h */
template <int D, int KIND>
__global__ __launch_bounds__(PR_THREADS) void pair_energy_hvp_kernel(PairArgs a) {
    extern __shared__ float s_mem[];
    const int tid = threadIdx.x, n = a.n, nd = a.nd, S = a.nd | 1, T = a.rows * S;
    float* s_x = s_mem;
    const int64_t n_tiles = (a.B + a.rows - 1) / a.rows;
    const float rm2 = a.p1 * a.p1, c12 = -12.0f * a.p0 / rm2;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t b0 = tile * a.rows;
        const int rows = (int)((a.B - b0) < a.rows ? (a.B - b0) : a.rows);
        stage_rows(a, b0, rows, S, s_x);
        for (int i = tid; i < rows * nd; i += PR_THREADS) {
            const int r = (int)__umulhi((unsigned)i, a.magic), c = i - r * nd;
            s_mem[T + r * S + c] = a.vec[(b0 + r) * nd + c];
        }
        __syncthreads();
        if (tid < rows)
            bgk_pair_row_hvp<D, KIND>(s_x + tid * S, s_mem + T + tid * S, s_mem + 2 * T + tid * S, s_mem + 3 * T + tid * S, n, a.p0, a.p1,
                                      a.p3, rm2, c12, a.osc);
        __syncthreads();
        for (int i = tid; i < rows * nd; i += PR_THREADS) {
            const int r = (int)__umulhi((unsigned)i, a.magic), c = i - r * nd;
            if (a.g_x) a.g_x[(b0 + r) * nd + c] = s_mem[2 * T + r * S + c] * a.inv_t;
            a.hu[(b0 + r) * nd + c] = s_mem[3 * T + r * S + c] * a.inv_t;
        }
        __syncthreads();
    }
}

template <int KIND>
void launch_fwd(int d, int grid, size_t lds, hipStream_t s, const PairArgs& a) {
    if (d == 1) hipLaunchKernelGGL((pair_energy_kernel<1, KIND>), dim3(grid), dim3(PR_THREADS), lds, s, a);
    else if (d == 2) hipLaunchKernelGGL((pair_energy_kernel<2, KIND>), dim3(grid), dim3(PR_THREADS), lds, s, a);
    else hipLaunchKernelGGL((pair_energy_kernel<3, KIND>), dim3(grid), dim3(PR_THREADS), lds, s, a);
}

template <int KIND>
void launch_bwd(int d, int grid, size_t lds, hipStream_t s, const PairArgs& a) {
    if (d == 1) hipLaunchKernelGGL((pair_energy_bwd_kernel<1, KIND>), dim3(grid), dim3(PR_THREADS), lds, s, a);
    else if (d == 2) hipLaunchKernelGGL((pair_energy_bwd_kernel<2, KIND>), dim3(grid), dim3(PR_THREADS), lds, s, a);
    else hipLaunchKernelGGL((pair_energy_bwd_kernel<3, KIND>), dim3(grid), dim3(PR_THREADS), lds, s, a);
}

template <int KIND>
void launch_hvp(int d, int grid, size_t lds, hipStream_t s, const PairArgs& a) {
    if (d == 1) hipLaunchKernelGGL((pair_energy_hvp_kernel<1, KIND>), dim3(grid), dim3(PR_THREADS), lds, s, a);
    else if (d == 2) hipLaunchKernelGGL((pair_energy_hvp_kernel<2, KIND>), dim3(grid), dim3(PR_THREADS), lds, s, a);
    else hipLaunchKernelGGL((pair_energy_hvp_kernel<3, KIND>), dim3(grid), dim3(PR_THREADS), lds, s, a);
}

/* one call of the pair-energy launchers, filled by field name in the extern "C" entries */
struct BgkPairCall {
    const char* what;
    const float* x; int64_t ldx; int64_t B; int32_t n_particles, n_dims, kind;
    double p0, p1, p2, p3, osc_scale, temperature;
    float* u; const float* dlogp; int32_t drop_nonfinite; float* partial; int32_t nblk; double* loss_sums;     /* forward */
    const float* g_u; const float* g_scalar; const float* u_saved; float* g_dlogp; float* g_x; int64_t ldg;   /* backward */
    const float* box_params; int32_t n_box_params; int32_t is_box;     /* the bgk_box_* entries: kinds 3 / 4, host parameters */
    void* stream;
};

int pair_common(const BgkPairCall& c, PairArgs* a) {
    BGK_CHECK_ARG(c.B >= 0 && c.temperature > 0.0, "%s: bad batch size / temperature", c.what);
    if (c.is_box) {
        BGK_CHECK_ARG(c.kind == 3 || c.kind == 4, "%s: kind %d (3 repulsive particles, 4 harmonic particles)", c.what, c.kind);
        BGK_CHECK_ARG(c.box_params && c.n_box_params == BGK_BOX_N_PARAMS, "%s: params must be %d floats (see bgflow_amd.h)", c.what,
                      BGK_BOX_N_PARAMS);
    } else {
        BGK_CHECK_ARG(c.kind >= 0 && c.kind <= 2, "%s: kind %d (0 Lennard-Jones, 1 multi-double-well, 2 mean-free normal)", c.what, c.kind);
    }
    if (!(c.n_particles >= 2 && c.n_particles <= PR_MAX_N && c.n_dims >= 1 && c.n_dims <= PR_MAX_D)) {
        bgk_set_error("%s: %d particles in %d dimensions are outside the kernel's envelope (2..%d particles, 1..%d dimensions)", c.what,
                      c.n_particles, c.n_dims, PR_MAX_N, PR_MAX_D);
        return BGK_EUNSUPPORTED;
    }
    a->x = c.x; a->ldx = c.ldx; a->B = c.B; a->n = c.n_particles; a->nd = c.n_particles * c.n_dims;
    a->magic = (uint32_t)(((1ull << 32) + (uint64_t)a->nd - 1) / (uint64_t)a->nd);
    a->p0 = (float)c.p0; a->p1 = (float)c.p1; a->p2 = (float)c.p2; a->p3 = (float)c.p3; a->osc = (float)c.osc_scale;
    a->inv_t = (float)(1.0 / c.temperature);
    a->dlogp = c.dlogp; a->drop_nonfinite = c.drop_nonfinite;
    if (c.is_box) bgk_box_params_from_host(c.box_params, &a->box);
    return 0;
}

int pair_forward(const BgkPairCall& c) {
    PairArgs a{};
    const int st = pair_common(c, &a);
    if (st) return st;
    BGK_CHECK_ARG(!c.loss_sums || (c.dlogp && c.partial && c.nblk >= 1), "%s: the loss sums need dlogp and a [nblk, 2] workspace", c.what);
    hipStream_t s = (hipStream_t)c.stream;
    if (c.B == 0) {             /* an empty batch (its tensors have no storage: null pointers): the loss sums are zero */
        if (c.loss_sums) { hipError_t e = hipMemsetAsync(c.loss_sums, 0, 2 * sizeof(double), s); if (e != hipSuccess) return (int)e; }
        return 0;
    }
    BGK_CHECK_ARG(c.x && c.u && c.ldx >= a.nd, "%s: null tensor / row stride", c.what);
    a.rows = PR_THREADS;
    a.u = c.u; a.partial = c.loss_sums ? c.partial : nullptr; if (!c.loss_sums) a.dlogp = nullptr;
    const size_t lds = (size_t)a.rows * (a.nd | 1) * sizeof(float);
    const int64_t n_tiles = (c.B + a.rows - 1) / a.rows;
    int grid = (int)(n_tiles < 256 * 16 ? n_tiles : 256 * 16);
    if (c.loss_sums && grid > c.nblk) grid = c.nblk;
    if (c.kind == 0) launch_fwd<0>(c.n_dims, grid, lds, s, a);
    else if (c.kind == 1) launch_fwd<1>(c.n_dims, grid, lds, s, a);
    else if (c.kind == 2) launch_fwd<2>(c.n_dims, grid, lds, s, a);
    else if (c.kind == 3) hipLaunchKernelGGL((pair_energy_kernel<2, 3>), dim3(grid), dim3(PR_THREADS), lds, s, a);
    else hipLaunchKernelGGL((pair_energy_kernel<2, 4>), dim3(grid), dim3(PR_THREADS), lds, s, a);
    const int st2 = bgk_launch_status(c.what);
    if (st2 || !c.loss_sums) return st2;
    return bgk_loss_partial_reduce(c.partial, grid, c.loss_sums, c.stream);
}

int pair_backward(const BgkPairCall& c) {
    PairArgs a{};
    const int st = pair_common(c, &a);
    if (st) return st;
    BGK_CHECK_ARG(c.g_u || (c.g_scalar && c.u_saved && c.dlogp), "%s: need g_u [B] or (g_scalar, u, dlogp)", c.what);
    if (c.B == 0) return 0;
    BGK_CHECK_ARG(c.x && c.g_x && c.ldx >= a.nd && c.ldg >= a.nd, "%s: null tensor / row stride", c.what);
    const int S = a.nd | 1;
    a.rows = 2 * PR_THREADS * S * (int)sizeof(float) + PR_THREADS * (int)sizeof(float) <= PR_LDS_LIMIT ? PR_THREADS : PR_THREADS / 2;
    a.u = const_cast<float*>(c.u_saved); a.g_u = c.g_u; a.g_scalar = c.g_scalar; a.g_dlogp = c.g_dlogp; a.g_x = c.g_x; a.ldg = c.ldg;
    const size_t lds = ((size_t)2 * a.rows * S + PR_THREADS) * sizeof(float);
    const int64_t n_tiles = (c.B + a.rows - 1) / a.rows;
    const int grid = (int)(n_tiles < 256 * 16 ? n_tiles : 256 * 16);
    hipStream_t s = (hipStream_t)c.stream;
    if (c.kind == 0) launch_bwd<0>(c.n_dims, grid, lds, s, a);
    else if (c.kind == 1) launch_bwd<1>(c.n_dims, grid, lds, s, a);
    else if (c.kind == 2) launch_bwd<2>(c.n_dims, grid, lds, s, a);
    else if (c.kind == 3) hipLaunchKernelGGL((pair_energy_bwd_kernel<2, 3>), dim3(grid), dim3(PR_THREADS), lds, s, a);
    else hipLaunchKernelGGL((pair_energy_bwd_kernel<2, 4>), dim3(grid), dim3(PR_THREADS), lds, s, a);
    return bgk_launch_status(c.what);
}

int pair_hvp(const BgkPairCall& c, const float* vec, float* hu) {
    PairArgs a{};
    const int st = pair_common(c, &a);
    if (st) return st;
    if (c.B == 0) return 0;
    BGK_CHECK_ARG(c.x && vec && hu && c.ldx >= a.nd, "%s: null tensor / row stride", c.what);
    const int S = a.nd | 1;
    a.rows = PR_THREADS;
    while (4 * a.rows * S * (int)sizeof(float) > PR_LDS_LIMIT) --a.rows;
    a.vec = vec; a.hu = hu; a.g_x = c.g_x;
    const size_t lds = (size_t)4 * a.rows * S * sizeof(float);
    const int64_t n_tiles = (c.B + a.rows - 1) / a.rows;
    const int grid = (int)(n_tiles < 256 * 16 ? n_tiles : 256 * 16);
    hipStream_t s = (hipStream_t)c.stream;
    if (c.kind == 0) launch_hvp<0>(c.n_dims, grid, lds, s, a);
    else if (c.kind == 1) launch_hvp<1>(c.n_dims, grid, lds, s, a);
    else launch_hvp<2>(c.n_dims, grid, lds, s, a);
    return bgk_launch_status(c.what);
}

}  // namespace

extern "C" int bgk_pair_energy(const float* x, int64_t ldx, int64_t B, int32_t n_particles, int32_t n_dims, int32_t kind,
                               double p0, double p1, double p2, double p3, double osc_scale, double temperature,
                               float* u, void* stream) {
    BgkPairCall c{};
    c.what = "bgk_pair_energy";
    c.x = x; c.ldx = ldx; c.B = B; c.n_particles = n_particles; c.n_dims = n_dims; c.kind = kind;
    c.p0 = p0; c.p1 = p1; c.p2 = p2; c.p3 = p3; c.osc_scale = osc_scale; c.temperature = temperature;
    c.u = u; c.stream = stream;
    return pair_forward(c);
}

extern "C" int bgk_pair_energy_kl_sums(const float* x, int64_t ldx, int64_t B, int32_t n_particles, int32_t n_dims, int32_t kind,
                                       double p0, double p1, double p2, double p3, double osc_scale, double temperature,
                                       float* u, const float* dlogp, int32_t drop_nonfinite, float* partial, int32_t nblk,
                                       double* loss_sums, void* stream) {
    BGK_CHECK_ARG(loss_sums, "bgk_pair_energy_kl_sums: loss_sums is NULL");
    BgkPairCall c{};
    c.what = "bgk_pair_energy_kl_sums";
    c.x = x; c.ldx = ldx; c.B = B; c.n_particles = n_particles; c.n_dims = n_dims; c.kind = kind;
    c.p0 = p0; c.p1 = p1; c.p2 = p2; c.p3 = p3; c.osc_scale = osc_scale; c.temperature = temperature;
    c.u = u; c.dlogp = dlogp; c.drop_nonfinite = drop_nonfinite; c.partial = partial; c.nblk = nblk; c.loss_sums = loss_sums;
    c.stream = stream;
    return pair_forward(c);
}

extern "C" int bgk_pair_energy_backward(const float* x, int64_t ldx, int64_t B, int32_t n_particles, int32_t n_dims, int32_t kind,
                                        double p0, double p1, double p2, double p3, double osc_scale, double temperature,
                                        const float* g_u, const float* g_scalar, const float* u, const float* dlogp,
                                        int32_t drop_nonfinite, float* g_dlogp, float* g_x, int64_t ldg, void* stream) {
    BgkPairCall c{};
    c.what = "bgk_pair_energy_backward";
    c.x = x; c.ldx = ldx; c.B = B; c.n_particles = n_particles; c.n_dims = n_dims; c.kind = kind;
    c.p0 = p0; c.p1 = p1; c.p2 = p2; c.p3 = p3; c.osc_scale = osc_scale; c.temperature = temperature;
    c.g_u = g_u; c.g_scalar = g_scalar; c.u_saved = u; c.dlogp = dlogp; c.drop_nonfinite = drop_nonfinite;
    c.g_dlogp = g_dlogp; c.g_x = g_x; c.ldg = ldg; c.stream = stream;
    return pair_backward(c);
}

extern "C" int bgk_pair_energy_hvp(const float* x, int64_t ldx, int64_t B, int32_t n_particles, int32_t n_dims, int32_t kind,
                                   double p0, double p1, double p2, double p3, double osc_scale, double temperature,
                                   const float* u, float* g_out, float* hu_out, void* stream) {
    BgkPairCall c{};
    c.what = "bgk_pair_energy_hvp";
    c.x = x; c.ldx = ldx; c.B = B; c.n_particles = n_particles; c.n_dims = n_dims; c.kind = kind;
    c.p0 = p0; c.p1 = p1; c.p2 = p2; c.p3 = p3; c.osc_scale = osc_scale; c.temperature = temperature;
    c.g_x = g_out; c.stream = stream;
    return pair_hvp(c, u, hu_out);
}

/* The particle box (kinds 3 / 4 of bgk_pair_terms.h) on the same kernels: RepulsiveParticles._energy / HarmonicParticles._energy
 * (bgflow/distribution/energy/particles.py:99-123, 191-210, 235-254, 272-277, 354-381) and, backward, what autograd makes of them (for the
 * repulsive kind also force(), particles.py:161-189, 212-233, 256-270, 324-327).  Two dimensions; params: BGK_BOX_N_PARAMS host floats. */
extern "C" int bgk_box_energy(const float* x, int64_t ldx, int64_t B, int32_t n_particles, int32_t kind, const float* params,
                              int32_t n_params, double temperature, float* u, void* stream) {
    BgkPairCall c{};
    c.what = "bgk_box_energy";
    c.x = x; c.ldx = ldx; c.B = B; c.n_particles = n_particles; c.n_dims = 2; c.kind = kind;
    c.box_params = params; c.n_box_params = n_params; c.is_box = 1; c.temperature = temperature;
    c.u = u; c.stream = stream;
    return pair_forward(c);
}

extern "C" int bgk_box_energy_kl_sums(const float* x, int64_t ldx, int64_t B, int32_t n_particles, int32_t kind, const float* params,
                                      int32_t n_params, double temperature, float* u, const float* dlogp, int32_t drop_nonfinite,
                                      float* partial, int32_t nblk, double* loss_sums, void* stream) {
    BGK_CHECK_ARG(loss_sums, "bgk_box_energy_kl_sums: loss_sums is NULL");
    BgkPairCall c{};
    c.what = "bgk_box_energy_kl_sums";
    c.x = x; c.ldx = ldx; c.B = B; c.n_particles = n_particles; c.n_dims = 2; c.kind = kind;
    c.box_params = params; c.n_box_params = n_params; c.is_box = 1; c.temperature = temperature;
    c.u = u; c.dlogp = dlogp; c.drop_nonfinite = drop_nonfinite; c.partial = partial; c.nblk = nblk; c.loss_sums = loss_sums;
    c.stream = stream;
    return pair_forward(c);
}

extern "C" int bgk_box_energy_backward(const float* x, int64_t ldx, int64_t B, int32_t n_particles, int32_t kind, const float* params,
                                       int32_t n_params, double temperature, const float* g_u, const float* g_scalar, const float* u,
                                       const float* dlogp, int32_t drop_nonfinite, float* g_dlogp, float* g_x, int64_t ldg,
                                       void* stream) {
    BgkPairCall c{};
    c.what = "bgk_box_energy_backward";
    c.x = x; c.ldx = ldx; c.B = B; c.n_particles = n_particles; c.n_dims = 2; c.kind = kind;
    c.box_params = params; c.n_box_params = n_params; c.is_box = 1; c.temperature = temperature;
    c.g_u = g_u; c.g_scalar = g_scalar; c.u_saved = u; c.dlogp = dlogp; c.drop_nonfinite = drop_nonfinite;
    c.g_dlogp = g_dlogp; c.g_x = g_x; c.ldg = ldg; c.stream = stream;
    return pair_backward(c);
}
