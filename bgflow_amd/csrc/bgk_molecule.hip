/* bgk_molecule.hip -- a classical force-field energy over the Cartesian coordinates x [B, 3 n] of one molecule of n atoms (the target of
 * bgflow_amd/molecule.py::MolecularMechanicsEnergy): harmonic bonds and angles, periodic torsions, Lennard-Jones and Coulomb pairs with
 * exclusions and exceptions, in OpenMM's forms and units (HarmonicBondForce, HarmonicAngleForce, PeriodicTorsionForce, NonbondedForce
 * with NoCutoff; nm, kJ/mol, rad).  u = E / unit_energy / temperature.  The formulas and the table layout are in bgk_molecule_terms.h.
 *
 * By the rules of bgk_pair_tile.h: one wave per workgroup, ONE LANE PER SAMPLE, a tile of rows staged through LDS at the odd stride
 * S = (3 n) | 1, terms in table order and pairs in ascending (i, j) order, no atomics -- a row's result depends on that row alone, not on
 * its neighbours or the grid.  The backward accumulates d E / d x of a sample in the lane's OWN row of a second LDS tile, then all lanes
 * store the tile coalesced, scaled by g_row / (unit_energy temperature); a row whose scale is 0 (a sample the loss sums dropped) is
 * written as exact zeros.  The term tables are read wave-uniformly from `const __restrict__` memory, i.e. through the scalar cache.
 * Optional epilogue: the KL integrand's sums [sum (u - dlogp), n kept] in two stages in f64 -- a lane's rows, the wave (bgk_wave_reduce
 * of bgk_reduce.h), one f64 pair per workgroup; then ONE workgroup merges the pairs in a fixed order.
 *
 * Envelope: 2 <= n <= 64 (S <= 193), at most 256 bonds, 512 angles, 1024 torsion terms.  Dynamic LDS below 64 KiB:
 *   forward   64 rows: 64 x 193 x 4 B = 49,408 B at n = 64 (alanine dipeptide, n = 22, S = 67: 17,152 B)
 *   backward  x tile + gradient tile + 64 row scales: 64 rows while 2 x 64 x S x 4 + 256 <= 65,536 B (S <= 127; n = 22: 34,560 B),
 *             else 32 rows: 2 x 32 x 193 x 4 + 256 = 49,664 B at n = 64 (lanes 32..63 only stage and store)
 *
 * The bgk_molecule_solvent_* entries add an implicit solvent (Generalised Born, OBC2, plus the surface term; bgk_solvent_terms.h) in the SAME
 * launch on the row tile staged once: the kernels' SOLVENT instantiations run the vacuum functions unchanged, then the solvent functions
 * on the same LDS row.  Each lane owns an extension behind the tiles, at an odd stride: forward n | 1 floats (the Born radii), backward
 * (3 n) | 1 (B_i, d E / d B_i, the chain factors).  Rows per tile are the most of 64 / 32 / 16 that fit 64 KiB:
 *   forward   64 x (67 + 23) x 4 = 23,040 B at n = 22; n = 64: 64 x (193 + 65) x 4 = 66,048 B does not fit, 32 rows: 33,024 B
 *   backward  64 x (2 x 67 + 67) x 4 + 256 = 51,712 B at n = 22; n = 64: 16 rows, 16 x (2 x 193 + 193) x 4 + 256 = 37,312 B */
#include "bgk_common.h"
#include "bgk_pair_tile.h"
#include "bgk_reduce.h"
#include "bgk_molecule_terms.h"
#include "bgk_solvent_terms.h"

namespace {

constexpr int MM_LDS_LIMIT = 65536;

struct MolArgs {
    const float* x; int64_t B;
    BgkMolecule m; int nd; uint32_t magic; int rows;    /* nd = 3 n; magic: i / nd by multiply-high (tile_stage); rows per tile */
    float inv;                                          /* 1 / (unit_energy temperature) */
    float* u; const float* dlogp; int drop_nonfinite; double* partial;                    /* forward (+ loss partials [gridDim.x][2]) */
    const float* g_u; const float* g_scalar; float* g_dlogp; float* g_x;                  /* backward */
    BgkSolvent sv; int ext;                             /* the solvent kernels: the lane's stride in the extension after the tiles */
};

template <bool SOLVENT>
__global__ __launch_bounds__(BGK_TILE_THREADS) void molecule_energy_kernel(MolArgs a, const int4* __restrict__ terms,
                                                                            const float* __restrict__ pairs,
                                                                            const float4* __restrict__ atoms) {
    extern __shared__ float s_x[];
    const int tid = threadIdx.x, S = a.nd | 1;
    const int64_t n_tiles = (a.B + a.rows - 1) / a.rows;
    double bsum = 0.0, bcnt = 0.0;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t b0 = tile * a.rows;
        const int rows = (int)((a.B - b0) < a.rows ? (a.B - b0) : a.rows);
        tile_stage(a.x, b0, rows, a.nd, a.magic, s_x);
        __syncthreads();
        if (tid < rows) {
            float e = bgk_mm_row_energy(s_x + tid * S, terms, pairs, a.m);
            if constexpr (SOLVENT)                     /* E_vacuum + (E_GB + E_SA), on the same staged row; +inf + +inf stays +inf */
                e += bgk_gb_row_energy(s_x + tid * S, s_x + a.rows * S + tid * a.ext, atoms, a.sv);
            const float u = e * a.inv;
            a.u[b0 + tid] = u;
            if (a.partial) {
                const float loss = u - a.dlogp[b0 + tid];
                const bool ok = !a.drop_nonfinite || __builtin_isfinite(loss);
                bsum += ok ? (double)loss : 0.0;
                bcnt += ok ? 1.0 : 0.0;
            }
        }
        __syncthreads();
    }
    if (a.partial) {                   /* the wave's pair onto lane 0, in the fixed order of bgk_wave_reduce */
        bgk_wave_reduce(bsum, [](double& acc, double o) { acc += o; });
        bgk_wave_reduce(bcnt, [](double& acc, double o) { acc += o; });
        if (tid == 0) { a.partial[2 * blockIdx.x] = bsum; a.partial[2 * blockIdx.x + 1] = bcnt; }
    }
}

/* stage 2 of the loss sums: one wave, lane l adds the pairs l, l + 64, ... in ascending order, then the lanes merge */
__global__ __launch_bounds__(BGK_WAVE) void molecule_loss_merge_kernel(const double* partial, int n_partials, double* loss_sums) {
    double s = 0.0, c = 0.0;
    for (int i = threadIdx.x; i < n_partials; i += BGK_WAVE) { s += partial[2 * i]; c += partial[2 * i + 1]; }
    bgk_wave_reduce(s, [](double& acc, double o) { acc += o; });
    bgk_wave_reduce(c, [](double& acc, double o) { acc += o; });
    if (threadIdx.x == 0) { loss_sums[0] = s; loss_sums[1] = c; }
}

template <bool SOLVENT>
__global__ __launch_bounds__(BGK_TILE_THREADS) void molecule_energy_bwd_kernel(MolArgs a, const int4* __restrict__ terms,
                                                                                const float* __restrict__ pairs,
                                                                                const float4* __restrict__ atoms) {
    extern __shared__ float s_mem[];
    const int tid = threadIdx.x, nd = a.nd, S = nd | 1;
    float* s_x = s_mem;
    float* s_g = s_mem + a.rows * S;
    float* s_scale = s_g + a.rows * S;                  /* [BGK_TILE_THREADS] g_row / (unit_energy T) of the tile's rows */
    const int64_t n_tiles = (a.B + a.rows - 1) / a.rows;
    const float gs = a.g_scalar ? a.g_scalar[0] : 0.0f;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t b0 = tile * a.rows;
        const int rows = (int)((a.B - b0) < a.rows ? (a.B - b0) : a.rows);
        tile_stage(a.x, b0, rows, nd, a.magic, s_x);
        __syncthreads();
        if (tid < rows) {
            const int64_t b = b0 + tid;
            float gr;
            if (a.g_u) gr = a.g_u[b];
            else gr = (!a.drop_nonfinite || __builtin_isfinite(a.u[b] - a.dlogp[b])) ? gs : 0.0f;
            if (a.g_dlogp) a.g_dlogp[b] = -gr;          /* d(sum_i (u_i - dlogp_i)) / d dlogp_i = -1 for the kept samples */
            s_scale[tid] = gr * a.inv;
            bgk_mm_row_gradient(s_x + tid * S, s_g + tid * S, terms, pairs, a.m);
            if constexpr (SOLVENT)
                bgk_gb_row_gradient(s_x + tid * S, s_g + tid * S, s_scale + BGK_TILE_THREADS + tid * a.ext, atoms, a.sv);
        }
        __syncthreads();
        for (int i = tid; i < rows * nd; i += BGK_TILE_THREADS) {    /* tile_store, scaled by the row's g / (unit_energy T) */
            const int r = (int)__umulhi((unsigned)i, a.magic), c = i - r * nd;
            const float sc = s_scale[r];
            a.g_x[b0 * nd + i] = sc == 0.0f ? 0.0f : s_g[r * S + c] * sc;
        }
        __syncthreads();
    }
}

/* checks the envelope and fills the record: 0, BGK_EINVAL or BGK_EUNSUPPORTED */
int molecule_common(const char* what, const float* x, int64_t B, int32_t n_atoms, int32_t n_bonds, int32_t n_angles, int32_t n_torsions,
                    int32_t n_pairs, const int32_t* tables, double unit_energy, double temperature, MolArgs* a, const int4** terms,
                    const float** pairs) {
    BGK_CHECK_ARG(B >= 0 && temperature > 0.0 && unit_energy > 0.0, "%s: bad batch size / temperature / unit energy", what);
    BGK_CHECK_ARG(n_atoms >= 1 && n_bonds >= 0 && n_angles >= 0 && n_torsions >= 0, "%s: negative table size", what);
    if (!(n_atoms >= 2 && n_atoms <= BGK_MOLECULE_MAX_ATOMS && n_bonds <= BGK_MOLECULE_MAX_BONDS && n_angles <= BGK_MOLECULE_MAX_ANGLES &&
          n_torsions <= BGK_MOLECULE_MAX_TORSIONS)) {
        bgk_set_error("%s: %d atoms, %d bonds, %d angles, %d torsion terms are outside the kernel's envelope (2..%d atoms, %d / %d / %d terms)",
                      what, n_atoms, n_bonds, n_angles, n_torsions, BGK_MOLECULE_MAX_ATOMS, BGK_MOLECULE_MAX_BONDS, BGK_MOLECULE_MAX_ANGLES,
                      BGK_MOLECULE_MAX_TORSIONS);
        return BGK_EUNSUPPORTED;
    }
    BGK_CHECK_ARG(n_pairs == 0 || n_pairs == n_atoms * (n_atoms - 1) / 2, "%s: n_pairs must be 0 or n_atoms (n_atoms - 1) / 2", what);
    BGK_CHECK_ARG(B == 0 || (x && tables && (uintptr_t)tables % 16 == 0), "%s: null tensor / tables not aligned to 16 bytes", what);
    a->x = x; a->B = B;
    a->m = BgkMolecule{n_atoms, n_bonds, n_angles, n_torsions, n_pairs};
    a->nd = 3 * n_atoms; a->magic = tile_magic(a->nd);
    a->inv = (float)(1.0 / (unit_energy * temperature));
    *terms = reinterpret_cast<const int4*>(tables);
    *pairs = reinterpret_cast<const float*>(tables + 4 * (n_bonds + n_angles + n_torsions));
    return 0;
}

/* the solvent table and prefactor of the bgk_molecule_solvent_* entries */
struct SolventSpec { const float* table; double prefactor; };

/* checks the solvent arguments and fills the record's solvent part */
int molecule_solvent(const char* what, const SolventSpec& sol, int64_t B, MolArgs* a, const float4** atoms) {
    BGK_CHECK_ARG(B == 0 || (sol.table && (uintptr_t)sol.table % 16 == 0), "%s: null solvent table / not aligned to 16 bytes", what);
    BGK_CHECK_ARG(std::isfinite(sol.prefactor), "%s: the solvent prefactor is not finite", what);
    a->sv = BgkSolvent{a->m.n, (float)sol.prefactor};
    *atoms = reinterpret_cast<const float4*>(sol.table);
    return 0;
}

/* the most rows of a tile (64, 32 or 16) whose LDS stays within the limit: rows x words_per_row + fixed_words floats */
int molecule_rows(int words_per_row, int fixed_words) {
    int rows = BGK_TILE_THREADS;
    while (rows > 16 && (rows * words_per_row + fixed_words) * (int)sizeof(float) > MM_LDS_LIMIT) rows /= 2;
    return rows;
}

/* loss_sums != NULL: also the KL loss sums, over dlogp, through the [nblk, 2] f64 workspace `partial`; sol != NULL: with the solvent terms */
int molecule_forward(const char* what, const float* x, int64_t B, int32_t n_atoms, int32_t n_bonds, int32_t n_angles, int32_t n_torsions,
                     int32_t n_pairs, const int32_t* tables, double unit_energy, double temperature, float* u, const float* dlogp,
                     int32_t drop_nonfinite, double* partial, int32_t nblk, double* loss_sums, void* stream, const SolventSpec* sol = nullptr) {
    MolArgs a{};
    const int4* terms; const float* pairs; const float4* atoms = nullptr;
    int st = molecule_common(what, x, B, n_atoms, n_bonds, n_angles, n_torsions, n_pairs, tables, unit_energy, temperature, &a, &terms, &pairs);
    if (st) return st;
    if (sol && (st = molecule_solvent(what, *sol, B, &a, &atoms))) return st;
    BGK_CHECK_ARG(!loss_sums || (dlogp && partial && nblk >= 1), "%s: the loss sums need dlogp and a [nblk, 2] f64 workspace", what);
    hipStream_t s = (hipStream_t)stream;
    if (B == 0) {               /* an empty batch: the loss sums are zero */
        if (loss_sums) { hipError_t e = hipMemsetAsync(loss_sums, 0, 2 * sizeof(double), s); if (e != hipSuccess) return (int)e; }
        return 0;
    }
    BGK_CHECK_ARG(u, "%s: null output", what);
    a.ext = sol ? (n_atoms | 1) : 0;                    /* the Born radii of a lane, at an odd stride */
    a.rows = sol ? molecule_rows((a.nd | 1) + a.ext, 0) : BGK_TILE_THREADS;
    a.u = u; a.drop_nonfinite = drop_nonfinite;
    if (loss_sums) { a.dlogp = dlogp; a.partial = partial; }
    const size_t lds = (size_t)a.rows * ((a.nd | 1) + a.ext) * sizeof(float);
    int grid = tile_grid(B, a.rows);
    if (loss_sums && grid > nblk) grid = nblk;
    if (sol) hipLaunchKernelGGL(molecule_energy_kernel<true>, dim3(grid), dim3(BGK_TILE_THREADS), lds, s, a, terms, pairs, atoms);
    else hipLaunchKernelGGL(molecule_energy_kernel<false>, dim3(grid), dim3(BGK_TILE_THREADS), lds, s, a, terms, pairs, atoms);
    const int st2 = bgk_launch_status(what);
    if (st2 || !loss_sums) return st2;
    hipLaunchKernelGGL(molecule_loss_merge_kernel, dim3(1), dim3(BGK_WAVE), 0, s, partial, grid, loss_sums);
    return bgk_launch_status(what);
}

int molecule_backward(const char* what, const float* x, int64_t B, int32_t n_atoms, int32_t n_bonds, int32_t n_angles, int32_t n_torsions,
                      int32_t n_pairs, const int32_t* tables, double unit_energy, double temperature, const float* g_u, const float* g_scalar,
                      const float* u, const float* dlogp, int32_t drop_nonfinite, float* g_dlogp, float* g_x, void* stream,
                      const SolventSpec* sol = nullptr) {
    MolArgs a{};
    const int4* terms; const float* pairs; const float4* atoms = nullptr;
    int st = molecule_common(what, x, B, n_atoms, n_bonds, n_angles, n_torsions, n_pairs, tables, unit_energy, temperature, &a, &terms, &pairs);
    if (st) return st;
    if (sol && (st = molecule_solvent(what, *sol, B, &a, &atoms))) return st;
    BGK_CHECK_ARG(g_u || (g_scalar && u && dlogp), "%s: need g_u [B] or (g_scalar, u, dlogp)", what);
    if (B == 0) return 0;
    BGK_CHECK_ARG(g_x, "%s: null output", what);
    const int S = a.nd | 1;
    a.ext = sol ? (a.nd | 1) : 0;                       /* B_i, d E / d B_i and the chain factors of a lane, at an odd stride */
    a.rows = molecule_rows(2 * S + a.ext, BGK_TILE_THREADS);                                        /* x tile, gradient tile, row scales */
    a.u = const_cast<float*>(u); a.dlogp = dlogp; a.drop_nonfinite = drop_nonfinite;
    a.g_u = g_u; a.g_scalar = g_scalar; a.g_dlogp = g_dlogp; a.g_x = g_x;
    const size_t lds = ((size_t)a.rows * (2 * S + a.ext) + BGK_TILE_THREADS) * sizeof(float);
    const dim3 grid(tile_grid(B, a.rows));
    if (sol) hipLaunchKernelGGL(molecule_energy_bwd_kernel<true>, grid, dim3(BGK_TILE_THREADS), lds, (hipStream_t)stream, a, terms, pairs, atoms);
    else hipLaunchKernelGGL(molecule_energy_bwd_kernel<false>, grid, dim3(BGK_TILE_THREADS), lds, (hipStream_t)stream, a, terms, pairs, atoms);
    return bgk_launch_status(what);
}

}  // namespace

extern "C" int bgk_molecule_energy(const float* x, int64_t B, int32_t n_atoms, int32_t n_bonds, int32_t n_angles, int32_t n_torsions,
                                   int32_t n_pairs, const int32_t* tables, double unit_energy, double temperature, float* u, void* stream) {
    return molecule_forward("bgk_molecule_energy", x, B, n_atoms, n_bonds, n_angles, n_torsions, n_pairs, tables, unit_energy, temperature, u,
                            nullptr, 0, nullptr, 0, nullptr, stream);
}

extern "C" int bgk_molecule_energy_kl_sums(const float* x, int64_t B, int32_t n_atoms, int32_t n_bonds, int32_t n_angles, int32_t n_torsions,
                                           int32_t n_pairs, const int32_t* tables, double unit_energy, double temperature, float* u,
                                           const float* dlogp, int32_t drop_nonfinite, double* partial, int32_t nblk, double* loss_sums,
                                           void* stream) {
    BGK_CHECK_ARG(loss_sums, "bgk_molecule_energy_kl_sums: loss_sums is NULL");
    return molecule_forward("bgk_molecule_energy_kl_sums", x, B, n_atoms, n_bonds, n_angles, n_torsions, n_pairs, tables, unit_energy,
                            temperature, u, dlogp, drop_nonfinite, partial, nblk, loss_sums, stream);
}

extern "C" int bgk_molecule_energy_backward(const float* x, int64_t B, int32_t n_atoms, int32_t n_bonds, int32_t n_angles, int32_t n_torsions,
                                            int32_t n_pairs, const int32_t* tables, double unit_energy, double temperature, const float* g_u,
                                            const float* g_scalar, const float* u, const float* dlogp, int32_t drop_nonfinite,
                                            float* g_dlogp, float* g_x, void* stream) {
    return molecule_backward("bgk_molecule_energy_backward", x, B, n_atoms, n_bonds, n_angles, n_torsions, n_pairs, tables, unit_energy,
                             temperature, g_u, g_scalar, u, dlogp, drop_nonfinite, g_dlogp, g_x, stream);
}

extern "C" int bgk_molecule_solvent_energy(const float* x, int64_t B, int32_t n_atoms, int32_t n_bonds, int32_t n_angles, int32_t n_torsions,
                                           int32_t n_pairs, const int32_t* tables, double unit_energy, double temperature,
                                           const float* solvent, double gb_prefactor, float* u, void* stream) {
    const SolventSpec sol{solvent, gb_prefactor};
    return molecule_forward("bgk_molecule_solvent_energy", x, B, n_atoms, n_bonds, n_angles, n_torsions, n_pairs, tables, unit_energy,
                            temperature, u, nullptr, 0, nullptr, 0, nullptr, stream, &sol);
}

extern "C" int bgk_molecule_solvent_energy_kl_sums(const float* x, int64_t B, int32_t n_atoms, int32_t n_bonds, int32_t n_angles,
                                                   int32_t n_torsions, int32_t n_pairs, const int32_t* tables, double unit_energy,
                                                   double temperature, const float* solvent, double gb_prefactor, float* u,
                                                   const float* dlogp, int32_t drop_nonfinite, double* partial, int32_t nblk,
                                                   double* loss_sums, void* stream) {
    BGK_CHECK_ARG(loss_sums, "bgk_molecule_solvent_energy_kl_sums: loss_sums is NULL");
    const SolventSpec sol{solvent, gb_prefactor};
    return molecule_forward("bgk_molecule_solvent_energy_kl_sums", x, B, n_atoms, n_bonds, n_angles, n_torsions, n_pairs, tables, unit_energy,
                            temperature, u, dlogp, drop_nonfinite, partial, nblk, loss_sums, stream, &sol);
}

extern "C" int bgk_molecule_solvent_energy_backward(const float* x, int64_t B, int32_t n_atoms, int32_t n_bonds, int32_t n_angles,
                                                    int32_t n_torsions, int32_t n_pairs, const int32_t* tables, double unit_energy,
                                                    double temperature, const float* solvent, double gb_prefactor, const float* g_u,
                                                    const float* g_scalar, const float* u, const float* dlogp, int32_t drop_nonfinite,
                                                    float* g_dlogp, float* g_x, void* stream) {
    const SolventSpec sol{solvent, gb_prefactor};
    return molecule_backward("bgk_molecule_solvent_energy_backward", x, B, n_atoms, n_bonds, n_angles, n_torsions, n_pairs, tables,
                             unit_energy, temperature, g_u, g_scalar, u, dlogp, drop_nonfinite, g_dlogp, g_x, stream, &sol);
}
