/* bgk_colmap.hip -- column maps of one [B, n] field in one launch: every output column is an elementwise function of at most one
 * input column, or a constant.  Covers what the builder's constraint layers append (bgflow/factory/generator_builder.py:461-526):
 *   SetConstantFlow + index MergeFlow (nn/flow/base.py / coupling.py:13-110, 227-272: `repeat`, `empty`, one `index_copy_` per part)
 *   TorchTransform(AffineTransform) (nn/flow/torchtransform.py:25-33), CircularShiftFlow and IncreaseMultiplicityFlow
 *   (nn/flow/modulo.py:24-76), in both directions, and -- with another table -- their backward.
 * Table: n_out entries (kind, src, p0, p1), wave-uniform, read through the constant address space (scalar loads; the kind is a
 * scalar branch).  Every kind is one or two correctly rounded IEEE operations or an exact fmod, in the order torch evaluates them
 * (the unit is compiled without fma contraction and with correctly rounded division), so the results are the reference's bits.
 * Layout: field rows are short and mostly odd, so a lane per row would read and write uncoalesced.  A wave stages its [64][n_in]
 * tile through LDS (the tile is the memory image of contiguous rows: coalesced loads), lane = row works on LDS with a row stride
 * made odd (conflict-free banks), and the [64][n_out] tile leaves the same way.
 * Sheaf draw of MULT_FWD: Philox4x32-10 with the counter layout of bgk_philox.hip -- (row low, row high, field 0 << 20 | 4-column
 * block, call offset), key = seed -- a pure function of (seed, call, GLOBAL row, column); u = u01 of bgk_philox.h, below 1. */
#include "bgk_common.h"
#include "bgk_philox.h"

namespace {

constexpr int CM_COPY = 0, CM_CONST = 1, CM_AFFINE_FWD = 2, CM_AFFINE_INV = 3, CM_SHIFT = 4, CM_MULT_INV = 5, CM_MULT_FWD = 6;
constexpr int CM_LDS_BYTES = 160 * 1024;

struct CEntry { int32_t kind, src; float p0, p1; };                      /* one output column: s_load_dwordx4 */
typedef const __attribute__((address_space(4))) CEntry* ctab_t;

struct CArgs {
    const float* in; float* out; const CEntry* tab; const float* u; float* dlogp; int32_t* bad;
    int64_t B, row0;
    int n_in, n_out, ldi, ldo;        /* ldi / ldo: LDS row strides (the widths made odd) */
    int logdet_mode;                  /* 0: dlogp untouched, 1: dlogp[b] = c, 2: dlogp[b] += c */
    float logdet;
    uint32_t seed_lo, seed_hi, offset;
};

/* torch's remainder for a positive divisor: fmod, then + b if the result is non-zero and negative */
__device__ __forceinline__ float remainder_pos(float a, float b) {
    float m = fmodf(a, b);
    if (m != 0.0f && m < 0.0f) m += b;
    return m;
}
/* the unit-interval test of modulo.py:42-44 on f32 operands */
__device__ __forceinline__ int outside_unit(float x) { return (x > 1.000001f || x < -1e-6f) ? 1 : 0; }

/* copy `rows` contiguous global rows of width n between global memory and an LDS tile of row stride ld (lane-contiguous on the
 * global side); (r, c) of a lane's element advance incrementally: one division per lane */
template <bool TO_LDS>
__device__ __forceinline__ void tile_copy(float* __restrict__ lds, float* __restrict__ glob, int rows, int n, int ld, int lane) {
    const int total = rows * n;
    if (ld == n) {
        for (int q = lane; q < total; q += 64) { if (TO_LDS) lds[q] = glob[q]; else glob[q] = lds[q]; }
        return;
    }
    int r = lane / n, c = lane - r * n;
    const int dr = 64 / n, dc = 64 - dr * n;
    for (int q = lane; q < total; q += 64) {
        if (TO_LDS) lds[r * ld + c] = glob[q]; else glob[q] = lds[r * ld + c];
        r += dr; c += dc;
        if (c >= n) { c -= n; ++r; }
    }
}

__global__ __launch_bounds__(256) void colmap_kernel(CArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63, pw = (int)blockDim.x >> 6;
    const int64_t tile = (int64_t)blockIdx.x * pw + wave;
    if (tile >= ((a.B + 63) >> 6)) return;
    float* s_in = smem + (size_t)wave * 64 * (a.ldi + a.ldo);
    float* s_out = s_in + 64 * a.ldi;
    const int64_t b0 = tile * 64;
    const int rows = (int)((a.B - b0) < 64 ? (a.B - b0) : 64);
    tile_copy<true>(s_in, const_cast<float*>(a.in) + b0 * a.n_in, rows, a.n_in, a.ldi, lane);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (lane < rows) {
        const ctab_t tab = (ctab_t)a.tab;
        const float* x_row = s_in + lane * a.ldi;
        float* y_row = s_out + lane * a.ldo;
        const uint64_t grow = (uint64_t)(a.row0 + b0 + lane);
        uint32_t o[4] = {0u, 0u, 0u, 0u};
        int have_cb = -1, bad = 0;
        for (int j = 0; j < a.n_out; ++j) {
            const int kind = tab[j].kind, src = tab[j].src;
            const float p0 = tab[j].p0, p1 = tab[j].p1;
            float y;
            if (kind == CM_CONST) {
                y = p0;
            } else {
                const float x = x_row[src];
                if (kind == CM_COPY) {
                    y = x;
                } else if (kind == CM_AFFINE_FWD) {
                    const float t = p1 * x;
                    y = p0 + t;
                } else if (kind == CM_AFFINE_INV) {
                    y = (x - p0) / p1;
                } else if (kind == CM_SHIFT) {
                    bad += outside_unit(x);
                    y = remainder_pos(x + p0, 1.0f);
                } else if (kind == CM_MULT_INV) {
                    bad += outside_unit(x);
                    y = remainder_pos(x, p1) * p0;
                } else {                                    /* CM_MULT_FWD */
                    bad += outside_unit(x);
                    float uu;
                    if (a.u) {
                        uu = a.u[(b0 + lane) * a.n_in + src];
                    } else {
                        if ((src >> 2) != have_cb) {
                            have_cb = src >> 2;
                            philox4x32_10((uint32_t)grow, (uint32_t)(grow >> 32), (uint32_t)have_cb, a.offset, a.seed_lo, a.seed_hi, o);
                        }
                        const int w = src & 3;
                        uu = u01(w == 0 ? o[0] : w == 1 ? o[1] : w == 2 ? o[2] : o[3]);
                    }
                    /* u01 is at most 1 - 2^-24 (unclamped, the 256 largest words, probability 2^-24, would round to 1.0), but the
                     * f32 product u * m can still round up to m, and handed-in uniforms are the caller's: keep the sheaf below m */
                    float sheaf = floorf(uu * p0);
                    sheaf = sheaf > p0 - 1.0f ? p0 - 1.0f : sheaf;
                    y = (x + sheaf) / p0;
                }
            }
            y_row[j] = y;
        }
        if (a.logdet_mode == 1) a.dlogp[b0 + lane] = a.logdet;
        else if (a.logdet_mode == 2) a.dlogp[b0 + lane] += a.logdet;
        if (bad && a.bad) atomicAdd(a.bad, bad);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    tile_copy<false>(s_out, a.out + b0 * a.n_out, rows, a.n_out, a.ldo, lane);
}

}  // namespace

extern "C" int bgk_colmap(const float* in, int32_t n_in, float* out, int32_t n_out, const void* table, const float* u,
                          uint64_t seed, uint32_t offset, int64_t row0, int64_t B,
                          float* dlogp, int32_t accumulate, double logdet, int32_t* bad_count, void* stream) {
    BGK_CHECK_ARG(B >= 0 && row0 >= 0, "bgk_colmap: bad batch");
    if (B == 0) return 0;
    BGK_CHECK_ARG(in && out && table && n_in >= 1 && n_out >= 1 && n_in <= BGK_COLMAP_MAX_WIDTH && n_out <= BGK_COLMAP_MAX_WIDTH,
                  "bgk_colmap: widths %d -> %d outside [1, %d]", n_in, n_out, BGK_COLMAP_MAX_WIDTH);
    CArgs a{};
    a.in = in; a.out = out; a.tab = (const CEntry*)table; a.u = u; a.dlogp = dlogp; a.bad = bad_count;
    a.B = B; a.row0 = row0; a.n_in = n_in; a.n_out = n_out; a.ldi = n_in | 1; a.ldo = n_out | 1;
    /* accumulate: a zero log-det leaves the running buffer alone; otherwise the launch is the buffer's first writer */
    a.logdet = (float)logdet;
    a.logdet_mode = !dlogp ? 0 : (!accumulate ? 1 : (a.logdet != 0.0f ? 2 : 0));
    a.seed_lo = (uint32_t)seed; a.seed_hi = (uint32_t)(seed >> 32); a.offset = offset;
    const size_t per_wave = sizeof(float) * 64 * (size_t)(a.ldi + a.ldo);
    /* four waves per workgroup while their tiles fit 64 KiB (two or more workgroups per CU), else one wave per workgroup */
    const int pw = 4 * per_wave <= (size_t)64 * 1024 ? 4 : 1;
    const size_t shmem = per_wave * pw;
    BGK_CHECK_ARG(shmem <= (size_t)CM_LDS_BYTES, "bgk_colmap: tiles of %d + %d columns do not fit the LDS", n_in, n_out);
    if (shmem > 64 * 1024) (void)hipFuncSetAttribute(reinterpret_cast<const void*>(colmap_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, CM_LDS_BYTES);
    const int64_t n_wg = (((B + 63) >> 6) + pw - 1) / pw;
    BGK_CHECK_ARG(n_wg < (int64_t)0x7fffffff, "bgk_colmap: batch too large for one launch");
    hipLaunchKernelGGL(colmap_kernel, dim3((unsigned)n_wg), dim3(pw * 64), shmem, (hipStream_t)stream, a);
    return bgk_launch_status("bgk_colmap");
}
