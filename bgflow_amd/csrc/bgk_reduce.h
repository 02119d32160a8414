/* bgk_reduce.h -- what the two-stage reductions of bgk_bar.hip, bgk_mbar.hip, bgk_hist.hip and bgk_moments.hip share: the slice walk, the
 * lane merge, NaN-keeping selects, the solvers' record slots, the entry checks.  DESIGN.md "Shared plumbing of the free-energy kernels"
 * is the one description; what maps elements to threads, and the merge of the waves through LDS on thread 0, stay in the kernels. */
#ifndef BGK_REDUCE_H
#define BGK_REDUCE_H

#include "bgk_common.h"

/* ---- NaN-keeping maximum / minimum (torch.max / torch.min; fmax / fmin would drop it).  above(v, m): v replaces the running maximum m ---- */
template <typename T> __device__ __forceinline__ bool bgk_nan_above(T v, T m) { return v > m || v != v; }
template <typename T> __device__ __forceinline__ T bgk_nan_max(T m, T v) { return (v > m || v != v) ? v : m; }
template <typename T> __device__ __forceinline__ T bgk_nan_min(T m, T v) { return (v < m || v != v) ? v : m; }

/* ---- the 16-byte piece of an element type ---- */
template <typename T> struct BgkPiece;
template <> struct BgkPiece<float> { typedef float4 type; static constexpr int N = 4; };
template <> struct BgkPiece<double> { typedef double2 type; static constexpr int N = 2; };

/* f(element as double) for the piece's elements in memory order; r[0 .. N) = the same elements */
template <typename F> __device__ __forceinline__ void bgk_piece_each(const float4& v, F f) { f((double)v.x); f((double)v.y); f((double)v.z); f((double)v.w); }
template <typename F> __device__ __forceinline__ void bgk_piece_each(const double2& v, F f) { f(v.x); f(v.y); }
template <typename P> __device__ __forceinline__ void bgk_piece_unpack(const P& v, double* r) { bgk_piece_each(v, [&](double x) { *r++ = x; }); }

/* ---- a block's slice: block b takes [b per, (b + 1) per) clipped to n.  per is a multiple of 4 elements (16 bytes of f32, 32 of f64), so
 * every slice starts at the array's own phase of 16 bytes: a scalar head up to the first 16-byte boundary, 16-byte pieces, a scalar tail ---- */
static inline int64_t bgk_slice_per(int64_t n, int n_blocks) { return ((n + n_blocks - 1) / n_blocks + 3) / 4 * 4; }

template <typename T>
struct BgkSlice {
    const T* p;                                  /* the slice's first element */
    int64_t len;                                 /* its elements: p[0 .. len) */
    int64_t head;                                /* scalar elements p[0 .. head) before the first 16-byte boundary */
    int64_t body;                                /* len - head elements from p[head]: pieces pv[0 .. body / N), then body % N scalars */
    const typename BgkPiece<T>::type* pv;

    __device__ __forceinline__ BgkSlice(const T* base, int64_t n, int64_t per, int64_t block) {
        const int64_t i0 = block * per < n ? block * per : n;
        const int64_t i1 = (i0 + per) < n ? (i0 + per) : n;
        p = base + i0;
        len = i1 - i0;
        head = (int64_t)(((16u - (unsigned)((uintptr_t)p & 15u)) & 15u) / sizeof(T));
        head = head < len ? head : len;
        body = len - head;
        pv = reinterpret_cast<const typename BgkPiece<T>::type*>(p + head);
    }
};

/* ---- lanes 63 .. 1 onto lane 0, a <- merge(a, the lane `off` above) at offsets 32, 16, .., 1; bgk_shfl_down is overloaded per type ---- */
__device__ __forceinline__ double bgk_shfl_down(double v, int off) { return __shfl_down(v, off, BGK_WAVE); }

template <typename V, typename Merge>
__device__ __forceinline__ void bgk_wave_reduce(V& a, Merge merge) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) merge(a, bgk_shfl_down(a, off));
}

/* ---- the record of a two-stage solver (stage 1, then ONE workgroup that merges and advances it; both return at once when it is done;
 * the host reads it back once per chunk of steps, bgflow_amd/_driver.py): the slots and status codes every solver shares ---- */
enum { BGK_R_PHASE = 0, BGK_R_STATUS = 1 };
enum { BGK_ST_CONVERGED = 0, BGK_ST_BUDGET = 1, BGK_ST_NO_ROOT = 2, BGK_ST_NAN = 3 };

__device__ __forceinline__ int bgk_solver_phase(const double* record) { return (int)record[BGK_R_PHASE]; }
__device__ __forceinline__ void bgk_solver_finish(double* record, int status, int phase_done) { record[BGK_R_STATUS] = (double)status; record[BGK_R_PHASE] = (double)phase_done; }

/* ---- entry checks and dtype dispatch (host) ---- */
enum { BGK_F32 = 0, BGK_F64 = 1 };
static_assert(BGK_BAR_F32 == BGK_F32 && BGK_MBAR_F32 == BGK_F32 && BGK_HIST_F32 == BGK_F32 && BGK_BAR_F64 == BGK_F64 &&
              BGK_MBAR_F64 == BGK_F64 && BGK_HIST_F64 == BGK_F64, "one table of dtype codes");

#define BGK_CHECK_DTYPE(who, dtype) \
    BGK_CHECK_ARG((dtype) == BGK_F32 || (dtype) == BGK_F64, "%s: dtype code %d (0 = f32, 1 = f64)", who, (int)(dtype))
#define BGK_CHECK_ALIGNED(who, ok) BGK_CHECK_ARG(ok, "%s: a pointer is not aligned to its element size", who)

static inline uintptr_t bgk_dtype_size(int32_t dtype) { return dtype == BGK_F32 ? 4 : 8; }

template <typename... P>       /* every pointer is a multiple of size (a null pointer is) */
static inline bool bgk_aligned(uintptr_t size, P... p) { return (((uintptr_t)p % size == 0) && ...); }

/* f(float()) or f(double()): the argument's type is the element type */
template <typename F>
static inline void bgk_dtype_dispatch(int32_t dtype, F f) {
    if (dtype == BGK_F32) f(float());
    else f(double());
}

#endif /* BGK_REDUCE_H */
