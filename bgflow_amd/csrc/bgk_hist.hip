/* bgk_hist.hip -- bootstrap histograms: the resampling loop of free_energy_bootstrap (distribution/sampling/_mcmc/analysis.py:105-123:
 * per replicate np.random.choice, two gathers and a weighted np.histogram on the host) as two stages behind one entry,
 *
 *     out[s, b] = sum over the draws j of replicate s of  w[i(s, j)]  where  bin(d[i(s, j)]) == b.
 *
 * Roofline: S replicates of n draws are S n random reads of one 8-byte (f32) or 16-byte (f64) record and S n / 2 Philox calls
 * (~100 integer ops each); the records (8 MiB at n = 2^20) stay in L2 / the Infinity Cache, so HBM bytes and flops are not the limit.
 * Measured (DESIGN.md "Bootstrap histogram"): 1.2e11 records/s at n = 2^20, half of that at 2^24; samples spread evenly over the bins
 * run at most 4 % faster, so lanes adding onto one bin are not the limit; gather latency and the LDS add rate are not separated.
 *
 * Stage 1 (hist_digitize_kernel, once per call): sample i -> record {bin, weight}.  The bin is np.histogram(x, bins=edges)'s on the f64
 * edges: x is widened to f64, the guess (x - e[0]) nb / (e[nb] - e[0]) is checked against e[idx] <= x < e[idx + 1] in f64 and, where it
 * fails (rounding at an edge, or edges that are not equidistant), replaced by a bisection over the edges (at most 12 steps); bins are
 * half-open, the last one is closed at e[nb]; values outside [e[0], e[nb]], NaN and +-inf get bin -1 (counted in n_ignored[0]).  The
 * weight is w[i] or 1; a sample inside the range whose weight is NaN, infinite or negative gets bin -1 too (counted in n_ignored[1];
 * numpy would carry a NaN weight into every later bin through its cumulative sum -- a documented deviation).  The two counts are
 * integer adds, one per block and counter.
 * Stage 2 (hist_resample_kernel, grid n_replicates x n_chunks): block (s, c) takes the draws j of chunk c (an even number of draws per
 * chunk, fixed by the replicate's draw count and n_chunks) of replicate replicate0 + s.  Source of draw j:
 *     indices[s, j]                          (an index outside [0, n) is skipped)
 *     segments[s] + j, j < segments[s + 1] - segments[s]      (the plain histogram of a segment; the segment is clipped to [0, n))
 *     mulhi64(r, n), r = 64 bits of Philox4x32-10 (bgk_philox.h) at counter (k low, k high, replicate, offset), k = j / 2, key = seed:
 *         words (o0, o1) = (low, high) for the even draw of a call, (o2, o3) for the odd one.
 * The draws of a replicate depend on (seed, offset, absolute replicate number, n) alone: not on n_chunks, the grid or the split of the
 * replicates over calls.  The 64-bit multiply-high keeps the non-uniformity of an index below n / 2^64.  A thread keeps HIST_UNROLL
 * calls = 2 HIST_UNROLL records in flight.  Each wave adds into its own f64 histogram in LDS (one copy per wave up to 1024 bins, one
 * shared copy beyond) with atomicAdd(double*) -- one ds_add_f64 on gfx950, no compare-and-swap loop --, the copies are summed in wave
 * order into partial[s, c, :].  hist_merge_kernel sums the chunks in ascending order into out[s, :].  No global float atomics, nothing
 * waits on another block: the order between the stages is stream order.
 *
 * Reproducibility: unweighted sums are sums of 1.0 in f64, exact and bitwise reproducible in any order.  Weighted sums depend on the
 * arrival order of the LDS adds in their last bits: |sum - exact| <= m 2^-52 exact for a bin that received m draws (any order of m
 * positive f64 terms is within (m - 1) 2^-53; the factor 2 covers the wave and chunk merges and the second-order term). */
#include "bgk_reduce.h"
#include "bgk_philox.h"

namespace {

constexpr int HIST_THREADS = 256;
constexpr int HIST_WAVES = HIST_THREADS / BGK_WAVE;
constexpr int HIST_MAX_BINS = 4096;
constexpr int HIST_MAX_CHUNKS = 512;
constexpr int HIST_COPY_BINS = 1024;        /* up to this many bins every wave has its own histogram (4 x 1024 x 8 B = 32 KiB) */
constexpr int HIST_UNROLL = 4;              /* Philox calls (pairs of draws) a thread keeps in flight */
constexpr int HIST_DIGITIZE_BLOCKS = 2048;

template <typename T> struct Rec;
template <> struct Rec<float> { int32_t bin; float w; };
template <> struct Rec<double> { int64_t bin; double w; };
static_assert(sizeof(Rec<float>) == 8 && sizeof(Rec<double>) == 16, "record layout");

/* the launch-argument record of stage 2 and the merge */
struct HistArgs {
    const void* records;
    const int64_t* indices;
    const int64_t* segments;
    double* partial;
    double* out;
    int64_t n, n_replicates, replicate0;
    uint32_t seed_lo, seed_hi, offset;
    int32_t nb, n_chunks, copies;
};

__device__ __forceinline__ int hist_bin(double x, const double* __restrict__ e, int nb, double e0, double en, double scale) {
    if (!(x >= e0 && x <= en)) return -1;               /* outside, NaN, +-inf */
    const double t = (x - e0) * scale;
    int idx = t >= 0.0 ? (t < (double)nb ? (int)t : nb - 1) : 0;      /* (a NaN guess: 0) */
    if (x >= e[idx] && (x < e[idx + 1] || idx == nb - 1)) return idx;
    int lo = 0, hi = nb;                                 /* largest idx in [0, nb) with e[idx] <= x; x == e[nb] -> nb - 1 */
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (x >= e[mid]) lo = mid; else hi = mid;
    }
    return lo;
}

template <typename T>
__global__ __launch_bounds__(HIST_THREADS) void hist_digitize_kernel(const T* __restrict__ d, const T* __restrict__ w, int64_t n,
                                                                      const double* __restrict__ edges, int nb,
                                                                      Rec<T>* __restrict__ records,
                                                                      unsigned long long* __restrict__ n_ignored) {
    __shared__ unsigned int s_cnt[2];
    if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0u;
    __syncthreads();
    const double e0 = edges[0], en = edges[nb];
    const double scale = (double)nb / (en - e0);
    unsigned int bad_value = 0u, bad_weight = 0u;
    for (int64_t i = (int64_t)blockIdx.x * HIST_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * HIST_THREADS) {
        int bin = hist_bin((double)d[i], edges, nb, e0, en, scale);
        T wt = w ? w[i] : (T)1;
        if (bin < 0) {
            ++bad_value;
        } else if (!(wt >= (T)0 && wt < (T)__builtin_huge_val())) {      /* NaN, +-inf, negative */
            ++bad_weight;
            bin = -1;
        }
        Rec<T> r;
        r.bin = bin;
        r.w = bin < 0 ? (T)0 : wt;
        records[i] = r;
    }
    if (bad_value) atomicAdd(&s_cnt[0], bad_value);
    if (bad_weight) atomicAdd(&s_cnt[1], bad_weight);
    __syncthreads();
    if (n_ignored && threadIdx.x < 2 && s_cnt[threadIdx.x]) atomicAdd(&n_ignored[threadIdx.x], (unsigned long long)s_cnt[threadIdx.x]);
}

template <typename T>
__device__ __forceinline__ void hist_add(double* h, const Rec<T>& r) {
    if (r.bin >= 0) atomicAdd(&h[r.bin], (double)r.w);
}

template <typename T>
__global__ __launch_bounds__(HIST_THREADS) void hist_resample_kernel(HistArgs a) {
    extern __shared__ double s_hist[];                  /* [copies][nb] */
    const int t = threadIdx.x;
    const int nb = a.nb;
    for (int b = t; b < a.copies * nb; b += HIST_THREADS) s_hist[b] = 0.0;
    __syncthreads();
    const int64_t s = (int64_t)blockIdx.x / a.n_chunks;
    const int c = (int)((int64_t)blockIdx.x - s * a.n_chunks);
    double* h = s_hist + (a.copies > 1 ? (t / BGK_WAVE) * nb : 0);
    const Rec<T>* __restrict__ rec = reinterpret_cast<const Rec<T>*>(a.records);
    const int64_t n = a.n;
    /* the replicate's draws and this chunk's share: an even number per chunk */
    int64_t start = 0, m = n;
    if (a.segments) {
        int64_t s0 = a.segments[s], s1 = a.segments[s + 1];
        s0 = s0 < 0 ? 0 : (s0 > n ? n : s0);
        s1 = s1 < s0 ? s0 : (s1 > n ? n : s1);
        start = s0; m = s1 - s0;
    }
    int64_t per = (m + a.n_chunks - 1) / a.n_chunks;
    per += per & 1;
    const int64_t j0 = (int64_t)c * per < m ? (int64_t)c * per : m;
    const int64_t j1 = j0 + per < m ? j0 + per : m;
    if (a.indices || a.segments) {
        const int64_t* __restrict__ idx = a.indices ? a.indices + s * n : nullptr;
        for (int64_t j = j0 + t; j < j1; j += (int64_t)HIST_THREADS * 2 * HIST_UNROLL) {
            Rec<T> r[2 * HIST_UNROLL];
#pragma unroll
            for (int u = 0; u < 2 * HIST_UNROLL; ++u) {
                const int64_t jj = j + (int64_t)u * HIST_THREADS;
                r[u].bin = -1; r[u].w = (T)0;
                if (jj < j1) {
                    const int64_t i = idx ? idx[jj] : start + jj;
                    if ((uint64_t)i < (uint64_t)n) r[u] = rec[i];
                }
            }
#pragma unroll
            for (int u = 0; u < 2 * HIST_UNROLL; ++u) hist_add<T>(h, r[u]);
        }
    } else {
        const uint32_t replicate = (uint32_t)(uint64_t)(a.replicate0 + s);
        const int64_t k0 = j0 >> 1, k1 = j0 < j1 ? (j1 + 1) >> 1 : k0;      /* a chunk with draws starts at an even j0: calls k0 .. k1 - 1 */
        for (int64_t k = k0 + t; k < k1; k += (int64_t)HIST_THREADS * HIST_UNROLL) {
            Rec<T> r[2 * HIST_UNROLL];
#pragma unroll
            for (int u = 0; u < HIST_UNROLL; ++u) {
                const int64_t kk = k + (int64_t)u * HIST_THREADS;
                r[2 * u].bin = -1; r[2 * u].w = (T)0;
                r[2 * u + 1].bin = -1; r[2 * u + 1].w = (T)0;
                if (kk < k1) {
                    uint32_t o[4];
                    philox4x32_10((uint32_t)(uint64_t)kk, (uint32_t)((uint64_t)kk >> 32), replicate, a.offset, a.seed_lo, a.seed_hi, o);
                    const uint64_t i_even = __umul64hi(((uint64_t)o[1] << 32) | o[0], (uint64_t)n);
                    const uint64_t i_odd = __umul64hi(((uint64_t)o[3] << 32) | o[2], (uint64_t)n);
                    r[2 * u] = rec[i_even];                      /* mulhi64(r, n) < n */
                    if (2 * kk + 1 < j1) r[2 * u + 1] = rec[i_odd];
                }
            }
#pragma unroll
            for (int u = 0; u < 2 * HIST_UNROLL; ++u) hist_add<T>(h, r[u]);
        }
    }
    __syncthreads();
    double* dst = a.partial + (int64_t)blockIdx.x * nb;
    for (int b = t; b < nb; b += HIST_THREADS) {
        double v = s_hist[b];
        for (int q = 1; q < a.copies; ++q) v += s_hist[q * nb + b];
        dst[b] = v;
    }
}

__global__ __launch_bounds__(HIST_THREADS) void hist_merge_kernel(HistArgs a) {
    const int64_t total = a.n_replicates * a.nb;
    for (int64_t e = (int64_t)blockIdx.x * HIST_THREADS + threadIdx.x; e < total; e += (int64_t)gridDim.x * HIST_THREADS) {
        const int64_t s = e / a.nb;
        const int b = (int)(e - s * a.nb);
        const double* src = a.partial + s * a.n_chunks * a.nb + b;
        double v = src[0];
        for (int c = 1; c < a.n_chunks; ++c) v += src[(int64_t)c * a.nb];
        a.out[e] = v;
    }
}

template <typename T>
void hist_enqueue(const void* d, const void* w, const double* edges, void* records, int64_t* n_ignored, const HistArgs& a, hipStream_t st) {
    const int64_t want = (a.n + HIST_THREADS - 1) / HIST_THREADS;
    const int dblocks = (int)(want < HIST_DIGITIZE_BLOCKS ? want : HIST_DIGITIZE_BLOCKS);
    hipLaunchKernelGGL(hist_digitize_kernel<T>, dim3(dblocks), dim3(HIST_THREADS), 0, st, (const T*)d, (const T*)w, a.n, edges, a.nb,
                       (Rec<T>*)records, (unsigned long long*)n_ignored);
    const size_t lds = (size_t)a.copies * a.nb * sizeof(double);
    hipLaunchKernelGGL(hist_resample_kernel<T>, dim3((unsigned)(a.n_replicates * a.n_chunks)), dim3(HIST_THREADS), lds, st, a);
    const int64_t mwant = (a.n_replicates * a.nb + HIST_THREADS - 1) / HIST_THREADS;
    hipLaunchKernelGGL(hist_merge_kernel, dim3((unsigned)(mwant < 4096 ? mwant : 4096)), dim3(HIST_THREADS), 0, st, a);
}

}  // namespace

extern "C" int bgk_bootstrap_histogram(const void* d, const void* w, int64_t n, int32_t dtype, const double* edges, int32_t nb,
                                       int64_t n_replicates, int64_t replicate0, const int64_t* indices, const int64_t* segments,
                                       uint64_t seed, uint32_t offset, int32_t n_chunks, void* records, double* partial, double* out,
                                       int64_t* n_ignored, void* stream) {
    BGK_CHECK_ARG(d && edges && records && partial && out, "bgk_bootstrap_histogram: null pointer (d, edges, records, partial, out)");
    BGK_CHECK_ARG(n >= 1, "bgk_bootstrap_histogram: bad size (n = %lld, at least one sample)", (long long)n);
    BGK_CHECK_DTYPE("bgk_bootstrap_histogram", dtype);
    BGK_CHECK_ARG(nb >= 1, "bgk_bootstrap_histogram: nb = %d bins (at least 1)", (int)nb);
    if (nb > HIST_MAX_BINS) {
        bgk_set_error("bgk_bootstrap_histogram: nb = %d bins is outside the envelope (1 .. %d)", (int)nb, HIST_MAX_BINS);
        return BGK_EUNSUPPORTED;
    }
    BGK_CHECK_ARG(n_chunks >= 1 && n_chunks <= HIST_MAX_CHUNKS, "bgk_bootstrap_histogram: n_chunks must be in 1 .. %d", HIST_MAX_CHUNKS);
    BGK_CHECK_ARG(n_replicates >= 0 && replicate0 >= 0 && replicate0 <= ((int64_t)1 << 32) && n_replicates <= ((int64_t)1 << 32) - replicate0,
                  "bgk_bootstrap_histogram: replicates %lld .. +%lld: negative, or beyond 2^32 (the Philox counter word)",
                  (long long)replicate0, (long long)n_replicates);
    BGK_CHECK_ARG(n_replicates * (int64_t)n_chunks <= 0x7fffffffLL, "bgk_bootstrap_histogram: n_replicates * n_chunks exceeds the grid (2^31 - 1 blocks)");
    BGK_CHECK_ARG(!(indices && segments), "bgk_bootstrap_histogram: both indices and segments given");
    const uintptr_t elem = bgk_dtype_size(dtype);
    BGK_CHECK_ALIGNED("bgk_bootstrap_histogram", bgk_aligned(elem, d, w) && bgk_aligned(2 * elem, records) &&
                      bgk_aligned(8, edges, partial, out, indices, segments, n_ignored));
    if (n_replicates == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    if (n_ignored) {
        hipError_t e = hipMemsetAsync(n_ignored, 0, 2 * sizeof(int64_t), st);
        if (e != hipSuccess) {
            bgk_set_error("bgk_bootstrap_histogram: hipMemsetAsync: %s", hipGetErrorString(e));
            return (int)e;
        }
    }
    HistArgs a{};
    a.records = records; a.indices = indices; a.segments = segments; a.partial = partial; a.out = out;
    a.n = n; a.n_replicates = n_replicates; a.replicate0 = replicate0;
    a.seed_lo = (uint32_t)seed; a.seed_hi = (uint32_t)(seed >> 32); a.offset = offset;
    a.nb = nb; a.n_chunks = n_chunks; a.copies = nb <= HIST_COPY_BINS ? HIST_WAVES : 1;
    bgk_dtype_dispatch(dtype, [&](auto e) { hist_enqueue<decltype(e)>(d, w, edges, records, n_ignored, a, st); });
    return bgk_launch_status("bgk_bootstrap_histogram");
}
