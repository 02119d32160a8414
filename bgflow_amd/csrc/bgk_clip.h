/* bgk_clip.h -- device arithmetic of the robust-training wrappers (bgflow/utils/train.py:60-118), shared by bgk_clip.hip and the
 * energy kernels that fold the wrappers in (bgk_energy.hip).  Every function is the reference's f32 operation sequence:
 *   linlogcut     where(v >= high, high + log(1 + v - high), v), then clamp(max = max_val)            (train.py:60-62)
 *   clip_tensor   nan_to_num(g, nan = 0) (so +-inf -> +-FLT_MAX), groups of norm_dim consecutive elements, factor
 *                 min(clip / |group|_2, 1) with torch.minimum's NaN propagation                        (train.py:107-118) */
#ifndef BGK_CLIP_H
#define BGK_CLIP_H

#include "bgk_common.h"

constexpr float BGK_FLT_MAX = 3.402823466e+38f;

/* torch.nan_to_num(g, nan = 0.0): NaN -> 0, +-inf -> +-FLT_MAX */
__device__ __forceinline__ float bgk_clip_clean(float g) {
    if (g != g) return 0.0f;
    return g > BGK_FLT_MAX ? BGK_FLT_MAX : (g < -BGK_FLT_MAX ? -BGK_FLT_MAX : g);
}

/* min(clip / norm, 1) of a group whose sum of squares (of cleaned values, f32, ascending order) is ss: an overflowed sum gives the
 * factor 0 (clip / inf), a zero group the factor 1 (clip / 0 = inf); 0 / 0 stays NaN like torch.minimum(NaN, 1) */
__device__ __forceinline__ float bgk_clip_factor(float ss, float clip) {
    const float f = clip / __builtin_sqrtf(ss);
    return f < 1.0f ? f : (f != f ? f : 1.0f);
}

/* norm_dim = 1 (clipping by value): the norm of a group of one is |g| -- no square, so nothing overflows, and the reference maps
 * +-inf (cleaned to +-FLT_MAX) to +-clip.  For |g| > 2^64 the factor clip / |g| can be a denormal, which the division flushes to zero
 * on this target: there the quotient is formed against |g| 2^-64 and applied to g 2^-64 (both exact). */
__device__ __forceinline__ float bgk_clip_value(float g, float clip) {
    constexpr float P64 = 18446744073709551616.0f, M64 = 1.0f / P64;
    const float a = __builtin_fabsf(g);
    if (a > P64) {
        const float f = clip / (a * M64);
        return (g * M64) * (f < P64 ? f : (f != f ? f : P64));
    }
    const float f = clip / a;
    return g * (f < 1.0f ? f : (f != f ? f : 1.0f));
}

/* the group clip inside one float4 for norm_dim 1, 2 or 4 (groups never leave the lane) */
__device__ __forceinline__ float4 bgk_clip_quad(float4 g, int nd, float clip) {
    g.x = bgk_clip_clean(g.x); g.y = bgk_clip_clean(g.y); g.z = bgk_clip_clean(g.z); g.w = bgk_clip_clean(g.w);
    float fx, fy, fz, fw;
    if (nd == 1) return make_float4(bgk_clip_value(g.x, clip), bgk_clip_value(g.y, clip), bgk_clip_value(g.z, clip), bgk_clip_value(g.w, clip));
    if (nd == 2) {
        fx = fy = bgk_clip_factor(g.x * g.x + g.y * g.y, clip);
        fz = fw = bgk_clip_factor(g.z * g.z + g.w * g.w, clip);
    } else {
        fx = fy = fz = fw = bgk_clip_factor(((g.x * g.x + g.y * g.y) + g.z * g.z) + g.w * g.w, clip);
    }
    return make_float4(g.x * fx, g.y * fy, g.z * fz, g.w * fw);
}

/* log of t >= 1 (bgk_logf takes finite arguments: log(inf) = inf apart) */
__device__ __forceinline__ float bgk_cut_log(float t) { return t > BGK_FLT_MAX ? t : bgk_logf(t); }

__device__ __forceinline__ float bgk_linlogcut(float v, float high, float max_val) {
    const float c = v >= high ? high + bgk_cut_log((1.0f + v) - high) : v;
    return c > max_val ? max_val : c;            /* (NaN passes through, like clamp) */
}

/* d linlogcut / d v: 1 below `high`, 1 / (1 + v - high) above, 0 where the clamp is active (torch: clamp passes the gradient where
 * the value is <= max_val).  The cut value is recomputed with the forward's own operations, so both agree on the branch. */
__device__ __forceinline__ float bgk_linlogcut_grad(float v, float high, float max_val) {
    const float t = (1.0f + v) - high;
    const float c = v >= high ? high + bgk_cut_log(t) : v;
    if (c > max_val) return 0.0f;
    return v >= high ? 1.0f / t : 1.0f;
}

#endif /* BGK_CLIP_H */
