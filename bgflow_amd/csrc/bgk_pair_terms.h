/* bgk_pair_terms.h -- the energy of ONE particle-system sample, as bgk_pair.hip's forward and bgk_mcmc.hip's chain step both add it up:
 * the pairs i < j in ascending (i, j) order, the terms of one i in f32, the n - 1 row sums and the centroid term in f64.  One source, so
 * the two kernels give the same bits for the same row (the library is built with -ffp-contract=off: the same sequence of IEEE ops).
 * The parameters come in the target record, BgkPairTarget of bgk_pair_tile.h (tg: n, p0..p3, osc; box for KIND 3 / 4); rm2 = p1 p1 and
 * c12 = -12 p0 / rm2 are formed from it here, on the device, in f32.
 *   KIND 0  Lennard-Jones        p0 = eps, p1 = rm, rm2 = rm^2:  eps sum [(rm2 / (d2 + 1e-6))^6 - 2 (rm2 / (d2 + 1e-6))^3]
 *   KIND 1  multi-double-well    p0 = a, p1 = b, p2 = c, p3 = offset:  sum [a t^4 + b t^2 + c], t = sqrt(d2) - offset
 *   KIND 2  mean-free normal     no pair term
 *   + osc 0.5 sum_i |x_i - xbar|^2 when osc != 0
 * xr: the sample's row [n D] (LDS or registers' backing memory), read-only.
 * bgk_pair_row_gradient: d e / d x of the same row, as bgk_pair.hip's backward and bgk_langevin.hip's force both add it up.
 * bgk_pair_row_hvp: that gradient and (d^2 e / d x^2) u in one pass over the pairs, for bgk_pair.hip's hvp kernel and bgk_langevin.hip's
 * adjoint sweep.
 * The particle box (bgflow/distribution/energy/particles.py: a dimer, particles 0 and 1, in a bath of solvent particles in a 2-d box;
 * rows [x0, y0, x1, y1, ...]) is two further kinds with a parameter record of their own, BgkBoxParams (tg.box), and the same discipline:
 *   KIND 3  RepulsiveParticles   eps sum (rm2 / d2)^6 over the pairs i < j except (0, 1); no epsilon: coincident particles give +inf
 *   KIND 4  HarmonicParticles    spring sum (sqrt(d2) - rc)^2 over those pairs with d2 < rc^2
 *   + dimer  dimer_k (x0 + x1)^2 + dimer_k y0^2 + dimer_k y1^2 + slope t - a t^2 + b t^4,  t = 2 (|r0 - r1| - dmid)
 *   + box    2 box_k delta^2 for every coordinate c and both delta = -(c + half) and delta = c - half, where delta > 0
 *            (the reference's (sign(delta) + 1) box_k delta^2: the factor is 2, and 0 where delta < 0; delta = 0 adds 0 either way)
 * bgk_box_row_energy / bgk_box_row_gradient; no Hessian-vector form.  The kernels call bgk_row_energy / bgk_row_gradient (at the end),
 * which pick the pair or the box form by KIND. */
#ifndef BGK_PAIR_TERMS_H
#define BGK_PAIR_TERMS_H

#include "bgk_pair_tile.h"     /* BgkPairTarget, BgkBoxParams */

/* 0.5 sum_i |x_i - xbar|^2 of the row (f64 sum of f32 squares); xbar[k] left in `mean` */
template <int D>
__device__ __forceinline__ double bgk_pair_centroid_term(const float* xr, int n, float* mean) {
    float inv_n = 1.0f / (float)n;
#pragma unroll
    for (int k = 0; k < D; ++k) {
        float s = 0.0f;
        for (int i = 0; i < n; ++i) s += xr[i * D + k];
        mean[k] = s * inv_n;
    }
    double acc = 0.0;
    for (int i = 0; i < n; ++i) {
        float q = 0.0f;
#pragma unroll
        for (int k = 0; k < D; ++k) { const float t = xr[i * D + k] - mean[k]; q += t * t; }
        acc += (double)q;
    }
    return 0.5 * acc;
}

/* e(x) of the row at temperature 1, before the rounding to f32 */
template <int D, int KIND>
__device__ __forceinline__ double bgk_pair_row_energy(const float* xr, const BgkPairTarget& tg) {
    const int n = tg.n;
    const float p0 = tg.p0, p1 = tg.p1, p2 = tg.p2, p3 = tg.p3, osc = tg.osc, rm2 = p1 * p1;
    double e = 0.0;
    if (KIND != 2) {
        for (int i = 0; i + 1 < n; ++i) {
            float xi[D];
#pragma unroll
            for (int k = 0; k < D; ++k) xi[k] = xr[i * D + k];
            float row = 0.0f;
            for (int j = i + 1; j < n; ++j) {
                float d2 = 0.0f;
#pragma unroll
                for (int k = 0; k < D; ++k) { const float t = xi[k] - xr[j * D + k]; d2 += t * t; }
                if (KIND == 0) {
                    const float s = rm2 / (d2 + 1e-6f), s3 = s * s * s;
                    row += s3 * s3 - 2.0f * s3;
                } else {
                    const float t = __builtin_sqrtf(d2) - p3, t2 = t * t;
                    row += (p0 * t2) * t2 + p1 * t2 + p2;
                }
            }
            e += (double)row;
        }
        if (KIND == 0) e *= (double)p0;
    }
    if (osc != 0.0f) { float mean[D]; e += (double)osc * bgk_pair_centroid_term<D>(xr, n, mean); }
    return e;
}

/* d e / d x of the row at temperature 1, as bgk_pair.hip's backward and bgk_langevin.hip's force both add it up: gw [n D] is the lane's
 * OWN row of an LDS tile (zeroed here; g_i in registers over the j loop, g_j read-modify-write, pairs in ascending (i, j) order, then
 * the oscillator term), all in f32.  c12 = -12 p0 / rm2 (KIND 0).  At d_ij = 0 the double-well pair gradient is 0. */
template <int D, int KIND>
__device__ __forceinline__ void bgk_pair_row_gradient(const float* xr, float* gw, const BgkPairTarget& tg) {
    const int n = tg.n;
    const float p0 = tg.p0, p1 = tg.p1, p3 = tg.p3, osc = tg.osc, rm2 = p1 * p1, c12 = -12.0f * p0 / rm2;
    for (int c = 0; c < n * D; ++c) gw[c] = 0.0f;
    if (KIND != 2) {
        for (int i = 0; i + 1 < n; ++i) {
            float xi[D], gi[D];
#pragma unroll
            for (int k = 0; k < D; ++k) { xi[k] = xr[i * D + k]; gi[k] = 0.0f; }
            for (int j = i + 1; j < n; ++j) {
                float df[D], d2 = 0.0f;
#pragma unroll
                for (int k = 0; k < D; ++k) { df[k] = xi[k] - xr[j * D + k]; d2 += df[k] * df[k]; }
                float cf;                       /* d e_ij / d x_i = cf (x_i - x_j) */
                if (KIND == 0) {
                    const float s = rm2 / (d2 + 1e-6f), s3 = s * s * s;
                    cf = c12 * ((s3 * s3 - s3) * s);
                } else {
                    const float dist = __builtin_sqrtf(d2), t = dist - p3;
                    cf = dist > 0.0f ? (4.0f * p0 * (t * t * t) + 2.0f * p1 * t) / dist : 0.0f;
                }
#pragma unroll
                for (int k = 0; k < D; ++k) { const float v = cf * df[k]; gi[k] += v; gw[j * D + k] -= v; }
            }
#pragma unroll
            for (int k = 0; k < D; ++k) gw[i * D + k] += gi[k];
        }
    }
    if (osc != 0.0f) {                          /* d / d x_i of osc 0.5 sum |x - xbar|^2 = osc (x_i - xbar) */
        float mean[D];
        const float inv_n = 1.0f / (float)n;
#pragma unroll
        for (int k = 0; k < D; ++k) {
            float s = 0.0f;
            for (int i = 0; i < n; ++i) s += xr[i * D + k];
            mean[k] = s * inv_n;
        }
        for (int i = 0; i < n; ++i)
#pragma unroll
            for (int k = 0; k < D; ++k) gw[i * D + k] += osc * (xr[i * D + k] - mean[k]);
    }
}

/* g = d e / d x AND Hu = (d^2 e / d x^2) u of the row at temperature 1 in ONE pass over the pairs, in bgk_pair_row_gradient's order and
 * with its arithmetic for g (the same bits); ur [n D]: the vector, gw and hw [n D]: the lane's OWN rows of two LDS tiles (zeroed here).
 * WITH_G = false: only Hu (gw is not touched).  Per pair, df = x_i - x_j, d2 = |df|^2, du = u_i - u_j, s = df . du:
 *   (Hu)_i += cf du + 2 cf' s df,  (Hu)_j -= the same,  cf as in the gradient, cf' = d cf / d d2:
 *   KIND 0  q = d2 + 1e-6, sg = rm2 / q:  cf = c12 (sg^7 - sg^4),  cf' = -c12 (7 sg^7 - 4 sg^4) / q
 *   KIND 1  r = sqrt(d2), t = r - offset, f1 = 4 a t^3 + 2 b t, f2 = 12 a t^2 + 2 b:  cf = f1 / r,  cf' = (f2 / r - f1 / r^2) / (2 r);
 *           at r = 0 both are 0, the gradient's convention
 *   oscillator  (Hu)_i += osc (u_i - ubar) */
template <int D, int KIND, bool WITH_G = true>
__device__ __forceinline__ void bgk_pair_row_hvp(const float* xr, const float* ur, float* gw, float* hw, const BgkPairTarget& tg) {
    const int n = tg.n;
    const float p0 = tg.p0, p1 = tg.p1, p3 = tg.p3, osc = tg.osc, rm2 = p1 * p1, c12 = -12.0f * p0 / rm2;
    for (int c = 0; c < n * D; ++c) { if (WITH_G) gw[c] = 0.0f; hw[c] = 0.0f; }
    if (KIND != 2) {
        for (int i = 0; i + 1 < n; ++i) {
            float xi[D], ui[D], gi[D], hi[D];
#pragma unroll
            for (int k = 0; k < D; ++k) { xi[k] = xr[i * D + k]; ui[k] = ur[i * D + k]; gi[k] = 0.0f; hi[k] = 0.0f; }
            for (int j = i + 1; j < n; ++j) {
                float df[D], du[D], d2 = 0.0f, s = 0.0f;
#pragma unroll
                for (int k = 0; k < D; ++k) {
                    df[k] = xi[k] - xr[j * D + k]; du[k] = ui[k] - ur[j * D + k];
                    d2 += df[k] * df[k]; s += df[k] * du[k];
                }
                float cf, cfp;                  /* d e_ij / d x_i = cf (x_i - x_j); cfp = d cf / d d2 */
                if (KIND == 0) {
                    const float q = d2 + 1e-6f, sg = rm2 / q, s3 = sg * sg * sg, s4 = s3 * sg, s7 = (s3 * s3) * sg;
                    cf = c12 * ((s3 * s3 - s3) * sg);
                    cfp = -c12 * (7.0f * s7 - 4.0f * s4) / q;
                } else {
                    const float dist = __builtin_sqrtf(d2), t = dist - p3;
                    const float f1 = 4.0f * p0 * (t * t * t) + 2.0f * p1 * t, f2 = 12.0f * p0 * (t * t) + 2.0f * p1;
                    cf = dist > 0.0f ? f1 / dist : 0.0f;
                    cfp = dist > 0.0f ? (f2 / dist - f1 / d2) / (2.0f * dist) : 0.0f;
                }
                const float c2s = 2.0f * cfp * s;
#pragma unroll
                for (int k = 0; k < D; ++k) {
                    if (WITH_G) { const float v = cf * df[k]; gi[k] += v; gw[j * D + k] -= v; }
                    const float w = cf * du[k] + c2s * df[k];
                    hi[k] += w; hw[j * D + k] -= w;
                }
            }
#pragma unroll
            for (int k = 0; k < D; ++k) { if (WITH_G) gw[i * D + k] += gi[k]; hw[i * D + k] += hi[k]; }
        }
    }
    if (osc != 0.0f) {                          /* the Hessian of osc 0.5 sum |x - xbar|^2 is osc (1 - 1 1^T / n) per dimension */
        float mean[D], umean[D];
        const float inv_n = 1.0f / (float)n;
#pragma unroll
        for (int k = 0; k < D; ++k) {
            float s = 0.0f, su = 0.0f;
            for (int i = 0; i < n; ++i) { s += xr[i * D + k]; su += ur[i * D + k]; }
            mean[k] = s * inv_n; umean[k] = su * inv_n;
        }
        for (int i = 0; i < n; ++i)
#pragma unroll
            for (int k = 0; k < D; ++k) {
                if (WITH_G) gw[i * D + k] += osc * (xr[i * D + k] - mean[k]);
                hw[i * D + k] += osc * (ur[i * D + k] - umean[k]);
            }
    }
}

/* e(x) of the row [2 n] at temperature 1, before the rounding to f32: the pair terms of one i in f32, the row sums, the dimer's terms and
 * the box terms of one particle in f64 */
template <int KIND>
__device__ __forceinline__ double bgk_box_row_energy(const float* xr, int n, const BgkBoxParams& p) {
    double e = 0.0;
    for (int i = 0; i + 1 < n; ++i) {
        const float xi = xr[2 * i], yi = xr[2 * i + 1];
        float row = 0.0f;
        for (int j = i == 0 ? 2 : i + 1; j < n; ++j) {      /* (0, 1) is the dimer: no pair term */
            const float dx = xi - xr[2 * j], dy = yi - xr[2 * j + 1];
            const float d2 = dx * dx + dy * dy;
            if (KIND == 3) {
                const float s = p.rm2 / d2, s3 = s * s * s;
                row += s3 * s3;
            } else {
                const float t = __builtin_sqrtf(d2) - p.rc;
                row += d2 < p.rc2 ? t * t : 0.0f;
            }
        }
        e += (double)row;
    }
    e *= (double)(KIND == 3 ? p.eps : p.spring);
    {
        const float x0 = xr[0], y0 = xr[1], x1 = xr[2], y1 = xr[3];
        const float sx = x0 + x1, dx = x0 - x1, dy = y0 - y1;
        const float t = 2.0f * (__builtin_sqrtf(dx * dx + dy * dy) - p.dimer_dmid), t2 = t * t;
        e += (double)(p.dimer_k * (sx * sx));
        e += (double)(p.dimer_k * (y0 * y0));
        e += (double)(p.dimer_k * (y1 * y1));
        e += (double)(p.dimer_slope * t);
        e -= (double)(p.dimer_a * t2);
        e += (double)(p.dimer_b * (t2 * t2));
    }
    const float k2 = 2.0f * p.box_k;
    for (int i = 0; i < n; ++i) {
        float w = 0.0f;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const float c = xr[2 * i + k], lo = -(c + p.box_half), hi = c - p.box_half;
            w += lo > 0.0f ? k2 * (lo * lo) : 0.0f;
            w += hi > 0.0f ? k2 * (hi * hi) : 0.0f;
        }
        e += (double)w;
    }
    return e;
}

/* d e / d x of that row in bgk_pair_row_gradient's pattern: gw [2 n] is the lane's OWN row of an LDS tile (zeroed here), all in f32.
 * The harmonic pair gradient at d_ij = 0 is 0 (the double-well kind's convention); the repulsive one at d_ij = 0 and the dimer's at
 * |r0 - r1| = 0 are what the f32 arithmetic gives (non-finite). */
template <int KIND>
__device__ __forceinline__ void bgk_box_row_gradient(const float* xr, float* gw, int n, const BgkBoxParams& p) {
    for (int c = 0; c < 2 * n; ++c) gw[c] = 0.0f;
    const float c12 = -12.0f * p.eps / p.rm2, k2s = 2.0f * p.spring;
    for (int i = 0; i + 1 < n; ++i) {
        const float xi = xr[2 * i], yi = xr[2 * i + 1];
        float gx = 0.0f, gy = 0.0f;
        for (int j = i == 0 ? 2 : i + 1; j < n; ++j) {
            const float dx = xi - xr[2 * j], dy = yi - xr[2 * j + 1];
            const float d2 = dx * dx + dy * dy;
            float cf;                           /* d e_ij / d x_i = cf (x_i - x_j) */
            if (KIND == 3) {
                const float s = p.rm2 / d2, s3 = s * s * s;
                cf = c12 * ((s3 * s3) * s);     /* -12 eps rm2^6 / d2^7 */
            } else {
                const float dist = __builtin_sqrtf(d2);
                cf = (d2 < p.rc2 && dist > 0.0f) ? k2s * (dist - p.rc) / dist : 0.0f;
            }
            const float vx = cf * dx, vy = cf * dy;
            gx += vx; gy += vy;
            gw[2 * j] -= vx; gw[2 * j + 1] -= vy;
        }
        gw[2 * i] += gx; gw[2 * i + 1] += gy;
    }
    {
        const float x0 = xr[0], y0 = xr[1], x1 = xr[2], y1 = xr[3];
        const float sx = x0 + x1, dx = x0 - x1, dy = y0 - y1;
        const float r = __builtin_sqrtf(dx * dx + dy * dy), t = 2.0f * (r - p.dimer_dmid);
        /* d / d r of slope t - a t^2 + b t^4 with d t / d r = 2 */
        const float f = 2.0f * (p.dimer_slope - 2.0f * p.dimer_a * t + 4.0f * p.dimer_b * (t * t * t)) / r;
        const float kc = 2.0f * p.dimer_k;
        gw[0] += kc * sx + f * dx; gw[1] += kc * y0 + f * dy;
        gw[2] += kc * sx - f * dx; gw[3] += kc * y1 - f * dy;
    }
    const float k4 = 4.0f * p.box_k;
    for (int c = 0; c < 2 * n; ++c) {
        const float v = xr[c], lo = -(v + p.box_half), hi = v - p.box_half;
        gw[c] += (hi > 0.0f ? k4 * hi : 0.0f) - (lo > 0.0f ? k4 * lo : 0.0f);
    }
}

/* the row's energy / gradient for any KIND: the one place that chooses between the pair and the box forms */
template <int D, int KIND>
__device__ __forceinline__ double bgk_row_energy(const float* xr, const BgkPairTarget& tg) {
    if constexpr (KIND >= 3) return bgk_box_row_energy<KIND>(xr, tg.n, tg.box);
    else return bgk_pair_row_energy<D, KIND>(xr, tg);
}

template <int D, int KIND>
__device__ __forceinline__ void bgk_row_gradient(const float* xr, float* gw, const BgkPairTarget& tg) {
    if constexpr (KIND >= 3) bgk_box_row_gradient<KIND>(xr, gw, tg.n, tg.box);
    else bgk_pair_row_gradient<D, KIND>(xr, gw, tg);
}

#endif
