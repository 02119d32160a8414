/* bgk_philox.h -- the counter-based generator of bgk_philox.hip, shared with the kernels that draw inside their own launch
 * (bgk_mcmc.hip): Philox4x32-10 (Salmon et al., SC'11), the word -> [2^-25, 1 - 2^-24] map and the Box-Muller pair on the deterministic
 * log / sincos of bgk_detmath.h.  Counter layout of every user: (global row low, high, field << 20 | 4-column block, call offset),
 * key = seed; one call gives the four columns 4 cb .. 4 cb + 3 of a row. */
#ifndef BGK_PHILOX_H
#define BGK_PHILOX_H

#include "bgk_common.h"

__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t (&o)[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    o[0] = c0; o[1] = c1; o[2] = c2; o[3] = c3;
}
/* u = ((x >> 8) + 0.5) 2^-24 in f32, in [2^-25, 1 - 2^-24].  The sum needs 25 significand bits: exact for x >> 8 < 2^23, rounded
 * to even above (|error| <= 2^-25, mean 0).  Unclamped, the 256 largest words would round to 1.0; the minimum moves only those. */
__device__ __forceinline__ float u01(uint32_t x) {
    return __builtin_fminf(((float)(x >> 8) + 0.5f) * 5.9604644775390625e-08f /* 2^-24 */, 0x1.fffffep-1f);
}

/* four standard normals from the four words of one call: r = sqrt(-2 ln u1), (r cos 2 pi u2, r sin 2 pi u2) per word pair */
__device__ __forceinline__ void philox_normal4(const uint32_t (&o)[4], float (&v)[4]) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const float rad = __builtin_sqrtf(-2.0f * bgk_logf(u01(o[2 * h])));
        float sn, cs;
        bgk_sincos2pif(u01(o[2 * h + 1]), &sn, &cs);
        v[2 * h] = rad * cs; v[2 * h + 1] = rad * sn;
    }
}

/* the four normals of columns 4 cb .. 4 cb + 3 of a field: the explicit row (columns beyond n d: 0) or the Philox block */
__device__ __forceinline__ void philox_field_normal4(const float* row, int nd, int cb, uint32_t r_lo, uint32_t r_hi, uint32_t field,
                                                     uint32_t off, uint32_t k0, uint32_t k1, float (&w)[4]) {
    if (row) {
#pragma unroll
        for (int j = 0; j < 4; ++j) w[j] = 4 * cb + j < nd ? row[4 * cb + j] : 0.0f;
    } else {
        uint32_t o[4];
        philox4x32_10(r_lo, r_hi, (field << 20) | (uint32_t)cb, off, k0, k1, o);
        philox_normal4(o, w);
    }
}

/* the one uniform of a field: the explicit number, or word 0 of the field's block 0 */
__device__ __forceinline__ float philox_field_uniform(const float* given, uint32_t r_lo, uint32_t r_hi, uint32_t field, uint32_t off,
                                                      uint32_t k0, uint32_t k1) {
    if (given) return *given;
    uint32_t o[4];
    philox4x32_10(r_lo, r_hi, field << 20, off, k0, k1, o);
    return u01(o[0]);
}

#endif
