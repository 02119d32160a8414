/* bgk_molecule_terms.h -- the force-field energy of ONE molecule's row and its gradient, as bgk_molecule.hip's kernels add them up; the
 * functions are host and device code, so that the same arithmetic can be run on a CPU.  Units nm, kJ/mol, rad; the forms are OpenMM's:
 *   bonds     (HarmonicBondForce)      k / 2 (r - r0)^2
 *   angles    (HarmonicAngleForce)     k / 2 (theta - theta0)^2 at the middle atom; theta = atan2(|a x b|, a . b), its derivative through
 *                                      the cross product c = a x b: d theta / d a = (a x c) / (|a|^2 |c|), d theta / d b = (c x b) / (|b|^2 |c|)
 *                                      -- singular only where the three atoms are collinear, not where 1 - cos^2 rounds to zero
 *   torsions  (PeriodicTorsionForce)   k (1 + cos(n phi - phase)) = k + kc cos(n phi) + ks sin(n phi), kc = k cos(phase), ks = k sin(phase);
 *                                      b1 = x_j - x_i, b2 = x_k - x_j, b3 = x_l - x_k, n1 = b1 x b2, n2 = b2 x b3 (IUPAC: trans = pi),
 *                                      (cos phi, sin phi) = (n1 . n2, |b2| b1 . n2) normalised; (cos, sin)(n phi) by n - 1 complex products,
 *                                      n <= 6: no transcendental call; d phi / d x_i = -|b2| n1 / |n1|^2, d phi / d x_l = |b2| n2 / |n2|^2,
 *                                      d phi / d x_j = (p - 1) d_i - q d_l, d phi / d x_k = (q - 1) d_l - p d_i with p = -(b1 . b2) / |b2|^2,
 *                                      q = -(b3 . b2) / |b2|^2 (Blondel and Karplus 1996): singular only where three atoms are collinear
 *   pairs     (NonbondedForce, NoCutoff)  e4 ((sigma / r)^12 - (sigma / r)^6) + qq / r over the dense table of the pairs i < j in ascending
 *                                      (i, j) order, (qq, sigma, e4) = (138.935458 q_i q_j, sigma_ij, 4 eps_ij) with the combination rules,
 *                                      exclusions and exceptions applied by the host; qq = 0 and e4 = 0: the pair is excluded
 * The terms are added in table order (bonds, angles, torsions, pairs) in f32 with a compensated running sum.  A pair that interacts at
 * r = 0 makes the row's energy +inf (never NaN) and contributes no gradient.
 * Tables (packed by bgflow_amd/molecule.py, read-only, wave-uniform reads): `terms` int4 [n_bonds + n_angles + n_torsions], word 0 the atoms
 * in 6-bit fields (i | j << 6 | k << 12 | l << 18, torsions: | periodicity << 24), words 1..3 f32 bits: bonds (r0, k, -), angles (theta0, k, -),
 * torsions (k, kc, ks); `pairs` float [n (n - 1) / 2][3] or none.  An atom index is clamped to n - 1: no read or write leaves the row.
 * xr: the row [3 n] (LDS), read-only; gw: the lane's OWN row of a second tile. */
#ifndef BGK_MOLECULE_TERMS_H
#define BGK_MOLECULE_TERMS_H

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#define BGK_MM_FN __host__ __device__ __forceinline__

struct BgkMolecule {
    int n, n_bonds, n_angles, n_torsions, n_pairs;      /* n_pairs: 0 (no nonbonded tables) or n (n - 1) / 2 */
};

struct BgkMMSum {                                       /* compensated f32 running sum (the library is built without fast-math) */
    float s, c;
    BGK_MM_FN void add(float v) { const float y = v - c; const float t = s + y; c = (t - s) - y; s = t; }
};

struct BgkMMVec { float x, y, z; };

BGK_MM_FN float bgk_mm_bits(int32_t w) { union { int32_t i; float f; } c; c.i = w; return c.f; }
BGK_MM_FN int bgk_mm_atom(int32_t w, int shift, int n) { const int a = (w >> shift) & 63; return 3 * (a < n ? a : n - 1); }
BGK_MM_FN BgkMMVec bgk_mm_diff(const float* xr, int a3, int b3) { return BgkMMVec{xr[a3] - xr[b3], xr[a3 + 1] - xr[b3 + 1], xr[a3 + 2] - xr[b3 + 2]}; }
BGK_MM_FN float bgk_mm_dot(const BgkMMVec& a, const BgkMMVec& b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
BGK_MM_FN BgkMMVec bgk_mm_cross(const BgkMMVec& a, const BgkMMVec& b) { return BgkMMVec{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
BGK_MM_FN void bgk_mm_axpy(float* g, int a3, float s, const BgkMMVec& v) { g[a3] += s * v.x; g[a3 + 1] += s * v.y; g[a3 + 2] += s * v.z; }

/* (cos, sin)(phi) of a torsion and what its derivative needs */
struct BgkMMTorsion { BgkMMVec n1, n2; float c, s, lb2, n1n1, n2n2, p, q; };

BGK_MM_FN BgkMMTorsion bgk_mm_torsion(const float* xr, int i3, int j3, int k3, int l3) {
    const BgkMMVec b1 = bgk_mm_diff(xr, j3, i3), b2 = bgk_mm_diff(xr, k3, j3), b3 = bgk_mm_diff(xr, l3, k3);
    BgkMMTorsion t;
    t.n1 = bgk_mm_cross(b1, b2); t.n2 = bgk_mm_cross(b2, b3);
    const float b2b2 = bgk_mm_dot(b2, b2);
    t.lb2 = __builtin_sqrtf(b2b2);
    const float X = bgk_mm_dot(t.n1, t.n2), Y = t.lb2 * bgk_mm_dot(b1, t.n2);
    const float inv = 1.0f / __builtin_sqrtf(X * X + Y * Y);
    t.c = X * inv; t.s = Y * inv;
    t.n1n1 = bgk_mm_dot(t.n1, t.n1); t.n2n2 = bgk_mm_dot(t.n2, t.n2);
    t.p = -bgk_mm_dot(b1, b2) / b2b2; t.q = -bgk_mm_dot(b3, b2) / b2b2;
    return t;
}

/* (cos, sin)(m phi), m = 1..6, from (c, s) = (cos, sin)(phi) */
BGK_MM_FN void bgk_mm_multiple(float c, float s, int m, float* cm, float* sm) {
    float a = c, b = s;
    for (int r = 1; r < m; ++r) { const float a2 = a * c - b * s; b = b * c + a * s; a = a2; }
    *cm = a; *sm = b;
}

/* E(x) of the row in kJ/mol; +inf where a pair that interacts is at distance 0 */
BGK_MM_FN float bgk_mm_row_energy(const float* xr, const int4* __restrict__ terms, const float* __restrict__ pairs, const BgkMolecule& m) {
    const int n = m.n;
    BgkMMSum e{0.0f, 0.0f};
    bool singular = false;
    int t = 0;
    for (int end = m.n_bonds; t < end; ++t) {
        const int4 w = terms[t];
        const BgkMMVec d = bgk_mm_diff(xr, bgk_mm_atom(w.x, 0, n), bgk_mm_atom(w.x, 6, n));
        const float dr = __builtin_sqrtf(bgk_mm_dot(d, d)) - bgk_mm_bits(w.y);
        e.add(0.5f * bgk_mm_bits(w.z) * (dr * dr));
    }
    for (int end = t + m.n_angles; t < end; ++t) {
        const int4 w = terms[t];
        const int j3 = bgk_mm_atom(w.x, 6, n);
        const BgkMMVec a = bgk_mm_diff(xr, bgk_mm_atom(w.x, 0, n), j3), b = bgk_mm_diff(xr, bgk_mm_atom(w.x, 12, n), j3);
        const BgkMMVec c = bgk_mm_cross(a, b);
        const float dth = atan2f(__builtin_sqrtf(bgk_mm_dot(c, c)), bgk_mm_dot(a, b)) - bgk_mm_bits(w.y);
        e.add(0.5f * bgk_mm_bits(w.z) * (dth * dth));
    }
    for (int end = t + m.n_torsions; t < end; ++t) {
        const int4 w = terms[t];
        const BgkMMTorsion ts = bgk_mm_torsion(xr, bgk_mm_atom(w.x, 0, n), bgk_mm_atom(w.x, 6, n), bgk_mm_atom(w.x, 12, n), bgk_mm_atom(w.x, 18, n));
        float cm, sm;
        bgk_mm_multiple(ts.c, ts.s, (w.x >> 24) & 7, &cm, &sm);
        e.add(bgk_mm_bits(w.y) + (bgk_mm_bits(w.z) * cm + bgk_mm_bits(w.w) * sm));
    }
    if (m.n_pairs) {
        int p = 0;
        for (int i = 0; i + 1 < n; ++i) {
            const float xi = xr[3 * i], yi = xr[3 * i + 1], zi = xr[3 * i + 2];
            for (int j = i + 1; j < n; ++j, ++p) {
                const float qq = pairs[3 * p], sg = pairs[3 * p + 1], e4 = pairs[3 * p + 2];
                if (qq == 0.0f && e4 == 0.0f) continue;
                const float dx = xi - xr[3 * j], dy = yi - xr[3 * j + 1], dz = zi - xr[3 * j + 2];
                const float d2 = (dx * dx + dy * dy) + dz * dz;
                if (d2 == 0.0f) { singular = true; continue; }
                const float inv_r = 1.0f / __builtin_sqrtf(d2), sr = sg * inv_r, sr2 = sr * sr, s6 = sr2 * sr2 * sr2;
                e.add(e4 * (s6 * s6 - s6) + qq * inv_r);
            }
        }
    }
    return singular ? INFINITY : e.s;
}

/* d E / d x of the row in gw [3 n] (zeroed here), accumulated in table order in f32 */
BGK_MM_FN void bgk_mm_row_gradient(const float* xr, float* gw, const int4* __restrict__ terms, const float* __restrict__ pairs,
                                   const BgkMolecule& m) {
    const int n = m.n;
    for (int c = 0; c < 3 * n; ++c) gw[c] = 0.0f;
    int t = 0;
    for (int end = m.n_bonds; t < end; ++t) {
        const int4 w = terms[t];
        const int i3 = bgk_mm_atom(w.x, 0, n), j3 = bgk_mm_atom(w.x, 6, n);
        const BgkMMVec d = bgk_mm_diff(xr, i3, j3);
        const float r = __builtin_sqrtf(bgk_mm_dot(d, d));
        const float f = r > 0.0f ? bgk_mm_bits(w.z) * (r - bgk_mm_bits(w.y)) / r : 0.0f;
        bgk_mm_axpy(gw, i3, f, d); bgk_mm_axpy(gw, j3, -f, d);
    }
    for (int end = t + m.n_angles; t < end; ++t) {
        const int4 w = terms[t];
        const int i3 = bgk_mm_atom(w.x, 0, n), j3 = bgk_mm_atom(w.x, 6, n), k3 = bgk_mm_atom(w.x, 12, n);
        const BgkMMVec a = bgk_mm_diff(xr, i3, j3), b = bgk_mm_diff(xr, k3, j3);
        const BgkMMVec c = bgk_mm_cross(a, b);
        const float cn = __builtin_sqrtf(bgk_mm_dot(c, c));
        const float f = bgk_mm_bits(w.z) * (atan2f(cn, bgk_mm_dot(a, b)) - bgk_mm_bits(w.y));
        const float fa = f / (bgk_mm_dot(a, a) * cn), fb = f / (bgk_mm_dot(b, b) * cn);
        const BgkMMVec da = bgk_mm_cross(a, c), db = bgk_mm_cross(c, b);
        bgk_mm_axpy(gw, i3, fa, da); bgk_mm_axpy(gw, k3, fb, db);
        bgk_mm_axpy(gw, j3, -fa, da); bgk_mm_axpy(gw, j3, -fb, db);
    }
    for (int end = t + m.n_torsions; t < end; ++t) {
        const int4 w = terms[t];
        const int i3 = bgk_mm_atom(w.x, 0, n), j3 = bgk_mm_atom(w.x, 6, n), k3 = bgk_mm_atom(w.x, 12, n), l3 = bgk_mm_atom(w.x, 18, n);
        const BgkMMTorsion ts = bgk_mm_torsion(xr, i3, j3, k3, l3);
        const int mult = (w.x >> 24) & 7;
        float cm, sm;
        bgk_mm_multiple(ts.c, ts.s, mult, &cm, &sm);
        const float f = (float)mult * (bgk_mm_bits(w.w) * cm - bgk_mm_bits(w.z) * sm);      /* d E / d phi */
        const float fi = -f * ts.lb2 / ts.n1n1, fl = f * ts.lb2 / ts.n2n2;                  /* d E / d x_i = fi n1, d E / d x_l = fl n2 */
        bgk_mm_axpy(gw, i3, fi, ts.n1); bgk_mm_axpy(gw, l3, fl, ts.n2);
        bgk_mm_axpy(gw, j3, (ts.p - 1.0f) * fi, ts.n1); bgk_mm_axpy(gw, j3, -ts.q * fl, ts.n2);
        bgk_mm_axpy(gw, k3, (ts.q - 1.0f) * fl, ts.n2); bgk_mm_axpy(gw, k3, -ts.p * fi, ts.n1);
    }
    if (m.n_pairs) {
        int p = 0;
        for (int i = 0; i + 1 < n; ++i) {
            const float xi = xr[3 * i], yi = xr[3 * i + 1], zi = xr[3 * i + 2];
            float gx = 0.0f, gy = 0.0f, gz = 0.0f;
            for (int j = i + 1; j < n; ++j, ++p) {
                const float qq = pairs[3 * p], sg = pairs[3 * p + 1], e4 = pairs[3 * p + 2];
                if (qq == 0.0f && e4 == 0.0f) continue;
                const float dx = xi - xr[3 * j], dy = yi - xr[3 * j + 1], dz = zi - xr[3 * j + 2];
                const float d2 = (dx * dx + dy * dy) + dz * dz;
                if (d2 == 0.0f) continue;
                const float inv_r = 1.0f / __builtin_sqrtf(d2), sr = sg * inv_r, sr2 = sr * sr, s6 = sr2 * sr2 * sr2;
                const float cf = -((e4 * (12.0f * (s6 * s6) - 6.0f * s6) + qq * inv_r) * (inv_r * inv_r));     /* d e_ij / d x_i = cf (x_i - x_j) */
                const float vx = cf * dx, vy = cf * dy, vz = cf * dz;
                gx += vx; gy += vy; gz += vz;
                gw[3 * j] -= vx; gw[3 * j + 1] -= vy; gw[3 * j + 2] -= vz;
            }
            gw[3 * i] += gx; gw[3 * i + 1] += gy; gw[3 * i + 2] += gz;
        }
    }
}

#endif /* BGK_MOLECULE_TERMS_H */
