/* bgk_solvent_terms.h -- the implicit-solvent energy (Generalised Born, OBC2, plus the ACE surface term: the arithmetic of OpenMM's
 * GBSAOBCForce, stated from its published form) of ONE molecule's row and its gradient, as bgk_molecule.hip's solvent kernels add them to
 * the vacuum terms of bgk_molecule_terms.h; host and device code, one lane per sample.  Units nm, kJ/mol, elementary charges.
 *   per atom i: charge q_i, radius r_i, scale s_i;  rho_i = r_i - 0.009,  sigma_i = s_i rho_i
 *   over ALL ordered pairs j != i (no exclusions, no exceptions), r the distance:
 *     H(r, rho_i, sigma_j) = 0                                                     if rho_i >= r + sigma_j      (a) j's sphere inside i's
 *       else, l = 1 / max(rho_i, |r - sigma_j|), u = 1 / (r + sigma_j):
 *     H = l - u + (r / 4)(u^2 - l^2) + ln(u / l) / (2 r) + sigma_j^2 (l^2 - u^2) / (4 r)
 *         + 2 (1 / rho_i - l)                                                      only if rho_i < sigma_j - r  (d) i inside j's sphere
 *     ((b) separate spheres: l = 1 / (r - sigma_j); (c) overlapping spheres: l = 1 / rho_i; H is continuous across the four)
 *     d H / d r = -(l^2 - u^2)(1 + sigma_j^2 / r^2) / 4 - ln(u / l) / (2 r^2)      in (b), (c), (d): d H / d l = 0 where l moves with r
 *                                                                                  and d H / d u = 0 throughout; 0 in (a)
 *     Psi_i = (rho_i / 2) sum_j H,   1 / B_i = 1 / rho_i - tanh(Psi_i - 0.8 Psi_i^2 + 4.85 Psi_i^3) / r_i      (B_i > 0: rho_i < r_i)
 *   E_GB = pre [ sum_i q_i^2 / (2 B_i) + sum_{i<j} q_i q_j / f_ij ],  f_ij^2 = r^2 + B_i B_j exp(-r^2 / (4 B_i B_j)),
 *          pre = -138.935458 (1 / eps_solute - 1 / eps_solvent)
 *   E_SA = sum_i sa_i / B_i^6,  sa_i = 4 pi gamma (r_i + 0.14)^2 r_i^6
 * The four regimes of H differ per lane: H and d H / d r are selects over one code path.  Sums run in a fixed order (pairs in ascending
 * (i, j), atoms in atom order), the energy in a compensated f32 sum.  ANY two atoms at r = 0 make the row's solvent energy +inf (never NaN);
 * the solvent terms then contribute no gradient to the row.
 * Table (packed by bgflow_amd/molecule.py in double, rounded once; read-only, wave-uniform reads): `atoms` float4 [n] = (q_i, rho_i, sigma_i,
 * r_i), followed by float [n] = sa_i.
 * xr: the row [3 n] (LDS), read-only.  born: n floats of the lane's own (B_i).  scratch: 3 n floats of the lane's own (B_i; d E / d B_i, then
 * its product with the chain factor; the chain factor d B_i / d Psi_i rho_i / 2).  gw: the lane's OWN gradient row, added to. */
#ifndef BGK_SOLVENT_TERMS_H
#define BGK_SOLVENT_TERMS_H

#include "bgk_molecule_terms.h"

struct BgkSolvent {
    int n;
    float pre;                                          /* -138.935458 (1 / eps_solute - 1 / eps_solvent) */
};

/* H(r, rho_i, sigma_j) and d H / d r; inv_r = 1 / r, inv_rho = 1 / rho_i */
BGK_MM_FN float bgk_gb_h(float r, float inv_r, float rho, float inv_rho, float sg, float* dh) {
    const float l = 1.0f / fmaxf(rho, fabsf(r - sg)), u = 1.0f / (r + sg);
    const float l2u2 = l * l - u * u, lg = logf(u / l), sg2 = sg * sg;
    float h = (l - u) - 0.25f * r * l2u2 + 0.5f * inv_r * lg + 0.25f * sg2 * inv_r * l2u2;
    h += rho < sg - r ? 2.0f * (inv_rho - l) : 0.0f;
    const float d = -0.25f * l2u2 * (1.0f + sg2 * (inv_r * inv_r)) - 0.5f * lg * (inv_r * inv_r);
    const bool inside = rho >= r + sg;
    *dh = inside ? 0.0f : d;
    return inside ? 0.0f : h;
}

/* pass 1: born[i] = B_i for every atom (chain != NULL: chain[i] = d B_i / d Psi_i rho_i / 2); false if two atoms coincide */
BGK_MM_FN bool bgk_gb_born(const float* xr, float* born, float* chain, const float4* __restrict__ atoms, const BgkSolvent& m) {
    const int n = m.n;
    bool apart = true;
    for (int i = 0; i < n; ++i) born[i] = 0.0f;                     /* sum_j H(i, j) while the pairs run */
    for (int i = 0; i < n; ++i) {
        const float4 ai = atoms[i];
        const float xi = xr[3 * i], yi = xr[3 * i + 1], zi = xr[3 * i + 2], inv_rho_i = 1.0f / ai.y;
        float hi = 0.0f;
        for (int j = i + 1; j < n; ++j) {
            const float4 aj = atoms[j];
            const float dx = xi - xr[3 * j], dy = yi - xr[3 * j + 1], dz = zi - xr[3 * j + 2];
            const float d2 = (dx * dx + dy * dy) + dz * dz;
            apart = apart && d2 > 0.0f;
            const float r = __builtin_sqrtf(d2 > 0.0f ? d2 : 1.0f), inv_r = 1.0f / r;
            float unused;
            hi += bgk_gb_h(r, inv_r, ai.y, inv_rho_i, aj.z, &unused);
            born[j] += bgk_gb_h(r, inv_r, aj.y, 1.0f / aj.y, ai.z, &unused);
        }
        const float psi = 0.5f * ai.y * (born[i] + hi);
        const float th = tanhf(psi - 0.8f * (psi * psi) + 4.85f * (psi * psi * psi));
        const float b = 1.0f / (inv_rho_i - th / ai.w);
        born[i] = b;
        if (chain) chain[i] = (b * b) * (1.0f - th * th) * (1.0f - 1.6f * psi + 14.55f * (psi * psi)) / ai.w * (0.5f * ai.y);
    }
    return apart;
}

/* E_GB + E_SA of the row in kJ/mol; +inf where two atoms coincide */
BGK_MM_FN float bgk_gb_row_energy(const float* xr, float* born, const float4* __restrict__ atoms, const BgkSolvent& m) {
    const int n = m.n;
    const float* __restrict__ sa = reinterpret_cast<const float*>(atoms + n);
    if (!bgk_gb_born(xr, born, nullptr, atoms, m)) return INFINITY;
    BgkMMSum e{0.0f, 0.0f};
    for (int i = 0; i + 1 < n; ++i) {
        const float xi = xr[3 * i], yi = xr[3 * i + 1], zi = xr[3 * i + 2], bi = born[i], qi = m.pre * atoms[i].x;
        for (int j = i + 1; j < n; ++j) {
            const float dx = xi - xr[3 * j], dy = yi - xr[3 * j + 1], dz = zi - xr[3 * j + 2];
            const float d2 = (dx * dx + dy * dy) + dz * dz, bb = bi * born[j];
            e.add(qi * atoms[j].x / __builtin_sqrtf(d2 + bb * expf(-d2 / (4.0f * bb))));
        }
    }
    for (int i = 0; i < n; ++i) {
        const float q = atoms[i].x, ib = 1.0f / born[i], ib2 = ib * ib;
        e.add(0.5f * m.pre * (q * q) * ib);
        e.add(sa[i] * (ib2 * ib2 * ib2));
    }
    return e.s;
}

/* adds d (E_GB + E_SA) / d x of the row into gw [3 n]; nothing where two atoms coincide */
BGK_MM_FN void bgk_gb_row_gradient(const float* xr, float* gw, float* scratch, const float4* __restrict__ atoms, const BgkSolvent& m) {
    const int n = m.n;
    const float* __restrict__ sa = reinterpret_cast<const float*>(atoms + n);
    float* born = scratch;
    float* de = scratch + n;                           /* d E / d B_i, then times the chain factor */
    float* chain = scratch + 2 * n;
    if (!bgk_gb_born(xr, born, chain, atoms, m)) return;
    for (int i = 0; i < n; ++i) de[i] = 0.0f;
    for (int i = 0; i + 1 < n; ++i) {                  /* pass 2: the pairs at fixed Born radii, and d E / d B */
        const float xi = xr[3 * i], yi = xr[3 * i + 1], zi = xr[3 * i + 2], bi = born[i], qi = m.pre * atoms[i].x;
        float gx = 0.0f, gy = 0.0f, gz = 0.0f, dei = 0.0f;
        for (int j = i + 1; j < n; ++j) {
            const float dx = xi - xr[3 * j], dy = yi - xr[3 * j + 1], dz = zi - xr[3 * j + 2];
            const float d2 = (dx * dx + dy * dy) + dz * dz, bj = born[j], bb = bi * bj;
            const float D = d2 / (4.0f * bb), ex = expf(-D);
            const float inv_f = 1.0f / __builtin_sqrtf(d2 + bb * ex), qf3 = qi * atoms[j].x * (inv_f * inv_f * inv_f);
            const float cf = -(qf3 * (1.0f - 0.25f * ex));                  /* d e_ij / d x_i = cf (x_i - x_j) at fixed B */
            const float cb = -0.5f * qf3 * ex * (1.0f + D);                 /* d e_ij / d B_i = cb B_j */
            const float vx = cf * dx, vy = cf * dy, vz = cf * dz;
            gx += vx; gy += vy; gz += vz;
            gw[3 * j] -= vx; gw[3 * j + 1] -= vy; gw[3 * j + 2] -= vz;
            dei += cb * bj;
            de[j] += cb * bi;
        }
        gw[3 * i] += gx; gw[3 * i + 1] += gy; gw[3 * i + 2] += gz;
        de[i] += dei;
    }
    for (int i = 0; i < n; ++i) {                      /* self and surface terms; then d E / d Psi_i rho_i / 2 */
        const float q = atoms[i].x, ib = 1.0f / born[i], ib2 = ib * ib, ib6 = ib2 * ib2 * ib2;
        de[i] = ((de[i] - 0.5f * m.pre * (q * q) * ib2) - 6.0f * sa[i] * (ib6 * ib)) * chain[i];
    }
    for (int i = 0; i + 1 < n; ++i) {                  /* pass 3: the chain through Psi, both directions of a pair */
        const float4 ai = atoms[i];
        const float xi = xr[3 * i], yi = xr[3 * i + 1], zi = xr[3 * i + 2], inv_rho_i = 1.0f / ai.y, wi = de[i];
        float gx = 0.0f, gy = 0.0f, gz = 0.0f;
        for (int j = i + 1; j < n; ++j) {
            const float4 aj = atoms[j];
            const float dx = xi - xr[3 * j], dy = yi - xr[3 * j + 1], dz = zi - xr[3 * j + 2];
            const float r = __builtin_sqrtf((dx * dx + dy * dy) + dz * dz), inv_r = 1.0f / r;
            float dij, dji;
            bgk_gb_h(r, inv_r, ai.y, inv_rho_i, aj.z, &dij);
            bgk_gb_h(r, inv_r, aj.y, 1.0f / aj.y, ai.z, &dji);
            const float c = (wi * dij + de[j] * dji) * inv_r;
            const float vx = c * dx, vy = c * dy, vz = c * dz;
            gx += vx; gy += vy; gz += vz;
            gw[3 * j] -= vx; gw[3 * j + 1] -= vy; gw[3 * j + 2] -= vz;
        }
        gw[3 * i] += gx; gw[3 * i + 1] += gy; gw[3 * i + 2] += gz;
    }
}

#endif /* BGK_SOLVENT_TERMS_H */
