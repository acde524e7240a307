/*! Ewald lattice sum of a periodic cubic box: constants and math of the gfx950 kernels (csrc/hip/ewald.hip).
 *
 * Parity (behaviour): reference ryoanji/src/ryoanji/nbody/traversal_ewald_cpu.hpp:46-402. Same sum, constants and
 * meaning as the OpenMP oracle (csrc/cpu/gravity_extra_cpu.cpp: struct Ewald, computeGravityEwald): splitting
 * parameter alpha = 2/L, real-space images |n|_inf <= 2, k-vectors |n|_inf <= 5.
 *
 * The k-space sum is evaluated in factored form. With X = k_f x (k_f = 2 pi / L) and f(i, j, k) = 4 pi / V
 * exp(-k^2 / 4 alpha^2) / k^2, which depends on |i|, |j|, |k| only, the eight sign combinations of a k-vector add to
 *     sum_{+-} cos(+-iX +- jY +- kZ) = 8 cos(iX) cos(jY) cos(kZ),
 * so the 11^3 - 1 terms become 6^3 - 1 products of per-axis cos(nX), sin(nX), n = 0..5, with the multiplicities
 * (1 for n = 0, 2 otherwise) folded into the coefficient table.
 */
#pragma once

#include "annotation.hpp"

namespace sphx
{

constexpr double kEwaldAlphaL  = 2.0; //!< alpha * L
constexpr int kEwaldRealShells = 2;   //!< real-space images |n|_inf <= 2
constexpr int kEwaldKMax       = 5;   //!< k-vectors |n|_inf <= 5
constexpr int kEwaldKDim       = kEwaldKMax + 1;
constexpr int kEwaldTableSize  = kEwaldKDim * kEwaldKDim * kEwaldKDim;

constexpr double kEwaldPi = 3.14159265358979323846;

/*! @brief k-space coefficients w_i w_j w_k 4 pi / V exp(-k^2 / 4 alpha^2) / k^2 for i, j, k in [0, kEwaldKMax],
 *         w_0 = 1, w_n = 2 (the +-n pair); entry (0, 0, 0) is zero. Host, once per box length.
 */
inline void ewaldKTable(double L, double table[kEwaldTableSize])
{
    const double alpha = kEwaldAlphaL / L, a2 = alpha * alpha;
    const double V = L * L * L, kf = 2.0 * kEwaldPi / L;
    for (int i = 0; i <= kEwaldKMax; ++i)
        for (int j = 0; j <= kEwaldKMax; ++j)
            for (int k = 0; k <= kEwaldKMax; ++k)
            {
                double k2 = kf * kf * double(i * i + j * j + k * k);
                double w  = double((i ? 2 : 1) * (j ? 2 : 1) * (k ? 2 : 1));
                table[(i * kEwaldKDim + j) * kEwaldKDim + k] =
                    (i | j | k) ? w * 4.0 * kEwaldPi / V * std::exp(-k2 / (4.0 * a2)) / k2 : 0.0;
            }
}

//! @brief c[n] = cos(n X), s[n] = sin(n X), n = 0..kEwaldKMax, from one sincos and the angle-addition recurrence
SPHX_HD void ewaldHarmonics(double X, double c[kEwaldKDim], double s[kEwaldKDim])
{
    double s1, c1;
    sincos(X, &s1, &c1);
    c[0] = 1.0, s[0] = 0.0;
    for (int n = 1; n <= kEwaldKMax; ++n)
    {
        c[n] = c[n - 1] * c1 - s[n - 1] * s1;
        s[n] = s[n - 1] * c1 + c[n - 1] * s1;
    }
}

/*! @brief k-space part of psi and its gradient at x (relative to the lattice origin), added to p and g
 *
 * @param table  ewaldKTable of the box (LDS on the GPU)
 */
SPHX_HD void ewaldKSpace(const double x[3], double L, const double* table, double& p, double g[3])
{
    const double kf = 2.0 * kEwaldPi / L;
    double cx[kEwaldKDim], sx[kEwaldKDim], cy[kEwaldKDim], sy[kEwaldKDim], cz[kEwaldKDim], sz[kEwaldKDim];
    ewaldHarmonics(kf * x[0], cx, sx);
    ewaldHarmonics(kf * x[1], cy, sy);
    ewaldHarmonics(kf * x[2], cz, sz);
    double pk = 0, gx = 0, gy = 0, gz = 0;
    for (int i = 0; i <= kEwaldKMax; ++i)
        for (int j = 0; j <= kEwaldKMax; ++j)
        {
            const double* t = table + (i * kEwaldKDim + j) * kEwaldKDim;
            double A = 0, B = 0; // sum_k f cos(kZ), sum_k f k sin(kZ)
            for (int k = 0; k <= kEwaldKMax; ++k)
            {
                A += t[k] * cz[k];
                B += t[k] * double(k) * sz[k];
            }
            double cc = cx[i] * cy[j];
            pk += cc * A;
            gx += double(i) * sx[i] * cy[j] * A;
            gy += double(j) * cx[i] * sy[j] * A;
            gz += cc * B;
        }
    p += pk;
    g[0] -= kf * gx;
    g[1] -= kf * gy;
    g[2] -= kf * gz;
}

//! @brief real-space part of psi and its gradient (erfc-screened images |n|_inf <= kEwaldRealShells), added to p, g
SPHX_HD void ewaldRealSpace(const double x[3], double L, double& p, double g[3])
{
    const double alpha = kEwaldAlphaL / L, a2 = alpha * alpha;
    const double sq = 2.0 * alpha / sqrt(kEwaldPi);
    for (int i = -kEwaldRealShells; i <= kEwaldRealShells; ++i)
        for (int j = -kEwaldRealShells; j <= kEwaldRealShells; ++j)
            for (int k = -kEwaldRealShells; k <= kEwaldRealShells; ++k)
            {
                double r[3] = {x[0] + i * L, x[1] + j * L, x[2] + k * L};
                double rr2  = r[0] * r[0] + r[1] * r[1] + r[2] * r[2];
                double rr   = sqrt(rr2);
                double e    = erfc(alpha * rr) / rr;
                p += e;
                double coef = (e + sq * exp(-a2 * rr2)) / rr2;
                for (int d = 0; d < 3; ++d)
                    g[d] -= coef * r[d];
            }
}

//! @brief psi(x) = sum_n 1/|x + nL| with neutralizing background and its gradient, x not a lattice point
SPHX_HD void ewaldPsi(const double x[3], double L, const double* table, double& p, double g[3])
{
    const double alpha = kEwaldAlphaL / L;
    p = 0, g[0] = g[1] = g[2] = 0;
    ewaldRealSpace(x, L, p, g);
    ewaldKSpace(x, L, table, p, g);
    p -= kEwaldPi / (alpha * alpha * L * L * L);
}

} // namespace sphx
