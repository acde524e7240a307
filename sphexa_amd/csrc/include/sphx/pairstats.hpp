/*! Pair statistics (pair counts per radial bin, weighted counts, velocity structure-function sums): the geometry, the
 *  bin tables, the per-pair fp64 arithmetic and the fixed-point quanta shared by the host path
 *  (cpu/pairstats_cpu.cpp) and the gfx950 kernels (hip/pairstats.hip). Definitions: ops/pairstats.py.
 *
 *  Cells. The grid is a FofGrid (sphx/fof.hpp: cell keys, half-stencil runs, range search are reused as they are) built
 *  by makePairGrid: every cell edge is at least r_max (1 + 2^-20), so two particles whose cell coordinates differ by 2
 *  or more on any axis are farther apart than r_max whatever the rounding of the cell coordinate, and the reach of the
 *  stencil is one cell (R = 1). A periodic axis is tiled exactly and needs at least 3 cells (r_max <= L / 3, less the
 *  2^-20): the 27 stencil cells are then distinct and the image that the cell offset names is the only one inside
 *  r_max. With R = 1 the 13 cells of the half stencil are 5 contiguous key runs (x is the fastest key digit): the next
 *  cell of the own row, and the three cells of the rows (dy, dz) = (1, 0), (-1, 1), (0, 1), (1, 1).
 *
 *  fp32 filter. The device forms d^2 in fp32 from cell-relative coordinates in length units. Each component is off by
 *  less than 2^-22 of the cell edge (two roundings of a position inside its cell, one of the difference, one of the
 *  shifted sum), the vector by less than delta = 2^-20 e_max, so |d2_f32 - d2| < 2 d delta + delta^2 + 2^-22 d2. An
 *  edge E = e_k^2 is decided in fp32 outside E -+ band_k, band_k = 2 e_k delta + delta^2 + 2^-15 E; inside it the pair
 *  is evaluated again from the fp64 coordinates. The bins are therefore exactly those of the fp64 definition.
 */
#pragma once

#include <cmath>
#include <limits>

#include "fof.hpp"

namespace sphx
{

constexpr int kPairMaxBins   = 64;
constexpr int kPairChannels  = 6; // count, ww, dl1, dl2, dl3, dv2: the rows of the int64 result
constexpr int kPairWeights   = 1; // channel-set bits
constexpr int kPairVelocity  = 2;

//! @p ext = [min x, max x, min y, max y, min z, max z] of the particles (read for open axes only)
inline FofGrid makePairGrid(const Box& box, double rmax, const double* ext)
{
    if (!(rmax > 0.0) || !(rmax < 1e300)) throw std::invalid_argument("pairstats: the largest radius must be positive");
    FofGrid g;
    g.b               = rmax;
    const double eMin = rmax * (1.0 + 9.5367431640625e-7);
    for (int a = 0; a < 3; ++a)
    {
        g.per[a] = box.periodic(a);
        g.R[a]   = 1;
        double nc;
        if (g.per[a])
        {
            g.lo[a] = box.lo[a];
            nc      = std::floor(box.len(a) / eMin);
            if (!(nc >= 3.0))
                throw std::invalid_argument("pairstats: a periodic axis is shorter than 3 cells (r_max > L / 3)");
            g.e[a] = box.len(a) / nc;
        }
        else
        {
            if (!(ext[2 * a + 1] - ext[2 * a] >= 0.0) || !(ext[2 * a + 1] - ext[2 * a] < 1e300))
                throw std::invalid_argument("pairstats: the particle coordinates are not finite");
            g.lo[a] = ext[2 * a];
            nc      = std::floor((ext[2 * a + 1] - ext[2 * a]) / eMin) + 1.0;
            g.e[a]  = eMin;
        }
        if (nc > double(kFofMaxCells))
            throw std::invalid_argument("pairstats: more than 2^21 cells on an axis (r_max too short for the box)");
        g.n[a] = int(nc);
    }
    return g;
}

//! squared edges in fp64 and the fp32 tables of the device's filter and 6-step bin search
struct PairTables
{
    int nb;
    double e2[kPairMaxBins + 1];
    float search[kPairMaxBins]; // e2[1 .. nb - 1], then +inf: the bin is the number of entries <= d2
    float safeLo[kPairMaxBins]; // bin k is certain for safeLo[k] < d2_f32 < safeHi[k]
    float safeHi[kPairMaxBins];
    float cutLo, cutHi;         // candidates outside [cutLo, cutHi) are certainly outside [e_0, e_nb)
};

inline PairTables makePairTables(const double* edges, int nb, const FofGrid& g)
{
    if (nb < 1 || nb > kPairMaxBins) throw std::invalid_argument("pairstats: between 1 and 64 bins");
    if (!(edges[0] >= 0.0)) throw std::invalid_argument("pairstats: the first edge must not be negative");
    for (int k = 0; k < nb; ++k)
        if (!(edges[k] < edges[k + 1])) throw std::invalid_argument("pairstats: the edges must ascend");
    PairTables t;
    t.nb               = nb;
    const double eMax  = std::fmax(g.e[0], std::fmax(g.e[1], g.e[2]));
    const double delta = eMax * 9.5367431640625e-7;
    double band[kPairMaxBins + 1];
    for (int k = 0; k <= nb; ++k)
    {
        t.e2[k] = edges[k] * edges[k];
        band[k] = 2.0 * edges[k] * delta + delta * delta + t.e2[k] * 3.0517578125e-5;
    }
    for (int k = 0; k < kPairMaxBins; ++k)
    {
        t.search[k] = k + 1 < nb ? float(t.e2[k + 1]) : std::numeric_limits<float>::infinity();
        t.safeLo[k] = k < nb ? float(t.e2[k] + band[k]) : std::numeric_limits<float>::infinity();
        t.safeHi[k] = k < nb ? float(t.e2[k + 1] - band[k + 1]) : 0.0f;
    }
    t.cutLo = float(t.e2[0] - band[0]);
    t.cutHi = float(t.e2[nb] + band[nb]);
    return t;
}

//! @brief d = minimg(r_j - r_i) and d2 = (dx dx + dy dy) + dz dz, every product rounded on its own
SPHX_HD void pairSeparation(double xi, double yi, double zi, double xj, double yj, double zj, const Box& box,
                            double d[3], double& d2)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    d[0] = fofMinImage(xj - xi, box, 0);
    d[1] = fofMinImage(yj - yi, box, 1);
    d[2] = fofMinImage(zj - zi, box, 2);
    const double xx = d[0] * d[0], yy = d[1] * d[1], zz = d[2] * d[2];
    d2 = (xx + yy) + zz;
}

//! @brief bin k with e2[k] <= d2 < e2[k + 1], or -1
SPHX_HD int pairBin(const double* e2, int nb, double d2)
{
    if (!(d2 >= e2[0]) || !(d2 < e2[nb])) return -1;
    int lo = 0, hi = nb;
    while (hi - lo > 1)
    {
        const int mid = (lo + hi) >> 1;
        if (e2[mid] <= d2) lo = mid;
        else hi = mid;
    }
    return lo;
}

//! @brief the velocity terms of a pair: t = {u, u^2, u^3, dv . dv}, u = (dv . d) / sqrt(d2), 0 for d2 == 0
SPHX_HD void pairVelocityTerms(const double d[3], double d2, double dvx, double dvy, double dvz, double t[4])
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double ax = dvx * d[0], ay = dvy * d[1], az = dvz * d[2];
    const double dot = (ax + ay) + az;
    const double u   = d2 > 0.0 ? dot / sqrt(d2) : 0.0;
    const double uu  = u * u;
    const double xx = dvx * dvx, yy = dvy * dvy, zz = dvz * dvz;
    t[0] = u;
    t[1] = uu;
    t[2] = uu * u;
    t[3] = (xx + yy) + zz;
}

//! @brief a term as a multiple of its quantum (invq = 1 / q is a power of two: the product is exact)
SPHX_HD long long pairQuantise(double t, double invq) { return llrint(t * invq); }

//! smallest power of two >= v (1 for v == 0: every term is 0 then)
inline double pairPow2Ceil(double v)
{
    if (!(v > 0.0)) return 1.0;
    int e;
    const double m = std::frexp(v, &e);
    return std::ldexp(1.0, m == 0.5 ? e - 1 : e);
}

/*! @brief the quanta q[0 .. 4] of ww, dl1, dl2, dl3, dv2 for a bound @p pBound on the number of pairs in a bin:
 *         q_c = B_c Pp 2^-62, Pp and B_c the smallest powers of two >= pBound and >= the bound of one term (W^2; D,
 *         D^2, D^3, D^2 with D^2 = sum of the squared velocity ranges @p vrange). No sum of Pp terms reaches 2^63. */
inline void pairQuanta(double W, const double* vrange, int64_t pBound, double* q)
{
    if (!(W >= 0.0) || !(W < 1e150)) throw std::invalid_argument("pairstats: the weights are not finite");
    const double D2 = vrange[0] * vrange[0] + vrange[1] * vrange[1] + vrange[2] * vrange[2];
    if (!(D2 >= 0.0) || !(D2 < 1e100)) throw std::invalid_argument("pairstats: the velocities are not finite");
    const double D    = std::sqrt(D2);
    const double B[5] = {W * W, D, D2, D2 * D, D2};
    const double Pp   = pairPow2Ceil(double(pBound < 1 ? 1 : pBound));
    for (int c = 0; c < 5; ++c)
        q[c] = std::ldexp(pairPow2Ceil(B[c]) * Pp, -62);
}

} // namespace sphx
