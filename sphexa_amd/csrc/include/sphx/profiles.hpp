/*! Radial profiles and spherical-overdensity masses about many centres: the geometry, the keys, the per-hit fp64
 *  arithmetic and the crossing rule shared by the host path (cpu/profiles_cpu.cpp) and the gfx950 kernels
 *  (hip/profiles.hip). Definitions: ops/profiles.py.
 *
 *  Cells. The grid is makePairGrid's (sphx/pairstats.hpp): cell edges of at least r_max (1 + 2^-20), stencil reach one
 *  cell, a periodic axis tiled exactly with at least 3 cells. A centre has a cell of its own, found like a particle's
 *  but not clamped on an open axis: a centre outside the particles' extent keeps the cell it would have (down to -2 and
 *  up to n + 1, beyond which its stencil is empty anyway). Its 27 stencil cells are 9 rows (dy, dz) of 3 cells along x,
 *  the fastest key digit: a row is one contiguous key range, or two pieces where it wraps around a periodic x axis. So
 *  a centre has kProfileSlots = 18 slots, slot = 2 row + piece, row = 3 (dz + 1) + (dy + 1), most of the second pieces
 *  empty. The emission order of a centre's hits is slot by slot, ascending sorted position inside a slot.
 *
 *  Key. d = minimg(r_j - c) and d2 as pairSeparation forms them; the key of the pair is k = float(d2). E_i =
 *  float(e_i e_i); a hit has k < E_nb, bin i holds E_i <= k < E_{i+1}. Membership is decided on the keys alone, so the
 *  two paths and a dense numpy evaluation agree bit for bit. The device drops a candidate in fp32 only where its
 *  cell-relative d2 is at or above PairTables::cutHi = e_nb^2 + band_nb: the band's 2^-15 E covers the filter's error
 *  (2^-22 d2 and the two delta terms) and the 2^-24 E between E_nb and e_nb^2 many times over.
 */
#pragma once

#include "pairstats.hpp"

namespace sphx
{

constexpr int kProfileMaxBins       = kPairMaxBins;
constexpr int kProfileMaxThresholds = 8;
constexpr int kProfileSlots         = 18;
constexpr int kProfileChannels      = 6; // rows of a partial: count, mass, mvr, mvr2, mv2, mu
constexpr int64_t kProfileMaxCentres = int64_t(1) << 24;
constexpr int64_t kProfileMaxHits    = (int64_t(1) << 31) - 1;
constexpr double kFourPiThird        = 4.18879020478639098;

//! a centre's cell and its position inside it in cell edges; cx < -2: the centre is not finite, no slot holds anything
struct ProfileCentre
{
    float fx, fy, fz;
    int cx, cy, cz;
};

//! @brief cell coordinate of the centre coordinate v on axis a (not clamped on an open axis) and the position inside
SPHX_HD bool profileCell(const FofGrid& g, int a, double v, int& c, float& f)
{
    const double u = (v - g.lo[a]) / g.e[a];
    if (!(fabs(u) < 4.0e15)) return false;
    const double fl = floor(u);
    f               = float(u - fl);
    long long ci    = (long long)fl;
    if (g.per[a])
    {
        ci %= g.n[a];
        if (ci < 0) ci += g.n[a];
    }
    else { ci = ci < -2 ? -2 : (ci > g.n[a] + 1 ? g.n[a] + 1 : ci); }
    c = int(ci);
    return true;
}

SPHX_HD ProfileCentre profileCentre(const FofGrid& g, double x, double y, double z)
{
    ProfileCentre c{0.f, 0.f, 0.f, -3, 0, 0};
    int cx, cy, cz;
    if (profileCell(g, 0, x, cx, c.fx) && profileCell(g, 1, y, cy, c.fy) && profileCell(g, 2, z, cz, c.fz))
        c.cx = cx, c.cy = cy, c.cz = cz;
    return c;
}

//! @brief the cell keys [kLo, kHi] of slot @p slot of a centre in cell (cx, cy, cz) and the row offset; false: empty
SPHX_HD bool profileSlot(const FofGrid& g, int cx, int cy, int cz, int slot, int64_t& kLo, int64_t& kHi, int& dy,
                         int& dz)
{
    const int row = slot >> 1, piece = slot & 1;
    dy = row % 3 - 1;
    dz = row / 3 - 1;
    if (cx < -2) return false;
    int ry = cy + dy, rz = cz + dz;
    if (g.per[1]) ry = ry < 0 ? ry + g.n[1] : (ry >= g.n[1] ? ry - g.n[1] : ry);
    else if (ry < 0 || ry >= g.n[1]) return false;
    if (g.per[2]) rz = rz < 0 ? rz + g.n[2] : (rz >= g.n[2] ? rz - g.n[2] : rz);
    else if (rz < 0 || rz >= g.n[2]) return false;
    const int n = g.n[0], a = cx - 1, b = cx + 1;
    int xa, xb;
    if (!g.per[0])
    {
        if (piece) return false;
        xa = a < 0 ? 0 : a;
        xb = b >= n ? n - 1 : b;
    }
    else if (a < 0)
    {
        xa = piece ? 0 : a + n;
        xb = piece ? b : n - 1;
    }
    else if (b >= n)
    {
        xa = piece ? 0 : a;
        xb = piece ? b - n : n - 1;
    }
    else
    {
        if (piece) return false;
        xa = a;
        xb = b;
    }
    if (xa > xb) return false;
    const int64_t rowBase = fofKey(g, 0, ry, rz);
    kLo = rowBase + xa;
    kHi = rowBase + xb;
    return true;
}

//! the squared edges as keys, and the fp32 cut of the device's filter
struct ProfileTables
{
    int nb;
    float E[kProfileMaxBins + 1];
    float cutHi;
};

inline ProfileTables makeProfileTables(const double* edges, int nb, const FofGrid& g)
{
    const PairTables p = makePairTables(edges, nb, g); // (checks the edges)
    ProfileTables t;
    t.nb = nb;
    for (int i = 0; i <= kProfileMaxBins; ++i)
        t.E[i] = float(p.e2[i < nb ? i : nb]);
    t.cutHi = p.cutHi;
    return t;
}

//! @brief bin i with E[i] <= k < E[i + 1], -1 below E[0]; k < E[nb] is the caller's (it is a hit)
SPHX_HD int profileBin(const float* E, int nb, float k)
{
    if (!(k >= E[0])) return -1;
    int lo = 0, hi = nb;
    while (hi - lo > 1)
    {
        const int mid = (lo + hi) >> 1;
        if (E[mid] <= k) lo = mid;
        else hi = mid;
    }
    return lo;
}

//! @brief the terms of a hit: t = {m w_r, m w_r^2, m w.w}, w_r = ((wx dx + wy dy) + wz dz) / sqrt(d2), 0 for d2 == 0;
//!        every product rounded on its own
SPHX_HD void profileVelocityTerms(double m, const double d[3], double d2, double wx, double wy, double wz, double t[3])
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double ax = wx * d[0], ay = wy * d[1], az = wz * d[2];
    const double dot = (ax + ay) + az;
    const double wr  = d2 > 0.0 ? dot / sqrt(d2) : 0.0;
    const double xx = wx * wx, yy = wy * wy, zz = wz * wz;
    const double mwr = m * wr;
    t[0] = mwr;
    t[1] = mwr * wr;
    t[2] = m * ((xx + yy) + zz);
}

//! @brief r_q of a key and the mass a sphere of that radius holds at density rho: ((4 pi / 3) rho) ((r r) r)
SPHX_HD double profileRadius(float k) { return sqrt(double(k)); }

SPHX_HD double profileSphereMass(double rho, float k)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double r  = profileRadius(k);
    const double rr = r * r;
    return (kFourPiThird * rho) * (rr * r);
}

} // namespace sphx
