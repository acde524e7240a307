/*! Friends-of-friends groups: the geometry and the union-find shared by the host path (cpu/fof_cpu.cpp) and the gfx950
 *  kernels (hip/fof.hip). Definitions: ops/fof.py.
 *
 *  Cells. The cell edge of every axis is at most (b / sqrt 3)(1 - 2^-20): the diagonal of a cell is shorter than the
 *  linking length b by more than any rounding of the cell coordinate, so two particles of one cell are always friends
 *  and no pair inside a cell is ever tested. A periodic axis is tiled exactly (e = L / ceil(L / e_max)), an open axis
 *  starts at the smallest coordinate. Friends in other cells lie within R = ceil(b / e) cells per axis (2, or 3 on a
 *  short periodic axis); a periodic axis needs 2 R + 1 <= n, so that the stencil's cells are distinct and the image
 *  that the cell offset names is the only one that can be a friend (|d| < (R + 1) e, every other image is farther
 *  than L - (R + 1) e >= R e >= b).
 *
 *  Stencil. Keys are linear cell indices with x fastest, so the 2 R + 1 stencil cells of a neighbouring (y, z) row
 *  are one contiguous key range. Every unordered cell pair is visited once: from cell (cx, cy, cz) the runs are the
 *  cells cx + 1 .. cx + R of its own row, then the rows (dy, 0), dy = 1 .. R, and (dy, dz), dz = 1 .. R, |dy| <= R
 *  (13 runs for R = 2). A run that wraps around a periodic x axis comes in two pieces.
 *
 *  Union-find over the occupied cells: int32 parent[], parent[i] <= i at all times, slots are only ever lowered.
 */
#pragma once

#include <stdexcept>

#include "annotation.hpp"
#include "box.hpp"

namespace sphx
{

constexpr int kFofMaxCells   = 1 << 21;     // per axis: three coordinates fit a 63-bit key
constexpr int64_t kFofMaxN   = int64_t(1) << 30;
constexpr float kFofBand     = 6.103515625e-5f; // 2^-14: fp32 d^2 / b^2 is decided outside 1 -+ band (error < 2e-6)
constexpr int kFofPiece      = 32;          // members per ordered piece of a catalogue sum

struct FofGrid
{
    double lo[3]; // origin
    double e[3];  // cell edges
    double b;     // linking length
    int n[3];     // cells per axis
    int R[3];     // stencil reach in cells
    int per[3];
};

//! @p ext = [min x, max x, min y, max y, min z, max z] of the particles (read for open axes only)
inline FofGrid makeFofGrid(const Box& box, double b, const double* ext)
{
    if (!(b > 0.0) || !(b < 1e300)) throw std::invalid_argument("fof: the linking length must be positive");
    FofGrid g;
    g.b               = b;
    const double eMax = b / 1.7320508075688772 * (1.0 - 9.5367431640625e-7);
    for (int a = 0; a < 3; ++a)
    {
        g.per[a] = box.periodic(a);
        double nc;
        if (g.per[a])
        {
            g.lo[a] = box.lo[a];
            nc      = std::ceil(box.len(a) / eMax);
            g.e[a]  = box.len(a) / nc;
        }
        else
        {
            if (!(ext[2 * a + 1] - ext[2 * a] >= 0.0) || !(ext[2 * a + 1] - ext[2 * a] < 1e300))
                throw std::invalid_argument("fof: the particle coordinates are not finite");
            g.lo[a] = ext[2 * a];
            nc      = std::floor((ext[2 * a + 1] - ext[2 * a]) / eMax) + 1.0;
            g.e[a]  = eMax;
        }
        if (!(nc >= 1.0) || nc > double(kFofMaxCells))
            throw std::invalid_argument("fof: more than 2^21 cells on an axis (linking length too short for the box)");
        g.n[a] = int(nc);
        g.R[a] = int(std::ceil(b / g.e[a] * (1.0 + 1e-6)));
        if (g.per[a] && 2 * g.R[a] + 1 > g.n[a])
            throw std::invalid_argument("fof: a periodic axis is shorter than the stencil (2 R + 1 cells)");
    }
    return g;
}

//! @brief cell coordinate of v on axis a and the position inside the cell, f in [0, 1]; false: v is not finite
SPHX_HD bool fofCell(const FofGrid& g, int a, double v, int& c, float& f)
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
    else { ci = ci < 0 ? 0 : (ci >= g.n[a] ? g.n[a] - 1 : ci); }
    c = int(ci);
    return true;
}

SPHX_HD int64_t fofKey(const FofGrid& g, int cx, int cy, int cz) { return (int64_t(cz) * g.n[1] + cy) * g.n[0] + cx; }

SPHX_HD int fofNumRuns(const FofGrid& g) { return 1 + g.R[1] + g.R[2] * (2 * g.R[1] + 1); }

struct FofRun
{
    int64_t kLo, kHi, rowBase; // key range of the piece, key of cell x = 0 of its row
    int dy, dz;                // row offset (not wrapped: the image the pair test uses)
};

/*! @brief piece @p p (0 or 1) of run @p r of the half stencil for targets in the cells [cxLo, cxHi] of row (cy, cz):
 *         run 0 is the own row (cells above cxLo), the others the rows (dy, dz) listed above. false: nothing there */
SPHX_HD bool fofRun(const FofGrid& g, int r, int p, int cxLo, int cxHi, int cy, int cz, FofRun& out)
{
    int dy = 0, dz = 0;
    if (r > 0)
    {
        int i = r - 1;
        if (i < g.R[1]) dy = i + 1;
        else
        {
            i -= g.R[1];
            dz = i / (2 * g.R[1] + 1) + 1;
            dy = i % (2 * g.R[1] + 1) - g.R[1];
        }
    }
    int ry = cy + dy, rz = cz + dz;
    if (g.per[1]) ry = ry < 0 ? ry + g.n[1] : (ry >= g.n[1] ? ry - g.n[1] : ry);
    else if (ry < 0 || ry >= g.n[1]) return false;
    if (g.per[2]) rz = rz < 0 ? rz + g.n[2] : (rz >= g.n[2] ? rz - g.n[2] : rz);
    else if (rz < 0 || rz >= g.n[2]) return false;
    const int n  = g.n[0];
    const int a  = r == 0 ? cxLo + 1 : cxLo - g.R[0];
    const int b  = cxHi + g.R[0];
    int xa, xb;
    if (!g.per[0])
    {
        if (p) return false;
        xa = a < 0 ? 0 : a;
        xb = b >= n ? n - 1 : b;
    }
    else if (b - a + 1 >= n)
    {
        if (p) return false;
        xa = 0;
        xb = n - 1;
    }
    else if (a < 0)
    {
        xa = p ? 0 : a + n;
        xb = p ? b : n - 1;
    }
    else if (b >= n)
    {
        xa = p ? 0 : a;
        xb = p ? b - n : n - 1;
    }
    else
    {
        if (p) return false;
        xa = a;
        xb = b;
    }
    if (xa > xb) return false;
    out.rowBase = fofKey(g, 0, ry, rz);
    out.kLo     = out.rowBase + xa;
    out.kHi     = out.rowBase + xb;
    out.dy      = dy;
    out.dz      = dz;
    return true;
}

//! @brief whether source cell x @p sx is in the stencil of target cell x @p tx (own row: above it only); ddx: offset
SPHX_HD bool fofInStencil(const FofGrid& g, bool ownRow, int tx, int sx, int& ddx)
{
    ddx = sx - tx;
    if (g.per[0])
    {
        if (ddx > g.R[0]) ddx -= g.n[0];
        else if (ddx < -g.R[0]) ddx += g.n[0];
    }
    return ownRow ? (ddx >= 1 && ddx <= g.R[0]) : (ddx >= -g.R[0] && ddx <= g.R[0]);
}

//! @brief fp32 pair test on a separation in units of b: 1 friends, 0 not, -1 inside the rounding band (re-test in fp64)
SPHX_HD int fofPairF32(float ux, float uy, float uz)
{
    const float d2 = ux * ux + uy * uy + uz * uz;
    return d2 <= 1.0f - kFofBand ? 1 : (d2 >= 1.0f + kFofBand ? 0 : -1);
}

//! @brief one component of the minimum image, as distanceSqPbc forms it
SPHX_HD double fofMinImage(double d, const Box& box, int a)
{
    return box.bc[a] == kPeriodic ? d - box.len(a) * rint(d * box.ilen(a)) : d;
}

//! @brief the exact pair test: minimum-image d^2 <= b^2 in fp64, every product rounded on its own (no fused
//!        multiply-add: the host and the device form the same bits)
SPHX_HD bool fofPairExact(double xi, double yi, double zi, double xj, double yj, double zj, const Box& box, double b)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double dx = fofMinImage(xi - xj, box, 0), dy = fofMinImage(yi - yj, box, 1),
                 dz = fofMinImage(zi - zj, box, 2);
    const double xx = dx * dx, yy = dy * dy, zz = dz * dz;
    return (xx + yy) + zz <= b * b;
}

// ------------------------------------------------------------------------------------------------------- union-find

SPHX_HD int fofLoad(const int* p)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
    return __atomic_load_n(p, __ATOMIC_RELAXED);
#endif
}

//! @brief *p = min(*p, v), returns the value before
SPHX_HD int fofAtomicMin(int* p, int v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return atomicMin(p, v);
#else
    int old = __atomic_load_n(p, __ATOMIC_RELAXED);
    // (every failed exchange has seen another thread lower the slot: at most old - v of them)
    while (old > v && !__atomic_compare_exchange_n(p, &old, v, true, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
    return old;
#endif
}

//! @brief root of x, read-only. parent[i] <= i and a non-root has parent[i] < i: x falls strictly, at most x steps. A
//!        stale read returns an earlier parent, which stays in x's component (fofUnion), so equal roots always mean
//!        one component; unequal roots of one component only cost a test
SPHX_HD int fofFind(const int* parent, int x)
{
    for (;;)
    {
        const int p = fofLoad(parent + x);
        if (p >= x) return x;
        x = p;
    }
}

/*! @brief joins the components of a and b. Per pass: both roots are found, the larger root's slot is lowered to the
 *         smaller root by an atomic minimum. If the slot still held its own index the larger root now hangs below the
 *         smaller one: done. Otherwise another thread had hung it below `old` in the meantime: the slot now holds
 *         min(old, lo), and what remains is to join old and lo (hi keeps an edge to one of them, the other is what
 *         this pass continues with), so no link is ever lost.
 *         Termination: old < hi (slots only hold values below their index once they are no roots) and lo < hi, so the
 *         larger root of the next pass is below hi: hi falls strictly, at most hi passes; no pass waits for another
 *         thread. */
SPHX_HD void fofUnion(int* parent, int a, int b)
{
    for (;;)
    {
        a = fofFind(parent, a);
        b = fofFind(parent, b);
        if (a == b) return;
        const int hi = a > b ? a : b, lo = a > b ? b : a;
        const int old = fofAtomicMin(parent + hi, lo);
        if (old >= hi) return;
        a = old;
        b = lo;
    }
}

} // namespace sphx
