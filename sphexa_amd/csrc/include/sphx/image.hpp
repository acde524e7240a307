/*! SPH images (slices, column projections, opacity renderings): the view shared by the OpenMP path
 *  (cpu/image_cpu.cpp) and the gfx950 kernels (hip/image.hip). Definitions: ops/image.py.
 */
#pragma once

#include <cmath>
#include <cstdint>
#include <stdexcept>

#include "annotation.hpp"
#include "box.hpp"

namespace sphx
{

constexpr int kImageTableLen = 16385; // samples of F_n in u = q^2/4 on [0, 1] (ops/image.py TABLE_LENGTH)

//! @brief one particle as the tile kernel reads it: 32 B, 16-B aligned (two records per cache line, as SrcPos)
struct alignas(16) ImageRec
{
    float cu, cv; // centre in pixels relative to the window origin (pixel k has its centre at k + 0.5)
    float ih;     // 1 / h_eff
    float zq;     // slice: depth offset / h_eff
    float w0, w1; // channel weights (rendering: kappa m and the source value)
    float ru, rv; // half extents of the footprint in pixels (< 0: contributes nothing)
};
static_assert(sizeof(ImageRec) == 32, "ImageRec is two 16-byte chunks");

struct ImageView
{
    int proj;           // 0: slice at s0, 1: projection or rendering over [s0, s1]
    int render;         // 1: the entries of a pixel are composited in depth order (ops/image.py), not summed
    int reversed;       // rendering seen from the far side: descending depth
    int ia, iu, iv;     // view axis and the image plane's axes (cyclic order)
    int nu, nv;         // pixels
    int perA, perU, perV;
    double u0, v0;      // window origin
    double pu, pv;      // pixel sizes
    double s0, s1;
    double hMin;        // h floor as a length (0: off)
    double La, Lu, Lv;  // box lengths
    double K;           // 3-D kernel normalisation
    double n;           // sinc index
};

//! @p v = [kind (0 slice, 1 projection, 2 rendering), axis (a, or -(a + 1) for a rendering's reversed view), u0, u1,
//!        v0, v1, s0, s1, h floor in pixels, sinc index, K]
inline ImageView makeImageView(const Box& b, const double* v, int nu, int nv)
{
    ImageView V;
    const int kind = int(v[0]);
    V.proj         = kind >= 1;
    V.render       = kind == 2;
    V.reversed     = v[1] < 0;
    V.ia           = V.reversed ? -int(v[1]) - 1 : int(v[1]);
    if (kind < 0 || kind > 2 || (V.reversed && !V.render)) throw std::invalid_argument("image view: kind");
    if (V.ia < 0 || V.ia > 2 || nu < 1 || nv < 1) throw std::invalid_argument("image view: axis or resolution");
    V.iu   = (V.ia + 1) % 3;
    V.iv   = (V.ia + 2) % 3;
    V.nu   = nu;
    V.nv   = nv;
    V.perA = b.periodic(V.ia);
    V.perU = b.periodic(V.iu);
    V.perV = b.periodic(V.iv);
    V.u0   = v[2];
    V.v0   = v[4];
    V.pu   = (v[3] - v[2]) / nu;
    V.pv   = (v[5] - v[4]) / nv;
    V.s0   = v[6];
    V.s1   = v[7];
    V.hMin = v[8] * (V.pu > V.pv ? V.pu : V.pv);
    V.La   = b.len(V.ia);
    V.Lu   = b.len(V.iu);
    V.Lv   = b.len(V.iv);
    V.n    = v[9];
    V.K    = v[10];
    return V;
}

//! @brief depth test of a particle at view-axis coordinate a with smoothing length h: whether it contributes, its
//!        depth offset dz (slices, minimum image) and in-plane radius R
SPHX_HD bool imageDepth(const ImageView& V, double a, double h, double& dz, double& R)
{
    if (V.proj)
    {
        dz = 0;
        R  = 2 * h;
        return a >= V.s0 && a <= V.s1;
    }
    dz = a - V.s0;
    if (V.perA) dz -= V.La * rint(dz / V.La);
    const double r2 = 4 * h * h - dz * dz;
    R               = r2 > 0 ? sqrt(r2) : 0;
    return r2 > 0;
}

/*! @brief a rendering's depth key of a particle at view-axis coordinate a: the order-preserving uint64 image of the
 *         fp64 depth (negated for the reversed view; -0.0 and +0.0 made one first). Outside the slab (NaN included):
 *         the largest key. A stable sort of the keys by (key, index) is the compositing order. */
SPHX_HD uint64_t imageDepthKey(const ImageView& V, double a)
{
    if (!(a >= V.s0 && a <= V.s1)) return ~uint64_t(0);
    union
    {
        double d;
        uint64_t u;
    } c;
    c.d = (V.reversed ? -a : a) + 0.0;
    return c.u >> 63 ? ~c.u : c.u | (uint64_t(1) << 63);
}

} // namespace sphx
