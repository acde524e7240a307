/*! SPH volumes on regular 3-D grids: the view shared by the OpenMP path (cpu/volume_cpu.cpp) and the gfx950 kernels
 *  (hip/volume.hip). Definitions: ops/volume.py.
 */
#pragma once

#include <stdexcept>

#include "annotation.hpp"
#include "box.hpp"

namespace sphx
{

//! @brief one particle as the brick kernel reads it: 32 B, 16-B aligned (two records per cache line, as ImageRec)
struct alignas(16) VolumeRec
{
    float cx, cy, cz; // centre in voxels relative to the window origin (voxel k has its centre at k + 0.5)
    float ih;         // 1 / h_eff
    float w[4];       // channel weights (channels past C: 0)
};
static_assert(sizeof(VolumeRec) == 32, "VolumeRec is two 16-byte chunks");

struct VolumeView
{
    int n[3];      // voxels per axis (x, y, z)
    int per[3];    // periodic axes
    double lo[3];  // window origin
    double d[3];   // voxel edges
    double L[3];   // box lengths
    double hMin;   // h floor as a length (0: off)
    double K;      // 3-D kernel normalisation
    double sinc;   // sinc index
};

//! @p v = [lo x, y, z, hi x, y, z, h floor in voxels (of the largest edge), sinc index, K]
inline VolumeView makeVolumeView(const Box& b, const double* v, int nx, int ny, int nz)
{
    VolumeView V;
    const int n[3] = {nx, ny, nz};
    double dmax    = 0;
    for (int a = 0; a < 3; ++a)
    {
        if (n[a] < 1 || !(v[3 + a] > v[a])) throw std::invalid_argument("volume view: window or resolution");
        V.n[a]   = n[a];
        V.per[a] = b.periodic(a);
        V.lo[a]  = v[a];
        V.d[a]   = (v[3 + a] - v[a]) / n[a];
        V.L[a]   = b.len(a);
        dmax     = V.d[a] > dmax ? V.d[a] : dmax;
    }
    V.hMin = v[6] * dmax;
    V.sinc = v[7];
    V.K    = v[8];
    return V;
}

} // namespace sphx
