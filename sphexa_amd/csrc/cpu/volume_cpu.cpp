// SPH volumes on the host: the definition of ops/volume.py summed in fp64, OpenMP over the grid's rows (z, y). Every
// row visits every particle (short, not fast); the gfx950 path is hip/volume.hip.
#include <algorithm>
#include <cmath>
#include <vector>

#include "cpu_api.hpp"

// no fused multiply-adds here: q^2 near the support's edge decides the kernel value's last digits, and the fp64 oracle
// of tests/test_volume.py forms it from separately rounded products
#pragma GCC optimize("fp-contract=off")

namespace sphx::cpu
{

void sphVolume(int64_t first, int64_t last, int64_t n, const double* x, const double* y, const double* z,
               const float* h, const float* w, int C, const VolumeView& V, double* out)
{
    const double halfPi = 1.5707963267948966;
    const int nx = V.n[0], ny = V.n[1], nz = V.n[2];
    const int mx = V.per[0] ? 1 : 0, my = V.per[1] ? 1 : 0, mz = V.per[2] ? 1 : 0;
#pragma omp parallel for schedule(dynamic, 4)
    for (int row = 0; row < nz * ny; ++row)
    {
        // voxel space, as the records of the gfx950 path: centres (p - origin) / edge and 1/h per particle,
        // separations scaled by edge / h
        const double gy = row % ny + 0.5, gz = row / ny + 0.5;
        std::vector<double> line(size_t(C) * nx, 0.0);
        for (int64_t j = first; j < last; ++j)
        {
            const double hj = std::max(double(h[j]), V.hMin);
            const double ih = 1.0 / hj;
            const double cx0 = (x[j] - V.lo[0]) / V.d[0], cy0 = (y[j] - V.lo[1]) / V.d[1],
                         cz0 = (z[j] - V.lo[2]) / V.d[2];
            const double ax = V.d[0] * ih, ay = V.d[1] * ih, az = V.d[2] * ih;
            const double val0 = ih * ih * ih;
            for (int sz = -mz; sz <= mz; ++sz)
            {
                const double dw = (gz - (cz0 + sz * V.L[2] / V.d[2])) * az;
                if (!(dw * dw < 4.0)) continue;
                for (int sy = -my; sy <= my; ++sy)
                {
                    const double dv = (gy - (cy0 + sy * V.L[1] / V.d[1])) * ay;
                    if (!(dv * dv < 4.0)) continue;
                    for (int sx = -mx; sx <= mx; ++sx)
                    {
                        const double cu   = cx0 + sx * V.L[0] / V.d[0];
                        const double half = 2.0 / ax + 1.0; // voxels, one to spare: q2 < 4 decides
                        const int k0 = int(std::max(0.0, std::ceil(cu - half))),
                                  k1 = int(std::min(double(nx - 1), std::floor(cu + half)));
                        for (int k = k0; k <= k1; ++k)
                        {
                            const double du = ((k + 0.5) - cu) * ax;
                            const double q2 = du * du + dv * dv + dw * dw;
                            if (!(q2 < 4.0)) continue;
                            const double a   = halfPi * std::sqrt(q2);
                            const double val = V.K * std::pow(a > 0 ? std::sin(a) / a : 1.0, V.sinc) * val0;
                            for (int c = 0; c < C; ++c)
                                line[size_t(c) * nx + k] += double(w[size_t(c) * n + j]) * val;
                        }
                    }
                }
            }
        }
        for (int c = 0; c < C; ++c)
            std::copy_n(line.data() + size_t(c) * nx, nx, out + (size_t(c) * nz * ny + row) * nx);
    }
}

} // namespace sphx::cpu
