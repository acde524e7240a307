// SPH slices, column projections and opacity renderings on the host: the definitions of ops/image.py in fp64, OpenMP
// over image rows. Every row visits every particle (short, not fast); the gfx950 path is hip/image.hip.
#include <algorithm>
#include <cmath>
#include <numeric>
#include <vector>

#include "cpu_api.hpp"

// no fused multiply-adds here: q^2 near the support's edge decides the kernel value's last digits, and the fp64 oracle
// of tests/test_image.py forms it from separately rounded products
#pragma GCC optimize("fp-contract=off")

namespace sphx::cpu
{

void sphImage(int64_t first, int64_t last, int64_t n, const double* x, const double* y, const double* z,
              const float* h, const float* w, int C, const ImageView& V, const double* table, int tableLen,
              double* out)
{
    const double* pos[3] = {x, y, z};
    const double halfPi  = 1.5707963267948966;
    const int su0 = V.perU ? -1 : 0, sv0 = V.perV ? -1 : 0;
    // rendering: the particles of the slab in compositing order, a stable sort by the depth key (ties by index);
    // every row then walks them in that order, shift codes ascending (sv outer, su inner)
    std::vector<int64_t> order;
    if (V.render)
    {
        if (C != 2) throw std::invalid_argument("sphImage: a rendering has two channels");
        order.resize(size_t(last - first));
        std::iota(order.begin(), order.end(), first);
        std::vector<uint64_t> key(order.size());
        for (size_t k = 0; k < key.size(); ++k)
            key[k] = imageDepthKey(V, pos[V.ia][first + int64_t(k)]);
        std::stable_sort(order.begin(), order.end(),
                         [&](int64_t a, int64_t b) { return key[size_t(a - first)] < key[size_t(b - first)]; });
    }
#pragma omp parallel for schedule(dynamic, 4)
    for (int py = 0; py < V.nv; ++py)
    {
        // pixel space, as the records of the gfx950 path: centres (p - origin) / pixel, 1/h and dz/h per particle,
        // separations scaled by pixel / h
        const double gy = py + 0.5;
        std::vector<double> row(size_t(C) * V.nu, 0.0);
        if (V.render) std::fill(row.begin() + V.nu, row.end(), 1.0); // (I, T) = (0, 1)
        for (int64_t t = first; t < last; ++t)
        {
            const int64_t j = V.render ? order[size_t(t - first)] : t;
            const double hj = std::max(double(h[j]), V.hMin);
            double dz, R;
            if (!imageDepth(V, pos[V.ia][j], hj, dz, R)) continue;
            const double ih = 1.0 / hj, zq = dz / hj;
            const double cu0 = (pos[V.iu][j] - V.u0) / V.pu, cv0 = (pos[V.iv][j] - V.v0) / V.pv;
            const double au = V.pu * ih, av = V.pv * ih;
            for (int sv = sv0; sv <= -sv0; ++sv)
            {
                const double dv = (gy - (cv0 + sv * V.Lv / V.pv)) * av;
                if (!(dv * dv < 4.0)) continue;
                for (int su = su0; su <= -su0; ++su)
                {
                    const double cu = cu0 + su * V.Lu / V.pu;
                    const double half = 2.0 / au + 1.0; // pixels, one to spare: q2 < 4 decides
                    const int k0 = int(std::max(0.0, std::ceil(cu - half))), k1 = int(std::min(double(V.nu - 1), std::floor(cu + half)));
                    for (int k = k0; k <= k1; ++k)
                    {
                        const double du = ((k + 0.5) - cu) * au;
                        const double q2 = du * du + dv * dv + zq * zq;
                        if (!(q2 < 4.0)) continue;
                        double val;
                        if (V.proj)
                        {
                            const double t = q2 * 0.25 * (tableLen - 1);
                            const int i    = std::min(int(t), tableLen - 2);
                            val            = (table[i] + (t - i) * (table[i + 1] - table[i])) * ih * ih;
                        }
                        else
                        {
                            const double a = halfPi * std::sqrt(q2);
                            val            = V.K * std::pow(a > 0 ? std::sin(a) / a : 1.0, V.n) * (ih * ih * ih);
                        }
                        if (V.render)
                        {
                            const double tau = double(w[j]) * val;
                            double &I = row[k], &T = row[size_t(V.nu) + k];
                            I += T * -std::expm1(-tau) * double(w[size_t(n) + j]);
                            T *= std::exp(-tau);
                            continue;
                        }
                        for (int c = 0; c < C; ++c)
                            row[size_t(c) * V.nu + k] += double(w[size_t(c) * n + j]) * val;
                    }
                }
            }
        }
        for (int c = 0; c < C; ++c)
            std::copy_n(row.data() + size_t(c) * V.nu, V.nu, out + (size_t(c) * V.nv + py) * V.nu);
    }
}

} // namespace sphx::cpu
