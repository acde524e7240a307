// Radial profiles and spherical-overdensity masses on the host (definitions: ops/profiles.py): the reference
// configuration of hip/profiles.hip. A sorted cell list on the grid of sphx/pairstats.hpp, OpenMP over the centres;
// per centre the hits of its 18 slots in emission order (sphx/profiles.hpp), a stable sort by key, then the sums and
// the crossing search along the sorted hits.
#include <algorithm>
#include <cmath>
#include <string>
#include <utility>
#include <vector>

#include "cpu_api.hpp"

// no fused multiply-adds: every product of the hit arithmetic is rounded on its own, as on the device
#pragma GCC optimize("fp-contract=off")

namespace sphx::cpu
{

void radialProfiles(int64_t C, const double* cxyz, const double* vc, int64_t np, const double* x, const double* y,
                    const double* z, const uint8_t* select, const double* m, const double* vx, const double* vy,
                    const double* vz, const double* u, const Box& box, const FofGrid& g, const ProfileTables& T, int nt,
                    const double* rho, int64_t* count, double* sums, double* soR, double* soM, int64_t* soN,
                    uint8_t* soTrunc, int64_t* hits)
{
    if (np > kFofMaxN) throw std::invalid_argument("profiles: more than 2^30 particles");
    if (C > kProfileMaxCentres) throw std::invalid_argument("profiles: more than 2^24 centres");
    if (nt < 0 || nt > kProfileMaxThresholds) throw std::invalid_argument("profiles: at most 8 thresholds");
    std::vector<std::pair<int64_t, int32_t>> order; // (cell key, particle)
    order.reserve(np);
    for (int64_t i = 0; i < np; ++i)
    {
        int c[3];
        float f;
        if ((select && !select[i]) || !fofCell(g, 0, x[i], c[0], f) || !fofCell(g, 1, y[i], c[1], f) ||
            !fofCell(g, 2, z[i], c[2], f))
            continue;
        order.emplace_back(fofKey(g, c[0], c[1], c[2]), int32_t(i));
    }
    std::sort(order.begin(), order.end());
    const int64_t ns = int64_t(order.size());
    std::vector<int64_t> cellKey;
    std::vector<int32_t> cellStart;
    for (int64_t p = 0; p < ns; ++p)
        if (p == 0 || order[p].first != order[p - 1].first)
        {
            cellKey.push_back(order[p].first);
            cellStart.push_back(int32_t(p));
        }
    cellStart.push_back(int32_t(ns));

    const int nb = T.nb;
    int64_t total = 0;
#pragma omp parallel
    {
        std::vector<std::pair<float, int32_t>> hit; // (key, particle)
#pragma omp for schedule(dynamic, 4)
        for (int64_t c = 0; c < C; ++c)
        {
            const double cX = cxyz[3 * c], cY = cxyz[3 * c + 1], cZ = cxyz[3 * c + 2];
            const ProfileCentre r = profileCentre(g, cX, cY, cZ);
            hit.clear();
            for (int slot = 0; slot < kProfileSlots; ++slot)
            {
                int64_t kLo, kHi;
                int dy, dz;
                if (!profileSlot(g, r.cx, r.cy, r.cz, slot, kLo, kHi, dy, dz)) continue;
                const int32_t p0 = cellStart[std::lower_bound(cellKey.begin(), cellKey.end(), kLo) - cellKey.begin()];
                const int32_t p1 =
                    cellStart[std::lower_bound(cellKey.begin(), cellKey.end(), kHi + 1) - cellKey.begin()];
                for (int32_t p = p0; p < p1; ++p)
                {
                    const int32_t j = order[p].second;
                    double d[3], d2;
                    pairSeparation(cX, cY, cZ, x[j], y[j], z[j], box, d, d2);
                    const float k = float(d2);
                    if (k < T.E[nb]) hit.emplace_back(k, j);
                }
            }
            std::stable_sort(hit.begin(), hit.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
            const int64_t nh = int64_t(hit.size());
            hits[c]          = nh;
#pragma omp atomic
            total += nh;

            double best[kProfileMaxThresholds][2];
            int64_t bestN[kProfileMaxThresholds];
            for (int t = 0; t < nt; ++t)
                best[t][0] = best[t][1] = std::nan(""), bestN[t] = 0;
            double M = 0.0;
            for (int64_t q = 0; q < nh; ++q)
            {
                const float k   = hit[q].first;
                const int32_t j = hit[q].second;
                M += m[j];
                const int bin = profileBin(T.E, nb, k);
                if (bin >= 0)
                {
                    const int64_t o = c * nb + bin;
                    count[o] += 1;
                    sums[o] += m[j];
                    if (vx)
                    {
                        double d[3], d2, t[3];
                        pairSeparation(cX, cY, cZ, x[j], y[j], z[j], box, d, d2);
                        profileVelocityTerms(m[j], d, d2, vx[j] - (vc ? vc[3 * c] : 0.0),
                                             vy[j] - (vc ? vc[3 * c + 1] : 0.0), vz[j] - (vc ? vc[3 * c + 2] : 0.0), t);
                        for (int a = 0; a < 3; ++a)
                            sums[(1 + a) * C * nb + o] += t[a];
                    }
                    if (u) sums[4 * C * nb + o] += m[j] * u[j];
                }
                if (q + 1 < nh && hit[q + 1].first == k) continue; // inside a tie run
                for (int t = 0; t < nt; ++t)
                    if (M >= profileSphereMass(rho[t], k))
                        best[t][0] = profileRadius(k), best[t][1] = M, bestN[t] = q + 1;
            }
            for (int t = 0; t < nt; ++t)
            {
                soR[c * nt + t]     = best[t][0];
                soM[c * nt + t]     = best[t][1];
                soN[c * nt + t]     = bestN[t];
                soTrunc[c * nt + t] = bestN[t] == nh && nh > 0 ? 1 : 0;
            }
        }
    }
    if (total > kProfileMaxHits)
        throw std::invalid_argument("profiles: " + std::to_string(total) + " hits, more than 2^31 - 1");
}

} // namespace sphx::cpu
