// Bound groups on the host (definitions: sphx/groups.hpp, ops/groups.py): the members in catalogue order with their
// fp32-rounded offsets, the self-potential as an ordered fp64 sum over the group's bound members, and the unbinding
// loop with the summation order of the device (pieces of kGroupPiece bound members, added in piece order). OpenMP
// over the members. The gfx950 path is hip/groups.hip; both yield the same bound sets wherever no energy lies within
// the device's error of zero.
#include <algorithm>
#include <cmath>
#include <limits>
#include <utility>
#include <vector>

#include "cpu_api.hpp"

// no fused multiply-adds: every product is rounded on its own, as on the device
#pragma GCC optimize("fp-contract=off")

namespace sphx::cpu
{

namespace
{

//! the sums of the members [b0, b0 + c) in the fixed order: pieces of kGroupPiece, added in piece order
template<int N, class F>
void pieceSums(int64_t b0, int64_t c, double (&acc)[N], F&& term)
{
    for (int i = 0; i < N; ++i)
        acc[i] = 0.0;
    for (int64_t p0 = 0; p0 < c; p0 += kGroupPiece)
    {
        double ps[N];
        for (int i = 0; i < N; ++i)
            ps[i] = 0.0;
        for (int64_t p = p0; p < std::min(p0 + kGroupPiece, c); ++p)
            term(b0 + p, ps);
        for (int i = 0; i < N; ++i)
            acc[i] += ps[i];
    }
}

} // namespace

BoundGroups boundGroups(int64_t n, const int32_t* label, const double* x, const double* y, const double* z,
                        const double* m, const double* vx, const double* vy, const double* vz, const double* u,
                        const Box& box, double eps, double Gc, int64_t minMembers, int maxIter, uint8_t* bound,
                        double* phiOut)
{
    if (n > kGroupMaxN) throw std::invalid_argument("groups: more than 2^30 particles");
    if (!(eps > 0.0) || maxIter < 0) throw std::invalid_argument("groups: eps > 0 and max_iter >= 0");
    std::vector<std::pair<int32_t, int32_t>> order; // (label, particle)
    for (int64_t i = 0; i < n; ++i)
    {
        bound[i]  = 0;
        phiOut[i] = std::numeric_limits<double>::quiet_NaN();
        if (label[i] >= 0) order.emplace_back(label[i], int32_t(i));
    }
    std::sort(order.begin(), order.end());
    struct Group
    {
        int64_t count, start;
        int32_t label;
    };
    std::vector<Group> groups;
    for (int64_t p = 0, q; p < int64_t(order.size()); p = q)
    {
        for (q = p + 1; q < int64_t(order.size()) && order[q].first == order[p].first; ++q) {}
        if (q - p >= minMembers) groups.push_back({q - p, p, order[p].first});
    }
    std::sort(groups.begin(), groups.end(), [](const Group& a, const Group& b)
              { return a.count != b.count ? a.count > b.count : a.label < b.label; });
    const int64_t G = int64_t(groups.size());

    // the compact member arrays, catalogue order
    std::vector<float> dx, dy, dz;
    std::vector<int32_t> idx, grp;
    std::vector<int64_t> start(G + 1, 0);
    for (int64_t k = 0; k < G; ++k)
    {
        const int32_t r = order[groups[k].start].second;
        for (int64_t p = 0; p < groups[k].count; ++p)
        {
            const int32_t j = order[groups[k].start + p].second;
            dx.push_back(groupOffset(x[j], x[r], box, 0));
            dy.push_back(groupOffset(y[j], y[r], box, 1));
            dz.push_back(groupOffset(z[j], z[r], box, 2));
            idx.push_back(j);
            grp.push_back(int32_t(k));
        }
        start[k + 1] = start[k] + groups[k].count;
    }

    BoundGroups out;
    out.iterations = 0;
    std::vector<double> phi, e, V(4 * G, 0.0);
    const double eps2 = eps * eps;
    for (;;)
    {
        const int64_t M = int64_t(idx.size());
        phi.assign(M, 0.0);
        e.assign(M, 0.0);
#pragma omp parallel for schedule(dynamic, 64)
        for (int64_t q = 0; q < M; ++q)
        {
            const int64_t k = grp[q];
            const double ax = dx[q], ay = dy[q], az = dz[q];
            double s = 0.0;
            for (int64_t p = start[k]; p < start[k + 1]; ++p)
            {
                if (p == q) continue; // by member index, not by distance
                const double tx = ax - dx[p], ty = ay - dy[p], tz = az - dz[p];
                s += m[idx[p]] / std::sqrt(((tx * tx + ty * ty) + tz * tz) + eps2);
            }
            phi[q] = -Gc * s;
        }
#pragma omp parallel for schedule(dynamic, 16)
        for (int64_t k = 0; k < G; ++k)
        {
            double acc[4];
            pieceSums(start[k], start[k + 1] - start[k], acc,
                      [&](int64_t q, double(&ps)[4])
                      {
                          const int32_t j = idx[q];
                          ps[0] += m[j];
                          ps[1] += m[j] * vx[j];
                          ps[2] += m[j] * vy[j];
                          ps[3] += m[j] * vz[j];
                      });
            V[4 * k] = acc[0];
            for (int a = 0; a < 3; ++a)
                V[4 * k + 1 + a] = start[k + 1] > start[k] ? acc[1 + a] / acc[0] : 0.0;
        }
#pragma omp parallel for schedule(static)
        for (int64_t q = 0; q < M; ++q)
        {
            const int32_t j = idx[q];
            e[q] = groupEnergy(vx[j], vy[j], vz[j], V.data() + 4 * grp[q] + 1, u ? u[j] : 0.0, phi[q]);
        }
        if (out.iterations == maxIter) break;
        ++out.iterations;

        // removal: e > 0 leaves, a group below minMembers is dissolved; a stable compaction
        std::vector<int64_t> kept(G, 0);
        for (int64_t q = 0; q < M; ++q)
            if (!(e[q] > 0.0)) ++kept[grp[q]];
        int64_t w = 0;
        for (int64_t q = 0; q < M; ++q)
        {
            if (e[q] > 0.0 || kept[grp[q]] < minMembers) continue;
            dx[w] = dx[q], dy[w] = dy[q], dz[w] = dz[q], idx[w] = idx[q], grp[w] = grp[q];
            ++w;
        }
        if (w == M) break;
        dx.resize(w), dy.resize(w), dz.resize(w), idx.resize(w), grp.resize(w);
        for (int64_t k = 0; k < G; ++k)
            start[k + 1] = start[k] + (kept[k] >= minMembers ? kept[k] : 0);
    }

    out.boundCount.resize(G);
    out.sums.resize(10 * G);
    out.centreIndex.resize(G);
    out.mostBound.resize(G);
    const double nan = std::numeric_limits<double>::quiet_NaN();
#pragma omp parallel for schedule(dynamic, 16)
    for (int64_t k = 0; k < G; ++k)
    {
        const int64_t b0 = start[k], c = start[k + 1] - start[k];
        const double* Vk = V.data() + 4 * k + 1;
        double acc[4];
        pieceSums(b0, c, acc,
                  [&](int64_t q, double(&ps)[4])
                  {
                      const int32_t j = idx[q];
                      const double wx = vx[j] - Vk[0], wy = vy[j] - Vk[1], wz = vz[j] - Vk[2];
                      const double xx = wx * wx, yy = wy * wy, zz = wz * wz;
                      ps[0] += m[j];
                      ps[1] += 0.5 * m[j] * ((xx + yy) + zz);
                      if (u) ps[2] += m[j] * u[j];
                      ps[3] += m[j] * phi[q];
                  });
        int64_t qP = -1, qE = -1;
        for (int64_t q = b0; q < b0 + c; ++q) // ties: the smallest index stays
        {
            if (qP < 0 || phi[q] < phi[qP]) qP = q;
            if (qE < 0 || e[q] < e[qE]) qE = q;
        }
        double* o         = out.sums.data() + 10 * k;
        out.boundCount[k] = c;
        o[0]              = acc[0];
        for (int a = 0; a < 3; ++a)
            o[1 + a] = c > 0 ? Vk[a] : nan;
        o[4] = acc[1], o[5] = acc[2], o[6] = 0.5 * acc[3];
        double cx = nan, cy = nan, cz = nan;
        if (c > 0)
        {
            cx = x[idx[qP]], cy = y[idx[qP]], cz = z[idx[qP]];
            putInBox(cx, cy, cz, box);
        }
        o[7] = cx, o[8] = cy, o[9] = cz;
        out.centreIndex[k] = c > 0 ? idx[qP] : -1;
        out.mostBound[k]   = c > 0 ? idx[qE] : -1;
    }
    for (size_t q = 0; q < idx.size(); ++q)
    {
        bound[idx[q]]  = 1;
        phiOut[idx[q]] = phi[q];
    }
    return out;
}

} // namespace sphx::cpu
