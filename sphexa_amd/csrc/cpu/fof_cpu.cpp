// Friends-of-friends groups on the host (definitions: ops/fof.py): a sorted cell list and the union-find of
// sphx/fof.hpp over the occupied cells, OpenMP over the cells, every pair test in fp64. The gfx950 path is hip/fof.hip;
// both walk the same cells, stencil runs and pair test, and both give the component minima as labels.
#include <algorithm>
#include <cmath>
#include <utility>
#include <vector>

#include "cpu_api.hpp"

// no fused multiply-adds: the pair test and the catalogue sums round every product on its own, as the device does
#pragma GCC optimize("fp-contract=off")

namespace sphx::cpu
{

void fofLabels(int64_t np, const double* x, const double* y, const double* z, const uint8_t* select, const Box& box,
               const FofGrid& g, int32_t* label)
{
    if (np > kFofMaxN) throw std::invalid_argument("fof: more than 2^30 particles");
    std::vector<std::pair<int64_t, int32_t>> order; // (cell key, particle): ascending particle inside a cell
    order.reserve(np);
    for (int64_t i = 0; i < np; ++i)
    {
        int c[3];
        float f;
        label[i] = -1;
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
    const int ncells = int(cellKey.size());
    cellStart.push_back(int32_t(ns));
    std::vector<int> parent(ncells);
    for (int c = 0; c < ncells; ++c)
        parent[c] = c;

    const int nRuns = fofNumRuns(g);
#pragma omp parallel for schedule(dynamic, 64)
    for (int A = 0; A < ncells; ++A)
    {
        const int64_t key = cellKey[A];
        const int cx = int(key % g.n[0]), cy = int(key / g.n[0] % g.n[1]), cz = int(key / (int64_t(g.n[0]) * g.n[1]));
        for (int r = 0; r < nRuns; ++r)
            for (int p = 0; p < 2; ++p)
            {
                FofRun run;
                if (!fofRun(g, r, p, cx, cx, cy, cz, run)) continue;
                int B = int(std::lower_bound(cellKey.begin(), cellKey.end(), run.kLo) - cellKey.begin());
                for (; B < ncells && cellKey[B] <= run.kHi; ++B)
                {
                    // one link joins two cells (a cell's particles are all friends): cells of one component are skipped
                    if (fofFind(parent.data(), A) == fofFind(parent.data(), B)) continue;
                    bool hit = false;
                    for (int32_t s = cellStart[A]; s < cellStart[A + 1] && !hit; ++s)
                        for (int32_t t = cellStart[B]; t < cellStart[B + 1] && !hit; ++t)
                        {
                            const int32_t i = order[s].second, j = order[t].second;
                            hit = fofPairExact(x[i], y[i], z[i], x[j], y[j], z[j], box, g.b);
                        }
                    if (hit) fofUnion(parent.data(), A, B);
                }
            }
    }

    // the smallest particle of a component: cells in ascending order, a cell's first particle is its smallest
    std::vector<int32_t> root(ncells), least(ncells, 0x7fffffff);
    for (int c = 0; c < ncells; ++c)
    {
        root[c]        = fofFind(parent.data(), c);
        least[root[c]] = std::min(least[root[c]], order[cellStart[c]].second);
    }
#pragma omp parallel for
    for (int c = 0; c < ncells; ++c)
        for (int32_t s = cellStart[c]; s < cellStart[c + 1]; ++s)
            label[order[s].second] = least[root[c]];
}

FofCatalog fofCatalog(int64_t n, const int32_t* label, const double* x, const double* y, const double* z,
                      const double* m, const double* vx, const double* vy, const double* vz, const Box& box,
                      int64_t minMembers)
{
    std::vector<std::pair<int32_t, int32_t>> order; // (label, particle)
    for (int64_t i = 0; i < n; ++i)
        if (label[i] >= 0) order.emplace_back(label[i], int32_t(i));
    std::sort(order.begin(), order.end());
    struct Group
    {
        int64_t count;
        int32_t label;
        int64_t start;
    };
    std::vector<Group> groups;
    for (int64_t p = 0, q; p < int64_t(order.size()); p = q)
    {
        for (q = p + 1; q < int64_t(order.size()) && order[q].first == order[p].first; ++q) {}
        if (q - p >= minMembers) groups.push_back({q - p, order[p].first, p});
    }
    std::sort(groups.begin(), groups.end(), [](const Group& a, const Group& b)
              { return a.count != b.count ? a.count > b.count : a.label < b.label; });
    const int64_t G = int64_t(groups.size());
    FofCatalog cat;
    cat.label.resize(G);
    cat.count.resize(G);
    cat.sums.resize(7 * G);
#pragma omp parallel for schedule(dynamic, 16)
    for (int64_t k = 0; k < G; ++k)
    {
        const Group& grp = groups[k];
        const int32_t i0 = order[grp.start].second; // the root: the label particle itself
        double acc[7]    = {0, 0, 0, 0, 0, 0, 0};
        for (int64_t p0 = 0; p0 < grp.count; p0 += kFofPiece)
        {
            double ps[7] = {0, 0, 0, 0, 0, 0, 0};
            for (int64_t p = p0; p < std::min(p0 + kFofPiece, grp.count); ++p)
            {
                const int32_t j = order[grp.start + p].second;
                ps[0] += m[j];
                ps[1] += m[j] * fofMinImage(x[j] - x[i0], box, 0);
                ps[2] += m[j] * fofMinImage(y[j] - y[i0], box, 1);
                ps[3] += m[j] * fofMinImage(z[j] - z[i0], box, 2);
                if (vx)
                {
                    ps[4] += m[j] * vx[j];
                    ps[5] += m[j] * vy[j];
                    ps[6] += m[j] * vz[j];
                }
            }
            for (int q = 0; q < 7; ++q)
                acc[q] += ps[q];
        }
        double com[3] = {x[i0] + acc[1] / acc[0], y[i0] + acc[2] / acc[0], z[i0] + acc[3] / acc[0]};
        putInBox(com[0], com[1], com[2], box);
        cat.label[k] = grp.label;
        cat.count[k] = grp.count;
        double* out  = cat.sums.data() + 7 * k;
        out[0]       = acc[0];
        for (int a = 0; a < 3; ++a)
        {
            out[1 + a] = com[a];
            out[4 + a] = acc[4 + a] / acc[0];
        }
    }
    return cat;
}

} // namespace sphx::cpu
