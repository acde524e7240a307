// Pair statistics on the host (definitions: ops/pairstats.py): the reference configuration of hip/pairstats.hip. A
// sorted cell list on the grid of sphx/pairstats.hpp, OpenMP over the cells, every pair through the shared fp64
// separation, bin and term functions and the same quantisation; per-thread int64 histograms are added at the end.
#include <algorithm>
#include <utility>
#include <vector>

#include "cpu_api.hpp"

// no fused multiply-adds: every product of the pair arithmetic is rounded on its own, as on the device
#pragma GCC optimize("fp-contract=off")

namespace sphx::cpu
{

int64_t pairStatistics(int64_t np, const double* x, const double* y, const double* z, const uint8_t* select,
                       const Box& box, const FofGrid& g, const PairTables& T, const double* w, const float* vx,
                       const float* vy, const float* vz, double W, const double* vrange, int64_t maxBound, double* q,
                       int64_t* out)
{
    if (np > kFofMaxN) throw std::invalid_argument("pairstats: more than 2^30 particles");
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
    const int ncells = int(cellKey.size());
    cellStart.push_back(int32_t(ns));

    // the source cells of every cell: itself, then its half stencil
    const int nRuns = fofNumRuns(g);
    auto sources    = [&](int A, std::vector<int>& cells)
    {
        const int64_t key = cellKey[A];
        const int cx = int(key % g.n[0]), cy = int(key / g.n[0] % g.n[1]), cz = int(key / (int64_t(g.n[0]) * g.n[1]));
        cells.assign(1, A);
        for (int r = 0; r < nRuns; ++r)
            for (int p = 0; p < 2; ++p)
            {
                FofRun run;
                if (!fofRun(g, r, p, cx, cx, cy, cz, run)) continue;
                int B = int(std::lower_bound(cellKey.begin(), cellKey.end(), run.kLo) - cellKey.begin());
                for (; B < ncells && cellKey[B] <= run.kHi; ++B)
                    cells.push_back(B);
            }
    };

    int64_t bound = 0;
#pragma omp parallel for schedule(dynamic, 64) reduction(+ : bound)
    for (int A = 0; A < ncells; ++A)
    {
        std::vector<int> cells;
        sources(A, cells);
        int64_t n = 0;
        for (int B : cells)
            n += cellStart[B + 1] - cellStart[B];
        bound += n * (cellStart[A + 1] - cellStart[A]);
    }
    if (bound > maxBound)
        throw std::invalid_argument("pairstats: more than 2^38 candidate pairs; subsample the particles with select");
    pairQuanta(W, vrange, bound, q);
    double invq[5];
    for (int c = 0; c < 5; ++c)
        invq[c] = 1.0 / q[c];

    const int nb = T.nb, rows = kPairChannels * nb;
    std::fill(out, out + rows, int64_t(0));
#pragma omp parallel
    {
        std::vector<int64_t> hist(rows, 0);
        std::vector<int> cells;
#pragma omp for schedule(dynamic, 16)
        for (int A = 0; A < ncells; ++A)
        {
            sources(A, cells);
            for (int32_t s = cellStart[A]; s < cellStart[A + 1]; ++s)
            {
                const int32_t i = order[s].second;
                for (size_t b = 0; b < cells.size(); ++b)
                    for (int32_t t = b == 0 ? s + 1 : cellStart[cells[b]]; t < cellStart[cells[b] + 1]; ++t)
                    {
                        const int32_t j = order[t].second;
                        double d[3], d2;
                        pairSeparation(x[i], y[i], z[i], x[j], y[j], z[j], box, d, d2);
                        const int k = pairBin(T.e2, nb, d2);
                        if (k < 0) continue;
                        hist[k] += 1;
                        if (w) hist[nb + k] += pairQuantise(w[i] * w[j], invq[0]);
                        if (vx)
                        {
                            double term[4];
                            pairVelocityTerms(d, d2, double(vx[j]) - double(vx[i]), double(vy[j]) - double(vy[i]),
                                              double(vz[j]) - double(vz[i]), term);
                            for (int a = 0; a < 4; ++a)
                                hist[(2 + a) * nb + k] += pairQuantise(term[a], invq[1 + a]);
                        }
                    }
            }
        }
#pragma omp critical
        for (int r = 0; r < rows; ++r)
            out[r] += hist[r];
    }
    return bound;
}

} // namespace sphx::cpu
