/*! Pair statistics on gfx950: pair counts and pair sums per radial bin (definitions: ops/pairstats.py; geometry, bin
 *  tables, per-pair fp64 arithmetic and quanta: sphx/pairstats.hpp, shared with the host path cpu/pairstats_cpu.cpp).
 *
 *  1. Preparation. fofPrepare (fof.hip) runs unchanged on the grid of makePairGrid (cells of at least r_max, R = 1):
 *     16-byte fp32 records {position inside the cell, cell x}, distinct keys cell << shift | particle, the sample
 *     sort, the cell starts, and cell-aligned items of at most 64 sorted positions of one (y, z) row. Then
 *     pairBoundKernel, a thread per occupied cell, adds count(cell) * count(cell and its half stencil) to the bound on
 *     the candidate pairs, and pairGatherKernel writes the fp64 coordinates (and fp32 velocities, fp64 weights) in
 *     sorted order, so the pair kernel addresses everything by sorted position. One host read returns the counts.
 *  2. pairKernel, the hot path: a wave per item, a lane per target. Sources are contiguous sorted ranges:
 *       own row: the positions behind the item's first up to the end of the cell after its last one; a lane takes a
 *                source only from a position behind its own (i < j inside a cell and across the items of a dense
 *                cell); on a periodic x axis the lanes of the last cell also take cell 0 of the row;
 *       the 4 other rows of the half stencil: the cells [first - 1, last + 1] of the row, in two pieces if they wrap.
 *     The range ends come from a 64-ary wave search of cellKey. A range streams through the wave's 1 KiB of LDS in
 *     chunks of 64 sources, SoA {x, y, z in length units, cell x}; the next chunk's records are loaded into registers
 *     before the current one is walked. Every lane reads source s as a broadcast. The test is the wrapped cell
 *     offset, three differences and d2 = dx dx + dy dy + dz dz as a multiply and two FMAs in fp32. Sources two or more
 *     cells away are simply too far: no stencil test is needed.
 *     Counts-only instance: the bin comes from d2_f32 by a branch-free 6-step search over the squared edges in LDS; a
 *     pair inside the band around an edge (sphx/pairstats.hpp) is evaluated again from the fp64 coordinates.
 *     Value instances: every pair that passes the fp32 cut [e_0, e_nb) -+ band is evaluated in fp64 by the shared
 *     term functions; its terms enter as int64 multiples of the channel's quantum.
 *  3. Accumulation. The wave keeps a histogram in LDS (dynamic shared memory), replicated R times and indexed by
 *     lane & (R - 1), bins x replicas with the replica fastest: R is the largest power of two <= 16 for which
 *     R nb (4 + 8 nv) bytes fit kPairHistBytes. Counts are uint32 (ds_add_u32), values native 64-bit LDS adds. A wave
 *     walks the items wave, wave + W, ... of a grid of at most kPairMaxBlocks blocks and folds its replicas into the
 *     int64 result (one global atomic per non-zero bin and channel) when it is done, or earlier before a uint32 count
 *     could wrap: fewer same-address global atomics than a fold per item, the same sums (integer adds commute).
 *     Variant 1 (kept for comparison, profiles/r16/pairstats/README.md): a ballot per distinct bin, wave reductions of
 *     the terms, one lane adds to an unreplicated histogram.
 *
 *  Every loop is bounded: the searches by their shrinking range, the chunk loop by the range. Indices read from memory
 *  are clamped before they address anything (and flagged in the device-check build, bit 10).
 *  No matrix instructions: 3-D distances against a handful of bins have no inner product to feed them.
 */
#include <climits>
#include <cmath>

#include "common.h"
#include "hip_api.h"

namespace sphx::hip
{

namespace
{

constexpr int kChunk         = 64;
constexpr int kPairBlock     = 256;
constexpr int kPairWaves     = kPairBlock / kWave;
constexpr int kPairMaxBlocks = 2048;       // 256 CUs x 8 resident blocks
constexpr int kPairHistBytes = 4096;       // per-wave LDS budget of the replicated histogram
constexpr unsigned kFoldSteps = 1u << 25;  // walked sources between folds: a uint32 slot gains at most 64 per source

__device__ __forceinline__ int clampP(int v, int lo, int hi)
{
    SPHX_DCHECK(v >= lo && v <= hi, 10);
    return v < lo ? lo : (v > hi ? hi : v);
}

//! first index in [lo, hi) whose key is >= v (hi: none): 64 probes per pass, see waveLowerBound in fof.hip
__device__ __forceinline__ int pairLowerBound(const int64_t* __restrict__ keys, int lo, int hi, int64_t v)
{
    while (hi > lo)
    {
        const int stride    = (hi - lo + 63) >> 6;
        const int64_t probe = int64_t(lo) + int64_t(laneId()) * stride;
        const bool below    = probe < hi && keys[probe] < v;
        const int c         = popcount64(ballot(below));
        if (c == 0) return lo;
        const int nextLo = lo + (c - 1) * stride + 1;
        hi               = sphx::smin(hi, lo + c * stride);
        lo               = nextLo;
    }
    return lo;
}

__device__ __forceinline__ void cellOfKey(const FofGrid& g, int64_t key, int& cx, int& cy, int& cz)
{
    cx = int(key % g.n[0]);
    cy = int(key / g.n[0] % g.n[1]);
    cz = int(key / (int64_t(g.n[0]) * g.n[1]));
}

//! counts[3] += count(c) * (count(c) + count(half stencil of c)) over the occupied cells c: the candidate pairs
__global__ void __launch_bounds__(256)
pairBoundKernel(int64_t np, FofGrid g, const int32_t* __restrict__ cellStart, const int64_t* __restrict__ cellKey,
                int64_t* __restrict__ counts)
{
    const int64_t c   = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    const int ncells  = int(sphx::smin(counts[1], np));
    const int ns      = int(sphx::smin(counts[0], np));
    unsigned long long pairs = 0;
    if (c < ncells)
    {
        int cx, cy, cz;
        cellOfKey(g, cellKey[c], cx, cy, cz);
        const int s0 = clampP(cellStart[c], 0, ns), s1 = clampP(cellStart[c + 1], s0, ns);
        unsigned long long sources = s1 - s0;
        const int nRuns = fofNumRuns(g);
        for (int r = 0; r < nRuns; ++r)
            for (int piece = 0; piece < 2; ++piece)
            {
                FofRun run;
                if (!fofRun(g, r, piece, cx, cx, cy, cz, run)) continue;
                int lo = 0, hi = ncells;
                while (lo < hi)
                {
                    const int mid = (lo + hi) >> 1;
                    if (cellKey[mid] < run.kLo) lo = mid + 1;
                    else hi = mid;
                }
                // (a run holds at most 3 cells)
                for (int b = lo; b < ncells && b < lo + 3 && cellKey[b] <= run.kHi; ++b)
                    sources += clampP(cellStart[b + 1], 0, ns) - clampP(cellStart[b], 0, ns);
            }
        pairs = (unsigned long long)(s1 - s0) * sources;
    }
    pairs = waveSum(pairs);
    if (laneId() == 0 && pairs) atomicAdd(reinterpret_cast<unsigned long long*>(counts + 3), pairs);
}

struct PairGatherArgs
{
    int64_t np;
    const int32_t* perm;
    const int64_t* counts;
    const double *x, *y, *z, *w;
    const float *vx, *vy, *vz;
    double *xs, *ys, *zs, *ws;
    float4* vs;
};

__global__ void __launch_bounds__(256) pairGatherKernel(PairGatherArgs A)
{
    const int64_t p = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (p >= sphx::smin(A.counts[0], A.np)) return;
    const int i = clampP(A.perm[p], 0, int(A.np - 1));
    A.xs[p] = A.x[i];
    A.ys[p] = A.y[i];
    A.zs[p] = A.z[i];
    if (A.w) A.ws[p] = A.w[i];
    if (A.vx) A.vs[p] = float4{A.vx[i], A.vy[i], A.vz[i], 0.f};
}

struct PairArgs
{
    FofGrid g;
    Box box;
    PairTables t;
    double invq[5];
    int ns, ncells, R;
    int64_t nItems;
    const int32_t *itemStart, *cellStart, *cellOf;
    const int64_t* cellKey;
    const float4* rec;
    const double *xs, *ys, *zs, *ws;
    const float4* vs;
    unsigned long long* out;   // kPairChannels rows of nb
    unsigned long long* stats; // [0] candidates tested, [1] passed the fp32 filter, [2] evaluated in fp64
};

template<int CH>
struct PairLds
{
    static constexpr int nv = (CH & kPairWeights ? 1 : 0) + (CH & kPairVelocity ? 4 : 0);
    static constexpr int slotBytes = 4 + 8 * nv;
};

/*! @brief the wave's histogram in LDS: nv planes of uint64 [bin * R + replica], then one plane of uint32 counts */
template<int CH>
struct PairHist
{
    unsigned long long* val;
    unsigned* cnt;
    int plane; // nb * R

    __device__ __forceinline__ void clear(int lane)
    {
        for (int i = lane; i < plane; i += kWave)
        {
            cnt[i] = 0;
#pragma unroll
            for (int c = 0; c < PairLds<CH>::nv; ++c)
                val[c * plane + i] = 0;
        }
    }

    //! adds the replicas of bin `lane` to the global result and clears them
    __device__ __forceinline__ void fold(const PairArgs& A, int lane, int R)
    {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        const int nb = A.t.nb;
        if (lane < nb)
        {
            unsigned long long c = 0;
            for (int r = 0; r < R; ++r)
            {
                c += cnt[lane * R + r];
                cnt[lane * R + r] = 0;
            }
            if (c) atomicAdd(A.out + lane, c);
            int row = 1;
#pragma unroll
            for (int ch = 0; ch < 5; ++ch)
            {
                const bool on = ch == 0 ? (CH & kPairWeights) != 0 : (CH & kPairVelocity) != 0;
                if (!on) continue;
                const int pl = ch == 0 ? 0 : (CH & kPairWeights ? ch : ch - 1);
                unsigned long long v = 0;
                for (int r = 0; r < R; ++r)
                {
                    v += val[pl * plane + lane * R + r];
                    val[pl * plane + lane * R + r] = 0;
                }
                if (v) atomicAdd(A.out + (row + ch) * nb + lane, v);
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
};

//! sum over the lanes of mask m of v (0 in the others), in every lane
__device__ __forceinline__ unsigned long long maskedSum(unsigned long long v, bool in)
{
    return waveSum(in ? v : 0ull);
}

template<int CH, int VARIANT, bool STATS>
__global__ void __launch_bounds__(kPairBlock) pairKernel(PairArgs A)
{
    constexpr int nv = PairLds<CH>::nv;
    __shared__ float sX[kPairWaves][kChunk], sY[kPairWaves][kChunk], sZ[kPairWaves][kChunk];
    __shared__ int sC[kPairWaves][kChunk];
    __shared__ float sSearch[kPairMaxBins], sLo[kPairMaxBins], sHi[kPairMaxBins];
    __shared__ double sE2[kPairMaxBins + 1];
    extern __shared__ unsigned long long sHist[];

    const int wave = threadIdx.x >> 6, lane = laneId();
    const FofGrid& g = A.g;
    const int nb = A.t.nb, R = VARIANT == 0 ? A.R : 1;

    if (threadIdx.x < kPairMaxBins)
    {
        sSearch[threadIdx.x] = A.t.search[threadIdx.x];
        sLo[threadIdx.x]     = A.t.safeLo[threadIdx.x];
        sHi[threadIdx.x]     = A.t.safeHi[threadIdx.x];
    }
    if (threadIdx.x <= kPairMaxBins) sE2[threadIdx.x] = A.t.e2[threadIdx.x <= nb ? threadIdx.x : nb];
    PairHist<CH> H;
    H.plane = nb * R;
    // a wave's region: nv planes of 8 bytes, one of 4, rounded up to 8 bytes
    const int regionWords = (H.plane * PairLds<CH>::slotBytes + 7) / 8;
    H.val = sHist + size_t(wave) * regionWords;
    H.cnt = reinterpret_cast<unsigned*>(H.val + nv * H.plane);
    H.clear(lane);
    __syncthreads(); // the only block barrier: the tables are read-only from here on

    const float ex = float(g.e[0]), ey = float(g.e[1]), ez = float(g.e[2]);
    const float cutLo = A.t.cutLo, cutHi = A.t.cutHi;
    const int rep = lane & (R - 1);
    unsigned sinceFold = 0;
    unsigned long long nTested = 0, nPassed = 0, nExact = 0;

    const int64_t nWaves = int64_t(gridDim.x) * kPairWaves;
    for (int64_t item = int64_t(blockIdx.x) * kPairWaves + wave; item < A.nItems; item += nWaves)
    {
        const int t0 = clampP(A.itemStart[item], 0, A.ns - 1);
        const int nt = clampP(A.itemStart[item + 1] - t0, 1, sphx::smin(kChunk, A.ns - t0));
        const bool valid = lane < nt;
        const int tq     = t0 + (valid ? lane : 0);
        const float4 tr  = A.rec[tq];
        const int tcx    = __float_as_int(tr.w);
        const float tx = tr.x * ex, tyl = tr.y * ey, tzl = tr.z * ez;
        double txd = 0, tyd = 0, tzd = 0, tw = 0;
        float4 tv{0.f, 0.f, 0.f, 0.f};
        if (nv > 0)
        {
            txd = A.xs[tq];
            tyd = A.ys[tq];
            tzd = A.zs[tq];
            if (CH & kPairWeights) tw = A.ws[tq];
            if (CH & kPairVelocity) tv = A.vs[tq];
        }

        // the item's row and its extent in x (the targets are sorted by cell)
        const int cxLo = __builtin_amdgcn_readfirstlane(tcx), cxHi = readLaneI(tcx, nt - 1);
        const int c0 = clampP(A.cellOf[t0], 0, A.ncells - 1); // the item's first cell
        const int64_t key0 = A.cellKey[c0];
        int kx, cy, cz;
        cellOfKey(g, key0, kx, cy, cz);
        const int64_t rowKey = key0 - kx;

        const int nRuns = fofNumRuns(g);
        for (int r = 0; r < nRuns; ++r)
            for (int piece = 0; piece < 2; ++piece)
            {
                // the sorted range [p0, p1) of the piece, the row offsets, and which lanes take part
                int64_t kLo, kHi;
                int dy = 0, dz = 0;
                bool laneOk = valid;
                const bool own = r == 0 && piece == 0;
                if (r == 0)
                {
                    if (piece == 0)
                    {
                        kLo = rowKey + cxLo;
                        kHi = rowKey + sphx::smin(cxHi + 1, g.n[0] - 1);
                    }
                    else
                    {
                        if (!g.per[0] || cxHi != g.n[0] - 1) continue;
                        kLo = kHi = rowKey;
                        laneOk    = valid && tcx == g.n[0] - 1;
                    }
                }
                else
                {
                    FofRun run;
                    if (!fofRun(g, r, piece, cxLo, cxHi, cy, cz, run)) continue;
                    kLo = run.kLo;
                    kHi = run.kHi;
                    dy  = run.dy;
                    dz  = run.dz;
                }
                int p0, p1;
                {
                    const int cb0 = own ? c0 : pairLowerBound(A.cellKey, 0, A.ncells, kLo);
                    if (cb0 >= A.ncells || A.cellKey[cb0] > kHi) continue;
                    // keys are distinct integers: at most kHi - kLo + 1 cells lie in the range
                    const int to  = int(sphx::smin(int64_t(A.ncells), int64_t(cb0) + (kHi - kLo + 1)));
                    const int cb1 = pairLowerBound(A.cellKey, cb0, to, kHi + 1);
                    p0 = own ? t0 + 1 : clampP(A.cellStart[cb0], 0, A.ns);
                    p1 = clampP(A.cellStart[clampP(cb1, 0, A.ncells)], 0, A.ns);
                }
                if (p0 >= p1) continue;
                const bool wrapX = g.per[0] && !own;
                const float ty = tyl - float(dy) * ey, tz = tzl - float(dz) * ez;

                float4 nxt = p0 + lane < p1 ? A.rec[p0 + lane] : float4{0.f, 0.f, 0.f, 0.f};
                for (int base = p0; base < p1; base += kChunk)
                {
                    const int cnt = sphx::smin(kChunk, p1 - base);
                    __builtin_amdgcn_wave_barrier(); // the chunk before has been read
                    sX[wave][lane] = nxt.x * ex;
                    sY[wave][lane] = nxt.y * ey;
                    sZ[wave][lane] = nxt.z * ez;
                    sC[wave][lane] = __float_as_int(nxt.w);
                    if (base + kChunk + lane < p1) nxt = A.rec[base + kChunk + lane];
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

                    for (int s = 0; s < cnt; ++s)
                    {
                        const int j = base + s;
                        int ddx     = sC[wave][s] - tcx;
                        if (wrapX) ddx = ddx > 1 ? ddx - g.n[0] : (ddx < -1 ? ddx + g.n[0] : ddx);
                        const bool take = own ? (valid && j > tq) : laneOk;
                        const float ux = fmaf(float(ddx), ex, sX[wave][s] - tx);
                        const float uy = sY[wave][s] - ty, uz = sZ[wave][s] - tz;
                        const float d2f = fmaf(uz, uz, fmaf(uy, uy, ux * ux));
                        const bool pass = take && d2f >= cutLo && d2f < cutHi;
                        if (STATS)
                        {
                            nTested += take;
                            nPassed += pass;
                        }
                        int k = -1;
                        long long q[nv > 0 ? nv : 1] = {};
                        if (pass)
                        {
                            bool exact = nv > 0;
                            if (nv == 0)
                            {
                                int pos = 0;
#pragma unroll
                                for (int step = 32; step > 0; step >>= 1)
                                    pos += sSearch[pos + step - 1] <= d2f ? step : 0;
                                k     = pos;
                                exact = !(d2f > sLo[k] && d2f < sHi[k]);
                            }
                            if (exact)
                            {
                                double d[3], d2;
                                if (nv == 0)
                                {
                                    txd = A.xs[tq];
                                    tyd = A.ys[tq];
                                    tzd = A.zs[tq];
                                }
                                pairSeparation(txd, tyd, tzd, A.xs[j], A.ys[j], A.zs[j], A.box, d, d2);
                                k = pairBin(sE2, nb, d2);
                                if (STATS) ++nExact;
                                if (nv > 0 && k >= 0)
                                {
                                    int c = 0;
                                    if (CH & kPairWeights) q[c++] = pairQuantise(tw * A.ws[j], A.invq[0]);
                                    if (CH & kPairVelocity)
                                    {
                                        const float4 sv = A.vs[j];
                                        double t[4];
                                        pairVelocityTerms(d, d2, double(sv.x) - double(tv.x),
                                                          double(sv.y) - double(tv.y), double(sv.z) - double(tv.z), t);
#pragma unroll
                                        for (int a = 0; a < 4; ++a)
                                            q[c + a] = pairQuantise(t[a], A.invq[1 + a]);
                                    }
                                }
                            }
                        }
                        if (VARIANT == 0)
                        {
                            if (k >= 0)
                            {
                                atomicAdd(H.cnt + k * R + rep, 1u);
#pragma unroll
                                for (int c = 0; c < nv; ++c)
                                    atomicAdd(H.val + c * H.plane + k * R + rep, (unsigned long long)q[c]);
                            }
                        }
                        else
                        {
                            // a ballot per distinct bin of this step; the lowest lane of the bin adds the wave's sums
                            uint64_t left = ballot(k >= 0);
                            while (left)
                            {
                                const int kb       = readLaneI(k, ctz64(left));
                                const bool in      = k == kb;
                                const uint64_t m   = ballot(in);
                                const bool adder   = in && (m & lanemaskLt()) == 0;
                                if (adder) atomicAdd(H.cnt + kb, unsigned(popcount64(m)));
#pragma unroll
                                for (int c = 0; c < nv; ++c)
                                {
                                    const unsigned long long sum = maskedSum((unsigned long long)q[c], in);
                                    if (adder) atomicAdd(H.val + c * H.plane + kb, sum);
                                }
                                left &= ~m;
                            }
                        }
                    }
                    sinceFold += unsigned(cnt);
                    if (sinceFold >= kFoldSteps)
                    {
                        H.fold(A, lane, R);
                        sinceFold = 0;
                    }
                }
            }
    }
    H.fold(A, lane, R);

    if (STATS)
    {
        nTested = waveSum(nTested);
        nPassed = waveSum(nPassed);
        nExact  = waveSum(nExact);
        if (lane == 0)
        {
            atomicAdd(A.stats + 0, nTested);
            atomicAdd(A.stats + 1, nPassed);
            atomicAdd(A.stats + 2, nExact);
        }
    }
}

template<int CH, int VARIANT>
void launchPair(const PairArgs& A, unsigned blocks, size_t ldsBytes, hipStream_t s)
{
    if (A.stats) pairKernel<CH, VARIANT, true><<<blocks, kPairBlock, ldsBytes, s>>>(A);
    else pairKernel<CH, VARIANT, false><<<blocks, kPairBlock, ldsBytes, s>>>(A);
}

template<int CH>
void launchPairVariant(const PairArgs& A, int variant, unsigned blocks, size_t ldsBytes, hipStream_t s)
{
    if (variant == 0) launchPair<CH, 0>(A, blocks, ldsBytes, s);
    else launchPair<CH, 1>(A, blocks, ldsBytes, s);
}

} // namespace

int pairReplicas(int nb, int channels)
{
    const int nv   = (channels & kPairWeights ? 1 : 0) + (channels & kPairVelocity ? 4 : 0);
    const int slot = nb * (4 + 8 * nv);
    int R          = 16;
    while (R > 1 && R * slot > kPairHistBytes)
        R >>= 1;
    return R;
}

void pairPrepare(int64_t np, const double* x, const double* y, const double* z, const uint8_t* select,
                 const FofGrid& g, const FofBuffers& B, const double* w, const float* vx, const float* vy,
                 const float* vz, const PairSorted& S, hipStream_t s)
{
    fofPrepare(np, x, y, z, select, g, B, s);
    const unsigned nb = gridFor(np, 256);
    pairBoundKernel<<<nb, 256, 0, s>>>(np, g, B.cellStart, B.cellKey, B.counts);
    SPHX_LAUNCH_CHECK();
    const PairGatherArgs A{np, B.perm, B.counts, x, y, z, w, vx, vy, vz, S.x, S.y, S.z, S.w, S.v};
    pairGatherKernel<<<nb, 256, 0, s>>>(A);
    SPHX_LAUNCH_CHECK();
}

void pairRun(int64_t np, int64_t ns, int64_t ncells, int64_t nItems, const Box& box, const FofGrid& g,
             const PairTables& t, int channels, const double* q, const FofBuffers& B, const PairSorted& S, int variant,
             unsigned long long* stats, int64_t* out, hipStream_t s)
{
    if (np < 1 || np > kFofMaxN || ns < 0 || ns > np || ncells < 0 || ncells > ns || nItems < 0 || nItems > ns ||
        (ns > 0 && (ncells < 1 || nItems < 1)))
        throw std::invalid_argument("pairstats: inconsistent counts");
    if (channels < 0 || channels > 3 || variant < 0 || variant > 1)
        throw std::invalid_argument("pairstats: unknown channel set or variant");
    if (!S.x || !S.y || !S.z || ((channels & kPairWeights) && !S.w) || ((channels & kPairVelocity) && !S.v))
        throw std::invalid_argument("pairstats: a sorted buffer of the channel set is missing");
    if (nItems == 0) return;
    PairArgs A{};
    A.g   = g;
    A.box = box;
    A.t   = t;
    for (int c = 0; c < 5; ++c)
        A.invq[c] = 1.0 / q[c];
    A.ns        = int(ns);
    A.ncells    = int(ncells);
    A.R         = pairReplicas(t.nb, channels);
    A.nItems    = nItems;
    A.itemStart = B.itemStart;
    A.cellStart = B.cellStart;
    A.cellOf    = B.cellOf;
    A.cellKey   = B.cellKey;
    A.rec       = B.rec;
    A.xs = S.x, A.ys = S.y, A.zs = S.z, A.ws = S.w, A.vs = S.v;
    A.out   = reinterpret_cast<unsigned long long*>(out);
    A.stats = stats;
    const int nv        = (channels & kPairWeights ? 1 : 0) + (channels & kPairVelocity ? 4 : 0);
    const int R         = variant == 0 ? A.R : 1;
    const size_t region = size_t((t.nb * R * (4 + 8 * nv) + 7) / 8) * 8;
    const size_t lds    = region * kPairWaves;
    const unsigned blocks = unsigned(sphx::smin(int64_t(gridFor(nItems, kPairWaves)), int64_t(kPairMaxBlocks)));
    switch (channels)
    {
        case 0: launchPairVariant<0>(A, variant, blocks, lds, s); break;
        case 1: launchPairVariant<1>(A, variant, blocks, lds, s); break;
        case 2: launchPairVariant<2>(A, variant, blocks, lds, s); break;
        default: launchPairVariant<3>(A, variant, blocks, lds, s); break;
    }
    SPHX_LAUNCH_CHECK();
}

SPHX_DCHECK_READER(dcheckPairstats)

} // namespace sphx::hip
