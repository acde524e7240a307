/*! Radial profiles and spherical-overdensity masses about many centres on gfx950 (definitions: ops/profiles.py; cells,
 *  slots, keys, per-hit fp64 arithmetic and the crossing rule: sphx/profiles.hpp, shared with cpu/profiles_cpu.cpp).
 *
 *  1. Preparation. pairPrepare (pairstats.hip) runs unchanged on the grid of makePairGrid: the 16-byte fp32 records
 *     {position inside the cell, cell x} and the fp64 coordinates, both in sorted order, cellStart and cellKey.
 *     profileSlotsKernel, a thread per (centre, slot), writes the centre's cell-relative record, the sorted range of
 *     each of its 18 slots (two binary searches of cellKey) and the number of items of the slot; a scan numbers the
 *     items. The item count travels with the host read of the preparation's counts.
 *  2. profileHitKernel, the hot path: a streaming filter, a wave per item = (centre, slot, segment of at most `seg`
 *     sorted positions). The wave finds its slot by a 64-ary search of the item offsets, then reads 64 records per
 *     step (one coalesced 16-byte load per lane, the next step's load issued before this step's test) and tests them
 *     in fp32 against the wave-uniform centre record: wrapped cell offset in x, the row offsets of the slot in y and
 *     z, a multiply and two FMAs. What is not at or above cutHi forms d2 in fp64 from the sorted coordinates and the
 *     key float(d2); hits (key < E_nb) are compacted by ballot. The kernel runs twice around one scan of the item
 *     counts: the count pass writes a count per item, the write pass puts an item's hits in stream order at the
 *     item's offset as key64 = centre << 32 | bits(key) and the sorted position of the particle. No atomics on
 *     positions: the hit list is identical from run to run. Nothing is staged in LDS: a record is read by one lane
 *     only, and the centre lives in scalar registers.
 *  3. The sample sort orders the hit keys (stable: ties keep the emission order); profileStartsKernel searches the
 *     sorted keys for every centre's first hit and counts its segments of `seg` sorted hits; a scan numbers them.
 *  4. profileSumKernel, a wave per (centre, segment): a lane per hit of a chunk of 64 gathers m, v, u by particle,
 *     forms the terms in fp64 and finds its bin by a search of its key in the E table (LDS). Bins are contiguous lane
 *     runs of a sorted chunk: a segmented wave scan sums each run and the run's last lane adds the run to the wave's
 *     row in LDS, one writer per bin and step, so there are no LDS atomics and no histogram. The wave writes a partial
 *     row and the segment's total mass, and the hits' masses in sorted order. profileCombineKernel adds the partial
 *     rows of a centre in segment order and turns the segment masses into carried-in masses.
 *  5. profileCrossKernel, a wave per (centre, segment): a wave scan per 64 hits on top of the carried-in mass gives
 *     M_q; the condition M_q >= (4 pi / 3) rho_t r_q^3 is evaluated at tie-run ends only (the next key differs, read
 *     across the chunk and segment boundary: a run belongs to the segment where it ends), lane t keeps the outermost
 *     crossing of threshold t. profilePickKernel keeps the outermost over a centre's segments.
 *
 *  No atomics on values: every sum has a fixed order, the results are bit-identical from run to run. Every loop is
 *  bounded by its range; indices read from memory are clamped before they address anything (and flagged in the
 *  device-check build, bit 12). No matrix instructions: a streaming 3-D distance filter has no inner product to feed.
 */
#include <cmath>

#include "common.h"
#include "hip_api.h"

namespace sphx::hip
{

namespace
{

constexpr int kProfBlock = 256;
constexpr int kProfWaves = kProfBlock / kWave;

__device__ __forceinline__ int64_t clampQ(int64_t v, int64_t lo, int64_t hi)
{
    SPHX_DCHECK(v >= lo && v <= hi, 12);
    return v < lo ? lo : (v > hi ? hi : v);
}

//! first index in [0, n) whose entry is > v (n: none), found by the whole wave (see waveLowerBound in fof.hip)
__device__ __forceinline__ int64_t waveUpperBound(const int64_t* __restrict__ a, int64_t n, int64_t v)
{
    int64_t lo = 0, hi = n;
    while (hi > lo)
    {
        const int64_t stride = (hi - lo + 63) >> 6;
        const int64_t probe  = lo + int64_t(laneId()) * stride;
        const bool notAbove  = probe < hi && a[probe] <= v;
        const int c          = popcount64(ballot(notAbove));
        if (c == 0) return lo;
        const int64_t nextLo = lo + (c - 1) * stride + 1;
        hi                   = sphx::smin(hi, lo + c * stride);
        lo                   = nextLo;
    }
    return lo;
}

__device__ __forceinline__ double waveInclusiveSum(double v, int lane)
{
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1)
    {
        const double t = __shfl_up(v, o);
        if (lane >= o) v += t;
    }
    return v;
}

__device__ __forceinline__ float keyOf(uint64_t key64) { return __uint_as_float(unsigned(key64 & 0xffffffffull)); }

// ------------------------------------------------------------------------------------------------------ the plan

/*! @brief thread t = centre * 18 + slot: the sorted range of the slot and its item count (entry C * 18: 0, for the
 *         scan's total); the thread of slot 0 writes the centre's record */
__global__ void __launch_bounds__(256)
profileSlotsKernel(int64_t C, int64_t np, const double* __restrict__ cxyz, FofGrid g, int seg,
                   const int64_t* __restrict__ counts, const int32_t* __restrict__ cellStart,
                   const int64_t* __restrict__ cellKey, ProfileCentre* __restrict__ crec, int32_t* __restrict__ slotLo,
                   int32_t* __restrict__ slotHi, int64_t* __restrict__ itemCount)
{
    const int64_t t = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (t > C * kProfileSlots) return;
    if (t == C * kProfileSlots)
    {
        itemCount[t] = 0;
        return;
    }
    const int64_t c = t / kProfileSlots;
    const int slot  = int(t % kProfileSlots);
    const int ns = int(clampQ(counts[0], 0, np)), ncells = int(clampQ(counts[1], 0, ns));
    const ProfileCentre r = profileCentre(g, cxyz[3 * c], cxyz[3 * c + 1], cxyz[3 * c + 2]);
    if (slot == 0) crec[c] = r;
    int64_t kLo, kHi;
    int dy, dz, p0 = 0, p1 = 0;
    if (ncells > 0 && profileSlot(g, r.cx, r.cy, r.cz, slot, kLo, kHi, dy, dz))
    {
        int b[2];
        for (int e = 0; e < 2; ++e)
        {
            const int64_t v = e ? kHi + 1 : kLo;
            int lo = 0, hi = ncells;
            while (lo < hi)
            {
                const int mid = (lo + hi) >> 1;
                if (cellKey[mid] < v) lo = mid + 1;
                else hi = mid;
            }
            b[e] = lo;
        }
        p0 = int(clampQ(cellStart[b[0]], 0, ns)); // (cellStart has ncells + 1 entries)
        p1 = int(clampQ(cellStart[b[1]], p0, ns));
    }
    slotLo[t]    = p0;
    slotHi[t]    = p1;
    itemCount[t] = (p1 - p0 + seg - 1) / seg;
}

// ------------------------------------------------------------------------------------------------- the hit kernel

struct ProfileHitArgs
{
    FofGrid g;
    Box box;
    float cutHi, Enb;
    int seg, ns;
    int64_t C, nItems, H;
    const ProfileCentre* crec;
    const double* cxyz;
    const int32_t *slotLo, *slotHi;
    const int64_t* itemOff; // C * 18 + 1
    const float4* rec;
    const double *xs, *ys, *zs;
    int64_t* itemHits; // nItems + 1: the count pass writes counts, the write pass reads offsets
    uint64_t* keys;    // H
    int32_t* pidx;     // H
    unsigned long long* stats; // null: not counted. [0] candidates tested, [1] evaluated in fp64, [2] hits
};

template<bool WRITE>
__global__ void __launch_bounds__(kProfBlock) profileHitKernel(ProfileHitArgs A)
{
    const int lane     = laneId();
    const int64_t item = int64_t(blockIdx.x) * kProfWaves + (threadIdx.x >> 6);
    if (item >= A.nItems) return; // (waves never meet at a block barrier)
    if (!WRITE && item == 0 && lane == 0) A.itemHits[A.nItems] = 0;
    const FofGrid& g = A.g;

    const int64_t nSlots = A.C * kProfileSlots;
    const int64_t t      = clampQ(waveUpperBound(A.itemOff, nSlots + 1, item) - 1, 0, nSlots - 1);
    const int64_t c      = t / kProfileSlots;
    const int slot       = int(t % kProfileSlots);
    const int64_t local  = clampQ(item - A.itemOff[t], 0, A.ns / A.seg);
    const int s0 = int(clampQ(A.slotLo[t], 0, A.ns)), s1 = int(clampQ(A.slotHi[t], s0, A.ns));
    const int p0 = int(sphx::smin(int64_t(s1), s0 + local * A.seg));
    const int p1 = int(sphx::smin(int64_t(s1), int64_t(p0) + A.seg));

    const ProfileCentre cr = A.crec[c];
    const double cX = A.cxyz[3 * c], cY = A.cxyz[3 * c + 1], cZ = A.cxyz[3 * c + 2];
    const int dy = (slot >> 1) % 3 - 1, dz = (slot >> 1) / 3 - 1;
    const float ex = float(g.e[0]), ey = float(g.e[1]), ez = float(g.e[2]);
    const float tx = cr.fx * ex, ty = cr.fy * ey - float(dy) * ey, tz = cr.fz * ez - float(dz) * ez;
    const bool wrapX = g.per[0] != 0;
    const uint64_t hi32 = uint64_t(c) << 32;

    int64_t off = WRITE ? clampQ(A.itemHits[item], 0, A.H) : 0;
    unsigned long long nTested = 0, nExact = 0;
    int count = 0;

    float4 nxt = p0 + lane < p1 ? A.rec[p0 + lane] : float4{0.f, 0.f, 0.f, 0.f};
    for (int base = p0; base < p1; base += kWave)
    {
        const int p     = base + lane;
        const bool in   = p < p1;
        const float4 r  = nxt;
        if (base + kWave + lane < p1) nxt = A.rec[base + kWave + lane];
        int ddx = __float_as_int(r.w) - cr.cx;
        if (wrapX) ddx = ddx > 1 ? ddx - g.n[0] : (ddx < -1 ? ddx + g.n[0] : ddx);
        const float ux = fmaf(float(ddx), ex, r.x * ex - tx);
        const float uy = r.y * ey - ty, uz = r.z * ez - tz;
        const float d2f = fmaf(uz, uz, fmaf(uy, uy, ux * ux));
        const bool pass = in && d2f < A.cutHi;
        bool hit = false;
        float k  = 0.f;
        if (pass)
        {
            double d[3], d2;
            pairSeparation(cX, cY, cZ, A.xs[p], A.ys[p], A.zs[p], A.box, d, d2);
            k   = float(d2);
            hit = k < A.Enb;
        }
        const uint64_t hm = ballot(hit);
        if (WRITE)
        {
            const int64_t pos = off + popcount64(hm & lanemaskLt());
            SPHX_DCHECK(!hit || pos < A.H, 12);
            if (hit && pos < A.H)
            {
                A.keys[pos] = hi32 | uint64_t(__float_as_uint(k));
                A.pidx[pos] = p;
            }
            off += popcount64(hm);
        }
        else
        {
            count += popcount64(hm);
            if (A.stats)
            {
                nTested += popcount64(ballot(in));
                nExact += popcount64(ballot(pass));
            }
        }
    }
    if (!WRITE && lane == 0)
    {
        A.itemHits[item] = count;
        if (A.stats)
        {
            atomicAdd(A.stats + 0, nTested);
            atomicAdd(A.stats + 1, nExact);
            atomicAdd(A.stats + 2, (unsigned long long)count);
        }
    }
}

// ------------------------------------------------------------------------------------------------ the reduction

struct ProfileReduceArgs
{
    Box box;
    ProfileTables t;
    int T, seg;
    double rho[kProfileMaxThresholds];
    int64_t C, H, U, np, ns;
    const uint64_t* keys;                   // H, sorted
    const int32_t *hperm, *pidx, *perm;     // sorted hit -> emitted hit -> sorted position -> particle
    const double *xs, *ys, *zs;
    ProfileFields f;
    const double *cxyz, *vc;
    int64_t *start, *segOff;                // C + 1 each
    double *partial, *segMass, *carry, *hmass; // U rows of 6 nb; U; U; H
    int64_t* segQ;                          // U * 8
    double* segM;                           // U * 8
    int64_t* count;                         // C * nb
    double* sums;                           // 5 * C * nb
    double *soR, *soM;                      // C * T
    int64_t* soN;
    uint8_t* soTrunc;
    int64_t* hits;                          // C
};

//! start[c] = first sorted hit of centre c (start[C] = H), segOff[c] = its segments (0 for c == C, the scan's total)
__global__ void __launch_bounds__(256) profileStartsKernel(ProfileReduceArgs A)
{
    const int64_t c = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (c > A.C) return;
    int64_t b[2];
    for (int e = 0; e < 2; ++e)
    {
        const uint64_t v = uint64_t(c + e) << 32;
        int64_t lo = 0, hi = A.H;
        while (lo < hi)
        {
            const int64_t mid = (lo + hi) >> 1;
            if (A.keys[mid] < v) lo = mid + 1;
            else hi = mid;
        }
        b[e] = lo;
    }
    A.start[c]  = b[0];
    A.segOff[c] = c < A.C ? (b[1] - b[0] + A.seg - 1) / A.seg : 0;
}

//! the segment of this wave: centre c, sorted hits [h0, h1), the centre's hits end at hEnd; false: no such segment
__device__ __forceinline__ bool profileSegment(const ProfileReduceArgs& A, int64_t sgi, int64_t& c, int64_t& h0,
                                               int64_t& h1, int64_t& hEnd)
{
    const int64_t nSeg = clampQ(A.segOff[A.C], 0, A.U);
    if (sgi >= nSeg) return false;
    c                   = clampQ(waveUpperBound(A.segOff, A.C + 1, sgi) - 1, 0, A.C - 1);
    const int64_t local = clampQ(sgi - A.segOff[c], 0, A.H / A.seg);
    const int64_t b     = clampQ(A.start[c], 0, A.H);
    hEnd                = clampQ(A.start[c + 1], b, A.H);
    h0                  = sphx::smin(hEnd, b + local * A.seg);
    h1                  = sphx::smin(hEnd, h0 + A.seg);
    return true;
}

__global__ void __launch_bounds__(kProfBlock) profileSumKernel(ProfileReduceArgs A)
{
    __shared__ float sE[kProfileMaxBins + 1];
    __shared__ double sAcc[kProfWaves][kProfileChannels][kProfileMaxBins];

    const int wave = threadIdx.x >> 6, lane = laneId();
    if (threadIdx.x <= kProfileMaxBins) sE[threadIdx.x] = A.t.E[threadIdx.x];
#pragma unroll
    for (int ch = 0; ch < kProfileChannels; ++ch)
        sAcc[wave][ch][lane] = 0.0;
    __syncthreads(); // the only block barrier: the table is read-only from here on

    const int64_t sgi = int64_t(blockIdx.x) * kProfWaves + wave;
    int64_t c, h0, h1, hEnd;
    if (!profileSegment(A, sgi, c, h0, h1, hEnd)) return;
    const int nb      = A.t.nb;
    const bool hasV   = A.f.vx != nullptr, hasU = A.f.u != nullptr;
    const double cX = A.cxyz[3 * c], cY = A.cxyz[3 * c + 1], cZ = A.cxyz[3 * c + 2];
    const double Vx = A.vc ? A.vc[3 * c] : 0.0, Vy = A.vc ? A.vc[3 * c + 1] : 0.0, Vz = A.vc ? A.vc[3 * c + 2] : 0.0;
    double total = 0.0;

    for (int64_t base = h0; base < h1; base += kWave)
    {
        const int64_t i = base + lane;
        const bool in   = i < h1;
        double t[kProfileChannels] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        int bin = -1;
        if (in)
        {
            const int64_t e = clampQ(A.hperm[i], 0, A.H - 1);
            const int64_t p = clampQ(A.pidx[e], 0, A.ns - 1);
            const int64_t j = clampQ(A.perm[p], 0, A.np - 1);
            const double m  = A.f.m[j];
            bin  = profileBin(sE, nb, keyOf(A.keys[i]));
            t[0] = 1.0;
            t[1] = m;
            if (hasV)
            {
                double d[3], d2;
                pairSeparation(cX, cY, cZ, A.xs[p], A.ys[p], A.zs[p], A.box, d, d2);
                profileVelocityTerms(m, d, d2, A.f.vx[j] - Vx, A.f.vy[j] - Vy, A.f.vz[j] - Vz, t + 2);
            }
            if (hasU) t[5] = m * A.f.u[j];
            A.hmass[i] = m;
        }
        total += readLaneD(waveInclusiveSum(t[1], lane), kWave - 1);

        // bins are contiguous lane runs: a segmented scan, then the last lane of a run adds it to the wave's row
#pragma unroll
        for (int o = 1; o < kWave; o <<= 1)
        {
            const bool same = __shfl_up(bin, o) == bin && lane >= o;
            const double a0 = __shfl_up(t[0], o), a1 = __shfl_up(t[1], o);
            if (same) t[0] += a0, t[1] += a1;
            if (hasV)
            {
                const double a2 = __shfl_up(t[2], o), a3 = __shfl_up(t[3], o), a4 = __shfl_up(t[4], o);
                if (same) t[2] += a2, t[3] += a3, t[4] += a4;
            }
            if (hasU)
            {
                const double a5 = __shfl_up(t[5], o);
                if (same) t[5] += a5;
            }
        }
        const int next = __shfl_down(bin, 1);
        if (bin >= 0 && (lane == kWave - 1 || next != bin))
        {
#pragma unroll
            for (int ch = 0; ch < kProfileChannels; ++ch)
                sAcc[wave][ch][bin] += t[ch];
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    if (lane < nb)
    {
#pragma unroll
        for (int ch = 0; ch < kProfileChannels; ++ch)
            A.partial[(sgi * kProfileChannels + ch) * nb + lane] = sAcc[wave][ch][lane];
    }
    if (lane == 0) A.segMass[sgi] = total;
}

//! thread (centre, bin): the partial rows added in segment order; the thread of bin 0 also turns the segment masses
//! into carried-in masses and writes the centre's hit count
__global__ void __launch_bounds__(256) profileCombineKernel(ProfileReduceArgs A)
{
    const int nb    = A.t.nb;
    const int64_t q = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (q >= A.C * nb) return;
    const int64_t c = q / nb;
    const int bin   = int(q % nb);
    const int64_t s0 = clampQ(A.segOff[c], 0, A.U), s1 = clampQ(A.segOff[c + 1], s0, A.U);
    double acc[kProfileChannels] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int64_t sg = s0; sg < s1; ++sg)
#pragma unroll
        for (int ch = 0; ch < kProfileChannels; ++ch)
            acc[ch] += A.partial[(sg * kProfileChannels + ch) * nb + bin];
    A.count[q] = int64_t(acc[0]); // (whole numbers below 2^31: exact)
#pragma unroll
    for (int ch = 1; ch < kProfileChannels; ++ch)
        A.sums[(ch - 1) * A.C * nb + q] = acc[ch];
    if (bin == 0)
    {
        double run = 0.0;
        for (int64_t sg = s0; sg < s1; ++sg)
        {
            A.carry[sg] = run;
            run += A.segMass[sg];
        }
        A.hits[c] = A.start[c + 1] - A.start[c];
    }
}

__global__ void __launch_bounds__(kProfBlock) profileCrossKernel(ProfileReduceArgs A)
{
    const int lane    = laneId();
    const int64_t sgi = int64_t(blockIdx.x) * kProfWaves + (threadIdx.x >> 6);
    int64_t c, h0, h1, hEnd;
    if (!profileSegment(A, sgi, c, h0, h1, hEnd)) return; // (no block barrier in this kernel)
    double baseM = A.carry[sgi];
    int64_t bestQ = -1; // lane t: the outermost crossing of threshold t in this segment
    double bestM  = 0.0;
    for (int64_t base = h0; base < h1; base += kWave)
    {
        const int64_t i = base + lane;
        const bool in   = i < h1;
        const uint64_t key = in ? A.keys[i] : 0;
        const double pre   = waveInclusiveSum(in ? A.hmass[i] : 0.0, lane);
        const double M     = baseM + pre;
        const bool runEnd  = in && (i + 1 >= hEnd || A.keys[i + 1] != key);
        const float k      = keyOf(key);
        for (int t = 0; t < A.T; ++t)
        {
            const uint64_t bm = ballot(runEnd && M >= profileSphereMass(A.rho[t], k));
            if (bm)
            {
                const int top   = 63 - clz64(bm);
                const double Mq = readLaneD(M, top);
                if (lane == t) bestQ = base + top, bestM = Mq;
            }
        }
        baseM += readLaneD(pre, kWave - 1);
    }
    if (lane < A.T)
    {
        A.segQ[sgi * kProfileMaxThresholds + lane] = bestQ;
        A.segM[sgi * kProfileMaxThresholds + lane] = bestM;
    }
}

//! thread (centre, threshold): the outermost crossing over the centre's segments
__global__ void __launch_bounds__(256) profilePickKernel(ProfileReduceArgs A)
{
    const int64_t q = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (q >= A.C * A.T) return;
    const int64_t c = q / A.T;
    const int t     = int(q % A.T);
    const int64_t s0 = clampQ(A.segOff[c], 0, A.U), s1 = clampQ(A.segOff[c + 1], s0, A.U);
    const int64_t b = clampQ(A.start[c], 0, A.H), hEnd = clampQ(A.start[c + 1], b, A.H);
    double R = nan(""), M = nan("");
    int64_t N = 0;
    bool trunc = false;
    for (int64_t sg = s1 - 1; sg >= s0; --sg)
    {
        const int64_t hq = A.segQ[sg * kProfileMaxThresholds + t];
        if (hq < 0) continue;
        const int64_t h = clampQ(hq, b, hEnd - 1);
        R     = profileRadius(keyOf(A.keys[h]));
        M     = A.segM[sg * kProfileMaxThresholds + t];
        N     = h - b + 1;
        trunc = h == hEnd - 1;
        break;
    }
    A.soR[q]     = R;
    A.soM[q]     = M;
    A.soN[q]     = N;
    A.soTrunc[q] = trunc ? 1 : 0;
}

} // namespace

void profilePlan(int64_t C, int64_t np, const double* cxyz, const FofGrid& g, int seg, const FofBuffers& B,
                 const ProfileBuffers& P, hipStream_t s)
{
    if (C < 1 || C > kProfileMaxCentres) throw std::invalid_argument("profiles: between 1 and 2^24 centres");
    if (np < 1 || np > kFofMaxN) throw std::invalid_argument("profiles: between 1 and 2^30 particles");
    if (seg < kWave || seg % kWave) throw std::invalid_argument("profiles: the segment must be a multiple of 64");
    const int64_t n = C * kProfileSlots + 1;
    profileSlotsKernel<<<gridFor(n, 256), 256, 0, s>>>(C, np, cxyz, g, seg, B.counts, B.cellStart, B.cellKey, P.crec,
                                                       P.slotLo, P.slotHi, P.itemOff);
    SPHX_LAUNCH_CHECK();
    exclusiveScanI64(P.itemOff, P.itemOff, n, P.tmp, P.tmpBytes, s);
}

void profileHits(bool write, int64_t C, int64_t ns, int64_t nItems, int64_t H, const double* cxyz, const Box& box,
                 const FofGrid& g, const ProfileTables& t, int seg, const FofBuffers& B, const PairSorted& S,
                 const ProfileBuffers& P, int64_t* itemHits, uint64_t* keys, int32_t* pidx, unsigned long long* stats,
                 hipStream_t s)
{
    if (C < 1 || C > kProfileMaxCentres || ns < 0 || ns > kFofMaxN || nItems < 0 || H < 0 || H > kProfileMaxHits ||
        nItems > C * (kProfileSlots + ns / seg))
        throw std::invalid_argument("profiles: inconsistent counts");
    if (seg < kWave || seg % kWave) throw std::invalid_argument("profiles: the segment must be a multiple of 64");
    if (nItems == 0 || (write && H == 0)) return;
    const ProfileHitArgs A{g,        box,      t.cutHi,   t.E[t.nb], seg,  int(ns), C,    nItems, H,    P.crec, cxyz,
                           P.slotLo, P.slotHi, P.itemOff, B.rec,     S.x,  S.y,     S.z,  itemHits, keys, pidx, stats};
    const unsigned blocks = gridFor(nItems, kProfWaves);
    if (write) profileHitKernel<true><<<blocks, kProfBlock, 0, s>>>(A);
    else
    {
        profileHitKernel<false><<<blocks, kProfBlock, 0, s>>>(A);
        SPHX_LAUNCH_CHECK();
        exclusiveScanI64(itemHits, itemHits, nItems + 1, P.tmp, P.tmpBytes, s);
    }
    SPHX_LAUNCH_CHECK();
}

int64_t profileMaxSegments(int64_t C, int64_t H, int seg) { return C + H / seg; }

void profileReduce(int64_t C, int64_t H, int64_t np, int64_t ns, const Box& box, const ProfileTables& t, int T,
                   const double* rho, int seg, const uint64_t* keysSorted, const int32_t* hperm, const int32_t* pidx,
                   const int32_t* perm, const PairSorted& S, const ProfileFields& f, const double* cxyz,
                   const double* vc, const ProfileWork& W, const ProfileOut& O, void* tmp, size_t tmpBytes,
                   hipStream_t s)
{
    if (C < 1 || C > kProfileMaxCentres || H < 1 || H > kProfileMaxHits || ns < 1 || ns > np || np > kFofMaxN)
        throw std::invalid_argument("profiles: inconsistent counts");
    if (T < 0 || T > kProfileMaxThresholds) throw std::invalid_argument("profiles: at most 8 thresholds");
    if (seg < kWave || seg % kWave) throw std::invalid_argument("profiles: the segment must be a multiple of 64");
    if (!f.m || (f.vx && (!f.vy || !f.vz))) throw std::invalid_argument("profiles: a field is missing");
    ProfileReduceArgs A{};
    A.box = box, A.t = t, A.T = T, A.seg = seg;
    for (int i = 0; i < T; ++i)
        A.rho[i] = rho[i];
    A.C = C, A.H = H, A.U = profileMaxSegments(C, H, seg), A.np = np, A.ns = ns;
    A.keys = keysSorted, A.hperm = hperm, A.pidx = pidx, A.perm = perm;
    A.xs = S.x, A.ys = S.y, A.zs = S.z, A.f = f, A.cxyz = cxyz, A.vc = vc;
    A.start = W.start, A.segOff = W.segOff, A.partial = W.partial, A.segMass = W.segMass, A.carry = W.carry;
    A.hmass = W.hmass, A.segQ = W.segQ, A.segM = W.segM;
    A.count = O.count, A.sums = O.sums, A.soR = O.soR, A.soM = O.soM, A.soN = O.soN, A.soTrunc = O.soTrunc;
    A.hits = O.hits;
    profileStartsKernel<<<gridFor(C + 1, 256), 256, 0, s>>>(A);
    SPHX_LAUNCH_CHECK();
    exclusiveScanI64(W.segOff, W.segOff, C + 1, tmp, tmpBytes, s);
    // the segment count stays on the device: the grids cover the bound U = C + H / seg, a wave beyond the count returns
    const unsigned blocks = gridFor(A.U, kProfWaves);
    profileSumKernel<<<blocks, kProfBlock, 0, s>>>(A);
    SPHX_LAUNCH_CHECK();
    profileCombineKernel<<<gridFor(C * t.nb, 256), 256, 0, s>>>(A);
    SPHX_LAUNCH_CHECK();
    if (T == 0) return;
    profileCrossKernel<<<blocks, kProfBlock, 0, s>>>(A);
    SPHX_LAUNCH_CHECK();
    profilePickKernel<<<gridFor(C * T, 256), 256, 0, s>>>(A);
    SPHX_LAUNCH_CHECK();
}

SPHX_DCHECK_READER(dcheckProfiles)

} // namespace sphx::hip
