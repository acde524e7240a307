/*! Barnes-Hut self-gravity on gfx950: multipole upsweep, wave64 group traversal, direct sum.
 *
 * Parity: reference ryoanji/src/ryoanji/nbody/upwardpass.cuh:44-231 (computeLeafMultipoles, upsweepMultipoles
 * per level), nbody/traversal.cuh:60-526 (traverse: warp per target group, breadth-first with approx (M2P) and
 * body (P2P) queues, potential reduction), nbody/direct.cuh:44-112 (O(N^2) tiled direct sum).
 *
 * Design: one wave = 64 SFC-consecutive targets. The node stack lives in LDS; MAC-accepted nodes are queued in an
 * LDS M2P list, the particles of MAC-failing leaves in an LDS P2P list; both are flushed whenever they fill. M2P
 * node data are wave-uniform scalar loads, pipelined one node ahead. P2P sources are staged 64 at a time in LDS
 * (fp32, relative to the group center) and evaluated as 64x16 target-source tiles on the matrix cores:
 * v_mfma_f32_16x16x4_f32 forms the squared distances and the softening radii (h_i + h_j)^2, the VALU does the
 * rsqrt and accumulates the weights (see P2PTarget).
 */
#include <cfloat>

#include "common.h"
#include "gravity_eval.h"
#include "hip_api.h"
#include "sphx/gravity.hpp"

namespace sphx::hip
{

//! @brief leaf mass centers and traceless quadrupoles (p2m), one wave per node: the lanes read the leaf's particles
//!        coalesced and the moments are wave reductions (a thread per leaf looping over its particles touched 64
//!        cache lines per load instruction)
__global__ __launch_bounds__(256) void gravityLeavesKernel(const int32_t* __restrict__ n2l, int64_t N,
                                                           const int32_t* __restrict__ ns,
                                                           const int32_t* __restrict__ ne,
                                                           const double* __restrict__ x, const double* __restrict__ y,
                                                           const double* __restrict__ z, const float* __restrict__ m,
                                                           double* __restrict__ centers, Quadrupole* __restrict__ mp)
{
    const int64_t i = int64_t(blockIdx.x) * 4 + (threadIdx.x >> 6);
    if (i >= N || n2l[i] < 0) return; // wave-uniform
    const int lane = threadIdx.x & 63;
    const int32_t a = ns[i], b = ne[i];
    double c[4] = {0, 0, 0, 0};
    for (int32_t p = a + lane; p < b; p += 64)
    {
        double mi = m[p];
        c[0] += mi * x[p];
        c[1] += mi * y[p];
        c[2] += mi * z[p];
        c[3] += mi;
    }
    for (int k = 0; k < 4; ++k)
        c[k] = waveSum(c[k]);
    const double inv    = c[3] != 0 ? 1.0 / c[3] : 0.0;
    const double com[3] = {c[0] * inv, c[1] * inv, c[2] * inv};
    double acc[6] = {0, 0, 0, 0, 0, 0};
    for (int32_t p = a + lane; p < b; p += 64)
    {
        double rx = x[p] - com[0], ry = y[p] - com[1], rz = z[p] - com[2], mi = m[p];
        acc[0] += rx * rx * mi;
        acc[1] += rx * ry * mi;
        acc[2] += rx * rz * mi;
        acc[3] += ry * ry * mi;
        acc[4] += ry * rz * mi;
        acc[5] += rz * rz * mi;
    }
    for (int k = 0; k < 6; ++k)
        acc[k] = waveSum(acc[k]);
    if (lane != 0) return;
    const double tr = acc[0] + acc[3] + acc[5];
    Quadrupole q;
    q.q[qMass]         = MT(c[3]);
    q.q[qXX]           = MT(3 * acc[0] - tr);
    q.q[qYY]           = MT(3 * acc[3] - tr);
    q.q[qZZ]           = MT(3 * acc[5] - tr);
    q.q[qXY]           = MT(3 * acc[1]);
    q.q[qXZ]           = MT(3 * acc[2]);
    q.q[qYZ]           = MT(3 * acc[4]);
    q.q[qTrace]        = MT(tr);
    mp[i]              = q;
    centers[4 * i + 0] = com[0];
    centers[4 * i + 1] = com[1];
    centers[4 * i + 2] = com[2];
    centers[4 * i + 3] = c[3];
}

__global__ void gravityUpsweepKernel(int64_t a, int64_t b, const int32_t* __restrict__ n2l,
                                     const int32_t* __restrict__ child, double* __restrict__ centers,
                                     Quadrupole* __restrict__ mp)
{
    int64_t i = a + int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= b || n2l[i] >= 0) return;
    int32_t co  = child[i];
    double c[4] = {0, 0, 0, 0};
    for (int k = 0; k < 8; ++k)
    {
        const double* cc = centers + 4 * (co + k);
        c[0] += cc[3] * cc[0];
        c[1] += cc[3] * cc[1];
        c[2] += cc[3] * cc[2];
        c[3] += cc[3];
    }
    double inv    = c[3] != 0 ? 1.0 / c[3] : 0.0;
    double com[3] = {c[0] * inv, c[1] * inv, c[2] * inv};
    Quadrupole q{};
    for (int k = 0; k < 8; ++k)
    {
        const double* cc = centers + 4 * (co + k);
        addQuadrupole(q, com[0] - cc[0], com[1] - cc[1], com[2] - cc[2], mp[co + k]);
    }
    mp[i]              = q;
    centers[4 * i + 0] = com[0];
    centers[4 * i + 1] = com[1];
    centers[4 * i + 2] = com[2];
    centers[4 * i + 3] = c[3];
}

__global__ void gravitySetMacKernel(int64_t N, const KeyT* __restrict__ prefixes, Box box, int kind, double invTheta,
                                    double* __restrict__ centers)
{
    int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= N) return;
    double gc[3], gs[3];
    nodeGeometry(kind, prefixes[i], box, gc, gs);
    double* c = centers + 4 * i;
    if (c[3] == 0)
    {
        c[0] = gc[0];
        c[1] = gc[1];
        c[2] = gc[2];
        c[3] = 0;
    }
    else { c[3] = vecMacR2(c, gc, gs, invTheta); }
}

/*! @brief the whole upsweep in one launch (leaves, every internal level, vector-MAC radii): a wave per leaf computes
 *         its multipole like gravityLeavesKernel; then lane 0 climbs: it counts itself into the parent's arrival
 *         counter (release fence first) and the eighth sibling to arrive (acquire fence) forms the parent from its
 *         children (agent-scope loads: the children were written by waves on other XCDs), sets the children's MAC
 *         radii (they are not read again) and climbs on. The counter is re-armed to 0 by its eighth arrival. Replaces
 *         2 + depth launches (the level loop of ops/gravity.py) that at small per-rank sizes cost more host time than
 *         GPU time.
 */
__device__ __forceinline__ double ldAgent(const double* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ float ldAgent(const float* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ void setMacOf(int64_t i, const double c[4], const KeyT* prefixes, const Box& box, int kind,
                                         double invTheta, double* centers)
{
    double gc[3], gs[3];
    nodeGeometry(kind, prefixes[i], box, gc, gs);
    double* o = centers + 4 * i;
    if (c[3] == 0)
    {
        o[0] = gc[0], o[1] = gc[1], o[2] = gc[2], o[3] = 0;
    }
    else { o[3] = vecMacR2(c, gc, gs, invTheta); }
}

__global__ __launch_bounds__(256) void gravityUpsweepFusedKernel(const int32_t* __restrict__ n2l, int64_t N,
                                                                 const int32_t* __restrict__ ns,
                                                                 const int32_t* __restrict__ ne,
                                                                 const double* __restrict__ x,
                                                                 const double* __restrict__ y,
                                                                 const double* __restrict__ z,
                                                                 const float* __restrict__ m,
                                                                 const int32_t* __restrict__ child,
                                                                 const int32_t* __restrict__ parents,
                                                                 const KeyT* __restrict__ prefixes, Box box, int kind,
                                                                 double invTheta, double* centers, Quadrupole* mp,
                                                                 unsigned* cnt)
{
    const int64_t i = int64_t(blockIdx.x) * 4 + (threadIdx.x >> 6);
    if (i >= N || n2l[i] < 0) return; // wave-uniform
    const int lane = threadIdx.x & 63;
    const int32_t a = ns[i], b = ne[i];
    double c[4] = {0, 0, 0, 0};
    for (int32_t p = a + lane; p < b; p += 64)
    {
        double mi = m[p];
        c[0] += mi * x[p];
        c[1] += mi * y[p];
        c[2] += mi * z[p];
        c[3] += mi;
    }
    for (int k = 0; k < 4; ++k)
        c[k] = waveSum(c[k]);
    const double inv    = c[3] != 0 ? 1.0 / c[3] : 0.0;
    const double com[3] = {c[0] * inv, c[1] * inv, c[2] * inv};
    double acc[6] = {0, 0, 0, 0, 0, 0};
    for (int32_t p = a + lane; p < b; p += 64)
    {
        double rx = x[p] - com[0], ry = y[p] - com[1], rz = z[p] - com[2], mi = m[p];
        acc[0] += rx * rx * mi;
        acc[1] += rx * ry * mi;
        acc[2] += rx * rz * mi;
        acc[3] += ry * ry * mi;
        acc[4] += ry * rz * mi;
        acc[5] += rz * rz * mi;
    }
    for (int k = 0; k < 6; ++k)
        acc[k] = waveSum(acc[k]);
    if (lane != 0) return;
    const double tr = acc[0] + acc[3] + acc[5];
    Quadrupole q;
    q.q[qMass]         = MT(c[3]);
    q.q[qXX]           = MT(3 * acc[0] - tr);
    q.q[qYY]           = MT(3 * acc[3] - tr);
    q.q[qZZ]           = MT(3 * acc[5] - tr);
    q.q[qXY]           = MT(3 * acc[1]);
    q.q[qXZ]           = MT(3 * acc[2]);
    q.q[qYZ]           = MT(3 * acc[4]);
    q.q[qTrace]        = MT(tr);
    mp[i]              = q;
    double own[4]      = {com[0], com[1], com[2], c[3]};
    centers[4 * i + 0] = own[0];
    centers[4 * i + 1] = own[1];
    centers[4 * i + 2] = own[2];
    centers[4 * i + 3] = own[3];

    int64_t node = i;
    while (node > 0)
    {
        const int32_t pn = parents[(node - 1) / 8];
        __threadfence(); // release: this node's multipole before the arrival
        if (atomicAdd(&cnt[pn], 1u) != 7u) return;
        cnt[pn] = 0u;    // every sibling has arrived: re-armed for the next launch
        __threadfence(); // acquire: the siblings' multipoles
        const int32_t co = child[pn];
        double ch[8][4];
        double s[4] = {0, 0, 0, 0};
        for (int k = 0; k < 8; ++k)
        {
            for (int d = 0; d < 4; ++d)
                ch[k][d] = ldAgent(centers + 4 * (co + k) + d);
            s[0] += ch[k][3] * ch[k][0];
            s[1] += ch[k][3] * ch[k][1];
            s[2] += ch[k][3] * ch[k][2];
            s[3] += ch[k][3];
        }
        const double iv = s[3] != 0 ? 1.0 / s[3] : 0.0;
        const double pc[3] = {s[0] * iv, s[1] * iv, s[2] * iv};
        Quadrupole pq{};
        for (int k = 0; k < 8; ++k)
        {
            Quadrupole cq;
            const float* src = reinterpret_cast<const float*>(mp + co + k);
            for (int e = 0; e < 8; ++e)
                cq.q[e] = ldAgent(src + e);
            addQuadrupole(pq, pc[0] - ch[k][0], pc[1] - ch[k][1], pc[2] - ch[k][2], cq);
        }
        mp[pn]              = pq;
        centers[4 * pn + 0] = pc[0];
        centers[4 * pn + 1] = pc[1];
        centers[4 * pn + 2] = pc[2];
        centers[4 * pn + 3] = s[3];
        for (int k = 0; k < 8; ++k)
            setMacOf(co + k, ch[k], prefixes, box, kind, invTheta, centers);
        own[0] = pc[0], own[1] = pc[1], own[2] = pc[2], own[3] = s[3];
        node = pn;
    }
    setMacOf(0, own, prefixes, box, kind, invTheta, centers); // the root (reached by exactly one climber)
}

void gravityUpsweepFused(const int32_t* n2l, int64_t N, const int32_t* ns, const int32_t* ne, const double* x,
                         const double* y, const double* z, const float* m, const int32_t* child,
                         const int32_t* parents, const KeyT* prefixes, const Box& box, int kind, double invTheta,
                         double* centers, void* mp, unsigned* cnt, hipStream_t s)
{
    if (N <= 0) return;
    gravityUpsweepFusedKernel<<<unsigned((N + 3) / 4), 256, 0, s>>>(n2l, N, ns, ne, x, y, z, m, child, parents,
                                                                    prefixes, box, kind, invTheta, centers,
                                                                    (Quadrupole*)mp, cnt);
    SPHX_LAUNCH_CHECK();
}

void gravityLeaves(const int32_t* n2l, int64_t N, const int32_t* ns, const int32_t* ne, const double* x,
                   const double* y, const double* z, const float* m, double* centers, void* mp, hipStream_t s)
{
    if (N <= 0) return;
    gravityLeavesKernel<<<unsigned((N + 3) / 4), 256, 0, s>>>(n2l, N, ns, ne, x, y, z, m, centers, (Quadrupole*)mp);
    SPHX_LAUNCH_CHECK();
}

void gravityUpsweepLevel(int64_t a, int64_t b, const int32_t* n2l, const int32_t* child, double* centers, void* mp,
                         hipStream_t s)
{
    if (b <= a) return;
    gravityUpsweepKernel<<<gridFor(b - a, 256), 256, 0, s>>>(a, b, n2l, child, centers, (Quadrupole*)mp);
    SPHX_LAUNCH_CHECK();
}

void gravitySetMac(int64_t N, const KeyT* prefixes, const Box& box, int kind, double invTheta, double* centers,
                   hipStream_t s)
{
    gravitySetMacKernel<<<gridFor(N, 256), 256, 0, s>>>(N, prefixes, box, kind, invTheta, centers);
    SPHX_LAUNCH_CHECK();
}

__global__ void gravityRecordsKernel(int64_t n, const double* __restrict__ x, const double* __restrict__ y,
                                     const double* __restrict__ z, const float* __restrict__ h,
                                     const double* __restrict__ mm, int4* __restrict__ rec)
{
    const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const GravFrame f = gravFrame(mm);
    rec[i] = make_int4(int(gravQuant(x[i], f, 0)), int(gravQuant(y[i], f, 1)), int(gravQuant(z[i], f, 2)),
                       __float_as_int(h[i]));
}

__global__ void gravityNodeRecordsKernel(int64_t N, const double* __restrict__ centers,
                                         const Quadrupole* __restrict__ mp, const double* __restrict__ mm,
                                         float4* __restrict__ a, float4* __restrict__ b, float2* __restrict__ c)
{
    const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const GravFrame f = gravFrame(mm);
    const double* cc  = centers + 4 * i;
    const float4* q   = reinterpret_cast<const float4*>(mp + i);
    const float4 q0 = q[0], q1 = q[1]; // M, qxx, qxy, qxz | qyy, qyz, qzz, (trace)
    a[i] = make_float4(float(cc[0] - f.org[0]), float(cc[1] - f.org[1]), float(cc[2] - f.org[2]), q0.x);
    b[i] = make_float4(q0.y, q0.z, q0.w, q1.x);
    c[i] = make_float2(q1.y, q1.z);
}

__global__ __launch_bounds__(256) void gravityListKernel(int64_t first, int64_t last, GravTree t,
                                                         const double* __restrict__ x, const double* __restrict__ y,
                                                         const double* __restrict__ z, GravSlabs S,
                                                         unsigned long long* __restrict__ stats,
                                                         int32_t* __restrict__ spillList, int stackCap)
{
    __shared__ int32_t stackAll[kGWaves][kGStack];
    const int lane          = laneId();
    const int wave          = threadIdx.x >> 6;
    const int64_t numGroups = (last - first + 63) / 64;
    const int64_t g         = int64_t(xcdRemap(blockIdx.x, gridDim.x)) * kGWaves + wave;
    if (g >= numGroups) return;
    int32_t* stack   = stackAll[wave];
    const int64_t ii = min(first + g * 64 + lane, last - 1);
    double ac[3], as[3], bc[3], bs[3];
    halfBoxes(x[ii], y[ii], z[ii], ac, as, bc, bs);

    // M2P entries of both halves fill the M2P slab from the front, those of half A only from its back; opened leaves
    // fill the leaf slab from the front, M2P entries of half B only from its back. The evaluation kernels run each
    // class as its own pass (no per-entry masks in the inner loops).
    int32_t* ml = S.mlist + g * S.capM;
    int32_t* ll = S.llist + g * S.capL;
    int sp = 1, nm = 0, nA = 0, nB = 0, nl = 0, np = 0;
    bool ok = true, slabFull = false;
    if (lane == 0) stack[0] = int32_t((kHalfA | kHalfB) << kTagShift); // the root, walked by both halves
    gWaveSync<false>();
    while (sp > 0)
    {
        int32_t nd;
        unsigned mM2P, mLeaf;
        if (!popAndTestHalves<false>(t, stack, sp, stackCap, ac, as, bc, bs, nd, mM2P, mLeaf))
        {
            ok = false;
            break;
        }
        const bool isBoth = mM2P == (kHalfA | kHalfB), isA = mM2P == kHalfA, isB = mM2P == kHalfB;
        const bool isLeaf = mLeaf != 0;
        const uint64_t b3 = ballot(isBoth), bA = ballot(isA), bB = ballot(isB), bl = ballot(isLeaf);
        const int c3 = __popcll(b3), cA = __popcll(bA), cB = __popcll(bB), cl = __popcll(bl);
        // a group that outgrows its slabs finishes the traversal counting only, so the host learns the whole
        // demand ([6] leaf slab, [7] M2P slab) and sizes the slabs for it in one step (the group itself falls back)
        slabFull = slabFull || nm + nA + c3 + cA > S.capM || nl + nB + cl + cB > S.capL;
        if (!slabFull)
        {
            const uint64_t lt = lanemaskLt();
            if (isBoth) ml[nm + __popcll(b3 & lt)] = nd;
            if (isA) ml[S.capM - 1 - nA - __popcll(bA & lt)] = nd;
            if (isB) ll[S.capL - 1 - nB - __popcll(bB & lt)] = nd;
            if (isLeaf)
            {
                ll[nl + __popcll(bl & lt)] = nd | int32_t(mLeaf << kTagShift);
                np += (t.ne[nd] - t.ns[nd]) * __popc(mLeaf); // half-group units
            }
        }
        nm += c3;
        nA += cA;
        nB += cB;
        nl += cl;
        gWaveSync<false>();
    }
    if (slabFull)
    {
        if (lane == 0)
        {
            atomicMax(&stats[6], (unsigned long long)(nl + nB));
            atomicMax(&stats[7], (unsigned long long)(nm + nA));
        }
        ok = false;
    }
    np = waveSum(np);
    if (lane == 0)
    {
        S.counts[4 * g]     = ok ? nm : -1;
        S.counts[4 * g + 1] = ok ? nl : -1;
        S.counts[4 * g + 2] = ok ? nA : 0;
        S.counts[4 * g + 3] = ok ? nB : 0;
        S.pcount[g]         = ok ? (np + 1) / 2 : 0;
        if (!ok) spillList[atomicAdd(&stats[5], 1ull)] = int32_t(g);
    }
}

/* Cost-ordered dispatch of the evaluation kernels. A group's P2P (M2P) work is its particle (node) count, which
 * varies ~7x between Evrard groups (mean 3.8 k P2P per target, max 27 k): dispatched in SFC order, the heaviest
 * groups can start late and leave most SIMDs idle at the end of the kernel. The groups are therefore handed out
 * heaviest first (longest-processing-time order), binned by work with 4 bins per octave: a histogram kernel and a
 * scatter kernel (order within a bin is arbitrary; every group is evaluated independently, results are unchanged).
 */
constexpr int kOrdBins = 128;

//! @brief bin of a group's work, heaviest bin first (0); empty and fallback groups (count <= 0) last
__device__ __forceinline__ int costBin(int c)
{
    if (c <= 0) return kOrdBins - 1;
    const unsigned u = unsigned(c);
    const int e      = 31 - __clz(u);
    const int sub    = e >= 2 ? int(u >> (e - 2)) & 3 : 0;
    return kOrdBins - 2 - min(4 * e + sub, kOrdBins - 2);
}

//! @brief work of group g in evaluation kernel k (0: M2P nodes, 1: P2P particles)
__device__ __forceinline__ int groupWork(const GravSlabs& S, int64_t g, int k)
{
    const int nm = S.counts[4 * g];
    return k == 0 ? (nm < 0 ? nm : nm + (S.counts[4 * g + 2] + S.counts[4 * g + 3]) / 2)
                  : (nm < 0 ? 0 : S.pcount[g]);
}

__global__ __launch_bounds__(256) void gravityOrderHistKernel(int64_t groups, GravSlabs S, int32_t* __restrict__ hist)
{
    __shared__ int32_t h[2 * kOrdBins];
    for (int k = threadIdx.x; k < 2 * kOrdBins; k += blockDim.x)
        h[k] = 0;
    __syncthreads();
    for (int64_t g = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; g < groups; g += int64_t(gridDim.x) * blockDim.x)
    {
        atomicAdd(&h[costBin(groupWork(S, g, 0))], 1);
        atomicAdd(&h[kOrdBins + costBin(groupWork(S, g, 1))], 1);
    }
    __syncthreads();
    for (int k = threadIdx.x; k < 2 * kOrdBins; k += blockDim.x)
        if (h[k]) atomicAdd(&hist[k], h[k]);
}

//! @brief order[k][pos] = group, bins in ascending order (heaviest first); hist/cursor: 2 x kOrdBins (cursor zeroed).
//!        Ranks within a bin are taken in LDS per block and one global atomic per (block, bin) reserves their range:
//!        one global atomic per group and kernel on a handful of hot bins took ~1 ms for 74 k groups.
__global__ __launch_bounds__(256) void gravityOrderScatterKernel(int64_t groups, GravSlabs S,
                                                                 const int32_t* __restrict__ hist,
                                                                 int32_t* __restrict__ cursor,
                                                                 int32_t* __restrict__ order)
{
    __shared__ int32_t off[2 * kOrdBins], cnt[2 * kOrdBins], base[2 * kOrdBins];
    if (threadIdx.x < 2)
    {
        int s = 0;
        for (int b = 0; b < kOrdBins; ++b)
        {
            off[threadIdx.x * kOrdBins + b] = s;
            s += hist[threadIdx.x * kOrdBins + b];
        }
    }
    for (int64_t g0 = int64_t(blockIdx.x) * blockDim.x; g0 < groups; g0 += int64_t(gridDim.x) * blockDim.x)
    {
        for (int k = threadIdx.x; k < 2 * kOrdBins; k += blockDim.x)
            cnt[k] = 0;
        __syncthreads();
        const int64_t g = g0 + threadIdx.x;
        int b[2], r[2];
#pragma unroll
        for (int k = 0; k < 2; ++k)
        {
            b[k] = k * kOrdBins + (g < groups ? costBin(groupWork(S, g, k)) : 0);
            r[k] = g < groups ? atomicAdd(&cnt[b[k]], 1) : 0;
        }
        __syncthreads();
        for (int k = threadIdx.x; k < 2 * kOrdBins; k += blockDim.x)
            base[k] = cnt[k] ? atomicAdd(&cursor[k], cnt[k]) : 0;
        __syncthreads();
        if (g < groups)
        {
#pragma unroll
            for (int k = 0; k < 2; ++k)
                order[k * groups + off[b[k]] + base[b[k]] + r[k]] = int32_t(g);
        }
        __syncthreads();
    }
}

/* XCD-coherent cost order of the P2P kernel (variant -DSPHX_GRAV_SG_ORDER): the heaviest-first order of single groups
 * scatters the groups that run at the same time on one XCD over the whole domain, and their source particles miss in
 * its L2 (TCC hit rate 36 % on Evrard -n 200). Here the unit is a super-group of kSG = 16 SFC-consecutive groups (4 blocks, which share
 * most of their sources): super-groups are ranked by total work (same bins), rank r goes to XCD r % 8 as its
 * (r / 8)-th run of 4 consecutive blocks on that XCD (the dispatcher deals block b to XCD b % 8), so every XCD works
 * heaviest first through a balanced share while the 4 blocks of a super-group run side by side in one L2.
 * Measured (Evrard -n 200, gpurun_out/go4): L2 hit rate 36 -> 66 %, but P2P 9.07 -> 9.43 ms: the coarser unit balances
 * worse, and the misses were not what bounds the loop (profiles/r3_grav_pmc.md). Not the default.
 */
constexpr int kSG = 16;

__device__ __forceinline__ int sgWork(const GravSlabs& S, int64_t sg, int64_t groups)
{
    long long w = 0;
    for (int64_t g = sg * kSG; g < min(groups, (sg + 1) * kSG); ++g)
        w += groupWork(S, g, 1);
    return int(min(w, (long long)INT32_MAX));
}

//! @brief grid (blocks) of the P2P kernel under the super-group order: whole runs of 4 blocks on all 8 XCDs
__host__ __device__ inline int64_t sgGridBlocks(int64_t groups)
{
    const int64_t nsg = (groups + kSG - 1) / kSG;
    return 8 * (kSG / kGWaves) * ((nsg + 7) / 8);
}

__global__ __launch_bounds__(256) void gravitySgHistKernel(int64_t groups, GravSlabs S, int32_t* __restrict__ hist)
{
    __shared__ int32_t h[kOrdBins];
    for (int k = threadIdx.x; k < kOrdBins; k += blockDim.x)
        h[k] = 0;
    __syncthreads();
    const int64_t nsg = (groups + kSG - 1) / kSG;
    for (int64_t sg = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; sg < nsg; sg += int64_t(gridDim.x) * blockDim.x)
        atomicAdd(&h[costBin(sgWork(S, sg, groups))], 1);
    __syncthreads();
    for (int k = threadIdx.x; k < kOrdBins; k += blockDim.x)
        if (h[k]) atomicAdd(&hist[k], h[k]);
}

__global__ __launch_bounds__(256) void gravitySgScatterKernel(int64_t groups, GravSlabs S,
                                                              const int32_t* __restrict__ hist,
                                                              int32_t* __restrict__ cursor,
                                                              int32_t* __restrict__ order)
{
    __shared__ int32_t off[kOrdBins], cnt[kOrdBins], base[kOrdBins];
    if (threadIdx.x == 0)
    {
        int s = 0;
        for (int b = 0; b < kOrdBins; ++b)
        {
            off[b] = s;
            s += hist[b];
        }
    }
    const int64_t nsg   = (groups + kSG - 1) / kSG;
    const int64_t slots = sgGridBlocks(groups) * kGWaves;
    for (int64_t s0 = int64_t(blockIdx.x) * blockDim.x; s0 < (nsg + 7) / 8 * 8; s0 += int64_t(gridDim.x) * blockDim.x)
    {
        for (int k = threadIdx.x; k < kOrdBins; k += blockDim.x)
            cnt[k] = 0;
        __syncthreads();
        const int64_t sg = s0 + threadIdx.x;
        const int b      = sg < nsg ? costBin(sgWork(S, sg, groups)) : 0;
        const int r0     = sg < nsg ? atomicAdd(&cnt[b], 1) : 0;
        __syncthreads();
        for (int k = threadIdx.x; k < kOrdBins; k += blockDim.x)
            base[k] = cnt[k] ? atomicAdd(&cursor[k], cnt[k]) : 0;
        __syncthreads();
        if (sg < nsg)
        {
            const int64_t r = off[b] + base[b] + r0;
            for (int t = 0; t < kSG / kGWaves; ++t)
            {
                const int64_t blk = 8 * ((kSG / kGWaves) * (r >> 3) + t) + (r & 7);
                for (int w = 0; w < kGWaves; ++w)
                {
                    const int64_t g = sg * kSG + t * kGWaves + w;
                    order[blk * kGWaves + w] = int32_t(g < groups ? g : groups);
                }
            }
        }
        else if (sg < (nsg + 7) / 8 * 8)
        {
            // the slots of the padding ranks (nsg .. multiple of 8) hold no group
            const int64_t r = sg;
            for (int t = 0; t < kSG / kGWaves; ++t)
            {
                const int64_t blk = 8 * ((kSG / kGWaves) * (r >> 3) + t) + (r & 7);
                for (int w = 0; w < kGWaves; ++w)
                    if (blk * kGWaves + w < slots) order[blk * kGWaves + w] = int32_t(groups);
            }
        }
        __syncthreads();
    }
}

/*! @brief M2P part of the evaluation (one wave per group): light on registers, so many waves per SIMD hide the
 *         LDS and transcendental latencies of the multipole loop
 */
__global__ __launch_bounds__(256, SPHX_M2P_WAVES) void gravityM2PKernel(int64_t first, int64_t last, GravTree t,
                                                           const double* __restrict__ x,
                                                           const double* __restrict__ y,
                                                           const double* __restrict__ z,
                                                           const float* __restrict__ h, const float* __restrict__ m,
                                                           float G, float* __restrict__ ax, float* __restrict__ ay,
                                                           float* __restrict__ az, double* __restrict__ ugrav,
                                                           double* __restrict__ out,
                                                           unsigned long long* __restrict__ stats, GravSlabs S,
                                                           const int32_t* __restrict__ order, int64_t numSlots,
                                                           NodeRecs R, const double* __restrict__ mm)
{
    __shared__ float4 stage[kGWaves][5 * 64];
    __shared__ double red[kGWaves];
    const int wave          = threadIdx.x >> 6;
    const int64_t numGroups = (last - first + 63) / 64;
    const int64_t g         = evalGroup(order, numSlots, numGroups);
    double upot             = 0;
    int nm                  = g < numGroups ? __builtin_amdgcn_readfirstlane(S.counts[4 * g]) : -1;
    SPHX_DCHECK(nm <= S.capM, 3);
#ifdef SPHX_DEVICE_CHECKS
    nm = min(nm, S.capM);
#endif
    if (nm >= 0)
    {
        const int nA = __builtin_amdgcn_readfirstlane(S.counts[4 * g + 2]);
        const int nB = __builtin_amdgcn_readfirstlane(S.counts[4 * g + 3]);
        EvalTarget e    = evalTarget(g, first, last, x, y, z, h);
        const P2PSrc fr = p2pSrc(nullptr, nullptr, mm, e.tc); // quantized group center
        M2PTarget T;
        m2pInit(T, e.xr + fr.dc[0], e.yr + fr.dc[1], e.zr + fr.dc[2]);
        // three passes: nodes of both halves, of half A only, of half B only
        evalM2PMfma<0, 4>(S.mlist + g * S.capM, nm, R, fr, stage[wave], T);
        evalM2PMfma<0, 2>(S.mlist + g * S.capM + S.capM - nA, nA, R, fr, stage[wave], T);
        evalM2PMfma<2, 4>(S.llist + g * S.capL + S.capL - nB, nB, R, fr, stage[wave], T);
        float acc[4] = {0, 0, 0, 0};
        m2pFinish(T, acc);
        gravityStore(g, first, last, acc, G, m, ax, ay, az, ugrav, stats, 0ull,
                     (unsigned long long)(nm + (nA + nB + 1) / 2), upot);
    }
    blockEnergy(upot, red, kGWaves, out);
}

#ifndef SPHX_P2P_WAVES
#define SPHX_P2P_WAVES 3 // waves per SIMD of the MFMA P2P kernel (4 spills registers)
#endif

//! @brief P2P part of the evaluation (one wave per group): leaf list -> particle list -> MFMA tiles
__global__ __launch_bounds__(256, SPHX_P2P_WAVES) void gravityP2PKernel(int64_t first, int64_t last, GravTree t,
                                                           const double* __restrict__ x,
                                                           const double* __restrict__ y,
                                                           const double* __restrict__ z,
                                                           const float* __restrict__ h, const float* __restrict__ m,
                                                           float G, float* __restrict__ ax, float* __restrict__ ay,
                                                           float* __restrict__ az, double* __restrict__ ugrav,
                                                           double* __restrict__ out,
                                                           unsigned long long* __restrict__ stats, GravSlabs S,
                                                           float4* __restrict__ pacc, const int4* __restrict__ rec,
                                                           const double* __restrict__ mm,
                                                           const int32_t* __restrict__ order, int64_t numSlots)
{
    __shared__ GravLds lds[kGWaves];
    __shared__ double red[kGWaves];
    const int lane          = laneId();
    const int wave          = threadIdx.x >> 6;
    const int64_t numGroups = (last - first + 63) / 64;
    const int64_t g         = evalGroup(order, numSlots, numGroups);
    double upot             = 0;
    const int nl            = g < numGroups ? __builtin_amdgcn_readfirstlane(S.counts[4 * g + 1]) : -1;
    if (nl >= 0)
    {
        GravLists L  = listsOf(lds[wave]);
        EvalTarget e = evalTarget(g, first, last, x, y, z, h);
        float acc[4] = {0, 0, 0, 0};
        const P2PSrc src = p2pSrc(rec, m, mm, e.tc);
        float txr, tyr, tzr;
        src.offset(min(first + g * 64 + lane, last - 1), txr, tyr, tzr);
        P2PTarget T;
        p2pInit(T, txr, tyr, tzr, e.hi);
        int np2 = 0; // applied sources in half-group units (2 per source of both halves)
        // windows of up to 255 opened leaves: sizes prefix-summed into LDS (plst holds the prefix (256) | the starts
        // (255)), the source indices generated per chunk (no expanded index list, no host-sized buffer). The window's
        // leaves are ordered by half mask (both | A only | B only), and each class runs as its own pass
        static_assert(kGP2P >= 2 * 256, "leaf window of the P2P kernel");
        const int32_t* ll = S.llist + g * S.capL;
        int32_t* pre      = L.plst;
        int32_t* st       = L.plst + 256;
        const uint64_t lt = lanemaskLt();
        for (int w0 = 0; w0 < nl; w0 += 255)
        {
            const int nw = min(255, nl - w0);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); // the previous window's reads are done
            int32_t a0[4], sz[4];
            unsigned hm[4];
#pragma unroll
            for (int b = 0; b < 4; ++b)
            {
                const int k      = 64 * b + lane;
                const int32_t e  = k < nw ? ll[w0 + k] : -1;
                const int32_t lf = e & kIdMask;
                hm[b]            = e != -1 ? tagOf(e) : 0u;
                a0[b]            = e != -1 ? t.ns[lf] : 0;
                sz[b]            = e != -1 ? t.ne[lf] - a0[b] : 0;
            }
            int run = 0, placed = 0, bound[4] = {0, 0, 0, 0}, first[3] = {0, 0, 0}; // per class: offset, leaf
            const unsigned order[3] = {kHalfA | kHalfB, kHalfA, kHalfB};
#pragma unroll
            for (int c = 0; c < 3; ++c)
            {
#pragma unroll
                for (int b = 0; b < 4; ++b)
                {
                    const bool sel    = hm[b] == order[c];
                    const uint64_t bs = ballot(sel);
                    if (bs == 0) continue;
                    const int s = sel ? sz[b] : 0;
                    int inc     = s; // inclusive wave scan of the selected sizes
                    for (int o = 1; o < 64; o <<= 1)
                    {
                        const int v = __shfl_up(inc, o);
                        if (lane >= o) inc += v;
                    }
                    if (sel)
                    {
                        const int k = placed + __popcll(bs & lt);
                        pre[k]      = run + inc - s;
                        st[k]       = a0[b];
                    }
                    run += __shfl(inc, 63);
                    placed += __popcll(bs);
                }
                bound[c + 1] = run;
                if (c < 2) first[c + 1] = placed;
            }
            if (lane == 0) pre[nw] = run;
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            flushP2P<kP2PBoth>(LeafCursor{pre, st, nw, 0, 0}, 0, bound[1], L, src, T);
            flushP2P<kP2PHalfA>(LeafCursor{pre, st, nw, first[1], bound[1]}, bound[1], bound[2] - bound[1], L, src,
                                T);
            flushP2P<kP2PHalfB>(LeafCursor{pre, st, nw, first[2], bound[2]}, bound[2], bound[3] - bound[2], L, src,
                                T);
            np2 += 2 * bound[1] + (bound[3] - bound[1]);
        }
        p2pFinish(T, acc);
        // [8]: chunks on the MFMA tile (low 32 bits) / on the VALU fallback (high 32 bits)
        if (lane == 0) atomicAdd(&stats[8], (unsigned long long)T.nMfma | ((unsigned long long)T.nValu << 32));
        unsigned long long totP2P = (unsigned long long)((np2 + 1) / 2);
        gravityStore(g, first, last, acc, G, m, ax, ay, az, ugrav, stats, totP2P, 0ull, upot, pacc);
    }
    else if (g < numGroups)
    {
        // fallback group: its P2P share comes from the fused kernel, which adds to ax directly
        const int64_t i = first + g * 64 + lane;
        if (i < last) pacc[i - first] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    blockEnergy(upot, red, kGWaves, out);
}

//! @brief add the P2P partials (kept apart from the M2P sums, optionally computed on a second stream) to the outputs
__global__ void gravityCombineKernel(int64_t first, int64_t last, const float4* __restrict__ pacc,
                                     const float* __restrict__ m, float G, float* __restrict__ ax,
                                     float* __restrict__ ay, float* __restrict__ az, double* __restrict__ ugrav)
{
    int64_t i = first + int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= last) return;
    float4 a = pacc[i - first];
    ax[i] += G * a.y;
    ay[i] += G * a.z;
    az[i] += G * a.w;
    if (ugrav) ugrav[i] += double(G) * double(m[i]) * double(a.x);
}

static int64_t padTo64(int64_t v) { return (v + 63) / 64 * 64; }

size_t gravityScratchBytes(int64_t n, int capM, int capL)
{
    int64_t groups = (n + 63) / 64;
    return size_t(padTo64(groups) + int64_t(kGSpillWaves) * kGSpillFront + padTo64(4 * groups) + padTo64(groups) +
                  groups * int64_t(capM + capL) + padTo64(2 * groups) + padTo64(4 * sgGridBlocks(groups)) +
                  4 * kOrdBins) *
           sizeof(int32_t);
}

struct GravScratch
{
    int32_t* spillList;
    int32_t* spillMem;
    GravSlabs S;
    int32_t* order;   // 2 x groups: M2P order, P2P order (heaviest first, single groups)
    int32_t* orderSG; // P2P wave slots under the super-group order (sgGridBlocks x kGWaves)
    int32_t* hist;  // 2 x kOrdBins histogram + 2 x kOrdBins scatter cursors
};

static GravScratch carve(void* scratch, int64_t groups, int capM, int capL)
{
    GravScratch c;
    c.spillList = static_cast<int32_t*>(scratch);
    c.spillMem  = c.spillList + padTo64(groups);
    int32_t* counts = c.spillMem + int64_t(kGSpillWaves) * kGSpillFront;
    int32_t* pcount = counts + padTo64(4 * groups);
    int32_t* mlist  = pcount + padTo64(groups);
    int32_t* llist  = mlist + groups * int64_t(capM);
    c.S             = GravSlabs{mlist, llist, counts, pcount, capM, capL};
    c.order         = llist + groups * int64_t(capL);
    c.orderSG       = c.order + padTo64(2 * groups);
    c.hist          = c.orderSG + padTo64(4 * sgGridBlocks(groups));
    return c;
}

//! @brief int32-word offsets of {spillList, counts, pcount, mlist, llist} in the scratch of an evaluation of n targets
//!        (tests read the interaction-list slabs through them), followed by the entry tag constants {kTagShift, kIdMask}
//!        and the capacity of the list kernel's LDS traversal stack {kGStack}
std::vector<int64_t> gravityScratchLayout(int64_t n, int capM, int capL)
{
    int64_t groups = (n + 63) / 64;
    // carve() only adds offsets to its base: a one-word array stands in for the scratch, no carved pointer is read
    static int32_t origin[1];
    const GravScratch c = carve(origin, groups, capM, capL);
    auto words = [&](const int32_t* p) { return int64_t((uintptr_t(p) - uintptr_t(origin)) / sizeof(int32_t)); };
    return {words(c.spillList), words(c.S.counts), words(c.S.pcount), words(c.S.mlist), words(c.S.llist),
            int64_t(kTagShift), int64_t(kIdMask), int64_t(kGStack)};
}

void computeGravityLists(int64_t first, int64_t last, const int32_t* child, const int32_t* n2l, const int32_t* ns,
                         const int32_t* ne, const double* centers, const void* mp, const double* x, const double* y,
                         const double* z, unsigned long long* stats, void* scratch, int testFrontCap, int capM,
                         int capL, hipStream_t s)
{
    int64_t n = last - first;
    if (n <= 0) return;
    GravTree t{child, n2l, ns, ne, centers, (const Quadrupole*)mp};
    int64_t groups = (n + 63) / 64;
    GravScratch c  = carve(scratch, groups, capM, capL);
    unsigned grid  = unsigned((groups + kGWaves - 1) / kGWaves);
    int cap        = testFrontCap > 0 ? min(testFrontCap, kGStack) : kGStack;
    gravityListKernel<<<grid, 64 * kGWaves, 0, s>>>(first, last, t, x, y, z, c.S, stats, c.spillList, cap);
    SPHX_LAUNCH_CHECK();
}

void computeGravityEval(int64_t first, int64_t last, const int32_t* child, const int32_t* n2l, const int32_t* ns,
                        const int32_t* ne, const double* centers, const void* mp, const double* x, const double* y,
                        const double* z, const float* h, const float* m, float G, float* ax, float* ay, float* az,
                        double* ugrav, double* out, unsigned long long* stats, void* scratch, int capM, int capL,
                        void* paccBuf, int64_t nsrc, int64_t numNodes, void* recBuf, const double* mm,
                        hipStream_t s, int phase, int order, const float* Q)
{
    float4* pacc = static_cast<float4*>(paccBuf);
    int4* rec    = static_cast<int4*>(recBuf);
    int64_t n = last - first;
    if (n <= 0) return;
    // phase 0: everything; split evaluation (models/propagators.py): 1 = node records + M2P (no smoothing lengths:
    // it may run beside the neighbor search), 2 = particle records + P2P, 3 = P2P combine + spill groups (after 1, 2)
    const bool all = phase == 0;
    // P2P source records of all particles of the tree and M2P node records (frame: mm = [min, max] per dimension,
    // on the device); the node records follow the particle records in the same buffer
    if (all || phase == 2)
    {
        gravityRecordsKernel<<<gridFor(nsrc, 256), 256, 0, s>>>(nsrc, x, y, z, h, mm, rec);
        SPHX_LAUNCH_CHECK();
    }
    float4* nra = reinterpret_cast<float4*>(rec + nsrc);
    float4* nrb = nra + numNodes;
    float2* nrc = reinterpret_cast<float2*>(nrb + numNodes);
    // order > 0: the far field is the order-P expansion of the raw moments Q (gravity_order.hip) over the same lists
    if (order > 0 && !Q) throw std::invalid_argument("computeGravityEval: an order needs the raw moments");
    if (order > 0 && (all || phase == 1)) gravityOrderRecords(order, numNodes, centers, Q, mm, nra, s);
    else if (all || phase == 1)
    {
        gravityNodeRecordsKernel<<<gridFor(numNodes, 256), 256, 0, s>>>(numNodes, centers, (const Quadrupole*)mp, mm,
                                                                       nra, nrb, nrc);
        SPHX_LAUNCH_CHECK();
    }
    const NodeRecs nrec{nra, nrb, nrc};
    GravTree t{child, n2l, ns, ne, centers, (const Quadrupole*)mp};
    int64_t groups = (n + 63) / 64;
    GravScratch c  = carve(scratch, groups, capM, capL);
    unsigned grid  = unsigned((groups + kGWaves - 1) / kGWaves);
    unsigned gridP = grid; // P2P grid (the super-group order pads it to whole runs on all XCDs)
    int64_t slotsP = groups; // valid entries of the P2P order
#ifdef SPHX_GRAV_SFC_ORDER
    const int32_t* orderM = nullptr;
    const int32_t* orderP = nullptr;
#else
    // M2P keeps the SFC order by default: heaviest-first dispatch scatters the node lists of concurrently running
    // groups over the tree (A/B on Evrard -n 200: P2P 10.14 -> 9.29 ms, M2P 8.10 -> 8.60 ms with both ordered)
#ifdef SPHX_GRAV_M2P_ORDER
    // the order is built with the P2P phase (2): a split evaluation would run the M2P (phase 1) before it exists
    if (!all) throw std::runtime_error("SPHX_GRAV_M2P_ORDER builds evaluate gravity in one phase (phase 0) only");
    const int32_t* orderM = c.order;
#else
    const int32_t* orderM = nullptr;
#endif
    if (all || phase == 2)
    {
        SPHX_CHECK(hipMemsetAsync(c.hist, 0, 4 * kOrdBins * sizeof(int32_t), s));
        const unsigned og = unsigned(std::min<int64_t>((groups + 255) / 256, 1024));
#ifndef SPHX_GRAV_SG_ORDER
        gravityOrderHistKernel<<<og, 256, 0, s>>>(groups, c.S, c.hist);
        SPHX_LAUNCH_CHECK();
        gravityOrderScatterKernel<<<og, 256, 0, s>>>(groups, c.S, c.hist, c.hist + 2 * kOrdBins, c.order);
        SPHX_LAUNCH_CHECK();
#else
        const unsigned sgb = unsigned(std::min<int64_t>(((groups + kSG - 1) / kSG + 255) / 256 + 1, 1024));
        gravitySgHistKernel<<<sgb, 256, 0, s>>>(groups, c.S, c.hist + kOrdBins);
        SPHX_LAUNCH_CHECK();
        gravitySgScatterKernel<<<sgb, 256, 0, s>>>(groups, c.S, c.hist + kOrdBins, c.hist + 3 * kOrdBins, c.orderSG);
        SPHX_LAUNCH_CHECK();
#endif
    }
#ifndef SPHX_GRAV_SG_ORDER
    const int32_t* orderP = c.order + groups;
#else
    const int32_t* orderP = c.orderSG;
    gridP                 = unsigned(sgGridBlocks(groups));
    slotsP                = int64_t(gridP) * kGWaves;
#endif
#endif
    // P2P partials land in pacc and are added by gravityCombineKernel. The two evaluation kernels run one after the
    // other on s: run concurrently (P2P on a side stream, SPHX_GRAV_CONCURRENT) they compete for the same SIMDs and
    // the step is ~1 ms slower on Evrard -n 200 (37.4 vs 38.4 ms, profiles/r2_perf_log.md)
    hipStream_t side = s;
    static thread_local hipEvent_t fork = nullptr, join = nullptr;
    if (!fork)
    {
        SPHX_CHECK(hipEventCreateWithFlags(&fork, hipEventDisableTiming));
        SPHX_CHECK(hipEventCreateWithFlags(&join, hipEventDisableTiming));
    }
#ifdef SPHX_GRAV_CONCURRENT
    static thread_local hipStream_t sideStream = nullptr;
    if (!sideStream) SPHX_CHECK(hipStreamCreateWithFlags(&sideStream, hipStreamNonBlocking));
    side = sideStream;
#endif
    if (all)
    {
        SPHX_CHECK(hipEventRecord(fork, s));
        SPHX_CHECK(hipStreamWaitEvent(side, fork, 0));
    }
    if (all || phase == 2)
    {
        gravityP2PKernel<<<gridP, 64 * kGWaves, 0, side>>>(first, last, t, x, y, z, h, m, G, ax, ay, az, ugrav, out,
                                                          stats, c.S, pacc, rec, mm, orderP, slotsP);
        SPHX_LAUNCH_CHECK();
    }
    if (all) SPHX_CHECK(hipEventRecord(join, side));
    if (order > 0 && (all || phase == 1))
        gravityOrderM2P(order, grid, first, last, x, y, z, h, m, G, ax, ay, az, ugrav, out, stats, c.S, orderM, groups,
                        nra, mm, s);
    else if (all || phase == 1)
    {
        gravityM2PKernel<<<grid, 64 * kGWaves, 0, s>>>(first, last, t, x, y, z, h, m, G, ax, ay, az, ugrav, out,
                                                       stats, c.S, orderM, groups, nrec, mm);
        SPHX_LAUNCH_CHECK();
    }
    if (all) SPHX_CHECK(hipStreamWaitEvent(s, join, 0));
    if (all || phase == 3)
    {
        gravityCombineKernel<<<gridFor(n, 256), 256, 0, s>>>(first, last, pacc, m, G, ax, ay, az, ugrav);
        SPHX_LAUNCH_CHECK();
        if (order > 0)
            gravityOrderSpill(order, first, last, t, x, y, z, h, m, G, ax, ay, az, ugrav, out, stats, c.spillList,
                              c.spillMem, rec, mm, Q, s);
        else
        {
            gravitySpillKernel<QuadM2P><<<kGSpillWaves, 64, 0, s>>>(first, last, t, x, y, z, h, m, G, ax, ay, az,
                                                                    ugrav, out, stats, c.spillList, c.spillMem, rec,
                                                                    mm, QuadM2P{});
            SPHX_LAUNCH_CHECK();
        }
    }
}

// --------------------------------------------------------------------------------------------- direct sum

constexpr int kDirectTile = 256;

__global__ __launch_bounds__(kDirectTile) void directKernel(int64_t first, int64_t last, int64_t n,
                                                            const double* __restrict__ x,
                                                            const double* __restrict__ y,
                                                            const double* __restrict__ z,
                                                            const float* __restrict__ h, const float* __restrict__ m,
                                                            float G, float* __restrict__ ax, float* __restrict__ ay,
                                                            float* __restrict__ az, double* __restrict__ ugrav,
                                                            double* __restrict__ out)
{
    __shared__ double sx[kDirectTile], sy[kDirectTile], sz[kDirectTile];
    __shared__ float sm[kDirectTile], sh[kDirectTile];
    __shared__ double red[kDirectTile / 64];
    int64_t i   = first + int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    bool valid  = i < last;
    double xi = valid ? x[i] : 0, yi = valid ? y[i] : 0, zi = valid ? z[i] : 0;
    float hi  = valid ? h[i] : 0;
    double acc[4] = {0, 0, 0, 0};
    for (int64_t t0 = 0; t0 < n; t0 += kDirectTile)
    {
        int64_t j = t0 + threadIdx.x;
        if (j < n)
        {
            sx[threadIdx.x] = x[j];
            sy[threadIdx.x] = y[j];
            sz[threadIdx.x] = z[j];
            sm[threadIdx.x] = m[j];
            sh[threadIdx.x] = h[j];
        }
        __syncthreads();
        int cnt = int(min<int64_t>(kDirectTile, n - t0));
        for (int k = 0; k < cnt; ++k)
            p2p(sx[k] - xi, sy[k] - yi, sz[k] - zi, double(sm[k]), double(hi), double(sh[k]), acc);
        __syncthreads();
    }
    double u = 0;
    if (valid)
    {
        u = double(G) * double(m[i]) * acc[0];
        if (ugrav) ugrav[i] = u;
        ax[i] = float(G * acc[1]);
        ay[i] = float(G * acc[2]);
        az[i] = float(G * acc[3]);
    }
    double s = waveSum(u);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0)
    {
        double tot = 0;
        for (int w = 0; w < kDirectTile / 64; ++w)
            tot += red[w];
        atomicAdd(out, 0.5 * tot);
    }
}

void directSum(int64_t first, int64_t last, int64_t n, const double* x, const double* y, const double* z,
               const float* h, const float* m, float G, float* ax, float* ay, float* az, double* ugrav, double* out,
               hipStream_t s)
{
    if (last <= first) return;
    directKernel<<<gridFor(last - first, kDirectTile), kDirectTile, 0, s>>>(first, last, n, x, y, z, h, m, G, ax, ay,
                                                                             az, ugrav, out);
    SPHX_LAUNCH_CHECK();
}

} // namespace sphx::hip

// --------------------------------------------------------------------------------------- LET selection / M2P

namespace sphx::hip
{

__global__ void markLetKernel(int64_t nb, const double* __restrict__ bc, const double* __restrict__ bh,
                              const int32_t* __restrict__ child, const int32_t* __restrict__ n2l,
                              const double* __restrict__ tc, const double* __restrict__ th,
                              const double* __restrict__ gc, Box box, uint8_t* failed)
{
    int64_t b = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (b >= nb) return;
    markLetBox(bc + 3 * b, bh + 3 * b, child, n2l, tc, th, gc, box, failed);
}

void markLet(int64_t nb, const double* bc, const double* bh, const int32_t* child, const int32_t* n2l,
             const double* tc, const double* th, const double* gc, const Box& box, uint8_t* failed, hipStream_t s)
{
    if (nb == 0) return;
    markLetKernel<<<gridFor(nb, 64), 64, 0, s>>>(nb, bc, bh, child, n2l, tc, th, gc, box, failed);
    SPHX_LAUNCH_CHECK();
}

/* LET selection of one receiver from its open flags (failed | outside): particle flags of the opened leaves (one
 * thread per leaf writes its particle range) and the send flags of the multipoles, the first unopened non-empty node
 * below an opened one (reference the LET of ryoanji/interface/multipole_holder.cu via domain exchange). One launch
 * instead of the torch gather/searchsorted/compare kernels of ops/gravity.py let_selection_masks. */
__global__ void letSelectKernel(int64_t N, int64_t L, int64_t np, const uint8_t* __restrict__ failed,
                                const uint8_t* __restrict__ outside, const int32_t* __restrict__ leafToNode,
                                const int32_t* __restrict__ ns, const int32_t* __restrict__ ne, int64_t offset,
                                const Quadrupole* __restrict__ mp, const int32_t* __restrict__ parents,
                                uint8_t* __restrict__ pflags, uint8_t* __restrict__ send)
{
    const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    auto open = [&](int64_t n) { return (failed[n] | (outside ? outside[n] : uint8_t(0))) != 0; };
    if (i < N)
    {
        bool s = !open(i) && mp[i].q[qMass] > MT(0);
        if (i > 0) s = s && open(parents[(i - 1) >> 3]);
        send[i] = uint8_t(s);
    }
    if (i < L)
    {
        const int32_t nd = leafToNode[i];
        const uint8_t v  = uint8_t(open(nd));
        const int64_t k0 = int64_t(ns[nd]) - offset, k1 = int64_t(ne[nd]) - offset;
        for (int64_t k = k0 > 0 ? k0 : 0; k < k1 && k < np; ++k) // (clamped to the flag array)
            pflags[k] = v;
    }
}

void letSelect(int64_t N, int64_t L, int64_t np, const uint8_t* failed, const uint8_t* outside,
               const int32_t* leafToNode, const int32_t* ns, const int32_t* ne, int64_t offset, const void* mp,
               const int32_t* parents, uint8_t* pflags, uint8_t* send, hipStream_t s)
{
    const int64_t n = N > L ? N : L;
    if (n <= 0) return;
    letSelectKernel<<<gridFor(n, 256), 256, 0, s>>>(N, L, np, failed, outside, leafToNode, ns, ne, offset,
                                                     static_cast<const Quadrupole*>(mp), parents, pflags, send);
    SPHX_LAUNCH_CHECK();
}

//! @brief open every node whose key range is not inside the sender's assigned range [lo, hi): remote LET nodes of
//!        different senders are then disjoint (cpu/let_tree_cpu.cpp)
__global__ void markOutsideRangeKernel(int64_t N, const KeyT* __restrict__ prefixes, KeyT lo, KeyT hi,
                                       uint8_t* __restrict__ failed)
{
    int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const int l    = placeholderLevel(prefixes[i]);
    const KeyT k   = placeholderKey(prefixes[i]);
    const KeyT end = k + nodeRange(l);
    if (k < lo || end > hi) failed[i] = 1;
}

void markOutsideRange(int64_t N, const KeyT* prefixes, KeyT lo, KeyT hi, uint8_t* failed, hipStream_t s)
{
    if (N <= 0) return;
    markOutsideRangeKernel<<<gridFor(N, 256), 256, 0, s>>>(N, prefixes, lo, hi, failed);
    SPHX_LAUNCH_CHECK();
}

constexpr int kFlatBlock = 256;

/*! @brief every target against every remote multipole (all of them pass the MAC by construction of the LET);
 *         multipoles are staged through LDS in chunks shared by the block, r = target - center in fp32
 */
__global__ __launch_bounds__(kFlatBlock) void m2pFlatKernel(int64_t first, int64_t last, const double* __restrict__ x,
                                                            const double* __restrict__ y,
                                                            const double* __restrict__ z,
                                                            const float* __restrict__ m, int64_t M,
                                                            const double* __restrict__ mc,
                                                            const Quadrupole* __restrict__ mp, float G,
                                                            float* __restrict__ ax, float* __restrict__ ay,
                                                            float* __restrict__ az, double* __restrict__ ugrav,
                                                            double* __restrict__ out)
{
    __shared__ double sc[kFlatBlock][3];
    __shared__ Quadrupole sq[kFlatBlock];
    __shared__ double red[kFlatBlock / 64];
    int64_t i   = first + int64_t(blockIdx.x) * kFlatBlock + threadIdx.x;
    bool valid  = i < last;
    double xi = valid ? x[i] : 0, yi = valid ? y[i] : 0, zi = valid ? z[i] : 0;
    float acc[4] = {0, 0, 0, 0};
    for (int64_t base = 0; base < M; base += kFlatBlock)
    {
        int cnt = int(min(int64_t(kFlatBlock), M - base));
        __syncthreads();
        if (int(threadIdx.x) < cnt)
        {
            int64_t k = base + threadIdx.x;
            sc[threadIdx.x][0] = mc[3 * k];
            sc[threadIdx.x][1] = mc[3 * k + 1];
            sc[threadIdx.x][2] = mc[3 * k + 2];
            sq[threadIdx.x]    = mp[k];
        }
        __syncthreads();
        for (int k = 0; k < cnt; ++k)
            m2p(float(xi - sc[k][0]), float(yi - sc[k][1]), float(zi - sc[k][2]), sq[k], acc);
    }
    double u = 0;
    if (valid)
    {
        u = double(G) * double(m[i]) * double(acc[0]);
        if (ugrav) ugrav[i] += u;
        ax[i] += G * acc[1];
        ay[i] += G * acc[2];
        az[i] += G * acc[3];
    }
    double s = waveSum(u);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0)
    {
        double tot = 0;
        for (int w = 0; w < kFlatBlock / 64; ++w)
            tot += red[w];
        atomicAdd(out, 0.5 * tot);
    }
}

void m2pFlat(int64_t first, int64_t last, const double* x, const double* y, const double* z, const float* m,
             int64_t M, const double* mc, const void* mp, float G, float* ax, float* ay, float* az, double* ugrav,
             double* out, hipStream_t s)
{
    if (last <= first || M == 0) return;
    m2pFlatKernel<<<gridFor(last - first, kFlatBlock), kFlatBlock, 0, s>>>(
        first, last, x, y, z, m, M, mc, (const Quadrupole*)mp, G, ax, ay, az, ugrav, out);
    SPHX_LAUNCH_CHECK();
}

SPHX_DCHECK_READER(dcheckGravity)

} // namespace sphx::hip
