/*! Bound groups on gfx950: the self-potential of every member of every friends-of-friends group and the unbinding
 *  loop around it (definitions and the error bound: sphx/groups.hpp; the sequence of launches and the one host read per
 *  iteration: ops/groups.py; the host path: cpu/groups_cpu.cpp).
 *
 *  1. Members. fofGroups (fof.hip) leaves the particles sorted by label; groupCountKernel takes the member counts of
 *     the kept groups in catalogue order (count descending, label ascending), a scan gives their starts, and
 *     groupMembersKernel, a thread per member, writes the compact member arrays in that order, ascending particle
 *     index inside a group: the 16-B record {dx, dy, dz, m} in fp32, the particle index and the group. Velocities,
 *     internal energies and fp64 masses are read through the particle index where they are needed (the kernels around
 *     the pair loop are not the cost), so an iteration moves 24 B per member.
 *  2. Items. groupPlanKernel turns the bound counts into three scans: member starts, item offsets and offsets of the
 *     partial rows. An item is (group, target tile of 64 R consecutive members, source segment of at most SEG members;
 *     R = 1, see kR below);
 *     a group of c members has ceil(c / 64 R) ceil(c / SEG) of them, tile-major. The items of the largest groups come
 *     first, which is the catalogue order. There is no item array: a wave finds its group by a binary search of the
 *     item offsets, a scalar loop of log2 G steps.
 *  3. groupPotentialKernel, the hot path: one wave per item, four waves per block, no block-level barrier (the idiom of
 *     fofLinkKernel). A lane keeps R target offsets and R fp32 accumulators in registers. The wave streams its source
 *     segment through its own 1-KiB LDS slice in chunks of 64 records, one coalesced 16-B load per lane, the next chunk
 *     fetched into registers while the current one is evaluated; behind the end of the segment the records are zero,
 *     so every chunk runs the same 64 steps and a padded source adds exactly 0 (its mass). A source is read by all
 *     lanes as one wave-uniform ds_read_b128 broadcast and serves R pairs per lane: three subtractions, a product, two
 *     multiply-adds, the add of eps^2, v_rsq_f32 and one multiply-add onto the accumulator. j != i is an index test,
 *     and it exists only in the chunk that coincides with one of the tile's R rows of 64 (tiles, segments and chunks
 *     are all 64-aligned inside a group): that chunk takes the masked copy of the loop, the others carry no compare.
 *     After each chunk the fp32 partial goes into an fp64 accumulator.
 *     Not on the matrix cores: the expanded form |t|^2 + |s|^2 - 2 t.s has a rounding error of 2^-24 D^2 (D the
 *     group's extent), which would have to stay far below eps^2, and an unbinding run cannot promise that; the f32
 *     MFMA also issues at the packed-VALU rate on this part (README, gravity notes), so nothing would be gained.
 *  4. Segment sums. An item of a group with more than one segment writes the fp64 partial row [segment][member];
 *     groupSegSumKernel adds the rows in segment order. No atomics on values: bit-identical from run to run.
 *  5. Iteration: groupBulkKernel (a wave per group, pieces of 32 in lane order, fp64) forms the bulk velocity,
 *     groupEnergyKernel the specific energies, groupRemovedKernel the new bound counts (a group below min_members is
 *     dissolved) and the total removed (an integer atomic), groupFlagsKernel / scan / groupScatterKernel compact the
 *     members stably into the second set of arrays.
 *  6. groupCatalogKernel, a wave per group: the fp64 sums in the same piece order, the member of lowest phi (the
 *     centre) and of lowest e (most bound), ties to the smallest index; groupOutputKernel scatters mask and phi.
 *
 *  Every loop is bounded by counts that are clamped to the array sizes; indices read from memory are clamped before
 *  they address anything (device-check build: bit 11). Resources: profiles/r17/groups/README.md.
 */
#include <climits>
#include <cmath>

#include "common.h"
#include "hip_api.h"

namespace sphx::hip
{

namespace
{

// target rows of 64 per item. R = 2 (two targets per lane and broadcast) was built and timed as well: never faster on
// the whole calls, and slower where a single large group yields too few items to fill the device
// (profiles/r17/groups/README.md), so R = 1 is the only instance
constexpr int kR        = 1;
constexpr int kTile     = kGroupChunk * kR;
constexpr int kPotBlock = 256;
constexpr int kPotWaves = kPotBlock / kWave;

__device__ __forceinline__ int64_t clampG(int64_t v, int64_t lo, int64_t hi)
{
    SPHX_DCHECK(v >= lo && v <= hi, 11);
    return v < lo ? lo : (v > hi ? hi : v);
}

//! bound count of catalogue group k at the start: its member count
__global__ void __launch_bounds__(256)
groupCountKernel(int64_t G, int64_t Gall, const int32_t* __restrict__ perm2, const int32_t* __restrict__ gstart,
                 int64_t* __restrict__ bcount)
{
    const int64_t k = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (k >= G) return;
    const int64_t gi = clampG(perm2[k], 0, Gall - 1);
    bcount[k]        = sphx::smax(int64_t(gstart[gi + 1]) - gstart[gi], int64_t(0));
}

//! the three counts that are scanned: members, items, doubles of partial rows (entry G: 0, for the totals)
__global__ void __launch_bounds__(256)
groupPlanKernel(int64_t G, int seg, const int64_t* __restrict__ bcount, int64_t* __restrict__ bstart,
                int64_t* __restrict__ itemOff, int64_t* __restrict__ partOff)
{
    const int64_t k = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (k > G) return;
    const int64_t c = k < G ? clampG(bcount[k], 0, kGroupMaxN) : 0;
    const int64_t T = (c + kTile - 1) / kTile, S = (c + seg - 1) / seg;
    bstart[k]  = c;
    itemOff[k] = T * S;
    partOff[k] = S > 1 ? S * c : 0;
}

//! counters: [0] members removed (left alone here), [1] items, [2] doubles of partial rows, [3] bound members
__global__ void groupTotalsKernel(int64_t G, const int64_t* __restrict__ bstart, const int64_t* __restrict__ itemOff,
                                  const int64_t* __restrict__ partOff, int64_t* __restrict__ counters)
{
    counters[1] = itemOff[G];
    counters[2] = partOff[G];
    counters[3] = bstart[G];
}

//! largest k in [0, G) with off[k] <= v (off ascending, off[0] <= v < off[G])
__device__ __forceinline__ int64_t groupOf(const int64_t* __restrict__ off, int64_t G, int64_t v)
{
    int64_t lo = 0, hi = G;
    while (hi - lo > 1)
    {
        const int64_t mid = (lo + hi) >> 1;
        if (off[mid] <= v) lo = mid;
        else hi = mid;
    }
    return lo;
}

struct GroupMemberArgs
{
    int64_t n, G, Gall, M;
    const int32_t *perm2, *gstart, *perm;
    const int64_t* bstart;
    const double *x, *y, *z, *m;
    Box box;
    float4* rec;
    int32_t *idx, *grp;
};

__global__ void __launch_bounds__(256) groupMembersKernel(GroupMemberArgs A)
{
    const int64_t q = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (q >= A.M) return;
    const int64_t k  = groupOf(A.bstart, A.G, q);
    const int64_t gi = clampG(A.perm2[k], 0, A.Gall - 1);
    const int64_t s0 = clampG(A.gstart[gi], 0, A.n - 1);
    const int64_t p  = clampG(s0 + (q - A.bstart[k]), 0, A.n - 1);
    const int64_t j = clampG(A.perm[p], 0, A.n - 1), r = clampG(A.perm[s0], 0, A.n - 1);
    A.rec[q] = float4{groupOffset(A.x[j], A.x[r], A.box, 0), groupOffset(A.y[j], A.y[r], A.box, 1),
                      groupOffset(A.z[j], A.z[r], A.box, 2), float(A.m[j])};
    A.idx[q] = int32_t(j);
    A.grp[q] = int32_t(k);
}

struct GroupPotArgs
{
    int64_t G, M, nItems, nPartial;
    int seg;
    float eps2;
    double negG;
    const int64_t *bstart, *itemOff, *partOff;
    const float4* rec;
    double *phi, *partial;
};

//! one source against the lane's R targets
template<bool Masked>
__device__ __forceinline__ void groupPair(const float4 s, const float4 (&t)[kR], float eps2, int jj, int lane,
                                          int diagRow, float (&a)[kR])
{
#pragma unroll
    for (int r = 0; r < kR; ++r)
    {
        const float dx = t[r].x - s.x, dy = t[r].y - s.y, dz = t[r].z - s.z;
        const float r2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx)) + eps2;
        float mj       = s.w;
        if (Masked) mj = (r == diagRow && jj == lane) ? 0.0f : mj; // j != i: the member itself, by index
        a[r] = fmaf(mj, __builtin_amdgcn_rsqf(r2), a[r]);
    }
}

__global__ void __launch_bounds__(kPotBlock) groupPotentialKernel(GroupPotArgs A)
{
    __shared__ float4 sRec[kPotWaves][kGroupChunk];

    const int wave = threadIdx.x >> 6, lane = laneId();
    const int64_t item = int64_t(blockIdx.x) * kPotWaves + wave;
    if (item >= A.nItems) return; // (waves never meet at a block barrier)

    const int64_t k  = groupOf(A.itemOff, A.G, item);
    const int64_t b0 = clampG(A.bstart[k], 0, A.M - 1);
    const int c      = int(clampG(A.bstart[k + 1] - b0, 1, A.M - b0));
    const int S      = (c + A.seg - 1) / A.seg;
    const int64_t local = clampG(item - A.itemOff[k], 0, int64_t(S) * ((c + kTile - 1) / kTile) - 1);
    const int tile = int(local / S), sg = int(local - int64_t(tile) * S);
    const int t0 = tile * kTile, s0 = sg * A.seg, s1 = sphx::smin(s0 + A.seg, c);

    float4 t[kR];
    double acc[kR];
#pragma unroll
    for (int r = 0; r < kR; ++r)
    {
        const int ti = t0 + r * kGroupChunk + lane;
        t[r]         = A.rec[b0 + (ti < c ? ti : 0)];
        acc[r]       = 0.0;
    }

    const float4 zero{0.f, 0.f, 0.f, 0.f};
    float4 next = s0 + lane < s1 ? A.rec[b0 + s0 + lane] : zero;
    for (int jb = s0; jb < s1; jb += kGroupChunk)
    {
        __builtin_amdgcn_wave_barrier(); // the chunk before has been read
        sRec[wave][lane] = next;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        const int jn = jb + kGroupChunk + lane;
        next         = jn < s1 ? A.rec[b0 + jn] : zero;

        float a[kR];
#pragma unroll
        for (int r = 0; r < kR; ++r)
            a[r] = 0.0f;
        const int diag = jb - t0; // a multiple of 64: the chunk is row diag / 64 of the tile, or none of its rows
        if (diag >= 0 && diag < kTile)
        {
            const int diagRow = diag / kGroupChunk;
#pragma unroll 8
            for (int jj = 0; jj < kGroupChunk; ++jj)
                groupPair<true>(sRec[wave][jj], t, A.eps2, jj, lane, diagRow, a);
        }
        else
        {
#pragma unroll 8
            for (int jj = 0; jj < kGroupChunk; ++jj)
                groupPair<false>(sRec[wave][jj], t, A.eps2, jj, lane, 0, a);
        }
#pragma unroll
        for (int r = 0; r < kR; ++r)
            acc[r] += double(a[r]);
    }

#pragma unroll
    for (int r = 0; r < kR; ++r)
    {
        const int ti = t0 + r * kGroupChunk + lane;
        if (ti >= c) continue;
        const double v = A.negG * acc[r];
        if (S == 1) A.phi[b0 + ti] = v;
        else if (A.partial) A.partial[clampG(A.partOff[k] + int64_t(sg) * c + ti, 0, A.nPartial - 1)] = v;
    }
}

//! phi of the members of groups with more than one segment: the partial rows in segment order
__global__ void __launch_bounds__(256)
groupSegSumKernel(int64_t G, int64_t M, int64_t nPartial, int seg, const int64_t* __restrict__ bstart,
                  const int64_t* __restrict__ partOff, const int32_t* __restrict__ grp,
                  const double* __restrict__ partial, double* __restrict__ phi)
{
    const int64_t q = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (q >= M) return;
    const int64_t k = clampG(grp[q], 0, G - 1);
    const int64_t c = bstart[k + 1] - bstart[k], S = (c + seg - 1) / seg;
    if (S <= 1) return;
    const int64_t ti = clampG(q - bstart[k], 0, c - 1);
    double v         = 0.0;
    for (int64_t sg = 0; sg < S; ++sg)
        v += partial[clampG(partOff[k] + sg * c + ti, 0, nPartial - 1)];
    phi[q] = v;
}

struct GroupFields
{
    const double *x, *y, *z, *m, *vx, *vy, *vz, *u; // by particle; u may be null
};

/*! @brief the sums of a group in the fixed order: lane l sums piece l of a pass (kGroupPiece consecutive members,
 *         ascending), the pieces are added in piece order; every lane ends with the same totals. term(q, ps) adds
 *         member q's terms to the piece sums */
template<int N, class F>
__device__ __forceinline__ void groupSums(int64_t b0, int64_t c, double (&acc)[N], F&& term)
{
    const int lane = laneId();
#pragma unroll
    for (int i = 0; i < N; ++i)
        acc[i] = 0.0;
    for (int64_t pass = 0; pass < c; pass += int64_t(kWave) * kGroupPiece)
    {
        double ps[N];
#pragma unroll
        for (int i = 0; i < N; ++i)
            ps[i] = 0.0;
        const int64_t a = pass + int64_t(lane) * kGroupPiece, b = sphx::smin(a + kGroupPiece, c);
        for (int64_t p = a; p < b; ++p)
            term(b0 + p, ps);
        const int pieces = int(sphx::smin(int64_t(kWave), (c - pass + kGroupPiece - 1) / kGroupPiece));
        for (int l = 0; l < pieces; ++l)
#pragma unroll
            for (int i = 0; i < N; ++i)
                acc[i] += readLaneD(ps[i], l);
    }
}

//! Vg[4 k ..] = {bound mass, bulk velocity} of group k (zeros for a group without bound members)
__global__ void __launch_bounds__(256)
groupBulkKernel(int64_t n, int64_t G, int64_t M, const int64_t* __restrict__ bstart, const int32_t* __restrict__ idx,
                GroupFields F, double* __restrict__ Vg)
{
#pragma clang fp contract(off)
    const int64_t k = int64_t(blockIdx.x) * (256 / kWave) + (threadIdx.x >> 6);
    if (k >= G) return;
    const int64_t b0 = clampG(bstart[k], 0, M), c = clampG(bstart[k + 1] - b0, 0, M - b0);
    double acc[4];
    groupSums(b0, c, acc,
              [&](int64_t q, double(&ps)[4])
              {
#pragma clang fp contract(off)
                  const int64_t j = clampG(idx[q], 0, n - 1);
                  const double mj = F.m[j];
                  ps[0] += mj;
                  ps[1] += mj * F.vx[j];
                  ps[2] += mj * F.vy[j];
                  ps[3] += mj * F.vz[j];
              });
    if (laneId() != 0) return;
    Vg[4 * k] = acc[0];
    for (int a = 0; a < 3; ++a)
        Vg[4 * k + 1 + a] = c > 0 ? acc[1 + a] / acc[0] : 0.0;
}

__global__ void __launch_bounds__(256)
groupEnergyKernel(int64_t n, int64_t G, int64_t M, const int32_t* __restrict__ idx, const int32_t* __restrict__ grp,
                  GroupFields F, const double* __restrict__ Vg, const double* __restrict__ phi, double* __restrict__ e)
{
    const int64_t q = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (q >= M) return;
    const int64_t j = clampG(idx[q], 0, n - 1), k = clampG(grp[q], 0, G - 1);
    e[q] = groupEnergy(F.vx[j], F.vy[j], F.vz[j], Vg + 4 * k + 1, F.u ? F.u[j] : 0.0, phi[q]);
}

//! the bound counts after the removal of e > 0 (below minMembers: 0, the group is dissolved); counters[0] += removed
__global__ void __launch_bounds__(256)
groupRemovedKernel(int64_t G, int64_t M, int64_t minMembers, const int64_t* __restrict__ bstart,
                   const double* __restrict__ e, int64_t* __restrict__ bcount, int64_t* __restrict__ counters)
{
    const int64_t k = int64_t(blockIdx.x) * (256 / kWave) + (threadIdx.x >> 6);
    if (k >= G) return;
    const int64_t b0 = clampG(bstart[k], 0, M), c = clampG(bstart[k + 1] - b0, 0, M - b0);
    int64_t kept = 0;
    for (int64_t p = 0; p < c; p += kWave)
        kept += popcount64(ballot(p + laneId() < c && !(e[b0 + sphx::smin(p + laneId(), c - 1)] > 0.0)));
    if (kept < minMembers) kept = 0;
    if (laneId() != 0) return;
    bcount[k] = kept;
    if (c > kept) atomicAdd(reinterpret_cast<unsigned long long*>(counters), (unsigned long long)(c - kept));
}

//! flags[q] = 1 for the members that stay (flags[M] = 0 for the scan's total)
__global__ void __launch_bounds__(256)
groupFlagsKernel(int64_t G, int64_t M, const int32_t* __restrict__ grp, const double* __restrict__ e,
                 const int64_t* __restrict__ bcount, int64_t* __restrict__ flags)
{
    const int64_t q = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (q > M) return;
    flags[q] = (q < M && !(e[q] > 0.0) && bcount[clampG(grp[q], 0, G - 1)] > 0) ? 1 : 0;
}

__global__ void __launch_bounds__(256)
groupScatterKernel(int64_t M, const int64_t* __restrict__ scan, const float4* __restrict__ rec,
                   const int32_t* __restrict__ idx, const int32_t* __restrict__ grp, float4* __restrict__ rec2,
                   int32_t* __restrict__ idx2, int32_t* __restrict__ grp2)
{
    const int64_t q = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (q >= M || scan[q + 1] == scan[q]) return;
    const int64_t d = clampG(scan[q], 0, q);
    rec2[d] = rec[q];
    idx2[d] = idx[q];
    grp2[d] = grp[q];
}

struct GroupCatalogArgs
{
    int64_t n, G, M;
    const int64_t* bstart;
    const int32_t* idx;
    const double *phi, *e, *Vg;
    GroupFields F;
    Box box;
    int64_t* boundCount;
    double* sums; // 10 per group: bound mass, vel, ekin, eint, epot, centre
    int32_t *centreIndex, *mostBound;
};

__global__ void __launch_bounds__(256) groupCatalogKernel(GroupCatalogArgs A)
{
#pragma clang fp contract(off)
    const int lane  = laneId();
    const int64_t k = int64_t(blockIdx.x) * (256 / kWave) + (threadIdx.x >> 6);
    if (k >= A.G) return;
    const int64_t b0 = clampG(A.bstart[k], 0, A.M), c = clampG(A.bstart[k + 1] - b0, 0, A.M - b0);
    const double* V  = A.Vg + 4 * k + 1;
    double acc[4];
    groupSums(b0, c, acc,
              [&](int64_t q, double(&ps)[4])
              {
#pragma clang fp contract(off)
                  const int64_t j = clampG(A.idx[q], 0, A.n - 1);
                  const double mj = A.F.m[j];
                  const double wx = A.F.vx[j] - V[0], wy = A.F.vy[j] - V[1], wz = A.F.vz[j] - V[2];
                  const double xx = wx * wx, yy = wy * wy, zz = wz * wz;
                  ps[0] += mj;
                  ps[1] += 0.5 * mj * ((xx + yy) + zz);
                  if (A.F.u) ps[2] += mj * A.F.u[j];
                  ps[3] += mj * A.phi[q];
              });
    // the members of lowest phi and of lowest e: a lane scans every 64th member, the lanes are compared in lane
    // order; only a strictly lower value replaces, so ties go to the smallest member position (the smallest index)
    double bestP = INFINITY, bestE = INFINITY;
    int64_t qP = -1, qE = -1;
    for (int64_t p = lane; p < c; p += kWave)
    {
        const double ph = A.phi[b0 + p], en = A.e[b0 + p];
        if (ph < bestP || qP < 0) bestP = ph, qP = b0 + p;
        if (en < bestE || qE < 0) bestE = en, qE = b0 + p;
    }
    for (int o = 1; o < kWave; o <<= 1)
    {
        const double oP = __shfl_xor(bestP, o), oE = __shfl_xor(bestE, o);
        const int64_t oqP = __shfl_xor((long long)qP, o), oqE = __shfl_xor((long long)qE, o);
        if (oqP >= 0 && (qP < 0 || oP < bestP || (oP == bestP && oqP < qP))) bestP = oP, qP = oqP;
        if (oqE >= 0 && (qE < 0 || oE < bestE || (oE == bestE && oqE < qE))) bestE = oE, qE = oqE;
    }
    if (lane != 0) return;
    double* out     = A.sums + 10 * k;
    A.boundCount[k] = c;
    out[0]          = acc[0];
    for (int a = 0; a < 3; ++a)
        out[1 + a] = c > 0 ? V[a] : NAN;
    out[4] = acc[1];
    out[5] = acc[2];
    out[6] = 0.5 * acc[3];
    int32_t ci = -1, mb = -1;
    double cx = NAN, cy = NAN, cz = NAN;
    if (c > 0)
    {
        ci = int32_t(clampG(A.idx[clampG(qP, b0, b0 + c - 1)], 0, A.n - 1));
        mb = int32_t(clampG(A.idx[clampG(qE, b0, b0 + c - 1)], 0, A.n - 1));
        cx = A.F.x[ci], cy = A.F.y[ci], cz = A.F.z[ci];
        putInBox(cx, cy, cz, A.box);
    }
    out[7] = cx, out[8] = cy, out[9] = cz;
    A.centreIndex[k] = ci;
    A.mostBound[k]   = mb;
}

__global__ void __launch_bounds__(256)
groupOutputKernel(int64_t n, int64_t M, const int32_t* __restrict__ idx, const double* __restrict__ phi,
                  uint8_t* __restrict__ bound, double* __restrict__ phiOut)
{
    const int64_t q = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (q >= M) return;
    const int64_t j = clampG(idx[q], 0, n - 1);
    bound[j]  = 1;
    phiOut[j] = phi[q];
}

void checkCounts(int64_t n, int64_t G, int64_t M)
{
    if (n < 1 || n > kGroupMaxN || G < 1 || G > n || M < 0 || M > n)
        throw std::invalid_argument("groups: inconsistent counts");
}

void plan(int64_t G, int seg, const GroupBuffers& B, hipStream_t s)
{
    groupPlanKernel<<<gridFor(G + 1, 256), 256, 0, s>>>(G, seg, B.bcount, B.bstart, B.itemOff, B.partOff);
    SPHX_LAUNCH_CHECK();
    exclusiveScanI64(B.bstart, B.bstart, G + 1, B.tmp, B.tmpBytes, s);
    exclusiveScanI64(B.itemOff, B.itemOff, G + 1, B.tmp, B.tmpBytes, s);
    exclusiveScanI64(B.partOff, B.partOff, G + 1, B.tmp, B.tmpBytes, s);
    groupTotalsKernel<<<1, 1, 0, s>>>(G, B.bstart, B.itemOff, B.partOff, B.counters);
    SPHX_LAUNCH_CHECK();
}

} // namespace

int groupTile() { return kTile; }

void groupInit(int64_t n, int64_t Gall, int64_t G, int seg, const int32_t* perm2, const int32_t* gstart,
               const GroupBuffers& B, hipStream_t s)
{
    checkCounts(n, G, 0);
    if (Gall < G || Gall > n) throw std::invalid_argument("groups: inconsistent group counts");
    groupCountKernel<<<gridFor(G, 256), 256, 0, s>>>(G, Gall, perm2, gstart, B.bcount);
    SPHX_LAUNCH_CHECK();
    plan(G, groupSegment(seg), B, s);
}

void groupMembers(int64_t n, int64_t Gall, int64_t G, int64_t M, const int32_t* perm2, const int32_t* gstart,
                  const int32_t* perm, const double* x, const double* y, const double* z, const double* m,
                  const Box& box, const GroupBuffers& B, hipStream_t s)
{
    checkCounts(n, G, M);
    if (M < 1) return;
    const GroupMemberArgs A{n, G, Gall, M, perm2, gstart, perm, B.bstart, x, y, z, m, box, B.rec[0], B.idx[0],
                            B.grp[0]};
    groupMembersKernel<<<gridFor(M, 256), 256, 0, s>>>(A);
    SPHX_LAUNCH_CHECK();
}

void groupEvaluate(int64_t n, int64_t G, int64_t M, int64_t nItems, int64_t nPartial, int seg, int cur, double eps,
                   double Gc, const GroupFields4& f, const GroupBuffers& B, double* partial, hipStream_t s)
{
    checkCounts(n, G, M);
    if (!(eps > 0.0) || nItems < 0 || nPartial < 0 || (nPartial > 0 && !partial) || (cur != 0 && cur != 1))
        throw std::invalid_argument("groups: eps must be positive and the plan consistent");
    const GroupFields F{nullptr, nullptr, nullptr, f.m, f.vx, f.vy, f.vz, f.u};
    if (M > 0 && nItems > 0)
    {
        const GroupPotArgs A{G, M, nItems, nPartial, groupSegment(seg), float(eps * eps), -Gc, B.bstart, B.itemOff,
                             B.partOff, B.rec[cur], B.phi, partial};
        groupPotentialKernel<<<gridFor(nItems, kPotWaves), kPotBlock, 0, s>>>(A);
        SPHX_LAUNCH_CHECK();
        if (nPartial > 0)
        {
            groupSegSumKernel<<<gridFor(M, 256), 256, 0, s>>>(G, M, nPartial, seg, B.bstart, B.partOff, B.grp[cur],
                                                              partial, B.phi);
            SPHX_LAUNCH_CHECK();
        }
    }
    groupBulkKernel<<<gridFor(G, 256 / kWave), 256, 0, s>>>(n, G, M, B.bstart, B.idx[cur], F, B.Vg);
    SPHX_LAUNCH_CHECK();
    if (M > 0)
    {
        groupEnergyKernel<<<gridFor(M, 256), 256, 0, s>>>(n, G, M, B.idx[cur], B.grp[cur], F, B.Vg, B.phi, B.e);
        SPHX_LAUNCH_CHECK();
    }
}

void groupRemove(int64_t n, int64_t G, int64_t M, int64_t minMembers, int seg, int cur, const GroupBuffers& B,
                 hipStream_t s)
{
    checkCounts(n, G, M);
    if (cur != 0 && cur != 1) throw std::invalid_argument("groups: buffer set 0 or 1");
    groupRemovedKernel<<<gridFor(G, 256 / kWave), 256, 0, s>>>(G, M, minMembers, B.bstart, B.e, B.bcount, B.counters);
    SPHX_LAUNCH_CHECK();
    groupFlagsKernel<<<gridFor(M + 1, 256), 256, 0, s>>>(G, M, B.grp[cur], B.e, B.bcount, B.scan);
    SPHX_LAUNCH_CHECK();
    exclusiveScanI64(B.scan, B.scan, M + 1, B.tmp, B.tmpBytes, s);
    if (M > 0)
    {
        groupScatterKernel<<<gridFor(M, 256), 256, 0, s>>>(M, B.scan, B.rec[cur], B.idx[cur], B.grp[cur],
                                                           B.rec[1 - cur], B.idx[1 - cur], B.grp[1 - cur]);
        SPHX_LAUNCH_CHECK();
    }
    plan(G, groupSegment(seg), B, s);
}

void groupCatalog(int64_t n, int64_t G, int64_t M, int cur, const double* x, const double* y, const double* z,
                  const GroupFields4& f, const Box& box, const GroupBuffers& B, int64_t* boundCount, double* sums,
                  int32_t* centreIndex, int32_t* mostBound, uint8_t* bound, double* phiOut, hipStream_t s)
{
    checkCounts(n, G, M);
    if (cur != 0 && cur != 1) throw std::invalid_argument("groups: buffer set 0 or 1");
    const GroupCatalogArgs A{n, G, M, B.bstart, B.idx[cur], B.phi, B.e, B.Vg, GroupFields{x, y, z, f.m, f.vx, f.vy,
                             f.vz, f.u}, box, boundCount, sums, centreIndex, mostBound};
    groupCatalogKernel<<<gridFor(G, 256 / kWave), 256, 0, s>>>(A);
    SPHX_LAUNCH_CHECK();
    if (M > 0)
    {
        groupOutputKernel<<<gridFor(M, 256), 256, 0, s>>>(n, M, B.idx[cur], B.phi, bound, phiOut);
        SPHX_LAUNCH_CHECK();
    }
}

SPHX_DCHECK_READER(dcheckGroups)

} // namespace sphx::hip
