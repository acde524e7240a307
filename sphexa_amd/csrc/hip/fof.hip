/*! Friends-of-friends groups on gfx950 (definitions: ops/fof.py; geometry, stencil, pair test and union-find:
 *  sphx/fof.hpp, shared with the host path cpu/fof_cpu.cpp).
 *
 *  1. fofKeysKernel, one thread per particle: the cell coordinates are formed in fp64; the key is the linear cell index
 *     with x fastest (made distinct by the particle index below it where the bits allow; a particle that takes no
 *     part sorts behind every cell), the 16-B record is {fx, fy, fz, cx}: the position inside the cell in cell edges, rounded once to fp32, and the cell's x coordinate.
 *  2. The project's stable sample sort orders the keys: a cell's particles come out in ascending index, its first
 *     particle is its smallest. There is no dense cell array: fofFlagsKernel marks the first position of every
 *     occupied cell, a scan numbers the cells, fofCellsKernel writes cellStart / cellKey, the sorted records and
 *     cellOf, and sets parent[c] = c.
 *  3. Work items: fofItemCountKernel and fofItemFillKernel cut the sorted positions into cell-aligned items of at most
 *     64 positions of one (y, z) row (a cell of more than 64 particles becomes slices of 64). An item starts where a
 *     row starts, at a cell that does not fit the 64-aligned block of positions it starts in, and after such a cell:
 *     all of this is local to a cell and the one before it, so the items come from one scan.
 *  4. fofLinkKernel, the hot path: one wave per item, a lane per target particle. For every run of the half stencil
 *     (13 for R = 2; a run is one contiguous range of the sorted array) the wave finds the first occupied cell by a
 *     64-ary search of cellKey (every lane probes, a ballot narrows: 4 passes for 16 M cells), then streams the
 *     sources through its own LDS region in chunks of 64 (one coalesced 16-B record and one cell index per lane) and
 *     walks them in a wave-uniform loop with broadcast LDS reads. Friendship is settled between cells: on entering a
 *     source cell B every lane compares the root of its own cell with the root of B; if a ballot shows that no lane
 *     still needs B the wave jumps to the end of B (cellStart, not the chunk), else the needing lanes test their
 *     particle against B's staged particles until the first hit. The lowest hitting lane of a target cell unions the
 *     two cells; the cell's other lanes learn of it from the ballot of the hits, masked with the lanes of their own
 *     cell, and stop (a register mask instead of a flag in LDS: no traffic at all); slices of one cell in other
 *     waves learn of it at their next root comparison. Two dense neighbouring cells cost O(1) tests, not n_A n_B.
 *     The fp32 test decides outside a band of 2^-14 around d^2 = b^2 (its error is below 2e-6); inside it the pair is
 *     re-tested from the fp64 coordinates: the links are exactly those of the fp64 definition.
 *  5. fofFlattenKernel finds every cell's root and lowers least[root] to the cell's first particle (atomicMin);
 *     fofLabelKernel gives every particle least[root of its cell]. The labels are the component minima, whatever the
 *     order in which the links were found.
 *
 *  Every loop is bounded: the union-find by the arguments in sphx/fof.hpp, the search by its shrinking range, the
 *  source walk by pos, which only grows. Indices read from memory are clamped before they address anything.
 *
 *  Catalogue: the labels are sorted (stable: ascending particle index inside a group), flags and a scan give the group
 *  starts, the groups of at least min_members get the key (2^31 - 1 - count) << 32 | label and are sorted once more;
 *  fofSumKernel, a wave per group, sums pieces of 32 members in ascending order, a lane per piece, and adds the pieces
 *  in piece order.
 *
 *  Resources (compiler report, profiles/r15/fof/README.md): no scratch; the link kernel keeps 1.25 KiB of LDS per
 *  wave. No matrix instructions: the distances are 3-D and almost all of them are never formed.
 */
#include <climits>
#include <cmath>

#include "common.h"
#include "hip_api.h"

namespace sphx::hip
{

namespace
{

constexpr int kItem      = 64; // target positions per item: a wave
constexpr int kChunk     = 64; // staged sources per chunk
constexpr int kLinkBlock = 256;
constexpr int kLinkWaves = kLinkBlock / kWave;
constexpr uint64_t kNoKeyBit = uint64_t(1) << 63; // keys of particles (groups) that take no part: behind all others
constexpr int kLabelShift    = 30;                // catalogue keys: label << 30 | particle

/*! The sample sort handles runs of more than 2048 equal keys slowly (one wave sorts such a bucket in global memory),
 *  and a collapsed core puts far more particles than that into one cell, and a halo into one label. So the keys are
 *  made distinct wherever the bits allow: cell << shift | particle (shift = bits of the particle count; 0, the bare
 *  cell index, only if cell and particle bits together exceed 63), label << 30 | particle, and the keys of what
 *  takes no part carry their own index below the top bit. What a key names is key >> shift. */
__device__ __forceinline__ bool noKey(uint64_t key) { return (key & kNoKeyBit) != 0; }

__device__ __forceinline__ int clampI(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__global__ void __launch_bounds__(256)
fofKeysKernel(int64_t np, const double* __restrict__ x, const double* __restrict__ y, const double* __restrict__ z,
              const uint8_t* __restrict__ select, FofGrid g, int shift, uint64_t* __restrict__ keys,
              float4* __restrict__ rec)
{
    const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= np) return;
    int cx = 0, cy = 0, cz = 0;
    float4 r{0.f, 0.f, 0.f, 0.f};
    const bool sel = (!select || select[i]) && fofCell(g, 0, x[i], cx, r.x) && fofCell(g, 1, y[i], cy, r.y) &&
                     fofCell(g, 2, z[i], cz, r.z);
    r.w     = __int_as_float(cx);
    const uint64_t cell = uint64_t(fofKey(g, cx, cy, cz));
    keys[i] = sel ? (shift ? (cell << shift | uint64_t(i)) : cell) : (kNoKeyBit | uint64_t(i));
    rec[i]  = r;
}

//! flags[p] = 1 where a run of equal key >> shift starts (a key that takes no part starts none), flags[n] = 0 for the
//! scan's total
__global__ void __launch_bounds__(256)
fofFlagsKernel(int64_t n, int shift, const uint64_t* __restrict__ keys, int64_t* __restrict__ flags)
{
    const int64_t p = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (p > n) return;
    flags[p] = (p < n && !noKey(keys[p]) && (p == 0 || keys[p - 1] >> shift != keys[p] >> shift)) ? 1 : 0;
}

//! counts: [0] selected particles, [1] occupied cells (both stay 0 when nothing is selected)
__global__ void __launch_bounds__(256)
fofCellsKernel(int64_t np, int shift, const uint64_t* __restrict__ keys, const int64_t* __restrict__ scan,
               const int32_t* __restrict__ perm, const float4* __restrict__ recIn, float4* __restrict__ rec,
               int32_t* __restrict__ cellOf, int32_t* __restrict__ cellStart, int64_t* __restrict__ cellKey,
               int32_t* __restrict__ parent, int32_t* __restrict__ least, int64_t* __restrict__ counts)
{
    const int64_t p = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (p >= np) return;
    const uint64_t key = keys[p];
    const bool sel     = !noKey(key);
    const bool start   = sel && (p == 0 || keys[p - 1] >> shift != key >> shift);
    const int32_t c    = int32_t(scan[p]) - (start ? 0 : 1);
    cellOf[p]          = sel ? c : -1;
    rec[p]             = recIn[clampI(perm[p], 0, int(np - 1))];
    if (start)
    {
        cellStart[c] = int32_t(p);
        cellKey[c]   = int64_t(key >> shift);
        parent[c]    = c;
        least[c]     = INT_MAX;
    }
    if (sel && (p + 1 == np || noKey(keys[p + 1])))
    {
        counts[0]        = p + 1;
        counts[1]        = c + 1;
        cellStart[c + 1] = int32_t(p + 1);
    }
}

//! items that start at cell c (see 3. above); icount has np + 1 entries, those from the cell count on are 0
__global__ void __launch_bounds__(256)
fofItemCountKernel(int64_t np, int nx, const int64_t* __restrict__ counts, const int32_t* __restrict__ cellStart,
                   const int64_t* __restrict__ cellKey, int64_t* __restrict__ icount)
{
    const int64_t c = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (c > np) return;
    int64_t k = 0;
    if (c < counts[1])
    {
        const int s = cellStart[c], t = cellStart[c + 1], size = t - s;
        if (size > kItem) k = (size + kItem - 1) / kItem;
        else
        {
            bool start = c == 0;
            if (!start)
            {
                const int ps    = cellStart[c - 1];
                const bool cuts = (t - 1) / kItem != s / kItem, prevCuts = (s - 1) / kItem != ps / kItem;
                start = cellKey[c] / nx != cellKey[c - 1] / nx || cuts || prevCuts || s - ps > kItem ||
                        s / kItem != ps / kItem;
            }
            k = start ? 1 : 0;
        }
    }
    icount[c] = k;
}

//! itemStart[i] = first sorted position of item i; the entry behind the last item is the selected count. counts[2]
__global__ void __launch_bounds__(256)
fofItemFillKernel(int64_t np, int64_t* __restrict__ counts, const int32_t* __restrict__ cellStart,
                  const int64_t* __restrict__ ioff, int32_t* __restrict__ itemStart)
{
    const int64_t c      = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    const int64_t ncells = counts[1];
    if (c > ncells) return;
    const int64_t o = ioff[c];
    if (c == ncells)
    {
        counts[2] = o;
        if (o <= np) itemStart[o] = int32_t(counts[0]);
        return;
    }
    const int64_t k = ioff[c + 1] - o;
    for (int64_t j = 0; j < k; ++j)
        if (o + j < np) itemStart[o + j] = cellStart[c] + int32_t(j) * kItem;
}

/*! @brief first index in [0, n) whose key is >= v (n: none), found by the whole wave: 64 probes per pass, the ballot
 *         of "below v" is a prefix of the lanes. The new range lies between two neighbouring probes: it is shorter
 *         than the stride, which is 1/64 of the old range rounded up, so the loop ends after log64(n) + 1 passes */
__device__ __forceinline__ int waveLowerBound(const int64_t* __restrict__ keys, int n, int64_t v)
{
    int lo = 0, hi = n;
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

struct FofLinkArgs
{
    FofGrid g;
    Box box;
    int ns, ncells;
    int64_t nItems;
    const int32_t *itemStart, *cellStart, *cellOf, *perm;
    const int64_t* cellKey;
    const float4* rec;
    const double *x, *y, *z;
    int32_t* parent;
    unsigned long long* stats; // null: not counted. [0] cell pairs entered, [1] of those skipped by equal roots,
                               // [2] particle pairs tested, [3] of those re-tested in fp64
};

__global__ void __launch_bounds__(kLinkBlock) fofLinkKernel(FofLinkArgs A)
{
    __shared__ float4 sRec[kLinkWaves][kChunk];
    __shared__ int sCell[kLinkWaves][kChunk];

    const int wave = threadIdx.x >> 6, lane = laneId();
    const int64_t item = int64_t(blockIdx.x) * kLinkWaves + wave;
    if (item >= A.nItems) return; // (waves never meet at a block barrier)
    const FofGrid& g = A.g;

    const int t0   = clampI(A.itemStart[item], 0, A.ns - 1);
    const int nt   = clampI(A.itemStart[item + 1] - t0, 1, sphx::smin(kItem, A.ns - t0));
    const bool valid = lane < nt;
    const int tq     = t0 + (valid ? lane : 0);
    const float4 tr  = A.rec[tq];
    const int myCell = clampI(A.cellOf[tq], 0, A.ncells - 1);
    const int tcx    = __float_as_int(tr.w);

    // the item's row and its extent in x (the targets are sorted by cell)
    const int64_t key0 = A.cellKey[__builtin_amdgcn_readfirstlane(myCell)];
    const int cxLo = int(key0 % g.n[0]), cy = int(key0 / g.n[0] % g.n[1]),
              cz = int(key0 / (int64_t(g.n[0]) * g.n[1]));
    const int cxHi = __shfl(tcx, nt - 1);

    // the lanes of this lane's own cell, as a mask: the lanes from the cell's first lane to the next cell's
    const int before     = __shfl_up(myCell, 1);
    const bool head      = valid && (lane == 0 || before != myCell);
    const uint64_t heads = ballot(head);
    const uint64_t upto  = lanemaskLt() | (uint64_t(1) << lane);
    const int gs         = 63 - clz64(heads & upto);
    const uint64_t above = heads & ~upto;
    const int ge         = above ? ctz64(above) : nt;
    const uint64_t myGroup = (ge >= 64 ? ~uint64_t(0) : (uint64_t(1) << ge) - 1) & ~((uint64_t(1) << gs) - 1);

    const float rx = float(g.e[0] / g.b), ry = float(g.e[1] / g.b), rz = float(g.e[2] / g.b);
    int myRoot = myCell; // the last root seen of the own cell: always in its component
    unsigned long long nEntered = 0, nSkipped = 0, nTested = 0, nExact = 0;

    const int nRuns = fofNumRuns(g);
    for (int r = 0; r < nRuns; ++r)
        for (int piece = 0; piece < 2; ++piece)
        {
            FofRun run;
            if (!fofRun(g, r, piece, cxLo, cxHi, cy, cz, run)) continue;
            const int cb0 = waveLowerBound(A.cellKey, A.ncells, run.kLo);
            if (cb0 >= A.ncells || A.cellKey[cb0] > run.kHi) continue;
            const float fdy = float(run.dy), fdz = float(run.dz);
            int pos  = A.cellStart[cb0]; // wave-uniform, grows in every pass of the loop below
            int base = -1;
            while (pos >= 0 && pos < A.ns)
            {
                if (base < 0 || pos >= base + kChunk)
                {
                    base = pos;
                    __builtin_amdgcn_wave_barrier(); // the chunk before has been read
                    if (base + lane < A.ns)
                    {
                        sRec[wave][lane]  = A.rec[base + lane];
                        sCell[wave][lane] = A.cellOf[base + lane];
                    }
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                }
                // entering (or, behind a chunk boundary, re-entering) source cell B
                const int cB = clampI(__builtin_amdgcn_readfirstlane(sCell[wave][pos - base]), 0, A.ncells - 1);
                const int64_t kB = A.cellKey[cB];
                if (kB > run.kHi) break;
                const int endB = clampI(A.cellStart[cB + 1], pos + 1, A.ns);
                int ddx;
                bool need = valid && fofInStencil(g, r == 0, tcx, int(kB - run.rowBase), ddx);
                uint64_t nm = ballot(need);
                if (nm == 0)
                {
                    pos = endB;
                    continue;
                }
                const int rootB = fofFind(A.parent, cB);
                if (need)
                {
                    myRoot = fofFind(A.parent, myRoot);
                    need   = myRoot != rootB;
                }
                const uint64_t entered = nm & heads; // one lane per target cell that has B in its stencil
                nm                     = ballot(need);
                nEntered += popcount64(entered);
                nSkipped += popcount64(entered & ~nm);
                const float fdx = float(ddx);
                const int jEnd  = sphx::smin(endB, base + kChunk);
                int j           = pos;
                while (nm != 0 && j < jEnd)
                {
                    bool hit = false;
                    if (need)
                    {
                        const float4 s = sRec[wave][j - base];
                        int t = fofPairF32((fdx + (s.x - tr.x)) * rx, (fdy + (s.y - tr.y)) * ry,
                                           (fdz + (s.z - tr.z)) * rz);
                        if (t < 0)
                        {
                            const int64_t i = A.perm[tq], k = A.perm[j];
                            t = fofPairExact(A.x[i], A.y[i], A.z[i], A.x[k], A.y[k], A.z[k], A.box, g.b) ? 1 : 0;
                            ++nExact;
                        }
                        hit = t > 0;
                    }
                    nTested += popcount64(nm);
                    const uint64_t hm = ballot(hit);
                    if (hm != 0)
                    {
                        if (hit && (hm & myGroup & lanemaskLt()) == 0) fofUnion(A.parent, myRoot, rootB);
                        if (hm & myGroup) need = false;
                        nm = ballot(need);
                    }
                    ++j;
                }
                pos = nm != 0 ? j : endB;
            }
        }

    if (A.stats)
    {
        nExact = waveSum(nExact);
        if (lane == 0)
        {
            atomicAdd(A.stats + 0, nEntered);
            atomicAdd(A.stats + 1, nSkipped);
            atomicAdd(A.stats + 2, nTested);
            atomicAdd(A.stats + 3, nExact);
        }
    }
}

__global__ void __launch_bounds__(256)
fofFlattenKernel(int ncells, int64_t np, const int32_t* __restrict__ parent, const int32_t* __restrict__ cellStart,
                 const int32_t* __restrict__ perm, int32_t* __restrict__ root, int32_t* __restrict__ least)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= ncells) return;
    const int r = fofFind(parent, c);
    root[c]     = r;
    atomicMin(least + r, perm[clampI(cellStart[c], 0, int(np - 1))]);
}

__global__ void __launch_bounds__(256)
fofLabelKernel(int64_t np, int ncells, const int32_t* __restrict__ cellOf, const int32_t* __restrict__ perm,
               const int32_t* __restrict__ root, const int32_t* __restrict__ least, int32_t* __restrict__ label)
{
    const int64_t p = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (p >= np) return;
    const int c = cellOf[p];
    label[clampI(perm[p], 0, int(np - 1))] = (c >= 0 && c < ncells) ? least[clampI(root[c], 0, ncells - 1)] : -1;
}

// ---------------------------------------------------------------------------------------------------- catalogue

__global__ void __launch_bounds__(256)
fofLabelKeysKernel(int64_t n, const int32_t* __restrict__ label, uint64_t* __restrict__ keys)
{
    const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n) return;
    keys[i] = label[i] < 0 ? (kNoKeyBit | uint64_t(i)) : (uint64_t(label[i]) << kLabelShift | uint64_t(i));
}

//! counts: [0] groups. gstart[g] = first sorted position of group g, behind the last group: the labelled count
__global__ void __launch_bounds__(256)
fofGroupStartsKernel(int64_t n, const uint64_t* __restrict__ keys, const int64_t* __restrict__ scan,
                     int32_t* __restrict__ gstart, int64_t* __restrict__ counts)
{
    const int64_t p = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const uint64_t key = keys[p];
    if (noKey(key)) return;
    const bool start = p == 0 || keys[p - 1] >> kLabelShift != key >> kLabelShift;
    const int64_t gi = scan[p] - (start ? 0 : 1);
    if (start) gstart[gi] = int32_t(p);
    if (p + 1 == n || noKey(keys[p + 1]))
    {
        gstart[gi + 1] = int32_t(p + 1);
        counts[0]      = gi + 1;
    }
}

//! order keys of the groups: (2^31 - 1 - count) << 32 | label for those that are kept, behind them the others.
//! counts[1] = groups kept
__global__ void __launch_bounds__(256)
fofGroupKeysKernel(int64_t minMembers, const uint64_t* __restrict__ keys, const int32_t* __restrict__ gstart,
                   int64_t* __restrict__ counts, uint64_t* __restrict__ okeys)
{
    const int64_t gi = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (gi >= counts[0]) return;
    const int64_t count = gstart[gi + 1] - gstart[gi];
    const bool keep     = count >= minMembers;
    okeys[gi] = keep ? (uint64_t(0x7fffffff - count) << 32 | keys[gstart[gi]] >> kLabelShift)
                     : (kNoKeyBit | uint64_t(gi));
    if (keep) atomicAdd(reinterpret_cast<unsigned long long*>(counts + 1), 1ull);
}

struct FofSumArgs
{
    int64_t n, G, Gall;
    const int32_t *perm2, *gstart, *perm;
    const uint64_t* keys;
    const double *x, *y, *z, *m, *vx, *vy, *vz;
    Box box;
    int32_t* label;
    int64_t* count;
    double *mass, *com, *vel;
};

//! a wave per group: lane l sums the piece of kFofPiece members l of a pass in ascending order, the pieces are added in
//! piece order (every lane forms the same total); every product is rounded on its own, as on the host
__global__ void __launch_bounds__(256) fofSumKernel(FofSumArgs A)
{
#pragma clang fp contract(off)
    const int lane  = laneId();
    const int64_t k = int64_t(blockIdx.x) * (256 / kWave) + (threadIdx.x >> 6);
    if (k >= A.G) return;
    const int64_t gi = clampI(A.perm2[k], 0, int(A.Gall - 1));
    const int64_t s0 = clampI(A.gstart[gi], 0, int(A.n - 1));
    const int64_t s1 = clampI(A.gstart[gi + 1], int(s0 + 1), int(A.n));
    const int i0     = clampI(A.perm[s0], 0, int(A.n - 1)); // the group's smallest particle: its label, the root
    const double x0 = A.x[i0], y0 = A.y[i0], z0 = A.z[i0];
    double acc[7];
#pragma unroll
    for (int q = 0; q < 7; ++q)
        acc[q] = 0.0;
    for (int64_t pass = s0; pass < s1; pass += int64_t(kWave) * kFofPiece)
    {
        double ps[7];
#pragma unroll
        for (int q = 0; q < 7; ++q)
            ps[q] = 0.0;
        const int64_t a = pass + int64_t(lane) * kFofPiece, b = sphx::smin(a + kFofPiece, s1);
        for (int64_t p = a; p < b; ++p)
        {
            const int j     = clampI(A.perm[p], 0, int(A.n - 1));
            const double mj = A.m[j];
            ps[0] += mj;
            ps[1] += mj * fofMinImage(A.x[j] - x0, A.box, 0);
            ps[2] += mj * fofMinImage(A.y[j] - y0, A.box, 1);
            ps[3] += mj * fofMinImage(A.z[j] - z0, A.box, 2);
            if (A.vx)
            {
                ps[4] += mj * A.vx[j];
                ps[5] += mj * A.vy[j];
                ps[6] += mj * A.vz[j];
            }
        }
        const int pieces = int(sphx::smin(int64_t(kWave), (s1 - pass + kFofPiece - 1) / kFofPiece));
        for (int l = 0; l < pieces; ++l)
#pragma unroll
            for (int q = 0; q < 7; ++q)
                acc[q] += readLaneD(ps[q], l);
    }
    if (lane != 0) return;
    double cx = x0 + acc[1] / acc[0], cy = y0 + acc[2] / acc[0], cz = z0 + acc[3] / acc[0];
    putInBox(cx, cy, cz, A.box);
    A.label[k]       = int32_t(A.keys[s0] >> kLabelShift);
    A.count[k]       = s1 - s0;
    A.mass[k]        = acc[0];
    A.com[3 * k]     = cx;
    A.com[3 * k + 1] = cy;
    A.com[3 * k + 2] = cz;
    if (A.vx)
        for (int a = 0; a < 3; ++a)
            A.vel[3 * k + a] = acc[4 + a] / acc[0];
}

} // namespace

void fofPrepare(int64_t np, const double* x, const double* y, const double* z, const uint8_t* select,
                const FofGrid& g, const FofBuffers& B, hipStream_t s)
{
    if (np < 1 || np > kFofMaxN) throw std::invalid_argument("fof: between 1 and 2^30 particles");
    const unsigned nb = gridFor(np + 1, 256);
    // distinct keys cell << shift | particle where 63 bits hold both (see noKey above)
    const int cellBits = 64 - clz64(uint64_t(int64_t(g.n[0]) * g.n[1] * g.n[2] - 1));
    const int partBits = sphx::smax(1, 64 - clz64(uint64_t(np - 1)));
    const int shift    = cellBits + partBits <= 63 ? partBits : 0;
    fofKeysKernel<<<nb, 256, 0, s>>>(np, x, y, z, select, g, shift, B.keys, B.recIn);
    SPHX_LAUNCH_CHECK();
    sortKeys(np, B.keys, B.keysSorted, B.perm, B.tmp, B.tmpBytes, s);
    fofFlagsKernel<<<nb, 256, 0, s>>>(np, shift, B.keysSorted, B.scan);
    SPHX_LAUNCH_CHECK();
    exclusiveScanI64(B.scan, B.scan, np + 1, B.tmp, B.tmpBytes, s);
    fofCellsKernel<<<nb, 256, 0, s>>>(np, shift, B.keysSorted, B.scan, B.perm, B.recIn, B.rec, B.cellOf, B.cellStart,
                                      B.cellKey, B.parent, B.least, B.counts);
    SPHX_LAUNCH_CHECK();
    fofItemCountKernel<<<nb, 256, 0, s>>>(np, g.n[0], B.counts, B.cellStart, B.cellKey, B.scan);
    SPHX_LAUNCH_CHECK();
    exclusiveScanI64(B.scan, B.scan, np + 1, B.tmp, B.tmpBytes, s);
    fofItemFillKernel<<<nb, 256, 0, s>>>(np, B.counts, B.cellStart, B.scan, B.itemStart);
    SPHX_LAUNCH_CHECK();
}

void fofLink(int64_t np, int64_t ns, int64_t ncells, int64_t nItems, const double* x, const double* y, const double* z,
             const Box& box, const FofGrid& g, const FofBuffers& B, unsigned long long* stats, int32_t* label,
             hipStream_t s)
{
    if (np < 1 || np > kFofMaxN || ns < 0 || ns > np || ncells < 0 || ncells > ns || nItems < 0 || nItems > ns ||
        (ns > 0 && (ncells < 1 || nItems < 1)))
        throw std::invalid_argument("fof: inconsistent counts");
    if (nItems > 0)
    {
        const FofLinkArgs A{g, box, int(ns), int(ncells), nItems, B.itemStart, B.cellStart, B.cellOf, B.perm,
                            B.cellKey, B.rec, x, y, z, B.parent, stats};
        fofLinkKernel<<<gridFor(nItems, kLinkWaves), kLinkBlock, 0, s>>>(A);
        SPHX_LAUNCH_CHECK();
        fofFlattenKernel<<<gridFor(ncells, 256), 256, 0, s>>>(int(ncells), np, B.parent, B.cellStart, B.perm, B.root,
                                                              B.least);
        SPHX_LAUNCH_CHECK();
    }
    fofLabelKernel<<<gridFor(np, 256), 256, 0, s>>>(np, int(ncells), B.cellOf, B.perm, B.root, B.least, label);
    SPHX_LAUNCH_CHECK();
}

void fofGroups(int64_t n, const int32_t* label, int64_t minMembers, uint64_t* keys, uint64_t* keysSorted,
               int32_t* perm, int64_t* scan, int32_t* gstart, int64_t* counts, void* tmp, size_t tmpBytes,
               hipStream_t s)
{
    if (n < 1 || n > kFofMaxN) throw std::invalid_argument("fof: between 1 and 2^30 particles");
    const unsigned nb = gridFor(n + 1, 256);
    fofLabelKeysKernel<<<nb, 256, 0, s>>>(n, label, keys);
    SPHX_LAUNCH_CHECK();
    sortKeys(n, keys, keysSorted, perm, tmp, tmpBytes, s);
    fofFlagsKernel<<<nb, 256, 0, s>>>(n, kLabelShift, keysSorted, scan);
    SPHX_LAUNCH_CHECK();
    exclusiveScanI64(scan, scan, n + 1, tmp, tmpBytes, s);
    fofGroupStartsKernel<<<nb, 256, 0, s>>>(n, keysSorted, scan, gstart, counts);
    SPHX_LAUNCH_CHECK();
    // (the unsorted label keys are done with: their buffer takes the groups' order keys)
    fofGroupKeysKernel<<<nb, 256, 0, s>>>(minMembers, keysSorted, gstart, counts, keys);
    SPHX_LAUNCH_CHECK();
}

void fofSums(int64_t n, int64_t Gall, int64_t G, const int32_t* perm2, const int32_t* gstart, const int32_t* perm,
             const uint64_t* keysSorted, const double* x, const double* y, const double* z, const double* m,
             const double* vx, const double* vy, const double* vz, const Box& box, int32_t* label, int64_t* count,
             double* mass, double* com, double* vel, hipStream_t s)
{
    if (G < 1) return;
    if (n < 1 || Gall < G || Gall > n) throw std::invalid_argument("fof: inconsistent group counts");
    const FofSumArgs A{n, G, Gall, perm2, gstart, perm, keysSorted, x, y, z, m, vx, vy, vz, box, label, count, mass,
                       com, vel};
    fofSumKernel<<<gridFor(G, 256 / kWave), 256, 0, s>>>(A);
    SPHX_LAUNCH_CHECK();
}

} // namespace sphx::hip
