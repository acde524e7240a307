/*! SPH volumes on regular 3-D grids on gfx950: particles are binned to bricks of 8x8x8 voxels, every brick sums its own
 *  sorted list (definitions: ops/volume.py; host form: cpu/volume_cpu.cpp), and the shell binning of a power spectrum.
 *
 *  1. volumeRecordsKernel, one thread per particle: the voxel-space centre and 1/h_eff are formed in fp64 and rounded
 *     once to fp32 into a 32-B record {cx, cy, cz, 1/h_eff, w0..w3}. The thread counts the (periodic image, brick) pairs
 *     that the bounding box of the footprint overlaps, for every image shift in {-1, 0, 1}^3 that meets the window.
 *  2. An exclusive scan of the counts sizes the entry list (the one host synchronisation); volumeFillKernel writes the
 *     keys brick << 35 | particle << 5 | shift code (particles < 2^30, bricks < 2^29, 27 shift codes) from the same fp32
 *     footprint function the count used; the project's sample sort orders them by (brick, particle, shift). The order
 *     of every brick's sum is thereby fixed: the volume is bit-reproducible from run to run.
 *  3. volumeRangesKernel finds every brick's range in the sorted keys and cuts it into segments of at most S entries;
 *     a scan of the segment counts numbers the (brick, segment) blocks.
 *  4. volumeBrickKernel<C>, 512 threads = 8 waves per (brick, segment): a wave owns one 4x4x4 sub-brick, a lane one
 *     voxel with C accumulators. The block walks its entries in batches of 512: each thread gathers one entry's record
 *     (the key two batches and the record one batch ahead of the batch being consumed), applies the entry's periodic
 *     shift, folds K h^-3 into the weights and stores the entry into LDS as {cx, cy, cz, 1/h} (one 16-B read) next to
 *     its C weights (one read of 4 C bytes). A spectrum grid is matched to the particle count: h is 1-2 voxels, the
 *     footprint a ball 6-7 voxels across whose bounding box meets ~6 bricks, 3000 voxels for 150 hits. So the culling
 *     has a level of its own below the brick: every wave tests the 512 staged balls 64 at a time against its own
 *     sub-brick by the clamped point-to-box distance in units of h (exact for the sphere, and for the ellipsoid that
 *     it is in voxel space when the voxel edges differ; not the bounding box), ballot-compacts the survivors into its
 *     own LDS index list and its lanes loop over those only, reading each survivor by LDS broadcast. Per voxel and
 *     entry: q^2 = |p - c|^2 / h^2 and, inside the support, acc_c += w_c sinc^n. For r = 3.3 voxels the ball plus
 *     4^3-cube Minkowski volume is ~940 voxel tests per particle for 150 hits, three times the brick-level box.
 *  5. A brick of one segment stores its voxels to the volume (clipped: grids need not be multiples of 8); the segments
 *     of a longer list store partial bricks to a workspace and volumeSumKernel adds them in segment order.
 *
 *  Resources per block (compiler report, profiles/r14/volume/README.md): 512 threads, LDS 18 / 20 / 24 KiB for
 *  C = 1 / 2 / 4 (8 KiB entries + 2 C KiB weights + 8 KiB survivor lists), 60 / 61 / 66 VGPRs, 4 / 4 / 3 blocks per CU,
 *  no scratch. The segment length S defaults to 4096 (ops/volume.py). No matrix instructions: the distances are
 *  3-D (K = 3, as image.hip argues), the cost is the culling and the sine per voxel.
 *
 *  spectrumShellsKernel bins the half spectrum of torch.fft.rfftn into shells b = floor(|k| + 0.5): fp64 LDS bins per
 *  block, per-block partial rows, summed in block order by spectrumSumKernel (ops/spectrum.py).
 */
#include <cmath>

#include "common.h"
#include "hip_api.h"

namespace sphx::hip
{

namespace
{

constexpr int kBrick      = 8;
constexpr int kBrickVox   = kBrick * kBrick * kBrick;
constexpr int kBrickBlock = 512;
constexpr int kBrickWaves = kBrickBlock / kWave;
constexpr int kShiftBits  = 5;
constexpr int kPartBits   = 30;
constexpr int kBrickShift = kShiftBits + kPartBits;
constexpr int kBrickBits  = 29;

//! the window in voxels, as the device sees it
struct VolumeGeom
{
    int n[3], nb[3], per[3];
    float Lvox[3]; // periodic image shifts in voxels
    float a[3];    // voxel edges
};

VolumeGeom geomOf(const VolumeView& V)
{
    VolumeGeom g;
    for (int d = 0; d < 3; ++d)
    {
        g.n[d]    = V.n[d];
        g.nb[d]   = (V.n[d] + kBrick - 1) / kBrick;
        g.per[d]  = V.per[d];
        g.Lvox[d] = float(V.L[d] / V.d[d]);
        g.a[d]    = float(V.d[d]);
    }
    return g;
}

int64_t bricksOf(const VolumeGeom& g) { return int64_t(g.nb[0]) * g.nb[1] * g.nb[2]; }

/*! @brief voxels of one axis whose centres (k + 0.5) lie within r of c, widened by 2^-10 voxel (the voxel test itself
 *         is q^2 < 4 in fp32; the box only has to contain it), clipped to [0, n). Written with explicit single
 *         roundings: the count and the fill must see the same box. A record that is not finite has no entries. */
__device__ __forceinline__ bool voxelRange(float c, float r, int n, int& k0, int& k1)
{
    const float pad = 0.5f + 0.0009765625f;
    float lo        = __fsub_rn(__fsub_rn(c, r), pad);
    float hi        = __fadd_rn(__fadd_rn(c, r), pad - 1.0f);
    lo              = fmaxf(ceilf(lo), 0.0f);
    hi              = fminf(floorf(hi), float(n - 1));
    k0              = int(lo);
    k1              = int(hi);
    return r >= 0.0f && c == c && lo <= hi; // (a NaN radius or centre: no entries; fmaxf / fminf would drop the NaN)
}

//! @brief half extent of the footprint along one axis in voxels: 2 h / edge, rounded up by 2^-20 (the fp32 rounding of
//!        the extent and of q^2); NaN for a 1/h that is NaN
__device__ __forceinline__ float halfExtent(float ih, float a)
{
    return __fmul_rn(__fdiv_rn(2.0f, __fmul_rn(a, ih)), 1.0f + 9.5367431640625e-7f);
}

//! @brief centre coordinate of the periodic image s of a record, in voxels
__device__ __forceinline__ float shifted(float c, int s, float Lvox) { return __fmaf_rn(float(s), Lvox, c); }

//! @brief calls f(brick, shift code) for every (periodic image, brick) the record's footprint box overlaps
template<class F>
__device__ __forceinline__ void forEachBrick(const VolumeRec& r, const VolumeGeom& g, F&& f)
{
    const float rx = halfExtent(r.ih, g.a[0]), ry = halfExtent(r.ih, g.a[1]), rz = halfExtent(r.ih, g.a[2]);
    const int mx = g.per[0] ? 1 : 0, my = g.per[1] ? 1 : 0, mz = g.per[2] ? 1 : 0;
    for (int sz = -mz; sz <= mz; ++sz)
    {
        int k0, k1;
        if (!voxelRange(shifted(r.cz, sz, g.Lvox[2]), rz, g.n[2], k0, k1)) continue;
        for (int sy = -my; sy <= my; ++sy)
        {
            int j0, j1;
            if (!voxelRange(shifted(r.cy, sy, g.Lvox[1]), ry, g.n[1], j0, j1)) continue;
            for (int sx = -mx; sx <= mx; ++sx)
            {
                int i0, i1;
                if (!voxelRange(shifted(r.cx, sx, g.Lvox[0]), rx, g.n[0], i0, i1)) continue;
                const int code = ((sz + 1) * 3 + (sy + 1)) * 3 + (sx + 1);
                for (int bz = k0 / kBrick; bz <= k1 / kBrick; ++bz)
                    for (int by = j0 / kBrick; by <= j1 / kBrick; ++by)
                        for (int bx = i0 / kBrick; bx <= i1 / kBrick; ++bx)
                            f((int64_t(bz) * g.nb[1] + by) * g.nb[0] + bx, code);
            }
        }
    }
}

__global__ void __launch_bounds__(256)
volumeRecordsKernel(int64_t first, int64_t last, int64_t n, const double* __restrict__ x, const double* __restrict__ y,
                    const double* __restrict__ z, const float* __restrict__ h, const float* __restrict__ w, int C,
                    VolumeView V, VolumeGeom g, VolumeRec* __restrict__ rec, int64_t* __restrict__ counts)
{
    const int64_t k = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    const int64_t i = first + k;
    if (i > last) return;
    if (i == last)
    {
        counts[k] = 0; // the scan's last element: its result is the total
        return;
    }
    const double hj = sphx::smax(double(h[i]), V.hMin);
    VolumeRec r;
    r.cx = float((x[i] - V.lo[0]) / V.d[0]);
    r.cy = float((y[i] - V.lo[1]) / V.d[1]);
    r.cz = float((z[i] - V.lo[2]) / V.d[2]);
    r.ih = float(1.0 / hj);
#pragma unroll
    for (int c = 0; c < 4; ++c)
        r.w[c] = c < C ? w[int64_t(c) * n + i] : 0.0f;
    rec[k]    = r;
    int64_t c = 0;
    forEachBrick(r, g, [&](int64_t, int) { ++c; });
    counts[k] = c;
}

__global__ void __launch_bounds__(256)
volumeFillKernel(int64_t np, VolumeGeom g, const VolumeRec* __restrict__ rec, const int64_t* __restrict__ offsets,
                 uint64_t* __restrict__ keys)
{
    const int64_t k = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (k >= np) return;
    int64_t pos       = offsets[k];
    const int64_t end = offsets[k + 1];
    forEachBrick(rec[k], g,
                 [&](int64_t brick, int code)
                 {
                     // (never beyond the particle's own slots, whatever the count was)
                     if (pos < end)
                         keys[pos++] = uint64_t(brick) << kBrickShift | uint64_t(k) << kShiftBits | uint64_t(code);
                 });
    for (; pos < end; ++pos)
        keys[pos] = ~uint64_t(0); // past every brick: in no brick's range
}

//! first position in the sorted keys whose key is >= v
__device__ __forceinline__ int64_t lowerBound(const uint64_t* __restrict__ keys, int64_t n, uint64_t v)
{
    int64_t lo = 0, hi = n;
    while (lo < hi)
    {
        const int64_t mid = (lo + hi) >> 1;
        if (keys[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

//! start[b] = first entry of brick b (b = nbricks: the end of the last brick), nseg[b] = blocks of brick b (at least
//! one: a brick without entries still stores its zeros), wseg[b] = partial bricks it needs in the workspace
__global__ void volumeRangesKernel(int64_t total, const uint64_t* __restrict__ keys, int64_t nbricks, int64_t segment,
                                   int64_t* __restrict__ start, int64_t* __restrict__ nseg, int64_t* __restrict__ wseg)
{
    const int64_t t = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (t > nbricks) return;
    const int64_t a = lowerBound(keys, total, uint64_t(t) << kBrickShift);
    start[t]        = a;
    if (t == nbricks)
    {
        nseg[t] = 0;
        wseg[t] = 0;
        return;
    }
    const int64_t b = lowerBound(keys, total, uint64_t(t + 1) << kBrickShift);
    const int64_t k = sphx::smax(int64_t(1), (b - a + segment - 1) / segment);
    nseg[t]         = k;
    wseg[t]         = k > 1 ? k : 0;
}

struct BrickArgs
{
    int64_t np, total;
    const uint64_t* keys;
    const VolumeRec* rec;
    VolumeGeom g;
    int64_t nbricks;
    int64_t segment;
    const int64_t* start;
    const int64_t* segOff;  // nbricks + 1: first block of every brick
    const int64_t* workOff; // nbricks + 1: first partial brick of every brick of several segments
    float* work;            // per partial brick: C x 512 sums, channel-major
    float* vol;
};

//! voxel of thread t in its brick: wave w owns the 4^3 sub-brick (w & 1, w >> 1 & 1, w >> 2), a lane one voxel of it
__device__ __forceinline__ void voxelOf(int t, int& sx, int& sy, int& sz, int& lx, int& ly, int& lz)
{
    const int lane = t & 63, wave = t >> 6;
    sx = 4 * (wave & 1);
    sy = 4 * ((wave >> 1) & 1);
    sz = 4 * (wave >> 2);
    lx = lane & 3;
    ly = (lane >> 2) & 3;
    lz = lane >> 4;
}

template<int C>
struct Weights;
template<>
struct Weights<1>
{
    using type = float;
};
template<>
struct Weights<2>
{
    using type = float2;
};
template<>
struct Weights<4>
{
    using type = float4;
};

template<int C>
__global__ void __launch_bounds__(kBrickBlock) volumeBrickKernel(BrickArgs A, KernelFn fn, float norm)
{
    using WT = typename Weights<C>::type;
    __shared__ float4 sP[kBrickBlock]; // {cx, cy, cz, 1/h} of the shifted image
    __shared__ WT sW[kBrickBlock];     // weights x K h^-3 / wqScale
    __shared__ uint16_t sList[kBrickWaves][kBrickBlock];

    const int64_t b = blockIdx.x;
    if (b >= A.segOff[A.nbricks]) return; // (the grid is the host's upper bound of the block count)
    // brick of this block: the last t with segOff[t] <= b
    int64_t brick;
    {
        int64_t lo = 0, hi = A.nbricks;
        while (hi - lo > 1)
        {
            const int64_t mid = (lo + hi) >> 1;
            if (A.segOff[mid] <= b) lo = mid;
            else hi = mid;
        }
        brick = lo;
    }
    SPHX_DCHECK(brick >= 0 && brick < A.nbricks && A.segOff[brick] <= b && b < A.segOff[brick + 1], 8);
    const int64_t seg0 = A.segOff[brick];
    const int64_t nseg = A.segOff[brick + 1] - seg0;
    const int64_t bEnd = A.start[brick + 1];
    const int64_t e0   = sphx::smin(A.start[brick] + (b - seg0) * A.segment, bEnd);
    const int64_t e1   = sphx::smin(e0 + A.segment, bEnd);
    const int nBatch   = int((e1 - e0 + kBrickBlock - 1) / kBrickBlock);
    const int tid      = threadIdx.x;
    const int wave     = tid >> 6;
    const int bx = int(brick % A.g.nb[0]), by = int(brick / A.g.nb[0] % A.g.nb[1]),
              bz = int(brick / (int64_t(A.g.nb[0]) * A.g.nb[1]));
    int sx, sy, sz, lx, ly, lz;
    voxelOf(tid, sx, sy, sz, lx, ly, lz);
    const int vx = bx * kBrick + sx + lx, vy = by * kBrick + sy + ly, vz = bz * kBrick + sz + lz;
    // the voxel's centre and the extent of the centres of the wave's sub-brick
    const float fx = float(vx) + 0.5f, fy = float(vy) + 0.5f, fz = float(vz) + 0.5f;
    const float x0 = float(bx * kBrick + sx) + 0.5f, x1 = x0 + 3.0f;
    const float y0 = float(by * kBrick + sy) + 0.5f, y1 = y0 + 3.0f;
    const float z0 = float(bz * kBrick + sz) + 0.5f, z1 = z0 + 3.0f;
    const float ax = A.g.a[0], ay = A.g.a[1], az = A.g.a[2];

    float acc[C];
#pragma unroll
    for (int c = 0; c < C; ++c)
        acc[c] = 0.0f;

    const float4* rec4 = reinterpret_cast<const float4*>(A.rec);
    auto loadKey       = [&](int batch) -> uint64_t
    {
        const int64_t e = e0 + int64_t(batch) * kBrickBlock + tid;
        return e < e1 ? A.keys[e] : ~uint64_t(0);
    };
    // record index of a key (the fill's padding keys and slots past the range: record 0, marked not staged)
    auto recIndex = [&](uint64_t key, bool& valid) -> int64_t
    {
        int64_t j = int64_t((key >> kShiftBits) & ((uint64_t(1) << kPartBits) - 1));
        valid     = key != ~uint64_t(0);
        SPHX_DCHECK(!valid || j < A.np, 9);
        return (valid && j < A.np) ? j : 0;
    };

    uint64_t keyCur = loadKey(0), keyNext = loadKey(1);
    bool validCur;
    int64_t j = recIndex(keyCur, validCur);
    float4 r0 = rec4[2 * j], r1 = rec4[2 * j + 1];

    for (int batch = 0; batch < nBatch; ++batch)
    {
        // the loads of the batches ahead: key of batch + 2, record of batch + 1
        const uint64_t keyNext2 = loadKey(batch + 2);
        bool validNext;
        const int64_t jn = recIndex(keyNext, validNext);
        const float4 n0 = rec4[2 * jn], n1 = rec4[2 * jn + 1];

        __syncthreads(); // the previous batch is consumed
        {
            const int code = int(keyCur & ((1u << kShiftBits) - 1));
            const int cz = code / 9 - 1, cy = code / 3 % 3 - 1, cx = code % 3 - 1;
            const float ih  = r0.w;
            const float wgt = norm * ih * ih * ih;
            // an unstaged slot lies at infinity for the cull (its record is read, never used)
            float4 p{3.0e38f, 3.0e38f, 3.0e38f, 1.0f};
            if (validCur)
                p = float4{shifted(r0.x, cx, A.g.Lvox[0]), shifted(r0.y, cy, A.g.Lvox[1]),
                           shifted(r0.z, cz, A.g.Lvox[2]), ih};
            sP[tid] = p;
            if constexpr (C == 1) sW[tid] = r1.x * wgt;
            if constexpr (C == 2) sW[tid] = float2{r1.x * wgt, r1.y * wgt};
            if constexpr (C == 4) sW[tid] = float4{r1.x * wgt, r1.y * wgt, r1.z * wgt, r1.w * wgt};
        }
        __syncthreads();

        // survivors of this wave's sub-brick, in entry order: the ball meets the box of the 4^3 voxel centres when the
        // centre's clamped distance to it, in units of h, is below 2 (2^-15 to spare: the voxel test rounds otherwise)
        int count = 0;
#pragma unroll
        for (int r = 0; r < kBrickBlock / kWave; ++r)
        {
            const int s    = r * kWave + laneId();
            const float4 p = sP[s];
            const float dx = fmaxf(fmaxf(x0 - p.x, p.x - x1), 0.0f) * (ax * p.w);
            const float dy = fmaxf(fmaxf(y0 - p.y, p.y - y1), 0.0f) * (ay * p.w);
            const float dz = fmaxf(fmaxf(z0 - p.z, p.z - z1), 0.0f) * (az * p.w);
            const bool hit = dx * dx + dy * dy + dz * dz < 4.0001220703125f;
            const uint64_t m = ballot(hit);
            if (hit) sList[wave][count + popcount64(m & lanemaskLt())] = uint16_t(s);
            count += popcount64(m);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

        for (int k = 0; k < count; ++k)
        {
            const int s    = sList[wave][k];
            const float4 p = sP[s];
            const WT w     = sW[s];
            const float du = (fx - p.x) * (ax * p.w);
            const float dv = (fy - p.y) * (ay * p.w);
            const float dw = (fz - p.z) * (az * p.w);
            const float q2 = du * du + dv * dv + dw * dw;
            if (q2 < 4.0f)
            {
                const float f = fn.wq(0.25f * sqrtF(q2));
                if constexpr (C == 1) acc[0] += w * f;
                if constexpr (C >= 2)
                {
                    acc[0] += w.x * f;
                    acc[1] += w.y * f;
                }
                if constexpr (C == 4)
                {
                    acc[2] += w.z * f;
                    acc[3] += w.w * f;
                }
            }
        }

        keyCur   = keyNext;
        keyNext  = keyNext2;
        validCur = validNext;
        r0       = n0;
        r1       = n1;
    }

    if (nseg == 1)
    {
        if (vx < A.g.n[0] && vy < A.g.n[1] && vz < A.g.n[2])
#pragma unroll
            for (int c = 0; c < C; ++c)
                A.vol[((size_t(c) * A.g.n[2] + vz) * A.g.n[1] + vy) * A.g.n[0] + vx] = acc[c];
    }
    else
    {
        float* out = A.work + size_t(A.workOff[brick] + (b - seg0)) * C * kBrickVox;
#pragma unroll
        for (int c = 0; c < C; ++c)
            out[c * kBrickBlock + tid] = acc[c];
    }
}

//! bricks of several segments: their partial bricks added in segment order
template<int C>
__global__ void __launch_bounds__(kBrickBlock) volumeSumKernel(BrickArgs A)
{
    const int64_t brick = blockIdx.x;
    const int64_t seg0  = A.segOff[brick];
    const int64_t nseg  = A.segOff[brick + 1] - seg0;
    if (nseg <= 1) return;
    const int tid = threadIdx.x;
    const int bx = int(brick % A.g.nb[0]), by = int(brick / A.g.nb[0] % A.g.nb[1]),
              bz = int(brick / (int64_t(A.g.nb[0]) * A.g.nb[1]));
    int sx, sy, sz, lx, ly, lz;
    voxelOf(tid, sx, sy, sz, lx, ly, lz);
    const int vx = bx * kBrick + sx + lx, vy = by * kBrick + sy + ly, vz = bz * kBrick + sz + lz;
    float acc[C];
#pragma unroll
    for (int c = 0; c < C; ++c)
        acc[c] = 0.0f;
    for (int64_t s = 0; s < nseg; ++s)
    {
        const float* in = A.work + size_t(A.workOff[brick] + s) * C * kBrickVox;
#pragma unroll
        for (int c = 0; c < C; ++c)
            acc[c] += in[c * kBrickBlock + tid];
    }
    if (vx < A.g.n[0] && vy < A.g.n[1] && vz < A.g.n[2])
#pragma unroll
        for (int c = 0; c < C; ++c)
            A.vol[((size_t(c) * A.g.n[2] + vz) * A.g.n[1] + vy) * A.g.n[0] + vx] = acc[c];
}

template<int C>
void launchBricks(unsigned nblocks, const BrickArgs& A, const KernelFn& fn, float norm, hipStream_t s)
{
    volumeBrickKernel<C><<<nblocks, kBrickBlock, 0, s>>>(A, fn, norm);
    SPHX_LAUNCH_CHECK();
    volumeSumKernel<C><<<unsigned(A.nbricks), kBrickBlock, 0, s>>>(A);
    SPHX_LAUNCH_CHECK();
}

// ---------------------------------------------------------------------------------------------------- spectrum shells

constexpr int kShellBlock     = 256;
constexpr int kShellMaxBlocks = 1024;
constexpr int kShellMaxBins   = 4096; // 64 KiB of fp64 (P, count) bins per block

//! shell b = floor(|k| + 0.5) of an integer wave vector of squared length k2: the b with (2b - 1)^2 <= 4 k2 < (2b + 1)^2
__device__ __forceinline__ int shellOf(int64_t k2)
{
    int64_t b = int64_t(sqrt(double(k2)) + 0.5);
    while ((2 * b + 1) * (2 * b + 1) <= 4 * k2)
        ++b;
    while (b > 0 && (2 * b - 1) * (2 * b - 1) > 4 * k2)
        --b;
    return int(b);
}

/*! @brief the half spectrum F = rfftn(u) (C x N x N x (N/2 + 1) complex64) summed into shells: with u^ = F / N^3,
 *         P[b] += wgt sum_c |u^_c(k)|^2 and count[b] += wgt, wgt = 1 in the planes kx = 0 and (even N) kx = N/2 that
 *         are their own mirror image, 2 elsewhere. fp64 throughout; LDS bins per block, one partial row per block */
__global__ void __launch_bounds__(kShellBlock)
spectrumShellsKernel(int C, int N, const float2* __restrict__ spec, int nbins, double scale,
                     double* __restrict__ partial)
{
    extern __shared__ double sBins[]; // P[nbins], count[nbins]
    for (int i = threadIdx.x; i < 2 * nbins; i += kShellBlock)
        sBins[i] = 0.0;
    __syncthreads();
    const int nh        = N / 2 + 1;
    const int64_t modes = int64_t(N) * N * nh;
    const int half      = (N + 1) / 2; // indices below: k = i, from there on: k = i - N
    for (int64_t m = int64_t(blockIdx.x) * kShellBlock + threadIdx.x; m < modes; m += int64_t(gridDim.x) * kShellBlock)
    {
        const int ix = int(m % nh), iy = int(m / nh % N), iz = int(m / (int64_t(nh) * N));
        const int64_t kx = ix, ky = iy < half ? iy : iy - N, kz = iz < half ? iz : iz - N;
        const int b      = shellOf(kx * kx + ky * ky + kz * kz);
        double p         = 0.0;
        for (int c = 0; c < C; ++c)
        {
            const float2 f = spec[c * modes + m];
            p += double(f.x) * double(f.x) + double(f.y) * double(f.y);
        }
        const double wgt = (ix == 0 || 2 * ix == N) ? 1.0 : 2.0;
        if (b < nbins)
        {
            atomicAdd(&sBins[b], wgt * p * scale);
            atomicAdd(&sBins[nbins + b], wgt);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 2 * nbins; i += kShellBlock)
        partial[size_t(blockIdx.x) * 2 * nbins + i] = sBins[i];
}

//! the partial rows added in block order
__global__ void spectrumSumKernel(int nblocks, int nbins, const double* __restrict__ partial, double* __restrict__ out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 2 * nbins) return;
    double s = 0.0;
    for (int b = 0; b < nblocks; ++b)
        s += partial[size_t(b) * 2 * nbins + i];
    out[i] = s;
}

} // namespace

void volumeRecords(int64_t first, int64_t last, int64_t n, const double* x, const double* y, const double* z,
                   const float* h, const float* w, int C, const VolumeView& V, VolumeRec* rec, int64_t* counts,
                   hipStream_t s)
{
    if (C != 1 && C != 2 && C != 4) throw std::invalid_argument("volumeRecords: one, two or four channels");
    if (last - first > (int64_t(1) << kPartBits)) throw std::invalid_argument("volumeRecords: more than 2^30 particles");
    const VolumeGeom g = geomOf(V);
    if (bricksOf(g) >= (int64_t(1) << kBrickBits)) throw std::invalid_argument("volumeRecords: 2^29 bricks or more");
    volumeRecordsKernel<<<gridFor(last - first + 1, 256), 256, 0, s>>>(first, last, n, x, y, z, h, w, C, V, g, rec,
                                                                       counts);
    SPHX_LAUNCH_CHECK();
}

void volumeFill(int64_t np, const VolumeView& V, const VolumeRec* rec, const int64_t* offsets, uint64_t* keys,
                hipStream_t s)
{
    if (np <= 0) return;
    volumeFillKernel<<<gridFor(np, 256), 256, 0, s>>>(np, geomOf(V), rec, offsets, keys);
    SPHX_LAUNCH_CHECK();
}

void volumeRanges(int64_t total, const uint64_t* keys, int64_t nbricks, int64_t segment, int64_t* start,
                  int64_t* nseg, int64_t* wseg, hipStream_t s)
{
    if (segment < 1) throw std::invalid_argument("volumeRanges: segment length");
    if (nbricks < 1 || nbricks >= (int64_t(1) << kBrickBits)) throw std::invalid_argument("volumeRanges: brick count");
    volumeRangesKernel<<<gridFor(nbricks + 1, 256), 256, 0, s>>>(total, keys, nbricks, segment, start, nseg, wseg);
    SPHX_LAUNCH_CHECK();
}

void volumeBricks(int C, int64_t np, int64_t total, const uint64_t* keys, const VolumeRec* rec, const VolumeView& V,
                  int64_t nbricks, int64_t segment, int64_t nblocks, const int64_t* start, const int64_t* segOff,
                  const int64_t* workOff, int64_t nwork, float* work, float* vol, hipStream_t s)
{
    const VolumeGeom g = geomOf(V);
    if (nbricks != bricksOf(g) || nbricks >= (int64_t(1) << kBrickBits))
        throw std::invalid_argument("volumeBricks: brick count");
    if (segment < 1 || nblocks < total / segment + nbricks || nblocks > 0x7fffffff)
        throw std::invalid_argument("volumeBricks: block count");
    // a brick of k > 1 segments holds more than (k - 1) S entries: at most 2 total / S partial bricks in all
    if (nwork < 2 * (total / segment)) throw std::invalid_argument("volumeBricks: workspace");
    const BrickArgs A{np, total, keys, rec, g, nbricks, segment, start, segOff, workOff, work, vol};
    const KernelFn fn{nullptr, nullptr, float(V.sinc), 0};
    // wqScale on the host is 1 (the table form): the device scale (2 pi)^n is applied here
    const float norm = float(V.K / std::exp2(V.sinc * 2.651496129472318798043279295));
    if (C == 1) launchBricks<1>(unsigned(nblocks), A, fn, norm, s);
    else if (C == 2) launchBricks<2>(unsigned(nblocks), A, fn, norm, s);
    else if (C == 4) launchBricks<4>(unsigned(nblocks), A, fn, norm, s);
    else throw std::invalid_argument("volumeBricks: one, two or four channels");
}

int spectrumShellBlocks(int N)
{
    const int64_t modes = int64_t(N) * N * (N / 2 + 1);
    return int(sphx::smin(int64_t(kShellMaxBlocks), (modes + kShellBlock - 1) / kShellBlock));
}

void spectrumShells(int C, int N, const float* spec, int nbins, double* partial, double* out, hipStream_t s)
{
    if (C < 1 || N < 1 || nbins < 1 || nbins > kShellMaxBins)
        throw std::invalid_argument("spectrumShells: channels, grid size or more than 4096 shells");
    const int nblocks  = spectrumShellBlocks(N);
    const double scale = 1.0 / (double(N) * N * N * double(N) * N * N);
    spectrumShellsKernel<<<nblocks, kShellBlock, size_t(2) * nbins * sizeof(double), s>>>(
        C, N, reinterpret_cast<const float2*>(spec), nbins, scale, partial);
    SPHX_LAUNCH_CHECK();
    spectrumSumKernel<<<gridFor(2 * nbins, 256), 256, 0, s>>>(nblocks, nbins, partial, out);
    SPHX_LAUNCH_CHECK();
}

SPHX_DCHECK_READER(dcheckVolume)

} // namespace sphx::hip
