/*! SPH slices and column projections as images on gfx950: particles are binned to 32x32-pixel tiles, every tile sums
 *  its own sorted list (definitions: ops/image.py; host form: cpu/image_cpu.cpp).
 *
 *  1. imageRecordsKernel, one thread per particle: the pixel-space centre, 1/h_eff and (slices) the depth offset over h
 *     are formed in fp64 from the coordinates and rounded once to fp32 into a 32-B record next to the weights and the
 *     footprint's half extents in pixels. The thread counts the tiles that the footprint's bounding box overlaps, for
 *     every periodic image shift in {-1, 0, 1}^2 that meets the window. Particles outside the depth range count nothing.
 *  2. An exclusive scan of the counts sizes the entry list (the one host synchronisation); imageFillKernel writes the
 *     keys tile << 34 | particle << 4 | shift code (particles < 2^30, tiles < 2^30, 9 shift codes) from the same fp32
 *     footprint function the count used, and the project's sample sort orders them by (tile, particle, shift). The
 *     order of every tile's sum is thereby fixed: the image is bit-reproducible from run to run.
 *  3. imageRangesKernel finds every tile's range in the sorted keys and cuts it into segments of at most S entries;
 *     a scan of the segment counts numbers the (tile, segment) blocks.
 *  4. imageTileKernel<Profile, C>, 256 threads = 4 waves per (tile, segment): a thread owns a 2x2 pixel quad (4 C
 *     accumulators), a wave a 32x8 strip. The block walks its entries in batches of 256: each thread gathers one
 *     entry's record (the key two batches and the record one batch ahead of the batch being consumed), applies the
 *     entry's periodic shift and stores the entry SoA into LDS. Each wave tests the 256 staged footprints against its
 *     strip 64 at a time, ballot-compacts the survivors into its own LDS index list (as the neighbor search compacts
 *     its frontier) and its lanes loop over those only, reading each survivor by LDS broadcast. Per pixel and entry:
 *     q^2 = (du^2 + dv^2 [+ dz^2]) / h^2 and, inside the support, acc_c += w_c profile(q^2). The profile is a policy:
 *     SliceProfile evaluates the project's sinc^n kernel function (h^-3 folded into the staged weights), ProjProfile
 *     interpolates the F_n table in u = q^2/4, copied into LDS once per block (h^-2 folded into the weights).
 *  5. A tile of one segment stores its pixels to the image; the segments of a longer list store partial tiles to a
 *     workspace and imageSumKernel adds them in segment order (deterministic as well).
 *
 *  No matrix instructions: the distances are 2-D/3-D (an MFMA form of |p - c|^2 would have K = 3 or 4 and spend the
 *  tile on padding), and the cost is the culling and the transcendental / table read per pixel, not the dot product.
 */
#include "common.h"
#include "hip_api.h"

namespace sphx::hip
{

namespace
{

constexpr int kTile      = 32;
constexpr int kTileBlock = 256;
constexpr int kShiftBits = 4;
constexpr int kPartBits  = 30;
constexpr int kTileShift = kShiftBits + kPartBits;

//! the window in pixels, as the device sees it
struct ImageGeom
{
    int nu, nv, ntu, ntv;
    int perU, perV;
    float LuPix, LvPix; // periodic image shifts in pixels
    float au, av;       // pixel sizes
};

ImageGeom geomOf(const ImageView& V)
{
    ImageGeom g;
    g.nu    = V.nu;
    g.nv    = V.nv;
    g.ntu   = (V.nu + kTile - 1) / kTile;
    g.ntv   = (V.nv + kTile - 1) / kTile;
    g.perU  = V.perU;
    g.perV  = V.perV;
    g.LuPix = float(V.Lu / V.pu);
    g.LvPix = float(V.Lv / V.pv);
    g.au    = float(V.pu);
    g.av    = float(V.pv);
    return g;
}

/*! @brief pixels of one axis whose centres (k + 0.5) lie within r of c, widened by 2^-10 pixel (the pixel test itself
 *         is q^2 < 4 in fp32; the box only has to contain it), clipped to [0, n). Written with explicit single
 *         roundings: the count, the fill and the tile kernel must see the same box. */
__device__ __forceinline__ bool pixelRange(float c, float r, int n, int& k0, int& k1)
{
    const float pad = 0.5f + 0.0009765625f;
    float lo        = __fsub_rn(__fsub_rn(c, r), pad);
    float hi        = __fadd_rn(__fadd_rn(c, r), pad - 1.0f);
    lo              = fmaxf(ceilf(lo), 0.0f);
    hi              = fminf(floorf(hi), float(n - 1));
    k0              = int(lo);
    k1              = int(hi);
    return r >= 0.0f && lo <= hi;
}

//! @brief centre of the periodic image (su, sv) of a record, in pixels
__device__ __forceinline__ void shifted(const ImageRec& r, int su, int sv, const ImageGeom& g, float& cu, float& cv)
{
    cu = __fmaf_rn(float(su), g.LuPix, r.cu);
    cv = __fmaf_rn(float(sv), g.LvPix, r.cv);
}

//! @brief calls f(tile, shift code) for every (periodic image, tile) the record's footprint box overlaps
template<class F>
__device__ __forceinline__ void forEachTile(const ImageRec& r, const ImageGeom& g, F&& f)
{
    if (!(r.ru >= 0.0f)) return;
    const int mu = g.perU ? 1 : 0, mv = g.perV ? 1 : 0;
    for (int sv = -mv; sv <= mv; ++sv)
        for (int su = -mu; su <= mu; ++su)
        {
            float cu, cv;
            shifted(r, su, sv, g, cu, cv);
            int i0, i1, j0, j1;
            if (!pixelRange(cu, r.ru, g.nu, i0, i1) || !pixelRange(cv, r.rv, g.nv, j0, j1)) continue;
            const int code = (sv + 1) * 3 + (su + 1);
            for (int tv = j0 / kTile; tv <= j1 / kTile; ++tv)
                for (int tu = i0 / kTile; tu <= i1 / kTile; ++tu)
                    f(tv * g.ntu + tu, code);
        }
}

__global__ void __launch_bounds__(256)
imageRecordsKernel(int64_t first, int64_t last, int64_t n, const double* __restrict__ x, const double* __restrict__ y,
                   const double* __restrict__ z, const float* __restrict__ h, const float* __restrict__ w, int C,
                   ImageView V, ImageGeom g, ImageRec* __restrict__ rec, int64_t* __restrict__ counts)
{
    const int64_t k = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    const int64_t i = first + k;
    if (i > last) return;
    if (i == last)
    {
        counts[k] = 0; // the scan's last element: its result is the total
        return;
    }
    const double p[3] = {x[i], y[i], z[i]};
    const double hj   = sphx::smax(double(h[i]), V.hMin);
    double dz, R;
    const bool in = imageDepth(V, p[V.ia], hj, dz, R);
    ImageRec r;
    r.cu = float((p[V.iu] - V.u0) / V.pu);
    r.cv = float((p[V.iv] - V.v0) / V.pv);
    r.ih = float(1.0 / hj);
    r.zq = float(dz / hj);
    r.w0 = w[i];
    r.w1 = C == 2 ? w[n + i] : 0.0f;
    // half extents in pixels, rounded up (2^-20 covers the fp32 rounding of the extents and of q^2); < 0: no entries
    r.ru = in ? float(R / V.pu * (1.0 + 9.5367431640625e-7)) : -1.0f;
    r.rv = in ? float(R / V.pv * (1.0 + 9.5367431640625e-7)) : -1.0f;
    rec[k]  = r;
    int64_t c = 0;
    forEachTile(r, g, [&](int, int) { ++c; });
    counts[k] = c;
}

__global__ void __launch_bounds__(256)
imageFillKernel(int64_t np, ImageGeom g, const ImageRec* __restrict__ rec, const int64_t* __restrict__ offsets,
                uint64_t* __restrict__ keys)
{
    const int64_t k = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (k >= np) return;
    int64_t pos       = offsets[k];
    const int64_t end = offsets[k + 1];
    forEachTile(rec[k], g,
                [&](int tile, int code)
                {
                    // (never beyond the particle's own slots, whatever the count was)
                    if (pos < end) keys[pos++] = uint64_t(tile) << kTileShift | uint64_t(k) << kShiftBits | uint64_t(code);
                });
    for (; pos < end; ++pos)
        keys[pos] = ~uint64_t(0); // past every tile: in no tile's range
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

//! start[t] = first entry of tile t (t = ntiles: the end of the last tile), nseg[t] = blocks of tile t (at least one:
//! a tile without entries still stores its zeros)
__global__ void imageRangesKernel(int64_t total, const uint64_t* __restrict__ keys, int ntiles, int64_t segment,
                                  int64_t* __restrict__ start, int64_t* __restrict__ nseg)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t > ntiles) return;
    const int64_t a = lowerBound(keys, total, uint64_t(t) << kTileShift);
    start[t]        = a;
    if (t == ntiles)
    {
        nseg[t] = 0;
        return;
    }
    const int64_t b = lowerBound(keys, total, uint64_t(t + 1) << kTileShift);
    nseg[t]         = sphx::smax(int64_t(1), (b - a + segment - 1) / segment);
}

struct TileArgs
{
    int64_t np, total;
    const uint64_t* keys;
    const ImageRec* rec;
    ImageGeom g;
    int ntiles;
    int64_t segment;
    const int64_t* start;
    const int64_t* segOff; // ntiles + 1: first block of every tile
    const float* table;
    float* work; // per block: C x 1024 partial sums, thread-major
    float* img;
};

//! slice: the project's sinc^n kernel at q; the staged weights carry K h^-3 / wqScale
struct SliceProfile
{
    static constexpr int kLds = 1;
    KernelFn fn;
    float norm; // K / wqScale
    __device__ __forceinline__ void load(float*, const float*) const {}
    __device__ __forceinline__ float weight(float ih) const { return norm * ih * ih * ih; }
    __device__ __forceinline__ float zq2(float zq) const { return zq * zq; }
    __device__ __forceinline__ float operator()(const float*, float q2) const { return fn.wq(0.25f * sqrtF(q2)); }
};

//! projection: F_n by linear interpolation in u = q^2/4 from the LDS copy of the table; weights carry h^-2
struct ProjProfile
{
    static constexpr int kLds = kImageTableLen + 1;
    __device__ __forceinline__ void load(float* lds, const float* table) const
    {
        for (int k = threadIdx.x; k < kLds; k += kTileBlock)
            lds[k] = k < kImageTableLen ? table[k] : 0.0f;
    }
    __device__ __forceinline__ float weight(float ih) const { return ih * ih; }
    __device__ __forceinline__ float zq2(float) const { return 0.0f; }
    __device__ __forceinline__ float operator()(const float* lds, float q2) const
    {
        const float t = q2 * (0.25f * float(kImageTableLen - 1));
        const int i   = sphx::smin(int(t), kImageTableLen - 2);
        const float a = lds[i], b = lds[i + 1];
        return a + (t - float(i)) * (b - a);
    }
};

//! pixel p (0..3) of thread t in its tile: a wave owns a 32x8 strip, a lane a 2x2 quad
__device__ __forceinline__ void quadOrigin(int t, int& px, int& py)
{
    const int lane = t & 63, wave = t >> 6;
    px = 2 * (lane & 15);
    py = wave * 8 + 2 * (lane >> 4);
}

template<class Profile, int C>
__global__ void __launch_bounds__(kTileBlock) imageTileKernel(TileArgs A, Profile prof)
{
    __shared__ float sTab[Profile::kLds];
    __shared__ float sCu[kTileBlock], sCv[kTileBlock], sAu[kTileBlock], sAv[kTileBlock], sZ2[kTileBlock],
        sRu[kTileBlock], sRv[kTileBlock], sW[C][kTileBlock];
    __shared__ uint16_t sList[kTileBlock / kWave][kTileBlock];

    const int64_t b = blockIdx.x;
    if (b >= A.segOff[A.ntiles]) return; // (the grid is the host's upper bound of the block count)
    // tile of this block: the last t with segOff[t] <= b
    int tile;
    {
        int lo = 0, hi = A.ntiles;
        while (hi - lo > 1)
        {
            const int mid = (lo + hi) >> 1;
            if (A.segOff[mid] <= b) lo = mid;
            else hi = mid;
        }
        tile = lo;
    }
    SPHX_DCHECK(tile >= 0 && tile < A.ntiles && A.segOff[tile] <= b && b < A.segOff[tile + 1], 6);
    const int64_t seg0  = A.segOff[tile];
    const int64_t nseg  = A.segOff[tile + 1] - seg0;
    const int64_t tEnd  = A.start[tile + 1];
    const int64_t e0    = sphx::smin(A.start[tile] + (b - seg0) * A.segment, tEnd);
    const int64_t e1    = sphx::smin(e0 + A.segment, tEnd);
    const int nBatch    = int((e1 - e0 + kTileBlock - 1) / kTileBlock);
    const int tid       = threadIdx.x;
    const int wave      = tid >> 6;
    const int tu = tile % A.g.ntu, tv = tile / A.g.ntu;
    int qx, qy;
    quadOrigin(tid, qx, qy);
    // pixel centres of the quad and the strip's extent of centres
    const float fx0 = float(tu * kTile + qx) + 0.5f, fx1 = fx0 + 1.0f;
    const float fy0 = float(tv * kTile + qy) + 0.5f, fy1 = fy0 + 1.0f;
    const float sx0 = float(tu * kTile) + 0.5f, sx1 = sx0 + float(kTile - 1);
    const float sy0 = float(tv * kTile + wave * 8) + 0.5f, sy1 = sy0 + 7.0f;

    prof.load(sTab, A.table);

    float acc[4][C];
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int c = 0; c < C; ++c)
            acc[p][c] = 0.0f;

    const float4* rec4 = reinterpret_cast<const float4*>(A.rec);
    auto loadKey       = [&](int batch) -> uint64_t
    {
        const int64_t e = e0 + int64_t(batch) * kTileBlock + tid;
        return e < e1 ? A.keys[e] : ~uint64_t(0);
    };
    // record index of a key (the fill's padding keys and slots past the range: record 0, marked not staged)
    auto recIndex = [&](uint64_t key, bool& valid) -> int64_t
    {
        int64_t j = int64_t((key >> kShiftBits) & ((uint64_t(1) << kPartBits) - 1));
        valid     = key != ~uint64_t(0);
        SPHX_DCHECK(!valid || j < A.np, 7);
        return (valid && j < A.np) ? j : 0;
    };

    uint64_t keyCur = loadKey(0), keyNext = loadKey(1);
    bool validCur;
    int64_t j  = recIndex(keyCur, validCur);
    float4 r0 = rec4[2 * j], r1 = rec4[2 * j + 1];

    for (int batch = 0; batch < nBatch; ++batch)
    {
        // the loads of the batches ahead: key of batch + 2, record of batch + 1
        const uint64_t keyNext2 = loadKey(batch + 2);
        bool validNext;
        const int64_t jn = recIndex(keyNext, validNext);
        const float4 n0 = rec4[2 * jn], n1 = rec4[2 * jn + 1];

        __syncthreads(); // the previous batch is consumed (first batch: the table is in LDS)
        {
            const int code = int(keyCur & ((1u << kShiftBits) - 1));
            const int sv = code / 3 - 1, su = code % 3 - 1;
            ImageRec r{r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w};
            float cu, cv;
            shifted(r, validCur ? su : 0, validCur ? sv : 0, A.g, cu, cv);
            const float wgt = prof.weight(r.ih);
            sCu[tid]    = cu;
            sCv[tid]    = cv;
            sAu[tid]    = A.g.au * r.ih;
            sAv[tid]    = A.g.av * r.ih;
            sZ2[tid]    = prof.zq2(r.zq);
            sRu[tid]    = validCur ? r.ru : -1.0f;
            sRv[tid]    = r.rv;
            sW[0][tid]  = r.w0 * wgt;
            if constexpr (C == 2) sW[1][tid] = r.w1 * wgt;
        }
        __syncthreads();

        // survivors of this wave's strip, in entry order
        int count = 0;
#pragma unroll
        for (int r = 0; r < kTileBlock / kWave; ++r)
        {
            const int s    = r * kWave + laneId();
            const float ru = sRu[s], rv = sRv[s], cu = sCu[s], cv = sCv[s];
            const bool hit = ru >= 0.0f && cu - ru <= sx1 + 0.001f && cu + ru >= sx0 - 0.001f &&
                             cv - rv <= sy1 + 0.001f && cv + rv >= sy0 - 0.001f;
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
            const float cu = sCu[s], cv = sCv[s], au = sAu[s], av = sAv[s], z2 = sZ2[s];
            float w[C];
            w[0] = sW[0][s];
            if constexpr (C == 2) w[1] = sW[1][s];
            const float a0 = (fx0 - cu) * au, a1 = (fx1 - cu) * au;
            const float b0 = (fy0 - cv) * av, b1 = (fy1 - cv) * av;
            const float a02 = a0 * a0 + z2, a12 = a1 * a1 + z2, b02 = b0 * b0, b12 = b1 * b1;
            const float q2[4] = {a02 + b02, a12 + b02, a02 + b12, a12 + b12};
#pragma unroll
            for (int p = 0; p < 4; ++p)
                if (q2[p] < 4.0f)
                {
                    const float f = prof(sTab, q2[p]);
#pragma unroll
                    for (int c = 0; c < C; ++c)
                        acc[p][c] += w[c] * f;
                }
        }

        keyCur   = keyNext;
        keyNext  = keyNext2;
        validCur = validNext;
        r0       = n0;
        r1       = n1;
    }

    // pixel p of the quad: (qx + (p & 1), qy + (p >> 1))
    if (nseg == 1)
    {
#pragma unroll
        for (int p = 0; p < 4; ++p)
        {
            const int px = tu * kTile + qx + (p & 1), py = tv * kTile + qy + (p >> 1);
            if (px < A.g.nu && py < A.g.nv)
#pragma unroll
                for (int c = 0; c < C; ++c)
                    A.img[(size_t(c) * A.g.nv + py) * A.g.nu + px] = acc[p][c];
        }
    }
    else
    {
        float* out = A.work + size_t(b) * C * (kTile * kTile);
#pragma unroll
        for (int c = 0; c < C; ++c)
#pragma unroll
            for (int p = 0; p < 4; ++p)
                out[(c * 4 + p) * kTileBlock + tid] = acc[p][c];
    }
}

//! tiles of several segments: their partial tiles added in segment order
template<int C>
__global__ void __launch_bounds__(kTileBlock) imageSumKernel(TileArgs A)
{
    const int tile     = blockIdx.x;
    const int64_t seg0 = A.segOff[tile];
    const int64_t nseg = A.segOff[tile + 1] - seg0;
    if (nseg <= 1) return;
    const int tid = threadIdx.x;
    const int tu = tile % A.g.ntu, tv = tile / A.g.ntu;
    int qx, qy;
    quadOrigin(tid, qx, qy);
    float acc[C * 4];
#pragma unroll
    for (int k = 0; k < C * 4; ++k)
        acc[k] = 0.0f;
    for (int64_t s = 0; s < nseg; ++s)
    {
        const float* in = A.work + size_t(seg0 + s) * C * (kTile * kTile);
#pragma unroll
        for (int k = 0; k < C * 4; ++k)
            acc[k] += in[k * kTileBlock + tid];
    }
#pragma unroll
    for (int c = 0; c < C; ++c)
#pragma unroll
        for (int p = 0; p < 4; ++p)
        {
            const int px = tu * kTile + qx + (p & 1), py = tv * kTile + qy + (p >> 1);
            if (px < A.g.nu && py < A.g.nv) A.img[(size_t(c) * A.g.nv + py) * A.g.nu + px] = acc[c * 4 + p];
        }
}

template<class Profile>
void launchTiles(int C, unsigned nblocks, const TileArgs& A, const Profile& prof, hipStream_t s)
{
    if (C == 1) imageTileKernel<Profile, 1><<<nblocks, kTileBlock, 0, s>>>(A, prof);
    else imageTileKernel<Profile, 2><<<nblocks, kTileBlock, 0, s>>>(A, prof);
    SPHX_LAUNCH_CHECK();
    if (C == 1) imageSumKernel<1><<<unsigned(A.ntiles), kTileBlock, 0, s>>>(A);
    else imageSumKernel<2><<<unsigned(A.ntiles), kTileBlock, 0, s>>>(A);
    SPHX_LAUNCH_CHECK();
}

} // namespace

void imageRecords(int64_t first, int64_t last, int64_t n, const double* x, const double* y, const double* z,
                  const float* h, const float* w, int C, const ImageView& V, ImageRec* rec, int64_t* counts,
                  hipStream_t s)
{
    if (C != 1 && C != 2) throw std::invalid_argument("imageRecords: one or two channels");
    if (last - first > (int64_t(1) << kPartBits)) throw std::invalid_argument("imageRecords: more than 2^30 particles");
    imageRecordsKernel<<<gridFor(last - first + 1, 256), 256, 0, s>>>(first, last, n, x, y, z, h, w, C, V, geomOf(V),
                                                                      rec, counts);
    SPHX_LAUNCH_CHECK();
}

void imageFill(int64_t np, const ImageView& V, const ImageRec* rec, const int64_t* offsets, uint64_t* keys,
               hipStream_t s)
{
    if (np <= 0) return;
    imageFillKernel<<<gridFor(np, 256), 256, 0, s>>>(np, geomOf(V), rec, offsets, keys);
    SPHX_LAUNCH_CHECK();
}

void imageRanges(int64_t total, const uint64_t* keys, int ntiles, int64_t segment, int64_t* start, int64_t* nseg,
                 hipStream_t s)
{
    if (segment < 1) throw std::invalid_argument("imageRanges: segment length");
    imageRangesKernel<<<gridFor(ntiles + 1, 256), 256, 0, s>>>(total, keys, ntiles, segment, start, nseg);
    SPHX_LAUNCH_CHECK();
}

void imageTiles(int C, int64_t np, int64_t total, const uint64_t* keys, const ImageRec* rec, const ImageView& V,
                int ntiles, int64_t segment, int64_t nblocks, const int64_t* start, const int64_t* segOff,
                const float* table, int tableLen, float* work, float* img, hipStream_t s)
{
    const ImageGeom g = geomOf(V);
    if (C != 1 && C != 2) throw std::invalid_argument("imageTiles: one or two channels");
    if (ntiles != g.ntu * g.ntv) throw std::invalid_argument("imageTiles: tile count");
    if (nblocks < total / segment + ntiles || nblocks > 0x7fffffff)
        throw std::invalid_argument("imageTiles: block count");
    if (V.proj && tableLen != kImageTableLen) throw std::invalid_argument("imageTiles: F_n table length");
    const TileArgs A{np, total, keys, rec, g, ntiles, segment, start, segOff, table, work, img};
    if (V.proj) launchTiles(C, unsigned(nblocks), A, ProjProfile{}, s);
    else
    {
        SliceProfile p;
        p.fn   = KernelFn{nullptr, nullptr, float(V.n), 0};
        // wqScale on the host is 1 (the table form): the device scale (2 pi)^n is applied here
        p.norm = float(V.K / std::exp2(V.n * 2.651496129472318798043279295));
        launchTiles(C, unsigned(nblocks), A, p, s);
    }
}

SPHX_DCHECK_READER(dcheckImage)

} // namespace sphx::hip
