/*! SPH slices, column projections and opacity renderings as images on gfx950: particles are binned to 32x32-pixel
 *  tiles, every tile sums (composites) its own sorted list (definitions: ops/image.py; host form: cpu/image_cpu.cpp).
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
 *  6. Opacity renderings composite a pixel's entries front to back, so the list order is part of the result.
 *     imageDepthKeysKernel writes the order-preserving uint64 image of every particle's fp64 depth, the stable sample
 *     sort turns the keys into a permutation (ties by particle index) and imageRecordsKernel forms record k from
 *     particle perm[k]: the entry keys of step 2 then sort into depth order inside every tile with no further work.
 *     imageRenderKernel walks the list as step 4 does (same staging, walkEntries) and carries (I, T) per pixel:
 *     tau = kappa m h^-2 F_n, a = exp(-tau), I += T (1 - a) s, T *= a. A lane's four pixels are four independent
 *     chains; per entry a chain is one multiply-add (I) and one multiply (T), everything else (table read,
 *     v_exp_f32, 1 - a) is computed off the chains. Segments start from (0, 1) and store (I_s, T_s) partial tiles;
 *     imageComposeKernel folds them in list order, I += T I_s, T *= T_s.
 *     Open lead: no early-out on opaque pixels. A segment does not know the transmittance in front of it, but a block
 *     could stop staging batches once all of its own 1024 T are 0 (one __syncthreads_and per batch).
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

//! rendering: the depth key of every particle of [first, first + np), a = its view-axis coordinates
__global__ void __launch_bounds__(256)
imageDepthKeysKernel(int64_t first, int64_t np, const double* __restrict__ a, ImageView V, uint64_t* __restrict__ keys)
{
    const int64_t k = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (k < np) keys[k] = imageDepthKey(V, a[first + k]);
}

//! record k of particle first + perm[k] (a rendering's depth order) or, without a permutation, first + k
__global__ void __launch_bounds__(256)
imageRecordsKernel(int64_t first, int64_t last, int64_t n, const double* __restrict__ x, const double* __restrict__ y,
                   const double* __restrict__ z, const float* __restrict__ h, const float* __restrict__ w, int C,
                   const int32_t* __restrict__ perm, ImageView V, ImageGeom g, ImageRec* __restrict__ rec,
                   int64_t* __restrict__ counts)
{
    const int64_t k = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (first + k > last) return;
    if (first + k == last)
    {
        counts[k] = 0; // the scan's last element: its result is the total
        return;
    }
    int64_t i = first + k;
    if (perm)
    {
        const int64_t pk = perm[k];
        SPHX_DCHECK(pk >= 0 && pk < last - first, 13);
        if (pk >= 0 && pk < last - first) i = first + pk;
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

//! LDS of a tile block's walk: one batch of 256 entries, SoA, with NW staged weights, and every wave's survivors.
//! Depth: the entries carry a depth term z2 = (dz / h)^2 (slices); without it nothing is staged or added for it
template<int NW, bool Depth>
struct TileStage
{
    float cu[kTileBlock], cv[kTileBlock], au[kTileBlock], av[kTileBlock], z2[Depth ? kTileBlock : 1], ru[kTileBlock],
        rv[kTileBlock], w[NW][kTileBlock];
    uint16_t list[kTileBlock / kWave][kTileBlock];
};

//! the (tile, segment) of a block: its tile, the tile's segment count, its entries [e0, e1) and the thread's quad
struct TileBlock
{
    int tu, tv, qx, qy;
    int64_t nseg, e0, e1;
};

//! @return false for the blocks past the scanned block count (the grid is the host's upper bound)
__device__ __forceinline__ bool tileBlockOf(const TileArgs& A, TileBlock& B)
{
    const int64_t b = blockIdx.x;
    if (b >= A.segOff[A.ntiles]) return false;
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
    const int64_t seg0 = A.segOff[tile];
    const int64_t tEnd = A.start[tile + 1];
    B.nseg             = A.segOff[tile + 1] - seg0;
    B.e0               = sphx::smin(A.start[tile] + (b - seg0) * A.segment, tEnd);
    B.e1               = sphx::smin(B.e0 + A.segment, tEnd);
    B.tu               = tile % A.g.ntu;
    B.tv               = tile / A.g.ntu;
    quadOrigin(threadIdx.x, B.qx, B.qy);
    return true;
}

/*! @brief walks the block's entries in list order, shared by the summing and the compositing tile kernel: stages them
 *         in batches of 256 (fold(record, w) fills an entry's staged weights and returns its depth term, used only
 *         with Depth), culls every batch against the wave's strip and calls body(q2, w) for every survivor, with q^2
 *         at the quad's four pixels. The ballot compaction keeps the survivors in entry order (a lane's slot is the
 *         count of the hits before it): the sums are thereby reproducible, and the compositing kernel's result
 *         depends on it. */
template<int NW, bool Depth, class Fold, class Body>
__device__ __forceinline__ void walkEntries(const TileArgs& A, const TileBlock& B, TileStage<NW, Depth>& st,
                                            Fold&& fold, Body&& body)
{
    const int64_t e0 = B.e0, e1 = B.e1;
    const int nBatch = int((e1 - e0 + kTileBlock - 1) / kTileBlock);
    const int tid    = threadIdx.x;
    const int wave   = tid >> 6;
    // pixel centres of the quad and the strip's extent of centres
    const float fx0 = float(B.tu * kTile + B.qx) + 0.5f, fx1 = fx0 + 1.0f;
    const float fy0 = float(B.tv * kTile + B.qy) + 0.5f, fy1 = fy0 + 1.0f;
    const float sx0 = float(B.tu * kTile) + 0.5f, sx1 = sx0 + float(kTile - 1);
    const float sy0 = float(B.tv * kTile + wave * 8) + 0.5f, sy1 = sy0 + 7.0f;

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
            float w[NW];
            const float z2 = fold(r, w);
            if constexpr (Depth) st.z2[tid] = z2;
            st.cu[tid] = cu;
            st.cv[tid] = cv;
            st.au[tid] = A.g.au * r.ih;
            st.av[tid] = A.g.av * r.ih;
            st.ru[tid] = validCur ? r.ru : -1.0f;
            st.rv[tid] = r.rv;
#pragma unroll
            for (int c = 0; c < NW; ++c)
                st.w[c][tid] = w[c];
        }
        __syncthreads();

        // survivors of this wave's strip, in entry order
        int count = 0;
#pragma unroll
        for (int r = 0; r < kTileBlock / kWave; ++r)
        {
            const int s    = r * kWave + laneId();
            const float ru = st.ru[s], rv = st.rv[s], cu = st.cu[s], cv = st.cv[s];
            const bool hit = ru >= 0.0f && cu - ru <= sx1 + 0.001f && cu + ru >= sx0 - 0.001f &&
                             cv - rv <= sy1 + 0.001f && cv + rv >= sy0 - 0.001f;
            const uint64_t m = ballot(hit);
            if (hit) st.list[wave][count + popcount64(m & lanemaskLt())] = uint16_t(s);
            count += popcount64(m);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

        for (int k = 0; k < count; ++k)
        {
            const int s    = st.list[wave][k];
            const float cu = st.cu[s], cv = st.cv[s], au = st.au[s], av = st.av[s];
            float w[NW];
#pragma unroll
            for (int c = 0; c < NW; ++c)
                w[c] = st.w[c][s];
            const float a0 = (fx0 - cu) * au, a1 = (fx1 - cu) * au;
            const float b0 = (fy0 - cv) * av, b1 = (fy1 - cv) * av;
            const float z2  = Depth ? st.z2[s] : 0.0f; // (not read, not added without Depth)
            const float a02 = Depth ? a0 * a0 + z2 : a0 * a0, a12 = Depth ? a1 * a1 + z2 : a1 * a1;
            const float b02 = b0 * b0, b12 = b1 * b1;
            const float q2[4] = {a02 + b02, a12 + b02, a02 + b12, a12 + b12};
            body(q2, w);
        }

        keyCur   = keyNext;
        keyNext  = keyNext2;
        validCur = validNext;
        r0       = n0;
        r1       = n1;
    }
}

/*! @brief the quad's values val[c][p], pixel p = (qx + (p & 1), qy + (p >> 1)): to the image if the tile has one
 *         segment, else to the block's partial tile in the workspace (thread-major) */
template<int C>
__device__ __forceinline__ void storeQuad(const TileArgs& A, const TileBlock& B, const float (&val)[C][4])
{
    if (B.nseg == 1)
    {
#pragma unroll
        for (int p = 0; p < 4; ++p)
        {
            const int px = B.tu * kTile + B.qx + (p & 1), py = B.tv * kTile + B.qy + (p >> 1);
            if (px < A.g.nu && py < A.g.nv)
#pragma unroll
                for (int c = 0; c < C; ++c)
                    A.img[(size_t(c) * A.g.nv + py) * A.g.nu + px] = val[c][p];
        }
    }
    else
    {
        float* out = A.work + size_t(blockIdx.x) * C * (kTile * kTile);
#pragma unroll
        for (int c = 0; c < C; ++c)
#pragma unroll
            for (int p = 0; p < 4; ++p)
                out[(c * 4 + p) * kTileBlock + threadIdx.x] = val[c][p];
    }
}

template<class Profile, int C>
__global__ void __launch_bounds__(kTileBlock) imageTileKernel(TileArgs A, Profile prof)
{
    __shared__ float sTab[Profile::kLds];
    // (projections stage their zero depth term as slices do: without it the compiler pairs the multiply-adds of q^2
    // differently and the last bits of the existing kinds change)
    __shared__ TileStage<C, true> st;
    TileBlock B;
    if (!tileBlockOf(A, B)) return;
    prof.load(sTab, A.table); // (in LDS by the walk's first barrier)

    float acc[C][4];
#pragma unroll
    for (int c = 0; c < C; ++c)
#pragma unroll
        for (int p = 0; p < 4; ++p)
            acc[c][p] = 0.0f;

    walkEntries(
        A, B, st,
        [&](const ImageRec& r, float(&w)[C])
        {
            const float wgt = prof.weight(r.ih);
            w[0]            = r.w0 * wgt;
            if constexpr (C == 2) w[1] = r.w1 * wgt;
            return prof.zq2(r.zq);
        },
        [&](const float(&q2)[4], const float(&w)[C])
        {
#pragma unroll
            for (int p = 0; p < 4; ++p)
                if (q2[p] < 4.0f)
                {
                    const float f = prof(sTab, q2[p]);
#pragma unroll
                    for (int c = 0; c < C; ++c)
                        acc[c][p] += w[c] * f;
                }
        });
    storeQuad<C>(A, B, acc);
}

constexpr float kLog2e     = 1.44269504088896340736f;
constexpr float kSmallTau = 0.25f; // below: 1 - exp(-tau) by its series (renderStep)

/*! @brief one compositing step of a pixel: I += T (1 - a) s, T *= a with a = exp(-tau) as the hardware's exp2
 *         (v_exp_f32) of -tau log2 e. Only the last two operations are on the pixel's dependent chains.
 *         1 - a: the subtraction itself is exact for a >= 1/2, so its error is that of a, about an ulp of a (6e-8),
 *         and relative to 1 - a ~ tau that grows as 1 / tau. Below |tau| = 1/4 (relative error of the subtraction:
 *         up to 5e-7) the alternating series tau (1 - tau/2 + tau^2/6 - ... - tau^5/720) is used instead; its first
 *         dropped term, tau^6/5040 < 4.9e-8, is below half an ulp of the bracket. */
__device__ __forceinline__ void renderStep(float tau, float s, float& I, float& T)
{
    const float a = __builtin_amdgcn_exp2f(-kLog2e * tau);
    float series  = fmaf(tau, -1.0f / 720.0f, 1.0f / 120.0f);
    series        = fmaf(tau, series, -1.0f / 24.0f);
    series        = fmaf(tau, series, 1.0f / 6.0f);
    series        = fmaf(tau, series, -0.5f);
    series        = fmaf(tau, series, 1.0f);
    const float e = (fabsf(tau) < kSmallTau ? tau * series : 1.0f - a) * s;
    I             = fmaf(T, e, I);
    T *= a;
}

/*! @brief opacity rendering of a (tile, segment): the block shape, staging and culling of imageTileKernel, the entries
 *         (in depth order, see imageRecordsKernel) composited from (I, T) = (0, 1). Staged weights: kappa m h^-2 and
 *         the source value. Output channels: 0 = I, 1 = T. */
__global__ void __launch_bounds__(kTileBlock) imageRenderKernel(TileArgs A)
{
    __shared__ float sTab[ProjProfile::kLds];
    __shared__ TileStage<2, false> st;
    TileBlock B;
    if (!tileBlockOf(A, B)) return;
    const ProjProfile prof;
    prof.load(sTab, A.table); // (in LDS by the walk's first barrier)

    float it[2][4] = {{0.0f, 0.0f, 0.0f, 0.0f}, {1.0f, 1.0f, 1.0f, 1.0f}};
    walkEntries(
        A, B, st,
        [&](const ImageRec& r, float(&w)[2])
        {
            w[0] = r.w0 * prof.weight(r.ih);
            w[1] = r.w1;
            return 0.0f;
        },
        [&](const float(&q2)[4], const float(&w)[2])
        {
#pragma unroll
            for (int p = 0; p < 4; ++p)
                if (q2[p] < 4.0f) renderStep(w[0] * prof(sTab, q2[p]), w[1], it[0][p], it[1][p]);
        });
    storeQuad<2>(A, B, it);
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

//! a rendering's tiles of several segments: the (I_s, T_s) partial tiles composed in segment order, which is the
//! list's depth order: (I, T) <- (I + T I_s, T T_s) from (0, 1)
__global__ void __launch_bounds__(kTileBlock) imageComposeKernel(TileArgs A)
{
    const int tile     = blockIdx.x;
    const int64_t seg0 = A.segOff[tile];
    const int64_t nseg = A.segOff[tile + 1] - seg0;
    if (nseg <= 1) return;
    const int tid = threadIdx.x;
    const int tu = tile % A.g.ntu, tv = tile / A.g.ntu;
    int qx, qy;
    quadOrigin(tid, qx, qy);
    float I[4] = {0.0f, 0.0f, 0.0f, 0.0f}, T[4] = {1.0f, 1.0f, 1.0f, 1.0f};
    for (int64_t s = 0; s < nseg; ++s)
    {
        const float* in = A.work + size_t(seg0 + s) * 2 * (kTile * kTile);
#pragma unroll
        for (int p = 0; p < 4; ++p)
        {
            I[p] = fmaf(T[p], in[p * kTileBlock + tid], I[p]);
            T[p] *= in[(4 + p) * kTileBlock + tid];
        }
    }
#pragma unroll
    for (int p = 0; p < 4; ++p)
    {
        const int px = tu * kTile + qx + (p & 1), py = tv * kTile + qy + (p >> 1);
        if (px >= A.g.nu || py >= A.g.nv) continue;
        A.img[size_t(py) * A.g.nu + px]            = I[p];
        A.img[(size_t(A.g.nv) + py) * A.g.nu + px] = T[p];
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

void imageDepthKeys(int64_t first, int64_t last, const double* x, const double* y, const double* z,
                    const ImageView& V, uint64_t* keys, hipStream_t s)
{
    if (!V.render) throw std::invalid_argument("imageDepthKeys: the view is no rendering");
    if (last <= first) return;
    const double* pos[3] = {x, y, z};
    imageDepthKeysKernel<<<gridFor(last - first, 256), 256, 0, s>>>(first, last - first, pos[V.ia], V, keys);
    SPHX_LAUNCH_CHECK();
}

void imageRecords(int64_t first, int64_t last, int64_t n, const double* x, const double* y, const double* z,
                  const float* h, const float* w, int C, const int32_t* perm, const ImageView& V, ImageRec* rec,
                  int64_t* counts, hipStream_t s)
{
    if (C != 1 && C != 2) throw std::invalid_argument("imageRecords: one or two channels");
    if (last - first > (int64_t(1) << kPartBits)) throw std::invalid_argument("imageRecords: more than 2^30 particles");
    if (V.render && (C != 2 || (!perm && last > first)))
        throw std::invalid_argument("imageRecords: a rendering has two channels and a depth order");
    imageRecordsKernel<<<gridFor(last - first + 1, 256), 256, 0, s>>>(first, last, n, x, y, z, h, w, C, perm, V,
                                                                      geomOf(V), rec, counts);
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
    if (V.render) throw std::invalid_argument("imageTiles: a rendering is composited by imageRender");
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

void imageRender(int64_t np, int64_t total, const uint64_t* keys, const ImageRec* rec, const ImageView& V, int ntiles,
                 int64_t segment, int64_t nblocks, const int64_t* start, const int64_t* segOff, const float* table,
                 int tableLen, float* work, float* img, hipStream_t s)
{
    const ImageGeom g = geomOf(V);
    if (!V.render) throw std::invalid_argument("imageRender: the view is no rendering");
    if (ntiles != g.ntu * g.ntv) throw std::invalid_argument("imageRender: tile count");
    if (nblocks < total / segment + ntiles || nblocks > 0x7fffffff)
        throw std::invalid_argument("imageRender: block count");
    if (tableLen != kImageTableLen) throw std::invalid_argument("imageRender: F_n table length");
    const TileArgs A{np, total, keys, rec, g, ntiles, segment, start, segOff, table, work, img};
    imageRenderKernel<<<unsigned(nblocks), kTileBlock, 0, s>>>(A);
    SPHX_LAUNCH_CHECK();
    imageComposeKernel<<<unsigned(ntiles), kTileBlock, 0, s>>>(A);
    SPHX_LAUNCH_CHECK();
}

SPHX_DCHECK_READER(dcheckImage)

} // namespace sphx::hip
