/*! Block-union LDS staging of the SPH pair loops (gfx950): the sources that the 4, 8 or 16 target groups of a block
 *  name are copied into LDS once per block, one wave walks one group, and every neighbor step reads its record there
 *  instead of gathering it from L2 (XMass, Gradh, IAD and AV: the production loops).
 *
 * Parity: the loops themselves are the reference's hydro_ve kernels (sph/include/sph/hydro_ve, the _kern.hpp files,
 * e.g. momentum_energy_kern.hpp:113-222), here through the shared J-loops of sphx/sph_math.hpp. What differs is where
 * a neighbor's record comes from. The reference re-traverses the tree per kernel (find_neighbors.cuh:204-347) and
 * reads each neighbor's fields from global memory, lane by lane.
 *
 * MI355X design: a group's source union is known from its chunk table alone: the search stores, for every chunk
 * slot, the 64-bit mask of the sources it staged for the group (packed_list.hpp), and every list code names one of
 * them (~550-600 sources for ~6,400 pair steps of a group: profiles/r6/union_*.txt). The prologue, the neighbor step
 * and the fallback to the gathered loop are described at BlockUnionShared below. An earlier design, one workgroup per
 * group with the lists split across its waves, was slower than gathering at every shape and was removed
 * (measurements: profiles/r6/staged/README.md).
 */
#pragma once

#include "common.h"
#include "sphx/packed_list.hpp"
#include "sphx/sph_math.hpp"

namespace sphx::hip
{

//! @brief record of LDS layout type R from its C staged chunks (the 16-byte records unpack as their own bits)
template<class R>
__device__ __forceinline__ R stagedUnpack(const float4* o)
{
    if constexpr (sizeof(R) == 16)
    {
        R r;
        const float4 v = o[0];
        __builtin_memcpy(&r, &v, 16);
        return r;
    }
    else return coopUnpack<R>(o);
}

// ------------------------------------------------------------------------------------------------------------
// Block-union staging: the source union of the NG SFC-consecutive groups of a block, staged in LDS once per block
// ------------------------------------------------------------------------------------------------------------

/*! One wave = one 64-target group, as in the gathered loops (no list rows split across waves, the per-target
 *  summation order is the gathered loops' order: results are bit-identical). The NG groups of a block are neighbors
 *  on the SFC and name mostly the same chunks: chunk bases are leaf-relative, so a chunk has the same base c0 in
 *  every group that staged it. Prologue (all waves):
 *    1. every wave reads its group's chunk bases and slot masks (one slot per lane, up to kBuSlots slots) and inserts
 *       them into an LDS hash keyed by c0 (compare-and-swap on the key, OR of the masks);
 *    2. one thread per hash entry: popcount of the merged mask, block-wide prefix sum -> the entry's first record
 *       position; the non-empty entries are listed densely;
 *    3. every lane looks its slot's merged entry up and keeps {c0, base, mask} in registers; the waves copy the
 *       records of the dense entries (lane k = particle c0 + k: coalesced) to their positions; every lane finds the
 *       record of its own target (the one or two slots of its wave that overlap the group's particles);
 *    4. the hash is dead: its memory becomes the per-wave slot tables, one 16-B entry per slot: for each half of the
 *       slot's 64 sources the byte offset of its first record and its 32-bit mask.
 *  Neighbor step: code (slot, off) -> table entry (one ds_read_b128) -> the half of off -> record offset = the half's
 *  offset + record size x popcount(mask below off) -> record (RC x ds_read_b128): 11 VALU instructions, no source
 *  index. The target's own entry is the one whose offset equals the target's; slot 0 (padding codes) has the entry
 *  {spare, 0, spare, 0} and decodes to the spare record past the capacity, which is skipped too.
 *  A block falls back, as a whole, to the gathered loop in the same kernel when the merged union exceeds UCAP records,
 *  a group has more than kBuSlots slots, the lists were searched without slot masks (T == Tc), a table value is out of
 *  range, the hash is full or a target is staged under two slots. The chunk tables of the gathered loop share the
 *  records' LDS. */
constexpr unsigned kBuSlots = 64;
constexpr uint32_t kBuEmpty = 0xFFFFFFFFu;

//! the group of one wave: its table and what groupTargetOf read from it
struct BlockLane
{
    const int32_t* tab;     // group table
    const int32_t* rowsInt; // row pool
    unsigned nch, Tc, T;    // chunk slots (0: no group), chunk-base rows, table rows
    unsigned gfirst;        // first particle of the group
    unsigned selfAddr;      // staged blocks: byte offset of this lane's own target in the LDS records (stageBlockUnion)

    __device__ __forceinline__ int32_t rowOf(unsigned o) const
    {
        return *(const __attribute__((address_space(4))) int32_t*)(tab + 2 + o);
    }
};

template<int NG, int UCAP, int RC>
struct BlockUnionShared
{
    static constexpr int HS = 64 * NG; // hash entries = threads of the block = slot-table entries
    union
    {
        uint4 rec[(UCAP + 1) * RC];    // (one record past the capacity: a code whose mask bit is missing stays inside)
        uint32_t ctab[NG][kChunkCap];  // gathered fallback: the groups' chunk tables
    };
    uint4 tab[HS];       // prologue: hash {c0, base, mask lo, mask hi}; loops: slot tables [wave][slot]
    uint16_t dense[HS];  // the non-empty hash entries
    unsigned wsum[NG];   // per-wave totals of the scan (records | entries << 16)
    unsigned fail;
};

/*! @brief the one reader of a group's table header, for every pair loop (targetOf in hydro.hip, UnionSource below):
 *         target i of this thread (clamped past the last particle; the return value tells whether it is valid), its
 *         list rows (pl, without a chunk table), the group's header (bl) and the neighbor count n (excluding self,
 *         capped). Threads past the last target stay alive with an empty list; they store nothing. kSlotsNeedBlocks:
 *         a group without list blocks is given no chunk slots either, the rule of UnionSource::open. */
template<int B, bool kSlotsNeedBlocks = false>
__device__ __forceinline__ bool groupTargetOf(const NbrArgs& a, int64_t& i, PackedLane& pl, unsigned& n, BlockLane& bl)
{
    const unsigned lb   = xcdRemap(blockIdx.x, gridDim.x);
    const int64_t t     = int64_t(lb) * B + threadIdx.x;
    i                   = a.first + t;
    const int64_t g     = t >> 6;
    const int64_t G     = (a.last - a.first + 63) / 64;
    const unsigned lane = threadIdx.x & 63;
    bl.tab              = a.nidx + g * int64_t(packedTableInts(a.ngmax));
    bl.rowsInt          = a.nidx + packedTableRegion(G, a.ngmax);
    bl.nch = bl.Tc = bl.T = 0;
    bl.gfirst             = unsigned(a.first + g * 64);
    bl.selfAddr           = 0;
    pl.nblk               = 0;
    if (g < G) // wave-uniform: waves past the last group have no table
    {
        pl.nblk          = unsigned(*(const __attribute__((address_space(4))) int32_t*)(bl.tab));
        const unsigned w = unsigned(*(const __attribute__((address_space(4))) int32_t*)(bl.tab + 1));
        bl.nch           = min(tableWordNch(w), kChunkCap);
        bl.Tc            = tableWordTc(w);
        bl.T             = tableWordT(w);
    }
    pl.tab  = bl.tab + 2 + bl.T;
    pl.rows = reinterpret_cast<const int4*>(bl.rowsInt) + lane;
    pl.ctab = nullptr;
#ifdef SPHX_DEVICE_CHECKS
    pl.ntot = a.ntot;
    SPHX_DCHECK(pl.nblk <= listBlocksMax(a.ngmax), 1);
    pl.nblk = min(pl.nblk, listBlocksMax(a.ngmax));
#endif
    if constexpr (kSlotsNeedBlocks) // (UnionSource::open)
        if (pl.nblk == 0) bl.nch = 0;
    if (i >= a.last)
    {
        i       = a.last - 1;
        pl.self = unsigned(i);
        n       = 0;
        return false;
    }
    pl.self = unsigned(i);
    const int cnt = a.nc[i] - 1;
    n             = unsigned(cnt < 0 ? 0 : (unsigned(cnt) < a.ngmax ? cnt : a.ngmax));
    return true;
}

/*! @brief the wave's chunk table (nch entries, one coalesced load per 64) into its LDS copy `ctab`, which the gathered
 *         loops decode the list codes through */
__device__ __forceinline__ void loadChunkTable(const BlockLane& bl, PackedLane& pl, uint32_t* ctab)
{
    const unsigned lane = threadIdx.x & 63;
    for (unsigned e = lane; e < bl.nch; e += 64)
        ctab[e] = uint32_t(bl.rowsInt[size_t(bl.rowOf(e >> 8)) * 256 + (e & 255)]);
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    pl.ctab = ctab;
}

/*! @brief the prologue (file comment above; all threads of the block call it): true if the block's union is staged
 *         (block-uniform), false if the block takes the gathered loop (nothing of sh is in use then) */
template<class R, int NG, int UCAP>
__device__ bool stageBlockUnion(BlockLane& bl, const R* __restrict__ rec, unsigned ntot,
                                BlockUnionShared<NG, UCAP, int(sizeof(R) / 16)>& sh, unsigned* counters)
{
    constexpr int RC = int(sizeof(R) / 16);
    constexpr int HS = 64 * NG;
    static_assert((HS & (HS - 1)) == 0, "hash size is a power of two");
    // at most NG * (kBuSlots - 1) < HS keys are inserted: the hash always has a free entry
    static_assert(UCAP + 64 < 65536 && NG * (kBuSlots - 1) * 64 < 65536, "the scan packs two 16-bit counts");
    const unsigned t = threadIdx.x, lane = t & 63, wave = t >> 6;
    sh.tab[t] = make_uint4(kBuEmpty, 0u, 0u, 0u);
    if (t == 0) sh.fail = 0u;
    __syncthreads();
    // 1. this wave's slots (slot = lane; slot 0 holds the padding codes only and is not staged)
    const bool masks  = bl.T >= bl.Tc + maskTabRows(bl.nch) && bl.T > bl.Tc;
    const bool waveOk = bl.nch <= kBuSlots && (bl.nch <= 1u || masks);
    const bool mine   = waveOk && lane >= 1u && lane < bl.nch;
    bool bad          = !waveOk;
    unsigned e        = 0;
    if (mine)
    {
        const uint32_t cb = uint32_t(bl.rowsInt[size_t(bl.rowOf(0)) * 256 + lane]);
        const int32_t* mr = bl.rowsInt + size_t(bl.rowOf(bl.Tc)) * 256 + 2 * lane;
        uint32_t lo = uint32_t(mr[0]), hi = uint32_t(mr[1]);
        if (cb >= ntot) bad = true; // (also excludes the empty key)
        else
        {
            // sources past the last record are never staged
            const unsigned avail = min(ntot - cb, 64u);
            const uint64_t keep  = avail >= 64u ? ~0ull : ((1ull << avail) - 1ull);
            lo &= uint32_t(keep);
            hi &= uint32_t(keep >> 32);
            unsigned hsh = (cb * 2654435761u) >> (32 - __builtin_ctz(unsigned(HS)));
            bool done    = false;
            for (int tries = 0; tries < HS && !done; ++tries)
            {
                const uint32_t old = atomicCAS(&sh.tab[hsh].x, kBuEmpty, cb);
                if (old == kBuEmpty || old == cb)
                {
                    if (lo) atomicOr(&sh.tab[hsh].z, lo);
                    if (hi) atomicOr(&sh.tab[hsh].w, hi);
                    e    = hsh;
                    done = true;
                }
                else hsh = (hsh + 1u) & unsigned(HS - 1);
            }
            if (!done) bad = true;
        }
    }
    if (bad) sh.fail = 1u;
    __syncthreads();
    // 2. positions: exclusive scan of the merged popcounts over the hash entries (and of the non-empty entries)
    uint4 ent          = sh.tab[t];
    const bool used    = ent.x != kBuEmpty;
    const unsigned cnt = used ? unsigned(__popc(ent.z) + __popc(ent.w)) : 0u;
    const unsigned pk  = cnt | (used ? 1u << 16 : 0u);
    unsigned incl      = pk;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1)
    {
        const unsigned up = unsigned(__shfl_up(int(incl), o));
        if (int(lane) >= o) incl += up;
    }
    if (lane == 63) sh.wsum[wave] = incl;
    __syncthreads();
    unsigned before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < NG; ++w)
    {
        const unsigned s = sh.wsum[w];
        before += unsigned(w) < wave ? s : 0u;
        total += s;
    }
    const unsigned excl = before + incl - pk;
    const unsigned nrec = total & 0xFFFFu, nent = total >> 16;
    const bool fits     = sh.fail == 0u && nrec <= unsigned(UCAP);
    if (!fits)
    {
        if (counters && t == 0) atomicAdd(&counters[1], 1u);
        __syncthreads(); // every thread has read fail and wsum: the chunk tables may overwrite the union's LDS
        return false;
    }
    if (used)
    {
        sh.tab[t].y               = excl & 0xFFFFu;
        sh.dense[excl >> 16]      = uint16_t(t);
    }
    __syncthreads();
    // 3. this lane's slot entry {c0, base, mask}; the record of this lane's target: in the slots of this wave whose
    //    64 sources overlap the group's 64 particles (wave-uniform loop, one or two slots)
    constexpr unsigned RS    = unsigned(RC) * 16u;    // bytes per record
    constexpr unsigned spare = unsigned(UCAP) * RS;   // the record past the capacity
    uint4 slotEnt = make_uint4(0u, 0u, 0u, 0u);
    if (mine) slotEnt = sh.tab[e];
    unsigned selfAddr = spare, found = 0;
    for (uint64_t ov = ballot(mine && slotEnt.x + 64u > bl.gfirst && slotEnt.x < bl.gfirst + 64u); ov; ov &= ov - 1)
    {
        const int s       = __builtin_ctzll(ov);
        const unsigned c0 = unsigned(__builtin_amdgcn_readlane(int(slotEnt.x), s));
        const unsigned b  = unsigned(__builtin_amdgcn_readlane(int(slotEnt.y), s));
        const uint64_t m  = uint64_t(unsigned(__builtin_amdgcn_readlane(int(slotEnt.w), s))) << 32 |
                           unsigned(__builtin_amdgcn_readlane(int(slotEnt.z), s));
        const unsigned d  = bl.gfirst + lane - c0;
        if (d < 64u && ((m >> d) & 1))
        {
            selfAddr = (b + unsigned(__popcll(m & ((1ull << d) - 1ull)))) * RS;
            ++found;
        }
    }
    bl.selfAddr = selfAddr;
    if (found > 1u) sh.fail = 1u; // (the self test is by record: a target staged twice cannot be told from a neighbor)
    for (unsigned k = wave; k < nent; k += NG)
    {
        const uint4 en   = sh.tab[sh.dense[k]];
        const uint64_t m = uint64_t(en.w) << 32 | en.z;
        if ((m >> lane) & 1)
        {
            const unsigned p = en.y + unsigned(__popcll(m & lanemaskLt()));
            const uint4* src = reinterpret_cast<const uint4*>(rec) + size_t(en.x + lane) * RC;
#pragma unroll
            for (int c = 0; c < RC; ++c)
                sh.rec[p * RC + c] = src[c];
        }
    }
    __syncthreads();
    const bool staged = sh.fail == 0u;
    if (counters && t == 0) atomicAdd(&counters[staged ? 0 : 1], 1u);
    __syncthreads(); // (every thread has read fail, and is done with the hash)
    if (!staged) return false;
    // 4. the hash becomes the slot tables: per half of the slot's sources, the byte offset of its first record and its
    //    mask; slot 0 and the slots past the table decode to the spare record
    sh.tab[t] = mine ? make_uint4(slotEnt.y * RS, slotEnt.z, (slotEnt.y + unsigned(__popc(slotEnt.z))) * RS, slotEnt.w)
                     : make_uint4(spare, 0u, spare, 0u);
    __syncthreads();
    return true;
}

/*! @brief the neighbor loop of a staged block: forEachNeighborDirect (sph_math.hpp) with the records read from the
 *         block's LDS union. Same entries, same order; the target itself and padding codes are skipped. */
template<class R, int NG, int UCAP, class F>
__device__ void forEachNeighborUnion(const PackedLane& pl, const BlockLane& bl,
                                     const BlockUnionShared<NG, UCAP, int(sizeof(R) / 16)>& sh, F&& f)
{
    constexpr int RC    = int(sizeof(R) / 16);
    const unsigned nblk = pl.nblk;
    if (nblk == 0) return;
    const uint4* wtab = sh.tab + (threadIdx.x >> 6) * 64;
    int4 w            = pl.block(0);
    constexpr unsigned RS = unsigned(RC) * 16u, spare = unsigned(UCAP) * RS;
    const char* recs      = reinterpret_cast<const char*>(sh.rec);
    const unsigned self   = bl.selfAddr;
    auto batch = [&](int w0, int w1)
    {
        const uint32_t ws[2] = {uint32_t(w0), uint32_t(w1)};
        unsigned a[4];
        R rr[4];
#pragma unroll
        for (int u = 0; u < 4; ++u)
        {
            // code = slot | off << 10 in the low or the high half of the word. A staged group has at most kBuSlots
            // slots: the masked slot stays inside the wave's table. The shift counts take the low five bits of off.
            const uint32_t wd   = ws[u >> 1];
            const bool hiHalf   = u & 1;
            const unsigned slot = (hiHalf ? wd >> 16 : wd) & (kBuSlots - 1u);
            const unsigned sh5  = (hiHalf ? wd >> 26 : wd >> kChunkSlotBits) & 31u;
            const bool upper    = hiHalf ? int32_t(wd) < 0 : (wd & 0x8000u) != 0u;
            const uint4 en      = wtab[slot];
            const uint32_t m    = (upper ? en.w : en.y) & ~(~0u << sh5);
            a[u]                = (upper ? en.z : en.x) + unsigned(__popc(m)) * RS;
#ifdef SPHX_DEVICE_CHECKS
            const unsigned code = (hiHalf ? wd >> 16 : wd) & 0xFFFFu;
            const bool ok       = (code & kChunkSlotMask) < max(bl.nch, 1u) && a[u] <= spare &&
                            ((code & kChunkSlotMask) != 0u || a[u] == spare);
            SPHX_DCHECK(ok, 0);
            if (!ok) a[u] = spare;
#endif
            uint4 o4[RC];
#pragma unroll
            for (int c = 0; c < RC; ++c)
                o4[c] = *reinterpret_cast<const uint4*>(recs + a[u] + c * 16);
            float4 o[RC];
#pragma unroll
            for (int c = 0; c < RC; ++c)
                o[c] = make_float4(__uint_as_float(o4[c].x), __uint_as_float(o4[c].y), __uint_as_float(o4[c].z),
                                   __uint_as_float(o4[c].w));
            rr[u] = stagedUnpack<R>(o);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
        {
            pinRegs(rr[u]);
            // (the loops staged this way do not use the source index: the body gets the target's)
            if (a[u] != self && a[u] != spare) f(pl.self, rr[u]);
        }
    };
    for (unsigned b = 0; b < nblk; ++b)
    {
        const int4 wn = pl.block(b + 1);
        batch(w.x, w.y);
        batch(w.z, w.w);
        w = wn;
    }
}

/*! @brief loader of a block-union kernel: staged blocks read the LDS union, the others gather per lane (the loop of
 *         the production kernels, forEachNeighborDirect) */
template<class R, int NG, int UCAP>
struct BlockUnionLoader
{
    using Shared = BlockUnionShared<NG, UCAP, int(sizeof(R) / 16)>;
    const R* r;
    const Shared* sh;
    const BlockLane* bl;
    bool staged; // block-uniform

    __device__ R operator()(unsigned j) const { return r[j]; }
};

template<int B, class R, int NG, int UCAP, class F>
__device__ void forEachNeighbor(const PackedLane* pl, int, unsigned, const BlockUnionLoader<R, NG, UCAP>& ld, F&& f)
{
    if (ld.staged) forEachNeighborUnion<R, NG, UCAP>(*pl, *ld.bl, *ld.sh, f);
    else forEachNeighborDirect(*pl, ld, f);
}

/*! @brief source policy of a pair-loop body (hydro.hip): the records of a block's groups from its LDS union. The kernel
 *         declares one Shared per block; the group's header (BlockLane) is a local of the body. */
template<class R, int B, int UCAP>
struct UnionSource
{
    using Loader = BlockUnionLoader<R, B / 64, UCAP>;
    using Shared = typename Loader::Shared;
    Shared& sh;
    unsigned* counters; // tests: blocks staged / fallen back (one atomic per block); null in production

    /*! @brief the prologue (all threads of the block call it): groupTargetOf, then the block's union into LDS; a block
     *         that cannot be staged is left on the gathered loop, its chunk tables in the records' LDS. Returns whether
     *         the block is staged (block-uniform), `valid` whether the target is. (This way round: with the staged
     *         flag handed back through a reference the union kernels compile to another instruction schedule, about 200
     *         of 1,700 instructions of XMass, measured 0.4-0.7 % slower.) */
    __device__ __forceinline__ bool open(const NbrArgs& a, const R* rec, int64_t& i, PackedLane& pl, unsigned& n,
                                         BlockLane& bl, bool& valid) const
    {
        // kSlotsNeedBlocks = true: a group without list blocks has no slots. Every searched group has at least its
        // targets' own entries, so nblk == 0 means that the search ran out of list rows for this group (neighbors.hip,
        // rowsLost): its row ordinals then point at row 0, another group's data, and a loop enqueued before the host
        // repeats the search (models/propagators.py) must neither stage nor decode it. (The flag and not a line here:
        // applied after the reader has returned, the rule costs the union kernels 2-4 VGPRs.)
        valid             = groupTargetOf<B, true>(a, i, pl, n, bl);
        const bool staged = stageBlockUnion<R, B / 64, UCAP>(bl, rec, a.ntot, sh, counters);
        if (!staged) loadChunkTable(bl, pl, sh.ctab[threadIdx.x >> 6]);
        return staged;
    }
    __device__ __forceinline__ Loader loader(const R* rec, int64_t, const BlockLane& bl, bool staged) const
    {
        return Loader{rec, &sh, &bl, staged};
    }
    /*! @brief this wave's 64 x 5 float4 of row staging for an epilogue's record writes: the records' LDS. The caller
     *         puts a block barrier between the neighbor loop and its first use: every wave must be done with the
     *         records (or chunk tables). */
    __device__ __forceinline__ float4* epilogueRows() const
    {
        static_assert(sizeof(sh.rec) >= sizeof(float4) * (B / 64) * 64 * 5, "the epilogue's rows fit the records' LDS");
        return reinterpret_cast<float4*>(sh.rec) + (threadIdx.x >> 6) * 64 * 5;
    }
};

} // namespace sphx::hip
