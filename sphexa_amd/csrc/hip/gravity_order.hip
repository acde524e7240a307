/*! Order-P far field (P = 1..6) over the Barnes-Hut interaction lists on gfx950.
 *
 * The interaction lists depend on the MAC only, not on the expansion order: these kernels evaluate the M2P slabs that
 * gravityListKernel wrote (both-half nodes at the front of mlist, A-only nodes at its back, B-only nodes at the back
 * of llist) in place of gravityM2PKernel, with the Cartesian multipoles of sphx/multipole.hpp instead of quadrupoles.
 * The P2P kernel, the combine and the phase split are those of gravity.hip; spilled groups walk the tree in
 * gravityGroup with the order-P evaluator OrderM2P.
 *
 * One wave per 64-target group, three passes over the list classes. Node records (fp32, centre offsets from the frame
 * origin as in gravityNodeRecordsKernel) are whole 16-B chunks and are gathered cooperatively: the lanes fetch the
 * contiguous chunks of the batch's 64 records and stage them in LDS; the next batch's chunks are in flight during
 * the arithmetic.
 *
 *  P = 4 (evalOrder4Mfma): with the traceless parts T(n) of the raw moments about the mass centre, r = t - c,
 *      V_n = T(n).r^(n-1), s_n = r.V_n, c_n = (2n-1)!!/n!:
 *          phi = -sum_n c_n s_n / r^(2n+1),   a = sum_n c_n [n V_n - (2n+1) s_n r / r^2] / r^(2n+1)
 *      V_2 and s_1 are the K = 4 products over [x, y, z, 1] of evalM2PMfma (one more column for the dipole); V_3,a =
 *      sum T_ajk (t - c)_j (t - c)_k is bilinear in the ten target monomials {xx, xy, xz, yy, yz, zz, x, y, z, 1} and
 *      the node coefficients {T_ajk (x2 off the diagonal), -2 (T_a c)_j, c.T_a c}: K = 10 padded to 12, three
 *      v_mfma_f32_16x16x4_f32 steps per component and 16-node x 16-target tile. The VALU does the powers of 1/r and
 *      the dot products.
 *  other P (evalOrderValu): every lane applies every node of the staged batch to its own target with m2pP<P>
 *      (sphx/multipole.hpp, the formula of the OpenMP path) through broadcast LDS reads.
 *
 * Resources (gfx950, hipcc -O3): see profiles/r12/multipole_order/README.md.
 */
#include "gravity_eval.h"
#include "hip_api.h"
#include "sphx/multipole.hpp"

namespace sphx::hip
{

//! @brief 16-B chunks of a node record: P = 4: {c, M | D, T2 (6) | T3 (10), 0}; else {raw moments, c, padding}
template<int P>
constexpr int orderChunks()
{
    return P == 4 ? 6 : (MultipoleOrder<P>::size + 3 + 3) / 4;
}

/*! @brief node records of the order-P evaluation, one thread per node. P = 4 detraces the raw moments of degree 2 and
 *         3 in fp64: T_ij = M_ij - delta_ij tr / 3, T_ijk = M_ijk - (delta_ij v_k + delta_ik v_j + delta_jk v_i) / 5
 *         with v_k = M_llk. Entry order of the degree-3 tensors: xxx xxy xxz xyy xyz xzz yyy yyz yzz zzz.
 */
template<int P>
__global__ void gravityOrderRecordsKernel(int64_t N, const double* __restrict__ centers, const float* __restrict__ Q,
                                          const double* __restrict__ mm, float* __restrict__ rec)
{
    constexpr int TS = MultipoleOrder<P>::size, RS = 4 * orderChunks<P>();
    const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const GravFrame f = gravFrame(mm);
    const double* cc  = centers + 4 * i;
    const float* q    = Q + int64_t(TS) * i;
    float* o          = rec + int64_t(RS) * i;
    const float c[3]  = {float(cc[0] - f.org[0]), float(cc[1] - f.org[1]), float(cc[2] - f.org[2])};
    if constexpr (P == 4)
    {
        const double tr = (double(q[4]) + double(q[7]) + double(q[9])) / 3;
        double m3[10];
#pragma unroll
        for (int k = 0; k < 10; ++k)
            m3[k] = q[10 + k];
        const double vx = (m3[0] + m3[3] + m3[5]) / 5, vy = (m3[1] + m3[6] + m3[8]) / 5,
                     vz = (m3[2] + m3[7] + m3[9]) / 5;
        o[0] = c[0], o[1] = c[1], o[2] = c[2], o[3] = q[0];
        o[4] = q[1], o[5] = q[2], o[6] = q[3];
        o[7]  = float(q[4] - tr); // T2: xx xy xz yy yz zz
        o[8]  = q[5];
        o[9]  = q[6];
        o[10] = float(q[7] - tr);
        o[11] = q[8];
        o[12] = float(q[9] - tr);
        o[13] = float(m3[0] - 3 * vx);
        o[14] = float(m3[1] - vy);
        o[15] = float(m3[2] - vz);
        o[16] = float(m3[3] - vx);
        o[17] = float(m3[4]);
        o[18] = float(m3[5] - vx);
        o[19] = float(m3[6] - 3 * vy);
        o[20] = float(m3[7] - vz);
        o[21] = float(m3[8] - vy);
        o[22] = float(m3[9] - 3 * vz);
        o[23] = 0.f;
    }
    else
    {
#pragma unroll
        for (int k = 0; k < TS; ++k)
            o[k] = q[k];
        o[TS] = c[0], o[TS + 1] = c[1], o[TS + 2] = c[2];
#pragma unroll
        for (int k = TS + 3; k < RS; ++k)
            o[k] = 0.f;
    }
}

/*! @brief cooperative gather of a batch of 64 node records of C chunks: chunk lane + 64 i of the batch (record
 *         (lane + 64 i) / C, contiguous within a record) per lane and step, staged to LDS record-major. The node ids
 *         of the batch sit one per lane (clamped to node 0 past the list's end: a valid record, never applied)
 */
template<int C>
__device__ __forceinline__ void gatherIssue(f32x4 (&r)[C], const float4* __restrict__ recs, int32_t idx)
{
    const int lane = laneId();
#pragma unroll
    for (int i = 0; i < C; ++i)
    {
        const int c = lane + 64 * i, node = c / C;
        const int32_t nd = __shfl(idx, node) & kIdMask;
        r[i]             = reinterpret_cast<const f32x4*>(recs)[int64_t(nd) * C + (c - node * C)];
    }
}

template<int C>
__device__ __forceinline__ void gatherStage(const f32x4 (&r)[C], float4* lds)
{
    const int lane = laneId();
#pragma unroll
    for (int i = 0; i < C; ++i)
        reinterpret_cast<f32x4*>(lds)[lane + 64 * i] = r[i];
}

//! @brief staged VALU evaluation of a list class (kHalves: the target halves its nodes apply to), any order
template<int P, unsigned kHalves>
__device__ inline void evalOrderValu(const int32_t* list, int n, const float4* __restrict__ recs, const P2PSrc& S,
                                     float4* stage, float xr, float yr, float zr, float acc[4])
{
    constexpr int C = orderChunks<P>(), TS = MultipoleOrder<P>::size;
    n = __builtin_amdgcn_readfirstlane(n);
    if (n <= 0) return;
    const int lane  = laneId();
    const bool mine = (kHalves & (lane < 32 ? kHalfA : kHalfB)) != 0;
    f32x4 gat[C]; // (a native vector type: the array stays in registers)
    int32_t idxN  = lane < n ? list[lane] : 0;
    int32_t idxNN = 64 + lane < n ? list[64 + lane] : 0;
    gatherIssue(gat, recs, idxN);
    for (int b0 = 0; b0 < n; b0 += 64)
    {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); // previous batch fully read before it is overwritten
        gatherStage(gat, stage);
        idxN  = idxNN;
        idxNN = b0 + 128 + lane < n ? list[b0 + 128 + lane] : 0;
        gatherIssue(gat, recs, idxN);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        const int cnt = min(64, n - b0);
        if (mine)
        {
            for (int k = 0; k < cnt; ++k)
            {
                const float* q = reinterpret_cast<const float*>(stage + k * C); // wave-uniform: broadcast reads
                m2pP<P>(xr - (q[TS] - S.co[0]), yr - (q[TS + 1] - S.co[1]), zr - (q[TS + 2] - S.co[2]), q, acc);
            }
        }
    }
}

//! @brief target side of the P = 4 tiles: M2PTarget (B operand [x, y, z, 1], coordinates, accumulators) plus the B
//!        operands of the three K = 4 steps over the monomials xx xy xz yy | yz zz x y | z 1 0 0
struct Order4Target
{
    M2PTarget q;
    float bM[3][4];
};

__device__ __forceinline__ void order4Init(Order4Target& T, float xr, float yr, float zr)
{
    m2pInit(T.q, xr, yr, zr);
    const int kq = laneId() >> 4;
#pragma unroll
    for (int tb = 0; tb < 4; ++tb)
    {
        const float X = T.q.tx[tb], Y = T.q.ty[tb], Z = T.q.tz[tb];
        T.bM[0][tb] = kq == 0 ? X * X : (kq == 1 ? X * Y : (kq == 2 ? X * Z : Y * Y));
        T.bM[1][tb] = kq == 0 ? Y * Z : (kq == 1 ? Z * Z : (kq == 2 ? X : Y));
        T.bM[2][tb] = kq == 0 ? Z : (kq == 1 ? 1.f : 0.f);
    }
}

// LDS of a wave of the P = 4 kernel (float4 units): node rows SoA | K = 4 operands | K = 12 operands (the staged raw
// records alias the K = 12 operands: they are consumed before the operands are written)
constexpr int kO4RowsAt = 0;       // 7 x 64 floats: cx cy cz M Dx Dy Dz
constexpr int kO4A2At   = 128;     // 4 (k) x 64 x {T2_xk, T2_yk, T2_zk, D_k}; k = 3: -(T2 c), -D.c
constexpr int kO4A3At   = 128 + 256; // 3 (component) x 12 (k) x 64 floats, k-major per component
constexpr int kO4Stage  = kO4A3At + 3 * 12 * 64 / 4;
static_assert(64 * orderChunks<4>() <= 3 * 12 * 64 / 4, "raw records alias the K = 12 operand area");

#ifndef SPHX_ORDER4_TBCHUNK
#define SPHX_ORDER4_TBCHUNK 2 // target blocks per tile pass: 2 x 7 MFMA result quads in flight
#endif

/*! @brief P = 4 on the matrix cores for the target blocks [kTb0, kTb1) (see the file comment). Lane ownership as in
 *         evalM2PMfma: nodes on the MFMA rows, targets on the columns, lane (kq, col) holds nodes 16 tile + 4 kq + r,
 *         r < 4, of target 16 tb + col; the partial sums are reduced by m2pFinish. The A operands are stored k-major
 *         (stores contiguous per k, the 16 lanes of a read on distinct banks).
 */
template<int kTb0, int kTb1>
__device__ inline void evalOrder4Mfma(const int32_t* list, int n, const float4* __restrict__ recs, const P2PSrc& S,
                                      float4* stage, Order4Target& T)
{
    constexpr int C = orderChunks<4>();
    n = __builtin_amdgcn_readfirstlane(n);
    if (n <= 0) return;
    const int lane = laneId(), kq = lane >> 4, col = lane & 15;
    float* sC  = reinterpret_cast<float*>(stage + kO4RowsAt);
    float4* sA = stage + kO4A2At;
    float* sB  = reinterpret_cast<float*>(stage + kO4A3At);
    float4* raw = stage + kO4A3At;
    f32x4 gat[C]; // (a native vector type: the array stays in registers)
    int32_t idxN  = lane < n ? list[lane] : 0;
    int32_t idxNN = 64 + lane < n ? list[64 + lane] : 0;
    gatherIssue(gat, recs, idxN);
    for (int b0 = 0; b0 < n; b0 += 64)
    {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); // previous batch fully read before it is overwritten
        gatherStage(gat, raw);
        idxN  = idxNN;
        idxNN = b0 + 128 + lane < n ? list[b0 + 128 + lane] : 0;
        gatherIssue(gat, recs, idxN);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        {
            // node b0 + lane: its record back from LDS, then its operands. Padding nodes (past n) are massless,
            // moment-free and far away (zero contribution)
            float4 R[C];
#pragma unroll
            for (int j = 0; j < C; ++j)
                R[j] = raw[lane * C + j];
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); // every lane has its record: the area is free
            const bool live = b0 + lane < n;
            const float z0  = live ? 1.f : 0.f;
            const float c[3] = {live ? R[0].x - S.co[0] : 1e10f, live ? R[0].y - S.co[1] : 1e10f,
                                live ? R[0].z - S.co[2] : 1e10f};
            const float M    = z0 * R[0].w;
            const float D[3] = {z0 * R[1].x, z0 * R[1].y, z0 * R[1].z};
            // T2 as rows, T3 as the three symmetric matrices T_a
            const float xx = z0 * R[1].w, xy = z0 * R[2].x, xz = z0 * R[2].y, yy = z0 * R[2].z, yz = z0 * R[2].w,
                        zz = z0 * R[3].x;
            const float t3[10] = {z0 * R[3].y, z0 * R[3].z, z0 * R[3].w, z0 * R[4].x, z0 * R[4].y,
                                  z0 * R[4].z, z0 * R[4].w, z0 * R[5].x, z0 * R[5].y, z0 * R[5].z};
            sC[lane]       = c[0];
            sC[64 + lane]  = c[1];
            sC[128 + lane] = c[2];
            sC[192 + lane] = M;
            sC[256 + lane] = D[0];
            sC[320 + lane] = D[1];
            sC[384 + lane] = D[2];
            sA[lane]       = make_float4(xx, xy, xz, D[0]);
            sA[64 + lane]  = make_float4(xy, yy, yz, D[1]);
            sA[128 + lane] = make_float4(xz, yz, zz, D[2]);
            sA[192 + lane] = make_float4(-(xx * c[0] + xy * c[1] + xz * c[2]), -(xy * c[0] + yy * c[1] + yz * c[2]),
                                         -(xz * c[0] + yz * c[1] + zz * c[2]),
                                         -(D[0] * c[0] + D[1] * c[1] + D[2] * c[2]));
            // entries of T_a: a = x: 0 1 2 / 1 3 4 / 2 4 5, a = y: 1 3 4 / 3 6 7 / 4 7 8, a = z: 2 4 5 / 4 7 8 / 5 8 9
            constexpr int kT[3][6] = {{0, 1, 2, 3, 4, 5}, {1, 3, 4, 6, 7, 8}, {2, 4, 5, 7, 8, 9}}; // 00 01 02 11 12 22
#pragma unroll
            for (int a = 0; a < 3; ++a)
            {
                const float t00 = t3[kT[a][0]], t01 = t3[kT[a][1]], t02 = t3[kT[a][2]], t11 = t3[kT[a][3]],
                            t12 = t3[kT[a][4]], t22 = t3[kT[a][5]];
                const float u0 = t00 * c[0] + t01 * c[1] + t02 * c[2];
                const float u1 = t01 * c[0] + t11 * c[1] + t12 * c[2];
                const float u2 = t02 * c[0] + t12 * c[1] + t22 * c[2];
                float* o = sB + a * 12 * 64 + lane;
                o[0 * 64]  = t00;
                o[1 * 64]  = 2.f * t01;
                o[2 * 64]  = 2.f * t02;
                o[3 * 64]  = t11;
                o[4 * 64]  = 2.f * t12;
                o[5 * 64]  = t22;
                o[6 * 64]  = -2.f * u0;
                o[7 * 64]  = -2.f * u1;
                o[8 * 64]  = -2.f * u2;
                o[9 * 64]  = u0 * c[0] + u1 * c[1] + u2 * c[2];
                o[10 * 64] = 0.f;
                o[11 * 64] = 0.f;
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        const int ntile = (min(64, n - b0) + 15) >> 4;
        for (int tile = 0; tile < ntile; ++tile)
        {
            const int nd    = 16 * tile + col;
            const float4 A2 = sA[64 * kq + nd];
            float A3[3][3]; // [component][step]
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int st = 0; st < 3; ++st)
                    A3[a][st] = sB[(a * 12 + 4 * st + kq) * 64 + nd];
            // node data of the lane's 4 rows 16 tile + 4 kq + r
            float4 N7[7];
#pragma unroll
            for (int v = 0; v < 7; ++v)
                N7[v] = reinterpret_cast<const float4*>(sC + 64 * v)[4 * tile + kq];
            const f32x4 zero     = {0.f, 0.f, 0.f, 0.f};
            constexpr int kChunk = SPHX_ORDER4_TBCHUNK < kTb1 - kTb0 ? SPHX_ORDER4_TBCHUNK : kTb1 - kTb0;
#pragma unroll
            for (int tc = kTb0; tc < kTb1; tc += kChunk)
            {
                f32x4 V2[4][3], S1[4], V3[4][3];
#pragma unroll
                for (int tb = tc; tb < tc + kChunk; ++tb)
                {
                    const float b = T.q.bT[tb];
                    V2[tb][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(A2.x, b, zero, 0, 0, 0);
                    V2[tb][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(A2.y, b, zero, 0, 0, 0);
                    V2[tb][2] = __builtin_amdgcn_mfma_f32_16x16x4f32(A2.z, b, zero, 0, 0, 0);
                    S1[tb]    = __builtin_amdgcn_mfma_f32_16x16x4f32(A2.w, b, zero, 0, 0, 0);
#pragma unroll
                    for (int a = 0; a < 3; ++a)
                    {
                        f32x4 v   = __builtin_amdgcn_mfma_f32_16x16x4f32(A3[a][0], T.bM[0][tb], zero, 0, 0, 0);
                        v         = __builtin_amdgcn_mfma_f32_16x16x4f32(A3[a][1], T.bM[1][tb], v, 0, 0, 0);
                        V3[tb][a] = __builtin_amdgcn_mfma_f32_16x16x4f32(A3[a][2], T.bM[2][tb], v, 0, 0, 0);
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int r = 0; r < 4; ++r)
                {
                    const float ncx = N7[0][r], ncy = N7[1][r], ncz = N7[2][r], nM = N7[3][r];
                    const float dx = N7[4][r], dy = N7[5][r], dz = N7[6][r];
#pragma unroll
                    for (int tb = tc; tb < tc + kChunk; ++tb)
                    {
                        const float rx = T.q.tx[tb] - ncx, ry = T.q.ty[tb] - ncy, rz = T.q.tz[tb] - ncz;
                        const float r2  = rx * rx + ry * ry + rz * rz;
                        const float ir  = __builtin_amdgcn_rsqf(r2);
                        const float ir2 = ir * ir, ir3 = ir2 * ir, ir5 = ir3 * ir2, ir7 = ir5 * ir2;
                        const float v2x = V2[tb][0][r], v2y = V2[tb][1][r], v2z = V2[tb][2][r];
                        const float v3x = V3[tb][0][r], v3y = V3[tb][1][r], v3z = V3[tb][2][r];
                        const float s2 = rx * v2x + ry * v2y + rz * v2z;
                        const float s3 = rx * v3x + ry * v3y + rz * v3z;
                        const float p0 = nM * ir, p1 = S1[tb][r] * ir3, p2 = 1.5f * s2 * ir5, p3 = 2.5f * s3 * ir7;
                        const float cmb = -(p0 + 3.f * p1 + 5.f * p2 + 7.f * p3) * ir2;
                        const float w2 = 3.f * ir5, w3 = 7.5f * ir7;
                        T.q.ph[tb][r & 1] -= (p0 + p1) + (p2 + p3);
                        T.q.ax[tb][r & 1] += (dx * ir3 + w2 * v2x + w3 * v3x) + cmb * rx;
                        T.q.ay[tb][r & 1] += (dy * ir3 + w2 * v2y + w3 * v3y) + cmb * ry;
                        T.q.az[tb][r & 1] += (dz * ir3 + w2 * v2z + w3 * v3z) + cmb * rz;
                    }
                }
            }
        }
    }
}

//! @brief LDS float4 per wave of the evaluation kernel
template<int P>
constexpr int orderStage()
{
    return P == 4 ? kO4Stage : 64 * orderChunks<P>();
}

//! @brief the order-P counterpart of gravityM2PKernel (same prologue, passes and epilogue)
template<int P>
__global__ __launch_bounds__(256, P <= 3 ? 4 : (P == 6 ? 1 : 2)) void gravityOrderM2PKernel(
    int64_t first, int64_t last, const double* __restrict__ x, const double* __restrict__ y,
    const double* __restrict__ z, const float* __restrict__ h, const float* __restrict__ m, float G,
    float* __restrict__ ax, float* __restrict__ ay, float* __restrict__ az, double* __restrict__ ugrav,
    double* __restrict__ out, unsigned long long* __restrict__ stats, GravSlabs S, const int32_t* __restrict__ order,
    int64_t numSlots, const float4* __restrict__ recs, const double* __restrict__ mm)
{
    __shared__ float4 stage[kGWaves][orderStage<P>()];
    __shared__ double red[kGWaves];
    const int wave          = threadIdx.x >> 6;
    const int64_t numGroups = (last - first + 63) / 64;
    const int64_t g         = evalGroup(order, numSlots, numGroups);
    double upot             = 0;
    const int nm            = g < numGroups ? __builtin_amdgcn_readfirstlane(S.counts[4 * g]) : -1;
    if (nm >= 0)
    {
        const int nA = __builtin_amdgcn_readfirstlane(S.counts[4 * g + 2]);
        const int nB = __builtin_amdgcn_readfirstlane(S.counts[4 * g + 3]);
        EvalTarget e    = evalTarget(g, first, last, x, y, z, h);
        const P2PSrc fr = p2pSrc(nullptr, nullptr, mm, e.tc); // quantized group center
        const float xr = e.xr + fr.dc[0], yr = e.yr + fr.dc[1], zr = e.zr + fr.dc[2];
        const int32_t* lBoth = S.mlist + g * S.capM;
        const int32_t* lA    = S.mlist + g * S.capM + S.capM - nA;
        const int32_t* lB    = S.llist + g * S.capL + S.capL - nB;
        float acc[4] = {0, 0, 0, 0};
        if constexpr (P == 4)
        {
            Order4Target T;
            order4Init(T, xr, yr, zr);
            evalOrder4Mfma<0, 4>(lBoth, nm, recs, fr, stage[wave], T);
            evalOrder4Mfma<0, 2>(lA, nA, recs, fr, stage[wave], T);
            evalOrder4Mfma<2, 4>(lB, nB, recs, fr, stage[wave], T);
            m2pFinish(T.q, acc);
        }
        else
        {
            evalOrderValu<P, kHalfA | kHalfB>(lBoth, nm, recs, fr, stage[wave], xr, yr, zr, acc);
            evalOrderValu<P, kHalfA>(lA, nA, recs, fr, stage[wave], xr, yr, zr, acc);
            evalOrderValu<P, kHalfB>(lB, nB, recs, fr, stage[wave], xr, yr, zr, acc);
        }
        gravityStore(g, first, last, acc, G, m, ax, ay, az, ugrav, stats, 0ull,
                     (unsigned long long)(nm + (nA + nB + 1) / 2), upot);
    }
    blockEnergy(upot, red, kGWaves, out);
}

//! @brief far field of a spilled group (gravityGroup): the queued nodes one after the other, centre and raw moments
//!        through wave-uniform loads, m2pP<P> per lane; entries carry their half masks
template<int P>
struct OrderM2P
{
    const float* Q;

    __device__ __forceinline__ void operator()(const int32_t* list, int n, const GravTree& t, const double tc[3],
                                               float xr, float yr, float zr, float4*, float acc[4]) const
    {
        constexpr int TS      = MultipoleOrder<P>::size;
        n                     = __builtin_amdgcn_readfirstlane(n);
        const unsigned myHalf = laneId() < 32 ? kHalfA : kHalfB;
        for (int k = 0; k < n; ++k)
        {
            const int32_t e  = __builtin_amdgcn_readfirstlane(list[k]);
            const int32_t nd = e & kIdMask;
            const double* c  = t.centers + 4 * nd;
            const float cx = float(c[0] - tc[0]), cy = float(c[1] - tc[1]), cz = float(c[2] - tc[2]);
            if (tagOf(e) & myHalf) m2pP<P>(xr - cx, yr - cy, zr - cz, Q + int64_t(TS) * nd, acc);
        }
    }
};

size_t gravityOrderRecordBytes(int order)
{
    size_t b = 0;
    withOrder(order, [&](auto o) { b = 16 * size_t(orderChunks<decltype(o)::value>()); });
    return b;
}

void gravityOrderRecords(int order, int64_t numNodes, const double* centers, const float* Q, const double* mm,
                         void* recs, hipStream_t s)
{
    if (numNodes <= 0) return;
    withOrder(order,
              [&](auto o)
              {
                  constexpr int P = decltype(o)::value;
                  gravityOrderRecordsKernel<P><<<gridFor(numNodes, 256), 256, 0, s>>>(numNodes, centers, Q, mm,
                                                                                      static_cast<float*>(recs));
                  SPHX_LAUNCH_CHECK();
              });
}

void gravityOrderM2P(int order, unsigned grid, int64_t first, int64_t last, const double* x, const double* y,
                     const double* z, const float* h, const float* m, float G, float* ax, float* ay, float* az,
                     double* ugrav, double* out, unsigned long long* stats, const GravSlabs& S,
                     const int32_t* groupOrder, int64_t numSlots, const void* recs, const double* mm, hipStream_t s)
{
    withOrder(order,
              [&](auto o)
              {
                  constexpr int P = decltype(o)::value;
                  gravityOrderM2PKernel<P><<<grid, 64 * kGWaves, 0, s>>>(first, last, x, y, z, h, m, G, ax, ay, az,
                                                                         ugrav, out, stats, S, groupOrder, numSlots,
                                                                         static_cast<const float4*>(recs), mm);
                  SPHX_LAUNCH_CHECK();
              });
}

void gravityOrderSpill(int order, int64_t first, int64_t last, const GravTree& t, const double* x, const double* y,
                       const double* z, const float* h, const float* m, float G, float* ax, float* ay, float* az,
                       double* ugrav, double* out, unsigned long long* stats, const int32_t* spillList,
                       int32_t* spillMem, const void* rec, const double* mm, const float* Q, hipStream_t s)
{
    withOrder(order,
              [&](auto o)
              {
                  constexpr int P = decltype(o)::value;
                  gravitySpillKernel<OrderM2P<P>><<<kGSpillWaves, 64, 0, s>>>(
                      first, last, t, x, y, z, h, m, G, ax, ay, az, ugrav, out, stats, spillList, spillMem,
                      static_cast<const int4*>(rec), mm, OrderM2P<P>{Q});
                  SPHX_LAUNCH_CHECK();
              });
}

} // namespace sphx::hip
