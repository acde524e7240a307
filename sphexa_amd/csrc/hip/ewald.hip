/*! Periodic self-gravity (cubic box) on gfx950: Barnes-Hut over the central box and S shells of replicas, plus the
 *  Ewald lattice sum of the root multipole for every farther image.
 *
 * Parity (behaviour): reference ryoanji/src/ryoanji/nbody/traversal_ewald_cpu.hpp:46-402 (CPU-only there). Same
 * algorithm, constants and argument meaning as the OpenMP path (csrc/cpu/gravity_extra_cpu.cpp computeGravityEwald),
 * which together with directEwald is the oracle of tests/test_ewald_gpu.py.
 *
 * Two kernels:
 *  - ewaldTraverseKernel: one wave64 per group of 64 SFC-consecutive targets (the structure of multipole.hip
 *    multipoleTraverseKernel). For every replica (a, b, c) in [-S, S]^3 the wave walks the tree depth-first with a
 *    wave-uniform stack in LDS against the group box shifted by -(a, b, c) L: the MAC is evaluated once per node, so
 *    control flow never diverges; an accepted node is one quadrupole M2P per lane (node loads are wave-uniform),
 *    an opened leaf one softened P2P loop per lane. Coordinate differences are formed in fp64 and rounded to fp32;
 *    each replica is accumulated in fp32, the replica sums are added in fp64 (they cancel heavily) and stored as
 *    four fp64 sums per target.
 *  - ewaldLatticeKernel: one thread per target, fp64. Adds M psi(r), M grad psi(r) of the root mass about the root
 *    mass center minus the (2S+1)^3 explicit images, the constant trace term and the quadrupole-only M2P of the
 *    images S < |n|_inf <= S + 2 to the target's sums, then writes G a, the per-particle energy and the wave's share
 *    of 0.5 sum G m phi. The k-space sum is factored per axis (sphx/ewald.hpp): one sincos per axis, harmonics by
 *    recurrence, coefficients from a host table staged in LDS.
 *
 * Several ranks: a rank's sources are its local tree (own particles and gravity halos) and the tree over the
 * multipoles it received (ops/gravity.py remote_let_tree: no particles, received leaves carry the always-accept
 * MAC). The potential is linear in the sources, so per replica the wave walks the local tree and then the remote
 * tree into the same fp32 accumulator, and the lattice kernel adds the correction of each root: still one traversal
 * launch, one lattice launch and one overflow flag. Both kernels are templates on "a remote tree is present"; without
 * one they are the one-tree kernels with the one-tree arithmetic, bit for bit.
 */
#include "common.h"
#include "hip_api.h"
#include "sphx/ewald.hpp"
#include "sphx/gravity.hpp"

namespace sphx::hip
{

constexpr int kEwaldStack = 512;

/*! @brief one depth-first walk of a tree by the wave for the replica seen at (px, py, pz) / group box (sc, ts), added
 *  to acc; false if the stack overflowed
 *
 * @tparam Particles  false: the tree over received multipoles. Its leaves hold no particles on this rank: the
 *                    received ones are never opened (negative MAC radius), the empty ones in between have no mass
 */
template<bool Particles>
__device__ __forceinline__ bool ewaldWalk(int32_t* stack, const int32_t* __restrict__ child,
                                          const int32_t* __restrict__ n2l, const int32_t* __restrict__ ns,
                                          const int32_t* __restrict__ ne, const double* __restrict__ centers,
                                          const Quadrupole* __restrict__ mp, const double* __restrict__ x,
                                          const double* __restrict__ y, const double* __restrict__ z,
                                          const float* __restrict__ h, const float* __restrict__ m, double px,
                                          double py, double pz, float hi, const double sc[3], const double ts[3],
                                          float acc[4])
{
    int sp = 1;
    __syncthreads();
    if (threadIdx.x == 0) stack[0] = 0;
    __syncthreads();
    while (sp > 0)
    {
        int32_t node     = __builtin_amdgcn_readfirstlane(stack[--sp]);
        const double* nc = centers + 4 * int64_t(node);
        if (!macViolated(nc, nc[3], sc, ts))
        {
            if (nc[3] != 0) m2p(float(px - nc[0]), float(py - nc[1]), float(pz - nc[2]), mp[node], acc);
        }
        else if (n2l[node] >= 0)
        {
            if constexpr (Particles)
                for (int32_t j = ns[node]; j < ne[node]; ++j)
                    p2p(float(x[j] - px), float(y[j] - py), float(z[j] - pz), m[j], hi, h[j], acc);
        }
        else
        {
            if (sp + 8 > kEwaldStack) return false;
            __syncthreads();
            if (threadIdx.x < 8) stack[sp + threadIdx.x] = child[node] + 7 - int(threadIdx.x);
            sp += 8;
            __syncthreads();
        }
    }
    return true;
}

template<bool Remote>
__global__ __launch_bounds__(64) void ewaldTraverseKernel(
    int64_t first, int64_t last, const int32_t* __restrict__ child, const int32_t* __restrict__ n2l,
    const int32_t* __restrict__ ns, const int32_t* __restrict__ ne, const double* __restrict__ centers,
    const Quadrupole* __restrict__ mp, const int32_t* __restrict__ rchild, const int32_t* __restrict__ rn2l,
    const double* __restrict__ rcenters, const Quadrupole* __restrict__ rmp, const double* __restrict__ x,
    const double* __restrict__ y, const double* __restrict__ z, const float* __restrict__ h,
    const float* __restrict__ m, double L, int S, double* __restrict__ sums, int* __restrict__ overflow)
{
    __shared__ int32_t stack[kEwaldStack];
    const unsigned g = xcdRemap(blockIdx.x, gridDim.x);
    int64_t i        = first + int64_t(g) * 64 + threadIdx.x;
    const bool valid = i < last;
    if (!valid) i = last - 1;
    const double tx = x[i], ty = y[i], tz = z[i];
    const float hi  = h[i];

    double tc[3], ts[3];
    {
        double lo[3] = {waveMin(tx), waveMin(ty), waveMin(tz)};
        double up[3] = {waveMax(tx), waveMax(ty), waveMax(tz)};
        for (int d = 0; d < 3; ++d)
        {
            tc[d] = 0.5 * (lo[d] + up[d]);
            ts[d] = 0.5 * (up[d] - lo[d]);
        }
    }

    double tot[4] = {0, 0, 0, 0};
    bool ovf      = false;
    for (int a = -S; a <= S && !ovf; ++a)
        for (int b = -S; b <= S && !ovf; ++b)
            for (int c = -S; c <= S && !ovf; ++c)
            {
                // the target point and the group box seen from replica (a, b, c)
                const double px = tx - a * L, py = ty - b * L, pz = tz - c * L;
                const double sc[3] = {tc[0] - a * L, tc[1] - b * L, tc[2] - c * L};

                float acc[4] = {0, 0, 0, 0};
                ovf = !ewaldWalk<true>(stack, child, n2l, ns, ne, centers, mp, x, y, z, h, m, px, py, pz, hi, sc, ts,
                                       acc);
                if constexpr (Remote)
                    if (!ovf)
                        ovf = !ewaldWalk<false>(stack, rchild, rn2l, nullptr, nullptr, rcenters, rmp, x, y, z, h, m,
                                                px, py, pz, hi, sc, ts, acc);
                for (int d = 0; d < 4; ++d)
                    tot[d] += double(acc[d]);
            }

    if (ovf && threadIdx.x == 0) atomicAdd(overflow, 1);
    if (valid)
    {
        double* out = sums + 4 * (i - first);
        for (int d = 0; d < 4; ++d)
            out[d] = tot[d];
    }
}

/*! @brief far field of one tree beyond its explicit replicas, added to the target's sums: rc, root = the mass
 *  center and quadrupole of the tree's root, (xi, yi, zi) the target
 */
__device__ __forceinline__ void ewaldRootCorrection(const double* __restrict__ rc, const Quadrupole& root, double xi,
                                                    double yi, double zi, double L, int S, const double* table,
                                                    double acc[4])
{
    // root: mass center, total mass, trace; quadrupole-only copy for the far images (their monopoles are in psi)
    const double M   = double(root.q[qMass]);
    Quadrupole qOnly = root;
    qOnly.q[qMass]   = 0;
    const double r[3] = {xi - rc[0], yi - rc[1], zi - rc[2]};

    // monopoles of all images beyond the explicit shells: Ewald sum minus the explicit images
    double p, gr[3];
    ewaldPsi(r, L, table, p, gr);
    for (int a = -S; a <= S; ++a)
        for (int b = -S; b <= S; ++b)
            for (int c = -S; c <= S; ++c)
            {
                double s[3] = {r[0] + a * L, r[1] + b * L, r[2] + c * L};
                double d2   = s[0] * s[0] + s[1] * s[1] + s[2] * s[2];
                double id   = 1.0 / sqrt(d2);
                double id3  = id * id * id;
                p -= id;
                for (int d = 0; d < 3; ++d)
                    gr[d] += s[d] * id3;
            }
    acc[0] -= M * p;
    for (int d = 0; d < 3; ++d)
        acc[1 + d] += M * gr[d];
    // second-moment (trace) term of the far field: a constant in the target position
    acc[0] -= 2.0 * kEwaldPi / (3.0 * L * L * L) * double(root.q[qTrace]);
    // quadrupoles of the next two shells of images
    const int S2 = S + 2;
    for (int a = -S2; a <= S2; ++a)
        for (int b = -S2; b <= S2; ++b)
            for (int c = -S2; c <= S2; ++c)
            {
                if (abs(a) <= S && abs(b) <= S && abs(c) <= S) continue;
                m2p(r[0] - a * L, r[1] - b * L, r[2] - c * L, qOnly, acc);
            }
}

template<bool Remote>
__global__ __launch_bounds__(64) void ewaldLatticeKernel(
    int64_t first, int64_t last, const double* __restrict__ centers, const Quadrupole* __restrict__ mp,
    const double* __restrict__ rcenters, const Quadrupole* __restrict__ rmp, const double* __restrict__ x,
    const double* __restrict__ y, const double* __restrict__ z, const float* __restrict__ m, double G, double L,
    int S, const double* __restrict__ ktable, const double* __restrict__ sums, float* __restrict__ ax,
    float* __restrict__ ay, float* __restrict__ az, double* __restrict__ ugrav, double* __restrict__ esum)
{
    __shared__ double table[kEwaldTableSize];
    for (int k = threadIdx.x; k < kEwaldTableSize; k += blockDim.x)
        table[k] = ktable[k];
    __syncthreads();

    int64_t i        = first + int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    const bool valid = i < last;
    if (!valid) i = last - 1;

    const double* s4 = sums + 4 * (i - first);
    double acc[4]    = {s4[0], s4[1], s4[2], s4[3]};

    // one correction per root present: the local tree's, then the remote tree's
    if constexpr (!Remote)
        ewaldRootCorrection(centers, mp[0], x[i], y[i], z[i], L, S, table, acc);
    else
    {
        // a loop with one copy of the code; the compiler barrier keeps the 216 LDS table reads inside the iteration:
        // hoisted out of the loop (or shared between two inlined copies) they spill (256 VGPRs + 0.7-1.8 KB scratch
        // per lane, against 185 VGPRs and none)
#pragma unroll 1
        for (int t = 0; t < 2; ++t)
        {
            asm volatile("" ::: "memory");
            ewaldRootCorrection(t == 0 ? centers : rcenters, t == 0 ? mp[0] : rmp[0], x[i], y[i], z[i], L, S, table,
                                acc);
        }
    }

    double u = valid ? G * double(m[i]) * acc[0] : 0.0;
    if (valid)
    {
        if (ugrav) ugrav[i] += u;
        ax[i] += float(G * acc[1]);
        ay[i] += float(G * acc[2]);
        az[i] += float(G * acc[3]);
    }
    u = waveSum(u);
    if (threadIdx.x == 0) atomicAdd(esum, 0.5 * u);
}

//! remote tree: rnodes nodes (0: none), child offsets, node-to-leaf map, centers and quadrupoles (no particles)
void computeGravityEwald(int64_t first, int64_t last, const int32_t* child, const int32_t* n2l, const int32_t* ns,
                         const int32_t* ne, const double* centers, const void* mp, int64_t rnodes,
                         const int32_t* rchild, const int32_t* rn2l, const double* rcenters, const void* rmp,
                         const double* x, const double* y, const double* z, const float* h, const float* m, double G,
                         double L, int numShells, const double* ktable, double* sums, float* ax, float* ay, float* az,
                         double* ugrav, double* esum, int* overflow, hipStream_t s)
{
    if (last <= first) return;
    if (numShells < 0) throw std::invalid_argument("Ewald gravity: the number of replica shells must be >= 0");
    if (rnodes > 0 && !(rchild && rn2l && rcenters && rmp))
        throw std::invalid_argument("Ewald gravity: remote tree arrays missing");
    const auto* q  = static_cast<const Quadrupole*>(mp);
    const auto* rq = static_cast<const Quadrupole*>(rmp);
    const unsigned grid = gridFor(last - first, 64);
    if (rnodes > 0)
    {
        ewaldTraverseKernel<true><<<grid, 64, 0, s>>>(first, last, child, n2l, ns, ne, centers, q, rchild, rn2l,
                                                      rcenters, rq, x, y, z, h, m, L, numShells, sums, overflow);
        SPHX_LAUNCH_CHECK();
        ewaldLatticeKernel<true><<<grid, 64, 0, s>>>(first, last, centers, q, rcenters, rq, x, y, z, m, G, L,
                                                     numShells, ktable, sums, ax, ay, az, ugrav, esum);
    }
    else
    {
        ewaldTraverseKernel<false><<<grid, 64, 0, s>>>(first, last, child, n2l, ns, ne, centers, q, nullptr, nullptr,
                                                       nullptr, nullptr, x, y, z, h, m, L, numShells, sums, overflow);
        SPHX_LAUNCH_CHECK();
        ewaldLatticeKernel<false><<<grid, 64, 0, s>>>(first, last, centers, q, nullptr, nullptr, x, y, z, m, G, L,
                                                      numShells, ktable, sums, ax, ay, az, ugrav, esum);
    }
    SPHX_LAUNCH_CHECK();
}

std::vector<double> ewaldKTableHost(double L)
{
    std::vector<double> t(kEwaldTableSize);
    ewaldKTable(L, t.data());
    return t;
}

} // namespace sphx::hip
