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
 */
#include "common.h"
#include "hip_api.h"
#include "sphx/ewald.hpp"
#include "sphx/gravity.hpp"

namespace sphx::hip
{

constexpr int kEwaldStack = 512;

__global__ __launch_bounds__(64) void ewaldTraverseKernel(
    int64_t first, int64_t last, const int32_t* __restrict__ child, const int32_t* __restrict__ n2l,
    const int32_t* __restrict__ ns, const int32_t* __restrict__ ne, const double* __restrict__ centers,
    const Quadrupole* __restrict__ mp, const double* __restrict__ x, const double* __restrict__ y,
    const double* __restrict__ z, const float* __restrict__ h, const float* __restrict__ m, double L, int S,
    double* __restrict__ sums, int* __restrict__ overflow)
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
                int sp       = 1;
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
                        for (int32_t j = ns[node]; j < ne[node]; ++j)
                            p2p(float(x[j] - px), float(y[j] - py), float(z[j] - pz), m[j], hi, h[j], acc);
                    }
                    else
                    {
                        if (sp + 8 > kEwaldStack)
                        {
                            ovf = true;
                            break;
                        }
                        __syncthreads();
                        if (threadIdx.x < 8) stack[sp + threadIdx.x] = child[node] + 7 - int(threadIdx.x);
                        sp += 8;
                        __syncthreads();
                    }
                }
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

__global__ __launch_bounds__(64) void ewaldLatticeKernel(
    int64_t first, int64_t last, const double* __restrict__ centers, const Quadrupole* __restrict__ mp,
    const double* __restrict__ x, const double* __restrict__ y, const double* __restrict__ z,
    const float* __restrict__ m, double G, double L, int S, const double* __restrict__ ktable,
    const double* __restrict__ sums, float* __restrict__ ax, float* __restrict__ ay, float* __restrict__ az,
    double* __restrict__ ugrav, double* __restrict__ esum)
{
    __shared__ double table[kEwaldTableSize];
    for (int k = threadIdx.x; k < kEwaldTableSize; k += blockDim.x)
        table[k] = ktable[k];
    __syncthreads();

    int64_t i        = first + int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    const bool valid = i < last;
    if (!valid) i = last - 1;

    // root: mass center, total mass, trace; quadrupole-only copy for the far images (their monopoles are in psi)
    const double M   = double(mp[0].q[qMass]);
    Quadrupole qOnly = mp[0];
    qOnly.q[qMass]   = 0;
    const double r[3] = {x[i] - centers[0], y[i] - centers[1], z[i] - centers[2]};

    const double* s4 = sums + 4 * (i - first);
    double acc[4]    = {s4[0], s4[1], s4[2], s4[3]};

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
    acc[0] -= 2.0 * kEwaldPi / (3.0 * L * L * L) * double(mp[0].q[qTrace]);
    // quadrupoles of the next two shells of images
    const int S2 = S + 2;
    for (int a = -S2; a <= S2; ++a)
        for (int b = -S2; b <= S2; ++b)
            for (int c = -S2; c <= S2; ++c)
            {
                if (abs(a) <= S && abs(b) <= S && abs(c) <= S) continue;
                m2p(r[0] - a * L, r[1] - b * L, r[2] - c * L, qOnly, acc);
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

void computeGravityEwald(int64_t first, int64_t last, const int32_t* child, const int32_t* n2l, const int32_t* ns,
                         const int32_t* ne, const double* centers, const void* mp, const double* x, const double* y,
                         const double* z, const float* h, const float* m, double G, double L, int numShells,
                         const double* ktable, double* sums, float* ax, float* ay, float* az, double* ugrav,
                         double* esum, int* overflow, hipStream_t s)
{
    if (last <= first) return;
    if (numShells < 0) throw std::invalid_argument("Ewald gravity: the number of replica shells must be >= 0");
    const auto* q = static_cast<const Quadrupole*>(mp);
    ewaldTraverseKernel<<<gridFor(last - first, 64), 64, 0, s>>>(first, last, child, n2l, ns, ne, centers, q, x, y,
                                                                z, h, m, L, numShells, sums, overflow);
    SPHX_LAUNCH_CHECK();
    ewaldLatticeKernel<<<gridFor(last - first, 64), 64, 0, s>>>(first, last, centers, q, x, y, z, m, G, L, numShells,
                                                               ktable, sums, ax, ay, az, ugrav, esum);
    SPHX_LAUNCH_CHECK();
}

std::vector<double> ewaldKTableHost(double L)
{
    std::vector<double> t(kEwaldTableSize);
    ewaldKTable(L, t.data());
    return t;
}

} // namespace sphx::hip
