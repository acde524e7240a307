/*! Barnes-Hut gravity with Cartesian multipoles of order P (1..6) on gfx950.
 *
 * Parity (capability): reference ryoanji/src/ryoanji/nbody/upwardpass.cuh:44-231 (computeLeafMultipoles one
 * thread per leaf, upsweepMultipoles per level), kernel.hpp:460-634 (P2M / M2M / M2P of SphericalMultipole<P>) and
 * traversal.cuh:60-526 (warp-per-target-group Barnes-Hut walk), as used by the single-GPU demo
 * (ryoanji/test/demo.cu, P = 4). The production quadrupole path is gravity.hip; this one serves higher-order far
 * fields.
 *
 * This file holds the upsweep (one thread per leaf / node): moments are accumulated in fp64 (P2M, M2M) and stored as
 * fp32. They are evaluated over the interaction lists of gravity.hip by the kernels of gravity_order.hip.
 */
#include "common.h"
#include "hip_api.h"
#include "sphx/gravity.hpp"
#include "sphx/multipole.hpp"

namespace sphx::hip
{

template<int P>
__global__ __launch_bounds__(64) void multipoleLeafKernel(int64_t N, const int32_t* __restrict__ n2l,
                                                         const int32_t* __restrict__ ns,
                                                         const int32_t* __restrict__ ne, const double* __restrict__ x,
                                                         const double* __restrict__ y, const double* __restrict__ z,
                                                         const float* __restrict__ m,
                                                         const double* __restrict__ centers, float* __restrict__ Q)
{
    constexpr int TS = MultipoleOrder<P>::size;
    int64_t i        = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= N || n2l[i] < 0) return;
    double q[TS];
#pragma unroll
    for (int k = 0; k < TS; ++k)
        q[k] = 0;
    const double cx = centers[4 * i], cy = centers[4 * i + 1], cz = centers[4 * i + 2];
    for (int32_t p = ns[i]; p < ne[i]; ++p)
        p2mAdd<P>(x[p] - cx, y[p] - cy, z[p] - cz, double(m[p]), q);
#pragma unroll
    for (int k = 0; k < TS; ++k)
        Q[TS * i + k] = float(q[k]);
}

template<int P>
__global__ __launch_bounds__(64) void multipoleLevelKernel(int64_t a, int64_t b, const int32_t* __restrict__ n2l,
                                                          const int32_t* __restrict__ child,
                                                          const double* __restrict__ centers, float* __restrict__ Q)
{
    constexpr int TS = MultipoleOrder<P>::size;
    int64_t i        = a + int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= b || n2l[i] >= 0) return;
    double q[TS];
#pragma unroll
    for (int k = 0; k < TS; ++k)
        q[k] = 0;
    const double cx = centers[4 * i], cy = centers[4 * i + 1], cz = centers[4 * i + 2];
    for (int k = 0; k < 8; ++k)
    {
        int32_t ci = child[i] + k;
        m2mAdd<P>(centers[4 * ci] - cx, centers[4 * ci + 1] - cy, centers[4 * ci + 2] - cz, Q + TS * ci, q);
    }
#pragma unroll
    for (int k = 0; k < TS; ++k)
        Q[TS * i + k] = float(q[k]);
}

void multipoleUpsweep(int order, int64_t N, const int32_t* n2l, const int32_t* child, const int64_t* levelRange,
                      const int32_t* ns, const int32_t* ne, const double* x, const double* y, const double* z,
                      const float* m, const double* centers, float* Q, hipStream_t s)
{
    withOrder(order,
              [&](auto o)
              {
                  constexpr int P = decltype(o)::value;
                  if (N <= 0) return;
                  multipoleLeafKernel<P><<<gridFor(N, 64), 64, 0, s>>>(N, n2l, ns, ne, x, y, z, m, centers, Q);
                  SPHX_LAUNCH_CHECK();
                  for (int l = kMaxLevel; l >= 0; --l)
                  {
                      int64_t a = levelRange[l], b = levelRange[l + 1];
                      if (b <= a) continue;
                      multipoleLevelKernel<P><<<gridFor(b - a, 64), 64, 0, s>>>(a, b, n2l, child, centers, Q);
                      SPHX_LAUNCH_CHECK();
                  }
              });
}

} // namespace sphx::hip
