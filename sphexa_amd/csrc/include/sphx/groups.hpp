/*! Bound groups: self-potential and unbinding of friends-of-friends groups. The definitions shared by the host path
 *  (cpu/groups_cpu.cpp) and the gfx950 kernels (hip/groups.hip); the sequence is in ops/groups.py.
 *
 *  Offsets. The members of the group with label particle r have the offsets d_i = minimg(x_i - x_r), formed in fp64
 *  (fofMinImage) and rounded once to fp32. Pair separations are differences of these offsets: no minimum image per
 *  pair, so a group that wraps more than half a periodic axis is still well defined.
 *
 *  Potential. Plummer softening with one scalar eps > 0,
 *      phi_i = -G sum_{j != i, j bound, same group} m_j / sqrt(|d_i - d_j|^2 + eps^2),
 *  j != i by member index: two different members at one position interact with -G m_j / eps.
 *
 *  Unbinding. Per iteration: V = sum m v / sum m over the bound members (fp64, ascending member index, pieces of
 *  kGroupPiece consecutive bound members added in piece order, every product rounded on its own, as fofSums does),
 *  e_i = 0.5 |v_i - V|^2 + u_i + phi_i in fp64, members with e_i > 0 leave, a group that falls below min_members is
 *  dissolved. The loop ends when an iteration removes nothing or after max_iter iterations; what is reported is the
 *  potential and the energy of the final bound set.
 *
 *  Error of the device's pair term (the bound of tests/test_groups.py), u = 2^-24 the unit roundoff of fp32, D the
 *  largest offset norm of the group, t = d_i - d_j, r2 = |t|^2 + eps^2:
 *    - one rounding of every offset component, at most u D each: a component of t is off by at most 2 u D, |t|^2 by
 *      2 (|t_x| + |t_y| + |t_z|) 2 u D <= 4 sqrt 3 u D |t|, and |t| / r2 <= 1 / (2 eps), so r2 is off by the
 *      fraction 2 sqrt 3 u D / eps and r2^(-1/2) by half of that: 1.74 u D / eps                     -> c' = 2
 *    - the three subtractions (u each on t_a, 2 u on t_a^2), the product, two multiply-adds and the add of eps^2
 *      (4 roundings of a sum of positive terms): 6 u on r2, 3 u on r2^(-1/2)                            -> 3
 *    - v_rsq_f32, 1 ulp = 2 u                                                                         -> 2
 *    - the mass rounded to fp32                                                                       -> 1
 *    - a chunk's fp32 partial sum: 64 multiply-adds onto a sum of positive terms, at most 64 u of it  -> 64
 *    - second-order terms and the fp64 additions of the chunk sums (n_g / 64 roundings of 2^-53)      -> 1
 *  so |phi_i - phi_ref,i| <= 2^-24 (71 + 2 D / eps) |phi_ref,i|: all terms have one sign, the bound does not grow with
 *  the group size. The host path sums in fp64 in member order: 2 n_g 2^-53 |phi_ref,i|.
 */
#pragma once

#include "fof.hpp"

namespace sphx
{

constexpr int kGroupPiece     = kFofPiece; // members per ordered piece of a group sum
constexpr int kGroupChunk     = 64;        // sources per staged chunk: the device's fp32 partial sums
constexpr int64_t kGroupMaxN  = kFofMaxN;
constexpr double kGroupErrC   = 71.0;      // the bound above: 2^-24 (kGroupErrC + kGroupErrCD D / eps) |phi|
constexpr double kGroupErrCD  = 2.0;
constexpr int kGroupSegment   = 2048;      // default sources per item (SPHX_GROUP_SEGMENT)

//! @brief one component of a member's offset from the label particle: fp64 minimum image, rounded once
SPHX_HD float groupOffset(double x, double xRoot, const Box& box, int a) { return float(fofMinImage(x - xRoot, box, a)); }

//! @brief the specific energy; every product rounded on its own (the host and the device form the same bits from the
//!        same phi)
SPHX_HD double groupEnergy(double vx, double vy, double vz, const double* V, double u, double phi)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double wx = vx - V[0], wy = vy - V[1], wz = vz - V[2];
    const double xx = wx * wx, yy = wy * wy, zz = wz * wz;
    return (0.5 * ((xx + yy) + zz) + u) + phi;
}

//! @brief sources per item from the knob: a positive multiple of the chunk
inline int groupSegment(int64_t knob)
{
    if (knob < kGroupChunk || knob % kGroupChunk != 0 || knob > (int64_t(1) << 24))
        throw std::invalid_argument("groups: SPHX_GROUP_SEGMENT must be a multiple of 64 between 64 and 2^24");
    return int(knob);
}

} // namespace sphx
