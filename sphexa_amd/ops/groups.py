"""Bound groups: the self-potential of friends-of-friends groups and their unbinding.

Definitions (sphx/groups.hpp): the members of a group have the offsets d_i = minimg(x_i - x_root) from the label
particle, formed in fp64 and rounded once to fp32; phi_i = -G sum_{j != i} m_j / sqrt(|d_i - d_j|^2 + eps^2) over the
bound members of the same group (Plummer softening, j != i by index); an iteration forms the bulk velocity V of the
bound members, the specific energies e_i = 0.5 |v_i - V|^2 + u_i + phi_i, removes the members with e_i > 0 and
dissolves a group that falls below ``min_members``. The loop ends when an iteration removes nothing or after
``max_iter`` iterations; what is returned belongs to the final bound set.

Device tensors run csrc/hip/groups.hip: a segmented all-pairs kernel over all groups at once, one wave per (group,
target tile, source segment). Host tensors run csrc/cpu/groups_cpu.cpp (OpenMP, fp64 sums). The cost is the sum of
n_g^2 over the groups: a single group of many millions of members wants a tree instead, which is not done here; a
group of more than SPHX_GROUP_SEGMENT members also takes 8 B n_g^2 / SPHX_GROUP_SEGMENT of partial rows.
"""

from __future__ import annotations

import os

import torch

from . import _lib
from .fof import MAX_PARTICLES, _coords, fof_catalog

SEGMENT = 2048  # sources per item (groups.hpp kGroupSegment); SPHX_GROUP_SEGMENT overrides, a multiple of 64


def bound_groups(labels, x, y, z, m, v, box, eps, G=1.0, u=None, min_members=20, max_iter=20):
    """(bound, phi, catalogue) of the groups ``labels`` (fof_labels' convention: the smallest member index, -1 left
    out) with at least ``min_members`` members: ``bound`` (n,) bool, ``phi`` (n,) float64 (NaN where not bound), and
    the catalogue of fof_catalog (``label``, ``count``, ``mass``, ``com``) with ``bound_count`` (G,) int64,
    ``bound_mass``, ``ekin`` = sum 0.5 m |v - V|^2, ``eint`` = sum m u (0 without ``u``), ``epot`` = 0.5 sum m phi
    (G,) float64, ``vel`` (the bulk velocity of the bound members) and ``centre`` (the bound member of lowest phi,
    wrapped into the box) (G, 3) float64, ``centre_index`` and ``most_bound`` (lowest e) (G,) int32 particle indices
    (-1, and NaN for vel and centre, where nothing is bound) and ``iterations``, the number of removal passes, the one
    that removed nothing included. ``v`` = (vx, vy, vz); ``max_iter`` = 0 evaluates the full groups."""
    n = labels.numel()
    _coords("bound_groups", x, y, z, n)
    dev = x.device
    if labels.dtype != torch.int32 or labels.device != dev or not labels.is_contiguous():
        raise ValueError(f"bound_groups: labels must be a contiguous int32 tensor on {dev}")
    if n > MAX_PARTICLES:
        raise ValueError(f"bound_groups: more than 2^30 particles ({n})")
    eps, max_iter, min_members = float(eps), int(max_iter), max(int(min_members), 1)
    if not eps > 0.0 or not eps < 1e150:
        raise ValueError("bound_groups: eps must be positive")
    if max_iter < 0:
        raise ValueError("bound_groups: max_iter must not be negative")
    fields = [m] + list(v) + ([u] if u is not None else [])
    if len(fields) not in (4, 5) or any(t.shape != (n,) or t.device != dev for t in fields):
        raise ValueError(f"bound_groups: m, v = (vx, vy, vz) and u must have shape ({n},) on {dev}")
    fields = [t.to(torch.float64).contiguous() for t in fields]
    fptr = [t.data_ptr() for t in fields] + ([0] if u is None else [])
    barr = box.to_array()
    cat = fof_catalog(labels, x, y, z, fields[0], box, min_members=min_members)
    ng = cat["label"].numel()
    bound = torch.zeros(n, dtype=torch.bool, device=dev)
    phi = torch.full((n,), float("nan"), dtype=torch.float64, device=dev)

    def result(iterations, bcount, sums, centre_index, most_bound):
        sums = sums.reshape(-1, 10)
        cat.update(bound_count=bcount, bound_mass=sums[:, 0].clone(), vel=sums[:, 1:4].clone(),
                   ekin=sums[:, 4].clone(), eint=sums[:, 5].clone(), epot=sums[:, 6].clone(),
                   centre=sums[:, 7:10].clone(), centre_index=centre_index, most_bound=most_bound,
                   iterations=int(iterations))
        return bound, phi, cat

    if dev.type != "cuda":
        out = _lib.cpu().bound_groups(n, labels.data_ptr(), x.data_ptr(), y.data_ptr(), z.data_ptr(), *fptr, barr, eps,
                                      float(G), min_members, max_iter, bound.data_ptr(), phi.data_ptr())
        return result(out[0], *(torch.from_numpy(a) for a in out[1:]))

    hp, s = _lib.hip(), _lib.stream
    seg = int(os.environ.get("SPHX_GROUP_SEGMENT", SEGMENT))
    if seg < 64 or seg % 64:
        raise ValueError("SPHX_GROUP_SEGMENT must be a positive multiple of 64")
    i32 = lambda *k: torch.empty(k, dtype=torch.int32, device=dev)
    i64 = lambda *k: torch.empty(k, dtype=torch.int64, device=dev)
    f64 = lambda *k: torch.empty(k, dtype=torch.float64, device=dev)
    bcount, sums, centre_index, most_bound = i64(ng), f64(ng, 10), i32(ng), i32(ng)
    if ng == 0:
        return result(0, bcount, sums, centre_index, most_bound)
    # the sorted membership, as fof_catalog forms it (the catalogue above has read the group counts already)
    cat_counts = torch.zeros(2, dtype=torch.int64, device=dev)
    keys, perm, scan, gstart = i64(2, n), i32(n), i64(n + 1), i32(n + 1)
    tmp = torch.empty(max(hp.sort_temp_bytes(n), hp.scan_temp_bytes(n + 1)), dtype=torch.uint8, device=dev)
    hp.fof_groups(n, labels.data_ptr(), min_members, keys[0].data_ptr(), keys[1].data_ptr(), perm.data_ptr(),
                  scan.data_ptr(), gstart.data_ptr(), cat_counts.data_ptr(), tmp.data_ptr(), tmp.numel(), s())
    g_all = int(cat_counts[0])  # (a host read of the set-up, as in fof_catalog)
    okeys, perm2 = i64(g_all), i32(g_all)
    hp.sort_keys(g_all, keys[0].data_ptr(), okeys.data_ptr(), perm2.data_ptr(), tmp.data_ptr(), tmp.numel(), s())
    M = int(cat["count"].sum())  # the members of the kept groups: at most n
    rec, idx, grp = torch.empty((2, M, 4), dtype=torch.float32, device=dev), i32(2, M), i32(2, M)
    plan, counters = i64(3, ng + 1), torch.zeros(4, dtype=torch.int64, device=dev)
    mphi, me, vg = f64(M), f64(M), f64(ng, 4)
    bufs = [rec[0].data_ptr(), rec[1].data_ptr(), idx[0].data_ptr(), idx[1].data_ptr(), grp[0].data_ptr(),
            grp[1].data_ptr(), bcount.data_ptr(), plan[0].data_ptr(), plan[1].data_ptr(), plan[2].data_ptr(),
            scan.data_ptr(), counters.data_ptr(), mphi.data_ptr(), me.data_ptr(), vg.data_ptr(), tmp.data_ptr(),
            tmp.numel()]
    hp.group_init(n, g_all, ng, seg, perm2.data_ptr(), gstart.data_ptr(), bufs, s())
    _, n_items, n_partial, m_dev = counters.tolist()  # a host read of the set-up: sizes the first potential launch
    if m_dev != M:
        raise RuntimeError("bound_groups: the member count of the plan differs from the catalogue's")
    hp.group_members(n, g_all, ng, M, perm2.data_ptr(), gstart.data_ptr(), perm.data_ptr(), x.data_ptr(),
                     y.data_ptr(), z.data_ptr(), fptr[0], barr, bufs, s())
    partial, cur, iterations = None, 0, 0
    while True:
        if n_partial and (partial is None or partial.numel() < n_partial):
            partial = f64(n_partial)
        hp.group_evaluate(n, ng, M, n_items, n_partial, seg, cur, eps, float(G), fptr, bufs,
                          partial.data_ptr() if n_partial else 0, s())
        if iterations == max_iter:
            break
        iterations += 1
        counters.zero_()
        hp.group_remove(n, ng, M, min_members, seg, cur, bufs, s())
        # the one synchronisation of an iteration: the members removed, and the sizes of the next launches
        removed, n_items, n_partial, m_next = counters.tolist()
        if removed == 0:
            break  # (the compacted set equals the current one: phi and e stay valid)
        if m_next != M - removed:
            raise RuntimeError("bound_groups: the compaction lost members")
        M, cur = m_next, 1 - cur
    hp.group_catalog(n, ng, M, cur, x.data_ptr(), y.data_ptr(), z.data_ptr(), fptr, barr, bufs, bcount.data_ptr(),
                     sums.data_ptr(), centre_index.data_ptr(), most_bound.data_ptr(), bound.data_ptr(),
                     phi.data_ptr(), s())
    _lib.raise_on_device_check("bound_groups")
    return result(iterations, bcount, sums, centre_index, most_bound)
