"""Friends-of-friends groups: labels and a group catalogue.

Two particles are friends if their minimum-image distance (sphx/box.hpp, fp64) is at most the linking length b:
dx^2 + dy^2 + dz^2 <= b^2. A group is a connected component of the friendship graph; its label is the smallest
particle index in it, so the labels do not depend on the order in which links are found and are identical from run to
run and between the host and the device.

Particles are binned to cells with edges of at most b / sqrt 3: all particles of a cell are friends, no pair inside a
cell is tested, and friendship is settled between cells (sphx/fof.hpp). Device tensors run csrc/hip/fof.hip, host
tensors csrc/cpu/fof_cpu.cpp (OpenMP, fp64). Groups are local to the caller's particles: merging across ranks is not
done here.
"""

from __future__ import annotations

import torch

from . import _lib
from .reduce import min_max

MAX_PARTICLES = 1 << 30


def _coords(name, x, y, z, n):
    for c, t in (("x", x), ("y", y), ("z", z)):
        # (the native code reads raw pointers)
        if t.dtype != torch.float64 or t.shape != (n,) or not t.is_contiguous() or t.device != x.device:
            raise ValueError(f"{name}: {c} must be a contiguous float64 tensor of shape ({n},) on {x.device}")


def fof_labels(x, y, z, box, linking_length, select=None, first=0, last=None, stats=None):
    """int32 labels of the particles [first, last): the smallest index, relative to ``first``, in each particle's
    group; -1 for particles that ``select`` (bool, optional) leaves out: they neither join nor bridge. A particle with
    a coordinate that is not finite is left out as well. ``stats`` (device path): a zeroed int64 tensor of 4 counters
    of the link kernel (cell pairs entered, of those skipped by equal roots, particle pairs tested, fp64 re-tests)"""
    n = x.numel()
    last = n if last is None else int(last)
    first = int(first)
    b = float(linking_length)
    _coords("fof_labels", x, y, z, n)
    if not 0 <= first <= last <= n:
        raise ValueError("fof_labels: [first, last) outside the particle range")
    if not b > 0.0:
        raise ValueError("fof_labels: the linking length must be positive")
    np_ = last - first
    if np_ > MAX_PARTICLES:
        raise ValueError(f"fof_labels: more than 2^30 particles ({np_})")
    if select is not None:
        if select.dtype != torch.bool or select.shape != (n,) or select.device != x.device:
            raise ValueError(f"fof_labels: select must be a bool tensor of shape ({n},) on {x.device}")
        select = select.contiguous()[first:last]
    dev = x.device
    label = torch.empty(np_, dtype=torch.int32, device=dev)
    if np_ == 0:
        return label
    xs, ys, zs = x[first:last], y[first:last], z[first:last]
    # the grid of an open axis starts at the particles' smallest coordinate (the extent of all of them: a superset
    # of the selected ones, so no particle falls outside)
    ext = [0.0] * 6 if all(bc == 1 for bc in box.bc) else min_max([xs, ys, zs]).tolist()
    sel_ptr = 0 if select is None else select.data_ptr()
    barr = box.to_array()
    if dev.type != "cuda":
        _lib.cpu().fof_labels(np_, xs.data_ptr(), ys.data_ptr(), zs.data_ptr(), sel_ptr, barr, b, ext,
                              label.data_ptr())
        return label
    hp, s = _lib.hip(), _lib.stream
    i32 = lambda k: torch.empty(k, dtype=torch.int32, device=dev)
    i64 = lambda k: torch.empty(k, dtype=torch.int64, device=dev)
    keys, rec = i64((2, np_)), torch.empty((2, np_, 4), dtype=torch.float32, device=dev)
    counts = torch.zeros(4, dtype=torch.int64, device=dev)
    tmp = torch.empty(max(hp.sort_temp_bytes(np_), hp.scan_temp_bytes(np_ + 1)), dtype=torch.uint8, device=dev)
    perm, cell_of, parent, least, root = (i32(np_) for _ in range(5))
    cell_start, item_start, scan, cell_key = i32(np_ + 1), i32(np_ + 1), i64(np_ + 1), i64(np_)
    bufs = [keys[0].data_ptr(), keys[1].data_ptr(), perm.data_ptr(), rec[0].data_ptr(), rec[1].data_ptr(),
            scan.data_ptr(), cell_of.data_ptr(), cell_start.data_ptr(), cell_key.data_ptr(), parent.data_ptr(),
            least.data_ptr(), root.data_ptr(), item_start.data_ptr(), counts.data_ptr(), tmp.data_ptr(), tmp.numel()]
    hp.fof_prepare(np_, xs.data_ptr(), ys.data_ptr(), zs.data_ptr(), sel_ptr, barr, b, ext, bufs, s())
    ns, ncells, nitems, _ = counts.tolist()  # the one host synchronisation: sizes the link kernel's grid
    hp.fof_link(np_, ns, ncells, nitems, xs.data_ptr(), ys.data_ptr(), zs.data_ptr(), barr, b, ext, bufs,
                0 if stats is None else stats.data_ptr(), label.data_ptr(), s())
    _lib.raise_on_device_check("fof_labels")
    return label


def fof_catalog(labels, x, y, z, m, box, min_members=20, v=None):
    """catalogue of the groups with at least ``min_members`` members, ``count`` descending, ties by ``label``
    ascending: ``label`` (G,) int32, ``count`` (G,) int64, ``mass`` (G,) float64, ``com`` (G, 3) float64 and, with
    ``v`` = (vx, vy, vz), ``vel`` (G, 3) float64. com = r_root + sum m_j minimg(r_j - r_root) / sum m_j, wrapped into
    the box on periodic axes, r_root the label particle. The sums are fp64, in ascending particle index within a
    group, cut into pieces of 32 members that are added in piece order. ``labels`` index x, y, z, m and v from 0."""
    n = labels.numel()
    _coords("fof_catalog", x, y, z, n)
    dev = x.device
    if labels.dtype != torch.int32 or labels.device != dev or not labels.is_contiguous():
        raise ValueError(f"fof_catalog: labels must be a contiguous int32 tensor on {dev}")
    if n > MAX_PARTICLES:
        raise ValueError(f"fof_catalog: more than 2^30 particles ({n})")
    fields = [m] + (list(v) if v is not None else [])
    if any(t.shape != (n,) or t.device != dev for t in fields) or len(fields) not in (1, 4):
        raise ValueError(f"fof_catalog: m and v = (vx, vy, vz) must have shape ({n},) on {dev}")
    fields = [t.to(torch.float64).contiguous() for t in fields]
    vptr = [t.data_ptr() for t in fields[1:]] or [0, 0, 0]
    min_members = max(int(min_members), 1)
    barr = box.to_array()

    def result(label, count, mass, com, vel):
        out = dict(label=label, count=count, mass=mass, com=com)
        if v is not None:
            out["vel"] = vel
        return out

    if dev.type != "cuda":
        label, count, sums = (torch.from_numpy(a) for a in _lib.cpu().fof_catalog(
            n, labels.data_ptr(), x.data_ptr(), y.data_ptr(), z.data_ptr(), fields[0].data_ptr(), *vptr, barr,
            min_members))
        sums = sums.reshape(-1, 7)
        return result(label, count, sums[:, 0].clone(), sums[:, 1:4].clone(), sums[:, 4:7].clone())
    hp, s = _lib.hip(), _lib.stream
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    G = 0
    if n:
        keys = torch.empty((2, n), dtype=torch.int64, device=dev)
        perm = torch.empty(n, dtype=torch.int32, device=dev)
        scan = torch.empty(n + 1, dtype=torch.int64, device=dev)
        gstart = torch.empty(n + 1, dtype=torch.int32, device=dev)
        tmp = torch.empty(max(hp.sort_temp_bytes(n), hp.scan_temp_bytes(n + 1)), dtype=torch.uint8, device=dev)
        hp.fof_groups(n, labels.data_ptr(), min_members, keys[0].data_ptr(), keys[1].data_ptr(), perm.data_ptr(),
                      scan.data_ptr(), gstart.data_ptr(), counts.data_ptr(), tmp.data_ptr(), tmp.numel(), s())
        g_all, G = counts.tolist()  # the one host synchronisation: the group count
    label = torch.empty(G, dtype=torch.int32, device=dev)
    count = torch.empty(G, dtype=torch.int64, device=dev)
    mass = torch.empty(G, dtype=torch.float64, device=dev)
    com = torch.empty((G, 3), dtype=torch.float64, device=dev)
    vel = torch.empty((G, 3), dtype=torch.float64, device=dev)
    if G:
        okeys = torch.empty(g_all, dtype=torch.int64, device=dev)
        perm2 = torch.empty(g_all, dtype=torch.int32, device=dev)
        if hp.sort_temp_bytes(g_all) > tmp.numel():
            tmp = torch.empty(hp.sort_temp_bytes(g_all), dtype=torch.uint8, device=dev)
        hp.sort_keys(g_all, keys[0].data_ptr(), okeys.data_ptr(), perm2.data_ptr(), tmp.data_ptr(), tmp.numel(), s())
        hp.fof_sums(n, g_all, G, perm2.data_ptr(), gstart.data_ptr(), perm.data_ptr(), keys[1].data_ptr(),
                    x.data_ptr(), y.data_ptr(), z.data_ptr(), fields[0].data_ptr(), *vptr, barr, label.data_ptr(),
                    count.data_ptr(), mass.data_ptr(), com.data_ptr(), vel.data_ptr(), s())
    _lib.raise_on_device_check("fof_catalog")
    return result(label, count, mass, com, vel)
