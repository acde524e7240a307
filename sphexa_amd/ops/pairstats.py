"""Pair statistics: pair counts per radial bin, weighted counts and velocity structure-function sums.

Inputs: fp64 coordinates ``x, y, z``, the simulation ``box``, ``edges``: nb + 1 ascending radii e_0 < ... < e_nb with
1 <= nb <= 64 and e_0 >= 0, optional weights ``w``, optional velocities ``v = (vx, vy, vz)`` (held as fp32), an
optional bool mask ``select`` and a particle range [first, last); the last three behave as in ``fof_labels``. A
particle with a coordinate that is not finite is left out.

A pair is an unordered {i, j}, i != j, both selected. d = minimg(r_j - r_i) in fp64 (sphx/box.hpp),
d2 = (dx*dx + dy*dy) + dz*dz, and the pair belongs to bin k iff e_k*e_k <= d2 < e_{k+1}*e_{k+1}, compared in fp64.
With dv = v_j - v_i (fp64, from the fp32 values) and u = (dv . d) / sqrt(d2) (u = 0 for d2 == 0) a bin holds

    count            number of pairs (int64, exact)       always
    ww               sum w_i w_j                          with w
    dl1, dl2, dl3    sum u, sum u^2, sum u^3              with v
    dv2              sum dv . dv                          with v

All of them are symmetric under i <-> j. The value channels are sums of integers: a term t of channel c enters as
llrint(t / q_c) into an int64. The quantum q_c = B_c Pp 2^-62 is a power of two: Pp is the smallest power of two at or
above ``pairs_bound``, the number of candidate pairs (the sum over the occupied cells of count(cell) * count(the cell
and its half stencil), formed during the preparation; an upper bound on every bin's count), and B_c the smallest
power of two at or above the bound of one term: W^2 for ww (W = max |w|), D, D^2, D^3, D^2 for dl1, dl2, dl3, dv2 with
D^2 = sum_a (max v_a - min v_a)^2 (``ops.reduce.min_max``). No sum can overflow, integer addition is associative, and
the result is bit-identical from run to run whatever the order in which the waves run. Returned are
sum_c = int_c * q_c as fp64 and ``quantum``, the q_c. More than 2^38 candidate pairs raise ValueError (fewer than 24
bits would be left below B_c): subsample with ``select``.

Geometry: the particles are binned to cells whose edge is at least r_max = e_nb (r_max (1 + 2^-20), to be exact), and
pairs are looked for in a cell and the 13 cells of its half stencil. Every periodic axis must hold at least 3 such
cells, r_max <= L / 3 (less the 2^-20), which makes the 27-cell stencil and the minimum image unambiguous, and no axis
may have more than 2^21 cells; otherwise ValueError.

Device tensors run csrc/hip/pairstats.hip, host tensors csrc/cpu/pairstats_cpu.cpp (OpenMP, the reference
configuration); both use the arithmetic of sphx/pairstats.hpp, so the counts are equal and the sums are equal wherever
the two compilers round the term function alike. Pairs are local to the caller's particles: nothing crosses ranks.
"""

from __future__ import annotations

import math

import torch

from . import _lib
from .fof import MAX_PARTICLES, _coords
from .reduce import min_max

MAX_BINS = 64
MAX_PAIRS_BOUND = 1 << 38
VALUE_CHANNELS = ("ww", "dl1", "dl2", "dl3", "dv2")
_variant = 0  # accumulation of the device path: 0 replicated LDS histogram, 1 ballot per distinct bin (measurements)


def pair_statistics(x, y, z, box, edges, w=None, v=None, select=None, first=0, last=None, stats=None):
    """dict of ``count`` (nb,) int64, the channels that ``w`` and ``v`` bring (each (nb,) float64), ``quantum`` (dict
    of the q_c of those channels) and ``pairs_bound`` for the particles [first, last); see the module's docstring.
    ``stats`` (device path): a zeroed int64 tensor of 3 counters of the pair kernel (candidates tested, passed the
    fp32 filter, evaluated in fp64)"""
    n = x.numel()
    last = n if last is None else int(last)
    first = int(first)
    _coords("pair_statistics", x, y, z, n)
    if not 0 <= first <= last <= n:
        raise ValueError("pair_statistics: [first, last) outside the particle range")
    dev = x.device
    # (a plain sequence of numbers is taken as float64; a tensor or an array must be float64 itself)
    edges = torch.as_tensor(edges, dtype=None if hasattr(edges, "dtype") else torch.float64)
    if edges.dtype != torch.float64 or edges.dim() != 1:
        raise ValueError("pair_statistics: edges must be a one-dimensional float64 tensor or array")
    edges = edges.tolist()
    nb = len(edges) - 1
    if not 1 <= nb <= MAX_BINS:
        raise ValueError(f"pair_statistics: between 1 and {MAX_BINS} bins, not {nb}")
    if not edges[0] >= 0.0 or not all(a < b for a, b in zip(edges, edges[1:])) or not edges[-1] < math.inf:
        raise ValueError("pair_statistics: the edges must be finite, ascending and not negative")
    np_ = last - first
    if np_ > MAX_PARTICLES:
        raise ValueError(f"pair_statistics: more than 2^30 particles ({np_})")
    if select is not None:
        if select.dtype != torch.bool or select.shape != (n,) or select.device != dev:
            raise ValueError(f"pair_statistics: select must be a bool tensor of shape ({n},) on {dev}")
        select = select.contiguous()[first:last]
    fields = ([w] if w is not None else []) + (list(v) if v is not None else [])
    if (v is not None and len(v) != 3) or any(
            not torch.is_tensor(t) or not t.is_floating_point() or t.shape != (n,) or t.device != dev for t in fields):
        raise ValueError(f"pair_statistics: w and v = (vx, vy, vz) must be floating-point tensors of shape ({n},) "
                         f"on {dev}")
    channels = (1 if w is not None else 0) | (2 if v is not None else 0)
    present = (["ww"] if w is not None else []) + (list(VALUE_CHANNELS[1:]) if v is not None else [])
    out = torch.zeros((6, nb), dtype=torch.int64, device=dev)

    def result(q, bound):
        res = dict(count=out[0].clone())
        for name in present:
            c = VALUE_CHANNELS.index(name)
            res[name] = out[1 + c].to(torch.float64) * q[c]
        res["quantum"] = {name: q[VALUE_CHANNELS.index(name)] for name in present}
        res["pairs_bound"] = int(bound)
        return res

    if np_ == 0:
        return result([1.0] * 5, 0)
    xs, ys, zs = x[first:last], y[first:last], z[first:last]
    ws = None if w is None else w[first:last].to(torch.float64).contiguous()
    vs = None if v is None else [t[first:last].to(torch.float32).contiguous() for t in v]
    # one host read: the extent of the coordinates (open axes: the grid starts at the smallest one), the velocity
    # ranges and the largest weight
    mm = torch.zeros(14, dtype=torch.float64, device=dev)

    def put(lo, tensors):
        if dev.type == "cuda":
            min_max(tensors, out=mm[lo:lo + 2 * len(tensors)])
        else:
            mm[lo:lo + 2 * len(tensors)] = min_max(tensors)

    put(0, [xs, ys, zs])
    if vs is not None:
        put(6, vs)
    if ws is not None:
        put(12, [ws])
    mm = mm.tolist()
    ext = [0.0] * 6 if all(bc == 1 for bc in box.bc) else mm[:6]
    vrange = [mm[7] - mm[6], mm[9] - mm[8], mm[11] - mm[10]] if vs is not None else [0.0] * 3
    W = max(abs(mm[12]), abs(mm[13])) if ws is not None else 0.0
    if not all(math.isfinite(t) for t in vrange + [W]):
        raise ValueError("pair_statistics: the weights and the velocities must be finite")
    ptr = lambda t: 0 if t is None else t.data_ptr()
    sel_ptr, w_ptr, v_ptr = ptr(select), ptr(ws), [ptr(t) for t in vs] if vs is not None else [0, 0, 0]
    barr = box.to_array()
    if dev.type != "cuda":
        bound, q = _lib.cpu().pair_statistics(np_, xs.data_ptr(), ys.data_ptr(), zs.data_ptr(), sel_ptr, barr, edges,
                                              ext, w_ptr, *v_ptr, W, vrange, MAX_PAIRS_BOUND, out.data_ptr())
        return result(q, bound)
    hp, s = _lib.hip(), _lib.stream
    i32 = lambda k: torch.empty(k, dtype=torch.int32, device=dev)
    i64 = lambda k: torch.empty(k, dtype=torch.int64, device=dev)
    f64 = lambda k: torch.empty(k, dtype=torch.float64, device=dev)
    keys, rec = i64((2, np_)), torch.empty((2, np_, 4), dtype=torch.float32, device=dev)
    counts = torch.zeros(4, dtype=torch.int64, device=dev)
    tmp = torch.empty(max(hp.sort_temp_bytes(np_), hp.scan_temp_bytes(np_ + 1)), dtype=torch.uint8, device=dev)
    perm, cell_of, parent, least, root = (i32(np_) for _ in range(5))
    cell_start, item_start, scan, cell_key = i32(np_ + 1), i32(np_ + 1), i64(np_ + 1), i64(np_)
    bufs = [keys[0].data_ptr(), keys[1].data_ptr(), perm.data_ptr(), rec[0].data_ptr(), rec[1].data_ptr(),
            scan.data_ptr(), cell_of.data_ptr(), cell_start.data_ptr(), cell_key.data_ptr(), parent.data_ptr(),
            least.data_ptr(), root.data_ptr(), item_start.data_ptr(), counts.data_ptr(), tmp.data_ptr(), tmp.numel()]
    xyz_sorted = f64((3, np_))
    w_sorted = f64(np_) if ws is not None else None
    v_sorted = torch.empty((np_, 4), dtype=torch.float32, device=dev) if vs is not None else None
    sorted_ = [xyz_sorted[0].data_ptr(), xyz_sorted[1].data_ptr(), xyz_sorted[2].data_ptr(), ptr(w_sorted),
               ptr(v_sorted)]
    hp.pair_prepare(np_, xs.data_ptr(), ys.data_ptr(), zs.data_ptr(), sel_ptr, barr, edges[-1], ext, bufs, w_ptr,
                    *v_ptr, sorted_, s())
    ns, ncells, nitems, bound = counts.tolist()  # the second host read: sizes the pair kernel's grid, and the bound
    if bound > MAX_PAIRS_BOUND:
        raise ValueError(f"pair_statistics: {bound} candidate pairs, more than 2^38; subsample the particles with "
                         f"select")
    q = hp.pair_run(np_, ns, ncells, nitems, bound, barr, edges, ext, channels, W, vrange, bufs, sorted_, _variant,
                    0 if stats is None else stats.data_ptr(), out.data_ptr(), s())
    _lib.raise_on_device_check("pair_statistics")
    return result(q, bound)


def structure_functions(stats):
    """velocity structure functions of the bins of a ``pair_statistics`` result with velocities: dict of
    S1L = dl1 / count, S2L = dl2 / count, S3L = dl3 / count (longitudinal), S2T = (dv2 - dl2) / (2 count) (one
    transverse component) and S2 = dv2 / count; NaN where count == 0"""
    if "dv2" not in stats:
        raise ValueError("structure_functions: the statistics hold no velocity channels")
    cnt = stats["count"].to(torch.float64)
    cnt = torch.where(cnt > 0, cnt, torch.full_like(cnt, math.nan))
    return dict(S1L=stats["dl1"] / cnt, S2L=stats["dl2"] / cnt, S3L=stats["dl3"] / cnt,
                S2T=(stats["dv2"] - stats["dl2"]) / (2.0 * cnt), S2=stats["dv2"] / cnt)


def correlation_function(stats, edges, n, box):
    """two-point correlation function of ``n`` particles in a fully periodic box: xi_k = count_k / RR_k - 1 with the
    expected pair count of a uniform distribution RR_k = n (n - 1) / 2 * 4 pi (e_{k+1}^3 - e_k^3) / (3 V)"""
    if any(bc != 1 for bc in box.bc):
        raise ValueError("correlation_function: defined for a fully periodic box only (no random catalogues here)")
    e = torch.as_tensor(edges, dtype=torch.float64, device=stats["count"].device)
    lx, ly, lz = box.lengths()
    rr = 0.5 * n * (n - 1) * 4.0 * math.pi * (e[1:] ** 3 - e[:-1] ** 3) / (3.0 * lx * ly * lz)
    return stats["count"].to(torch.float64) / rr - 1.0
