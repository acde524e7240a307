"""Radial profiles and spherical-overdensity (SO) masses about many centres at once.

Inputs: ``centres`` (C, 3) float64 (wrapped into the box on periodic axes), fp64 coordinates ``x, y, z``, masses ``m``,
the simulation ``box``, ``edges``: nb + 1 ascending radii e_0 < ... < e_nb with 1 <= nb <= 64 and e_0 >= 0 (r_max =
e_nb), optional velocities ``v = (vx, vy, vz)`` with optional centre velocities ``vc`` (C, 3), optional ``u``, up to 8
absolute density ``thresholds`` rho_t (the caller forms Delta * rho_ref), an optional bool mask ``select`` and a particle
range [first, last); the last three behave as in ``fof_labels``.

d = minimg(r_j - c) in fp64, d2 = (dx*dx + dy*dy) + dz*dz, and the *key* of a (centre, particle) pair is k =
float32(d2). With E_i = float32(e_i * e_i) the pair is a hit iff k < E_nb and lies in bin i iff E_i <= k < E_{i+1};
hits below E_0 are in no bin but count for the SO search. Everything is decided on keys, so the host path, the device
path and a dense numpy evaluation agree bit for bit on membership. Per (centre, bin), with w = v - vc and
w_r = (w . d) / sqrt(d2) (0 at d2 == 0):

    count            hits (int64, exact)                  always
    mass             sum m                                always
    mvr, mvr2, mv2   sum m w_r, sum m w_r^2, sum m w.w    with v
    mu               sum m u                              with u

Spherical overdensity, per (centre, threshold): the hits of a centre are ordered by key, ties in the order of the sorted
hit list; a tie run is a maximal run of equal keys. With M_q the mass of all hits up to and including the end q of a tie
run and r_q = sqrt(float64(k_q)), the crossing is the *outermost* tie-run end with M_q >= (4 pi / 3) rho_t r_q^3.
Returned are ``so_radius`` = r_q, ``so_mass`` = M_q, ``so_count`` = the hits up to q and ``so_truncated`` = (q is the
centre's last hit: the sphere may continue past r_max). No crossing: NaN, NaN, 0. This is the outermost crossing within
r_max; the first down-crossing of the enclosed density (what a profile with substructure outside the halo may want) is
not computed here.

Geometry: the cells of ``pair_statistics`` (edges of at least r_max, 27-cell stencil): a periodic axis needs
r_max <= L / 3 (less the 2^-20, as there), otherwise ValueError. At most 2^30 particles, 2^24 centres and 2^31 - 1 hits. A centre whose stencil
holds nothing (a centre outside the particles' extent on an open axis included) gets zeros and NaN.

Device tensors run csrc/hip/profiles.hip (a streaming hit filter, a sort of the hit keys, segment sums; hits and
segments are cut every SPHX_PROFILE_SEGMENT entries, default 4096, a multiple of 64), host tensors
csrc/cpu/profiles_cpu.cpp (OpenMP); both use the arithmetic of sphx/profiles.hpp. All sums have a fixed order: the
results are bit-identical from run to run. Hits are local to the caller's particles: nothing crosses ranks.
"""

from __future__ import annotations

import math
import os

import torch

from . import _lib
from .fof import MAX_PARTICLES, _coords
from .reduce import min_max

MAX_BINS = 64
MAX_THRESHOLDS = 8
MAX_CENTRES = 1 << 24
MAX_HITS = (1 << 31) - 1
SEGMENT = 4096  # sorted positions per hit item and sorted hits per reduction segment; SPHX_PROFILE_SEGMENT overrides
SLOTS = 18  # per centre: 9 stencil rows, each in up to two pieces (profiles.hpp kProfileSlots)
_stats = None  # measurements only: a zeroed int64 device tensor of 3 counters that the hit kernel's count pass adds to
               # (candidates tested, evaluated in fp64, hits); no result depends on it


def radial_profiles(centres, x, y, z, m, box, edges, v=None, u=None, vc=None, thresholds=None, select=None, first=0,
                    last=None):
    """dict of ``count`` (C, nb) int64, ``mass`` and the channels that ``v`` and ``u`` bring (each (C, nb) float64),
    ``so_radius``, ``so_mass`` (C, T) float64, ``so_count`` (C, T) int64, ``so_truncated`` (C, T) bool and ``hits``
    (C,) int64 for the particles [first, last); see the module's docstring"""
    n = x.numel()
    last = n if last is None else int(last)
    first = int(first)
    _coords("radial_profiles", x, y, z, n)
    if not 0 <= first <= last <= n:
        raise ValueError("radial_profiles: [first, last) outside the particle range")
    dev = x.device
    edges = torch.as_tensor(edges, dtype=None if hasattr(edges, "dtype") else torch.float64)
    if edges.dtype != torch.float64 or edges.dim() != 1:
        raise ValueError("radial_profiles: edges must be a one-dimensional float64 tensor or array")
    edges = edges.tolist()
    nb = len(edges) - 1
    if not 1 <= nb <= MAX_BINS:
        raise ValueError(f"radial_profiles: between 1 and {MAX_BINS} bins, not {nb}")
    if not edges[0] >= 0.0 or not all(a < b for a, b in zip(edges, edges[1:])) or not edges[-1] < math.inf:
        raise ValueError("radial_profiles: the edges must be finite, ascending and not negative")
    rho = [] if thresholds is None else [float(t) for t in thresholds]
    if len(rho) > MAX_THRESHOLDS or not all(t > 0.0 and t < math.inf for t in rho):
        raise ValueError(f"radial_profiles: at most {MAX_THRESHOLDS} thresholds, each positive and finite")
    nt = len(rho)
    if not torch.is_tensor(centres) or centres.dtype != torch.float64 or centres.dim() != 2 or \
            centres.shape[1] != 3 or centres.device != dev:
        raise ValueError(f"radial_profiles: centres must be a (C, 3) float64 tensor on {dev}")
    C = centres.shape[0]
    if C > MAX_CENTRES:
        raise ValueError(f"radial_profiles: more than 2^24 centres ({C})")
    if vc is not None and (v is None or not torch.is_tensor(vc) or vc.shape != (C, 3) or vc.device != dev):
        raise ValueError(f"radial_profiles: vc needs v and must be a ({C}, 3) tensor on {dev}")
    np_ = last - first
    if np_ > MAX_PARTICLES:
        raise ValueError(f"radial_profiles: more than 2^30 particles ({np_})")
    if select is not None:
        if select.dtype != torch.bool or select.shape != (n,) or select.device != dev:
            raise ValueError(f"radial_profiles: select must be a bool tensor of shape ({n},) on {dev}")
        select = select.contiguous()[first:last]
    fields = [m] + (list(v) if v is not None else []) + ([u] if u is not None else [])
    if (v is not None and len(v) != 3) or any(
            not torch.is_tensor(t) or not t.is_floating_point() or t.shape != (n,) or t.device != dev for t in fields):
        raise ValueError(f"radial_profiles: m, v = (vx, vy, vz) and u must be floating-point tensors of shape ({n},) "
                         f"on {dev}")
    seg = int(os.environ.get("SPHX_PROFILE_SEGMENT", SEGMENT))
    if seg < 64 or seg % 64:
        raise ValueError("SPHX_PROFILE_SEGMENT must be a positive multiple of 64")
    lo, L = box.lo, box.lengths()
    for a in range(3):
        # (makePairGrid's own condition: three cells of r_max (1 + 2^-20) must fit the axis)
        if box.bc[a] == 1 and not math.floor(L[a] / (edges[-1] * (1.0 + 2.0 ** -20))) >= 3:
            raise ValueError(f"radial_profiles: the periodic axis {a} ({L[a]}) is shorter than 3 cells of r_max = "
                             f"{edges[-1]} (r_max > L / 3, less the 2^-20)")

    count = torch.zeros((C, nb), dtype=torch.int64, device=dev)
    sums = torch.zeros((5, C, nb), dtype=torch.float64, device=dev)
    so_r = torch.full((C, nt), math.nan, dtype=torch.float64, device=dev)
    so_m = torch.full((C, nt), math.nan, dtype=torch.float64, device=dev)
    so_n = torch.zeros((C, nt), dtype=torch.int64, device=dev)
    so_t = torch.zeros((C, nt), dtype=torch.uint8, device=dev)
    hits = torch.zeros(C, dtype=torch.int64, device=dev)

    def result():
        res = dict(count=count, mass=sums[0])
        if v is not None:
            res.update(mvr=sums[1], mvr2=sums[2], mv2=sums[3])
        if u is not None:
            res["mu"] = sums[4]
        res.update(so_radius=so_r, so_mass=so_m, so_count=so_n, so_truncated=so_t.bool(), hits=hits)
        return res

    if np_ == 0 or C == 0:
        return result()
    cen = centres.clone()
    for a in range(3):
        if box.bc[a] == 1:  # (a centre inside the box keeps its bits)
            inside = (cen[:, a] >= lo[a]) & (cen[:, a] < lo[a] + L[a])
            cen[:, a] = torch.where(inside, cen[:, a], lo[a] + torch.remainder(cen[:, a] - lo[a], L[a]))
    cen = cen.contiguous()
    vcs = None if vc is None else vc.to(torch.float64).contiguous()
    xs, ys, zs = x[first:last], y[first:last], z[first:last]
    fs = [t[first:last].to(torch.float64).contiguous() for t in fields]
    ptr = lambda t: 0 if t is None else t.data_ptr()
    fptr = [fs[0].data_ptr()] + ([t.data_ptr() for t in fs[1:4]] if v is not None else [0, 0, 0]) + \
        [fs[-1].data_ptr() if u is not None else 0]
    # the grid of an open axis starts at the particles' smallest coordinate (a host read, as in pair_statistics)
    ext = [0.0] * 6 if all(bc == 1 for bc in box.bc) else min_max([xs, ys, zs]).tolist()
    barr = box.to_array()
    outs = [count.data_ptr(), sums.data_ptr(), so_r.data_ptr(), so_m.data_ptr(), so_n.data_ptr(), so_t.data_ptr(),
            hits.data_ptr()]
    if dev.type != "cuda":
        _lib.cpu().radial_profiles(C, cen.data_ptr(), ptr(vcs), np_, xs.data_ptr(), ys.data_ptr(), zs.data_ptr(),
                                   ptr(select), *fptr, barr, edges, ext, rho, *outs)
        return result()

    hp, s = _lib.hip(), _lib.stream
    i32 = lambda *k: torch.empty(k, dtype=torch.int32, device=dev)
    i64 = lambda *k: torch.empty(k, dtype=torch.int64, device=dev)
    f64 = lambda *k: torch.empty(k, dtype=torch.float64, device=dev)
    u8 = lambda k: torch.empty(k, dtype=torch.uint8, device=dev)
    # 1. the preparation of pair_statistics, unchanged: cells, sorted records, sorted fp64 coordinates
    keys, rec = i64(2, np_), torch.empty((2, np_, 4), dtype=torch.float32, device=dev)
    counts = torch.zeros(4, dtype=torch.int64, device=dev)
    nslots = C * SLOTS
    tmp = u8(max(hp.sort_temp_bytes(np_), hp.scan_temp_bytes(max(np_, nslots) + 1)))
    perm, cell_of, parent, least, root = (i32(np_) for _ in range(5))
    cell_start, item_start, scan, cell_key = i32(np_ + 1), i32(np_ + 1), i64(np_ + 1), i64(np_)
    bufs = [keys[0].data_ptr(), keys[1].data_ptr(), perm.data_ptr(), rec[0].data_ptr(), rec[1].data_ptr(),
            scan.data_ptr(), cell_of.data_ptr(), cell_start.data_ptr(), cell_key.data_ptr(), parent.data_ptr(),
            least.data_ptr(), root.data_ptr(), item_start.data_ptr(), counts.data_ptr(), tmp.data_ptr(), tmp.numel()]
    xyz_sorted = f64(3, np_)
    sorted_ = [xyz_sorted[0].data_ptr(), xyz_sorted[1].data_ptr(), xyz_sorted[2].data_ptr(), 0, 0]
    hp.pair_prepare(np_, xs.data_ptr(), ys.data_ptr(), zs.data_ptr(), ptr(select), barr, edges[-1], ext, bufs, 0, 0, 0,
                    0, sorted_, s())
    crec, slot_range, item_off = i32(C, 6), i32(2, nslots), i64(nslots + 1)
    pbufs = [crec.data_ptr(), slot_range[0].data_ptr(), slot_range[1].data_ptr(), item_off.data_ptr(), tmp.data_ptr(),
             tmp.numel()]
    hp.profile_plan(C, np_, cen.data_ptr(), barr, edges[-1], ext, seg, bufs, pbufs, s())
    # the preparation's host read, with the item count riding along
    ns, _, _, _, n_items = torch.cat([counts, item_off[-1:]]).tolist()
    if ns == 0 or n_items == 0:
        return result()
    # 2. the hit kernel: count pass, scan, the read that sizes the write pass, write pass
    item_hits = i64(n_items + 1)
    tmp2 = tmp  # (the preparation's workspace stays alive under its own name: bufs points into it)
    if hp.scan_temp_bytes(n_items + 1) > tmp2.numel():
        tmp2 = u8(hp.scan_temp_bytes(n_items + 1))
        pbufs[4:] = [tmp2.data_ptr(), tmp2.numel()]
    hit_args = (C, ns, n_items)
    tail = (cen.data_ptr(), barr, edges, ext, seg, bufs, sorted_, pbufs, item_hits.data_ptr())
    hp.profile_hits(False, *hit_args, 0, *tail, 0, 0, 0 if _stats is None else _stats.data_ptr(), s())
    H = int(item_hits[-1])
    if H > MAX_HITS:
        raise ValueError(f"radial_profiles: {H} hits, more than 2^31 - 1; use fewer centres per call or a smaller "
                         f"r_max")
    if H == 0:
        return result()
    hkeys, pidx, hperm = i64(2, H), i32(H), i32(H)
    hp.profile_hits(True, *hit_args, H, *tail, hkeys[0].data_ptr(), pidx.data_ptr(), 0, s())
    # 3. the sort of the hit keys (stable: ties keep the emission order)
    need = max(hp.sort_temp_bytes(H), hp.scan_temp_bytes(C + 1))
    tmp3 = tmp2 if need <= tmp2.numel() else u8(need)
    hp.sort_keys(H, hkeys[0].data_ptr(), hkeys[1].data_ptr(), hperm.data_ptr(), tmp3.data_ptr(), tmp3.numel(), s())
    # 4. starts, segment sums, combination, crossings
    U = hp.profile_max_segments(C, H, seg)
    start, seg_off = i64(C + 1), i64(C + 1)
    partial, seg_mass, carry, hmass = f64(U, 6 * nb), f64(U), f64(U), f64(H)
    seg_q, seg_m = i64(U, MAX_THRESHOLDS), f64(U, MAX_THRESHOLDS)
    work = [start.data_ptr(), seg_off.data_ptr(), partial.data_ptr(), seg_mass.data_ptr(), carry.data_ptr(),
            hmass.data_ptr(), seg_q.data_ptr(), seg_m.data_ptr()]
    hp.profile_reduce(C, H, np_, ns, barr, edges, ext, rho, seg, hkeys[1].data_ptr(), hperm.data_ptr(),
                      pidx.data_ptr(), perm.data_ptr(), sorted_, fptr, cen.data_ptr(), ptr(vcs), work, outs,
                      tmp3.data_ptr(), tmp3.numel(), s())
    _lib.raise_on_device_check("radial_profiles")
    return result()


def profile_quantities(result, edges):
    """profiles of the bins of a ``radial_profiles`` result: dict of ``r`` (the bins' mid radii), ``density`` =
    mass / V_shell, and, with velocities, ``vr`` = mvr / mass (mean radial velocity), ``sigma_r`` =
    sqrt(mvr2 / mass - vr^2) and ``sigma`` = sqrt(mv2 / mass) (radial and total dispersion about the centre's velocity),
    with ``u``, ``u`` = mu / mass (mass-weighted); NaN where a bin's count is 0"""
    mass = result["mass"]
    e = torch.as_tensor(edges, dtype=torch.float64, device=mass.device)
    shell = 4.0 * math.pi / 3.0 * (e[1:] ** 3 - e[:-1] ** 3)
    nan = torch.full_like(mass, math.nan)
    msafe = torch.where(result["count"] > 0, mass, nan)
    out = dict(r=0.5 * (e[1:] + e[:-1]), density=msafe / shell)
    if "mvr" in result:
        vr = result["mvr"] / msafe
        out.update(vr=vr, sigma_r=torch.sqrt(torch.clamp(result["mvr2"] / msafe - vr * vr, min=0.0)),
                   sigma=torch.sqrt(result["mv2"] / msafe))
    if "mu" in result:
        out["u"] = result["mu"] / msafe
    return out
