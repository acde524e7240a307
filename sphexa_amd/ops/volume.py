"""SPH interpolation of particle fields onto regular 3-D grids.

    V_c(p) = sum_j w_jc W_n(|r_p - r_j|, h_eff_j),    h_eff = max(h, h_floor * largest voxel edge)

for the voxel centres p = lo + (k + 0.5) d of a window (default: the box), W_n the normalised 3-D sinc^n kernel
(support 2h). Periodic dimensions contribute their images -1, 0, +1 per axis. The kernels only sum; ratios (field
averages) are formed by the caller from several channels (app/simulation.py Simulation.volume, power_spectrum).

Device tensors run csrc/hip/volume.hip (brick-binned, bit-reproducible), host tensors csrc/cpu/volume_cpu.cpp (fp64).
"""

from __future__ import annotations

import os

import torch

from . import _lib
from .image import kernel_norm

BRICK = 8  # voxels per brick edge (volume.hip kBrick)
SEGMENT = 4096  # entries per (brick, segment) block; SPHX_VOLUME_SEGMENT overrides. A/B over 1024 / 4096 / 16384:
# profiles/r14/volume/README.md (1024 slower, 16384 equal)
MAX_PARTICLES = 1 << 30  # key layout: brick << 35 | particle << 5 | shift code
MAX_BRICKS = (1 << 29) - 1  # the ranges kernel looks up brick count << 35, and the padding key is all ones
MAX_ENTRIES = (1 << 31) - 1  # the sample sort's element limit


def sph_volume(x, y, z, h, weights, box, res=(128, 128, 128), window=None, h_floor=0.5, first=0, last=None,
               sinc_index=6.0, out_dtype=torch.float32):
    """volume of the particles [first, last): ``weights`` (C, n) float32 with C = 1, 2 or 4, result (C, nz, ny, nx) on
    the inputs' device. ``res`` = (nx, ny, nz), ``window`` = (lo3, hi3) (default: the box), ``h_floor`` in voxels of the
    largest edge (0: off). ``out_dtype`` float64 is served by the host path only (which accumulates in fp64 anyway)"""
    n = x.numel()
    last = n if last is None else int(last)
    first = int(first)
    C = int(weights.shape[0])
    if C not in (1, 2, 4) or weights.shape[1] != n or weights.dtype != torch.float32:
        raise ValueError("sph_volume: weights must be float32 of shape (1, 2 or 4, n)")
    if not 0 <= first <= last <= n:
        raise ValueError("sph_volume: [first, last) outside the particle range")
    for name, t, dt in (("x", x, torch.float64), ("y", y, torch.float64), ("z", z, torch.float64),
                        ("h", h, torch.float32)):
        # (the native code reads raw pointers)
        if t.dtype != dt or t.shape != (n,) or not t.is_contiguous() or t.device != x.device:
            raise ValueError(f"sph_volume: {name} must be a contiguous {dt} tensor of shape ({n},) on {x.device}")
    if weights.device != x.device:
        raise ValueError(f"sph_volume: weights must be on {x.device}")
    lo, hi = (box.lo, box.hi) if window is None else window
    lo, hi = [float(v) for v in lo], [float(v) for v in hi]
    res = [int(r) for r in res]
    if len(res) != 3 or len(lo) != 3 or len(hi) != 3 or min(res) < 1 or not all(b > a for a, b in zip(lo, hi)):
        raise ValueError("sph_volume: empty window or resolution")
    nx, ny, nz = res
    weights = weights.contiguous()
    view = [*lo, *hi, float(h_floor), float(sinc_index), kernel_norm(sinc_index)]
    if x.device.type != "cuda":
        out = torch.zeros((C, nz, ny, nx), dtype=torch.float64)
        _lib.cpu().sph_volume(first, last, n, x.data_ptr(), y.data_ptr(), z.data_ptr(), h.data_ptr(),
                              weights.data_ptr(), C, box.to_array(), view, res, out.data_ptr())
        return out.to(out_dtype)
    if out_dtype != torch.float32:
        raise ValueError("sph_volume: the device path returns float32")
    return _volume_hip(x, y, z, h, weights, box, view, first, last, n, C, res)


def _volume_hip(x, y, z, h, weights, box, view, first, last, n, C, res):
    hp, dev, s = _lib.hip(), x.device, _lib.stream
    np_ = last - first
    nx, ny, nz = res
    segment = int(os.environ.get("SPHX_VOLUME_SEGMENT", SEGMENT))
    if segment < 1:
        raise ValueError("SPHX_VOLUME_SEGMENT must be positive")
    nbricks = -(-nx // BRICK) * -(-ny // BRICK) * -(-nz // BRICK)
    if np_ > MAX_PARTICLES:
        raise ValueError(f"sph_volume: more than 2^30 particles ({np_}) do not fit the entry keys")
    if nbricks > MAX_BRICKS:
        raise ValueError(f"sph_volume: 2^29 bricks or more ({nbricks}) do not fit the entry keys")
    vol = torch.empty((C, nz, ny, nx), dtype=torch.float32, device=dev)
    rec = torch.empty((max(np_, 1), 8), dtype=torch.float32, device=dev)
    counts = torch.empty(np_ + 1, dtype=torch.int64, device=dev)
    barr = box.to_array()
    hp.volume_records(first, last, n, x.data_ptr(), y.data_ptr(), z.data_ptr(), h.data_ptr(), weights.data_ptr(), C,
                      barr, view, res, rec.data_ptr(), counts.data_ptr(), s())
    tmp = torch.empty(hp.scan_temp_bytes(max(np_, nbricks) + 1), dtype=torch.uint8, device=dev)
    hp.exclusive_scan_i64(counts.data_ptr(), counts.data_ptr(), np_ + 1, tmp.data_ptr(), tmp.numel(), s())
    total = int(counts[np_])  # the one host synchronisation: sizes the entry buffers
    if total > MAX_ENTRIES:
        raise ValueError(f"sph_volume: {total} (particle, brick) entries exceed 2^31 - 1; lower the resolution or "
                         "bin the particle range in parts")
    keys = torch.empty((2, max(total, 1)), dtype=torch.int64, device=dev)
    if total:
        perm = torch.empty(total, dtype=torch.int32, device=dev)
        hp.volume_fill(np_, barr, view, res, rec.data_ptr(), counts.data_ptr(), keys[0].data_ptr(), s())
        stmp = torch.empty(hp.sort_temp_bytes(total), dtype=torch.uint8, device=dev)
        hp.sort_keys(total, keys[0].data_ptr(), keys[1].data_ptr(), perm.data_ptr(), stmp.data_ptr(), stmp.numel(),
                     s())
    # brick ranges in the sorted keys, then the (brick, segment) block list: at most total / segment + nbricks blocks
    start = torch.empty(nbricks + 1, dtype=torch.int64, device=dev)
    seg = torch.empty((2, nbricks + 1), dtype=torch.int64, device=dev)
    hp.volume_ranges(total, keys[1].data_ptr(), nbricks, segment, start.data_ptr(), seg[0].data_ptr(),
                     seg[1].data_ptr(), s())
    for row in seg:
        hp.exclusive_scan_i64(row.data_ptr(), row.data_ptr(), nbricks + 1, tmp.data_ptr(), tmp.numel(), s())
    nblocks = total // segment + nbricks
    # partial bricks are written by bricks of several segments only; a brick of k > 1 segments holds more than
    # (k - 1) * segment entries, so there are at most 2 total / segment of them
    nwork = 2 * (total // segment)
    work = torch.empty((max(nwork, 1), C, BRICK ** 3), dtype=torch.float32, device=dev)
    hp.volume_bricks(C, np_, total, keys[1].data_ptr(), rec.data_ptr(), barr, view, res, nbricks, segment, nblocks,
                     start.data_ptr(), seg[0].data_ptr(), seg[1].data_ptr(), nwork, work.data_ptr(), vol.data_ptr(),
                     s())
    _lib.raise_on_device_check("sph_volume")
    return vol
