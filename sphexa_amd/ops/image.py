"""SPH slices, column projections and opacity renderings of particle fields as 2-D images.

    slice at s0:        I_c(p) = sum_j w_jc W_n(|r_p - r_j|, h_j)
    projection [s0,s1]: I_c(p) = sum_j w_jc h_j^-2 F_n(d_uv / h_j),  F_n(q) = 2 int_0^sqrt(4-q^2) W_n(sqrt(q^2+s^2), 1) ds

for the view axis a in {x, y, z}, the image plane (u, v) = the other two axes in cyclic order, pixels sampled at their
centres, W_n the normalised 3-D sinc^n kernel (support 2h). Periodic dimensions contribute their images in u, v and
the minimum image in a slice's depth offset. These two kinds only sum; ratios (field averages) are formed by the
caller from two channels (app/simulation.py Simulation.image).

    render [s0,s1]: window, pixels, h floor, periodic images and slab membership (by the particle's centre) as a
    projection. Every particle is composited as a whole at the depth r_a of its centre. The entries (particle j,
    periodic image) of a pixel with q^2 < 4 are ordered by ascending r_a (descending for the reversed views "-x",
    "-y", "-z", whose plane axes are those of the unsigned axis), ties by ascending particle index, then by ascending
    shift code 3 (sv + 1) + (su + 1), and from I = 0, T = 1 each one does

        tau = w_j0 h_j^-2 F_n(d_uv / h_j)    a = exp(-tau)    I += T (1 - a) w_j1    T *= a

    with channel 0 the opacity weight kappa_j m_j and channel 1 the source value s_j. The result is (2, nv, nu) =
    [I, T], [0, 1] where nothing reaches. A list cut into segments, each from (0, 1), combines in list order as
    I = I_1 + T_1 I_2, T = T_1 T_2. The order is part of the result: images of several ranks do not add.

Device tensors run csrc/hip/image.hip (tile-binned, bit-reproducible), host tensors csrc/cpu/image_cpu.cpp (fp64).
"""

from __future__ import annotations

import functools
import math
import os

import numpy as np
import torch

from ..utils.kernel_tables import SINC_N, kernel_fn
from . import _lib

TILE = 32  # pixels per tile edge (image.hip kTile)
# F_n table: samples in u = q^2/4 on [0, 1]. 16385 samples leave the interpolation error of the default sinc^6 kernel
# (3.94e-8) below the fp32 rounding of F_6(0) (0.87 * 2^-24 = 5.2e-8); profiles/r13/image/README.md lists n = 4, 9
TABLE_LENGTH = 16385  # image.hpp kImageTableLen
SEGMENT = 4096  # entries per (tile, segment) block; SPHX_IMAGE_SEGMENT overrides (profiles/r13/image/README.md)
MAX_PARTICLES = 1 << 30  # key layout: tile << 34 | particle << 4 | shift code
MAX_ENTRIES = (1 << 31) - 1  # the sample sort's element limit
_GL_NODES = 96


@functools.lru_cache(maxsize=8)
def kernel_norm(sinc_index: float) -> float:
    """3-D normalisation K of the sinc^n kernel (W = K sinc^n(pi q / 2) / h^3) by Gauss-Legendre quadrature (the
    simulation's Simpson value, utils/kernel_tables.kernel_3d_k, agrees to ~3e-11)"""
    t, wt = np.polynomial.legendre.leggauss(200)
    v = t + 1.0
    return 1.0 / float(np.sum(wt * 4.0 * math.pi * v * v * kernel_fn(SINC_N, float(sinc_index))(v)))


def projected_kernel(q, sinc_index: float = 6.0) -> np.ndarray:
    """F_n(q) in fp64 by Gauss-Legendre quadrature along the line of sight (h = 1)"""
    q = np.atleast_1d(np.asarray(q, dtype=np.float64))
    t, wt = np.polynomial.legendre.leggauss(_GL_NODES)
    smax = np.sqrt(np.maximum(4.0 - q * q, 0.0))
    s = 0.5 * smax[:, None] * (t[None, :] + 1.0)
    r = np.minimum(np.sqrt(q[:, None] ** 2 + s * s), 2.0)
    w = kernel_fn(SINC_N, float(sinc_index))(r)
    return kernel_norm(sinc_index) * smax * (w * wt[None, :]).sum(axis=1)


@functools.lru_cache(maxsize=8)
def projection_table(sinc_index: float = 6.0, length: int = TABLE_LENGTH):
    """(table, max_interp_error): F_n sampled at ``length`` points of u = q^2/4 in [0, 1] (fp64), and the largest
    |linear interpolation - F_n| over 15 interior points of every interval (the midpoint, where the error of a linear
    interpolant peaks, among them)"""
    u = np.linspace(0.0, 1.0, length)
    table = projected_kernel(2.0 * np.sqrt(u), sinc_index)
    table[-1] = 0.0
    frac = np.arange(1, 16) / 16.0
    uf = (u[:-1, None] + frac[None, :] * (u[1] - u[0])).ravel()
    lerp = (table[:-1, None] + frac[None, :] * (table[1:] - table[:-1])[:, None]).ravel()
    err = float(np.abs(lerp - projected_kernel(2.0 * np.sqrt(uf), sinc_index)).max())
    table.setflags(write=False)
    return table, err


KINDS = {"slice": 0, "projection": 1, "render": 2}  # the first element of the native view array


def _view(box, kind, axis, window, res, s0, s1):
    """(a, window, res, s0, s1); a rendering's reversed view "-x", "-y", "-z" comes back as a = -1, -2, -3"""
    reverse = kind == "render" and axis in ("-x", "-y", "-z")
    if (axis[1:] if reverse else axis) not in ("x", "y", "z"):
        raise ValueError(f"sph_image: unknown axis {axis!r} for kind {kind!r}")
    a = "xyz".index(axis[-1])
    iu, iv = (a + 1) % 3, (a + 2) % 3
    if window is None:
        window = (box.lo[iu], box.hi[iu], box.lo[iv], box.hi[iv])
    u0, u1, v0, v1 = (float(w) for w in window)
    nu, nv = (int(r) for r in res)
    if nu < 1 or nv < 1 or not (u1 > u0 and v1 > v0):
        raise ValueError("sph_image: empty window or resolution")
    if kind not in KINDS:
        raise ValueError(f"sph_image: unknown kind {kind!r}")
    if kind == "slice":
        s0 = 0.5 * (box.lo[a] + box.hi[a]) if s0 is None else float(s0)
        s1 = s0
    else:
        s0 = -math.inf if s0 is None else float(s0)
        s1 = math.inf if s1 is None else float(s1)
    return (-a - 1 if reverse else a), (u0, u1, v0, v1), (nu, nv), s0, s1


def sph_image(x, y, z, h, weights, box, kind="slice", axis="z", window=None, res=(512, 512), s0=None, s1=None,
              h_floor=0.5, first=0, last=None, sinc_index=6.0, out_dtype=torch.float32):
    """image of the particles [first, last): ``weights`` (C, n) float32 with C = 1 or 2, result (C, nv, nu) on the
    inputs' device. ``window`` = (u0, u1, v0, v1) (default: the box), ``h_floor`` in pixels (0: off). ``out_dtype``
    float64 is served by the host path only (which accumulates in fp64 anyway). ``kind="render"`` takes exactly the
    two rows (kappa m, source value), also the signed axes "-x", "-y", "-z", and returns [I, T]"""
    n = x.numel()
    last = n if last is None else int(last)
    first = int(first)
    C = int(weights.shape[0])
    if C not in (1, 2) or weights.shape[1] != n or weights.dtype != torch.float32:
        raise ValueError("sph_image: weights must be float32 of shape (1 or 2, n)")
    if not 0 <= first <= last <= n:
        raise ValueError("sph_image: [first, last) outside the particle range")
    a, win, (nu, nv), s0, s1 = _view(box, kind, axis, window, res, s0, s1)
    if kind == "render" and C != 2:
        raise ValueError("sph_image: a rendering takes two weight rows, kappa m and the source value")
    table, _ = projection_table(float(sinc_index), TABLE_LENGTH)
    weights = weights.contiguous()
    view = [float(KINDS[kind]), float(a), *win, s0, s1, float(h_floor), float(sinc_index), kernel_norm(sinc_index)]
    if x.device.type != "cuda":
        out = torch.zeros((C, nv, nu), dtype=torch.float64)
        tab = torch.from_numpy(np.array(table))
        _lib.cpu().sph_image(first, last, n, x.data_ptr(), y.data_ptr(), z.data_ptr(), h.data_ptr(),
                             weights.data_ptr(), C, box.to_array(), view, nu, nv, tab.data_ptr(), tab.numel(),
                             out.data_ptr())
        return out.to(out_dtype)
    if out_dtype != torch.float32:
        raise ValueError("sph_image: the device path returns float32")
    return _image_hip(x, y, z, h, weights, box, view, first, last, n, C, nu, nv, table)


def _image_hip(x, y, z, h, weights, box, view, first, last, n, C, nu, nv, table):
    hp, dev, s = _lib.hip(), x.device, _lib.stream
    np_ = last - first
    segment = int(os.environ.get("SPHX_IMAGE_SEGMENT", SEGMENT))
    if segment < 1:
        raise ValueError("SPHX_IMAGE_SEGMENT must be positive")
    ntiles = -(-nu // TILE) * -(-nv // TILE)
    if np_ > MAX_PARTICLES:
        raise ValueError(f"sph_image: more than 2^30 particles ({np_}) do not fit the entry keys")
    if ntiles > (1 << 30):
        raise ValueError("sph_image: more than 2^30 tiles")
    img = torch.empty((C, nv, nu), dtype=torch.float32, device=dev)
    tab = torch.from_numpy(np.array(table, dtype=np.float32)).to(dev)
    rec = torch.empty((max(np_, 1), 8), dtype=torch.float32, device=dev)
    counts = torch.empty(np_ + 1, dtype=torch.int64, device=dev)
    barr = box.to_array()
    render = view[0] == KINDS["render"]
    order = 0  # no permutation: record k is particle first + k
    if render and np_:
        # depth order: record k is the particle of depth rank k, so the entry keys below sort every tile's list front
        # to back (the sort is stable by (key, index): equal depths come out by particle index)
        dkeys = torch.empty((2, np_), dtype=torch.int64, device=dev)
        dperm = torch.empty(np_, dtype=torch.int32, device=dev)
        hp.image_depth_keys(first, last, x.data_ptr(), y.data_ptr(), z.data_ptr(), barr, view, nu, nv,
                            dkeys[0].data_ptr(), s())
        dtmp = torch.empty(hp.sort_temp_bytes(np_), dtype=torch.uint8, device=dev)
        hp.sort_keys(np_, dkeys[0].data_ptr(), dkeys[1].data_ptr(), dperm.data_ptr(), dtmp.data_ptr(), dtmp.numel(),
                     s())
        order = dperm.data_ptr()
    hp.image_records(first, last, n, x.data_ptr(), y.data_ptr(), z.data_ptr(), h.data_ptr(), weights.data_ptr(), C,
                     order, barr, view, nu, nv, rec.data_ptr(), counts.data_ptr(), s())
    tmp = torch.empty(hp.scan_temp_bytes(max(np_, ntiles) + 1), dtype=torch.uint8, device=dev)
    hp.exclusive_scan_i64(counts.data_ptr(), counts.data_ptr(), np_ + 1, tmp.data_ptr(), tmp.numel(), s())
    total = int(counts[np_])  # the one host synchronisation: sizes the entry buffers
    if total > MAX_ENTRIES:
        raise ValueError(f"sph_image: {total} (particle, tile) entries exceed 2^31 - 1; lower the resolution or "
                         "render the particle range in parts")
    keys = torch.empty((2, max(total, 1)), dtype=torch.int64, device=dev)
    if total:
        perm = torch.empty(total, dtype=torch.int32, device=dev)
        hp.image_fill(np_, barr, view, nu, nv, rec.data_ptr(), counts.data_ptr(), keys[0].data_ptr(), s())
        stmp = torch.empty(hp.sort_temp_bytes(total), dtype=torch.uint8, device=dev)
        hp.sort_keys(total, keys[0].data_ptr(), keys[1].data_ptr(), perm.data_ptr(), stmp.data_ptr(), stmp.numel(),
                     s())
    # tile ranges in the sorted keys, then the (tile, segment) block list: at most total / segment + ntiles blocks
    start = torch.empty(ntiles + 1, dtype=torch.int64, device=dev)
    seg = torch.empty(ntiles + 1, dtype=torch.int64, device=dev)
    hp.image_ranges(total, keys[1].data_ptr(), ntiles, segment, start.data_ptr(), seg.data_ptr(), s())
    hp.exclusive_scan_i64(seg.data_ptr(), seg.data_ptr(), ntiles + 1, tmp.data_ptr(), tmp.numel(), s())
    nblocks = total // segment + ntiles
    work = torch.empty((nblocks, C, TILE * TILE), dtype=torch.float32, device=dev)
    if render:  # partial tiles are (I_s, T_s), composed in segment order
        hp.image_render(np_, total, keys[1].data_ptr(), rec.data_ptr(), barr, view, nu, nv, ntiles, segment, nblocks,
                        start.data_ptr(), seg.data_ptr(), tab.data_ptr(), tab.numel(), work.data_ptr(),
                        img.data_ptr(), s())
    else:
        hp.image_tiles(int(view[0]), C, np_, total, keys[1].data_ptr(), rec.data_ptr(), barr, view, nu, nv, ntiles,
                       segment, nblocks, start.data_ptr(), seg.data_ptr(), tab.data_ptr(), tab.numel(),
                       work.data_ptr(), img.data_ptr(), s())
    _lib.raise_on_device_check("sph_image")
    return img
