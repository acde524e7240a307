"""Shell-binned power spectrum of a field on a cubic grid.

With u^ = FFT(u) / N^3 and integer wave vectors k (components in [-N/2, N/2)), shell b = floor(|k| + 0.5):

    P[b] = sum_{k in shell b} sum_c |u^_c(k)|^2        count[b] = number of modes in shell b

so that sum_b P[b] = mean(sum_c u_c^2) (Parseval) and sum_b count[b] = N^3. The transform is torch.fft.rfftn (hipFFT
on the device); the half spectrum's modes count twice except in the planes kx = 0 and (even N) kx = N/2, which are
their own mirror images. Device tensors bin with csrc/hip/volume.hip spectrumShellsKernel (fp64 sums, per-block LDS
bins; not bit-reproducible), host tensors with numpy in fp64.
"""

from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib


def num_shells(N: int) -> int:
    """shells that the modes of an N^3 grid reach: the corner (N // 2)(1, 1, 1) lies in the last one"""
    return int(math.floor(math.sqrt(3.0) * (N // 2) + 0.5)) + 1


def power_spectrum(grid):
    """(k = arange(nbins), P, count), all float64 on the grid's device, of ``grid`` (C, N, N, N)"""
    if grid.dim() != 4 or not (grid.shape[1] == grid.shape[2] == grid.shape[3]) or grid.shape[0] < 1:
        raise ValueError(f"power_spectrum: a cubic grid (C, N, N, N) is needed, got {tuple(grid.shape)}")
    C, N = int(grid.shape[0]), int(grid.shape[1])
    nbins = num_shells(N)
    spec = torch.fft.rfftn(grid, dim=(1, 2, 3))
    if grid.device.type != "cuda":
        f = spec.to(torch.complex128).numpy()
        p = (f.real ** 2 + f.imag ** 2).sum(axis=0) / float(N) ** 6
        k1 = np.fft.fftfreq(N, 1.0 / N)
        kx = np.arange(N // 2 + 1, dtype=np.float64)
        k2 = k1[:, None, None] ** 2 + k1[None, :, None] ** 2 + kx[None, None, :] ** 2
        b = np.floor(np.sqrt(k2) + 0.5).astype(np.int64)
        wgt = np.where((kx == 0) | (2 * kx == N), 1.0, 2.0)[None, None, :] * np.ones_like(k2)
        P = np.bincount(b.ravel(), weights=(wgt * p).ravel(), minlength=nbins)
        cnt = np.bincount(b.ravel(), weights=wgt.ravel(), minlength=nbins)
        return torch.arange(nbins, dtype=torch.float64), torch.from_numpy(P), torch.from_numpy(cnt)
    if grid.dtype != torch.float32:
        raise ValueError("power_spectrum: the device path takes float32 grids")
    hp = _lib.hip()
    spec = torch.view_as_real(spec.contiguous())  # (C, N, N, N/2 + 1, 2) float32
    partial = torch.empty((hp.spectrum_shell_blocks(N), 2 * nbins), dtype=torch.float64, device=grid.device)
    out = torch.empty((2, nbins), dtype=torch.float64, device=grid.device)
    hp.spectrum_shells(C, N, spec.data_ptr(), nbins, partial.data_ptr(), out.data_ptr(), _lib.stream())
    return torch.arange(nbins, dtype=torch.float64, device=grid.device), out[0], out[1]
