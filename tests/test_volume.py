"""SPH volumes (ops/volume.py) against a dense all-pairs fp64 sum, and shell-binned power spectra (ops/spectrum.py).

Bound per voxel and channel: |got - ref64| <= 4 eps S, with S the sum of the magnitudes of the voxel's terms and eps
the error of the same numpy sum run in float32 on inputs rounded as the records round them (relative to S, largest over
the voxels; 64 * 2^-53 for the fp64 host path). The margin of 4 covers the kernel's different but fixed summation order
and its sinc evaluation. Measured ratios: profiles/r14/volume/README.md.
"""

import math

import numpy as np
import pytest
import torch

from sphexa_amd.ops.spectrum import power_spectrum
from sphexa_amd.ops.volume import sph_volume
from sphexa_amd.utils.box import OPEN, PERIODIC, Box

from mp_util import run_ranks

N_SINC = 6.0
_GL = np.polynomial.legendre.leggauss(200)
KERNEL_K = 1.0 / np.sum(_GL[1] * 4 * math.pi * (_GL[0] + 1.0) ** 2 * np.sinc((_GL[0] + 1.0) / 2) ** N_SINC)


def ref(x, y, z, h, w, box, res, window=None, h_floor=0.5, dtype=np.float64):
    """(volume, S), each (C, nz, ny, nx): every voxel x every particle x the 27 periodic images, 1024 voxels at a time"""
    lo, hi = window or (box.lo, box.hi)
    L, (nx, ny, nz) = box.lengths(), res
    d = [(hi[a] - lo[a]) / res[a] for a in range(3)]
    ih = (1.0 / np.maximum(h.astype(np.float64), h_floor * max(d))).astype(dtype)
    c = [((np.asarray(p, np.float64) - lo[a]) / d[a]).astype(dtype) for a, p in enumerate((x, y, z))]
    kz, ky, kx = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    g = [k.ravel().astype(dtype) + dtype(0.5) for k in (kx, ky, kz)]
    wd = w.astype(dtype)
    out = np.zeros((2, w.shape[0], nz * ny * nx), dtype)
    sh = [(-1, 0, 1) if box.bc[a] == PERIODIC else (0,) for a in range(3)]
    sep = lambda a, s, sl: (g[a][sl, None] - (c[a] + dtype(s * L[a] / d[a]))[None, :]) * (dtype(d[a]) * ih)[None, :]
    for v0 in range(0, nz * ny * nx, 1024):
        sl = slice(v0, v0 + 1024)
        for sz in sh[2]:
            dw = sep(2, sz, sl)
            for sy in sh[1]:
                dv = sep(1, sy, sl)
                for sx in sh[0]:
                    du = sep(0, sx, sl)
                    q2 = du * du + dv * dv + dw * dw
                    p, j = np.nonzero(q2 < 4)
                    val = dtype(KERNEL_K) * np.sinc(np.sqrt(q2[p, j]) / dtype(2)) ** dtype(N_SINC) * ih[j] ** 3
                    for ch in range(w.shape[0]):
                        np.add.at(out[0, ch], v0 + p, wd[ch, j] * val)
                        np.add.at(out[1, ch], v0 + p, np.abs(wd[ch, j] * val))
    return out.reshape(2, w.shape[0], nz, ny, nx)


def _row(name):
    rng = np.random.default_rng(11)
    if name == "one":  # partial bricks on every axis, a ball over several sub-bricks
        return dict(x=np.array([0.52]), y=np.array([0.47]), z=np.array([0.45]), h=np.array([0.3], np.float32),
                    w=np.array([[1.5]], np.float32), box=Box.cube(0, 1, OPEN), res=(9, 10, 11))
    if name == "batch":  # one more than a 512-entry staging batch; footprints wrap on all axes (2h < L/2)
        x, y, z = rng.random((3, 513))
        return dict(x=x, y=y, z=z, h=np.full(513, 0.2, np.float32), w=np.full((1, 513), 1 / 513, np.float32),
                    box=Box.cube(0, 1, PERIODIC), res=(16, 16, 16))
    if name.startswith("contrast"):
        x, y, z = rng.random((3, 2000))
        h = (0.0025 * 40 ** rng.random(2000)).astype(np.float32)  # voxel: 0.015 x 0.0167 x 0.0143
        x[0], y[0], z[0], h[0] = 0.7, 0.25, 0.5, 1.0  # reaches every brick
        m = (1e-3 * 10 ** rng.random(2000)).astype(np.float32)
        w = np.stack([m * (1 + x).astype(np.float32), m * (1 + y).astype(np.float32), m * (z - 0.5).astype(np.float32), m])
        return dict(x=x, y=y, z=z, h=h, w=w, box=Box.cube(0, 1, OPEN), res=(20, 12, 28),
                    window=((0.55, 0.15, 0.3), (0.85, 0.35, 0.7)), h_floor=0.0 if name == "contrast0" else 0.5)
    a = "xyz".index(name[-1])  # axes-x, axes-y, axes-z: periodic in the named axis only
    x, y, z = rng.random((3, 300))
    box = Box([0.0] * 3, [1.0] * 3, [PERIODIC if d == a else OPEN for d in range(3)])
    return dict(x=x, y=y, z=z, h=np.full(300, 0.1, np.float32), w=rng.random((2, 300)).astype(np.float32), box=box,
                res=(12, 12, 12))


ROWS = ["one", "batch", "contrast", "contrast0", "axes-x", "axes-y", "axes-z"]
_refs = {}


def _case(name):
    """the row's inputs and call arguments, its fp64 reference and the eps of the float32 twin (computed once)"""
    if name not in _refs:
        r = _row(name)
        kw = {k: v for k, v in r.items() if k in ("window", "res", "h_floor")}
        args = (r["x"], r["y"], r["z"], r["h"], r["w"], r["box"])
        r64, S = ref(*args, **kw)
        r32 = ref(*args, **kw, dtype=np.float32)[0]
        _refs[name] = (r, kw, r64, S, float((np.abs(r32 - r64)[S > 0] / S[S > 0]).max()))
    return _refs[name]


def _render(r, kw, device, dtype):
    t = lambda a, dt: torch.as_tensor(a, dtype=dt).to(device)
    return sph_volume(t(r["x"], torch.float64), t(r["y"], torch.float64), t(r["z"], torch.float64),
                      t(r["h"], torch.float32), t(r["w"], torch.float32), r["box"], sinc_index=N_SINC, out_dtype=dtype,
                      **kw)


def _check(tag, got, r64, S, eps):
    bound = 4 * eps * S
    err = np.abs(got.double().cpu().numpy() - r64)
    ratio = float((err[bound > 0] / bound[bound > 0]).max())
    print(f"{tag}: eps {eps:.3e} max |got - ref| / bound {ratio:.4f}")
    assert got.shape == r64.shape and np.isfinite(err).all()
    assert (err <= bound).all(), f"{tag}: ratio {ratio}"


@pytest.mark.parametrize("name", ROWS)
def test_cpu_rows(name):
    r, kw, r64, S, _ = _case(name)
    _check(f"cpu {name}", _render(r, kw, "cpu", torch.float64), r64, S, 64 * 2.0 ** -53)


# forced segment lengths: the issue's row (contrast, 64; its longest brick list is 40 entries, so it stays whole), the
# contrast set at 16 (bricks of 16 to 40 entries: one to three segments side by side) and the batch set at 64 (every
# brick holds at least 513 entries: nine segments and more)
SEGMENTS = {"segments": ("contrast", 64), "segments-16": ("contrast", 16), "segments-batch": ("batch", 64)}


@pytest.mark.gpu
@pytest.mark.parametrize("name", ROWS + list(SEGMENTS))
def test_gpu_rows(name, monkeypatch):
    row, forced = SEGMENTS.get(name, (name, None))  # forced: partial bricks and their ordered sum
    r, kw, r64, S, eps = _case(row)
    if forced:
        monkeypatch.setenv("SPHX_VOLUME_SEGMENT", str(forced))
    got = _render(r, kw, "cuda", torch.float32)
    again = _render(r, kw, "cuda", torch.float32)
    assert torch.equal(got, again), "two runs differ"
    _check(f"gpu {name}", got, r64, S, eps)
    if forced:
        monkeypatch.delenv("SPHX_VOLUME_SEGMENT")
        one = _render(r, kw, "cuda", torch.float32)
        diff = np.abs((got - one).double().cpu().numpy())
        print(f"gpu {name}: voxels that differ from the unsegmented run {int((diff > 0).sum())} of {diff.size}")
        assert (diff <= 4 * eps * S).all()
    with pytest.raises(ValueError):
        _render(r, kw, "cuda", torch.float64)


def test_rejects_wrong_inputs():
    r, kw = _row("one"), dict(res=(9, 10, 11))
    for bad in (dict(x=r["x"].astype(np.float32)), dict(h=r["h"].astype(np.float64)), dict(w=np.ones((3, 1), np.float32))):
        t = {k: torch.as_tensor(v) for k, v in {**r, **bad}.items() if k != "box"}
        with pytest.raises(ValueError):
            sph_volume(t["x"], t["y"], t["z"], t["h"], t["w"], r["box"], **kw)


def test_volume_conserves_mass():
    """whole-box volume of a periodic cube: sum(V) dV = sum m. The voxel-centre sum of one kernel is its integral plus
    its aliases at the reciprocal lattice; a 3-D lattice sum of the sinc^6 kernel at random offsets deviates from 1 by
    at most 6.3e-7 at h = 2 voxels and 6.2e-8 at h = 3 voxels (6.5e-5 at 1.5 voxels, 0.1 at 1 voxel). h in [2, 4]
    voxels here; the tolerance 2e-6 of the mass is 3x the measured worst case."""
    rng = np.random.default_rng(3)
    n, res = 400, (24, 24, 24)
    x, y, z = rng.random((3, n))
    r = dict(x=x, y=y, z=z, h=((2 + 2 * rng.random(n)) / 24).astype(np.float32),
             w=(rng.random((1, n)) / n).astype(np.float32), box=Box.cube(0, 1, PERIODIC))
    vol = _render(r, dict(res=res), "cpu", torch.float64)
    total, mass = float(vol.sum()) / 24 ** 3, float(r["w"].astype(np.float64).sum())
    print(f"mass: volume {total:.12e} particles {mass:.12e} rel {abs(total / mass - 1):.3e}")
    assert abs(total - mass) <= 2e-6 * mass


def _spectrum_case(N, C):
    """a seeded random field plus a plane wave, float32, and its fp64 spectrum from the full transform, shell by shell"""
    if (N, C) not in _refs:
        rng = np.random.default_rng(N)
        iz, iy, ix = np.meshgrid(*[np.arange(N)] * 3, indexing="ij")
        grid = (rng.standard_normal((C, N, N, N)) + 1.5 * np.cos(2 * np.pi * (2 * ix + iy) / N)).astype(np.float32)
        f = np.fft.fftn(grid.astype(np.float64), axes=(1, 2, 3)) / N ** 3
        k1 = np.fft.fftfreq(N, 1.0 / N)  # integers in [-N/2, N/2)
        b = np.floor(np.sqrt(k1[:, None, None] ** 2 + k1[None, :, None] ** 2 + k1[None, None, :] ** 2) + 0.5)
        p = (f.real ** 2 + f.imag ** 2).sum(axis=0)
        shells = range(int(b.max()) + 1)
        _refs[N, C] = (grid, np.array([p[b == i].sum() for i in shells]), np.array([(b == i).sum() for i in shells]))
    return _refs[N, C]


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("N", [8, 9, 10])  # 9: no Nyquist plane; 8, 10: radix-2 and not
def test_spectrum_cpu(N, C):
    grid, P64, cnt = _spectrum_case(N, C)
    k, P, count = (t.numpy() for t in power_spectrum(torch.from_numpy(grid).double()))
    mean_sq = float((grid.astype(np.float64) ** 2).sum(axis=0).mean())
    assert np.array_equal(k, np.arange(len(P64))) and P.dtype == count.dtype == np.float64
    assert abs(P.sum() - mean_sq) <= 1e-12 * mean_sq and abs(count.sum() - N ** 3) <= 1e-12 * N ** 3
    assert np.abs(P - P64).max() <= 1e-12 * P64.sum() and np.array_equal(count, cnt)
    with pytest.raises(ValueError):
        power_spectrum(torch.zeros(1, N, N, N + 1))


@pytest.mark.gpu
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("N", [8, 9, 10])
def test_spectrum_gpu(N, C):
    """against the fp64 reference; eps_fft is the error of the float32 transform on the host, binned in fp64, and the
    margin of 4 is for rocFFT's different factorisation"""
    grid, P64, cnt = _spectrum_case(N, C)
    eps = np.abs(power_spectrum(torch.from_numpy(grid))[1].numpy() - P64).max() / P64.sum()
    k, P, count = (t.cpu().numpy() for t in power_spectrum(torch.from_numpy(grid).cuda()))
    err = np.abs(P - P64).max() / P64.sum()
    print(f"spectrum N {N} C {C}: eps_fft {eps:.3e} max |P - P64| / sum P64 / (4 eps_fft) {err / (4 * eps):.4f}")
    assert np.array_equal(k, np.arange(len(P64))) and np.array_equal(count, cnt)
    assert err <= 4 * eps


def test_tools_volume_and_spectrum(tmp_path, monkeypatch):
    """the two commands on a 500-particle periodic dump, host path: the density grid conserves the mass (h = 2.1 voxels:
    2e-6, see test_volume_conserves_mass), the spectrum file sums to the mean square of the velocity grids that
    ``tools volume`` writes (float32 grids and transform: 1e-5), and an open box is refused"""
    from sphexa_amd.ops import _lib
    from sphexa_amd.tools.__main__ import main

    monkeypatch.chdir(tmp_path)
    io, rng = _lib.io(), np.random.default_rng(5)
    main(["init-file", "dump.h5", "-n", "500", "--seed", "1"])
    f = io.open("dump.h5", "a")
    g = io.open_step(f, 0)
    io.create_dataset(g, "rho", "f", 500)
    io.write_slice(g, "rho", (1 + rng.random(500)).astype(np.float32), 0)
    io.close_group(g)
    io.close(f)
    common = ["--res", "12", "--device", "cpu"]
    main(["volume", "dump.h5", "rho", "-o", "rho.npy"] + common)
    rho = np.load("rho.npy")
    assert rho.shape == (12, 12, 12) and abs(rho.astype(np.float64).sum() / 12 ** 3 - 1.0) <= 2e-6
    for name in ("vx", "vy", "vz"):
        main(["volume", "dump.h5", name] + common)
    mean_sq = sum(float((np.load(f"volume_{n}.npy").astype(np.float64) ** 2).mean()) for n in ("vx", "vy", "vz"))
    main(["spectrum", "dump.h5"] + common)
    k, P, count = np.loadtxt("spectrum.txt").T
    assert np.array_equal(k, np.arange(len(k))) and count.sum() == 12 ** 3 and abs(P.sum() - mean_sq) <= 1e-5 * mean_sq
    f = io.open("dump.h5", "a")
    g = io.open_step(f, 0)
    io.write_attr(g, "boundaryType", np.array([0, 0, 0], dtype=np.int8))
    io.close_group(g)
    io.close(f)
    with pytest.raises(SystemExit):
        main(["spectrum", "dump.h5"] + common)


def _rank_volume(rank, world, comm, n):
    from sphexa_amd.app.simulation import Simulation

    sim = Simulation("sedov", n=n, device="cpu", comm=comm)
    return {"rho": sim.volume("rho", res=(20, 20, 20)).numpy(),
            "h": sim.volume("h", weighted="mass", res=(20, 20, 20)).numpy()}


def test_two_ranks_equal_one():
    one, two = run_ranks(_rank_volume, 1, 12)[0], run_ranks(_rank_volume, 2, 12)
    for k in ("rho", "h"):
        assert one[k].shape == (20, 20, 20) and np.abs(one[k]).max() > 0
        for r in two:  # fp32 summation order of the all-reduced channels
            assert np.abs(r[k] - one[k]).max() <= 1e-6 * np.abs(one[k]).max()


@pytest.mark.gpu
def test_gpu_simulation_density_and_spectrum():
    from sphexa_amd.app.simulation import Simulation

    sim = Simulation("sedov", n=20, device="cuda").run(1)
    rho = sim.volume("rho", res=(32, 32, 32))
    box, mass = sim.domain.box, float(sim.local("m").double().sum())
    total = float(rho.double().sum()) * math.prod(box.lengths()) / 32 ** 3
    print(f"sedov density: volume mass {total:.9e} particles {mass:.9e} rel {abs(total / mass - 1):.3e}")
    assert rho.shape == (32, 32, 32) and torch.isfinite(rho).all() and (rho > 0).all()
    # h ~ 1.5 / 20 of the box = 2.4 voxels: aliasing below 1e-6 (see test_volume_conserves_mass); fp32 sums and the
    # fp32 records leave a few 1e-6
    assert abs(total - mass) <= 1e-5 * mass
    k, P, count = sim.power_spectrum(("vx", "vy", "vz"), res=32)
    mean_sq = sum(float((sim.volume(f, res=(32, 32, 32)).double() ** 2).mean()) for f in ("vx", "vy", "vz"))
    print(f"sedov spectrum: sum P {float(P.sum()):.9e} mean square {mean_sq:.9e}")
    assert torch.isfinite(P).all() and float(count.sum()) == 32 ** 3
    assert abs(float(P.sum()) - mean_sq) <= 1e-5 * mean_sq
