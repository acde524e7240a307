"""SPH slices and column projections (ops/image.py) against a dense all-pairs fp64 sum.

Bound per pixel and channel: |got - ref64| <= 4 eps S + E_tab T, with S the sum of the magnitudes of the pixel's
terms, eps the error of the same numpy sum run in float32 on inputs rounded as the records round them (relative to S,
largest over the pixels; 64 * 2^-53 for the fp64 host path), E_tab the table builder's own interpolation error and
T = sum |w| / h^2 over the particles that touch the pixel (projections only).
"""

import math

import numpy as np
import pytest
import torch

from sphexa_amd.ops.image import projected_kernel, projection_table, sph_image
from sphexa_amd.utils.box import OPEN, PERIODIC, Box

from mp_util import run_ranks

N_SINC = 6.0
_GL = np.polynomial.legendre.leggauss(200)


def kernel_k(n):
    v = _GL[0] + 1.0  # [0, 2]
    return 1.0 / np.sum(_GL[1] * 4 * math.pi * v * v * np.sinc(v / 2) ** n)


def ref(kind, x, y, z, h, w, box, axis="z", window=None, res=(32, 32), s0=None, s1=None, h_floor=0.5, dtype=np.float64):
    """(image, S, T), each (C, nv, nu): every pixel x every particle x the 9 periodic images"""
    a = "xyz".index(axis)
    iu, iv = (a + 1) % 3, (a + 2) % 3
    pos = [np.asarray(t, dtype=np.float64) for t in (x, y, z)]
    u0, u1, v0, v1 = window or (box.lo[iu], box.hi[iu], box.lo[iv], box.hi[iv])
    (nu, nv), L = res, box.lengths()
    pu, pv = (u1 - u0) / nu, (v1 - v0) / nv
    heff = np.maximum(h.astype(np.float64), h_floor * max(pu, pv))
    if kind == "slice":
        dz = pos[a] - (0.5 * (box.lo[a] + box.hi[a]) if s0 is None else s0)
        if box.bc[a] == PERIODIC:
            dz -= L[a] * np.rint(dz / L[a])
        sel = np.ones(len(heff), bool)
    else:
        dz = np.zeros_like(heff)
        sel = (pos[a] >= (-np.inf if s0 is None else s0)) & (pos[a] <= (np.inf if s1 is None else s1))
    cu, cv = ((pos[iu] - u0) / pu).astype(dtype), ((pos[iv] - v0) / pv).astype(dtype)
    ih, zq = (1.0 / heff).astype(dtype), (dz / heff).astype(dtype)
    gx, gy = np.meshgrid(np.arange(nu, dtype=dtype) + dtype(0.5), np.arange(nv, dtype=dtype) + dtype(0.5))
    gx, gy = gx.ravel()[:, None], gy.ravel()[:, None]
    wd = w.astype(dtype)
    out = np.zeros((3, w.shape[0], nv * nu), dtype)
    for su in ((-1, 0, 1) if box.bc[iu] == PERIODIC else (0,)):
        for sv in ((-1, 0, 1) if box.bc[iv] == PERIODIC else (0,)):
            du = (gx - (cu + dtype(su * L[iu] / pu))[None, :]) * (dtype(pu) * ih)[None, :]
            dv = (gy - (cv + dtype(sv * L[iv] / pv))[None, :]) * (dtype(pv) * ih)[None, :]
            q2 = du * du + dv * dv + (zq * zq)[None, :]
            p, j = np.nonzero((q2 < 4) & sel[None, :])
            q = np.sqrt(q2[p, j])
            if kind == "slice":
                val = dtype(kernel_k(N_SINC)) * np.sinc(q / dtype(2)) ** dtype(N_SINC) * ih[j] ** 3
            else:
                val = projected_kernel(q.astype(np.float64), N_SINC).astype(dtype) * ih[j] ** 2
            for c in range(w.shape[0]):
                np.add.at(out[0, c], p, wd[c, j] * val)
                np.add.at(out[1, c], p, np.abs(wd[c, j] * val))
                if kind == "projection":
                    np.add.at(out[2, c], p, np.abs(wd[c, j]) * ih[j] ** 2)
    return out.reshape(3, w.shape[0], nv, nu)


def _row(name):
    rng = np.random.default_rng(7)
    if name == "one":
        return dict(x=np.array([0.52]), y=np.array([0.47]), z=np.array([0.45]), h=np.array([0.3], np.float32),
                    w=np.array([[1.5]], np.float32), box=Box.cube(0, 1, OPEN), res=(33, 31))
    if name == "batch":
        x, y, z = rng.random((3, 257))
        return dict(x=x, y=y, z=z, h=np.full(257, 0.08, np.float32), w=np.full((1, 257), 1 / 257, np.float32),
                    box=Box.cube(0, 1, PERIODIC), res=(64, 64))
    if name.startswith("contrast"):
        x, y, z = rng.random((3, 2000))
        h = (0.0005 * 40 ** rng.random(2000)).astype(np.float32)  # pixel: 0.0043 x 0.004
        x[0], y[0], z[0], h[0] = 0.7, 0.25, 0.5, 1.0  # covers every tile
        m = (1e-3 * 10 ** rng.random(2000)).astype(np.float32)
        w = np.stack([m * (1 + x).astype(np.float32), m])
        return dict(x=x, y=y, z=z, h=h, w=w, box=Box.cube(0, 1, OPEN), res=(70, 50), window=(0.55, 0.85, 0.15, 0.35),
                    h_floor=0.0 if name == "contrast0" else 0.5)
    a = "xyz".index(name[-1])  # axes-x, axes-y, axes-z: periodic in the view axis only
    x, y, z = rng.random((3, 300))
    box = Box([0.0] * 3, [1.0] * 3, [PERIODIC if d == a else OPEN for d in range(3)])
    return dict(x=x, y=y, z=z, h=np.full(300, 0.1, np.float32), w=rng.random((1, 300)).astype(np.float32), box=box,
                res=(40, 40), axis=name[-1], s0=0.0, s1=0.5)


ROWS = ["one", "batch", "contrast", "contrast0", "axes-x", "axes-y", "axes-z"]
KINDS = ["slice", "projection"]
_refs = {}


def _case(kind, name):
    """the row's inputs and call arguments, its fp64 reference and the eps of the float32 twin (computed once)"""
    if (kind, name) not in _refs:
        r = _row(name)
        kw = {k: v for k, v in r.items() if k in ("axis", "window", "res", "h_floor", "s0")}
        if kind == "projection" and "s1" in r:
            kw["s1"] = r["s1"]
        args = (r["x"], r["y"], r["z"], r["h"], r["w"], r["box"])
        r64, S, T = ref(kind, *args, **kw)
        r32 = ref(kind, *args, **kw, dtype=np.float32)[0]
        eps = float((np.abs(r32 - r64)[S > 0] / S[S > 0]).max())
        _refs[kind, name] = (r, kw, r64, S, T, eps)
    return _refs[kind, name]


def _render(kind, r, kw, device, dtype):
    t = lambda a, dt: torch.as_tensor(a, dtype=dt).to(device)
    return sph_image(t(r["x"], torch.float64), t(r["y"], torch.float64), t(r["z"], torch.float64),
                     t(r["h"], torch.float32), t(r["w"], torch.float32), r["box"], kind=kind, sinc_index=N_SINC,
                     out_dtype=dtype, **kw)


def _check(tag, got, r64, S, T, eps):
    bound = 4 * eps * S + projection_table(N_SINC)[1] * T
    err = np.abs(got.double().cpu().numpy() - r64)
    ratio = float((err[bound > 0] / bound[bound > 0]).max())
    print(f"{tag}: eps {eps:.3e} max |got - ref| / bound {ratio:.4f}")
    assert got.shape == r64.shape and np.isfinite(err).all()
    assert (err <= bound).all(), f"{tag}: ratio {ratio}"


@pytest.mark.parametrize("name", ROWS)
@pytest.mark.parametrize("kind", KINDS)
def test_cpu_rows(kind, name):
    r, kw, r64, S, T, _ = _case(kind, name)
    _check(f"cpu {kind} {name}", _render(kind, r, kw, "cpu", torch.float64), r64, S, T, 64 * 2.0 ** -53)


@pytest.mark.parametrize("n", [4.0, 6.0, 9.0])
def test_projection_table(n):
    table, err = projection_table(n)
    v = _GL[0] + 1.0
    f0 = 2 * kernel_k(n) * np.sum(_GL[1] * np.sinc(v / 2) ** n)  # 2 int_0^2 W(s) ds
    assert abs(table[0] - f0) < 1e-10 and table[-1] == 0.0 and 0 < err < 1e-6
    assert abs(2 * math.pi * np.sum(_GL[1] * projected_kernel(v, n) * v) - 1.0) < 1e-10


def test_projection_conserves_mass():
    """whole-box projection of a periodic box, floor on: sum(image) * pixel area = sum m. The pixel-centre sum of one
    projected kernel is its integral plus its aliases at the reciprocal lattice (Poisson summation), k = 2 pi j h / pixel
    >= 4 pi for h >= 2 pixels, where the transform of the sinc^6 projection (width ~0.55 h, edge a sixth-order zero:
    tail ~ k^-7) is below 1e-7 of its mass; table and fp64 rounding are smaller still. Tolerance 1e-6 of the mass."""
    rng = np.random.default_rng(3)
    n, res = 400, (48, 48)
    x, y, z = rng.random((3, n))
    r = dict(x=x, y=y, z=z, h=((2 + 2 * rng.random(n)) / 48).astype(np.float32),
             w=(rng.random((1, n)) / n).astype(np.float32), box=Box.cube(0, 1, PERIODIC))
    img = _render("projection", r, dict(res=res), "cpu", torch.float64)
    total, mass = float(img.sum()) / (res[0] * res[1]), float(r["w"].astype(np.float64).sum())
    print(f"mass: image {total:.12e} particles {mass:.12e} rel {abs(total / mass - 1):.3e}")
    assert abs(total - mass) <= 1e-6 * mass


def _rank_image(rank, world, comm, n):
    from sphexa_amd.app.simulation import Simulation

    sim = Simulation("sedov", n=n, device="cpu", comm=comm)
    return {"rho": sim.image("rho", kind="projection", res=(40, 40)).numpy(),
            "h": sim.image("h", kind="slice", weighted="mass", res=(40, 40)).numpy()}


def test_two_ranks_equal_one():
    one, two = run_ranks(_rank_image, 1, 12)[0], run_ranks(_rank_image, 2, 12)
    for k in ("rho", "h"):
        assert np.abs(one[k]).max() > 0
        for r in two:  # fp32 summation order of the all-reduced channels
            assert np.abs(r[k] - one[k]).max() <= 1e-6 * np.abs(one[k]).max()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ROWS + ["segments"])
@pytest.mark.parametrize("kind", KINDS)
def test_gpu_rows(kind, name, monkeypatch):
    forced = name == "segments"  # the contrast set cut into 64-entry segments: partial tiles and their ordered sum
    r, kw, r64, S, T, eps = _case(kind, "contrast" if forced else name)
    if forced:
        monkeypatch.setenv("SPHX_IMAGE_SEGMENT", "64")
    got = _render(kind, r, kw, "cuda", torch.float32)
    again = _render(kind, r, kw, "cuda", torch.float32)
    assert torch.equal(got, again), "two runs differ"
    _check(f"gpu {kind} {name}", got, r64, S, T, eps)
    if forced:
        monkeypatch.delenv("SPHX_IMAGE_SEGMENT")
        bound = 4 * eps * S + projection_table(N_SINC)[1] * T
        one = _render(kind, r, kw, "cuda", torch.float32)
        assert (np.abs((got - one).double().cpu().numpy()) <= bound).all()


@pytest.mark.gpu
def test_gpu_simulation_column_density():
    from sphexa_amd.app.simulation import Simulation

    sim = Simulation("sedov", n=20, device="cuda").run(1)
    img = sim.image("rho", kind="projection", res=(64, 64))
    box, mass = sim.domain.box, float(sim.local("m").double().sum())
    area = (box.hi[0] - box.lo[0]) * (box.hi[1] - box.lo[1]) / (64 * 64)
    total = float(img.double().sum()) * area
    print(f"sedov column density: image mass {total:.9e} particles {mass:.9e} rel {abs(total / mass - 1):.3e}")
    assert torch.isfinite(img).all() and (img > 0).all()
    # h ~ 1.5 / 20 of the box = 4.8 pixels: aliasing below 1e-9 (see test_projection_conserves_mass); fp32 sums of
    # ~60 terms per pixel and the fp32 records leave a few 1e-6
    assert abs(total - mass) <= 1e-5 * mass
