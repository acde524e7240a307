"""Opacity renderings (ops/image.py kind="render") against a dense numpy compositing loop in float64.

Per pixel |I - I64| <= 4 eps_I S_I + E_tab Tt max|s| and |T - T64| <= 4 eps_T T64 (1 + tau64) + E_tab Tt: S_I = sum
|T (1 - a_k) s_j|, Tt = sum |w_0| / h^2, tau64 = sum tau_k; eps_I, eps_T the largest errors of the same loop in float32
(inputs rounded as the records round them) relative to S_I and T64 (1 + tau64), 64 * 2^-53 for the fp64 host path; E_tab
the F_n table's interpolation error (|dI/dtau_k| <= max|s|, |dT| <= T sum dtau). The 4 is the factor tests/test_image.py
grants its float32 twin. Every row keeps tau64 < 60: no fp32 transmittance is denormal."""

import numpy as np
import pytest
import torch

from sphexa_amd.app.simulation import Simulation
from sphexa_amd.ops.image import projected_kernel, projection_table, sph_image
from sphexa_amd.utils.box import OPEN, PERIODIC, Box

from mp_util import run_ranks

N_SINC, f32 = 6.0, np.float32


def ref(x, y, z, h, w, box, axis="z", window=None, res=(32, 32), s0=None, s1=None, h_floor=0.5, dtype=np.float64):
    """(I, T, tau, S_I, Tt), each (nv, nu): the entries of every pixel selected as tests/test_image.py::ref selects a
    projection's, ordered by (depth, particle index, shift code) and composited one rank of the order at a time"""
    a = "xyz".index(axis[-1])
    iu, iv = (a + 1) % 3, (a + 2) % 3
    pos = [np.asarray(t, dtype=np.float64) for t in (x, y, z)]
    u0, u1, v0, v1 = window or (box.lo[iu], box.hi[iu], box.lo[iv], box.hi[iv])
    (nu, nv), L = res, box.lengths()
    pu, pv = (u1 - u0) / nu, (v1 - v0) / nv
    heff = np.maximum(h.astype(np.float64), h_floor * max(pu, pv))
    sel = (pos[a] >= (-np.inf if s0 is None else s0)) & (pos[a] <= (np.inf if s1 is None else s1))
    depth = -pos[a] if axis[0] == "-" else pos[a]
    rank = np.empty(len(depth), np.int64)
    rank[np.lexsort((np.arange(len(depth)), depth))] = np.arange(len(depth))  # -0.0 == +0.0: a tie, broken by index
    cu, cv = ((pos[iu] - u0) / pu).astype(dtype), ((pos[iv] - v0) / pv).astype(dtype)
    ih, wd = (1.0 / heff).astype(dtype), w.astype(dtype)
    centres = np.meshgrid(np.arange(nu, dtype=dtype) + dtype(0.5), np.arange(nv, dtype=dtype) + dtype(0.5))
    gx, gy = (g.ravel()[:, None] for g in centres)
    ent = []  # (pixel, particle, shift code, tau)
    for sv in ((-1, 0, 1) if box.bc[iv] == PERIODIC else (0,)):
        for su in ((-1, 0, 1) if box.bc[iu] == PERIODIC else (0,)):
            du = (gx - (cu + dtype(su * L[iu] / pu))[None, :]) * (dtype(pu) * ih)[None, :]
            dv = (gy - (cv + dtype(sv * L[iv] / pv))[None, :]) * (dtype(pv) * ih)[None, :]
            q2 = du * du + dv * dv
            p, j = np.nonzero((q2 < 4) & sel[None, :])
            val = projected_kernel(np.sqrt(q2[p, j]).astype(np.float64), N_SINC).astype(dtype) * ih[j] ** 2
            ent.append((p, j, np.full(len(p), 3 * (sv + 1) + su + 1), wd[0, j] * val))
    p, j, code, tau = (np.concatenate(c) for c in zip(*ent))
    o = np.lexsort((code, rank[j], p))
    p, j, tau = p[o], j[o], tau[o]
    nth = np.arange(len(p)) - np.searchsorted(p, p)  # position of the entry in its pixel's order
    I, T, tsum, S, Tt = out = np.zeros((5, nv * nu), dtype)
    T[:] = 1
    for r in range(int(nth.max()) + 1 if len(p) else 0):
        k = nth == r
        term = T[p[k]] * -np.expm1(-tau[k]) * wd[1, j[k]]
        I[p[k]] += term
        S[p[k]] += np.abs(term)
        T[p[k]] *= np.exp(-tau[k])
        tsum[p[k]] += tau[k]
        Tt[p[k]] += np.abs(wd[0, j[k]]) * ih[j[k]] ** 2
    return out.reshape(5, nv, nu)


def _row(name):
    """inputs of a row; ``thick`` / ``thin``: the row must hold a pixel of tau > 5 / of 0 < tau < 1e-3"""
    rng = np.random.default_rng(11)
    if name == "one":  # footprint, [0, 1] background, partial tiles
        return dict(x=np.array([0.52]), y=np.array([0.47]), z=np.array([0.45]), h=np.array([0.3], f32),
                    w=np.array([[1.5], [0.7]], f32), box=Box.cube(0, 1, OPEN), res=(33, 31), thick=True, thin=True)
    if name.startswith("occlusion"):  # a dark sheet of tau ~ 20 at z = 0.3 over x < 0.5, a bright layer at z = 0.7
        g = (np.arange(12) + 0.5) / 12
        lx, ly = (t.ravel() for t in np.meshgrid(g, g))
        sx, sy, n, k = lx[lx < 0.5], ly[lx < 0.5], 144, 72
        w = np.stack([np.r_[np.full(k, 20 / 144), np.full(n, 2 / 144)], np.r_[np.zeros(k), np.ones(n)]]).astype(f32)
        return dict(x=np.r_[sx, lx], y=np.r_[sy, ly], z=np.r_[np.full(k, 0.3), np.full(n, 0.7)],
                    h=np.full(k + n, 0.15, f32), w=w, box=Box.cube(0, 1, OPEN), res=(40, 24),
                    axis="-z" if name.endswith("rev") else "z", thick=True)
    if name == "ties":  # 3 exact depth planes (one of them z = -0.0 / +0.0), every second particle on top of the first
        x, y = rng.random((2, 300))
        x[1::2], y[1::2] = x[0::2], y[0::2]
        z = np.repeat([0.0, 0.25, 0.5], 100)
        z[:100:3] = -0.0
        w = np.stack([0.0115 * (0.5 + rng.random(300)), rng.random(300)]).astype(f32)
        return dict(x=x, y=y, z=z, h=np.full(300, 0.1, f32), w=w, box=Box.cube(-1, 2, OPEN), window=(0, 1, 0, 1),
                    res=(40, 40))
    if name == "batch":  # a blob across the periodic corner: several 256-entry batches per tile, a thin rim
        x, y = (np.array([0.1, 0.9])[:, None] + 0.12 * rng.standard_normal((2, 600))) % 1.0
        w = np.stack([np.full(600, 0.0045), 1 + rng.random(600)]).astype(f32)
        return dict(x=x, y=y, z=rng.random(600), h=np.full(600, 0.08, f32), w=w, box=Box.cube(0, 1, PERIODIC),
                    res=(64, 64), thick=True, thin=True)
    if name == "contrast":  # h over a factor 40, one particle over every tile, a window; kappa for tau up to ~30
        x, y, z = rng.random((3, 2000))
        h = (0.0005 * 40 ** rng.random(2000)).astype(f32)  # pixel: 0.0043 x 0.004
        x[0], y[0], z[0], h[0] = 0.7, 0.25, 0.5, 1.0
        m = (1e-3 * 10 ** rng.random(2000)).astype(f32)
        return dict(x=x, y=y, z=z, h=h, w=np.stack([f32(0.02) * m, (1 + x).astype(f32)]), box=Box.cube(0, 1, OPEN),
                    res=(70, 50), window=(0.55, 0.85, 0.15, 0.35), thick=True)
    a = "xyz".index(name[-1])  # slab-x, slab-y: periodic in the view axis only
    x, y, z = rng.random((3, 300))
    box = Box([0.0] * 3, [1.0] * 3, [PERIODIC if d == a else OPEN for d in range(3)])
    w = np.stack([0.02 * rng.random(300), rng.random(300)]).astype(f32)
    return dict(x=x, y=y, z=z, h=np.full(300, 0.1, f32), w=w, box=box, res=(40, 40), axis=name[-1], s0=0.0, s1=0.5)


ROWS = ["one", "occlusion", "occlusion-rev", "ties", "batch", "contrast", "slab-x", "slab-y"]
_refs = {}


def _case(name, r=None):
    """(inputs, call arguments, fp64 reference, the float32 twin's (eps_I, eps_T)) of a row, computed once"""
    if name not in _refs:
        r = r or _row(name)
        kw = {k: v for k, v in r.items() if k in ("axis", "window", "res", "s0", "s1")}
        args = (r["x"], r["y"], r["z"], r["h"], r["w"], r["box"])
        r64, r32 = ref(*args, **kw), ref(*args, **kw, dtype=np.float32)
        I, T, tau, S, _ = r64
        assert tau.max() < 60 and (not r.get("thick") or tau.max() > 5)
        assert not r.get("thin") or ((tau > 0) & (tau < 1e-3)).any()
        eps = (float((np.abs(r32[0] - I)[S > 0] / S[S > 0]).max()), float((np.abs(r32[1] - T) / (T * (1 + tau))).max()))
        _refs[name] = (r, kw, r64, eps)
    return _refs[name]


def _render(r, kw, device, dtype):
    t = lambda a, dt: torch.as_tensor(a, dtype=dt).to(device)
    return sph_image(t(r["x"], torch.float64), t(r["y"], torch.float64), t(r["z"], torch.float64),
                     t(r["h"], torch.float32), t(r["w"], torch.float32), r["box"], kind="render", sinc_index=N_SINC,
                     out_dtype=dtype, **kw)


def _bounds(r, r64, eps):
    (I, T, tau, S, Tt), etab = r64, projection_table(N_SINC)[1]
    return np.stack([4 * eps[0] * S + etab * Tt * np.abs(r["w"][1]).max(), 4 * eps[1] * T * (1 + tau) + etab * Tt])


def _check(tag, got, r, r64, eps):
    bound = _bounds(r, r64, eps)
    err = np.abs(got.double().cpu().numpy() - r64[:2])
    ratio = [float((e[b > 0] / b[b > 0]).max()) for e, b in zip(err, bound)]
    print(f"{tag}: eps_I {eps[0]:.3e} eps_T {eps[1]:.3e} max |got - ref| / bound: I {ratio[0]:.4f} T {ratio[1]:.4f}")
    assert got.shape == r64[:2].shape and np.isfinite(err).all() and (err <= bound).all(), f"{tag}: ratios {ratio}"
    if tag.endswith("occlusion-rev"):  # the same scene from the front, under the sheet: the order decides the image
        front, under = _case("occlusion")[2][0], slice(0, 12)
        assert (np.abs(got[0].double().cpu().numpy() - front)[:, under] > 1e3 * bound[0][:, under]).all()


@pytest.mark.parametrize("name", ROWS)
def test_cpu_rows(name):
    r, kw, r64, _ = _case(name)
    _check(f"cpu {name}", _render(r, kw, "cpu", torch.float64), r, r64, (64 * 2.0 ** -53,) * 2)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ROWS + ["segments", "segments8"])
def test_gpu_rows(name, monkeypatch):
    # the contrast set with a forced segment length. Its six tiles hold 55, 41, 15, 29, 30 and 7 entries: 64 cuts none
    # of them, 8 cuts all but one into up to 7 partial tiles, composed in list order
    forced = name.startswith("segments")
    r, kw, r64, eps = _case("contrast" if forced else name)
    if forced:
        monkeypatch.setenv("SPHX_IMAGE_SEGMENT", name[8:] or "64")
    got = _render(r, kw, "cuda", torch.float32)
    assert torch.equal(got, _render(r, kw, "cuda", torch.float32)), "two runs differ"
    _check(f"gpu {name}", got, r, r64, eps)
    if forced:
        monkeypatch.delenv("SPHX_IMAGE_SEGMENT")
        one = _render(r, kw, "cuda", torch.float32)
        assert (np.abs((got - one).double().cpu().numpy()) <= _bounds(r, r64, eps)).all()
        assert name == "segments" or not torch.equal(got, one), "no tile was cut"


@pytest.mark.gpu
def test_gpu_simulation_render():
    sim = Simulation("evrard", n=20, device="cuda").run(1)  # (a VE run: rho = kx m / xm, set by the step)
    d, box, got = sim.d, sim.domain.box, sim.image("rho", kind="render", res=(32, 32))
    assert got.shape == (2, 32, 32) and torch.isfinite(got).all() and (got[1] >= 0).all() and (got[1] <= 1).all()
    # the default kappa makes the window's mean optical depth 1: the mean of -log T is that mean, sampled at the pixel
    # centres (by Jensen -log of the mean T is below it); a factor 2 either way holds the definition, not a precision
    assert 0.5 <= float(-torch.log(got[1].double()).mean()) <= 2.0
    host = lambda name: d[name].cpu().numpy()  # device and host path on the same particles against the dense oracle
    inside = (host("x") >= box.lo[0]) & (host("x") <= box.hi[0]) & (host("y") >= box.lo[1]) & (host("y") <= box.hi[1])
    kappa = (box.hi[0] - box.lo[0]) * (box.hi[1] - box.lo[1]) / host("m")[inside].sum(dtype=np.float64)
    r = dict(x=host("x"), y=host("y"), z=host("z"), h=host("h"), box=box, res=(32, 32),
             w=np.stack([np.float32(kappa) * host("m"), host("kx") * host("m") / host("xm")]).astype(np.float32))
    _, kw, r64, eps = _case("evrard", r)
    _check("gpu evrard", got, r, r64, eps)
    _check("cpu evrard", _render(r, kw, "cpu", torch.float64), r, r64, (64 * 2.0 ** -53,) * 2)


def _rank_render(rank, world, comm, n):
    with pytest.raises(NotImplementedError):
        Simulation("sedov", n=n, device="cpu", comm=comm).image("rho", kind="render", res=(16, 16))


def test_render_refusals():
    r, kw, _, _ = _case("one")
    with pytest.raises(ValueError, match="two weight rows"):
        _render(dict(r, w=r["w"][:1]), kw, "cpu", torch.float64)
    run_ranks(_rank_render, 2, 12)
