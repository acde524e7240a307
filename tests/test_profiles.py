"""Radial profiles and spherical-overdensity masses (ops/profiles.py) against a dense numpy oracle: the C x n fp64
matrix of minimum-image d2 with the product order of sphx/pairstats.hpp, cast to float32 keys, np.lexsort per centre and
cumulative sums in fp64 (definitions: sphx/profiles.hpp).

count, hits, so_count and so_truncated must be exactly the oracle's and so_radius equal in bits; the sum channels and
so_mass lie within the ordered-fp64 bound (2 k + 8) 2^-53 sum |terms| of k terms. The oracle asserts on every row and
at every tie-run end |M_q - thr_q| > 8 times that bound, so no rounding of either path can flip a crossing."""

import functools

import numpy as np
import pytest
import torch

from sphexa_amd.ops.profiles import profile_quantities, radial_profiles
from sphexa_amd.utils.box import OPEN, PERIODIC, Box

ROWS = ["single", "edges", "edges-default", "ties", "wrap", "wrap-open", "empty", "empty-open", "truncated", "overlap"]
U53, FOUR_PI_THIRD = 2.0 ** -53, 4.18879020478639098


@functools.lru_cache(maxsize=None)
def _row(name, device):
    """a row, computed once and shared: the numpy inputs pos, centres, box, edges, m, v, vc, u, rho, select, first,
    last, the segment it runs with, ``ref`` (the oracle's values) and the arguments ``args``, ``kw`` of radial_profiles
    as tensors on ``device``"""
    t = lambda a, dt=torch.float64: None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dt).to(device)
    cols = lambda a: None if a is None else tuple(t(a[:, k]) for k in range(3))
    tensors = lambda r: dict(
        args=(t(r["centres"]), *cols(r["pos"]), t(r["m"]), r["box"], r["edges"]),
        kw=dict(v=cols(r["v"]), u=t(r["u"]), vc=t(r["vc"]), thresholds=r["rho"], select=t(r["select"], torch.bool),
                first=r["first"], last=r["last"]))
    if device != "cpu":
        return {**_row(name, "cpu"), **tensors(_row(name, "cpu"))}
    rng = np.random.default_rng(ROWS.index(name.split("-")[0]) + 5)

    def _ball(rng, k, radius):  # k points inside a ball
        p = rng.normal(size=(k, 3))
        return p / np.linalg.norm(p, axis=1)[:, None] * radius * rng.random((k, 1)) ** (1 / 3)

    box, v, vc, u, select, first, last, segment = Box.cube(0.0, 1.0, OPEN), None, None, None, None, 0, None, None
    edges, m = np.array([0.0, 0.01, 0.02, 0.035, 0.05]), None
    if name == "single":  # by hand: at the centre, inside bin 0, on the inner edge 0.25, in bin 1, at r_max, far away
        off = [[0, 0, 0], [0.15, 0, 0], [0.25, 0, 0], [0, -0.3, 0.1], [0, 0.5, 0], [-0.4, -0.4, -0.4]]
        pos, centres, rho, m = 0.5 + np.array(off), np.full((1, 3), 0.5), [10.0], np.ones(6)
        edges = np.array([0.1, 0.25, 0.5])
    elif name in ("edges", "edges-default"):  # hit counts at the wave-scan and chunk boundaries; with a segment of
        # 128 the 600 hits split items and segments, edges-default runs the same points with the default segment
        sizes = [63, 64, 65, 127, 128, 129, 600]
        centres = np.array([[0.2, 0.2, 0.2], [0.5, 0.2, 0.2], [0.8, 0.2, 0.2], [0.2, 0.5, 0.2], [0.5, 0.5, 0.2],
                            [0.8, 0.5, 0.2], [0.5, 0.5, 0.8]]) + 0.01 * rng.random((7, 3))
        pos = np.concatenate([c + _ball(rng, k, 0.045) for c, k in zip(centres, sizes)])
        rho, segment = [20.0, 200.0], 128 if name == "edges" else None
    elif name == "ties":  # mirrored pairs on a dyadic lattice: every key comes at least twice; a pair of unit masses
        off = rng.integers(-40, 41, size=(200, 3)) / 1024.0
        pair = 0.25 + np.array([[1 / 32, 0, 0], [-1 / 32, 0, 0]])
        pos = np.concatenate([[[0.5, 0.5, 0.5]], 0.5 + off, 0.5 - off, pair])
        centres, edges = np.array([[0.5, 0.5, 0.5], [0.25, 0.25, 0.25]]), np.array([0.0, 16, 32, 48, 64]) / 1024.0
        m = np.concatenate([(0.5 + rng.random(401)) / 401, [1.0, 1.0]])
        # at r = 1 / 32 the sphere of the second threshold holds 1.5: above the first of the two unit masses, below both
        rho, segment = [2000.0, 1.5 / (FOUR_PI_THIRD / 32 ** 3)], 128
    elif name in ("wrap", "wrap-open"):  # dyadic coordinates: the wrapped and the shifted points have the same keys
        lo, L = np.array([0.0, -0.25, 0.125]), np.array([1.0, 1.25, 0.875])
        box = Box(list(lo), list(lo + L), [PERIODIC] * 3)
        off, c = rng.integers(-60, 61, size=(300, 3)) / 1024.0, np.full(3, 8 / 1024.0)
        pos, centres, rho = lo + (c + off) % L, (lo + c)[None, :], [100.0, 1e3]
        edges = np.array([0.0, 24, 48, 64]) / 1024.0
        if name == "wrap-open":
            box, pos, centres = Box(list(lo), list(lo + L), [OPEN] * 3), lo + 0.5 + c + off, (lo + 0.5 + c)[None, :]
    elif name in ("empty", "empty-open", "truncated"):  # a far centre, one outside the extent; a threshold too high
        box = Box.cube(0.0, 1.0, PERIODIC if name == "empty" else OPEN)
        pos = 0.2 + _ball(rng, 90, 0.04)
        centres = np.array([[0.2, 0.2, 0.2], [0.7, 0.7, 0.7], [1.5, 0.2, 0.2]])
        rho = [1e-6] if name == "truncated" else [50.0, 1e30]
    else:  # overlap: spheres that share particles; select, a particle range, velocities, centre velocities and u
        cl = np.array([[0.3, 0.3, 0.3], [0.36, 0.3, 0.3], [0.7, 0.6, 0.5]])
        pos = np.concatenate([c + rng.normal(size=(400, 3)) * 0.03 for c in cl] + [rng.random((100, 3))])
        pos = pos[rng.permutation(len(pos))]
        centres = pos[rng.choice(len(pos), 200, replace=False)] + 0.002 * rng.normal(size=(200, 3))
        v, vc, u = rng.normal(size=(len(pos), 3)), rng.normal(size=(200, 3)), 0.5 + rng.random(len(pos))
        select, first, last, rho = rng.random(len(pos)) < 0.8, 50, len(pos) - 30, [30.0, 150.0]
    n = len(pos)
    m = ((0.5 + rng.random(n)) / n) if m is None else m
    r = dict(pos=pos, centres=centres, box=box, edges=edges, m=m, v=v, vc=vc, u=u, rho=rho, select=select,
             first=first, last=n if last is None else last, segment=segment)
    return {**r, **tensors(r), "ref": _oracle(r)}


def _oracle(r):
    """reference values and bounds of the inputs r: dict of count, hits, so_* and per channel (value, bound)"""
    box, edges, m = r["box"], r["edges"], r["m"]
    take = np.arange(r["first"], r["last"])
    take = take if r["select"] is None else take[r["select"][take]]
    d = r["pos"][take][None, :, :] - r["centres"][:, None, :]
    for a in range(3):
        if box.bc[a] == PERIODIC:
            L = box.hi[a] - box.lo[a]
            d[..., a] -= L * np.rint(d[..., a] * (1.0 / L))
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    key, E = d2.astype(np.float32), (edges * edges).astype(np.float32)
    C, nb, T = len(r["centres"]), len(edges) - 1, len(r["rho"])
    names = ["mass"] + (["mvr", "mvr2", "mv2"] if r["v"] is not None else []) + (["mu"] if r["u"] is not None else [])
    out = dict(count=np.zeros((C, nb), np.int64), hits=np.zeros(C, np.int64), so_radius=np.full((C, T), np.nan),
               so_mass=np.full((C, T), np.nan), so_mass_bound=np.zeros((C, T)), so_count=np.zeros((C, T), np.int64),
               so_truncated=np.zeros((C, T), bool), **{k: np.zeros((2, C, nb)) for k in names})
    for c in range(C):
        order = np.lexsort((key[c],))
        order = order[key[c][order] < E[nb]]
        j, k = take[order], key[c][order]
        out["hits"][c] = len(j)
        terms = dict(mass=m[j])
        if r["v"] is not None:
            w = r["v"][j] - (0.0 if r["vc"] is None else r["vc"][c])
            dd, s2 = d[c][order], d2[c][order]
            dot = (w[:, 0] * dd[:, 0] + w[:, 1] * dd[:, 1]) + w[:, 2] * dd[:, 2]
            wr = np.divide(dot, np.sqrt(s2), out=np.zeros_like(dot), where=s2 > 0)
            terms.update(mvr=m[j] * wr, mvr2=(m[j] * wr) * wr,
                         mv2=m[j] * ((w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1]) + w[:, 2] * w[:, 2]))
        if r["u"] is not None:
            terms["mu"] = m[j] * r["u"][j]
        for b in range(nb):
            inb = (k >= E[b]) & (k < E[b + 1])
            out["count"][c, b] = inb.sum()
            for name in names:
                t = terms[name][inb]
                out[name][:, c, b] = np.cumsum(t)[-1] if len(t) else 0.0, (2 * len(t) + 8) * U53 * np.abs(t).sum()
        if len(j) == 0:
            continue
        M, end = np.cumsum(m[j]), np.append(k[1:] != k[:-1], True)
        bound = (2 * np.arange(1, len(j) + 1) + 8) * U53 * np.cumsum(np.abs(m[j]))
        rq = np.sqrt(k.astype(np.float64))
        for t, rho in enumerate(r["rho"]):
            thr = (FOUR_PI_THIRD * rho) * ((rq * rq) * rq)
            assert (np.abs(M - thr)[end] > 8 * bound[end]).all(), "a crossing within the rounding"
            q = np.nonzero(end & (M >= thr))[0]
            if len(q):
                q = q[-1]
                out["so_radius"][c, t], out["so_mass"][c, t], out["so_mass_bound"][c, t] = rq[q], M[q], bound[q]
                out["so_count"][c, t], out["so_truncated"][c, t] = q + 1, q == len(j) - 1
    return out


@pytest.mark.parametrize("name", ROWS)
def test_cpu_rows(name, monkeypatch, device="cpu"):
    r = _row(name, device)
    ref = r["ref"]
    if r["segment"] is not None:
        monkeypatch.setenv("SPHX_PROFILE_SEGMENT", str(r["segment"]))
    out = radial_profiles(*r["args"], **r["kw"])
    got = {k: v.cpu().numpy() for k, v in out.items()}
    for k in ("count", "hits", "so_count", "so_truncated"):
        assert np.array_equal(got[k], ref[k]), k
    assert np.array_equal(got["so_radius"].view(np.int64), ref["so_radius"].view(np.int64))
    for k in [k for k in ref if ref[k].ndim == 3] + ["so_mass"]:  # the sum channels: (value, bound)
        val, bnd = (ref[k][0], ref[k][1]) if k != "so_mass" else (ref[k], ref["so_mass_bound"])
        assert np.array_equal(np.isnan(got[k]), np.isnan(val)), k
        err = np.nan_to_num(np.abs(got[k] - val))
        assert (err <= bnd).all(), (k, (err - bnd).max())
    if name == "single":
        assert out["count"].tolist() == [[1, 2]] and out["hits"].tolist() == [4]
    if name.startswith("edges"):
        assert out["hits"].tolist() == [63, 64, 65, 127, 128, 129, 600]
    if name == "ties":  # the run across the first segment boundary; the pair of unit masses crosses as a run
        k = np.sort(np.linalg.norm(r["pos"][1:401] - 0.5, axis=1))
        assert k[126] == k[127] and out["so_count"][1].tolist() == [2, 2] and float(out["so_mass"][1, 1]) == 2.0
    if name.startswith("empty"):
        assert out["hits"].tolist()[1:] == [0, 0] and not out["count"][1:].any() and int(out["so_count"][0, 0]) > 0
        assert out["so_radius"][1:].isnan().all() and out["so_radius"][:, 1].isnan().all()
    if name == "truncated":
        assert out["so_truncated"][0, 0] and int(out["so_count"][0, 0]) == 90
    if name == "wrap":  # the same points in an open box
        o = _row("wrap-open", device)
        other = radial_profiles(*o["args"], **o["kw"])
        assert int(out["hits"][0]) > 100 and all(torch.equal(out[k], other[k]) for k in
                                                 ("count", "hits", "so_count", "so_truncated", "so_radius"))
    if device != "cpu":  # bit-identical from run to run
        again = radial_profiles(*r["args"], **r["kw"])
        assert all(torch.equal(out[k].nan_to_num(7.0), again[k].nan_to_num(7.0)) for k in out)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ROWS)
def test_gpu_rows(name, monkeypatch):
    test_cpu_rows(name, monkeypatch, device="cuda")  # the same checks on the device path


@pytest.mark.gpu
def test_device_equals_host():
    d, h = _row("overlap", "cuda"), _row("overlap", "cpu")
    dev, host = radial_profiles(*d["args"], **d["kw"]), radial_profiles(*h["args"], **h["kw"])
    for k in ("count", "hits", "so_count", "so_truncated"):
        assert torch.equal(dev[k].cpu(), host[k]), k
    assert torch.equal(dev["so_radius"].cpu().nan_to_num(7.0), host["so_radius"].nan_to_num(7.0))
    q = profile_quantities(host, h["edges"])
    assert torch.equal(q["density"].isnan(), host["count"] == 0) and (q["sigma"][host["count"] > 0] >= 0).all()


def test_rejects_wrong_inputs(monkeypatch):
    x, c = torch.rand(10, dtype=torch.float64), torch.full((2, 3), 0.5, dtype=torch.float64)
    box, per, e = Box.cube(0.0, 1.0, OPEN), Box.cube(0.0, 1.0, PERIODIC), [0.0, 0.1, 0.2]
    radial_profiles(c, x, x, x, x, box, e, thresholds=[1.0])
    for bad in (dict(box=per, edges=[0.0, 0.34]), dict(edges=[0.0, 0.2, 0.1]), dict(edges=np.linspace(0.0, 0.2, 66)),
                dict(thresholds=[1.0] * 9), dict(centres=c.float()), dict(centres=c.to("meta")), dict(m=x[:5]),
                dict(v=(x, x)), dict(vc=c), dict(u=x.to("meta"))):
        args = dict(centres=c, x=x, y=x, z=x, m=x, box=box, edges=e)
        with pytest.raises(ValueError):
            radial_profiles(**{**args, **bad})
    monkeypatch.setenv("SPHX_PROFILE_SEGMENT", "100")
    with pytest.raises(ValueError):
        radial_profiles(c, x, x, x, x, box, e)


@pytest.mark.parametrize("device", ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)])
def test_simulation_group_profiles(device):
    from sphexa_amd.app.simulation import Simulation

    sim = Simulation("evrard", n=20, prop="std", device=device).run(3)
    d, first, last = sim.d, sim.domain.start_index(), sim.domain.end_index()
    _, cat, _ = sim.find_groups(b=0.5, min_members=5, bound=True)
    edges = np.geomspace(0.02, 0.4, 9)
    out = sim.group_profiles(cat, edges, overdensity=(200.0, 500.0))
    assert out["count"].shape == (cat["label"].numel(), 8) and int(out["so_count"][0, 0]) > 0
    lx, ly, lz = sim.domain.box.lengths()
    own = lambda f: d[f][first:last].double().cpu().numpy()
    rho_ref = float(d["m"][first:last].sum(dtype=torch.float64)) / (lx * ly * lz)
    cen = torch.where(cat["centre"].isnan(), cat["com"], cat["centre"]).cpu().numpy()
    ref = _oracle(dict(pos=np.stack([own("x"), own("y"), own("z")], axis=1), centres=cen[:1], box=sim.domain.box,
                       edges=edges, m=own("m"), v=None, vc=None, u=None, rho=[200.0 * rho_ref, 500.0 * rho_ref],
                       select=None, first=0, last=last - first))
    assert np.array_equal(out["so_count"][:1].cpu().numpy(), ref["so_count"])
    assert (np.abs(out["so_mass"][:1].cpu().numpy() - ref["so_mass"]) <= ref["so_mass_bound"]).all()


def test_tools_fof_so(tmp_path, monkeypatch):
    """``tools fof --so`` on a 500-particle periodic dump, host path: the table round-trips the op's SO columns, and
    without ``--so`` the catalogue stays byte for byte what it was"""
    from sphexa_amd.ops.fof import fof_catalog, fof_labels
    from sphexa_amd.tools.__main__ import _read, main

    monkeypatch.chdir(tmp_path)
    main(["init-file", "dump.h5", "-n", "500", "--seed", "3"])
    common = ["fof", "dump.h5", "--b", "0.6", "--min-members", "3", "--device", "cpu"]
    main(common + ["-o", "plain.txt"])
    main(common + ["-o", "so.txt", "--so", "50,200", "--so-rmax", "0.2", "--profile-bins", "4", "--profiles-out",
                   "p.txt"])
    d = {k: torch.as_tensor(a, dtype=torch.float64) for k, a in
         _read("dump.h5", None, ["x", "y", "z", "m", "vx", "vy", "vz"]).items()}
    box, v = Box.cube(0.0, 1.0, PERIODIC), (d["vx"], d["vy"], d["vz"])
    labels = fof_labels(d["x"], d["y"], d["z"], box, 0.6 * 500 ** (-1 / 3))
    cat = fof_catalog(labels, d["x"], d["y"], d["z"], d["m"], box, 3, v=v)
    prof = radial_profiles(cat["com"], d["x"], d["y"], d["z"], d["m"], box, np.geomspace(0.002, 0.2, 5), v=v,
                           vc=cat["vel"], thresholds=[50.0 * float(d["m"].sum()), 200.0 * float(d["m"].sum())])
    plain, table = np.loadtxt("plain.txt", ndmin=2), np.loadtxt("so.txt", ndmin=2)
    want = torch.cat([torch.stack([prof["so_radius"][:, k], prof["so_mass"][:, k], prof["so_count"][:, k].double(),
                                   prof["so_truncated"][:, k].double()], dim=1) for k in range(2)], dim=1).numpy()
    assert len(table) > 0 and np.array_equal(table[:, :9], plain) and np.array_equal(table[:, 9:], want, equal_nan=True)
    assert np.loadtxt("p.txt", ndmin=2).shape == (4 * len(table), 9)
    lines = lambda f: [ln for ln in open(f).read().splitlines()]
    assert lines("plain.txt")[0].startswith("# label count mass cx cy cz vx vy vz  (linking length ")
    assert lines("plain.txt")[1:] == [" ".join(ln.split()[:9]) for ln in lines("so.txt")[1:]]
