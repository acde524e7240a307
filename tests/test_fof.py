"""Friends-of-friends groups (ops/fof.py) against a dense fp64 oracle: the all-pairs minimum-image distance matrix,
d^2 <= b^2, and a plain union-find over its edge list; labels are the component minima. Every row checks on its own
inputs that no pair lies within 1e-12 of d^2 = b^2, so the link set is unambiguous in fp64. Labels must be exactly
the oracle's; catalogue sums must be within the bound of an ordered fp64 sum against numpy's,
2 n_g 2^-53 sum |terms| (for com the terms are the root coordinate, the m d / M and the periodic wrap)."""

import functools

import numpy as np
import pytest
import torch

from sphexa_amd.ops.fof import fof_catalog, fof_labels
from sphexa_amd.utils.box import OPEN, PERIODIC, Box

ROWS = ["band", "axes-x", "axes-y", "axes-z", "wrap", "chain", "dense", "dense-bridge", "random", "select"]


def _min_image(d, box):
    for a in range(3):
        if box.bc[a] == PERIODIC:
            L = box.hi[a] - box.lo[a]
            d[..., a] -= L * np.rint(d[..., a] * (1.0 / L))
    return d


def _oracle(pos, box, b, select):
    n = len(pos)
    d = _min_image(pos[:, None, :] - pos[None, :, :], box)
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    assert not (np.abs(d2 / (b * b) - 1.0) < 1e-12).any(), "a pair too close to d = b: the row is ambiguous"
    link = np.triu(d2 <= b * b, 1) & select[:, None] & select[None, :]
    parent = np.arange(n)

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    for i, j in zip(*np.nonzero(link)):
        ri, rj = find(i), find(j)
        parent[max(ri, rj)] = min(ri, rj)  # the smaller index stays the root: roots are component minima
    return np.where(select, [find(i) for i in range(n)], -1).astype(np.int32)


@functools.lru_cache(maxsize=None)
def _row(name):
    """(pos, box, b, select, m, v, oracle labels) of a row; computed once and shared by the host and device tests"""
    rng = np.random.default_rng(ROWS.index(name.replace("select", "random")))
    box, select = Box.cube(0.0, 1.0, PERIODIC), None
    if name == "band":  # pairs at d / b = 1 -+ 1e-9 near the box centre: fp32 cannot tell them apart
        b = 0.05
        base = 0.5 + 0.2 * np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0], [0, 1, 1]], dtype=float)
        u = rng.normal(size=(6, 3))
        u /= np.linalg.norm(u, axis=1)[:, None]
        scale = b * (1.0 + 1e-9 * np.array([1, -1, 1, -1, -1, 1]))
        pos = np.concatenate([base, base + u * scale[:, None]])
    elif name in ("axes-x", "axes-y", "axes-z", "wrap"):  # 29.4, 38.3 and 26.6 cells of b / sqrt 3
        bc = [PERIODIC if name == "wrap" or name[-1] == c else OPEN for c in "xyz"]
        box, b = Box([0.0, -0.3, 0.1], [1.0, 1.0, 1.0], bc), 0.059
        L = np.array(box.lengths())
        corner = (rng.normal(size=(12, 3)) * 0.02) % L  # a group across the box corner
        pos = np.array(box.lo) + np.concatenate([rng.random((288, 3)) * L, corner])
    elif name == "chain":  # a helix of steps 0.9 b with one step of 1.1 b, in shuffled index order
        box, b = Box.cube(-1.0, 1.0, OPEN), 0.02
        phi = np.arange(599) * (2 * np.pi / 70)
        u = np.stack([-np.sin(phi), np.cos(phi), np.full(599, 0.06)], axis=1)
        step = np.where(np.arange(599) == 300, 1.1, 0.9) * b
        pos = np.concatenate([np.zeros((1, 3)), np.cumsum(u / np.linalg.norm(u, axis=1)[:, None] * step[:, None], 0)])
        pos = pos[rng.permutation(600)]
    elif name in ("dense", "dense-bridge"):  # a ball of radius 0.4 b (cells of > 64), a clump 1.5 b off its surface
        box, b = Box.cube(0.0, 1.0, OPEN), 0.1

        def ball(k, radius):
            p = rng.normal(size=(k, 3))
            return p / np.linalg.norm(p, axis=1)[:, None] * radius * rng.random((k, 1)) ** (1 / 3)

        c1, c2 = np.array([0.4, 0.5, 0.5]), np.array([0.4 + 2.2 * b, 0.5, 0.5])
        pos = np.concatenate([c1 + ball(700, 0.4 * b), c2 + ball(100, 0.3 * b)])
        if name == "dense-bridge":
            pos = np.concatenate([pos, [0.5 * (c1 + c2)]])
    else:  # random, select: singletons, small groups and large ones
        pos, b = rng.random((3000, 3)), 0.8 * 3000 ** (-1 / 3)
        if name == "select":
            select = rng.random(3000) > 0.15
    n = len(pos)
    select = np.ones(n, dtype=bool) if select is None else select
    m = (0.5 + rng.random(n)).astype(np.float32)
    v = rng.normal(size=(n, 3)).astype(np.float32)
    return pos, box, b, select, m, v, _oracle(pos, box, b, select)


def _reference_catalog(name, min_members):
    """numpy catalogue of the oracle's labels and the bound of every entry: rows of (label, count, values, bounds)"""
    pos, box, b, select, m, v, labels = _row(name)
    m, v, out = m.astype(np.float64), v.astype(np.float64), []
    for lab in np.unique(labels[labels >= 0]):
        idx = np.nonzero(labels == lab)[0]
        if len(idx) < min_members:
            continue
        M, eps = m[idx].sum(), 2.0 * len(idx) * 2.0 ** -53
        md = m[idx, None] * _min_image(pos[idx] - pos[lab], box)
        com = pos[lab] + md.sum(0) / M
        per = np.array(box.bc) == PERIODIC
        wrapped = np.where(per & (com > box.hi), com - box.lengths(), np.where(per & (com < box.lo),
                                                                               com + box.lengths(), com))
        mv = m[idx, None] * v[idx]
        vals = np.concatenate([[M], wrapped, mv.sum(0) / M])
        bounds = eps * np.concatenate([[M], np.abs(pos[lab]) + np.abs(md).sum(0) / M + np.abs(wrapped - com),
                                       np.abs(mv).sum(0) / M])
        out.append((int(lab), len(idx), vals, bounds))
    return sorted(out, key=lambda g: (-g[1], g[0]))


def _run(name, device):
    pos, box, b, select, m, v, _ = _row(name)
    t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt).to(device)
    x, y, z = (t(pos[:, a], torch.float64) for a in range(3))
    sel = None if select.all() else t(select, torch.bool)
    labels = fof_labels(x, y, z, box, b, select=sel)
    cats = [fof_catalog(labels, x, y, z, t(m, torch.float32), box, min_members=k,
                        v=tuple(t(v[:, a], torch.float32) for a in range(3))) for k in (1, 20)]
    return labels, cats


def _check(name, labels, cats):
    assert np.array_equal(labels.cpu().numpy(), _row(name)[-1])
    for k, cat in zip((1, 20), cats):
        ref = _reference_catalog(name, k)
        assert cat["label"].tolist() == [g[0] for g in ref] and cat["count"].tolist() == [g[1] for g in ref]
        got = torch.cat([cat["mass"][:, None], cat["com"], cat["vel"]], dim=1).cpu().numpy()
        if ref:
            err, bound = np.abs(got - np.stack([g[2] for g in ref])), np.stack([g[3] for g in ref])
            ratio = np.max(err / np.maximum(bound, 1e-300))
            print(f"{name} min_members {k}: {len(ref)} groups, largest error / bound {ratio:.3f}")
            assert (err <= bound).all()


@pytest.mark.parametrize("name", ROWS)
def test_cpu_rows(name):
    _check(name, *_run(name, "cpu"))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ROWS)
def test_gpu_rows(name):
    labels, cats = _run(name, "cuda")
    _check(name, labels, cats)
    again, cats2 = _run(name, "cuda")
    host, _ = _run(name, "cpu")
    assert torch.equal(labels, again) and torch.equal(labels.cpu(), host)
    for a, b in zip(cats, cats2):
        assert all(torch.equal(a[k], b[k]) for k in a)  # bit-identical from run to run


def test_rejects_wrong_inputs():
    x = torch.rand(10, dtype=torch.float64)
    box = Box.cube(0.0, 1.0, PERIODIC)
    for b in (0.0, -1.0, 1e-8, 0.5):  # not positive, more than 2^21 cells, a periodic axis shorter than the stencil
        with pytest.raises(ValueError):
            fof_labels(x, x, x, box, b)
    assert fof_labels(x, x, x, box, 0.1, select=torch.zeros(10, dtype=torch.bool)).tolist() == [-1] * 10


@pytest.mark.parametrize("device", ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)])
def test_simulation_find_groups(device):
    from sphexa_amd.app.simulation import Simulation

    sim = Simulation("evrard", n=20, prop="std", device=device).run(3)  # (std: holds rho)
    d, first, last = sim.d, sim.domain.start_index(), sim.domain.end_index()
    rho_min = float(d["rho"][first:last].median())
    labels, cat = sim.find_groups(b=0.5, rho_min=rho_min, min_members=5)
    lx, ly, lz = sim.domain.box.lengths()
    ll = 0.5 * (lx * ly * lz / d.numParticlesGlobal) ** (1 / 3)
    ref = fof_labels(d["x"], d["y"], d["z"], sim.domain.box, ll, select=d["rho"] >= rho_min, first=first, last=last)
    own = lambda f: d[f][first:last]
    ref_cat = fof_catalog(ref, own("x"), own("y"), own("z"), own("m"), sim.domain.box, min_members=5,
                          v=(own("vx"), own("vy"), own("vz")))
    assert torch.equal(labels, ref) and (labels >= 0).any() and (labels < 0).any() and cat["count"].numel() > 0
    assert all(torch.equal(cat[k], ref_cat[k]) for k in ref_cat)
    with pytest.raises(ValueError):
        sim.find_groups(linking_length=0.0)


def test_tools_fof(tmp_path, monkeypatch):
    """``tools fof`` on a 500-particle periodic dump, host path: the text catalogue and the labels are the ops' own"""
    from sphexa_amd.tools.__main__ import _read, main

    monkeypatch.chdir(tmp_path)
    main(["init-file", "dump.h5", "-n", "500", "--seed", "3"])
    main(["fof", "dump.h5", "--b", "0.6", "--min-members", "3", "--device", "cpu", "--labels", "labels.npy"])
    d = {k: torch.as_tensor(a, dtype=torch.float64) for k, a in
         _read("dump.h5", None, ["x", "y", "z", "m", "vx", "vy", "vz"]).items()}
    box = Box.cube(0.0, 1.0, PERIODIC)
    labels = fof_labels(d["x"], d["y"], d["z"], box, 0.6 * 500 ** (-1 / 3))
    cat = fof_catalog(labels, d["x"], d["y"], d["z"], d["m"], box, min_members=3, v=(d["vx"], d["vy"], d["vz"]))
    table = np.loadtxt("groups.txt", ndmin=2)
    assert np.array_equal(np.load("labels.npy"), labels.numpy()) and len(table) == cat["label"].numel() > 0
    want = torch.cat([cat["label"][:, None].double(), cat["count"][:, None].double(), cat["mass"][:, None], cat["com"],
                      cat["vel"]], dim=1).numpy()
    assert np.array_equal(table, want)  # (17 significant digits: the text round-trips the doubles)
