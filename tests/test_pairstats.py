"""Pair statistics (ops/pairstats.py) against a dense fp64 oracle: all pairs i < j of the N x N minimum-image separation
matrix, d2 = (dx dx + dy dy) + dz dz, binned by e_k^2 <= d2 < e_{k+1}^2. Every row checks on its own inputs that no pair
lies within 1e-12 of an edge, so the bins are unambiguous in fp64. Counts must be exactly the oracle's; a value channel
must be within count_k q_c + 16 2^-53 sum |terms| per bin: half a quantum per term, the fp64 rounding of a term, and
the conversion of the integer sum to a double."""

import functools

import numpy as np
import pytest
import torch

import sphexa_amd.ops.pairstats as ps
from sphexa_amd.ops.pairstats import correlation_function, pair_statistics, structure_functions
from sphexa_amd.utils.box import OPEN, PERIODIC, Box

ROWS = ["band", "axes-x", "axes-y", "axes-z", "wrap", "dense", "random", "select", "counts-only", "one-bin", "64-bins"]
SHARED = ("select", "counts-only", "one-bin", "64-bins")  # rows on the particles of "random"
CHANNELS = ("ww", "dl1", "dl2", "dl3", "dv2")


def _oracle(pos, box, edges, select, w, v):
    """(count, sums, sums of |terms|) per bin; sums: dict over CHANNELS"""
    n = len(pos)
    i, j = np.nonzero(np.triu(np.ones((n, n), dtype=bool), 1) & select[:, None] & select[None, :])
    d = pos[j] - pos[i]
    for a in range(3):
        if box.bc[a] == PERIODIC:
            L = box.hi[a] - box.lo[a]
            d[:, a] -= L * np.rint(d[:, a] * (1.0 / L))
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    e2, nb = edges * edges, len(edges) - 1
    near = d2 < 2.0 * e2[-1]  # (the others are in no bin and near no edge)
    i, j, d, d2 = i[near], j[near], d[near], d2[near]
    k = np.searchsorted(e2, d2, side="right") - 1
    for e in (e2[np.clip(k, 0, nb)], e2[np.clip(k + 1, 0, nb)]):  # the edges on either side of every pair
        assert not (np.abs(d2 / np.where(e > 0, e, 1.0) - 1.0) < 1e-12)[e > 0].any(), "a pair too close to an edge"
    ok = (k >= 0) & (k < nb)
    dv = v[j] - v[i]
    u = ((dv[:, 0] * d[:, 0] + dv[:, 1] * d[:, 1]) + dv[:, 2] * d[:, 2]) / np.sqrt(np.where(d2 > 0, d2, 1.0))
    terms = dict(ww=w[i] * w[j], dl1=u, dl2=u * u, dl3=u * u * u,
                 dv2=(dv[:, 0] * dv[:, 0] + dv[:, 1] * dv[:, 1]) + dv[:, 2] * dv[:, 2])
    hist = lambda t: np.bincount(k[ok], weights=t[ok], minlength=nb)
    return (np.bincount(k[ok], minlength=nb), {c: hist(t) for c, t in terms.items()},
            {c: hist(np.abs(t)) for c, t in terms.items()})


@functools.lru_cache(maxsize=None)
def _row(name):
    """(pos, box, edges, select, w, v, with values, oracle) of a row; computed once, shared by host and device tests"""
    rng = np.random.default_rng(ROWS.index("random" if name in SHARED else name))
    box, select = Box.cube(0.0, 1.0, PERIODIC), None
    if name == "band":  # pairs at r / e_k = 1 -+ 1e-9 for every edge: fp32 cannot tell them apart
        edges = np.array([0.02, 0.05, 0.1, 0.2])
        base = rng.random((8, 3))
        u = rng.normal(size=(8, 3))
        u /= np.linalg.norm(u, axis=1)[:, None]
        r = np.repeat(edges, 2) * (1.0 + 1e-9 * np.tile([1.0, -1.0], 4))
        pos = np.concatenate([base, (base + u * r[:, None]) % 1.0, rng.random((200, 3))])
    elif name in ("axes-x", "axes-y", "axes-z", "wrap"):  # 4.76, 6.19 and 4.28 cells of r_max
        bc = [PERIODIC if name == "wrap" or name[-1] == c else OPEN for c in "xyz"]
        box, edges = Box([0.0, -0.3, 0.1], [1.0, 1.0, 1.0], bc), np.array([0.0, 0.03, 0.08, 0.15, 0.21])
        L = np.array(box.lengths())
        corner = (rng.normal(size=(12, 3)) * 0.02) % L  # a clump across the box corner
        pos = np.array(box.lo) + np.concatenate([rng.random((288, 3)) * L, corner])
    elif name == "dense":  # 701 particles in one cell (11 items, 11 source chunks), 100 in the next, a coincident pair
        box, edges = Box.cube(0.0, 1.0, OPEN), np.array([0.0, 0.01, 0.03, 0.06, 0.1])

        def ball(k, radius):
            p = rng.normal(size=(k, 3))
            return p / np.linalg.norm(p, axis=1)[:, None] * radius * rng.random((k, 1)) ** (1 / 3)

        c1 = np.array([0.4, 0.5, 0.5])
        pos = np.concatenate([c1 + ball(700, 0.04), c1 + [0.12, 0.0, 0.0] + ball(100, 0.03)])
        pos = np.concatenate([pos, pos[:1]])
    else:
        pos = rng.random((3000, 3))
        edges = {"one-bin": np.array([0.05, 0.15]), "64-bins": np.linspace(0.01, 0.15, 65)}.get(
            name, np.geomspace(0.005, 0.15, 17))
        if name == "select":
            select = rng.random(3000) > 0.15
    n = len(pos)
    select = np.ones(n, dtype=bool) if select is None else select
    w = (0.5 + np.random.default_rng(99).random(n)).astype(np.float32)
    v = np.random.default_rng(98).normal(size=(n, 3)).astype(np.float32)
    return (pos, box, edges, select, w, v, name != "counts-only",
            _oracle(pos, box, edges, select, w.astype(np.float64), v.astype(np.float64)))


def _run(name, device):
    pos, box, edges, select, w, v, values, _ = _row(name)
    t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt).to(device)
    x, y, z = (t(pos[:, a], torch.float64) for a in range(3))
    return pair_statistics(x, y, z, box, edges, w=t(w, torch.float32) if values else None,
                           v=tuple(t(v[:, a], torch.float32) for a in range(3)) if values else None,
                           select=None if select.all() else t(select, torch.bool))


def _check(name, got, other=None):
    """``got`` against the oracle, or (factor 2 on the bound) against the result ``other`` of the other path"""
    count, sums, sums_abs = _row(name)[-1]
    assert np.array_equal(got["count"].cpu().numpy(), count)
    assert set(got) == {"count", "quantum", "pairs_bound"} | (set(CHANNELS) if _row(name)[6] else set())
    assert got["pairs_bound"] >= count.max()
    ratio = 0.0
    for c in got["quantum"]:
        bound = count * got["quantum"][c] + 16.0 * 2.0 ** -53 * sums_abs[c]
        ref = sums[c] if other is None else other[c].cpu().numpy()
        err = np.abs(got[c].cpu().numpy() - ref)
        ratio = max(ratio, np.max(err / np.maximum(bound, 1e-300)))
        assert (err <= (1 if other is None else 2) * bound).all(), c
    print(f"{name}: {count.sum()} pairs, largest error / bound {ratio:.3f}")


@pytest.mark.parametrize("name", ROWS)
def test_cpu_rows(name):
    _check(name, _run(name, "cpu"))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ROWS)
def test_gpu_rows(name):
    got, again, host = _run(name, "cuda"), _run(name, "cuda"), _run(name, "cpu")
    _check(name, got)
    assert got["quantum"] == again["quantum"] and got["pairs_bound"] == again["pairs_bound"]
    assert all(torch.equal(got[k], again[k]) for k in got if torch.is_tensor(got[k]))  # bit-identical
    assert torch.equal(got["count"].cpu(), host["count"])
    _check(name, got, other=host)


def test_rejects_wrong_inputs(monkeypatch):
    x = torch.rand(40, dtype=torch.float64)
    box, good = Box.cube(0.0, 1.0, PERIODIC), np.array([0.0, 0.1, 0.2])
    f32 = x.to(torch.float32)
    bad = [dict(edges=np.array([0.0, 0.2, 0.1])), dict(edges=np.linspace(0.0, 0.3, 67)),
           dict(edges=np.array([-0.1, 0.1])), dict(edges=np.array([0.0, 0.34])),  # r_max > L / 3
           dict(edges=good.astype(np.float32)), dict(edges=good, x=f32), dict(edges=good, w=torch.arange(40)),
           dict(edges=good, select=torch.ones(40))]
    for kw in bad:
        with pytest.raises(ValueError):
            pair_statistics(kw.pop("x", x), x, x, box, **kw)
    assert pair_statistics(x, x, x, box, good)["count"].sum() > 0
    monkeypatch.setattr(ps, "MAX_PAIRS_BOUND", 10)
    with pytest.raises(ValueError, match="select"):
        pair_statistics(x, x, x, box, good)


def test_derived():
    # positions and velocities are small multiples of 2^-10: v = Omega x r and v = H r are exact in fp32, dv . d is
    # exact in fp64, so a rigid rotation has u == 0 in every pair
    rng = np.random.default_rng(5)
    r = torch.as_tensor(rng.integers(0, 1024, (300, 3)) / 1024.0)
    box, edges = Box.cube(0.0, 1.0, OPEN), np.array([0.05, 0.1, 0.2, 0.3])
    om = torch.tensor([1.0, 2.0, -1.0], dtype=torch.float64)
    for kind, vel in (("rotation", torch.linalg.cross(om.expand(300, 3), r)), ("expansion", 0.5 * r)):
        st = pair_statistics(*r.T.contiguous(), box, edges, v=tuple(vel.T.to(torch.float32).contiguous()))
        sf, cnt = structure_functions(st), st["count"].double()
        assert (cnt > 0).all()
        if kind == "rotation":
            assert (sf["S1L"] == 0).all() and (st["dl2"].abs() <= cnt * st["quantum"]["dl2"]).all()
        else:  # u = H |d|: S1L lies in H [e_k, e_k+1), the transverse part vanishes up to the roundings of u^2
            e = torch.as_tensor(edges)
            assert (sf["S1L"] >= 0.5 * e[:-1]).all() and (sf["S1L"] < 0.5 * e[1:]).all()
            bound = cnt * (st["quantum"]["dl2"] + st["quantum"]["dv2"]) + 32.0 * 2.0 ** -53 * st["dv2"]
            assert ((st["dv2"] - st["dl2"]).abs() <= bound).all() and (sf["S2T"].abs() <= bound).all()
    with pytest.raises(ValueError):
        correlation_function(st, edges, 300, box)
    # Poisson at four sigma on the uniform row (seed checked against the oracle alone first: largest
    # |xi| sqrt(count) / 4 over the bins is 0.37)
    pos, pbox, pedges, _, _, _, _, (count, _, _) = _row("counts-only")
    xi = correlation_function(dict(count=torch.as_tensor(count)), pedges, len(pos), pbox).numpy()
    assert (np.abs(xi[count > 0]) <= 4.0 / np.sqrt(count[count > 0])).all()


@pytest.mark.parametrize("device", ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)])
def test_simulation_and_tool(device, tmp_path, monkeypatch):
    from sphexa_amd.app.simulation import Simulation
    from sphexa_amd.tools.__main__ import _read, main

    sim = Simulation("turbulence", n=16, device=device).run(2)
    d, first, last = sim.d, sim.domain.start_index(), sim.domain.end_index()
    edges = np.geomspace(0.02, 0.2, 9) * sim.domain.box.lengths()[0]
    got = sim.pair_statistics(edges, fields="velocity", stride=2)
    every = (torch.arange(d["x"].numel(), device=d["x"].device) - first) % 2 == 0
    ref = pair_statistics(d["x"], d["y"], d["z"], sim.domain.box, edges, v=(d["vx"], d["vy"], d["vz"]), select=every,
                          first=first, last=last)
    assert got["count"].sum() > 0 and got["quantum"] == ref["quantum"]
    assert all(torch.equal(got[k], ref[k]) for k in ref if torch.is_tensor(ref[k]))

    monkeypatch.chdir(tmp_path)
    main(["init-file", "dump.h5", "-n", "500", "--seed", "3"])
    main(["pairs", "dump.h5", "--rmin", "0.01", "--rmax", "0.3", "--bins", "6", "--log", "--velocity", "--mass",
          "--device", device])
    t = {k: torch.as_tensor(a, dtype=torch.float64).to(device) for k, a in
         _read("dump.h5", None, ["x", "y", "z", "m", "vx", "vy", "vz"]).items()}
    box, e = Box.cube(0.0, 1.0, PERIODIC), np.geomspace(0.01, 0.3, 7)
    st = pair_statistics(t["x"], t["y"], t["z"], box, e, w=t["m"], v=(t["vx"], t["vy"], t["vz"]))
    sf = structure_functions(st)
    want = torch.stack([c.cpu() for c in (torch.as_tensor(e[:-1]), torch.as_tensor(e[1:]), st["count"].double(),
                                          st["ww"], sf["S2L"], sf["S2T"], sf["S3L"],
                                          correlation_function(st, e, 500, box))], dim=1).numpy()
    assert np.array_equal(np.loadtxt("pairs.txt", ndmin=2), want, equal_nan=True)  # (17 digits round-trip a double)
