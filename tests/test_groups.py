"""Bound groups (ops/groups.py) against a dense fp64 oracle: per group the n_g x n_g matrix of the Plummer terms over
the fp32-rounded offsets from the label particle, and a Python unbinding loop (definitions: sphx/groups.hpp).

phi of every bound member must lie within B_i = 2^-24 (71 + 2 D_g / eps) |phi_ref,i| on the device (the derivation is
next to the definitions in sphx/groups.hpp; D_g the group's largest offset norm) and within 2 n_g 2^-53 |phi_ref,i| on
the host. Bound sets, counts, iterations, most_bound and the index behind centre must be exactly the oracle's: the
oracle asserts on every row, at every iteration and for every member |e_i| > 8 B_i, and that the two lowest phi and e
of a group lie more than 2 B apart, so no rounding of either path can flip a member. Catalogue sums carry ordered-fp64
bounds, epot in addition the phi bound summed with the masses."""

import functools

import numpy as np
import pytest
import torch

from sphexa_amd.ops.groups import bound_groups
from sphexa_amd.utils.box import OPEN, PERIODIC, Box

ROWS = ["pair", "edges", "segments", "coincident", "wrap", "unbind", "dissolve", "thermal"]
U24, U53 = 2.0 ** -24, 2.0 ** -53


def _ball(rng, k, sigma):
    return rng.normal(size=(k, 3)) * sigma


@functools.lru_cache(maxsize=None)
def _row(name):
    """inputs of a row: pos, box, labels, m, v, u, eps, min_members, max_iter, segment; computed once and shared"""
    rng = np.random.default_rng(ROWS.index(name.split("-")[0].replace("thermal", "unbind")) + 11)
    box, u, eps, min_members, max_iter, segment, vel = Box.cube(0.0, 1.0, OPEN), None, 0.005, 2, 20, None, None
    if name == "pair":  # a group of 2, a singleton below min_members and a particle that is left out
        pos, gid = np.array([[0.2, 0.2, 0.2], [0.23, 0.24, 0.2], [0.7, 0.7, 0.7], [0.5, 0.5, 0.5]]), [0, 0, 1, -1]
    elif name in ("edges", "segments"):  # clumps of the sizes at which a tile, a chunk or a segment ends
        sizes = [63, 64, 65, 127, 128, 129] if name == "edges" else [600] + list(rng.integers(2, 51, size=40))
        centres = 0.1 + 0.8 * rng.random((len(sizes), 3))
        pos = np.concatenate([c + _ball(rng, k, 0.01) for c, k in zip(centres, sizes)])
        gid = np.repeat(np.arange(len(sizes)), sizes)
        segment = 128 if name == "segments" else None
    elif name == "coincident":  # two members at one position, one member at D / eps = 2^10 from the root
        eps, max_iter = 1e-4, 0
        pos = 0.5 + np.concatenate([np.zeros((1, 3)), _ball(rng, 29, 0.002), [[1024 * eps, 0, 0]]])
        pos[7] = pos[3]
        gid = np.zeros(31, dtype=int)
    elif name in ("wrap", "wrap-open"):  # a group across the corner of a periodic box with unequal edges
        box = Box([0.0, -0.3, 0.1], [1.0, 1.0, 1.0], [PERIODIC] * 3)
        L, off = np.array(box.lengths()), _ball(rng, 100, 0.02)
        pos, gid = np.array(box.lo) + off % L, np.zeros(100, dtype=int)
        if name == "wrap-open":  # the same points in an open box, shifted to the middle
            box, pos = Box([0.0, -0.3, 0.1], [1.0, 1.0, 1.0], [OPEN] * 3), np.array(box.lo) + 0.5 * L + off
        vel = _ball(rng, 100, 4.0)  # some members leave
    elif name in ("unbind", "thermal"):  # a cold clump, interlopers above the escape speed, a drift on all
        min_members = 20
        pos = 0.5 + np.concatenate([_ball(rng, 300, 0.02), _ball(rng, 60, 0.02)])
        vel = np.concatenate([_ball(rng, 300, 0.5), [25.0, 0, 0] + _ball(rng, 60, 15.0)]) + [5.0, -3.0, 2.0]
        gid = np.zeros(360, dtype=int)
        if name == "thermal":
            u = np.where(rng.random(360) < 0.15, 80.0, 0.5)
    else:  # dissolve: a hot group, and a group of 25 that loses 8 and falls below min_members = 20
        min_members = 20
        pos = np.concatenate([0.3 + _ball(rng, 30, 0.02), 0.7 + _ball(rng, 25, 0.02)])
        vel = np.concatenate([_ball(rng, 30, 40.0), _ball(rng, 17, 0.3), _ball(rng, 8, 40.0)])
        gid = np.repeat([0, 1], [30, 25])
    n = len(pos)
    shuffle = rng.permutation(n) if name not in ("pair", "coincident") else np.arange(n)  # groups interleave
    pos, gid = pos[shuffle], np.asarray(gid)[shuffle]
    vel = (np.zeros((n, 3)) if vel is None else vel[shuffle]).astype(np.float32).astype(np.float64)
    u = None if u is None else u[shuffle]
    labels = np.array([-1 if g < 0 else np.nonzero(gid == g)[0][0] for g in gid], dtype=np.int32)
    m = ((0.5 + rng.random(n)) / n).astype(np.float32).astype(np.float64)
    return dict(pos=pos, box=box, labels=labels, m=m, v=vel, u=u, eps=eps, min_members=min_members,
                max_iter=max_iter, segment=segment)


@functools.lru_cache(maxsize=None)
def _oracle(name):
    """(bound, phi, B, iterations, groups): groups in catalogue order with the reference values and their bounds"""
    r = _row(name)
    pos, box, labels, m, v, eps = r["pos"], r["box"], r["labels"], r["m"], r["v"], r["eps"]
    n, u = len(pos), np.zeros(len(pos)) if r["u"] is None else r["u"]
    labs, counts = np.unique(labels[labels >= 0], return_counts=True)
    keep = counts >= r["min_members"]
    members = [np.nonzero(labels == lab)[0] for lab in labs[keep][np.lexsort((labs[keep], -counts[keep]))]]
    off = np.zeros((n, 3))
    for idx in members:
        d = pos[idx] - pos[idx[0]]
        for a in range(3):
            if box.bc[a] == PERIODIC:
                L = box.hi[a] - box.lo[a]
                d[:, a] -= L * np.rint(d[:, a] * (1.0 / L))
        off[idx] = d.astype(np.float32)
    iterations = 0
    while True:
        phi, e, B, V = np.full(n, np.nan), np.full(n, np.nan), np.zeros(n), []
        for idx in members:
            t = off[idx, None, :] - off[None, idx, :]
            w = m[idx][None, :] / np.sqrt((t[..., 0] ** 2 + t[..., 1] ** 2) + t[..., 2] ** 2 + eps * eps)
            np.fill_diagonal(w, 0.0)
            phi[idx] = -w.sum(1)  # G = 1
            D = np.linalg.norm(off[idx], axis=1).max() if len(idx) else 0.0
            B[idx] = U24 * (71.0 + 2.0 * D / eps) * np.abs(phi[idx])
            V.append((m[idx, None] * v[idx]).sum(0) / m[idx].sum() if len(idx) else np.full(3, np.nan))
            e[idx] = 0.5 * ((v[idx] - V[-1]) ** 2).sum(1) + u[idx] + phi[idx]
            for f in (phi[idx], e[idx]):  # the lowest member is unambiguous
                assert len(idx) < 2 or np.diff(np.sort(f)[:2])[0] > 2 * B[idx].max(), f"{name}: ambiguous minimum"
        if iterations == r["max_iter"]:
            break
        iterations += 1
        assert all((np.abs(e[idx]) > 8 * B[idx]).all() for idx in members), f"{name}: an energy too close to 0"
        new = [idx[e[idx] <= 0] for idx in members]
        new = [idx if len(idx) >= r["min_members"] else idx[:0] for idx in new]
        done = sum(map(len, new)) == sum(map(len, members))
        members = new
        if done:
            break
    groups = []
    for idx, Vg in zip(members, V):
        k, mi = len(idx), m[idx]
        w, s = v[idx] - Vg, (2 * len(idx) + 8) * U53
        dV = s * (np.abs(mi[:, None] * v[idx]).sum(0) / mi.sum()) if k else np.zeros(3)
        ek = 0.5 * mi * (w ** 2).sum(1)
        vals = dict(bound_mass=mi.sum(), vel=Vg, ekin=ek.sum(), eint=(mi * u[idx]).sum(), epot=0.5 * (mi * phi[idx]).sum())
        bnds = dict(bound_mass=s * mi.sum(), vel=dV, ekin=s * ek.sum() + (mi[:, None] * np.abs(w) * dV).sum(),
                    eint=s * (mi * u[idx]).sum(), epot=s * 0.5 * np.abs(mi * phi[idx]).sum())
        groups.append(dict(idx=idx, vals=vals, bnds=bnds, centre_index=idx[np.argmin(phi[idx])] if k else -1,
                           most_bound=idx[np.argmin(e[idx])] if k else -1))
    return ~np.isnan(phi), phi, B, iterations, groups


def _run(name, device, monkeypatch=None, segment="row"):
    r = _row(name)
    segment = r["segment"] if segment == "row" else segment
    if monkeypatch is not None and segment is not None:
        monkeypatch.setenv("SPHX_GROUP_SEGMENT", str(segment))
    t = lambda a, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(a), dtype=dt).to(device)
    x, y, z = (t(r["pos"][:, a]) for a in range(3))
    return bound_groups(t(r["labels"], torch.int32), x, y, z, t(r["m"], torch.float32),
                        tuple(t(r["v"][:, a], torch.float32) for a in range(3)), r["box"], r["eps"],
                        u=None if r["u"] is None else t(r["u"]), min_members=r["min_members"], max_iter=r["max_iter"])


def _check(name, out, device_bound):
    bound, phi, cat = out
    ref_bound, ref_phi, B, iterations, groups = _oracle(name)
    bound, phi = bound.cpu().numpy(), phi.cpu().numpy()
    assert np.array_equal(bound, ref_bound) and np.array_equal(np.isnan(phi), ~ref_bound)
    assert cat["iterations"] == iterations and cat["bound_count"].tolist() == [len(g["idx"]) for g in groups]
    assert cat["most_bound"].tolist() == [g["most_bound"] for g in groups]
    assert cat["centre_index"].tolist() == [g["centre_index"] for g in groups]
    ratio = 0.0
    for k, g in enumerate(groups):
        idx = g["idx"]
        if not len(idx):
            continue
        lim = B[idx] if device_bound else 2 * len(idx) * U53 * np.abs(ref_phi[idx])
        ratio = max(ratio, np.max(np.abs(phi[idx] - ref_phi[idx]) / lim))
        for key in ("bound_mass", "vel", "ekin", "eint", "epot"):
            extra = 0.5 * (_row(name)["m"][idx] * lim).sum() if key == "epot" else 0.0
            err = np.abs(cat[key][k].cpu().numpy() - g["vals"][key])
            assert (err <= g["bnds"][key] + extra).all(), (name, k, key, err, g["bnds"][key] + extra)
        want = _row(name)["pos"][g["centre_index"]]
        assert np.allclose(cat["centre"][k].cpu().numpy(), want, rtol=0, atol=0)
    print(f"{name}: {len(groups)} groups, {cat['iterations']} iterations, largest phi error / bound {ratio:.3f}")
    assert ratio <= 1.0
    return ratio


def _row_extras(name, out):
    bound, phi, cat = out
    r = _row(name)
    if name == "pair":
        d = np.linalg.norm((r["pos"][0] - r["pos"][1]).astype(np.float32).astype(np.float64))
        want = -r["m"][[1, 0]] / np.sqrt(d * d + r["eps"] ** 2)
        assert np.allclose(phi[:2].cpu().numpy(), want, rtol=1e-5, atol=0) and bound.tolist() == [True, True, False, False]
    if name == "unbind":
        assert cat["iterations"] >= 2 and 0 < int(cat["bound_count"][0]) < 360
    if name == "dissolve":
        assert cat["bound_count"].tolist() == [0, 0] and not bound.any()
    if name == "thermal":
        assert float(cat["eint"][0]) > 0 and int(cat["bound_count"][0]) < int(_oracle("unbind")[0].sum())


@pytest.mark.parametrize("name", ROWS)
def test_cpu_rows(name):
    out = _run(name, "cpu")
    _check(name, out, device_bound=False)
    _row_extras(name, out)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ROWS)
def test_gpu_rows(name, monkeypatch):
    out = _run(name, "cuda", monkeypatch)
    _check(name, out, device_bound=True)
    _row_extras(name, out)
    again, host = _run(name, "cuda"), _run(name, "cpu")
    assert torch.equal(out[0], again[0]) and torch.equal(out[1].nan_to_num(7.0), again[1].nan_to_num(7.0))
    assert all(torch.equal(torch.as_tensor(out[2][k]).nan_to_num(7.0), torch.as_tensor(again[2][k]).nan_to_num(7.0))
               for k in out[2])  # bit-identical from run to run
    assert torch.equal(out[0].cpu(), host[0])
    if name == "segments":  # the default segment: the same bound set, phi within the bound
        monkeypatch.delenv("SPHX_GROUP_SEGMENT")
        _check(name, _run(name, "cuda"), device_bound=True)
    if name == "wrap":  # the same points in an open box: both lie within B of the exact offsets' potential
        other = _run("wrap-open", "cuda")
        _check("wrap-open", other, device_bound=True)
        assert torch.equal(out[0], other[0])
        lim = torch.as_tensor(_oracle("wrap")[2] + _oracle("wrap-open")[2])
        assert ((out[1] - other[1]).abs().cpu()[out[0].cpu()] <= lim[out[0].cpu()]).all()


def test_rejects_wrong_inputs():
    x, lab, box = torch.rand(10, dtype=torch.float64), torch.zeros(10, dtype=torch.int32), Box.cube(0.0, 1.0, OPEN)
    ok = dict(eps=0.1, min_members=2)
    bound_groups(lab, x, x, x, x, (x, x, x), box, **ok)
    for bad in (dict(eps=0.0), dict(eps=-1.0), dict(max_iter=-1), dict(u=x[:5]), dict(u=x.to("meta"))):
        with pytest.raises(ValueError):
            bound_groups(lab, x, x, x, x, (x, x, x), box, **{**ok, **bad})
    for v in ((x, x, x[:5]), (x, x), (x, x, x.to("meta"))):
        with pytest.raises(ValueError):
            bound_groups(lab, x, x, x, x, v, box, **ok)


@pytest.mark.parametrize("device", ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)])
def test_simulation_find_groups(device):
    from sphexa_amd.app.simulation import Simulation

    sim = Simulation("evrard", n=20, prop="std", device=device).run(3)
    d, first, last = sim.d, sim.domain.start_index(), sim.domain.end_index()
    labels0, cat0 = sim.find_groups(b=0.5, min_members=5)
    labels, cat, bound = sim.find_groups(b=0.5, min_members=5, bound=True)
    assert torch.equal(labels, labels0) and all(torch.equal(cat[k], cat0[k]) for k in cat0)
    assert bound.any() and not (bound & (labels < 0)).any()
    lx, ly, lz = sim.domain.box.lengths()
    ll = 0.5 * (lx * ly * lz / d.numParticlesGlobal) ** (1 / 3)
    own = lambda f: d[f][first:last]
    ref = bound_groups(labels, own("x"), own("y"), own("z"), own("m"), (own("vx"), own("vy"), own("vz")),
                       sim.domain.box, 0.1 * ll, G=sim.d.g, min_members=5)
    assert torch.equal(bound, ref[0]) and torch.equal(cat["bound_count"], ref[2]["bound_count"])
    assert torch.equal(cat["epot"], ref[2]["epot"]) and cat["iterations"] == ref[2]["iterations"]


def test_tools_fof_bound(tmp_path, monkeypatch):
    """``tools fof --bound`` on a 500-particle periodic dump, host path: the text table round-trips the op's catalogue"""
    from sphexa_amd.tools.__main__ import _read, main
    from sphexa_amd.ops.fof import fof_catalog, fof_labels

    monkeypatch.chdir(tmp_path)
    main(["init-file", "dump.h5", "-n", "500", "--seed", "3"])
    main(["fof", "dump.h5", "--b", "0.6", "--min-members", "3", "--device", "cpu", "--bound", "--eps", "0.01", "--G",
          "2.0", "--max-iter", "5", "--bound-mask", "mask.npy"])
    d = {k: torch.as_tensor(a, dtype=torch.float64) for k, a in
         _read("dump.h5", None, ["x", "y", "z", "m", "vx", "vy", "vz"]).items()}
    box = Box.cube(0.0, 1.0, PERIODIC)
    labels = fof_labels(d["x"], d["y"], d["z"], box, 0.6 * 500 ** (-1 / 3))
    bound, _, cat = bound_groups(labels, d["x"], d["y"], d["z"], d["m"], (d["vx"], d["vy"], d["vz"]), box, 0.01, G=2.0,
                                 min_members=3, max_iter=5)
    table = np.loadtxt("groups.txt", ndmin=2)
    cat["all_vel"] = fof_catalog(labels, d["x"], d["y"], d["z"], d["m"], box, 3, v=(d["vx"], d["vy"], d["vz"]))["vel"]
    col = lambda k: cat[k].double().reshape(len(table), -1)
    want = torch.cat([col(k) for k in ("label", "count", "mass", "com", "all_vel", "bound_count", "bound_mass", "vel", "ekin",
                                       "eint", "epot", "centre", "most_bound")], dim=1).numpy()
    assert len(table) > 0 and np.array_equal(table, want, equal_nan=True)
    assert np.array_equal(np.load("mask.npy"), bound.numpy())
