"""Order-P far field over the Barnes-Hut interaction lists (csrc/hip/gravity_order.hip) against fp64.

The reference of a GPU evaluation is the sum of two fp64 parts over the lists the GPU itself built: the P2P part from
helpers/gravity_oracle.evaluate (node lists emptied; it brings its rounding budget Ba, Bphi) and the far field from
``m2p_oracle`` below (the three-term recurrence of sphx/multipole.hpp in numpy) on the fp32 moments of the GPU upsweep.
Bound per target: Ba_p2p + 4 eps_P Sa_m2p (+ the expanded-form term of the P = 4 tiles), eps_P from the oracle run in
float32 on the fp32 offsets of the node records; derivation and measured ratios: profiles/r12/multipole_order/README.md.
"""

import functools

import numpy as np
import pytest
import torch

from helpers import gravity_oracle as GO
from sphexa_amd.ops import _lib
from sphexa_amd.ops import gravity as G
from sphexa_amd.ops import octree as O
from sphexa_amd.ops import sfc
from sphexa_amd.utils.box import Box, OPEN

U = GO.U


def _terms(D):
    return [(nx, ny, d - nx - ny) for d in range(D) for nx in range(d, -1, -1) for ny in range(d - nx, -1, -1)]


def m2p_oracle(r, Q, P, dtype=np.float64):
    """phi (T, K), a (T, K, 3), |a| (T, K) of the raw moments Q (K, size) at separations r (T, K, 3) = target - centre:
    Taylor coefficients a_k of 1/|r - d| up to degree P by |k| r^2 a_k = (2|k| - 1) sum_i r_i a_{k - e_i}
    - (|k| - 1) sum_i a_{k - 2 e_i}, then phi = -sum Q_k a_k, a_i = -sum Q_k (k_i + 1) a_{k + e_i}"""
    r, Q = r.astype(dtype), Q.astype(dtype)
    terms = _terms(P + 1)
    at = {(0, 0, 0): 1 / np.sqrt((r * r).sum(-1))}
    inv2 = at[0, 0, 0] * at[0, 0, 0]
    for k in terms[1:]:
        d = sum(k)
        low = lambda i, s: at[tuple(k[j] - s * (i == j) for j in range(3))]
        s1 = sum(r[..., i] * low(i, 1) for i in range(3) if k[i] > 0)
        s2 = sum((low(i, 2) for i in range(3) if k[i] > 1), dtype(0))
        at[k] = (dtype(2 * d - 1) * s1 - dtype(d - 1) * s2) * inv2 / dtype(d)
    phi, a = 0, [0, 0, 0]
    for j, k in enumerate(_terms(P)):
        q = Q[None, :, j]
        phi = phi - q * at[k]
        for i in range(3):
            up = tuple(k[j2] + (i == j2) for j2 in range(3))
            a[i] = a[i] - q * dtype(up[i]) * at[up]
    a = np.stack(a, -1)
    return phi, a, np.sqrt((a.astype(np.float64) ** 2).sum(-1))


def test_oracle_matches_openmp_m2p():
    rng = np.random.default_rng(3)
    for P in range(1, 7):
        Q = rng.normal(size=(1, G.multipole_size(P)))
        r = rng.normal(size=3) * 3
        ref = np.array(_lib.cpu().multipole_m2p(P, *r, Q.ctypes.data))
        phi, a, _ = m2p_oracle(r[None, None, :], Q, P)
        assert np.allclose(np.concatenate([phi.ravel(), a.ravel()]), ref, rtol=1e-12, atol=0)


def _points(name):
    if name == "U":
        rng = np.random.default_rng(21)
        return rng.uniform(0, 1, (2000, 3)), np.ones(2000), 16, 0.5
    if name == "C":
        rng = np.random.default_rng(22)
        parts = [rng.uniform(0, 1, (100, 3))]
        for c in ([0.3, 0.3, 0.4], [0.7, 0.65, 0.6]):  # uniform radii: density ~ 1 / r^2
            v = rng.normal(size=(700, 3))
            parts.append(c + rng.uniform(0, 0.12, (700, 1)) * v / np.linalg.norm(v, axis=1, keepdims=True))
        return np.concatenate(parts), 10.0 ** rng.uniform(0, 1, 1500), 8, 0.8
    n = int(name[1:])  # "T<n>": n points at bucket 1
    return np.random.default_rng(30 + n).uniform(0, 1, (n, 3)), np.ones(n), 1, 0.5


@functools.lru_cache(maxsize=None)
def _case(name):
    X, m, bucket, theta = _points(name)
    box = Box([float(X[:, k].min()) - 1e-9 for k in range(3)], [float(X[:, k].max()) + 1e-9 for k in range(3)],
              [OPEN] * 3)
    x, y, z = (torch.from_numpy(X[:, k].copy()) for k in range(3))
    s, p = sfc.sort_keys(sfc.compute_keys(x, y, z, box))
    p = p.long()
    x, y, z = x[p].contiguous(), y[p].contiguous(), z[p].contiguous()
    m = torch.from_numpy((m / m.sum()).astype(np.float32))[p].contiguous()
    tree, counts = O.update_tree(None, s, bucket)
    return dict(n=X.shape[0], box=box, theta=theta, ot=O.build_octree(tree, counts, s, x, y, z), x=x, y=y, z=z, m=m,
                h=torch.full((X.shape[0],), 0.01, dtype=torch.float32))


def _tensor_norms(Q):
    """Frobenius norms of the dipole and of the traceless parts of the degree-2 and degree-3 moments (K each)"""
    K = Q.shape[0]
    M2, M3 = np.zeros((K, 3, 3)), np.zeros((K, 3, 3, 3))
    for j, k in enumerate(_terms(4)):
        ax = [i for i in range(3) for _ in range(k[i])]
        if len(ax) == 2:
            M2[:, ax[0], ax[1]] = M2[:, ax[1], ax[0]] = Q[:, j]
        if len(ax) == 3:
            for p in ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)):
                M3[:, ax[p[0]], ax[p[1]], ax[p[2]]] = Q[:, j]
    I = np.eye(3)
    T2 = M2 - np.einsum("kll,ab->kab", M2, I) / 3
    v = np.einsum("kllc->kc", M3)
    T3 = M3 - (np.einsum("ab,kc->kabc", I, v) + np.einsum("ac,kb->kabc", I, v) + np.einsum("bc,ka->kabc", I, v)) / 5
    return np.linalg.norm(Q[:, 1:4], axis=1), np.linalg.norm(T2, axis=(1, 2)), np.sqrt((T3 ** 2).sum((1, 2, 3)))


def _far_reference(lists, t, Q, P, X, first, last):
    """fp64 far field of the node lists with the half masks, its scales Sa, Sphi, the fp32 deviations of the same
    oracle (offsets as the node records hold them: fp32 from the frame origin, less the group centre's) and, for
    P = 4, the budget of the expanded tile products: per degree n U |T(n)| (r + R_group)^(n-1) in V_n"""
    n = last - first
    out = {k: np.zeros(n) for k in ("phi", "Sa", "Sphi", "d32a", "d32p", "Fa", "Fp")}
    out["a"] = np.zeros((n, 3))
    org, _ = GO.frame(X[:, 0], X[:, 1], X[:, 2])
    for g, L in enumerate(lists):
        nodes = np.concatenate([L["both"], L["A"], L["B"]]).astype(np.int64)
        if nodes.size == 0:
            continue
        idx = GO.group_targets(first, last, 64, g, False)
        sl = slice(idx[0] - first, idx[0] - first + idx.size)
        tc = X[GO.group_targets(first, last, 64, g, True)]
        gc = 0.5 * (tc.min(0) + tc.max(0))
        mask = np.concatenate([np.full(L["both"].size, 3), np.full(L["A"].size, 1), np.full(L["B"].size, 2)])
        on = (mask[None, :] & np.where(np.arange(idx.size) < 32, 1, 2)[:, None]) != 0
        r = X[idx][:, None, :] - t.c[nodes][None, :, :]
        r = np.where(on[..., None], r, 1.0)  # (a node of the other half only may sit on a target)
        phi, a, an = m2p_oracle(r, Q[nodes], P)
        t32 = (X[idx] - gc).astype(np.float32)
        c32 = (t.c[nodes] - org).astype(np.float32) - (gc - org).astype(np.float32)
        r32 = np.where(on[..., None], t32[:, None, :] - c32[None, :, :], np.float32(1))
        p32, a32, _ = m2p_oracle(r32, Q[nodes], P, np.float32)
        out["phi"][sl] = (on * phi).sum(1)
        out["a"][sl] = (on[..., None] * a).sum(1)
        out["Sa"][sl] = (on * an).sum(1)
        out["Sphi"][sl] = (on * np.abs(phi)).sum(1)
        out["d32a"][sl] = np.linalg.norm((on[..., None] * (a32.astype(np.float64) - a)).sum(1), axis=1)
        out["d32p"][sl] = np.abs((on * (p32.astype(np.float64) - phi)).sum(1))
        if P == 4:
            rr = np.sqrt((r * r).sum(-1))
            R = np.linalg.norm(X[idx] - gc, axis=1).max()
            for deg, cn, T in zip((1, 2, 3), (1.0, 1.5, 2.5), _tensor_norms(Q[nodes])):
                dV = U * T[None, :] * (rr + R) ** (deg - 1) * (rr + R if deg == 1 else 1.0)  # (degree 1: s_1 itself)
                pw = rr ** (2 * deg + 1)
                out["Fa"][sl] += (on * cn * (3 * deg + 1) * dV / pw * (1 / rr if deg == 1 else 1.0)).sum(1)
                out["Fp"][sl] += (on * cn * dV * (1.0 if deg == 1 else rr) / pw).sum(1)
    return out


def _run(gpu, name, P, first=0, last=None, phases=False, expect_spill=False):
    c = _case(name)
    n = c["n"]
    last = n if last is None else last
    x, y, z, h, m = (c[k].to(gpu) for k in ("x", "y", "z", "h", "m"))
    import dataclasses

    ot = dataclasses.replace(c["ot"], **{f.name: getattr(c["ot"], f.name).to(gpu) for f in dataclasses.fields(c["ot"])
                                         if isinstance(getattr(c["ot"], f.name), torch.Tensor)})
    centers, mp = G.upsweep(ot, x, y, z, m, c["box"], c["theta"])
    Qd = G.multipole_upsweep(ot, centers, x, y, z, m, P)
    gl = G.gravity_lists(ot, centers, mp, first, last, x, y, z, {})
    acc = [torch.zeros(n, dtype=torch.float32, device=gpu) for _ in range(3)]
    ug = torch.zeros(n, dtype=torch.float64, device=gpu)
    for ph in ((1, 2, 3) if phases else (0,)):
        pending = G.gravity_eval(gl, x, y, z, h, m, 1.0, *acc, ug, phase=ph, order=P, moments=Qd)
    pending.finish(pending.dev.cpu().tolist())
    slabs, _ = GO.from_slabs(gl, _lib.hip().gravity_scratch_layout(last - first, *gl.caps))
    xn, yn, zn, hn, mn = (c[k].numpy() for k in ("x", "y", "z", "h", "m"))
    X = np.stack([xn, yn, zn], 1)
    t = GO.Tree(ot, centers, mp)
    spilled = [g for g, S in enumerate(slabs) if S is None]
    assert bool(spilled) == expect_spill
    if spilled:  # spilled groups walk the tree themselves: the same rule
        wk = GO.walk(t, xn, yn, zn, first, last)
        slabs = [wk[g] if S is None else S for g, S in enumerate(slabs)]
    none = np.zeros(0, np.int64)
    near = GO.evaluate([dict(L, both=none, A=none, B=none) for L in slabs], t, xn, yn, zn, hn, mn, first, last,
                       with_budget=True)
    far = _far_reference(slabs, t, Qd.cpu().numpy().reshape(t.N, -1).astype(np.float64), P, X, first, last)
    eps_a = (far["d32a"] / (far["Sa"] + 1e-300)).max()
    eps_p = (far["d32p"] / (far["Sphi"] + 1e-300)).max()
    a = np.stack([v.cpu().numpy() for v in acc], 1).astype(np.float64)
    assert not a[:first].any() and not a[last:].any()
    da = np.linalg.norm(a[first:last] - near["a"] - far["a"], axis=1)
    dp = np.abs(ug.cpu().numpy()[first:last] / mn[first:last].astype(np.float64) - near["phi"] - far["phi"])
    Ba = near["Ba"] + 4 * eps_a * far["Sa"] + far["Fa"] + 1e-300
    Bp = near["Bphi"] + 4 * eps_p * far["Sphi"] + far["Fp"] + 1e-300
    print(f"[{name} P={P}] eps_a={eps_a:.3g} eps_phi={eps_p:.3g} a/B={(da / Ba).max():.3g} phi/B={(dp / Bp).max():.3g}"
          f" a/(4 eps Sa)={(da / (4 * eps_a * far['Sa'] + 1e-300)).max():.3g} spilled={len(spilled)}")
    assert (da <= Ba).all() and (dp <= Bp).all()
    return slabs


_SLABS = {}


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["U", "C", "T1", "T63", "T65"])
@pytest.mark.parametrize("P", [3, 4, 6])
def test_gpu_order_matches_oracle(gpu, P, name):
    _SLABS[name] = _run(gpu, name, P)


@pytest.mark.gpu
def test_gpu_order_lists_reach_every_branch(gpu):
    slabs = sum(((_SLABS.get(name) or _run(gpu, name, 3)) for name in ("U", "C")), [])
    assert any(L["both"].size > 128 for L in slabs)       # three batches
    assert any((L["both"].size % 16) != 0 for L in slabs)  # a ragged last tile
    assert any(L["A"].size for L in slabs) and any(L["B"].size for L in slabs)


@pytest.mark.gpu
@pytest.mark.parametrize("P", [3, 4, 6])
def test_gpu_order_sub_range_and_phases(gpu, P):
    _run(gpu, "U", P, first=70, last=1500, phases=True)


@pytest.mark.gpu
@pytest.mark.parametrize("P", [3, 4, 6])
def test_gpu_order_spilled_groups(gpu, monkeypatch, P):
    monkeypatch.setattr(G, "TEST_CAPS", (64, 64))
    _run(gpu, "U", P, expect_spill=True)


@pytest.mark.gpu
def test_simulation_multipole_order(gpu):
    from sphexa_amd.app.simulation import Simulation

    err = {}
    for order in (0, 4):
        sim = Simulation("evrard", n=20, multipole_order=order, device="cuda").run(2)
        d, holder = sim.d, sim.propagator.gravity
        assert holder.order == order
        assert all(bool(torch.isfinite(d[k]).all()) for k in ("ax", "ay", "az", "x"))
        sim.propagator.sync(sim.domain, d)  # tree and order of the moved particles
        x, y, z, h, m = (d[k] for k in ("x", "y", "z", "h", "m"))
        ref = [torch.zeros_like(d["ax"]) for _ in range(3)]
        G.direct_sum(0, x.numel(), x, y, z, h, m, d.g, *ref)
        got = [torch.zeros_like(d["ax"]) for _ in range(3)]
        holder.upsweep(d, sim.domain)
        holder.traverse(d, sim.domain, out=got)
        holder.finish_sync(d)
        num = torch.sqrt(sum((g - r) ** 2 for g, r in zip(got, ref)))
        err[order] = float(torch.quantile(num / torch.sqrt(sum(r ** 2 for r in ref)), 0.99))
    print("p99 relative acceleration error against the direct sum:", err)
    assert err[4] < err[0]


def test_multipole_order_validation():
    from sphexa_amd.app.simulation import check_multipole_order

    check_multipole_order(4, "cuda", 1, 0)
    for args in ((4, "cuda", 2, 0), (4, "cuda", 1, 1), (7, "cuda", 1, 0)):
        with pytest.raises(ValueError):
            check_multipole_order(*args)
