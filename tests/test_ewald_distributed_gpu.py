"""Periodic (Ewald) self-gravity with a remote LET tree on the GPU (csrc/hip/ewald.hip): ranks that share cuda:0 over
gloo, and the op alone with a synthetic remote tree.

Data: tests/ewald_mp.py (the blobs of tests/test_ewald_gpu.py). Every device call of the op runs with ``_lib.cpu``
patched to raise. Measured on an MI355X: profiles/r10/ewald_multirank/README.md.
"""

import numpy as np
import pytest
import torch

import ewald_mp as E
from mp_util import run_ranks
from test_ewald_gpu import _setup, _to_device

from sphexa_amd.ops import _lib
from sphexa_amd.ops import gravity as G

pytestmark = pytest.mark.gpu

THETA = 0.5


@pytest.fixture(scope="module")
def oracle():
    X = E.blob_positions()
    x, y, z = (torch.from_numpy(X[:, k].copy()) for k in range(3))
    m = torch.full((E.N,), 0.37 / E.N, dtype=torch.float32)
    (rx, ry, rz), e = G.direct_ewald(x, y, z, m, E.GRAV, E.L)
    return dict(X=X, ref=np.stack([rx.numpy(), ry.numpy(), rz.numpy()], 1), eref=e)


@pytest.fixture(scope="module")
def gpu_ranks():
    """one launch per world size, both shell counts: {world: per-rank results}"""
    return {w: run_ranks(E.op_worker, w, "cuda:0", (THETA,), (1, 2), timeout=300.0) for w in (1, 2)}


def _percentiles(acc, ref):
    err = np.sort(E.rel(acc, ref))
    return err[E.N // 2], err[int(0.99 * E.N)], err[-1]


@pytest.mark.parametrize("shells", [1, 2])
def test_ewald_gpu_ranks_match_direct_ewald(gpu, oracle, gpu_ranks, shells):
    """D1: 2 ranks on one GPU, theta 0.5, against the O(N^2) Ewald sum and against the one-rank GPU result"""
    key = (THETA, shells)
    two, one = gpu_ranks[2], gpu_ranks[1]
    assert all(r["res"][key]["nremote"] > 0 and r["res"][key]["remote_nodes"] > 0 for r in two)
    assert all(r["res"][key]["halos"] > 0 for r in two)
    out = {}
    for world, res in ((1, one), (2, two)):
        pos, acc, e = E.gather(res, key)
        o, xo = E.match(pos, oracle["X"])
        out[world] = _percentiles(acc[o], oracle["ref"][xo]) + (abs(e - oracle["eref"]) / abs(oracle["eref"]),)
    (med1, p991, mx1, e1), (med2, p992, mx2, e2) = out[1], out[2]
    print(f"D1 shells {shells}: 2 ranks median {med2:.2e} p99 {p992:.2e} max {mx2:.2e} energy {e2:.2e} | "
          f"1 rank median {med1:.2e} p99 {p991:.2e} max {mx1:.2e} energy {e1:.2e} | "
          f"remote multipoles {[r['res'][key]['nremote'] for r in two]}")
    assert med2 < 1e-3 and p992 < 1e-2
    assert e2 < 3e-3
    assert med2 <= 1.5 * med1 + 2e-6
    assert p992 <= 1.5 * p991 + 1e-5


@pytest.fixture(scope="module")
def blobs_gpu(gpu):
    ot, *fields = _setup(E.blob_positions(), E.blob_box(), 0.37 / E.N, 1e-4 * E.L)
    return _to_device(ot, fields, gpu)


def test_ewald_gpu_remote_none_is_bit_identical(gpu, monkeypatch, blobs_gpu):
    """D2: remote=None is the call without the argument: accelerations and ugrav bit for bit. The returned energy is
    the sum of one fp64 atomicAdd per wave, in an order nothing fixes (two calls without the argument may differ in
    the last bits as well; on an MI355X all three came out equal), so it is held to the 1e-13 that test A2 of
    tests/test_ewald_gpu.py grants the OpenMP reduction for the same reason, and its terms, ugrav, bit for bit"""
    otg, xg, yg, zg, mg, hg = blobs_gpu
    box = E.blob_box()
    first, last = 37, E.N - 5
    cg, mgp = G.upsweep(otg, xg, yg, zg, mg, box, THETA)

    def run(**kw):
        acc = [torch.zeros(E.N, dtype=torch.float32, device=gpu) for _ in range(3)]
        u = torch.zeros(E.N, dtype=torch.float64, device=gpu)
        with monkeypatch.context() as mpatch:
            mpatch.setattr(_lib, "cpu", E._no_cpu)
            e = G.compute_gravity_ewald(otg, cg, mgp, first, last, xg, yg, zg, hg, mg, E.GRAV, box, *acc, shells=1,
                                        ugrav=u, **kw)
        return [t.cpu() for t in acc] + [u.cpu()], e

    (base, e0), (none, e1), (again, e2) = run(), run(remote=None), run()
    print(f"D2: energy without the argument {e0!r}, again {e2!r}, remote=None {e1!r}")
    assert all(torch.equal(a, b) for a, b in zip(base, none))
    assert abs(e1 - e0) <= 1e-13 * abs(e0)
    assert abs(0.5 * float(none[3].sum()) - e1) <= 1e-12 * abs(e1)
    assert float(base[0].abs().max()) > 0


def _leaf_multipoles(ot, centers, mp):
    """(placeholder codes, centres (M, 3), quadrupoles (M, 8)) of the non-empty leaves of a tree: what the LET
    exchange sends for nodes that pass the MAC (it never sends an empty node)"""
    nodes = ot.leaf_to_node.long()
    q = mp.view(-1, 8)[nodes]
    keep = q[:, 0] > 0
    nodes = nodes[keep]
    return (ot.prefixes[nodes].contiguous(), centers.view(-1, 4)[nodes, :3].contiguous(),
            mp.view(-1, 8)[nodes].contiguous())


def test_ewald_gpu_synthetic_remote_tree_matches_cpu(gpu, monkeypatch):
    """D3: no communication. The blob particles split by index into A (the first blob) and B (the second): A's tree
    with its particles is the local tree, B goes through remote_let_tree as one leaf per non-empty bucket-16 leaf of
    B's own tree.
    theta = 1e-3: A's tree is fully opened and every internal remote node too, so the GPU and the OpenMP op sum the
    same interactions (A's particles + B's leaf quadrupoles, per replica, plus both roots' lattice terms)"""
    X, box, theta = E.blob_positions(), E.blob_box(), 1e-3
    XA, XB = X[:E.N // 2], X[E.N // 2:]
    mass, h = 0.37 / E.N, 1e-4 * E.L
    otA, xA, yA, zA, mA, hA = _setup(XA, box, mass, h)
    otB, xB, yB, zB, mB, _ = _setup(XB, box, mass, h)
    cA, qA = G.upsweep(otA, xA, yA, zA, mA, box, theta)
    cB, qB = G.upsweep(otB, xB, yB, zB, mB, box, theta)
    codes, rc, rq = _leaf_multipoles(otB, cB, qB)
    assert codes.numel() > 8 and abs(float(rq[:, 0].sum()) - mass * XB.shape[0]) < 1e-6 * mass * XB.shape[0]
    nA = XA.shape[0]
    first, last = 5, nA - 3

    remote_c = G.remote_let_tree(codes, rc, rq, box, theta)
    assert remote_c[0].num_nodes > 1
    c, ec, uc = _ewald_remote(monkeypatch, otA, cA, qA, first, last, xA, yA, zA, hA, mA, box, remote_c)
    c0, ec0, _ = _ewald_remote(monkeypatch, otA, cA, qA, first, last, xA, yA, zA, hA, mA, box, None)

    otg, xg, yg, zg, mg, hg = _to_device(otA, (xA, yA, zA, mA, hA), gpu)
    cg, qg = G.upsweep(otg, xg, yg, zg, mg, box, theta)
    remote_g = G.remote_let_tree(codes.to(gpu), rc.to(gpu), rq.to(gpu), box, theta, host_codes=codes)
    g, eg, ug = _ewald_remote(monkeypatch, otg, cg, qg, first, last, xg, yg, zg, hg, mg, box, remote_g)

    rel = E.rel(g[first:last], c[first:last])
    moved = E.rel(c[first:last], c0[first:last])
    print(f"D3: median {np.median(rel):.2e} max {rel.max():.2e} energy {abs(eg - ec) / abs(ec):.2e} "
          f"(remote tree {remote_g[0].num_nodes} nodes from {codes.numel()} leaves; it changes the accelerations by a "
          f"median {np.median(moved):.2e}, the energy by {abs(ec - ec0) / abs(ec0):.2e})")
    # the remote tree matters: without it the oracle itself is far away (CPU values: 1.6e-2 and 1.6e-1)
    assert np.median(moved) > 5e-3 and abs(ec - ec0) > 1e-2 * abs(ec0)
    assert np.median(rel) < 1e-4 and rel.max() < 2e-2
    assert abs(eg - ec) < 1e-3 * abs(ec)
    outside = np.r_[0:first, last:nA]
    assert np.all(g[outside] == 0.0) and np.all(ug[outside] == 0.0)
    assert abs(0.5 * ug.sum() - eg) <= 1e-6 * abs(eg)


def _ewald_remote(monkeypatch, ot, centers, mp, first, last, x, y, z, h, m, box, remote):
    n = x.numel()
    acc = [torch.zeros(n, dtype=torch.float32, device=x.device) for _ in range(3)]
    u = torch.zeros(n, dtype=torch.float64, device=x.device)
    with monkeypatch.context() as mpatch:
        if x.is_cuda:
            mpatch.setattr(_lib, "cpu", E._no_cpu)
        e = G.compute_gravity_ewald(ot, centers, mp, first, last, x, y, z, h, m, E.GRAV, box, *acc, shells=1, ugrav=u,
                                    remote=remote)
    return np.stack([t.cpu().numpy() for t in acc], 1).astype(np.float64), e, u.cpu().numpy()


def test_ewald_gpu_ranks_ve_step_matches_one_rank(gpu):
    """D4: one full VE step of the isobaric cube (4096 particles, every node open), 2 ranks on one GPU against 1"""
    one = run_ranks(E.ve_step_worker, 1, "cuda:0", timeout=300.0)
    two = run_ranks(E.ve_step_worker, 2, "cuda:0", timeout=300.0)
    E.ve_step_compare(one, two, "D4")
