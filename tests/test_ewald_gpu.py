"""Periodic (Ewald) self-gravity on the GPU (csrc/hip/ewald.hip) against the O(N^2) Ewald sum and the OpenMP path.

Data of A1/A2: the two wrapped Gaussian blobs of tests/test_ewald.py (seed 7) with n = 803 (a partial last group of
64 targets), scaled to a box of length 2.5 with lower corner -0.7 (catches k_f, volume and offset mistakes),
m = 0.37 / n, G = 0.7, h = 1e-4 L, bucket 16. Every device call runs with ``_lib.cpu`` patched to raise: the device
path must not touch the OpenMP module.

Measured on an MI355X (profiles/r7/ewald/README.md):
  A1 (theta 0.5)  shells 1: median 3.6e-4, p99 1.3e-3, energy 1.4e-3;  shells 2: median 1.7e-4, p99 8.2e-4, energy 4.9e-4
  A2 (all open)   shells 1: median 3.6e-7, max 2.0e-6, energy 1.5e-7;  shells 2: median 3.6e-7, max 1.9e-6, energy 4.6e-7
  A3 (6^3 lattice) max |a| 2.2e-3 (gate 5.0e-3)
"""

import numpy as np
import pytest
import torch

from sphexa_amd.ops import _lib
from sphexa_amd.ops import gravity as G
from sphexa_amd.ops import octree as O
from sphexa_amd.ops import sfc
from sphexa_amd.utils.box import Box, PERIODIC

pytestmark = pytest.mark.gpu

N, L, LO, GRAV = 803, 2.5, -0.7, 0.7


def _setup(X, box, mass, h, bucket=16):
    n = X.shape[0]
    x, y, z = (torch.from_numpy(X[:, k].copy()) for k in range(3))
    keys = sfc.compute_keys(x, y, z, box)
    s, p = sfc.sort_keys(keys)
    p = p.long()
    x, y, z = x[p], y[p], z[p]
    m = torch.full((n,), mass, dtype=torch.float32)
    hh = torch.full((n,), h, dtype=torch.float32)
    tree, counts = O.update_tree(None, s, bucket)
    ot = O.build_octree(tree, counts, s, x, y, z)
    ot.keys = s  # (for the device copy of the tree)
    return ot, x, y, z, m, hh


def _to_device(ot, fields, dev):
    xg, yg, zg, mg, hg = (t.to(dev) for t in fields)
    otg = O.build_octree(ot.tree.to(dev), ot.counts.to(dev), ot.keys.to(dev), xg, yg, zg)
    return otg, xg, yg, zg, mg, hg


def _no_cpu():
    raise AssertionError("the device path of compute_gravity_ewald called the OpenMP module")


def _ewald(monkeypatch, ot, centers, mp, first, last, x, y, z, h, m, grav, box, shells, with_u=False):
    """(accelerations (n, 3) float64 numpy, energy, ugrav or None); device tensors run with _lib.cpu disabled"""
    n = x.numel()
    acc = [torch.zeros(n, dtype=torch.float32, device=x.device) for _ in range(3)]
    u = torch.zeros(n, dtype=torch.float64, device=x.device) if with_u else None
    with monkeypatch.context() as mpatch:
        if x.is_cuda:
            assert hasattr(_lib.hip(), "compute_gravity_ewald")
            mpatch.setattr(_lib, "cpu", _no_cpu)
        e = G.compute_gravity_ewald(ot, centers, mp, first, last, x, y, z, h, m, grav, box, *acc, shells=shells,
                                    ugrav=u)
    a = np.stack([t.cpu().numpy() for t in acc], 1).astype(np.float64)
    return a, e, (u.cpu().numpy() if with_u else None)


def _rel(a, b):
    return np.linalg.norm(a - b, axis=1) / np.linalg.norm(b, axis=1)


@pytest.fixture(scope="module")
def blobs():
    """host data, tree and the direct Ewald oracle (computed once)"""
    rng = np.random.default_rng(7)
    n = N
    X = np.concatenate([rng.normal(0.3, 0.08, (n // 2, 3)), rng.normal(0.75, 0.05, (n - n // 2, 3))]) % 1.0
    X = X * L + LO
    box = Box([LO] * 3, [LO + L] * 3, [PERIODIC] * 3)
    ot, x, y, z, m, h = _setup(X, box, 0.37 / n, 1e-4 * L)
    (rx, ry, rz), ed = G.direct_ewald(x, y, z, m, GRAV, L)
    ref = np.stack([rx.numpy(), ry.numpy(), rz.numpy()], 1)
    return dict(box=box, ot=ot, fields=(x, y, z, m, h), ref=ref, eref=ed)


@pytest.fixture(scope="module")
def blobs_gpu(blobs, gpu):
    return _to_device(blobs["ot"], blobs["fields"], gpu)


@pytest.mark.parametrize("shells", [1, 2])
def test_ewald_gpu_matches_direct_ewald(gpu, monkeypatch, blobs, blobs_gpu, shells):
    """A1: theta = 0.5, full range, against the O(N^2) Ewald sum, and no worse than 1.5 x the OpenMP path's error"""
    assert hasattr(_lib.hip(), "compute_gravity_ewald")
    box, ot, ref, eref = blobs["box"], blobs["ot"], blobs["ref"], blobs["eref"]
    x, y, z, m, h = blobs["fields"]
    cc, mc = G.upsweep(ot, x, y, z, m, box, 0.5)
    c, ec, _ = _ewald(monkeypatch, ot, cc, mc, 0, N, x, y, z, h, m, GRAV, box, shells)
    otg, xg, yg, zg, mg, hg = blobs_gpu
    cg, mgp = G.upsweep(otg, xg, yg, zg, mg, box, 0.5)
    g, eg, _ = _ewald(monkeypatch, otg, cg, mgp, 0, N, xg, yg, zg, hg, mg, GRAV, box, shells)
    err_g, err_c = np.sort(_rel(g, ref)), np.sort(_rel(c, ref))
    med_g, p99_g = err_g[N // 2], err_g[int(0.99 * N)]
    med_c, p99_c = err_c[N // 2], err_c[int(0.99 * N)]
    print(f"A1 shells {shells}: GPU median {med_g:.2e} p99 {p99_g:.2e} energy {abs(eg - eref) / abs(eref):.2e} | "
          f"CPU median {med_c:.2e} p99 {p99_c:.2e} energy {abs(ec - eref) / abs(eref):.2e}")
    assert med_g < 1e-3 and p99_g < 1e-2
    assert abs(eg - eref) < 3e-3 * abs(eref)
    # the GPU's group MAC opens at least what the CPU's point MAC opens (not applied to the energy: the CPU's
    # energy error at shells = 2 is a cancellation)
    assert med_g <= 1.5 * med_c + 2e-6
    assert p99_g <= 1.5 * p99_c + 1e-5


@pytest.mark.parametrize("shells", [1, 2])
def test_ewald_gpu_all_open_matches_cpu(gpu, monkeypatch, blobs, blobs_gpu, shells):
    """A2: theta = 1e-3 opens every node on both paths (the CPU result is bit-identical at half theta), so the
    interaction sets are the same and the paths differ by rounding only; sub-range with first > 0 and ugrav"""
    assert hasattr(_lib.hip(), "compute_gravity_ewald")
    box, ot = blobs["box"], blobs["ot"]
    x, y, z, m, h = blobs["fields"]
    first, last = 37, N - 5
    cpu = []
    for theta in (1e-3, 5e-4):
        cc, mc = G.upsweep(ot, x, y, z, m, box, theta)
        cpu.append(_ewald(monkeypatch, ot, cc, mc, first, last, x, y, z, h, m, GRAV, box, shells, with_u=True))
    (c, ec, uc), (c2, ec2, uc2) = cpu
    # per-particle results are bit-identical; the energy is an OpenMP reduction whose order is not fixed
    assert np.array_equal(c, c2) and np.array_equal(uc, uc2)
    assert abs(ec - ec2) <= 1e-13 * abs(ec)
    otg, xg, yg, zg, mg, hg = blobs_gpu
    cg, mgp = G.upsweep(otg, xg, yg, zg, mg, box, 1e-3)
    g, eg, ug = _ewald(monkeypatch, otg, cg, mgp, first, last, xg, yg, zg, hg, mg, GRAV, box, shells, with_u=True)
    rel = _rel(g[first:last], c[first:last])
    print(f"A2 shells {shells}: median {np.median(rel):.2e} max {rel.max():.2e} energy {abs(eg - ec) / abs(ec):.2e}")
    assert np.median(rel) < 1e-4 and rel.max() < 2e-2
    assert abs(eg - ec) < 1e-3 * abs(ec)
    outside = np.r_[0:first, last:N]
    assert np.all(g[outside] == 0.0) and np.all(ug[outside] == 0.0)
    assert abs(0.5 * ug.sum() - eg) <= 1e-6 * abs(eg)
    assert abs(0.5 * uc.sum() - ec) <= 1e-12 * abs(ec)


def test_ewald_gpu_uniform_lattice_has_no_force(gpu, monkeypatch):
    """A3: a uniform lattice in a periodic box is force-free"""
    assert hasattr(_lib.hip(), "compute_gravity_ewald")
    k = 6
    gr = (np.arange(k) + 0.5) / k
    X = np.stack(np.meshgrid(gr, gr, gr, indexing="ij"), -1).reshape(-1, 3)
    n = X.shape[0]
    box = Box([0.0] * 3, [1.0] * 3, [PERIODIC] * 3)
    ot, *fields = _setup(X, box, 1.0 / n, 1e-4)
    otg, xg, yg, zg, mg, hg = _to_device(ot, fields, gpu)
    cg, mgp = G.upsweep(otg, xg, yg, zg, mg, box, 0.5)
    a, e, _ = _ewald(monkeypatch, otg, cg, mgp, 0, n, xg, yg, zg, hg, mg, 1.0, box, 1)
    print(f"A3: max |a| {np.abs(a).max():.2e} (gate {3e-2 * k ** 2 / n:.2e})")
    assert np.isfinite(e)
    assert np.abs(a).max() < 3e-2 * k ** 2 / n


def test_ewald_gpu_needs_cubic_box(gpu, monkeypatch, blobs, blobs_gpu):
    """A4: a non-cubic periodic box is refused for device tensors as well"""
    assert hasattr(_lib.hip(), "compute_gravity_ewald")
    otg, xg, yg, zg, mg, hg = blobs_gpu
    box = Box([LO] * 3, [LO + L, LO + L, LO + 2 * L], [PERIODIC] * 3)
    cg, mgp = G.upsweep(otg, xg, yg, zg, mg, blobs["box"], 0.5)
    with pytest.raises(ValueError):
        _ewald(monkeypatch, otg, cg, mgp, 0, N, xg, yg, zg, hg, mg, GRAV, box, 1)
