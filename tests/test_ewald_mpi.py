"""Periodic (Ewald) self-gravity on several CPU ranks (gloo): the local tree and the remote LET tree in one evaluation
(ops.gravity.compute_gravity_ewald(remote=...), MultipoleHolder.traverse_ewald), the propagators, Simulation and the
command line.

Data of M1/M2: tests/ewald_mp.py (the blobs of tests/test_ewald_gpu.py), Domain(bucket_size_focus=16, bucket_size=64).
Measured on the OpenMP path (profiles/r10/ewald_multirank/README.md): M1 median <= 6.9e-4, p99 <= 1.9e-3, energy
<= 1.2e-3 for 2 and 3 ranks.
"""

import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import ewald_mp as E
from mp_util import free_port, run_ranks

THETA, THETA_OPEN = 0.5, 1e-3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def oracle():
    """the O(N^2) Ewald sum of all particles (computed once)"""
    from sphexa_amd.ops import gravity as G

    X = E.blob_positions()
    x, y, z = (torch.from_numpy(X[:, k].copy()) for k in range(3))
    m = torch.full((E.N,), 0.37 / E.N, dtype=torch.float32)
    (rx, ry, rz), e = G.direct_ewald(x, y, z, m, E.GRAV, E.L)
    return dict(X=X, ref=np.stack([rx.numpy(), ry.numpy(), rz.numpy()], 1), eref=e)


@pytest.fixture(scope="module")
def one_rank_open():
    """the one-rank OpenMP result with every node open, per shell count: (X order, accelerations, energy)"""
    from sphexa_amd.ops import gravity as G
    from sphexa_amd.ops import octree as O
    from sphexa_amd.ops import sfc

    X, box = E.blob_positions(), E.blob_box()
    x, y, z = (torch.from_numpy(X[:, k].copy()) for k in range(3))
    s, p = sfc.sort_keys(sfc.compute_keys(x, y, z, box))
    p = p.long()
    x, y, z = x[p], y[p], z[p]
    m = torch.full((E.N,), 0.37 / E.N, dtype=torch.float32)
    h = torch.full((E.N,), 1e-4 * E.L, dtype=torch.float32)
    tree, counts = O.update_tree(None, s, 16)
    ot = O.build_octree(tree, counts, s, x, y, z)
    c, q = G.upsweep(ot, x, y, z, m, box, THETA_OPEN)
    out = {}
    for shells in (1, 2):
        acc = [torch.zeros(E.N, dtype=torch.float32) for _ in range(3)]
        e = G.compute_gravity_ewald(ot, c, q, 0, E.N, x, y, z, h, m, E.GRAV, box, *acc, shells=shells)
        out[shells] = (np.stack([x.numpy(), y.numpy(), z.numpy()], 1),
                       np.stack([t.numpy() for t in acc], 1).astype(np.float64), e)
    return out


_RUNS = {}


def _ranks(world):
    """both thetas and both shell counts of one world size in one launch of the ranks"""
    if world not in _RUNS:
        _RUNS[world] = run_ranks(E.op_worker, world, "cpu", (THETA, THETA_OPEN), (1, 2))
    return _RUNS[world]


@pytest.mark.parametrize("shells", [1, 2])
@pytest.mark.parametrize("world", [2, 3])
def test_ewald_ranks_match_direct_ewald(oracle, world, shells):
    """M1: theta 0.5, against the O(N^2) Ewald sum of all particles, matched by position. Every rank has halos (the
    halo route) and received multipoles (the remote-tree route)"""
    res = _ranks(world)
    key = (THETA, shells)
    assert all(r["res"][key]["nremote"] > 0 and r["res"][key]["remote_nodes"] > 0 for r in res)
    assert all(r["res"][key]["halos"] > 0 for r in res)
    pos, acc, e = E.gather(res, key)
    o, xo = E.match(pos, oracle["X"])
    err = np.sort(E.rel(acc[o], oracle["ref"][xo]))
    med, p99, eerr = err[E.N // 2], err[int(0.99 * E.N)], abs(e - oracle["eref"]) / abs(oracle["eref"])
    print(f"M1 ranks {world} shells {shells}: median {med:.2e} p99 {p99:.2e} max {err[-1]:.2e} energy {e:.7f} "
          f"({eerr:.2e}) remote multipoles {[r['res'][key]['nremote'] for r in res]}")
    assert med < 1e-3 and p99 < 1e-2
    assert eerr < 3e-3


@pytest.mark.parametrize("shells", [1, 2])
@pytest.mark.parametrize("world", [2, 3])
def test_ewald_ranks_all_open_match_one_rank(one_rank_open, world, shells):
    """M2: theta = 1e-3 opens every node, so every remote particle arrives as a halo and the remote tree is empty or
    absent; against the one-rank OpenMP result at the same theta"""
    res = _ranks(world)
    key = (THETA_OPEN, shells)
    assert all(r["res"][key]["nremote"] == 0 and r["res"][key]["remote_nodes"] == 0 for r in res)
    assert all(r["res"][key]["halos"] + r["res"][key]["pos"].shape[0] == E.N for r in res)
    pos, acc, e = E.gather(res, key)
    X1, a1, e1 = one_rank_open[shells]
    o, xo = E.match(pos, X1)
    err = E.rel(acc[o], a1[xo])
    print(f"M2 ranks {world} shells {shells}: median {np.median(err):.2e} max {err.max():.2e} "
          f"energy {abs(e - e1) / abs(e1):.2e}")
    assert np.median(err) < 1e-4 and err.max() < 2e-2
    assert abs(e - e1) < 1e-3 * abs(e1)


def test_ewald_ranks_lattice_at_rest():
    """M3: a full nbody step on 2 ranks; the uniform Sedov lattice is force-free under periodic gravity (the gate of
    tests/test_ewald_prop.py test_ewald_lattice_at_rest_cpu)"""
    res = run_ranks(E.lattice_worker, 2, "cpu")
    assert sum(r["n_per"] for r in res) == 12 ** 3
    ratio = max(r["per"] for r in res) / max(r["iso"] for r in res)
    print(f"M3 lattice at rest, 2 ranks: max|a| periodic / isolated = {ratio:.2e}")
    assert ratio < 1e-2


def test_ewald_ranks_ve_step_matches_one_rank():
    """M4: one full VE step of the isobaric cube (4096 particles, every node open) on 2 ranks against 1 rank"""
    one = run_ranks(E.ve_step_worker, 1, "cpu")
    two = run_ranks(E.ve_step_worker, 2, "cpu")
    E.ve_step_compare(one, two, "M4")


def test_ewald_ranks_cli(tmp_path):
    """M5: --ewald on 2 ranks through bin/sphexa (SPHEXA_RANKS: torch.distributed.run)"""
    env = dict(os.environ, PYTHON=sys.executable, OMP_NUM_THREADS="2", SPHEXA_RANKS="2", SPHEXA_PORT=str(free_port()))
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run([os.path.join(ROOT, "bin", "sphexa"), "--init", "sedov", "--prop", "nbody", "--G", "1", "-n",
                        "8", "-s", "1", "--ewald", "--device", "cpu", "--quiet"], cwd=tmp_path, env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
