"""Periodic (Ewald) self-gravity in the propagators, ``Simulation(ewald=S)`` and ``--ewald [S]``."""

import subprocess
import sys

import pytest
import torch

from sphexa_amd.app.simulation import Simulation
from sphexa_amd.models.init import base as init_base
from sphexa_amd.models.init import cases


@pytest.fixture
def small_glass(monkeypatch):
    blk = init_base.make_glass_block(8, relax_iters=10)
    monkeypatch.setattr(cases, "load_block", lambda path=None, n_side=16: blk)
    yield


def _max_acc(sim):
    return max(float(sim.local(k).abs().max()) for k in ("ax", "ay", "az"))


def _lattice_at_rest(device):
    """B1/B4: the Sedov lattice is uniform, so its periodic self-gravity vanishes, while the isolated sum pulls
    every particle to the centre. The cap mirrors the reference's 3e-2 lattice threshold; a periodic-gravity failure
    gives a ratio of order 1. Measured: 1.5e-3 (CPU, n = 12)"""
    iso = Simulation("sedov", n=12, prop="nbody", G=1.0, ewald=0, device=device).run(1)
    per = Simulation("sedov", n=12, prop="nbody", G=1.0, ewald=1, device=device).run(1)
    assert per.propagator.ewald_shells == 1 and iso.propagator.ewald_shells == 0
    ratio = _max_acc(per) / _max_acc(iso)
    print(f"lattice at rest ({device}): max|a| periodic / isolated = {ratio:.2e}")
    assert ratio < 1e-2


def test_ewald_lattice_at_rest_cpu():
    _lattice_at_rest("cpu")


@pytest.mark.parametrize("case,kwargs", [("evrard", dict(G=1.0)), ("sedov", dict(G=0.0)),
                                         ("kelvin-helmholtz", dict(G=1.0))])
def test_ewald_refused(small_glass, case, kwargs):
    """B2: open box, no gravity, non-cubic box"""
    with pytest.raises(ValueError):
        Simulation(case, n=8, prop="nbody" if kwargs["G"] else "ve", ewald=1, device="cpu", **kwargs)


def test_ewald_cli():
    """B3: --ewald without a value (one shell)"""
    cmd = [sys.executable, "-m", "sphexa_amd", "--init", "sedov", "--prop", "nbody", "--G", "1", "-n", "8", "-s", "1",
           "--ewald", "--device", "cpu", "--quiet"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr


@pytest.mark.gpu
def test_ewald_lattice_at_rest_gpu(gpu):
    _lattice_at_rest(gpu)


def _sorted_state(sim, names):
    order = torch.argsort(sim.local("keys").cpu())
    return {n: sim.local(n).cpu()[order].double() for n in names}


@pytest.mark.gpu
def test_ewald_step_gpu_matches_cpu(gpu, small_glass):
    """B5: one full VE step of the isobaric cube (4096 particles) with periodic gravity and every node open
    (theta = 1e-3: the same interaction set on both paths). Gates of test_gpu_cases.py test_case_gpu_matches_cpu;
    vx is the gravity-driven velocity from rest. Measured on an MI355X: see profiles/r7/ewald/README.md"""
    kw = dict(n=12, prop="ve", G=1.0, theta=1e-3, ewald=1)
    cpu = Simulation("isobaric-cube", device="cpu", **kw).run(1)
    dev = Simulation("isobaric-cube", device=gpu, **kw).run(1)
    assert cpu.d.numParticlesGlobal == 4096
    assert abs(dev.d.minDt - cpu.d.minDt) <= 1e-4 * cpu.d.minDt
    names = ["x", "vx", "h", "temp"]
    a, b = _sorted_state(cpu, names), _sorted_state(dev, names)
    errs = {k: float((a[k] - b[k]).abs().max()) / (float(a[k].abs().max()) + 1e-30) for k in names}
    eg_c, eg_d = cpu.conserved()["egrav"], dev.conserved()["egrav"]
    print("B5", {k: f"{v:.2e}" for k, v in errs.items()}, f"egrav {abs(eg_d - eg_c) / abs(eg_c):.2e}")
    for k in names:
        assert errs[k] < (1e-3 if k == "vx" else 2e-5), (k, errs[k])
    assert abs(eg_d - eg_c) <= 1e-3 * abs(eg_c)
