"""Block-union staged XMass and Gradh loops (csrc/hip/staged.h: the source union of a block's 4, 8 or 16 target groups
in LDS; XMass = staged bit 6, Gradh = bit 1) against the gathered loops on the same inputs, alone and together with the
staged IAD and AV loops (bits 2 and 3).

The staged loops read the same record bits and add them in the same order, one wave per target group: every field
must be bit-identical (torch.equal). A last-bit difference means a wrong, duplicated or skipped list entry."""

import os
import subprocess
import sys

import pytest
import torch

from sphexa_amd.app.simulation import Simulation
from sphexa_amd.ops import _lib
from sphexa_amd.ops import hydro as H

pytestmark = pytest.mark.gpu

FIELDS = ("x", "y", "z", "vx", "vy", "vz", "h", "temp", "u", "alpha", "xm", "kx", "du", "c", "nc")
XG = 2 | 64  # Gradh, XMass
XG32 = XG | 32  # also in runs on 256-thread blocks (Evrard: self-gravity)
ALL = XG | 4 | 8 | 32  # all four block-union loops

_gathered = {}


def _run(gpu, case, n, mask, steps=2, ng=None, kernel_fixed=True):
    """fields after `steps` steps, the block counters (staged, fallen back) of the block-union loops and whether the
    pair loops ran on the fixed-point records (the only path with staged loops)"""
    hp = _lib.hip()
    old = hp.staged_mask()
    counters = torch.zeros(2, dtype=torch.int32, device=gpu)
    hp.set_staged(mask)
    hp.set_staged_counters(counters.data_ptr())
    hp.set_pair_paths(kernel_fixed=kernel_fixed, mom_buf=True)
    try:
        sim = Simulation(case, n=n, device=gpu)
        if ng is not None:
            sim.d.ng0, sim.d.ngmax = ng
            sim.d["h"] = sim.d["h"] * (ng[0] / 100.0) ** (1.0 / 3.0)
        sim.run(steps)
        torch.cuda.synchronize()
        out = {}
        for f in FIELDS:
            try:
                v = sim.local(f)
            except Exception:  # (fields a case does not allocate)
                continue
            if v is not None and v.numel():
                out[f] = v.cpu()
        return out, tuple(int(c) for c in counters.cpu()) + (bool(sim.d.fixedPoint),)
    finally:
        hp.set_staged_counters(0)
        hp.set_staged(old)
        hp.set_pair_paths(kernel_fixed=True, mom_buf=True)


def _reference(gpu, case, n, steps=2, ng=None, kernel_fixed=True):
    """the gathered run of a case, computed once and shared"""
    key = (case, n, steps, ng, kernel_fixed)
    if key not in _gathered:
        out, counts = _run(gpu, case, n, 0, steps, ng, kernel_fixed)
        assert counts[:2] == (0, 0), "the gathered loops count no blocks"
        _gathered[key] = out
    return _gathered[key]


def _assert_identical(a, b):
    assert a.keys() == b.keys() and "x" in a and "xm" in a and "kx" in a
    bad = [f for f in a if not torch.equal(a[f], b[f])]
    assert not bad, f"staged vs gathered differ in {bad}"


@pytest.mark.parametrize("mask", [XG32, ALL])
@pytest.mark.parametrize("kernel_fixed", [True, False])
@pytest.mark.parametrize("case", ["sedov", "noh", "evrard"])
def test_whole_steps_bit_identical(gpu, case, kernel_fixed, mask):
    ref = _reference(gpu, case, 24, kernel_fixed=kernel_fixed)
    out, (staged, fell, _) = _run(gpu, case, 24, mask, kernel_fixed=kernel_fixed)
    print(f"{case} n=24 kernel_fixed={kernel_fixed} mask={mask}: blocks staged {staged}, fallen back {fell}")
    _assert_identical(ref, out)
    assert staged > 0


@pytest.mark.parametrize("n", [6, 9, 13])
def test_ragged_shapes(gpu, n):
    """216, 729 and 2197 particles: a partial last group, absent groups in the last block. (Where h is too large for
    the fixed-point frame the pair loops take the fp64 records, which have no staged loop: no block is counted.)"""
    ref = _reference(gpu, "sedov", n)
    out, (staged, fell, fixed) = _run(gpu, "sedov", n, XG32)
    print(f"sedov n={n}: fixed-point records {fixed}, blocks staged {staged}, fallen back {fell}")
    assert (n ** 3) % 64 != 0 and (n ** 3) % 256 != 0 and (n ** 3) % 512 != 0 and (n ** 3) % 1024 != 0
    _assert_identical(ref, out)
    assert (staged + fell > 0) == fixed
    if n == 13:
        assert fixed


def test_forced_fallback(gpu):
    """~300 neighbors per particle: every block's union exceeds the LDS capacity, every block runs the gathered loop"""
    ref = _reference(gpu, "sedov", 20, steps=1, ng=(300, 400))
    out, (staged, fell, _) = _run(gpu, "sedov", 20, XG32, steps=1, ng=(300, 400))
    print(f"sedov n=20, 300 neighbors: blocks staged {staged}, fallen back {fell}")
    assert float(ref["nc"].float().mean()) > 250
    _assert_identical(ref, out)
    assert staged == 0 and fell > 0


def test_lists_without_masks_fall_back(gpu):
    """lists searched while no staged bit was set have no slot masks (T == Tc): the staged XMass and Gradh ops must
    take the gathered loop, not read list rows as masks"""
    hp = _lib.hip()
    old = hp.staged_mask()
    hp.set_staged(0)
    counters = torch.zeros(2, dtype=torch.int32, device=gpu)
    try:
        sim = Simulation("sedov", n=20, device=gpu)
        sim.run(1)
        d, nl, box = sim.d, sim.propagator.nl, sim.domain.box
        s, e = sim.domain.start_index(), sim.domain.end_index()
        d.release("ay")  # (gradh takes its place, as in the propagator)
        d.acquire("gradh")

        def ops(mask):
            hp.set_staged(mask)
            H.compute_xmass(d, nl, box)
            H.compute_ve_def_gradh(d, nl, box)
            torch.cuda.synchronize()
            return {f: d[f][s:e].clone() for f in ("xm", "kx", "gradh")}

        ref = ops(0)
        hp.set_staged_counters(counters.data_ptr())
        out = ops(XG32)
    finally:
        hp.set_staged_counters(0)
        hp.set_staged(old)
    staged, fell = (int(c) for c in counters.cpu())
    print(f"mask-less lists: blocks staged {staged}, fallen back {fell}")
    for f in ref:
        assert torch.isfinite(ref[f]).all(), f
        assert torch.equal(ref[f], out[f]), f
    assert staged == 0 and fell > 0


def test_lost_rows_on_the_speculative_chain(gpu, monkeypatch):
    """one rank enqueues XMass and Gradh before the host knows that the search ran out of list rows; with 1 home row
    per group and 8 rows per overflow stripe every first search loses rows and is repeated. The staged loops must give
    such groups no slots (nblk == 0: blockTargetOf), and the redone step must equal the unforced run."""
    from sphexa_amd.ops import neighbors as N

    hp = _lib.hip()
    old = hp.staged_mask()
    hp.set_staged(XG32)
    results = []
    try:
        for forced in (False, True):
            if forced:
                monkeypatch.setattr(N, "_pool_plan", lambda prev, groups, ng0, stripes: (1, 8))
            sim = Simulation("sedov", n=24, device=gpu)
            sim.run(2)
            torch.cuda.synchronize()
            results.append({f: sim.local(f).cpu() for f in ("x", "vx", "h", "alpha", "xm", "kx", "du", "c", "nc")})
            if forced:
                groups = (24 ** 3 + 63) // 64
                assert sim.propagator.nl.rows_used > groups  # overflow rows were taken: the first search lost rows
    finally:
        hp.set_staged(old)
    for f in results[0]:
        assert torch.equal(results[0][f], results[1][f]), f


def test_device_check_build_clean():
    """the whole-step cases on the device-check build (SPHX_DEVICE_CHECKS=1): bit-identical, no check fires (LDS
    positions below the staged count, slots below the group's table size)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, SPHX_DEVICE_CHECKS="1")
    env.pop("SPHX_HIP_VARIANT", None)
    p = subprocess.run([sys.executable, os.path.join(root, "tests", "helpers", "staged_block_xg_run.py")], env=env,
                       capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    assert "staged block xg ok" in p.stdout
