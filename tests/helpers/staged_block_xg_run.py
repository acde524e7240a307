"""Runs under SPHX_DEVICE_CHECKS=1 (device-check HIP build) for tests/test_gpu_staged_block_xg.py: two steps of Sedov,
Noh and Evrard with the block-union staged XMass and Gradh loops, alone and with the staged IAD and AV loops, must equal
the gathered run bit for bit, stage some blocks and fire no device check (Simulation.step raises on one)."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from sphexa_amd.app.simulation import Simulation  # noqa: E402
from sphexa_amd.ops import _lib  # noqa: E402

FIELDS = ("x", "vx", "h", "alpha", "xm", "kx", "du", "c", "nc")
XG = 2 | 64


def run(dev, case, mask, counters):
    hp = _lib.hip()
    hp.set_staged(mask)
    hp.set_staged_counters(counters.data_ptr() if mask else 0)
    try:
        sim = Simulation(case, n=24, prop="ve", device=dev, out=None, quiet=True).run(2)
        _lib.raise_on_device_check(f"{case} staged {mask}")
        torch.cuda.synchronize()
        return {f: sim.local(f).cpu() for f in FIELDS}
    finally:
        hp.set_staged_counters(0)
        hp.set_staged(0)


def main():
    assert os.environ.get("SPHX_DEVICE_CHECKS") == "1"
    dev = torch.device("cuda", 0)
    assert _lib.hip().device_checks_enabled()
    for case in ("sedov", "noh", "evrard"):
        a = run(dev, case, 0, None)
        for mask in (XG | 32, XG | 4 | 8 | 32):
            counters = torch.zeros(2, dtype=torch.int32, device=dev)
            b = run(dev, case, mask, counters)
            staged, fell = (int(c) for c in counters.cpu())
            print(f"{case} mask {mask}: blocks staged {staged}, fallen back {fell}", flush=True)
            assert staged > 0, (case, mask)
            for f in FIELDS:
                assert torch.equal(a[f], b[f]), (case, mask, f)
    print("staged block xg ok", flush=True)


if __name__ == "__main__":
    main()
