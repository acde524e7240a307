#!/usr/bin/env python3
"""Share of blocks that the block-union staged loops (csrc/hip/staged.h; --mask 66 = XMass and Gradh, 12 = IAD and AV,
+ 32 in 256-thread runs) stage in LDS or hand to the gathered loop, counted by the kernels themselves over a few steps
of a case.

  python scripts/staged_block_share.py --init sedov -n 400 [--mask 44]
"""

import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--init", default="sedov")
    ap.add_argument("-n", type=int, default=100)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--mask", type=int, default=4 | 8 | 32, help="staged bits (hydro.hip g_staged)")
    args = ap.parse_args()
    from sphexa_amd.app.simulation import Simulation
    from sphexa_amd.ops import _lib

    dev = torch.device("cuda", 0)
    hp = _lib.hip()
    counters = torch.zeros(2, dtype=torch.int32, device=dev)
    hp.set_staged(args.mask)
    hp.set_staged_counters(counters.data_ptr())
    try:
        sim = Simulation(args.init, n=args.n, prop="ve", device=dev, out=None, quiet=True)
        for _ in range(args.steps):
            sim.step()
        torch.cuda.synchronize()
    finally:
        hp.set_staged_counters(0)
    staged, fell = (int(c) for c in counters.cpu())
    total = max(staged + fell, 1)
    print(f"case {args.init} -n {args.n}, {args.steps} steps, staged mask {args.mask}: blocks staged {staged}, "
          f"fallen back {fell} ({100.0 * fell / total:.2f} %)")


if __name__ == "__main__":
    main()
