#!/usr/bin/env python3
"""Exact neighbor unions of blocks of 4 and 8 SFC-consecutive 64-target groups, from the OpenMP search (no GPU).

A lower bound of what the block-union staged pair loops (csrc/hip/staged.h) hold in LDS: they stage the in-box
candidates of the groups' slot masks, not only the neighbors (626 candidates against 548 neighbors for one Sedov
group, profiles/r3_perf_log.md). scripts/block_union_stats.py reads the mask unions themselves on the GPU.

  python scripts/block_union_exact.py --init sedov -n 50
"""

import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--init", default="sedov")
    ap.add_argument("-n", type=int, default=50)
    ap.add_argument("--steps", type=int, default=1)
    args = ap.parse_args()
    from sphexa_amd.app.simulation import Simulation

    sim = Simulation(args.init, n=args.n, prop="ve", device=torch.device("cpu"), out=None, quiet=True)
    for _ in range(args.steps):
        sim.step()
    nl = sim.propagator.nl
    assert not nl.grouped
    n = nl.last - nl.first
    idx = nl.nidx[: n * nl.ngmax].view(n, nl.ngmax).long()
    nc = (sim.d["nc"][nl.first:nl.last].long() - 1).clamp(0, nl.ngmax)
    valid = torch.arange(nl.ngmax)[None, :] < nc[:, None]
    own = nl.first + torch.arange(n)
    big = torch.iinfo(torch.int64).max
    rows = torch.cat([torch.where(valid, idx, big), own[:, None]], dim=1)
    print(f"case {args.init} -n {args.n}: {n} particles, mean neighbors {float(nc.float().mean()):.1f}")
    for ng in (1, 4, 8):
        per = 64 * ng
        nb = n // per
        r = rows[: nb * per].reshape(nb, -1)
        srt, _ = r.sort(dim=1)
        new = torch.ones_like(srt, dtype=torch.bool)
        new[:, 1:] = srt[:, 1:] != srt[:, :-1]
        u = (new & (srt != big)).sum(dim=1).float()
        print(f"  exact union of {ng} group(s), {nb} blocks: mean {float(u.mean()):.0f} "
              f"p99 {float(torch.quantile(u, 0.99)):.0f} max {float(u.max()):.0f}")


if __name__ == "__main__":
    main()
