#!/usr/bin/env python3
"""Source unions of blocks of SFC-consecutive target groups, from the slot masks of the packed GPU neighbor lists
(design data of the block-union staged pair loops, csrc/hip/staged.h).

For a sample of blocks of 4, 8 and 16 groups (16: the 1024-thread blocks of the XMass and Gradh loops): the merged chunk slots (distinct chunk bases), the records of the merged
masks (what a block stages in LDS), the groups' slot counts, and the share of blocks that fit a capacity.

  python scripts/block_union_stats.py --init sedov -n 200 --caps 1128,2264
"""

import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def pct(t: torch.Tensor, qs=(0.5, 0.9, 0.99, 1.0)):
    t = t.float()
    return " ".join(f"p{int(q * 100)} {float(torch.quantile(t, q)):.0f}" for q in qs) + f" mean {float(t.mean()):.1f}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--init", default="sedov")
    ap.add_argument("-n", type=int, default=100)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--sample-blocks", type=int, default=2048)
    ap.add_argument("--caps", default="1128,2264")
    args = ap.parse_args()
    from sphexa_amd.app.simulation import Simulation
    from sphexa_amd.ops import _lib
    from sphexa_amd.ops.neighbors import GROUP, packed_table_ints, packed_table_region

    _lib.hip().set_list_masks(True)
    dev = torch.device("cuda", 0)
    sim = Simulation(args.init, n=args.n, prop="ve", device=dev, out=None, quiet=True)
    for _ in range(args.steps):
        sim.step()
    nl = sim.propagator.nl
    n = nl.last - nl.first
    G = (n + GROUP - 1) // GROUP
    Ti = packed_table_ints(nl.ngmax)
    tab = nl.nidx[:G * Ti].view(G, Ti).long()
    rows = nl.nidx[packed_table_region(G, nl.ngmax):]
    rows = rows[:rows.numel() // 256 * 256].view(-1, 256)
    nch = tab[:, 1] & 0x3FF
    tc = (tab[:, 1] >> 10) & 0x3F
    print(f"case {args.init} -n {args.n}: {n} particles, {G} groups, ngmax {nl.ngmax}")
    print(f"  slots per group (nch)           {pct(nch)}   groups above 64 slots: {float((nch > 64).float().mean()):.4f}")
    caps = [int(c) for c in args.caps.split(",")]
    s = torch.arange(64, device=dev)
    bit = torch.arange(32, device=dev)
    for ng in (4, 8, 16):
        nb = G // ng
        k = min(args.sample_blocks, nb)
        b0 = (nb - k) // 2
        gs = torch.arange(b0 * ng, (b0 + k) * ng, device=dev)
        live = (s[None, :] >= 1) & (s[None, :] < nch[gs, None].clamp(max=64))
        c0 = rows[tab[gs, 2], :64].long()                      # chunk bases of slots 0..63 (ordinal 0)
        mrow = rows[tab[gs, 2 + tc[gs]], :128].long()          # masks of slots 0..63 (ordinal Tc)
        lo, hi = mrow[:, 0::2], mrow[:, 1::2]
        bits = torch.cat([(lo[:, :, None] >> bit) & 1, (hi[:, :, None] >> bit) & 1], dim=2).bool()  # [g, 64, 64]
        bits &= live[:, :, None]
        j = torch.where(bits, c0[:, :, None] + torch.arange(64, device=dev), -1).view(k, -1)
        srt, _ = j.sort(dim=1)
        new = torch.ones_like(srt, dtype=torch.bool)
        new[:, 1:] = srt[:, 1:] != srt[:, :-1]
        union = (new & (srt >= 0)).sum(dim=1)
        per_group = bits.view(k, ng, -1).sum(dim=2).float().mean()
        cb = torch.where(live, c0, -1).view(k, -1).sort(dim=1)[0]
        newc = torch.ones_like(cb, dtype=torch.bool)
        newc[:, 1:] = cb[:, 1:] != cb[:, :-1]
        merged = (newc & (cb >= 0)).sum(dim=1)
        big = (nch[gs] > 64).view(k, ng).any(dim=1)
        print(f"  blocks of {ng} groups (sample {k}): mask records per single group {float(per_group):.1f}")
        print(f"    merged chunk slots            {pct(merged)}")
        print(f"    records of the merged masks   {pct(union)}")
        for c in caps:
            fit = (union <= c) & ~big
            print(f"    blocks that fit {c:5d} records: {float(fit.float().mean()):.4f}")


if __name__ == "__main__":
    main()
