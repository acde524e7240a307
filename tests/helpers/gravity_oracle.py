"""fp64 oracle of the Barnes-Hut gravity evaluation (tests/test_gravity_oracle.py).

Plain numpy, nothing from csrc/include/sphx/gravity.hpp: the traversal is written from its rule, the interactions from
the formulas (Hernquist 1987 quadrupole M2P, softened pairs). An fp64 evaluation of exactly the interactions a kernel
was given differs from the kernel by rounding only, so the comparison carries no Barnes-Hut truncation.

Interaction lists are a list with one entry per target group (None: a fallback group that carries no lists):
    {"both": ids, "A": ids, "B": ids, "leaves": ids, "masks": half masks of the leaves (1 = A, 2 = B, 3 = both),
     "ambiguous": entries whose MAC test is decided within rounding}
Targets of group g are first + g * group + lane; lanes 0-31 are half A, 32-63 half B (groups of 16: all "A").
The formulas of ``budget`` are written out in profiles/r11/gravity_oracle.md.
"""

import numpy as np

U = 2.0 ** -24  # unit roundoff of fp32
HALF_A, HALF_B = 1, 2
GUARD = (2 * 4e-6 / 6e-8) ** 0.5  # |x_s| + |x_t| over (h_s + h_t) admitted by the guard of the MFMA P2P tile
MFMA_P2P_TOL = 4e-6  # tolerated R2 error of the expanded-form P2P tile over (h_s + h_t)^2 (gravity.hip kMfmaP2PTol)


class Tree:
    """host arrays of an octree and its multipoles, as the kernels are given them"""

    def __init__(self, ot, centers, mp):
        self.child = ot.child_offsets.cpu().numpy().astype(np.int64)
        self.n2l = ot.node_to_leaf.cpu().numpy().astype(np.int64)
        self.ns = ot.node_start.cpu().numpy().astype(np.int64)
        self.ne = ot.node_end.cpu().numpy().astype(np.int64)
        c = centers.cpu().numpy().reshape(-1, 4)
        self.c = c[:, :3].copy()
        self.mac = c[:, 3].copy()
        self.q = mp.cpu().numpy().reshape(-1, 8).astype(np.float64)  # float32 values, exactly
        self.N = self.child.size


def _box(p):
    lo, hi = p.min(0), p.max(0)
    return 0.5 * (lo + hi), 0.5 * (hi - lo)


def group_targets(first, last, group, g, clamp):
    """particle indices of the lanes of group g (``clamp``: lanes past ``last`` repeat particle last - 1)"""
    i = first + g * group + np.arange(group)
    return np.minimum(i, last - 1) if clamp else i[i < last]


def walk(tree, x, y, z, first, last, group=64, halves=True, stack_cap=None):
    """interaction lists of every target group from the traversal rule: a node is opened for a half when the squared
    distance of its center to the half's box is below macSq (negative: never opened; zero: empty, no contribution);
    an accepted non-empty node is M2P for the halves that accepted it, an opened leaf P2P for the halves that opened
    it, children inherit the opening mask. With ``stack_cap`` the nodes are taken 64 at a time (one per lane of a
    wave) from the top of a stack and the children of an opened node pushed in their place: a group whose stack would exceed the capacity is
    marked "overflow" (its lists are complete all the same)."""
    X = np.stack([x, y, z], 1)
    out = []
    for g in range((last - first + group - 1) // group):
        idx = group_targets(first, last, group, g, halves)
        boxes = [_box(X[idx[:32]]), _box(X[idx[32:]])] if halves else [_box(X[idx])]
        nodes = np.zeros(1, np.int64)
        masks = np.full(1, 3 if halves else 1, np.int64)
        acc_n, acc_m, lf_n, lf_m, amb, overflow = [], [], [], [], 0, False
        while nodes.size:
            take = nodes.size if stack_cap is None else min(nodes.size, 64)
            rest_n, rest_m = nodes[:nodes.size - take], masks[:nodes.size - take]
            nodes, masks = nodes[nodes.size - take:], masks[masks.size - take:]
            c, mac = tree.c[nodes], tree.mac[nodes]
            opened = np.zeros(nodes.size, np.int64)
            for b, (bc, bs) in enumerate(boxes):
                d = np.abs(bc - c) - bs
                d = np.where(d > 0, d, 0.0)
                r2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
                walks = (masks >> b) & 1
                opened |= ((r2 < mac) & (walks == 1)).astype(np.int64) << b
                amb += int(((np.abs(r2 - mac) <= 1e-12 * mac) & (walks == 1) & (mac > 0)).sum())
            accepted = masks & ~opened
            isacc = (accepted != 0) & (mac != 0)
            acc_n.append(nodes[isacc])
            acc_m.append(accepted[isacc])
            leaf = tree.n2l[nodes] >= 0
            isl = leaf & (opened != 0)
            lf_n.append(nodes[isl])
            lf_m.append(opened[isl])
            inner = ~leaf & (opened != 0)
            kids = (tree.child[nodes[inner]][:, None] + np.arange(8)[None, :]).ravel()
            nodes = np.concatenate([rest_n, kids])
            masks = np.concatenate([rest_m, np.repeat(opened[inner], 8)])
            overflow = overflow or (stack_cap is not None and nodes.size > stack_cap)
        an, am = np.concatenate(acc_n), np.concatenate(acc_m)
        lv, lm = np.concatenate(lf_n), np.concatenate(lf_m)
        out.append({"both": an[am == (3 if halves else 1)], "A": an[(am == 1) & halves], "B": an[am == 2],
                    "leaves": lv, "masks": lm if halves else np.full(lv.size, 3, np.int64), "ambiguous": amb,
                    "overflow": overflow})
    return out


def from_slabs(gl, layout):
    """the lists of ``walk`` read from the GPU slabs of a GravityLists (``layout``: gravity_scratch_layout): counts
    [4g..4g+3] = nm, nl, nA, nB; both-half nodes at the front of mlist, A-only nodes at its back, tagged leaves at the
    front of llist, B-only nodes at its back; groups with count -1 are fallback groups (None). Also returns pcount."""
    s = gl.scratch.cpu().numpy().view(np.int32)
    cap_m, cap_l = gl.caps
    groups = (gl.last - gl.first + 63) // 64
    shift, idm = int(layout["tag_shift"]), int(layout["id_mask"])
    counts = s[layout["counts"]:layout["counts"] + 4 * groups].reshape(groups, 4).astype(np.int64)
    pcount = s[layout["pcount"]:layout["pcount"] + groups].astype(np.int64)
    out = []
    for g in range(groups):
        nm, nl, nA, nB = counts[g]
        if nm < 0 or nl < 0:
            assert nm == -1 and nl == -1, counts[g]
            out.append(None)
            continue
        assert nm + nA <= cap_m and nl + nB <= cap_l, (counts[g], gl.caps)
        ml = s[layout["mlist"] + g * cap_m:layout["mlist"] + (g + 1) * cap_m].astype(np.int64)
        ll = s[layout["llist"] + g * cap_l:layout["llist"] + (g + 1) * cap_l].astype(np.int64)
        lv = ll[:nl] & 0xFFFFFFFF
        out.append({"both": ml[:nm], "A": ml[cap_m - nA:], "B": ll[cap_l - nB:], "leaves": lv & idm,
                    "masks": lv >> shift, "ambiguous": 0})
    return out, pcount


def frame(x, y, z):
    """origin and quantum of the 31-bit fixed-point frame of the P2P source records: 1.5 x the particles' extent"""
    X = np.stack([x, y, z], 1)
    lo, hi = X.min(0), X.max(0)
    L = np.maximum(1.5 * (hi - lo), 1e-12 * np.maximum(np.abs(lo), np.abs(hi)) + 1e-300)
    return lo - 0.25 * (hi - lo), L / 2.0 ** 31


def _m2p(r, q):
    """Hernquist quadrupole M2P of nodes q (K, 8) on separations r (T, K, 3): phi (T, K), a (T, K, 3)"""
    Q = np.empty((q.shape[0], 3, 3))
    Q[:, 0, 0], Q[:, 0, 1], Q[:, 0, 2] = q[:, 1], q[:, 2], q[:, 3]
    Q[:, 1, 0], Q[:, 1, 1], Q[:, 1, 2] = q[:, 2], q[:, 4], q[:, 5]
    Q[:, 2, 0], Q[:, 2, 1], Q[:, 2, 2] = q[:, 3], q[:, 5], q[:, 6]
    r2 = (r * r).sum(-1)
    rm1 = 1.0 / np.sqrt(r2)
    rm2 = rm1 * rm1
    rm5 = rm2 * rm2 * rm1
    Qr = np.einsum("kab,tkb->tka", Q, r)
    rQr = (r * Qr).sum(-1)
    M = q[:, 0][None, :]
    phi = -(M * rm1 + 0.5 * rm5 * rQr)
    a = rm5[..., None] * Qr + ((-2.5 * rQr * rm5 - M * rm1) * rm2)[..., None] * r
    return phi, a


def evaluate(lists, tree, x, y, z, h, m, first, last, group=64, halves=True, with_budget=False):
    """phi and a (G = 1, per unit target mass) of every target in [first, last) from the interaction lists, fp64, with
    the float32 quadrupoles and h, m and the fp64 centers and positions as the kernels read them. Returns a dict:
    phi (n), a (n, 3), Sa / Sphi = sum of |contribution| over the target's interactions (the forward-error scales),
    m2p / p2p = per-group interaction counts in half-group units (2 per entry of both halves), and with
    ``with_budget`` the per-target rounding budgets Ba, Bphi, Ba0, Bphi0 (without the accumulation term) and Bself
    (the share of Ba0 allowed to sources at the target's own position on the MFMA tile)."""
    X = np.stack([x, y, z], 1)
    h = h.astype(np.float64)
    m = m.astype(np.float64)
    n = last - first
    keys = ("phi", "Sa", "Sphi") + (("Ba", "Bphi", "Ba0", "Bphi0", "Bself") if with_budget else ())
    res = {k: np.zeros(n) for k in keys}
    res["a"] = np.zeros((n, 3))
    res["m2p"], res["p2p"] = [], []
    org, quant = frame(x, y, z)
    for g, L in enumerate(lists):
        idx = group_targets(first, last, group, g, False)
        nt = idx.size
        sl = slice(idx[0] - first, idx[0] - first + nt)
        lane = np.arange(nt)
        half = np.where(lane < 32, HALF_A, HALF_B) if halves else np.full(nt, 3)
        xt = X[idx]
        gc, _ = _box(X[group_targets(first, last, group, g, halves)])  # the group box center the offsets refer to
        dt = np.abs(xt - gc)                                           # |x_t - c| per dimension
        rgroup = np.sqrt((dt * dt).sum(1)).max()
        # ---------------------------------------------------------------- M2P
        nodes = np.concatenate([L["both"], L["A"], L["B"]])
        nmask = np.concatenate([np.full(L["both"].size, 3), np.full(L["A"].size, 1), np.full(L["B"].size, 2)])
        res["m2p"].append(2 * L["both"].size + L["A"].size + L["B"].size)
        nint = np.zeros(nt)
        if nodes.size:
            on = (nmask[None, :] & half[:, None]) != 0
            q = tree.q[nodes]
            r = xt[:, None, :] - tree.c[nodes][None, :, :]
            with np.errstate(divide="ignore", invalid="ignore"):
                phi, a = _m2p(r, q)
            phi = np.where(on, phi, 0.0)
            a = np.where(on[..., None], a, 0.0)
            res["phi"][sl] += phi.sum(1)
            res["a"][sl] += a.sum(1)
            an = np.sqrt((a * a).sum(-1))
            res["Sa"][sl] += an.sum(1)
            res["Sphi"][sl] += np.abs(phi).sum(1)
            nint += on.sum(1)
            if with_budget:
                rr = np.where(on, np.sqrt((r * r).sum(-1)), 1.0)
                M = np.abs(q[:, 0])[None, :]
                qn = np.sqrt(q[:, 1] ** 2 + q[:, 4] ** 2 + q[:, 6] ** 2 +
                             2 * (q[:, 2] ** 2 + q[:, 3] ** 2 + q[:, 5] ** 2))[None, :]
                # node record fp32 offsets from the frame origin, the group center's, the targets' from the center
                dr = U * (np.linalg.norm(tree.c[nodes] - org, axis=1)[None, :] + np.linalg.norm(gc - org) +
                          np.linalg.norm(dt, axis=1)[:, None])
                amono, aquad = M / rr ** 2, 3.5 * qn / rr ** 4
                pmono, pquad = M / rr, 0.5 * qn / rr ** 3
                form = U * qn * (rr + rgroup)  # Q t - Q c on the matrix cores
                ba = (2 * amono + 4 * aquad) * dr / rr + 3.5 * form / rr ** 5 + 32 * U * (amono + aquad)
                bp = (pmono + 3 * pquad) * dr / rr + 0.5 * form / rr ** 4 + 32 * U * (pmono + pquad)
                ba0, bp0 = np.where(on, ba, 0.0).sum(1), np.where(on, bp, 0.0).sum(1)
                chain = (np.ceil(nint / 8) + 8) * U  # eight partial sums per target, then their combination
                res["Ba0"][sl] += ba0
                res["Bphi0"][sl] += bp0
                res["Ba"][sl] += ba0 + chain * an.sum(1)
                res["Bphi"][sl] += bp0 + chain * np.abs(phi).sum(1)
        # ---------------------------------------------------------------- P2P
        lv, lm = L["leaves"], L["masks"]
        sizes = tree.ne[lv] - tree.ns[lv]
        res["p2p"].append(int((sizes * np.array([0, 1, 1, 2])[lm]).sum()))
        if lv.size and sizes.sum():
            src = np.concatenate([np.arange(a, b) for a, b in zip(tree.ns[lv], tree.ne[lv])])
            smask = np.repeat(lm, sizes)
            on = (smask[None, :] & half[:, None]) != 0
            d = X[src][None, :, :] - xt[:, None, :]
            r2 = (d * d).sum(-1)
            hs = h[src][None, :] + h[idx][:, None]
            h2 = hs * hs
            w = np.where(on, m[src][None, :] / np.maximum(r2, h2) ** 1.5, 0.0)
            phi = -w * r2
            a = w[..., None] * d
            res["phi"][sl] += phi.sum(1)
            res["a"][sl] += a.sum(1)
            rr = np.sqrt(r2)
            res["Sa"][sl] += (w * rr).sum(1)
            res["Sphi"][sl] += np.abs(phi).sum(1)
            if with_budget:
                ds = np.abs(X[src] - gc)
                # offsets from the quantised group center: one fp32 rounding of |x - c| and half a quantum each
                es = np.linalg.norm(U * ds + 0.5 * quant, axis=1)[None, :]
                et = np.linalg.norm(U * dt + 0.5 * quant, axis=1)[:, None]
                dts = np.where(r2 > 0, es + et, 0.0)  # identical records give exactly zero separation
                er2 = np.where(r2 > 0, np.maximum(2 * rr * dts, MFMA_P2P_TOL * h2), 0.0)
                unsoft = r2 + er2 >= h2
                reff2 = np.maximum(r2, h2)
                ba = w * dts + 12 * U * w * rr + np.where(unsoft, 1.5 * w * er2 * rr / reff2, 0.0)
                bp = 12 * U * w * r2 + np.where(unsoft & (r2 >= h2), 0.5 * w * er2, w * er2)
                # a source at the target's own position (the self pair, a coincident particle) is at separation exactly
                # 0 on the VALU pair loop and contributes exactly 0 there. On the MFMA tile it does not: w x_s and
                # x_t sum w are two rounded products of w / (h_s + h_t)^3-sized weights that cancel only to rounding
                nt_c = np.linalg.norm(dt, axis=1)[:, None]
                tile = np.linalg.norm(ds, axis=1)[None, :] + nt_c <= GUARD * hs
                bself = np.where((r2 == 0) & on & tile, 2 * U * w * nt_c, 0.0).sum(1)
                res["Bself"][sl] += bself
                ba0, bp0 = ba.sum(1) + bself, bp.sum(1)
                # the MFMA tile sums w x_s and w apart and subtracts x_t sum w: its roundings scale with the offsets
                # from the group center, not with r; its guard admits a chunk only while |x_s|^2 + |x_t|^2 <=
                # (MFMA_P2P_TOL / 6e-8) (h_s + h_t)^2, so a pair whose offsets exceed GUARD (h_s + h_t) is never on
                # the tile: it runs on the VALU pair loop, whose roundings scale with r
                off = np.linalg.norm(ds, axis=1)[None, :] + np.linalg.norm(dt, axis=1)[:, None]
                soff = (w * np.where(off <= GUARD * hs, off, rr)).sum(1)
                chain = (np.ceil(on.sum(1) / 8) + 8) * U
                res["Ba0"][sl] += ba0
                res["Bphi0"][sl] += bp0
                res["Ba"][sl] += ba0 + chain * soff
                res["Bphi"][sl] += bp0 + chain * np.abs(phi).sum(1)
    return res


def budget(lists, tree, x, y, z, h, m, first, last):
    """per-target rounding budgets (Ba, Bphi) of the GPU evaluation of ``lists`` (profiles/r11/gravity_oracle.md)"""
    r = evaluate(lists, tree, x, y, z, h, m, first, last, with_budget=True)
    return r["Ba"], r["Bphi"]


def direct(x, y, z, h, m, first, last):
    """all-pairs softened sum on targets [first, last): phi, a, Sa"""
    X = np.stack([x, y, z], 1)
    h = h.astype(np.float64)
    m = m.astype(np.float64)
    d = X[None, :, :] - X[first:last, None, :]
    r2 = (d * d).sum(-1)
    hs = h[None, :] + h[first:last, None]
    w = m[None, :] / np.maximum(r2, hs * hs) ** 1.5
    return -(w * r2).sum(1), (w[..., None] * d).sum(1), (w * np.sqrt(r2)).sum(1)


def moments(tree, x, y, z, m):
    """mass, mass center, traceless quadrupole (the 8 entries of the kernels' records) of every node directly from its
    particle range in fp64 (no M2M), with the scale 3 sum m |x - c|^2 of the quadrupole entries and the number of
    tree levels below every node"""
    X = np.stack([x, y, z], 1)
    m = m.astype(np.float64)
    N = tree.N
    mass, com, quad, scale = np.zeros(N), np.zeros((N, 3)), np.zeros((N, 8)), np.zeros(N)
    height = np.zeros(N, np.int64)
    for i in range(N - 1, -1, -1):
        if tree.n2l[i] < 0:
            height[i] = 1 + height[tree.child[i]:tree.child[i] + 8].max()  # children follow their parent
        a, b = tree.ns[i], tree.ne[i]
        if b <= a:
            continue
        mi, xi = m[a:b], X[a:b]
        mass[i] = mi.sum()
        com[i] = (mi[:, None] * xi).sum(0) / mass[i]
        r = xi - com[i]
        S = np.einsum("p,pa,pb->ab", mi, r, r)
        tr = np.trace(S)
        quad[i] = [mass[i], 3 * S[0, 0] - tr, 3 * S[0, 1], 3 * S[0, 2], 3 * S[1, 1] - tr, 3 * S[1, 2],
                   3 * S[2, 2] - tr, tr]
        scale[i] = 3 * tr
    return mass, com, quad, scale, height
