"""Neighbor search (OpenMP and HIP) against an fp64 all-pairs oracle at the search's edges.

Every dataset of tests/helpers/neighbor_oracle.py is searched on the CPU and on the GPU and must give the oracle's
neighbor sets and counts exactly: anisotropic and mixed-boundary boxes, particles on the faces, boxes too small for the
fp32 group frame, ragged particle counts and a sub-range, clusters, coincident particles, pairs exactly at the radius
(the test is strict) and one ulp to either side, an h below the fixed-point quantum, and a sparse leaf far larger than
the group that touches it. On the GPU the split, spill and predicted-split kernels are forced and must have run.

The inputs are valid only if no decision hangs on rounding (``test_inputs_are_decided``): long double and float64 agree
on every pair, and no pair other than the constructed boundary pairs comes closer than 1e-12 (relative) to its radius,
so a fused multiply-add in the distance cannot change a set. The figures are in profiles/r19/neighbors_oracle/README.md.
"""

import time

import numpy as np
import pytest
import torch

from helpers import neighbor_oracle as NO
from sphexa_amd.ops import neighbors as N
from sphexa_amd.ops.neighbors import find_neighbors, neighbor_lists_as_sets, packed_table_ints

DEVICES = ["cpu", pytest.param("gpu", marks=pytest.mark.gpu)]
NAMES = list(NO.DATASETS)
PATH_CASES = ["clustered", "aniso_mixed", "boundary_pairs_periodic", "boundary_pairs_open"]
H_CASES = [("clustered", 300), ("aniso_mixed", 250), ("small_box_300", 150)]


def _device(request, dev):
    return request.getfixturevalue("gpu") if dev == "gpu" else torch.device("cpu")


def _search(request, dev, name, first=0, last=None):
    """search dataset ``name`` on ``dev`` without h iteration: (data, per-target sets, oracle rows in sorted order,
    oracle counts, wall time of the search)"""
    c, ref = NO.dataset(name), NO.reference(name)
    d, ot, perm = NO.build(_device(request, dev), c.X, c.h, c.box)
    d.ngmax = c.ngmax
    last = d.size if last is None else last
    t0 = time.perf_counter()
    nl = find_neighbors(d, ot, c.box, first, last, iterate_h=False)
    sets = neighbor_lists_as_sets(nl, d["nc"])
    dt = time.perf_counter() - t0
    M = ref.M[np.ix_(perm[first:last], perm)]
    return d, sets, M, ref.counts[perm[first:last]], dt


def _report(name, dev, d, M, dt):
    paths = ""
    if dev == "gpu":
        paths = f" queued={d.nc_queued} split={d.nc_split} predicted={d.nc_predicted} spilled={d.nc_spilled}"
    print(f"oracle-case {name} {dev}: N={d.size} pairs={int(M.sum())}{paths} time={dt:.2f}s")


def _assert_oracle(d, sets, M, counts, first=0):
    nc = d["nc"].cpu().numpy().astype(np.int64)[first:first + len(counts)]
    bad = np.flatnonzero(nc != counts + 1)
    assert not len(bad), f"nc of {len(bad)} targets, first {first + bad[0]}: {nc[bad[0]]} != {counts[bad[0]] + 1}"
    diff = NO.mismatches(sets, M, first)
    assert not diff, diff


@pytest.mark.parametrize("name", NAMES)
def test_inputs_are_decided(name):
    """the validity conditions of a dataset, on the oracle alone"""
    c, ref = NO.dataset(name), NO.reference(name)
    print(f"oracle-input {name}: N={c.n} pairs={int(ref.counts.sum())} max={int(ref.counts.max())} "
          f"margin={ref.margin:.3e} constructed={len(c.constructed)}")
    assert ref.differ == []  # the constructed pairs included
    assert ref.margin > NO.MARGIN_MIN
    assert int(ref.counts.max()) <= c.ngmax  # no list is truncated
    assert 150 <= c.ngmax <= 300 and packed_table_ints(c.ngmax) <= 64
    assert c.n <= 4097
    assert (c.X >= np.array(c.box.lo)).all() and (c.X <= np.array(c.box.hi)).all()


def test_boundary_pairs_are_what_they_claim():
    """exact separations of 2h are no neighbors, one ulp inside is, one ulp outside is not; every kind of construct
    occurs both inside one 64-particle group and across groups (by the particles' SFC order)"""
    for name in ("boundary_pairs_periodic", "boundary_pairs_open"):
        c, ref = NO.dataset(name), NO.reference(name)
        pairs = np.array(c.constructed)
        d2 = np.array([NO._dist_sq(c.X[i:i + 1], c.X[j:j + 1], c.box)[0, 0] for i, j in pairs])
        r2 = NO.radius_sq(c.h)[pairs[:, 0]]
        hit = ref.M[pairs[:, 0], pairs[:, 1]]
        near = d2 <= 1.0001 * r2  # (the wrap constructs are far apart in the open box)
        assert near.sum() == (132 if name.endswith("periodic") else 96)
        assert (d2 == r2).sum() == near.sum() // 3 and not hit[d2 == r2].any()
        assert hit[near].sum() == near.sum() // 3 and (hit == (d2 < r2)).all()
        _, _, perm = NO.build("cpu", c.X, c.h, c.box)
        where = np.empty(c.n, dtype=np.int64)
        where[perm] = np.arange(c.n)
        same = where[pairs[:, 0]] // 64 == where[pairs[:, 1]] // 64
        assert (same & near).any() and (~same & near).any()


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("dev", DEVICES)
def test_sets_equal_oracle(request, dev, name):
    d, sets, M, counts, dt = _search(request, dev, name)
    _report(name, dev, d, M, dt)
    _assert_oracle(d, sets, M, counts)


@pytest.mark.parametrize("dev", DEVICES)
def test_subrange_equals_oracle(request, dev):
    """targets [37, n - 21) of the 4097-particle set against all sources: ``first`` is not group-aligned"""
    n = NO.dataset("ragged_4097").n
    d, sets, M, counts, dt = _search(request, dev, "ragged_4097", 37, n - 21)
    _report("ragged_4097[37:n-21]", dev, d, M, dt)
    assert len(sets) == n - 58
    _assert_oracle(d, sets, M, counts, 37)


# ------------------------------------------------------------------------------------------ kernel paths (GPU)
@pytest.mark.gpu
@pytest.mark.parametrize("name", PATH_CASES)
def test_split_kernel_equals_oracle(request, monkeypatch, name):
    """every group through the split kernel's sub-group passes (no prediction: the paths taken do not depend on the
    searches before this one)"""
    monkeypatch.setattr(N, "SPLIT_PREDICT", False)
    monkeypatch.setattr(N, "TEST_FORCE_SPLIT", True)
    d, sets, M, counts, dt = _search(request, "gpu", name)
    _report(name + "/split", "gpu", d, M, dt)
    assert d.nc_split == (d.size + 63) // 64
    _assert_oracle(d, sets, M, counts)


@pytest.mark.gpu
@pytest.mark.parametrize("name", PATH_CASES)
def test_spill_kernel_equals_oracle(request, monkeypatch, name):
    """LDS frontiers of 16 entries: groups overflow down to single-lane passes and take the global-memory kernel
    (no prediction, as above)"""
    monkeypatch.setattr(N, "SPLIT_PREDICT", False)
    monkeypatch.setattr(N, "TEST_FRONT_CAP", 16)
    d, sets, M, counts, dt = _search(request, "gpu", name)
    _report(name + "/spill", "gpu", d, M, dt)
    assert d.nc_spilled > 0
    _assert_oracle(d, sets, M, counts)


@pytest.mark.gpu
@pytest.mark.parametrize("name", PATH_CASES)
def test_predicted_split_equals_oracle(request, monkeypatch, name):
    """the second of two searches hands the groups the first one queued to the split kernel on the second stream"""
    monkeypatch.setattr(N, "TEST_FRONT_CAP", 24)
    monkeypatch.setattr(N, "SPLIT_PREDICT", True)
    N._PRED.clear()
    try:
        for k in range(2):
            d, sets, M, counts, dt = _search(request, "gpu", name)
            _report(name + f"/predict{k}", "gpu", d, M, dt)
            assert d.nc_queued > 0 if k == 0 else d.nc_predicted > 0
            _assert_oracle(d, sets, M, counts)
    finally:
        N._PRED.clear()


# ------------------------------------------------------------------------------------------------- h iteration
@pytest.mark.parametrize("factor", [0.5, 2.0])
@pytest.mark.parametrize("name,ngmax", H_CASES)
@pytest.mark.parametrize("dev", DEVICES)
def test_h_iteration_ends_on_oracle_sets(request, dev, name, ngmax, factor):
    """from an h wrong by ``factor`` the coupled iteration ends within [ng0 / 4, ngmax + 1], and the lists it returns
    are the oracle's sets at the device's own final h (nothing of the CPU search's iteration enters).

    Not covered: a particle between a sparse background and a dense core. ``clustered`` keeps its tight cores in
    corners of the box with a seed that leaves no background particle next to them (helpers/neighbor_oracle.py
    _clustered): such a particle's count jumps across the whole window within a few per cent of h, the 10 rounds end
    without convergence, and this test requires nc_fail == 0."""
    c = NO.dataset(name)
    d, ot, perm = NO.build(_device(request, dev), c.X, (c.h * np.float32(factor)).astype(np.float32), c.box)
    d.ng0, d.ngmax = 50, ngmax
    nl = find_neighbors(d, ot, c.box, 0, d.size, iterate_h=True)
    sets = neighbor_lists_as_sets(nl, d["nc"])
    assert d.nc_fail == 0
    nc = d["nc"].cpu().numpy()
    assert (nc >= d.ng0 // 4).all() and (nc - 1 <= d.ngmax).all()
    X, h = c.X[perm], d["h"].cpu().numpy()
    differ, margin = NO.margins(X, h, c.box)
    print(f"oracle-h {name} {dev} x{factor}: margin={margin:.3e} nc={nc.min()}..{nc.max()}")
    assert differ == [] and margin > NO.MARGIN_MIN
    M, counts = NO.all_pairs(X, h, c.box)
    _assert_oracle(d, sets, M, counts)
