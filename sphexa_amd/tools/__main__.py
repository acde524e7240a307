"""Snapshot utilities (``python -m sphexa_amd.tools <command> ...``).

Parity: reference scripts/ — add_m1.py (create x_m1/y_m1/z_m1/du_m1 for restarting from files that lack them),
init_file.py (write a random initial-conditions file), set_parms.py (create/extend a settings file of key-value
attributes), radial_profile.py and slice.py (inspect a step: radial profile / thin slab of a field),
substep_timings.py (per-substep timing summary of a ``profile`` file). All HDF5 access goes through the native
``_sphx_io`` module (no h5py in this image); plots are written only if matplotlib is importable, otherwise the
data are printed as text columns.

Commands:
  steps FILE                                  list hdf5 step, iteration and time
  add-m1 FILE                                 add x_m1, y_m1, z_m1 (= v * minDt) and du_m1 (= 0) to the last step
  init-file OUT [-n N] [--seed S]             random initial conditions (unit cube, T = 273, v ~ U(0, 0.1))
  set-parms FILE [-a] --key value ...         write settings as file attributes
  radial-profile FILE FIELD [-s STEP] [--bins B]
  slice FILE FIELD [-s STEP] [--axis z] [--width W]
  image FILE FIELD [-s STEP] [--kind slice|projection|render] [--axis z] [--kappa K] [--res 512] [--device cuda]
        [-o out.npy]   (render: opacity rendering [I, T]; --axis=-z views from the far side)
                                              SPH-interpolated slice / column projection (ops/image.py)
  volume FILE FIELD [-s STEP] [--res 128] [--device cuda] [-o out.npy]
                                              SPH-interpolated (res, res, res) grid of FIELD (ops/volume.py)
  spectrum FILE [-s STEP] [--fields vx,vy,vz] [--res 128] [--device cuda] [-o spectrum.txt]
                                              shell-binned power spectrum of the interpolated fields: k, P, count
  fof FILE [-s STEP] [--b 0.2 | --ll L] [--rho-min R] [--min-members 20] [--device cuda] [-o groups.txt]
      [--labels labels.npy]                   friends-of-friends groups (ops/fof.py): label count mass cx cy cz vx vy vz
      [--bound [--eps E] [--G g] [--max-iter K] [--thermal] [--bound-mask FILE.npy]]
                                              unbinds the groups (ops/groups.py; eps defaults to 0.1 linking lengths) and
                                              adds: bound_count bound_mass bvx bvy bvz ekin eint epot px py pz most_bound
      [--so 200[,500] --so-rmax R [--profile-bins B --profile-rmin r] [--profiles-out FILE]]
                                              spherical-overdensity radii and masses against the box mean density
                                              (ops/profiles.py) about the bound centre (with --bound) or the centre of
                                              mass; adds per overdensity: R M N truncated; the profiles go to FILE as
                                              group r_lo r_hi count mass density vr sigma_r sigma
  pairs FILE [-s STEP] --rmin A --rmax B --bins N [--log] [--velocity] [--mass] [--stride K] [--device cuda]
      [-o pairs.txt]                          pair counts per radial bin (ops/pairstats.py): r_lo r_hi count [ww]
                                              [S2L S2T S3L] [xi]
  substep-timings PROFILE
"""

from __future__ import annotations

import argparse
import os
import sys

import numpy as np

from ..ops import _lib


def _steps(path):
    io = _lib.io()
    f = io.open(path, "r")
    out = []
    for s in range(io.num_steps(f)):
        g = io.open_step(f, s)
        a = dict(io.read_attrs(g))
        out.append((s, int(np.ravel(a.get("iteration", [s]))[0]), float(np.ravel(a.get("time", [0.0]))[0])))
        io.close_group(g)
    io.close(f)
    return out


def cmd_steps(args):
    print(f"{args.file} contains the following steps:")
    print("hdf5 step number".rjust(17), "sph iteration".rjust(15), "time".rjust(15))
    for s, it, t in _steps(args.file):
        print(f"{s:17d} {it:15d} {t:15.6f}")


def cmd_add_m1(args):
    io = _lib.io()
    f = io.open(args.file, "a")
    g = io.open_step(f, io.num_steps(f) - 1)
    attrs = dict(io.read_attrs(g))
    names = set(io.dataset_names(g))
    n = io.dataset_length(g, "x")
    dt = float(np.ravel(attrs["minDt"])[0])
    it = int(np.ravel(attrs.get("iteration", [0]))[0])
    for c, v in (("x_m1", "vx"), ("y_m1", "vy"), ("z_m1", "vz")):
        if c not in names:
            print(f"Adding {c} to SPH iteration {it}")
            data = (io.read_slice(g, v, 0, n, "d") * dt).astype(np.float32)
            io.create_dataset(g, c, "f", n)
            io.write_slice(g, c, data, 0)
    if "du_m1" not in names:
        print(f"Adding du_m1 to SPH iteration {it}")
        io.create_dataset(g, "du_m1", "f", n)
        io.write_slice(g, "du_m1", np.zeros(n, dtype=np.float32), 0)
    io.close_group(g)
    io.close(f)


def cmd_init_file(args):
    io = _lib.io()
    rng = np.random.default_rng(args.seed)
    n = args.n
    min_dt = 1e-7
    alphamin = 0.05
    v = [rng.random(n) * 0.1 for _ in range(3)]
    fields = {
        "x": rng.random(n), "y": rng.random(n), "z": rng.random(n),
        "vx": v[0].astype(np.float32), "vy": v[1].astype(np.float32), "vz": v[2].astype(np.float32),
        "x_m1": (v[0] * min_dt).astype(np.float32), "y_m1": (v[1] * min_dt).astype(np.float32),
        "z_m1": (v[2] * min_dt).astype(np.float32),
        "m": np.full(n, 1.0 / n, dtype=np.float32),
        "h": np.full(n, (0.523 / 100) ** (1.0 / 3.0), dtype=np.float32),
        "du_m1": np.zeros(n, dtype=np.float32), "temp": np.full(n, 273.0),
        "alpha": np.full(n, alphamin, dtype=np.float32),
    }
    f = io.open(args.out, "w")
    g = io.create_step(f, 0)
    attrs = {"iteration": np.array([0], dtype=np.int64), "numParticlesGlobal": np.array([n], dtype=np.int64),
             "time": np.array([0.0]), "minDt": np.array([min_dt]), "minDt_m1": np.array([min_dt]),
             "gravConstant": np.array([0.0]), "alphamin": np.array([alphamin]),
             "box": np.array([0.0, 1.0, 0.0, 1.0, 0.0, 1.0]), "boundaryType": np.array([1, 1, 1], dtype=np.int8)}
    for k, a in attrs.items():
        io.write_attr(g, k, a)
    for k, a in fields.items():
        io.create_dataset(g, k, "d" if a.dtype == np.float64 else "f", n)
        io.write_slice(g, k, a, 0)
    io.close_group(g)
    io.close(f)
    print(f"wrote {n} particles to {args.out}")


def cmd_set_parms(args, extra):
    io = _lib.io()
    f = io.open(args.file, "a" if (args.add and os.path.exists(args.file)) else "w")
    r = io.root(f)
    kv = dict(zip(extra[:-1:2], extra[1::2]))
    for k, v in kv.items():
        key = k.strip("-")
        try:
            val = np.array([int(v)], dtype=np.int64)
        except ValueError:
            val = np.array([float(v)])
        io.write_attr(r, key, val)
    print(f"{args.file} now contains the following settings:")
    for k, v in dict(io.read_attrs(r)).items():
        print("  ", k, np.ravel(v)[0] if np.size(v) == 1 else v)
    io.close_group(r)
    io.close(f)


def _read(path, step, names):
    io = _lib.io()
    f = io.open(path, "r")
    ns = io.num_steps(f)
    if step is None:
        hstep = ns - 1
    else:
        match = [s for s, it, _ in _steps(path) if it == step]
        if not match:
            io.close(f)
            raise SystemExit(f"{path}: iteration {step} not found")
        hstep = match[0]
    g = io.open_step(f, hstep)
    n = io.dataset_length(g, "x")
    out = {k: io.read_slice(g, k, 0, n, "d") for k in names}
    io.close_group(g)
    io.close(f)
    return out


def _quantity(data, what):
    if what == "v":
        return np.sqrt(data["vx"] ** 2 + data["vy"] ** 2 + data["vz"] ** 2)
    return data[what]


def cmd_radial_profile(args):
    names = ["x", "y", "z"] + (["vx", "vy", "vz"] if args.field == "v" else [args.field])
    d = _read(args.file, args.step, names)
    r = np.sqrt(d["x"] ** 2 + d["y"] ** 2 + d["z"] ** 2)
    q = _quantity(d, args.field)
    edges = np.linspace(0, r.max(), args.bins + 1)
    idx = np.clip(np.digitize(r, edges) - 1, 0, args.bins - 1)
    mean = np.bincount(idx, q, args.bins) / np.maximum(np.bincount(idx, minlength=args.bins), 1)
    try:
        import matplotlib

        matplotlib.use("Agg")
        import matplotlib.pyplot as plt

        plt.scatter(r, q, s=0.1)
        plt.xlabel("r")
        plt.ylabel(args.field)
        plt.savefig(f"radial_{args.field}.png")
        print(f"wrote radial_{args.field}.png")
    except ImportError:
        pass
    print("# r_center mean_" + args.field)
    for c, m in zip(0.5 * (edges[1:] + edges[:-1]), mean):
        print(f"{c:.6e} {m:.6e}")


def cmd_slice(args):
    names = ["x", "y", "z"] + (["vx", "vy", "vz"] if args.field == "v" else [args.field])
    d = _read(args.file, args.step, names)
    ax = "xyz".index(args.axis)
    others = [c for c in "xyz" if c != args.axis]
    coord = d[args.axis]
    sel = np.abs(coord - args.center) < 0.5 * args.width
    q = _quantity(d, args.field)[sel]
    a, b = d[others[0]][sel], d[others[1]][sel]
    try:
        import matplotlib

        matplotlib.use("Agg")
        import matplotlib.pyplot as plt

        plt.scatter(a, b, c=q, s=0.2)
        plt.colorbar()
        plt.savefig(f"slice_{args.field}.png")
        print(f"wrote slice_{args.field}.png")
    except ImportError:
        pass
    print(f"# {others[0]} {others[1]} {args.field}  ({sel.sum()} particles in |{args.axis}-{args.center}|<"
          f"{args.width / 2})")
    for row in zip(a, b, q):
        print(" ".join(f"{v:.6e}" for v in row))
    del ax


def _step_box(args):
    """(step attributes, box) of the step that ``args`` names (default: the last)"""
    from ..utils.box import Box

    io = _lib.io()
    f = io.open(args.file, "r")
    g = io.open_step(f, io.num_steps(f) - 1 if args.step is None else
                     next((s for s, it, _ in _steps(args.file) if it == args.step), io.num_steps(f) - 1))
    attrs = dict(io.read_attrs(g))
    io.close_group(g)
    io.close(f)
    return attrs, Box.from_attributes(np.ravel(attrs["box"]), np.ravel(attrs["boundaryType"]))


def cmd_image(args):
    """kernel-weighted slice (volume-weighted field average, V = m / rho) or mass-weighted column projection of FIELD;
    ``rho``: the SPH density (slice) or the column density (projection). Writes the (res, res) array as .npy.
    ``--kind render``: the opacity rendering of FIELD as emission (ops/image.py), opacity ``--kappa`` per mass (default:
    mean optical depth 1 over the box's face), front to back along ``--axis`` (-x, -y, -z: from the far side); writes the
    (2, res, res) stack [I, T]"""
    import torch

    from ..ops.image import sph_image

    attrs, box = _step_box(args)
    render = args.kind == "render"
    if (args.axis.startswith("-") or args.kappa is not None) and not render:
        raise SystemExit("a signed --axis and --kappa belong to --kind render")
    need = ["x", "y", "z", "h", "m"] + ([] if args.field == "rho" else
                                        (["vx", "vy", "vz"] if args.field == "v" else [args.field]))
    need += ["rho"] if (args.field != "rho" and args.kind == "slice") or (args.field == "rho" and render) else []
    d = _read(args.file, args.step, need)
    dev = torch.device(args.device)
    m = d["m"]
    if render:
        # channel 0: kappa m, channel 1: the field. Default kappa: mean optical depth 1 over the box's face
        a = "xyz".index(args.axis[-1])
        area = (box.hi[(a + 1) % 3] - box.lo[(a + 1) % 3]) * (box.hi[(a + 2) % 3] - box.lo[(a + 2) % 3])
        kappa = area / float(np.sum(m, dtype=np.float64)) if args.kappa is None else args.kappa
        w = [kappa * m, d["rho"] if args.field == "rho" else _quantity(d, args.field)]
    elif args.field == "rho":
        w = [m]
    else:
        vol = m / d["rho"] if args.kind == "slice" else m
        w = [vol * _quantity(d, args.field), vol]
    t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt).to(dev)
    img = sph_image(t(d["x"], torch.float64), t(d["y"], torch.float64), t(d["z"], torch.float64),
                    t(d["h"], torch.float32), t(np.stack(w), torch.float32), box, kind=args.kind, axis=args.axis,
                    res=(args.res, args.res), sinc_index=float(np.ravel(attrs.get("sincIndex", [6.0]))[0]))
    if not render:
        img = img[0] if len(w) == 1 else torch.where(img[1] != 0, img[0] / img[1], torch.zeros_like(img[0]))
    img = img.cpu().numpy()
    out = args.out or f"image_{args.field}.npy"
    np.save(out, img)
    print(f"wrote {out}: {args.kind} of {args.field} along {args.axis}, {img.shape[-1]} x {img.shape[-2]} pixels"
          f"{f' x [I, T], kappa {kappa:.6e}' if render else ''}, min {img.min():.6e} max {img.max():.6e}")


def _snapshot_grid(args, fields):
    """FIELD(s) of a step on a (res, res, res) grid over the box: the volume-weighted averages sum V A W / sum V W,
    V = m / rho (``rho`` alone: the SPH density sum m W), as a (len(fields), res, res, res) float32 tensor"""
    import torch

    from ..ops.volume import sph_volume

    attrs, box = _step_box(args)
    density = fields == ["rho"]
    if len(fields) > 3 or (not density and "rho" in fields):
        raise SystemExit("one to three fields; rho only on its own")
    need = ["x", "y", "z", "h", "m"] + ([] if density else ["rho"])
    for name in fields:
        need += [] if name == "rho" else (["vx", "vy", "vz"] if name == "v" else [name])
    d = _read(args.file, args.step, list(dict.fromkeys(need)))
    dev = torch.device(args.device)
    if density:
        w = [d["m"]]
    else:
        vol = d["m"] / d["rho"]
        w = [vol * _quantity(d, name) for name in fields]
        w += [np.zeros_like(vol)] * (len(w) == 2) + [vol]  # 2 or 4 channels, the normaliser last
    t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt).to(dev)
    grid = sph_volume(t(d["x"], torch.float64), t(d["y"], torch.float64), t(d["z"], torch.float64),
                      t(d["h"], torch.float32), t(np.stack(w), torch.float32), box, res=(args.res,) * 3,
                      sinc_index=float(np.ravel(attrs.get("sincIndex", [6.0]))[0]))
    if density:
        return grid, box
    n = len(fields)
    return torch.where(grid[-1:] != 0, grid[:n] / grid[-1:], torch.zeros_like(grid[:n])).contiguous(), box


def cmd_volume(args):
    """kernel-weighted grid of FIELD over the box. Writes the (res, res, res) array, indexed (z, y, x), as .npy"""
    grid, _ = _snapshot_grid(args, [args.field])
    vol = grid[0].cpu().numpy()
    out = args.out or f"volume_{args.field}.npy"
    np.save(out, vol)
    print(f"wrote {out}: {args.field} on {vol.shape[2]} x {vol.shape[1]} x {vol.shape[0]} voxels, "
          f"min {vol.min():.6e} max {vol.max():.6e}")


def cmd_spectrum(args):
    """power spectrum of the interpolated fields (default: the velocity) over a cubic box: text columns k, P, count"""
    from ..ops.spectrum import power_spectrum
    from ..utils.box import PERIODIC

    fields = args.fields.split(",")
    grid, box = _snapshot_grid(args, fields)
    L = box.lengths()
    if max(L) - min(L) > 1e-12 * max(L) or any(b != PERIODIC for b in box.bc):
        raise SystemExit(f"spectrum: the box is not cubic and fully periodic (edges {L}, boundaries {box.bc})")
    k, P, count = (t.cpu().numpy() for t in power_spectrum(grid))
    out = args.out or "spectrum.txt"
    np.savetxt(out, np.stack([k, P, count], axis=1), header=f"k P count  ({','.join(fields)}, {args.res}^3)")
    print(f"wrote {out}: {len(k)} shells, sum P {P.sum():.6e}")


def cmd_fof(args):
    """friends-of-friends group catalogue of a step as text columns; the linking length is ``--ll`` or ``--b`` mean
    particle spacings of the box"""
    import torch

    from ..ops.fof import fof_catalog, fof_labels

    _, box = _step_box(args)
    names = ["x", "y", "z", "m", "vx", "vy", "vz"] + (["rho"] if args.rho_min is not None else []) + \
        (["u"] if args.thermal else [])
    d = _read(args.file, args.step, names)
    dev = torch.device(args.device)
    t = {k: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64).to(dev) for k, a in d.items()}
    n = t["x"].numel()
    lx, ly, lz = box.lengths()
    ll = args.ll if args.ll is not None else args.b * (lx * ly * lz / n) ** (1.0 / 3.0)
    select = None if args.rho_min is None else t["rho"] >= args.rho_min
    labels = fof_labels(t["x"], t["y"], t["z"], box, ll, select=select)
    cat = fof_catalog(labels, t["x"], t["y"], t["z"], t["m"], box, min_members=args.min_members,
                      v=(t["vx"], t["vy"], t["vz"]))
    cols = [cat["label"].double(), cat["count"].double(), cat["mass"], *cat["com"].T, *cat["vel"].T]
    fmt, head = ["%d", "%d"] + ["%.17e"] * 7, "label count mass cx cy cz vx vy vz"
    if args.bound:
        from ..ops.groups import bound_groups

        mask, _, bc = bound_groups(labels, t["x"], t["y"], t["z"], t["m"], (t["vx"], t["vy"], t["vz"]), box,
                                   0.1 * ll if args.eps is None else args.eps, G=args.G, u=t.get("u"),
                                   min_members=args.min_members, max_iter=args.max_iter)
        cols += [bc["bound_count"].double(), bc["bound_mass"], *bc["vel"].T, bc["ekin"], bc["eint"], bc["epot"],
                 *bc["centre"].T, bc["most_bound"].double()]
        fmt += ["%d"] + ["%.17e"] * 10 + ["%d"]
        head += f" bound_count bound_mass bvx bvy bvz ekin eint epot px py pz most_bound  ({bc['iterations']} iterations)"
        if args.bound_mask:
            np.save(args.bound_mask, mask.cpu().numpy())
    if args.so:
        from ..ops.profiles import profile_quantities, radial_profiles

        if args.so_rmax is None:
            raise SystemExit("fof: --so needs --so-rmax, the radius out to which the spheres are searched")
        deltas = [float(v) for v in args.so.split(",")]
        rmin = 0.01 * args.so_rmax if args.profile_rmin is None else args.profile_rmin
        edges = np.geomspace(rmin, args.so_rmax, args.profile_bins + 1) if args.profile_bins else \
            np.array([0.0, args.so_rmax])
        nan_to = lambda a, b: torch.where(torch.isnan(a), b, a)
        cen, vc = (nan_to(bc["centre"], cat["com"]), nan_to(bc["vel"], cat["vel"])) if args.bound else \
            (cat["com"], cat["vel"])
        rho_ref = float(t["m"].sum()) / (lx * ly * lz)
        prof = radial_profiles(cen.contiguous(), t["x"], t["y"], t["z"], t["m"], box, edges,
                               v=(t["vx"], t["vy"], t["vz"]), vc=vc.contiguous(),
                               thresholds=[v * rho_ref for v in deltas])
        for k, delta in enumerate(deltas):
            cols += [prof["so_radius"][:, k], prof["so_mass"][:, k], prof["so_count"][:, k].double(),
                     prof["so_truncated"][:, k].double()]
            fmt += ["%.17e", "%.17e", "%d", "%d"]
            head += " R_{0:g} M_{0:g} N_{0:g} truncated_{0:g}".format(delta)
        head += f"  (reference density {rho_ref:.17e}, r_max {args.so_rmax:.17e})"
        if args.profiles_out:
            q = profile_quantities(prof, edges)
            ng, nbins = prof["count"].shape
            e = torch.as_tensor(edges)
            pcols = [torch.arange(ng).repeat_interleave(nbins).double(), e[:-1].repeat(ng), e[1:].repeat(ng),
                     prof["count"].double().flatten(), prof["mass"].flatten(), q["density"].flatten(),
                     q["vr"].flatten(), q["sigma_r"].flatten(), q["sigma"].flatten()]
            np.savetxt(args.profiles_out, torch.stack([c.cpu() for c in pcols], dim=1).numpy(),
                       fmt=["%d", "%.17e", "%.17e", "%d"] + ["%.17e"] * 5,
                       header="group r_lo r_hi count mass density vr sigma_r sigma")
    table = torch.stack([c.cpu() for c in cols], dim=1).numpy() if cat["label"].numel() else np.zeros((0, len(fmt)))
    out = args.out or "groups.txt"
    np.savetxt(out, table, fmt=fmt, header=f"{head}  (linking length {ll:.17e}, min members {args.min_members})")
    if args.labels:
        np.save(args.labels, labels.cpu().numpy())
    print(f"wrote {out}: {table.shape[0]} groups of at least {args.min_members} among {n} particles, linking length "
          f"{ll:.6e}" + (f", largest {int(table[0, 1])} members" if table.shape[0] else ""))


def cmd_pairs(args):
    """pair counts of a step in ``--bins`` linear or logarithmic radial bins between ``--rmin`` and ``--rmax`` as text
    columns; ``--mass`` adds the mass-weighted counts, ``--velocity`` the structure functions, and a fully periodic box
    the two-point correlation function xi"""
    import torch

    from ..ops.pairstats import correlation_function, pair_statistics, structure_functions

    _, box = _step_box(args)
    d = _read(args.file, args.step, ["x", "y", "z"] + (["m"] if args.mass else []) +
              (["vx", "vy", "vz"] if args.velocity else []))
    dev = torch.device(args.device)
    t = {k: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64).to(dev) for k, a in d.items()}
    n = t["x"].numel()
    edges = (np.geomspace if args.log else np.linspace)(args.rmin, args.rmax, args.bins + 1)
    select = None if args.stride <= 1 else torch.arange(n, device=dev) % args.stride == 0
    stats = pair_statistics(t["x"], t["y"], t["z"], box, edges, w=t["m"] if args.mass else None,
                            v=(t["vx"], t["vy"], t["vz"]) if args.velocity else None, select=select)
    e = torch.as_tensor(edges)
    names, cols = ["r_lo", "r_hi", "count"], [e[:-1], e[1:], stats["count"].double()]
    if args.mass:
        names, cols = names + ["ww"], cols + [stats["ww"]]
    if args.velocity:
        sf = structure_functions(stats)
        names, cols = names + ["S2L", "S2T", "S3L"], cols + [sf["S2L"], sf["S2T"], sf["S3L"]]
    if all(bc == 1 for bc in box.bc):
        taking_part = n if select is None else int(select.sum())
        names, cols = names + ["xi"], cols + [correlation_function(stats, edges, taking_part, box)]
    out = args.out or "pairs.txt"
    np.savetxt(out, torch.stack([c.cpu() for c in cols], dim=1).numpy(), fmt="%.17e",
               header=" ".join(names) + f"  ({stats['pairs_bound']} candidate pairs)")
    print(f"wrote {out}: {int(stats['count'].sum())} pairs of {n} particles in {args.bins} bins")


def cmd_substep_timings(args):
    """the profile file holds blocks: 'numRanks R numIterations K', a header of substep names, one row of times"""
    with open(args.profile) as fh:
        lines = [l.split() for l in fh if l.strip()]
    blocks = []
    i = 0
    while i + 2 < len(lines) + 1 and i < len(lines):
        if lines[i][0] == "numRanks":
            names, vals = lines[i + 1], [float(v) for v in lines[i + 2]]
            blocks.append((int(lines[i][3]), names, vals))
            i += 3
        else:
            i += 1
    if not blocks:
        raise SystemExit("no timing blocks found")
    iters, names, vals = blocks[-1]
    total = sum(vals)
    print(f"{'substep':32s} {'s/iteration':>12s} {'share':>7s}")
    for n, v in sorted(zip(names, vals), key=lambda t: -t[1]):
        per = v / max(iters, 1)
        print(f"{n:32s} {per:12.6f} {100 * v / total:6.1f}%")


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m sphexa_amd.tools", description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    p = sub.add_parser("steps")
    p.add_argument("file")
    p = sub.add_parser("add-m1")
    p.add_argument("file")
    p = sub.add_parser("init-file")
    p.add_argument("out")
    p.add_argument("-n", type=int, default=10000)
    p.add_argument("--seed", type=int, default=0)
    p = sub.add_parser("set-parms")
    p.add_argument("file")
    p.add_argument("-a", "--add", action="store_true")
    for name in ("radial-profile", "slice"):
        p = sub.add_parser(name)
        p.add_argument("file")
        p.add_argument("field")
        p.add_argument("-s", "--step", type=int, default=None)
        if name == "radial-profile":
            p.add_argument("--bins", type=int, default=50)
        else:
            p.add_argument("--axis", default="z")
            p.add_argument("--center", type=float, default=0.0)
            p.add_argument("--width", type=float, default=0.02)
    p = sub.add_parser("image")
    p.add_argument("file")
    p.add_argument("field")
    p.add_argument("-s", "--step", type=int, default=None)
    p.add_argument("--kind", choices=["slice", "projection", "render"], default="slice")
    p.add_argument("--axis", default="z", choices=["x", "y", "z", "-x", "-y", "-z"])
    p.add_argument("--kappa", type=float, default=None)
    p.add_argument("--res", type=int, default=512)
    p.add_argument("--device", default="cuda")
    p.add_argument("-o", "--out", default=None)
    for name in ("volume", "spectrum"):
        p = sub.add_parser(name)
        p.add_argument("file")
        if name == "volume":
            p.add_argument("field")
        else:
            p.add_argument("--fields", default="vx,vy,vz")
        p.add_argument("-s", "--step", type=int, default=None)
        p.add_argument("--res", type=int, default=128)
        p.add_argument("--device", default="cuda")
        p.add_argument("-o", "--out", default=None)
    p = sub.add_parser("fof")
    p.add_argument("file")
    p.add_argument("-s", "--step", type=int, default=None)
    g = p.add_mutually_exclusive_group()
    g.add_argument("--b", type=float, default=0.2)
    g.add_argument("--ll", type=float, default=None)
    p.add_argument("--rho-min", type=float, default=None)
    p.add_argument("--min-members", type=int, default=20)
    p.add_argument("--device", default="cuda")
    p.add_argument("-o", "--out", default=None)
    p.add_argument("--labels", default=None)
    p.add_argument("--bound", action="store_true")
    p.add_argument("--eps", type=float, default=None)
    p.add_argument("--G", type=float, default=1.0)
    p.add_argument("--max-iter", type=int, default=20)
    p.add_argument("--thermal", action="store_true")
    p.add_argument("--bound-mask", default=None)
    p.add_argument("--so", default=None)
    p.add_argument("--so-rmax", type=float, default=None)
    p.add_argument("--profile-bins", type=int, default=0)
    p.add_argument("--profile-rmin", type=float, default=None)
    p.add_argument("--profiles-out", default=None)
    p = sub.add_parser("pairs")
    p.add_argument("file")
    p.add_argument("-s", "--step", type=int, default=None)
    p.add_argument("--rmin", type=float, required=True)
    p.add_argument("--rmax", type=float, required=True)
    p.add_argument("--bins", type=int, required=True)
    p.add_argument("--log", action="store_true")
    p.add_argument("--velocity", action="store_true")
    p.add_argument("--mass", action="store_true")
    p.add_argument("--stride", type=int, default=1)
    p.add_argument("--device", default="cuda")
    p.add_argument("-o", "--out", default=None)
    p = sub.add_parser("substep-timings")
    p.add_argument("profile")
    args, extra = ap.parse_known_args(argv)
    if args.cmd == "set-parms":
        cmd_set_parms(args, extra)
    else:
        if extra:
            ap.error(f"unrecognized arguments: {' '.join(extra)}")
        {"steps": cmd_steps, "add-m1": cmd_add_m1, "init-file": cmd_init_file, "radial-profile": cmd_radial_profile,
         "slice": cmd_slice, "image": cmd_image, "volume": cmd_volume, "spectrum": cmd_spectrum, "fof": cmd_fof,
         "pairs": cmd_pairs, "substep-timings": cmd_substep_timings}[args.cmd](args)
    return 0


if __name__ == "__main__":
    sys.exit(main())
