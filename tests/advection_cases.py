"""Grids and states shared by tests/test_advection_reference.py (CPU: oracle against the long-double reference of
tests/advection_reference.py) and tests/test_advection_device.py (device against that reference): the plain WENO 5 / 7 / 9 momentum and
scalar tendencies.  Halo = (order + 1) / 2 in every non-Flat direction.

Grids, with the tiles and z chunks they produce (Float64; csrc/bz_tendency5.hip: pick_chunk5(fine), csrc/bz_tendency4.hip: pick_chunk_lds,
csrc/bz_tendency.hip: pick_kchunk, csrc/bz_tendency_generic.hip: march_chunk; stretched: z faces Lz linspace(0, 1, Nz + 1)^1.3):
  ragged   (70, 9, 21) stretched, periodic: 2 x 2 tiles of 64 x 8 — a ragged x tile (64 + 6) and a tail row (8 + 1).  Stored-velocity
           k6_u / k6_v / k5_scalar_pair: 4 tiles, fill = 128 capped at Nz / 2 = 10 chunks -> seven chunks of 3 levels; k6_w (20 faces): cap
           10 -> ten chunks of 2.  BZ_NO_K6_STORED=1 (generation-4 tiles): cap Nz / 8 = 2 -> chunks 11 + 10 (rho w: 10 + 10)
  cascade  (40, 16, 11) stretched, periodic: 1 x 2 tiles; k6: cap 5 -> chunks 3 + 3 + 3 + 2 (rho w: five of 2).  Nz = 11 gives the face
           buffers 1, 1, 2, 3, 4, 5, 5, 4, 3, 2, 1, 1 of order 9: every stage of the cascade, each order-9 face once per side.  Orders 7 / 9:
           Nx is no multiple of 64, so the generic kernels take their two passes with or without BZ_NO_GENERIC_MARCH
  march    (64, 8, 11) stretched, periodic: the one grid here on which the single-pass marching kernel k_tendency_m of orders 7 / 9 runs
           (Nx a multiple of 64, Ny of 4, no walls): 1 x 2 workgroups of 64 x 4, march_chunk = 8 -> level chunks 8 + 3
  thin     (32, 6, 7) stretched, periodic: one ragged tile, k6: cap 3 -> chunks 3 + 3 + 1; only faces 3 and 4 reach order 5
  flat     (48, 1, 12) regular z, (Periodic, Flat, Bounded), v != 0: no tiled kernels (tiled_tendencies = false) — the generation-1
           kernels of csrc/bz_tendency.hip, pick_kchunk: one chunk of 12 (rho w: 11)
  ywalls   (32, 16, 11) stretched, (Periodic, Bounded, Bounded): generation-1 kernels with row-wise buffers, one chunk; the cascade in y
           (face buffers 1, 1, 2, 3, 4, 5 ... 5, 4, 3, 2, 1, 1) and z at once.  The smallest such grid a context is created on: between y
           walls the pressure solver needs Nx a power of two >= 16 and Ny a multiple of 8 (csrc/bz_poisson.hip: bzi_poisson_setup), and
           Ny = 8 admits no order-9 face
  xwalls   (48, 12) stretched, (Bounded, Flat, Bounded): generation-1 kernels at order 5 (a Flat y has no tiles), one chunk; the cascade in
           x and z

State: helpers.randomize gives sign-changing rho u, rho v, rho w, theta on a 300 K mean and rough q.  On top of it (plant):
  * in rho u, rho v, rho w, along the field's own direction: eight values antisymmetric about a cell centre (rho u[i0 + 1 + d] =
    -rho u[i0 - d], d = 0 .. 3), so the symmetric interpolation of every order gives exactly zero at that centre with opposite signs
    either side; and one face value exactly zero between neighbours of opposite sign (the scalars' advecting velocity is zero there);
  * in every advected field (u, v, w, theta, q), along every direction: a run of min(8, N) equal cells (beta = tau = 0: eps decides),
    and a step of the field's own amplitude between two plateaus of four cells (tau / beta large);
  * one column whose theta perturbation is 1e-6 of the others (near-linear weights on a large mean: where expanded indicators cancel).
Specific fields and densities are written as they are (density = rho_r x specific) and not rediagnosed, so the planted values stay
exact; halos come from the oracle's fills.  The wall faces (u at i = 0 between x walls, v at j = 0 between y walls, w at k = 0, Nz) are
left alone.  Seeds were chosen on the CPU with the reference alone (the coverage conditions of tests/test_advection_reference.py)."""
import functools

import numpy as np

EXT = ((-10e3, 10e3), (-10e3, 10e3), (0.0, 10e3))
PPB, PFB, PBB, BFB = (("Periodic", "Periodic", "Bounded"), ("Periodic", "Flat", "Bounded"), ("Periodic", "Bounded", "Bounded"),
                      ("Bounded", "Flat", "Bounded"))
# name: (size, stretched, topology)
GRIDS = {"ragged": ((70, 9, 21), True, PPB), "cascade": ((40, 16, 11), True, PPB), "march": ((64, 8, 11), True, PPB),
         "thin": ((32, 6, 7), True, PPB), "flat": ((48, 12), False, PFB), "ywalls": ((32, 16, 11), True, PBB), "xwalls": ((48, 12), True, BFB)}
SEED = 73


def orders(name):
    return (5,) if name == "thin" else (5, 7, 9)


def z_faces(name):
    size, stretched, _ = GRIDS[name]
    a, b = EXT[2]
    return a + (b - a) * np.linspace(0.0, 1.0, size[-1] + 1) ** 1.3 if stretched else EXT[2]


def grid_arguments(name, order):
    """(size, keyword arguments) of oracle.Grid; RectilinearGrid takes the same with its own topology objects."""
    size, _, topo = GRIDS[name]
    H = (order + 1) // 2
    kw = dict(x=EXT[0], z=z_faces(name), topology=topo, halo=(H,) * len(size))
    if len(size) == 3:
        kw["y"] = EXT[1]
    return size, kw


def _line(shape, axis, feature, length, taken, lo):
    """index of a line of at most `length` entries along `axis` that keeps clear of the cells already `taken` in this field (a
    boolean array, updated) and starts at `lo` or above (1 in a Bounded direction: index 0 may be a wall face); the other two coordinates
    depend on the feature and the axis"""
    others = [a for a in range(3) if a != axis]
    n = shape[axis]
    start = max(lo, (n - length) // 2)
    for t in range(max(shape[others[0]], 1) * max(shape[others[1]], 1)):
        idx = [None] * 3
        idx[axis] = slice(start, min(start + length, n))
        for m, a in enumerate(others):
            na = shape[a]
            shift = t if m == 0 else t // max(shape[others[0]] - 1, 1)
            idx[a] = 0 if na == 1 else 1 + ((5 * feature + 3 * axis + 2 * a) * (na - 1) // 17 + shift) % (na - 1)
        idx = tuple(idx)
        if not taken[idx].any():
            taken[idx] = True
            return idx
    raise AssertionError("no free line")


def plant(om):
    g = om.grid
    I = g.interior
    rho = om.ref.density[g.Hz:g.Hz + g.Nz][:, None, None]
    rho_f = np.empty((g.Nz + 1, 1, 1))
    rho_f[:, 0, 0] = 0.5 * (om.ref.density[g.Hz - 1:g.Hz + g.Nz] + om.ref.density[g.Hz:g.Hz + g.Nz + 1])
    shape = (g.Nz, g.Ny, g.Nx)
    planted = {"zero": {}, "antisymmetric": {}, "run": {}, "step": {}}
    lo = (1, int(g.topo[1] == 1), int(g.topo[0] == 1))          # per axis (z, y, x)
    taken = {n: np.zeros(shape, dtype=bool) for n in ("ru", "rv", "rw", "rtheta", "rq")}      # per field: specific and density share the cells
    # advecting momentum: antisymmetric about a centre, and one zero face, along the field's own direction
    for name, axis in (("ru", 2), ("rv", 1), ("rw", 0)):
        n = shape[axis]
        if n == 1:
            continue
        a = I(getattr(om, name), name == "rw")
        p = min(4, (n - lo[axis]) // 2)          # pairs: faces c-p+1 .. c+p straddle centre c
        line = list(_line(shape, axis, 0, 2 * p, taken[name], lo[axis]))
        c = line[axis].start + p - 1
        low, hi = list(line), list(line)
        low[axis], hi[axis] = slice(c - p + 1, c + 1), slice(c + 1, c + p + 1)
        vals = np.abs(a[tuple(low)]) + 0.5
        a[tuple(low)] = vals
        a[tuple(hi)] = -vals[::-1]
        planted["antisymmetric"][name] = (tuple(line), c)
        z = list(_line(shape, axis, 1, 3, taken[name], lo[axis]))
        a[tuple(z)] = np.array([1.0, 0.0, -1.0]) * (np.abs(a[tuple(z)]) + 0.5)
        planted["zero"][name] = tuple(z)
    om.update_state(compute_tendencies=False)
    j, i = (g.Ny // 2, (2 * g.Nx) // 3)          # the column of small theta perturbations: planted last, its cells kept free
    taken["rtheta"][:, j, i] = True
    # advected fields
    for f, (spec, dens, amp) in enumerate((("u", "ru", 5.0), ("v", "rv", 5.0), ("w", "rw", 5.0), ("theta", "rtheta", 2.0), ("q", "rq", 5e-3))):
        zface = spec == "w"
        a, d = I(getattr(om, spec), zface), I(getattr(om, dens), zface)
        r = rho_f[:-1] if zface else rho
        if zface:
            a, d = a[:-1], d[:-1]
        for axis in range(3):
            if shape[axis] == 1:
                continue
            run = _line(shape, axis, 2 + 2 * f, 8, taken[dens], lo[axis])
            a[run] = a[run].flat[0]
            step = list(_line(shape, axis, 3 + 2 * f, 8, taken[dens], lo[axis]))
            n = step[axis].stop - step[axis].start
            base = a[tuple(step)].flat[0]
            a[tuple(step)] = base + amp * (np.arange(n) >= n // 2)
            for sl in (run, tuple(step)):
                d[sl] = np.broadcast_to(r, a.shape)[sl] * a[sl]
            planted["run"][(spec, axis)] = run
            planted["step"][(spec, axis)] = tuple(step)
    th = I(om.theta)
    th[:, j, i] = 300.0 + 1e-6 * (th[:, j, i] - 300.0)
    I(om.rtheta)[:, j, i] = rho[:, 0, 0] * th[:, j, i]
    planted["column"] = (j, i)
    # halos, each field by its own fill
    om.fill_momentum_halos()
    for f in (om.rtheta, om.rq, om.theta, om.q):
        om._halo_center(f)
    for f in (om.u, om.v, om.w):
        om._halo_velocity(f, yface=f is om.v, xface=f is om.u)
    return planted


@functools.lru_cache(maxsize=None)
def oracle_case(name, order, scalar_order=None):
    """the oracle model holding the planted state (computed once, shared, never changed) and the record of what was planted where"""
    from helpers import randomize
    from oracle import oracle
    oracle.build()
    size, kw = grid_arguments(name, max(order, scalar_order or order))
    okw = dict(scalar_advection=f"WENO{scalar_order}") if scalar_order else {}
    om = oracle.OracleModel(oracle.Grid(size, **kw), potential_temperature=300.0, advection=f"WENO{order}", **okw)
    randomize(om, seed=SEED)
    om.planted = plant(om)
    return om


def geometry(om):
    from advection_reference import Geometry
    g = om.grid
    names = {0: "Periodic", 1: "Bounded", 2: "Flat"}
    z = (float(g.zf[0]), float(g.zf[-1])) if g.regular_z else g.zf
    return Geometry(z, g.dx, g.dy, (g.Hx, g.Hy, g.Hz), tuple(names[t] for t in g.topo), Nz=g.Nz)
