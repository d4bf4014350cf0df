"""Grids and states shared by tests/test_bounded_weno_reference.py (CPU: oracle against the long-double reference) and
tests/test_bounded_weno_clients.py (device against oracle): the bounds-preserving WENO operator where its limiter works hard.

Grids (from the launch arithmetic of csrc/bz_bounded.hip: bzi_bounded_tendencies: 64 x 4 tiles, z chunks of at least 8 levels):
  ragged   (70, 9, 21), z faces Lz linspace(0, 1, Nz + 1)^1.3: a ragged x tile (64 + 6), a tail row of the 4-row tile, two z chunks
           11 + 10 with the seam at k = 11
  fit      (64, 4, 24), uniform z: exact tiles, three chunks of 8, two seams
  thin     (32, 6, 7), stretched z: Nz < 8, one chunk; only faces 3 and 4 are order 5, every reduced stencil runs
  flat     (48, 1, 12), (Periodic, Flat, Bounded): the flat_y branch, with v != 0 in the state

State: helpers.randomize gives sign-changing u, v, w; the limited scalar is then a "two-plateau rough" field, hi - 0.1 (hi - lo) r^2 inside
the centred box that covers the middle half of every direction and lo + 0.1 (hi - lo) r^2 outside, r uniform in (0, 1) per cell, plus
  * one run of min(8, N) equal cells along each direction (M - c = 0: the 1e-20 of the limiter's denominators decides),
  * five cells exactly at lo and five at hi (theta = 0),
  * one cell 1e-6 (hi - lo) below lo and one as far above hi (what a stepped state produces).
Halos are refilled through the oracle.  Seeds were chosen on the CPU with the reference alone (the activity condition of
tests/test_bounded_weno_reference.py)."""
import numpy as np

EXT = ((-10e3, 10e3), (-10e3, 10e3), (0.0, 10e3))
GRIDS = {"ragged": ((70, 9, 21), True), "fit": ((64, 4, 24), False), "thin": ((32, 6, 7), True), "flat": ((48, 1, 12), False)}
BOUNDS = ((0.0, 1.0), (0.0, 0.01))
SEED = 41


def z_faces(name):
    size, stretched = GRIDS[name]
    a, b = EXT[2]
    return a + (b - a) * np.linspace(0.0, 1.0, size[2] + 1) ** 1.3 if stretched else EXT[2]


def grid_arguments(name):
    """(size, keyword arguments) of oracle.Grid; RectilinearGrid takes the same with its own topology objects."""
    size, _ = GRIDS[name]
    if name == "flat":
        return (size[0], size[2]), dict(x=EXT[0], z=z_faces(name), topology=("Periodic", "Flat", "Bounded"))
    return size, dict(x=EXT[0], y=EXT[1], z=z_faces(name))


def oracle_model(oracle, name, **kw):
    size, gkw = grid_arguments(name)
    return oracle.OracleModel(oracle.Grid(size, **gkw), potential_temperature=300.0, **kw)


def two_plateau(shape, lo, hi, seed):
    """The rough two-plateau field with its planted cells, (Nz, Ny, Nx)."""
    rng = np.random.default_rng(seed)
    r = rng.uniform(size=shape)
    r = np.where(r > 0.0, r, 0.5)
    box = [(np.arange(n) >= n // 4) & (np.arange(n) < n - n // 4) for n in shape]
    inside = box[0][:, None, None] & box[1][None, :, None] & box[2][None, None, :]
    span = hi - lo
    q = np.where(inside, hi - 0.1 * span * r ** 2, lo + 0.1 * span * r ** 2)
    Nz, Ny, Nx = shape
    # a run of equal cells along x, y and z, away from each other (a direction shorter than 8 cells is equal from end to end)
    k, j, i = Nz // 3, Ny // 3, Nx // 8
    q[k, j, i:i + min(8, Nx)] = q[k, j, i]
    k, j, i = (2 * Nz) // 3, max(0, (Ny - 8) // 2), Nx // 2
    q[k, j:j + min(8, Ny), i] = q[k, j, i]
    k, j, i = max(0, (Nz - 8) // 2), (2 * Ny) // 3, (3 * Nx) // 4
    q[k:k + min(8, Nz), j, i] = q[k, j, i]
    cells = rng.choice(q.size, size=12, replace=False)
    flat = q.reshape(-1)
    flat[cells[:5]] = lo
    flat[cells[5:10]] = hi
    flat[cells[10]] = lo - 1e-6 * span
    flat[cells[11]] = hi + 1e-6 * span
    return q


def plant(om, specific, density, lo, hi, seed):
    """Overwrite the specific field `specific` of the oracle model (and its density field) with the two-plateau state; both get their halos
    from the oracle.  The specific values are stored as they are, not rediagnosed from the density: cells at a bound stay exactly there."""
    g = om.grid
    q = two_plateau((g.Nz, g.Ny, g.Nx), lo, hi, seed)
    rho = om.ref.density[g.Hz:g.Hz + g.Nz][:, None, None]
    g.interior(getattr(om, specific))[...] = q
    g.interior(getattr(om, density))[...] = rho * q
    for f in (specific, density):
        om._halo_center(getattr(om, f))
    if om.microphysics == "Kessler":      # the copies update_state keeps for the buoyancy: vapour and q^cl + q^r
        om.qv[...] = om.q
        om.ql[...] = om.qcl + om.qr
