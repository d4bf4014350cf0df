"""CPU pins of tests/compressible_walls_reference.py — the restatement of the compressible model on walls in y that the GPU tests of
tests/test_compressible_walls.py compare against.

A y-invariant state with v = 0 and no Coriolis force never feels the walls: every y reconstruction sees constant data (all WENO orders
return the constant), every y flux is an exact zero, the no-flux halo row equals the periodic image.  The walled restatement must then
give bitwise the fields of the unmodified oracle on (Periodic, Periodic, Bounded).  With a y-varying state the closed channel conserves
dry mass and vapour mass to rounding and keeps exact zeros on the wall faces."""
import numpy as np
import pytest

from compressible_walls_reference import WalledCompressibleOracleModel, column_mass

EXTENT = dict(x=(-4e3, 4e3), y=(-3e3, 3e3), z=(0.0, 8e3))
WALLS = ("Periodic", "Bounded", "Bounded")
PERIODIC = ("Periodic", "Periodic", "Bounded")
FIELDS = ("rho_d", "rho", "rtheta", "rq", "ru", "rv", "rw", "u", "v", "w", "theta", "q", "T", "p", "au", "av", "aw")


def bubble_xz(x, y, z):
    r = np.sqrt(x ** 2 + (z - 3000.0) ** 2)
    return 300.0 + 2.0 * np.maximum(0.0, 1.0 - r / 2000.0) + 0 * y


def vapour_xz(x, y, z):
    return 5e-3 * np.exp(-z / 2e3) * (1 + 0.2 * np.sin(2 * np.pi * x / 8e3)) + 0 * y


def set_y_invariant(om):
    g = om.grid
    rho = om.ref.density[g.Hz:g.Hz + g.Nz][:, None, None]
    om.set(rho=rho, theta=bubble_xz, u=lambda x, y, z: 3.0 + 0 * x + 0 * y + 0 * z, v=0.0, w=0.0, qv=vapour_xz)


@pytest.mark.parametrize("size", [(24, 16, 24), (24, 6, 24)], ids=["Ny16", "Ny6_reduced_buffers_everywhere"])
def test_y_invariant_state_is_bitwise_the_periodic_oracle(oracle, oc, size):
    out = []
    for cls, topo in ((oc.CompressibleOracleModel, PERIODIC), (WalledCompressibleOracleModel, WALLS)):
        og = oracle.Grid(size, topology=topo, **EXTENT)
        om = cls(og, time_discretization=oc.SplitExplicit(substeps=6), reference_potential_temperature=300.0)
        set_y_invariant(om)
        for _ in range(3):
            om.time_step(2.0)
        out.append({n: og.interior(getattr(om, n), n in ("rw", "w", "aw")).copy() for n in FIELDS})
    assert np.abs(out[0]["rw"]).max() > 1e-3          # the bubble moved
    for n in FIELDS:
        assert np.array_equal(out[0][n], out[1][n]), n


def y_varying_model(oracle, oc, size=(24, 16, 24), f=1e-4):
    og = oracle.Grid(size, topology=WALLS, **EXTENT)
    om = WalledCompressibleOracleModel(og, time_discretization=oc.SplitExplicit(substeps=6), reference_potential_temperature=300.0, coriolis_f=f)
    Lx, Ly = og.Nx * og.dx, og.Ny * og.dy

    def theta(x, y, z):
        r = np.sqrt(x ** 2 + (y - 500.0) ** 2 + (z - 3000.0) ** 2)
        return 300.0 + 2.0 * np.maximum(0.0, 1.0 - r / 2000.0)

    def qv(x, y, z):
        return 5e-3 * np.exp(-z / 2e3) * (1 + 0.2 * np.sin(2 * np.pi * x / Lx) * np.cos(np.pi * (y + Ly / 2) / Ly))

    def v(x, y, z):          # vanishes at the walls y = -Ly/2, Ly/2
        return 2.0 * np.cos(np.pi * y / Ly) * np.sin(2 * np.pi * x / Lx) + 0 * z

    rho = om.ref.density[og.Hz:og.Hz + og.Nz][:, None, None]
    om.set(rho=rho, theta=theta, u=lambda x, y, z: 3.0 + 0 * x + 0 * y + 0 * z, v=v, w=0.0, qv=qv)
    return om


def test_closed_channel_conserves_mass_and_keeps_wall_faces_at_zero(oracle, oc):
    om = y_varying_model(oracle, oc)
    g = om.grid
    m0, q0 = column_mass(om), column_mass(om, "rq")
    for _ in range(3):
        om.time_step(2.0)
    for n in FIELDS:
        assert np.isfinite(getattr(om, n)).all(), n
    assert np.abs(g.interior(om.rv)).max() > 0.1 and np.abs(g.interior(om.v)[:, 1:, :]).max() > 0.1
    assert abs(column_mass(om) - m0) <= 1e-12 * abs(m0)
    assert abs(column_mass(om, "rq") - q0) <= 1e-12 * abs(q0)
    Hy, Ny, Hz, Nz = g.Hy, g.Ny, g.Hz, g.Nz
    for n in ("rv", "v", "av"):          # wall faces 0 and Ny (first upper halo row): exact zeros, whole parent rows
        f = getattr(om, n)[Hz:Hz + Nz]
        assert not f[:, Hy, :].any() and not f[:, Hy + Ny, :].any(), n
    for n in ("rho_d", "rho", "rtheta", "rq", "ru", "rw", "u", "w", "theta", "q", "T", "p"):      # no-flux rows of the centre-in-y fields
        f = getattr(om, n)[Hz:Hz + Nz]
        assert np.array_equal(f[:, Hy - 1, :], f[:, Hy, :]) and np.array_equal(f[:, Hy + Ny, :], f[:, Hy + Ny - 1, :]), n


def test_validation_case_proportions_run_and_conserve_mass(oracle, oc):
    """The keyword list of validation/cartesian_baroclinic_wave at 16 x 12 x 10, halo 5: 100 km cells, 3 km levels, dt = 600 s, default
    SplitExplicit (adaptive substeps: 2, 3, 5), theta_ref(z) = 250 exp(g z / (cp 250)), f = 1.03e-4 — with a smooth jet of this test's own."""
    om = channel_model(oracle, oc)
    m0 = column_mass(om)
    for _ in range(2):
        om.time_step(600.0)
    assert om.last_substeps == [2, 3, 5]
    for n in FIELDS:
        assert np.isfinite(getattr(om, n)).all(), n
    assert abs(column_mass(om) - m0) <= 1e-12 * abs(m0)


CHANNEL = dict(size=(16, 12, 10), halo=(5, 5, 5), x=(0.0, 16e5), y=(0.0, 12e5), z=(0.0, 30e3))


def channel_theta_ref(z):
    return 250.0 * np.exp(9.80665 * z / (1005.0 * 250.0))


def channel_initial(og):
    Lx, Ly = og.Nx * og.dx, og.Ny * og.dy

    def jet(x, y, z):          # a westerly jet in mid-channel, strongest near 10 km
        return 20.0 * np.sin(np.pi * y / Ly) ** 2 * np.exp(-((z - 10e3) / 8e3) ** 2) + 0 * x

    def theta(x, y, z):        # the reference profile, colder towards the north wall, with a localised warm anomaly
        bump = np.exp(-((x - 0.4 * Lx) / 3e5) ** 2 - ((y - 0.5 * Ly) / 3e5) ** 2)
        return channel_theta_ref(z) * (1 - 0.02 * (y / Ly - 0.5)) + 1.0 * bump + 0 * z

    return jet, theta


def channel_model(oracle, oc):
    og = oracle.Grid(CHANNEL["size"], halo=CHANNEL["halo"], topology=WALLS, x=CHANNEL["x"], y=CHANNEL["y"], z=CHANNEL["z"])
    om = WalledCompressibleOracleModel(og, time_discretization=oc.SplitExplicit(), surface_pressure=1e5,
                                       reference_potential_temperature=channel_theta_ref, coriolis_f=1.03e-4)
    jet, theta = channel_initial(og)
    rho = om.ref.density[og.Hz:og.Hz + og.Nz][:, None, None]
    om.set(rho=rho, theta=theta, u=jet)
    return om
