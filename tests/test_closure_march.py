"""The anelastic instantiations of the z-marching closure kernels (csrc/bz_closure.hip: k_smagorinsky_march<8, ExnerColumn> and
k_closure_march<8, RhoColumn>, the kernels of every BOMEX-sized run) where a wrong level, lane or tile would show: a stretched z (every
metric, face density, Exner factor and filter width differs from level to level, so an index that is off by one reads another number),
more than one tile in x and in y (frame cells that belong to another tile, an interior tile), a launch of a multiple of 8 workgroups (the
XCD block order), ragged and minimal chunks of levels, and a halo of 5.

    shape            z          halo  tiles  chunks        workgroups
    (128, 16, 32)    stretched  3     2 x 2  16 + 16       8: the XCD remap is taken; tile seams in x and y
    (192, 24, 35)    stretched  3     3 x 3  18 + 17       18: an interior tile in x and in y
    (64, 8, 50)      stretched  3     1      17 + 17 + 16  3: a ragged last chunk
    (128, 8, 4)      stretched  3     2 x 1  4             2: the prologue's level kbeg - 1 and the look-ahead to Nz + 1 at the walls
    (64, 16, 12)     uniform    5     1 x 2  12            2: the order-9 BOMEX layout; one chunk shorter than 16

(chunks: kc = ceil(Nz / nch), nch = min(ceil(2048 / tiles), Nz / 16), at least 1; both kernels launch tiles x ceil(Nz / kc) workgroups.)

The cell-per-thread kernels (BZ_NO_CLOSURE_MARCH=1) evaluate the same expressions in the same order, so nu_e and the five tendencies of the
two runs are compared bit for bit, and both with the oracle at the bounds of tests/test_closure.py.  Which kernels ran is the verdict of the
library's one dispatch predicate (model.closure_marches()): the profile groups carry the same names on both paths.

Measured on the MI355X (each test prints its figures; the worst of the dry and the moist case): no cell of nu_e or of a tendency differs
between the two kernel pairs at any shape.  Against the oracle, shipped library: nu_e 2.6e-12 / 3.9e-12 / 1.5e-12 / 1.8e-13 / 2.0e-12 of its
maximum in the order of the table, rho theta 2.6e-9 / 2.0e-9 / 1.5e-9 / 1.6e-9 / 2.0e-9 (FMA contraction in the WENO fluxes; bound 5e-9), the
other four tendencies at most 9.3e-12; refdiv library: every tendency at most 3.2e-14, the closure part at most 1.8e-12 of its own maximum
(bound 1e-10).  Edge shapes: nu_e at most 2.0e-13, rho theta at most 2.6e-9.  Three steps: at most 9.0e-12 (refdiv 1.2e-11; bound 2e-9).

Stretched faces: round(3000 (0.35 s + 0.65 s^2)), s = linspace(0, 1, Nz + 1): whole numbers (tests/test_scalar_diffusivity.py: _z_faces);
the largest spacing is about 4.4 times the smallest at Nz = 32."""
import numpy as np
import pytest

from helpers import PROG, push_state, relerr
from test_closure import EXTENT, _turbulent_ic

pytestmark = pytest.mark.gpu

NAMES = ("ru", "rv", "rw", "rtheta", "rq")
# (shape, stretched, halo)
MARCH_SHAPES = [((128, 16, 32), True, 3), ((192, 24, 35), True, 3), ((64, 8, 50), True, 3), ((128, 8, 4), True, 3), ((64, 16, 12), False, 5)]
# Nz < 4; Ny no multiple of 8; Nx no multiple of 64: the cell-per-thread kernels.  (shape, smallest share of the closure in a tendency)
EDGE_SHAPES = [((64, 8, 3), 3e-3), ((64, 12, 8), 5e-3), ((96, 8, 8), 5e-3)]
SEED = 11


def _z(Nz, stretched):
    if not stretched:
        return EXTENT[2]
    s = np.linspace(0.0, 1.0, Nz + 1)
    return np.round(3000.0 * (0.35 * s + 0.65 * s ** 2))


def _oracle_model(oracle, shape, stretched, halo, moist, closure=True, forced=False):
    from oracle.closure import SmagorinskyLilly
    from test_forcings import _oracle_forcings
    og = oracle.Grid(shape, x=EXTENT[0], y=EXTENT[1], z=_z(shape[2], stretched), halo=(halo,) * 3)
    return oracle.OracleModel(og, surface_pressure=101500.0, potential_temperature=299.1, microphysics="SaturationAdjustment" if moist else None,
                              closure=SmagorinskyLilly() if closure else None, forcings=_oracle_forcings(oracle, og) if forced else None)


def _device_model(bz, shape, stretched, halo, moist, forced=False):
    from test_forcings import _hip_forcing_kwargs
    grid = bz.RectilinearGrid(shape, x=EXTENT[0], y=EXTENT[1], z=_z(shape[2], stretched), halo=(halo,) * 3)
    ref = bz.ReferenceState(grid, surface_pressure=101500.0, potential_temperature=299.1)
    return bz.AtmosphereModel(grid, dynamics=bz.AnelasticDynamics(ref), advection=bz.WENO(order=5), closure=bz.SmagorinskyLilly(),
                              microphysics=bz.SaturationAdjustment(equilibrium=bz.WarmPhaseEquilibrium()) if moist else None,
                              **(_hip_forcing_kwargs(bz) if forced else {}))


_REFERENCE = {}


def _reference(oracle, shape, stretched, halo, moist):
    """The oracle on _turbulent_ic(seed 11) after update_state!, once per case and never written again: (model, {name: tendency},
    {name: tendency of a model without closure on the same fields})."""
    key = (shape, stretched, halo, moist)
    if key not in _REFERENCE:
        om = _oracle_model(oracle, shape, stretched, halo, moist)
        om.set(**_turbulent_ic(om, SEED))
        om.update_state()
        om0 = _oracle_model(oracle, shape, stretched, halo, moist, closure=False)
        for n in NAMES:
            getattr(om0, n)[...] = getattr(om, n)
        om0.update_state()
        g = om.grid
        want = {n: g.interior(om.G[n], zface=(n == "rw")).copy() for n in NAMES}
        base = {n: g.interior(om0.G[n], zface=(n == "rw")).copy() for n in NAMES}
        _REFERENCE[key] = (om, want, base)
    return _REFERENCE[key]


def _guards(om, want, base, share):
    """The comparison is not empty, by the oracle alone: nu_e has capped (zero) and sheared cells, and in every field the closure is at
    least `share` of the tendency's maximum — so the 5e-9 bound on a tendency is at most 5e-9 / share = 1e-6 of its closure part."""
    assert (om.nu_e == 0).any() and om.nu_e.max() > 0
    shares = {n: np.abs(want[n] - base[n]).max() / np.abs(want[n]).max() for n in NAMES}
    assert min(shares.values()) >= share, shares
    return shares


def _device_run(bz, om, shape, stretched, halo, moist, monkeypatch, no_march):
    if no_march:
        monkeypatch.setenv("BZ_NO_CLOSURE_MARCH", "1")
    else:
        monkeypatch.delenv("BZ_NO_CLOSURE_MARCH", raising=False)
    try:
        hm = _device_model(bz, shape, stretched, halo, moist)
    finally:
        monkeypatch.delenv("BZ_NO_CLOSURE_MARCH", raising=False)
    push_state(om, hm, names=NAMES)
    bz.update_state_(hm, compute_tendencies=True)
    hm.synchronize()
    out = {n: hm.G[k].interior_cpu().copy() for n, k in PROG.items()}
    out["nu"] = hm.closure_fields["νₑ"].interior_cpu().copy()
    return hm, out


def _assert_oracle_bounds(bz, label, om, want, base, got):
    """The bounds of tests/test_closure.py::test_eddy_viscosity_and_closure_tendencies_match_oracle; every figure is printed first."""
    strict = "refdiv" in bz.LIB_PATH
    nu_err = np.abs(got["nu"] - om.nu_e).max() / om.nu_e.max()
    errs = {n: relerr(got[n], want[n]) for n in NAMES}
    parts = {n: np.abs((got[n] - base[n]) - (want[n] - base[n])).max() / np.abs(want[n] - base[n]).max() for n in NAMES}
    print(f"MARCH {label}: nu={nu_err:.2e} " + " ".join(f"{n}={errs[n]:.1e}" for n in NAMES) + " | part " + " ".join(f"{n}={parts[n]:.1e}" for n in NAMES))
    assert nu_err < 1e-11
    for n in NAMES:
        assert errs[n] < (1e-12 if strict else 5e-9), (n, errs[n])
        if strict:
            assert parts[n] < 1e-10, (n, parts[n])


@pytest.mark.parametrize("moist", [False, True])
@pytest.mark.parametrize("shape,stretched,halo", MARCH_SHAPES)
def test_march_carries_the_bits_of_the_cell_per_thread_kernels(oracle, bz, shape, stretched, halo, moist, monkeypatch):
    """update_state!(compute_tendencies = true) on the pushed oracle state, as shipped (the march, by the library's own verdict) and with
    BZ_NO_CLOSURE_MARCH=1 (cell per thread): nu_e and the five tendencies bit for bit, and against the oracle
    |nu - nu_oracle|max < 1e-11 nu_oracle.max(), every tendency within 5e-9 of its maximum (1e-12, and the closure part alone within 1e-10 of
    its own maximum, where the library is the refdiv build)."""
    om, want, base = _reference(oracle, shape, stretched, halo, moist)
    shares = _guards(om, want, base, 5e-3)
    a, ga = _device_run(bz, om, shape, stretched, halo, moist, monkeypatch, no_march=False)
    assert a.closure_marches(), "the dispatch predicate refuses a grid of whole tiles"
    b, gb = _device_run(bz, om, shape, stretched, halo, moist, monkeypatch, no_march=True)
    assert not b.closure_marches()
    different = {n: int(np.count_nonzero(ga[n] != gb[n])) for n in ga}
    print(f"MARCH {shape} moist={moist}: closure share " + " ".join(f"{n}={s:.1e}" for n, s in shares.items()),
          f"| nu_e zero in {np.mean(om.nu_e == 0):.0%} | cells that differ between the two kernels {different}")
    _assert_oracle_bounds(bz, f"{shape} moist={moist} march", om, want, base, ga)
    _assert_oracle_bounds(bz, f"{shape} moist={moist} cell-per-thread", om, want, base, gb)
    for n in ga:
        assert np.array_equal(ga[n], gb[n]), (n, different[n], np.argwhere(ga[n] != gb[n])[:4].tolist())


@pytest.mark.parametrize("shape,share", EDGE_SHAPES)
def test_dispatch_edges_keep_the_cell_per_thread_kernels(oracle, bz, shape, share, monkeypatch):
    """Three levels, a ragged tile row and a ragged tile column: the predicate says cell per thread, and the result holds the oracle's
    bounds.  (64, 8, 3): the closure is 4.3e-3 of the rho w tendency (a three-level column, most cells capped), so the guard is 3e-3 there."""
    om, want, base = _reference(oracle, shape, True, 3, True)
    _guards(om, want, base, share)
    hm, got = _device_run(bz, om, shape, True, 3, True, monkeypatch, no_march=False)
    assert not hm.closure_marches()
    _assert_oracle_bounds(bz, f"{shape} edge", om, want, base, got)


@pytest.mark.parametrize("whole_step", [True, False])
def test_three_steps_through_both_seams_on_stretched_whole_tiles(oracle, bz, whole_step):
    """(128, 16, 32) stretched, saturation adjustment, the forcing stack: three steps through the whole-step seam (the divergences applied in
    place to the densities with scale = alpha dt) and through the per-operator sequence, with the march on a stretched z in both.  2e-9 of
    the field scale, the momenta by their common maximum (tests/test_closure.py::test_bomex_stack_time_steps_match_oracle)."""
    shape, dt = (128, 16, 32), 3.0
    om = _oracle_model(oracle, shape, True, 3, True, forced=True)
    hm = _device_model(bz, shape, True, 3, True, forced=True)
    assert hm.closure_marches()
    ic = _turbulent_ic(om, 5)
    om.set(**ic)
    hm.set(θ=ic["theta"], qᵗ=ic["qt"], u=ic["u"], v=ic["v"])
    for _ in range(3):
        om.time_step(dt)
        bz.time_step_(hm, dt, whole_step=whole_step)
    hm.synchronize()
    g = om.grid
    assert om.nu_e.max() > 0.01 and np.isfinite(g.interior(om.rtheta)).all()
    mom = max(np.abs(g.interior(getattr(om, n), zface=(n == "rw"))).max() for n in ("ru", "rv", "rw"))
    errs = {}
    for n, k in PROG.items():
        want = g.interior(getattr(om, n), zface=(n == "rw"))
        got = hm.prognostic_fields()[k].interior_cpu()
        errs[n] = np.abs(got - want).max() / (mom if n in ("ru", "rv", "rw") else np.abs(want).max())
    print(f"MARCH STEPS whole_step={whole_step}: " + " ".join(f"{n}={e:.1e}" for n, e in errs.items()))
    for n, e in errs.items():
        assert e < 2e-9, (n, e)
