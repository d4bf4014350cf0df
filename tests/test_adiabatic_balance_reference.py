"""Adiabatic balance without a GPU: the reference composition on the oracle models (tests/adiabatic_balance_reference.py) meets the bounds
of the reference's own tests (test/balance_adiabatically.jl:87-163), and the host side of balance_adiabatically! / AdiabaticBalancer /
set!(model; balancer) validates, refuses and exports what it should before a device is needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import adiabatic_balance_reference as abr


# ---- the reference composition on the oracle --------------------------------------------------------------------------------------------
def test_compressible_rest_state_is_a_fixed_point(oracle, oc):
    """test/balance_adiabatically.jl:87-108 on the oracle: dt = 1, cycles = 1 from the discrete rest state."""
    om = abr.compressible_rest_oracle(oracle, oc)
    g = om.grid
    rho0, rth0 = g.interior(om.rho_d).copy(), g.interior(om.rtheta).copy()
    assert len(abr.initial_names(om)) == 5
    abr.balance(om, 1.0, cycles=1)
    e_rho = abr.max_abs(g.interior(om.rho_d) - rho0) / abr.max_abs(rho0)
    e_rth = abr.max_abs(g.interior(om.rtheta) - rth0) / abr.max_abs(rth0)
    w = abr.max_abs(g.interior(om.rw, True))
    print(f"rest state, oracle composition: rho_d {e_rho:.2e} rho theta {e_rth:.2e} max|rho w| {w:.2e}")
    assert e_rho <= 1e-9 and e_rth <= 1e-9
    assert w <= 1e-8
    assert (om.iteration, om.clock_time) == (0, 0.0)


def test_seeded_vertical_momentum_shrinks(oracle, oc):
    """test/balance_adiabatically.jl:110-126 on the oracle: w = 0.01 sin(2 pi z / 2 km), dt = 0.1."""
    om = abr.compressible_rest_oracle(oracle, oc)
    abr.seed_w(om)
    before = abr.max_abs(om.grid.interior(om.rw, True))
    abr.balance(om, 0.1, cycles=1)
    after = abr.max_abs(om.grid.interior(om.rw, True))
    print(f"seeded rho w, oracle composition: before {before:.6f} after {after:.6f}")
    assert before > 0
    assert after < before


def test_anelastic_rest_state_is_preserved(oracle):
    """test/balance_adiabatically.jl:128-163 on the oracle (the backward anelastic step included)."""
    om = abr.anelastic_rest_oracle(oracle)
    g = om.grid
    rth0 = g.interior(om.rtheta).copy()
    assert len(abr.initial_names(om)) == 4
    abr.balance(om, 1.0, cycles=1)
    assert np.isfinite(g.interior(om.ru)).all()
    assert abr.max_abs(g.interior(om.rtheta) - rth0) <= 1e-6 * abr.max_abs(rth0)
    assert abr.max_abs(g.interior(om.rw, True)) <= 1e-6
    assert (om.iteration, om.clock_time) == (0, 0.0)


@pytest.mark.parametrize("td", [dict(substeps=6), dict()])
def test_composition_stays_finite_on_a_warm_bubble(oracle, oc, td):
    """forward and backward split-explicit steps with a fixed and with the adaptive substep count (|dt| sizes it)"""
    og = oracle.Grid((12, 8, 10), x=(-4e3, 4e3), y=(-3e3, 3e3), z=(0.0, 8e3))
    om = oc.CompressibleOracleModel(og, time_discretization=oc.SplitExplicit(**td), reference_potential_temperature=300.0)
    rho = om.ref.density[og.Hz:og.Hz + og.Nz][:, None, None]
    om.set(rho=rho, theta=lambda x, y, z: 300.0 + 2.0 * np.maximum(0.0, 1.0 - np.sqrt(x ** 2 + y ** 2 + (z - 3000.0) ** 2) / 2000.0),
           u=3.0, v=0.0, w=0.0, qv=lambda x, y, z: 5e-3 * np.exp(-z / 2e3) + 0 * x + 0 * y)
    abr.balance(om, 2.0, cycles=2, weight=0.5)
    for n in om.PROGNOSTIC + ("T", "p"):
        assert np.isfinite(getattr(om, n)).all(), n
    assert abr.max_abs(og.interior(om.rw, True)) > 0


def test_nudge_is_the_weighted_mean():
    class M:
        PROGNOSTIC = ("ru", "rw", "rtheta")
    m = M()
    m.ru, m.rw, m.rtheta = np.full((3, 4), 1.0), np.full((4, 4), 7.0), np.full((3, 4), 2.0)
    snap = abr.snapshot(m)
    m.rtheta[...] = 5.0
    abr.nudge(m, snap, 2)
    assert np.array_equal(m.rtheta, np.full((3, 4), 3.0)) and np.array_equal(m.rw, np.full((4, 4), 7.0))


# ---- the host side ------------------------------------------------------------------------------------------------------------------------
def test_exports_and_bindings(bz):
    from breeze_jl_amd import _lib
    for name in ("balance_adiabatically_", "AdiabaticBalancer", "DefaultTimeStepping", "snapshot_initial_fields", "nudge_initial_fields_",
                 "initial_fields", "resolve_balance_Δt"):
        assert hasattr(bz, name), name
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "breeze_hip.h"), encoding="utf-8") as fh:
        code = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    for name in ("bz_nudge_fields", "bz_balance_adiabatically_compressible", "bz_balance_adiabatically_anelastic"):
        assert name in _lib.SYMBOLS and re.search(r"\b%s\s*\(" % name, code), name
    with open(os.path.join(root, "breeze.jl_amd", "csrc", "Makefile"), encoding="utf-8") as fh:
        assert "bz_adiabatic_balance.hip" in fh.read()
    res, args = _lib.SYMBOLS["bz_balance_adiabatically_compressible"]
    assert res is C.c_int and args[-4:] == [C.c_double, C.c_int32, C.c_double, C.c_int32]


def test_balancer_arguments(bz):
    b = bz.AdiabaticBalancer()
    assert (b.Δt, b.cycles, b.weight, b.with_moisture) == (None, 1, 2.0, True) and isinstance(b.time_stepping, bz.DefaultTimeStepping)
    b = bz.AdiabaticBalancer(Δt=0.5, cycles=3, weight=0.5, with_moisture=False, time_stepping=None)
    assert (b.Δt, b.cycles, b.weight, b.with_moisture, b.time_stepping) == (0.5, 3, 0.5, False, None)
    assert bz.AdiabaticBalancer(Δt=-1.0).Δt == -1.0          # a backward-first excursion is a valid request
    for bad in (dict(cycles=0), dict(cycles=-1), dict(cycles=1.5), dict(cycles=True), dict(Δt=0.0), dict(Δt=float("nan")),
                dict(Δt=float("inf")), dict(weight=-1), dict(weight=-2.5), dict(weight=float("nan")), dict(weight=float("inf"))):
        with pytest.raises(ValueError):
            bz.AdiabaticBalancer(**bad)
    with pytest.raises(TypeError):
        bz.AdiabaticBalancer(with_moisture=1)


def _periodic_grid(bz, topology=("Periodic", "Periodic", "Bounded")):
    if topology[1] == "Flat":
        return bz.RectilinearGrid((8, 4), x=(0, 1), z=(0, 1), topology=topology)
    return bz.RectilinearGrid((8, 8, 4), x=(0, 1), y=(0, 1), z=(0, 1), topology=topology)


def _fake(cls, grid, **attrs):
    m = object.__new__(cls)          # no context is made: the refusals come first
    m.grid = grid
    for k, v in attrs.items():
        setattr(m, k, v)
    return m


def test_false_is_a_no_op(bz):
    m = _fake(bz.CompressibleAtmosphereModel, _periodic_grid(bz))
    assert bz.balance_adiabatically_(m, False) is m
    other = object()
    assert bz.balance_adiabatically_(other, False) is other          # nothing is looked at


def test_default_time_stepping_is_refused_on_compressible_dynamics(bz):
    m = _fake(bz.CompressibleAtmosphereModel, _periodic_grid(bz))
    for call in (lambda: bz.balance_adiabatically_(m, bz.AdiabaticBalancer()), lambda: bz.balance_adiabatically_(m, True),
                 lambda: bz.compressible.set_(m, balancer=True), lambda: bz.compressible.set_(m, balancer=bz.AdiabaticBalancer(Δt=1.0))):
        with pytest.raises(NotImplementedError, match="ExplicitTimeStepping") as e:
            call()
        assert "time_stepping=None" in str(e.value)
    with pytest.raises(NotImplementedError, match="time_stepping"):
        bz.balance_adiabatically_(m, bz.AdiabaticBalancer(time_stepping=object()))
    with pytest.raises(TypeError):
        bz.balance_adiabatically_(m, "yes")
    m.__dict__.clear()


def test_models_out_of_scope_are_refused_by_name(bz):
    from breeze_jl_amd.compressible import SlabCompressibleModel
    from breeze_jl_amd.distributed import LibrarySlabAtmosphereModel, SlabAtmosphereModel
    grid = _periodic_grid(bz)
    good = bz.AdiabaticBalancer(Δt=1.0, time_stepping=None)

    def every_entry(m, match):
        setter = bz.compressible.set_ if isinstance(m, bz.CompressibleAtmosphereModel) else bz.set_
        for call in (lambda: bz.balance_adiabatically_(m, Δt=1.0), lambda: bz.balance_adiabatically_(m, good),
                     lambda: bz.balance_adiabatically_(m, True), lambda: setter(m, balancer=good)):
            with pytest.raises(NotImplementedError, match=match):
                call()
        m.__dict__.clear()

    for cls in (SlabCompressibleModel, LibrarySlabAtmosphereModel, SlabAtmosphereModel):
        every_entry(_fake(cls, grid), "y-slab")
    every_entry(_fake(bz.AtmosphereModel, grid, _kinematic=True), "kinematic")
    for topo in (("Periodic", "Bounded", "Bounded"), ("Bounded", "Flat", "Bounded")):
        every_entry(_fake(bz.AtmosphereModel, _periodic_grid(bz, topo), _kinematic=False), "walls")
    for topo in (("Periodic", "Bounded", "Bounded"), ("Bounded", "Periodic", "Bounded")):
        every_entry(_fake(bz.CompressibleAtmosphereModel, _periodic_grid(bz, topo), lateral_walls=True), "walls")
    with pytest.raises(TypeError):
        bz.balance_adiabatically_(object(), Δt=1.0)


def test_low_level_form_needs_a_step(bz):
    m = _fake(bz.AtmosphereModel, _periodic_grid(bz), _kinematic=False)
    with pytest.raises(TypeError, match="Δt"):
        bz.balance_adiabatically_(m)
    for bad in (dict(Δt=0.0), dict(Δt=1.0, cycles=0), dict(Δt=1.0, weight=-1.0)):
        with pytest.raises(ValueError):
            bz.balance_adiabatically_(m, **bad)
    m.__dict__.clear()
