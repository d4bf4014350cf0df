"""CPU tests of the surface-layer restatement (tests/surface_layer_reference.py) against the numbers the reference's own test file
holds (tests/golden/polynomial_bulk_coefficients.json, with that file's tolerances), and of the host-side classes."""
import json
import os

import numpy as np
import pytest

import surface_layer_reference as slr

GOLD = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "polynomial_bulk_coefficients.json")))


def test_neutral_coefficient_meets_reference_values():
    g = GOLD["neutral_drag_coefficient_10m"]
    assert tuple(g["polynomial"]) == slr.DRAG_POLYNOMIAL
    for case in g["cases"]:
        assert abs(slr.neutral_coefficient_10m(g["polynomial"], case["U"], g["minimum_wind_speed"]) - case["C"]) < g["atol"]
    # the clamp: below U_min the coefficient is the one at U_min
    assert slr.neutral_coefficient_10m(g["polynomial"], 0.0, 0.1) == slr.neutral_coefficient_10m(g["polynomial"], 0.1, 0.1)


def test_bulk_richardson_number_signs():
    assert slr.bulk_richardson_number(10.0, 288.0, 290.0, 10.0, 0.1) < 0
    assert abs(slr.bulk_richardson_number(10.0, 290.0, 290.0, 10.0, 0.1)) < 1e-10
    assert slr.bulk_richardson_number(10.0, 292.0, 290.0, 10.0, 0.1) > 0


def test_richardson_mapping_signs_and_monotonicity():
    a, b = np.log(1e4), np.log(7.3)
    z = lambda Ri, beta=b: float(slr.zeta_from_richardson(Ri, a, beta))
    assert abs(z(0.0)) < 1e-10
    assert z(-0.5) < 0 and z(-1.0) < 0 and z(0.1) > 0 and z(0.5) > 0
    assert z(-1.0) < z(-0.5) and z(0.5) > z(0.1)
    assert abs(z(0.0, 0.0)) < 1e-10 and z(-1.0, 0.0) < 0 and z(0.5, 0.0) > 0
    assert z(0.19) > 0 and z(0.21) > 0


def test_integrated_stability_functions_meet_reference_values():
    g = GOLD["integrated_stability_functions"]
    for case in g["cases"]:
        print("Psi", case["zeta"], float(slr.psi_momentum(case["zeta"])), float(slr.psi_scalar(case["zeta"])))
        assert abs(slr.psi_momentum(case["zeta"]) - case["psi_momentum"]) < g["atol"]
        assert abs(slr.psi_scalar(case["zeta"]) - case["psi_scalar"]) < g["atol"]
    n = GOLD["neutral_limits"]
    assert abs(slr.psi_momentum(0.0) - n["psi_at_zero"]) < n["atol"] and abs(slr.psi_scalar(0.0) - n["psi_at_zero"]) < n["atol"]
    assert slr.psi_momentum(-1.0) > 0 and slr.psi_scalar(-1.0) > 0 and slr.psi_momentum(1.0) < 0 and slr.psi_scalar(1.0) < 0
    assert slr.psi_momentum(-2.0) > slr.psi_momentum(-1.0) and slr.psi_scalar(-2.0) > slr.psi_scalar(-1.0)
    assert slr.psi_momentum(2.0) < slr.psi_momentum(1.0) and slr.psi_scalar(2.0) < slr.psi_scalar(1.0)


def test_stability_correction_factors():
    g = GOLD["exact_correction_factors"]
    a, b, pd, pt = g["alpha"], g["beta"], g["psi_momentum"], g["psi_scalar"]
    f = slr.stability_correction_factor
    assert f(a, b, 0.0, 0.0, "momentum") == pytest.approx(1.0) and f(a, b, 0.0, 0.0, "scalar") == pytest.approx(1.0)
    assert f(a, b, 1.0, 1.0, "momentum") > 1.0 and f(a, b, 1.0, 1.0, "scalar") > 1.0
    assert f(a, b, -2.0, -2.0, "momentum") < 1.0 and f(a, b, -2.0, -2.0, "scalar") < 1.0
    assert f(a, b, pd, 0.0, "momentum") == pytest.approx((a / (a - pd)) ** 2)
    assert f(a, b, pd, pt, "scalar") == pytest.approx((a / (a - pd)) * ((a + b) / ((a + b) - pt)))
    assert f(a, b, 1.0, 1.0, "momentum") != f(a, b, 1.0, 1.0, "scalar")
    # the floors: a Psi beyond alpha cannot flip the sign
    assert f(a, b, 20.0, 0.0, "momentum") == pytest.approx(100.0)
    s = GOLD["neutral_limits"]["stability_function_at_zero"]
    for kind in ("momentum", "scalar"):
        assert abs(slr.fitted_stability_function(0.0, np.log(s["alpha_exp"]), np.log(s["beta_exp"]), kind) - s["value"]) < s["atol"]


def test_filter_closed_forms():
    g = GOLD["filter"]
    c = g["velocities_update"]
    eps = c["dt"] / c["timescale"]
    for val in (c["u"], c["v"]):
        one = slr.filter_update(c["start"], val, eps)
        assert abs(one - (0.0 + 0.1 * val) / 1.1) < g["atol"]
        assert abs(slr.filter_update(one, val, eps) - (one + 0.1 * val) / 1.1) < g["atol"]
    for c in (g["scalar_update"], g["theta_v_update"]):
        eps = c["dt"] / c["timescale"]
        assert abs(slr.filter_update(c["start"], c["value"], eps) - (0.0 + eps * c["value"]) / (1 + eps)) < g["atol"]
    L = g["lag"]
    eps = L["dt"] / L["timescale"]
    u = slr.filter_update(L["u_start"], L["u_new"], eps)
    assert abs(u - L["u_start"] / (1 + eps)) < g["atol"] and u > L["lagged_above"]
    for _ in range(L["converge_updates"]):
        u = slr.filter_update(u, L["u_new"], 1.0)
    assert abs(u - L["u_new"]) < L["converged_atol"]
    th = slr.filter_update(L["theta_start"], L["theta_new"], eps)
    assert abs(th - (300.0 + eps * 290.0) / (1 + eps)) < g["atol"] and th > L["theta_lagged_above"]


def test_flux_restatement_reduces_to_the_constant_coefficient_oracle(oracle):
    """a number for the coefficient and for T0, no filter: the restatement's fluxes are the oracle's own constant-coefficient ones"""
    from oracle.forcings import BulkFluxes, ColumnForcings
    import helpers
    B = BulkFluxes(101500.0, 1e5, drag=(1.2e-3, 0.2, 299.8), heat=(1.1e-3, 0.2, 300.4), vapor=(1.3e-3, 0.1, 300.4))
    oms = []
    for bulk in (B, slr.SurfaceLayer(101500.0, 1e5, drag=B.drag_params, heat=B.heat, vapor=B.vapor)):
        og = oracle.Grid((8, 6, 6), x=(0, 800.0), y=(0, 600.0), z=(0, 600.0))
        om = oracle.OracleModel(og, surface_pressure=101500.0, potential_temperature=299.1, microphysics="SaturationAdjustment",
                                forcings=ColumnForcings(bulk=bulk))
        helpers.randomize(om, 5)
        for n in om.G:
            om.G[n][...] = 0.0
        oms.append(om)
    from oracle.forcings import add_flux_bc_tendencies
    add_flux_bc_tendencies(oms[0])
    with slr.patched_oracle():
        add_flux_bc_tendencies(oms[1])
    for n in ("ru", "rv", "rtheta", "rq"):
        a, b = oms[0].G[n], oms[1].G[n]
        assert np.abs(a).max() > 0 and np.abs(a - b).max() <= 1e-14 * np.abs(a).max(), n


# ---- host logic without a GPU -------------------------------------------------------------------------------------------------------
def _bcs(bz, grid, coefficient, T0, fv=None, same_drag=True):
    d = bz.BulkDrag(coefficient=coefficient, gustiness=1e-2, surface_temperature=T0, filtered_velocities=fv)
    return {"ρu": bz.FieldBoundaryConditions(bottom=d), "ρv": bz.FieldBoundaryConditions(bottom=d),
            "ρe": bz.FieldBoundaryConditions(bottom=bz.BulkSensibleHeatFlux(coefficient=coefficient, gustiness=1e-2, surface_temperature=T0, filtered_velocities=fv)),
            "ρqᵉ": bz.FieldBoundaryConditions(bottom=bz.BulkVaporFlux(coefficient=coefficient, gustiness=1e-2, surface_temperature=T0, filtered_velocities=fv))}


def test_host_fills_default_polynomials_and_roughness(bz):
    from breeze_jl_amd import forcings as F
    grid = bz.RectilinearGrid((8, 4), x=(-10e3, 10e3), z=(0, 1e3), topology=(bz.Periodic, bz.Flat, bz.Bounded))
    ref = bz.ReferenceState(grid, surface_pressure=101325, potential_temperature=285)
    coef = bz.PolynomialCoefficient(roughness_length=1.5e-4)
    assert coef.polynomial is None and coef.stability_function.scalar_roughness_length == 1.5e-4 / 7.3
    fv = bz.FilteredSurfaceVelocities(grid, filter_timescale=3600.0)
    T0 = lambda x: 285 + 2 * np.sign(np.cos(2 * np.pi * x / grid.Lx))
    L, keep, got_fv = F.materialize_surface_layer(grid, _bcs(bz, grid, coef, T0, fv), ref, bz.ThermodynamicConstants())
    assert got_fv is fv and L.filtered == 1 and L.filter_timescale == 3600.0 and L.filter_stage_mask == 0b101 and L.filter_height_set == 0
    for flux, poly in ((L.drag, slr.DRAG_POLYNOMIAL), (L.heat, slr.HEAT_POLYNOMIAL), (L.vapor, slr.VAPOR_POLYNOMIAL)):
        assert flux.enabled == 1 and flux.polynomial == 1 and (flux.poly.a0, flux.poly.a1, flux.poly.a2) == poly
        assert flux.poly.stability == 1 and flux.poly.scalar_roughness_length == 1.5e-4 / 7.3 and flux.poly.minimum_wind_speed == 0.1
        assert [getattr(flux.poly, n) for n in ("bs22", "aw22", "gamma_d", "psi_b")] == [-1.303, 52.50, 19.3, 2 / 3]
    # a callable T0 is evaluated at the cell centres
    want = np.array([[T0(x) for x in grid.xᶜ]])
    assert all(np.array_equal(k, want) for k in keep) and len(keep) == 3
    # an explicit polynomial wins; stability_function=None switches the correction off
    c2 = bz.PolynomialCoefficient(polynomial=(1.0, 2.0, 3.0), stability_function=None)
    L2, _, fv2 = F.materialize_surface_layer(grid, _bcs(bz, grid, c2, 290.0), ref, bz.ThermodynamicConstants())
    assert fv2 is None and L2.filtered == 0 and (L2.heat.poly.a0, L2.heat.poly.a1, L2.heat.poly.a2) == (1.0, 2.0, 3.0)
    assert L2.heat.poly.stability == 0 and not L2.heat.surface_temperature_field and L2.heat.surface_temperature == 290.0
    with pytest.raises(ValueError):      # bulk_drag.jl:78-80
        bz.BulkDrag(coefficient=bz.PolynomialCoefficient())
    h = bz.FilteredSurfaceVelocities(grid, height=10.0, filter_timescale=60.0)
    L3, _, _ = F.materialize_surface_layer(grid, _bcs(bz, grid, coef, 290.0, h), ref, bz.ThermodynamicConstants())
    assert L3.filter_height_set == 1 and L3.filter_height == 10.0
    # T0(x, y) on a 3-D grid
    g3 = bz.RectilinearGrid((4, 3, 4), x=(0, 4.0), y=(0, 3.0), z=(0, 1.0))
    a = F.surface_temperature_field(g3, lambda x, y: 280 + x + 10 * y)
    assert a.shape == (3, 4) and a[2, 1] == 280 + 1.5 + 25.0


def test_constant_conditions_still_produce_the_old_struct(bz):
    from breeze_jl_amd import forcings as F
    grid = bz.RectilinearGrid((8, 4), x=(-10e3, 10e3), z=(0, 1e3), topology=(bz.Periodic, bz.Flat, bz.Bounded))
    ref = bz.ReferenceState(grid, surface_pressure=101500.0, potential_temperature=299.1)
    bcs = {"ρu": bz.FieldBoundaryConditions(bottom=bz.BulkDrag(coefficient=1.2e-3, gustiness=0.2, surface_temperature=299.8)),
           "ρe": bz.FieldBoundaryConditions(bottom=bz.BulkSensibleHeatFlux(coefficient=1.1e-3, gustiness=0.2, surface_temperature=300.4)),
           "ρqᵉ": bz.FieldBoundaryConditions(bottom=bz.BulkVaporFlux(coefficient=1.3e-3, gustiness=0.1, surface_temperature=300.4))}
    assert not F.needs_surface_layer(bcs)
    assert F.materialize_surface_layer(grid, bcs, ref, bz.ThermodynamicConstants()) == (None, None, None)
    B = F.materialize_bulk_fluxes(bcs, ref, bz.ThermodynamicConstants())
    assert (B.drag_coefficient, B.drag_gustiness, B.drag_surface_temperature) == (1.2e-3, 0.2, 299.8)
    assert (B.heat_coefficient, B.heat_surface_temperature, B.vapor_coefficient, B.vapor_gustiness) == (1.1e-3, 300.4, 1.3e-3, 0.1)
    assert B.surface_pressure == 101500.0
