"""examples/prescribed_sea_surface_temperature.jl of the reference, its model built from the example's keyword list as written:
128 x 128 (Periodic, Flat, Bounded), halo 5, momentum WENO(order = 9) / scalars WENO(order = 5), warm-phase saturation adjustment,
BulkDrag / BulkSensibleHeatFlux / BulkVaporFlux keyed ρu, ρv, ρe, ρqᵉ with one PolynomialCoefficient, a top-hat T₀(x), a 1 h
FilteredSurfaceVelocities and Uᵍ = 1e-2 (lines 39-72, 149-200, 260-272); initial state of line 281."""
import numpy as np
import pytest


def build_example_model(bz, float_type=np.float64):
    grid = bz.RectilinearGrid(size=(128, 128), halo=(5, 5), x=(-10e3, 10e3), z=(0, 10e3), topology=(bz.Periodic, bz.Flat, bz.Bounded),
                              float_type=float_type)
    p0, θ0 = 101325, 285
    constants = bz.ThermodynamicConstants()
    reference_state = bz.ReferenceState(grid, constants, surface_pressure=p0, potential_temperature=θ0)
    dynamics = bz.AnelasticDynamics(reference_state)
    microphysics = bz.SaturationAdjustment(equilibrium=bz.WarmPhaseEquilibrium())
    momentum_advection, scalar_advection = bz.WENO(order=9), bz.WENO(order=5)
    Ug = 1e-2
    coef = bz.PolynomialCoefficient(roughness_length=1.5e-4)
    filtered_velocities = bz.FilteredSurfaceVelocities(grid, filter_timescale=3600.0)
    ΔT = 4
    T0 = lambda x: θ0 + ΔT / 2 * np.sign(np.cos(2 * np.pi * x / grid.Lx))
    ρu_surface_flux = ρv_surface_flux = bz.BulkDrag(coefficient=coef, gustiness=Ug, surface_temperature=T0, filtered_velocities=filtered_velocities)
    ρe_surface_flux = bz.BulkSensibleHeatFlux(coefficient=coef, gustiness=Ug, surface_temperature=T0, filtered_velocities=filtered_velocities)
    ρqe_surface_flux = bz.BulkVaporFlux(coefficient=coef, gustiness=Ug, surface_temperature=T0, filtered_velocities=filtered_velocities)
    bcs = {"ρu": bz.FieldBoundaryConditions(bottom=ρu_surface_flux), "ρv": bz.FieldBoundaryConditions(bottom=ρv_surface_flux),
           "ρe": bz.FieldBoundaryConditions(bottom=ρe_surface_flux), "ρqᵉ": bz.FieldBoundaryConditions(bottom=ρqe_surface_flux)}
    model = bz.AtmosphereModel(grid, momentum_advection=momentum_advection, scalar_advection=scalar_advection, microphysics=microphysics,
                               dynamics=dynamics, boundary_conditions=bcs)
    model.set(θ=reference_state.potential_temperature, u=1)
    return model


@pytest.mark.gpu
def test_example_model_constructs_and_steps(bz):
    model = build_example_model(bz)
    lo, hi = np.inf, -np.inf
    for _ in range(3):
        u1 = model.velocities["u"].interior_cpu()[0]
        lo, hi = min(lo, u1.min()), max(hi, u1.max())
        model.time_step(10.0)
    model.synchronize()
    u1 = model.velocities["u"].interior_cpu()[0]
    lo, hi = min(lo, u1.min()), max(hi, u1.max())
    for f in (*model.momentum.values(), model.potential_temperature_density, model.moisture_density, model.temperature):
        assert np.all(np.isfinite(f.interior_cpu()))
    uf = model.filtered_surface_field("u")
    print(f"example: filtered u in [{uf.min():.6f}, {uf.max():.6f}], live first-level u over the steps in [{lo:.6f}, {hi:.6f}]")
    assert np.all(np.isfinite(uf)) and lo <= uf.min() and uf.max() <= hi
    # the surface fluxes act: the first level over the warm half gained heat and moisture
    assert model.moisture_density.interior_cpu()[0].max() > 0.0
