"""Float64 restatement of the bulk surface fluxes on the compressible split-explicit model.  TEST INFRASTRUCTURE ONLY.

Restated (paths relative to the reference):
  where a stage adds them: after compute_slow_momentum_tendencies! / compute_slow_scalar_tendencies!, before the substep loop
                                                                               src/TimeSteppers/acoustic_runge_kutta_3.jl:187-196
  compute_flux_bc_tendencies!: G[i, j, 1] += J / dz_1 for a bottom flux        src/AtmosphereModels/update_atmosphere_model_state.jl:418-434
  BulkDrag  J^u = -rho0 C^D U~ u at the x face, J^v at the y face              src/BoundaryConditions/bulk_drag.jl:114-135
  BulkSensibleHeatFlux  J^th = -rho0 C^T U~ (theta - theta0)                   src/BoundaryConditions/bulk_scalar_fluxes.jl:82-90,123-137
  BulkVaporFlux  J^v = -rho0 C^v U~ (q^v - q^v+(T0, rho0)), planar liquid     src/BoundaryConditions/bulk_scalar_fluxes.jl:206-232
  q^v+ = p^v+(T0) / (rho0 R^v T0); p^v+ by Clausius-Clapeyron, or by the TetensFormula of a Kessler model's constants
                                                     src/Thermodynamics/clausius_clapeyron.jl:59, tetens_formula.jl:110-117
  U~ = sqrt(U^2 + gustiness^2), U^2 interpolated to the flux location          src/BoundaryConditions/BoundaryConditions.jl:64-85
  rho0 = p0 / (R^d T0) (surface_density), theta0 = T0 / (p0 / p_st)^(R^d / c_pd), p0 = the dynamics' surface_pressure
  BulkSensibleHeatFlux keyed rho e in this potential-temperature model: moved to rho theta with the potential-temperature difference,
  unchanged (PotentialTemperatureFlux)                 src/BoundaryConditions/BoundaryConditions.jl:218-227, thermodynamic_variable_bcs.jl
  BulkDrag without surface_temperature throws under CompressibleDynamics       src/CompressibleEquations/compressible_dynamics.jl:520-525
The surface temperature is a number or an (Ny, Nx) centre array; the drag at an x or y face reads the array at its own index.
q^v is the diagnosed vapour fraction under SaturationAdjustment and the specific prognostic moisture otherwise.

PARITY STATUS: unpinned against the reference (nothing of it runs here).  tests/test_compressible_surface_flux_reference.py pins this file
against the anelastic oracle's bulk-flux code (oracle/forcings.py: _add_bulk_fluxes, itself from the same lines) and against closed forms."""
import numpy as np

from oracle.oracle_compressible import CompressibleOracleModel


class SurfaceFluxes:
    """each of drag / heat / vapor: None or (coefficient, gustiness, T0) with T0 a number or an (Ny, Nx) array"""

    def __init__(self, drag=None, heat=None, vapor=None):
        self.drag, self.heat, self.vapor = drag, heat, vapor


def saturation_specific_humidity_liquid(T0, rho0, tc):
    """saturation_specific_humidity(T, rho, constants, PlanarLiquidSurface()): Clausius-Clapeyron with a constant heat-capacity difference"""
    dc = tc.cpv - tc.cl
    L0 = tc.Ll - dc * tc.T_energy
    ps = tc.ptr * (T0 / tc.Ttr) ** (dc / tc.Rv) * np.exp((1.0 / tc.Ttr - 1.0 / T0) * L0 / tc.Rv)
    return ps / (rho0 * tc.Rv * T0)


def first_level_fluxes(m, F):
    """{"ru" | "rv" | "rtheta" | "rq": J (Ny, Nx)} of the fluxes F on the model's first-level u, v, theta, q^v (halo cells current)"""
    from oracle.thermo import ThermoConstants
    g, c = m.grid, m.constants
    I = g.interior
    z = g.Hz
    y0, y1, x0, x1 = g.Hy, g.Hy + g.Ny, g.Hx, g.Hx + g.Nx
    u, v = m.u[z], m.v[z]                       # first level with halos
    sq = lambda a, jo, io: a[y0 + jo:y1 + jo, x0 + io:x1 + io] ** 2      # noqa: E731
    T0_of = lambda T0: np.broadcast_to(np.asarray(T0, dtype=np.float64), (g.Ny, g.Nx))      # noqa: E731
    J = {}
    if F.drag is not None:
        C, gust, T0 = F.drag
        rho0 = m.p0 / (c.Rd * T0_of(T0))
        v2_fc = ((sq(v, 0, -1) + sq(v, 1, -1)) / 2 + (sq(v, 0, 0) + sq(v, 1, 0)) / 2) / 2
        u2_cf = ((sq(u, -1, 0) + sq(u, -1, 1)) / 2 + (sq(u, 0, 0) + sq(u, 0, 1)) / 2) / 2
        ui, vi = u[y0:y1, x0:x1], v[y0:y1, x0:x1]
        J["ru"] = -rho0 * C * np.sqrt(ui ** 2 + v2_fc + gust ** 2) * ui
        J["rv"] = -rho0 * C * np.sqrt(u2_cf + vi ** 2 + gust ** 2) * vi
    U2c = (sq(u, 0, 0) + sq(u, 0, 1)) / 2 + (sq(v, 0, 0) + sq(v, 1, 0)) / 2
    if F.heat is not None:
        C, gust, T0 = F.heat
        T0 = T0_of(T0)
        rho0 = m.p0 / (c.Rd * T0)
        theta0 = T0 / (m.p0 / m.pst) ** (c.Rd / c.cpd)
        J["rtheta"] = -rho0 * C * np.sqrt(U2c + gust ** 2) * (I(m.theta)[0] - theta0)
    if F.vapor is not None:
        C, gust, T0 = F.vapor
        T0 = T0_of(T0)
        rho0 = m.p0 / (c.Rd * T0)
        if m.microphysics == "Kessler":      # a Kessler model's constants carry a TetensFormula: saturation_vapor_pressure dispatches on it
            t = m.tetens                     # (src/Thermodynamics/tetens_formula.jl:110-117; oracle/kessler.py)
            q0 = t.psat_ref * np.exp(t.a_liquid * (T0 - t.T_ref) / (T0 - t.dT_liquid)) / (rho0 * t.Rv * T0)
        else:
            q0 = saturation_specific_humidity_liquid(T0, rho0, ThermoConstants())
        qv = I(m.qv)[0] if m.microphysics == "SaturationAdjustment" else I(m.q)[0]
        J["rq"] = -rho0 * C * np.sqrt(U2c + gust ** 2) * (qv - q0)
    return J


def add_flux_bc_tendencies(m, F):
    """compute_flux_bc_tendencies!: G[.., 1] += J / dz_1"""
    g = m.grid
    dz = g.dzc[g.Hz]
    for name, J in first_level_fluxes(m, F).items():
        g.interior(m.G[name])[0] += J * 1.0 / dz


class SurfaceFluxMixin:
    """compute_slow_tendencies of the class behind it, then the bulk surface fluxes at k = 0 (`surface_fluxes`: a SurfaceFluxes, or None)"""
    surface_fluxes = None

    def compute_slow_tendencies(self):
        super().compute_slow_tendencies()
        if self.surface_fluxes is not None:
            add_flux_bc_tendencies(self, self.surface_fluxes)


class SurfaceFluxCompressibleModel(SurfaceFluxMixin, CompressibleOracleModel):
    def __init__(self, grid, surface_fluxes=None, **kw):
        super().__init__(grid, **kw)
        self.surface_fluxes = surface_fluxes
