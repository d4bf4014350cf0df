"""Host-side mirror of Breeze's compressible split-explicit API above the C ABI (include/breeze_hip.h):

  CompressibleDynamics(time_discretization; ...)   src/CompressibleEquations/compressible_dynamics.jl:44-160
  SplitExplicitTimeDiscretization(; ...)           src/CompressibleEquations/time_discretizations.jl:535-598
  ThermalDivergenceDamping / NoDivergenceDamping   src/CompressibleEquations/time_discretizations.jl:142-262
  ExnerReferenceState(grid, constants; ...)        src/Thermodynamics/reference_states.jl:588-672,717-815
  AcousticSubstepper / AcousticRungeKutta3         src/CompressibleEquations/acoustic_substepping.jl:91-270,
                                                   src/TimeSteppers/acoustic_runge_kutta_3.jl:64-103
  set! / update_state! / time_step!                src/AtmosphereModels/set_atmosphere_model.jl:198-362,
                                                   src/TimeSteppers/acoustic_runge_kutta_3.jl:230-319
  HydrostaticallyBalancedDensity / set_to_mean!    src/AtmosphereModels/set_to_mean.jl:152-229,243-310
(paths relative to /root/reference; Julia's `f!` is spelled `f_`).  Every numerical operation of the time step is a
HIP kernel behind libbreeze_hip.so; the numpy code here only builds the 1-D reference columns, at construction and in set_to_mean_.
"""
import ctypes as C

import numpy as np

from . import _context, _lib
from .grids import Bounded, Center, Face, Flat, Periodic, RectilinearGrid  # noqa: F401
from .model import WENO, Clock, Field, _LOC
from .thermodynamics import ThermodynamicConstants, dry_air_gas_constant, vapor_gas_constant


class NoDivergenceDamping:
    pass


class ThermalDivergenceDamping:
    def __init__(self, coefficient=0.1, length_scale=None, damp_vertical=False):
        if length_scale is not None and not float(length_scale) > 0:
            raise ValueError(f"`length_scale` must be positive (got {length_scale})")
        self.coefficient, self.damp_vertical = float(coefficient), bool(damp_vertical)
        self.length_scale = None if length_scale is None else float(length_scale)      # fixed diffusivity alpha l^2 / dtau


class DirectDivergenceDamping:
    """DirectDivergenceDamping(coefficient=0.1) (time_discretizations.jl:269-274): the horizontal theta-flux divergence of the
    perturbation momentum is differenced directly (acoustic_substepping.jl:1146-1188); horizontal only."""

    def __init__(self, coefficient=0.1):
        self.coefficient = float(coefficient)


class ProportionalSubsteps:
    """each stage covers beta dt with ceil(beta N) substeps sized to tile it (acoustic_substepping.jl:491-495; the default)"""
    code = 0


class ConstantSubstepSize:
    """one substep size dt / N for all stages, N rounded up to a multiple of 6 (acoustic_substepping.jl:497-501)"""
    code = 1


class MonolithicFirstStage:
    """stage 1 collapses to one substep of dt / 3, stages 2-3 as ConstantSubstepSize (acoustic_substepping.jl:503-508)"""
    code = 2


class LinearRamp:
    code = 1


class CubicRamp:
    code = 2


class Sin2Ramp:
    code = 3


class UpperSponge:
    """UpperSponge(damping_rate=0.2, depth=5e3, ramp=CubicRamp()) (time_discretizations.jl:435-512): implicit Rayleigh damping of
    (ρw)′ in a layer of thickness `depth` below z = grid.Lz, inside the column system of the acoustic substeps
    (acoustic_substepping.jl:584-602,639,948)."""

    def __init__(self, damping_rate=0.2, depth=5e3, ramp=None):
        ramp = CubicRamp() if ramp is None else ramp
        if not isinstance(ramp, (LinearRamp, CubicRamp, Sin2Ramp)):
            raise ValueError("`ramp` must be an `<:AbstractRamp` (e.g. `CubicRamp()`, `Sin2Ramp()`, `LinearRamp()`)")
        self.damping_rate, self.depth, self.ramp = float(damping_rate), float(depth), ramp


class SplitExplicitTimeDiscretization:
    def __init__(self, substeps=None, acoustic_cfl=0.5, forward_weight=0.65, thermodynamic_tendency_factor=1,
                 vertical_momentum_tendency_factor=1, apply_first_substep_pressure_gradient=False, damping=None,
                 sponge=None, substep_distribution=None, open_boundary_relaxation=0.5):
        damping = ThermalDivergenceDamping(coefficient=0.1) if damping is None else damping
        if not isinstance(damping, (ThermalDivergenceDamping, DirectDivergenceDamping, NoDivergenceDamping)):
            raise ValueError("`damping` must be an `AcousticDampingStrategy`")
        if sponge is not None and not isinstance(sponge, UpperSponge):
            raise ValueError("`sponge` must be an `UpperSponge` or None")
        if substep_distribution is not None and not isinstance(substep_distribution, (ProportionalSubsteps, ConstantSubstepSize, MonolithicFirstStage)):
            raise ValueError("`substep_distribution` must be ProportionalSubsteps(), ConstantSubstepSize() or MonolithicFirstStage()")
        if not acoustic_cfl > 0:
            raise ValueError(f"`acoustic_cfl` must be positive (got {acoustic_cfl})")
        if not 0 < open_boundary_relaxation <= 1:      # time_discretizations.jl:573-574
            raise ValueError(f"`open_boundary_relaxation` must be in (0, 1] (got {open_boundary_relaxation})")
        self.open_boundary_relaxation = float(open_boundary_relaxation)
        self.substeps = None if substeps is None else int(substeps)
        self.acoustic_cfl = float(acoustic_cfl)
        self.forward_weight = float(forward_weight)
        self.thermodynamic_tendency_factor = float(thermodynamic_tendency_factor)
        self.vertical_momentum_tendency_factor = float(vertical_momentum_tendency_factor)
        self.apply_first_substep_pressure_gradient = bool(apply_first_substep_pressure_gradient)
        self.damping = damping
        self.sponge = sponge
        self.substep_distribution = substep_distribution or ProportionalSubsteps()


class NormalFlowBoundaryCondition:
    """NormalFlowBoundaryCondition(value) on the wall-normal momentum of a Bounded side (the open boundary of
    test/acoustic_substepping_open_boundaries.jl:56-57): `condition is None` is the impenetrable default."""

    def __init__(self, condition=None):
        self.condition = condition


def is_active_open_bc(bc):
    """is_active_open_bc (acoustic_substepping.jl:1318)"""
    return isinstance(bc, NormalFlowBoundaryCondition) and bc.condition is not None


class NewtonSolver:
    """Breeze.Solvers.NewtonSolver (src/Solvers.jl:55-83): reltol = 0 only."""

    def __init__(self, abstol=1e-4, maxiter=8):
        self.reltol, self.abstol, self.maxiter = 0.0, float(abstol), int(maxiter)


def _z_metrics(grid):
    """Δzᶜ (Nz) and Δzᶠ (centre spacing at faces 0..Nz; entries 1..Nz-1 interior) as Oceananigans defines them."""
    Nz = grid.Nz
    if grid.regular_z:
        return np.full(Nz, grid.Δz), np.full(Nz + 1, grid.Δz)
    dzc = np.diff(grid.zᶠ)
    zc = grid.zᶜ
    dzf = np.empty(Nz + 1)
    dzf[1:Nz] = np.diff(zc)
    dzf[0] = 2 * (zc[0] - grid.zᶠ[0])
    dzf[Nz] = 2 * (grid.zᶠ[Nz] - zc[Nz - 1])
    return dzc, dzf


def _exner_column(θ, qv, dzc, dzf, p0, pst, c):
    """_compute_exner_column! (reference_states.jl:588-672) on float64 profiles θ, qᵛ of Nz levels: (π, p, ρ) and the surface Exner function."""
    Nz = len(θ)
    Rd, Rv = dry_air_gas_constant(c), vapor_gas_constant(c)
    cpd, cpv, g = c.dry_air_heat_capacity, c.vapor_heat_capacity, c.gravitational_acceleration

    def moist(q):      # moist_reference_constants (reference_states.jl:572-577); exactly the dry constants for q = 0
        qd = 1 - q
        Rm, cpm = qd * Rd + q * Rv, qd * cpd + q * cpv
        return Rm, cpm, Rm / cpm

    π, p, ρ = np.zeros(Nz), np.zeros(Nz), np.zeros(Nz)
    Rm1, cpm1, κ1 = moist(qv[0])
    π_surface = (p0 / pst) ** κ1
    π[0] = π_surface - g * dzc[0] / (2 * cpm1 * θ[0])
    p[0] = pst * π[0] ** (1 / κ1)
    ρ[0] = p[0] / (Rm1 * θ[0] * π[0])
    for k in range(1, Nz):
        Rm, cpm, κ = moist(qv[k])
        θface = (θ[k] + θ[k - 1]) / 2
        pk = pst * (π[k - 1] - g * dzf[k] / (cpm * θface)) ** (1 / κ)
        A = g * pst ** κ / (2 * Rm * θ[k])
        Cc = p[k - 1] / dzf[k] - g * ρ[k - 1] / 2
        for _ in range(5):                                   # FixedIterations(5) Newton on the discrete balance
            ρp = pk ** (-κ)
            f = pk / dzf[k] + A * pk * ρp - Cc
            df = 1 / dzf[k] + A * (1 - κ) * ρp
            pk -= f / df
        p[k] = pk
        π[k] = (pk / pst) ** κ
        ρ[k] = pk / (Rm * θ[k] * π[k])
    return π, p, ρ, π_surface, Rm1


class ExnerReferenceState:
    """1-D, isentropic-mode ExnerReferenceState, dry or moist (`vapor_mass_fraction` a number or qᵛ(z)): the discrete
    hydrostatic balance (p[k]-p[k-1])/Δzᶠ + g (ρ[k]+ρ[k-1])/2 = 0 holds to rounding at every interior face
    (src/Thermodynamics/reference_states.jl:572-672,718-827).  `from_profiles` builds one from θ and qᵛ given as arrays of Nz levels;
    `set_profiles_` recomputes the columns of an existing one in place (set_to_mean!): both run the integration of the constructor."""

    def __init__(self, grid, constants=None, surface_pressure=101325, potential_temperature=288, standard_pressure=1e5,
                 vapor_mass_fraction=None, reference_temperature=None):
        if reference_temperature is not None:
            raise NotImplementedError("the isothermal ExnerReferenceState mode is not implemented")
        Nz = grid.Nz
        θfun = potential_temperature if callable(potential_temperature) else (lambda z: float(potential_temperature) + 0.0 * z)
        θ = np.asarray(θfun(grid.zᶜ), dtype=np.float64)
        if vapor_mass_fraction is None:
            qv = np.zeros(Nz)
        elif callable(vapor_mass_fraction):
            qv = np.array([float(vapor_mass_fraction(z)) for z in grid.zᶜ])
        else:
            qv = np.full(Nz, float(vapor_mass_fraction))
        self._build(grid, constants, surface_pressure, standard_pressure, θ, qv, float(θfun(np.float64(0.0))))

    @classmethod
    def from_profiles(cls, grid, potential_temperature, vapor_mass_fraction=None, constants=None, surface_pressure=101325,
                      standard_pressure=1e5, surface_potential_temperature=None):
        """The reference state of θ and qᵛ given level by level (arrays of Nz values at the cell centres); the surface θ of the bottom
        boundary values defaults to the first level's."""
        θ = np.array(potential_temperature, dtype=np.float64).reshape(-1)
        qv = np.zeros(grid.Nz) if vapor_mass_fraction is None else np.array(vapor_mass_fraction, dtype=np.float64).reshape(-1)
        if θ.shape != (grid.Nz,) or qv.shape != (grid.Nz,):
            raise ValueError(f"profiles must have Nz = {grid.Nz} levels")
        self = cls.__new__(cls)
        self._build(grid, constants, surface_pressure, standard_pressure, θ, qv,
                    float(θ[0] if surface_potential_temperature is None else surface_potential_temperature))
        return self

    def _build(self, grid, constants, surface_pressure, standard_pressure, θ, qv, θ_surface):
        self.constants = c = constants or ThermodynamicConstants()
        self.grid = grid
        self.Nz, self.Hz = grid.Nz, grid.Hz
        self.surface_pressure = float(surface_pressure)
        self.standard_pressure = float(standard_pressure)
        self.surface_potential_temperature = θ_surface
        self.surface_density = None
        self.set_profiles_(θ, qv)

    def set_profiles_(self, potential_temperature, vapor_mass_fraction):
        """Recompute exner_function, pressure and density in place from level profiles of θ and qᵛ.  The halo levels follow the boundary
        conditions the reference's fields are built with (reference_states.jl:795-817): pressure and density carry the ValueBoundaryCondition
        of construction at the bottom — the surface pressure, and the surface density of the FIRST profiles, which set_to_mean! does not
        touch — and the default no-flux condition on top; the Exner function is no-flux on both sides."""
        Nz, Hz = self.Nz, self.Hz
        θ = np.asarray(potential_temperature, dtype=np.float64)
        qv = np.asarray(vapor_mass_fraction, dtype=np.float64)
        dzc, dzf = _z_metrics(self.grid)
        p0 = self.surface_pressure
        π, p, ρ, π_surface, Rm1 = _exner_column(θ, qv, dzc, dzf, p0, self.standard_pressure, self.constants)
        if self.surface_density is None:
            self.surface_density = p0 / (Rm1 * self.surface_potential_temperature * π_surface)
        ρ0 = self.surface_density

        def with_halos(a, bottom_value=None):
            out = np.zeros(Nz + 2 * Hz)
            out[Hz:Hz + Nz] = a
            out[Hz - 1] = a[0] if bottom_value is None else 2 * bottom_value - a[0]
            out[Hz + Nz] = a[-1]
            return out

        self.vapor_mass_fraction = np.array(qv)
        self.pressure = with_halos(p, p0)
        self.density = with_halos(ρ, ρ0)
        self.exner_function = with_halos(π)
        self.potential_temperature = with_halos(θ)


class HydrostaticallyBalancedDensity:
    """HydrostaticallyBalancedDensity(surface_pressure=None) (set_to_mean.jl:243-260): passed as `ρ` to `set`, the density is put into
    discrete moist hydrostatic balance with the θˡⁱ and qᵛ just set, column by column upward from `surface_pressure` (None: the dynamics'
    surface pressure)."""

    def __init__(self, surface_pressure=None):
        if surface_pressure is not None and not float(surface_pressure) > 0:
            raise ValueError(f"`surface_pressure` must be positive (got {surface_pressure})")
        self.surface_pressure = None if surface_pressure is None else float(surface_pressure)


class CompressibleDynamics:
    def __init__(self, time_discretization=None, standard_pressure=1e5, surface_pressure=101325.0,
                 reference_potential_temperature=None, reference_vapor_mass_fraction=None, reference_state="auto"):
        if time_discretization is None or not isinstance(time_discretization, SplitExplicitTimeDiscretization):
            raise NotImplementedError("the HIP path implements CompressibleDynamics(SplitExplicitTimeDiscretization(...)); "
                                      "ExplicitTimeStepping is outside the hot-path scope")
        self._reference_given = reference_state if isinstance(reference_state, ExnerReferenceState) else None
        if self._reference_given is not None:      # an already built state: its columns are taken as they are, halo levels included
            if reference_potential_temperature is not None or reference_vapor_mass_fraction is not None:
                raise ValueError("an ExnerReferenceState passed as `reference_state` is mutually exclusive with an explicit reference profile")
            reference_state = "auto"
        if reference_state not in ("auto", ":auto", None):
            raise ValueError(f"`reference_state` must be `:auto` or `nothing`; received {reference_state!r}.")
        if reference_state is None and reference_potential_temperature is not None:
            raise ValueError("`reference_state = nothing` disables the reference state and is mutually exclusive with an "
                             "explicit reference profile")
        self.time_discretization = time_discretization
        self.standard_pressure = float(standard_pressure)
        self.surface_pressure = float(surface_pressure)
        self._reference_vapor = reference_vapor_mass_fraction
        self._reference_spec = None if reference_state is None else (
            288.0 if reference_potential_temperature is None else reference_potential_temperature)
        # materialised by the model
        self.reference_state = None
        self.dry_density = self.total_density = self.pressure = None


class AcousticSubstepper:
    """Storage of the acoustic substepper (acoustic_substepping.jl:91-134, 207-231)."""

    FIELDS = (("exner", "ccc"), ("potential_temperature", "ccc"), ("gamma_R_mixture", "ccc"),
              ("density_perturbation", "ccc"), ("density_potential_temperature_perturbation", "ccc"),
              ("momentum_perturbation_u", "fcc"), ("momentum_perturbation_v", "cfc"), ("momentum_perturbation_w", "ccf"),
              ("density_predictor", "ccc"), ("density_potential_temperature_predictor", "ccc"),
              ("previous_density_potential_temperature_perturbation", "ccc"),
              ("time_averaged_u", "fcc"), ("time_averaged_v", "cfc"), ("time_averaged_w", "ccf"),
              ("slow_vertical_momentum_tendency", "ccf"), ("vertical_solver_source_term", "ccf"))

    # stored in substep_floattype (acoustic_substepping.jl:207-223); (rho w)', the solver's right-hand side, the slow vertical tendency
    # and the time-averaged velocities keep eltype(grid)
    WORKING = ("exner", "potential_temperature", "gamma_R_mixture", "density_perturbation", "density_potential_temperature_perturbation",
               "momentum_perturbation_u", "momentum_perturbation_v", "density_predictor", "density_potential_temperature_predictor",
               "previous_density_potential_temperature_perturbation")

    def __init__(self, grid, time_discretization, device, substep_floattype=None):
        td = time_discretization
        self.substeps, self.acoustic_cfl, self.forward_weight = td.substeps, td.acoustic_cfl, td.forward_weight
        self.damping = td.damping
        self.substep_floattype = np.dtype(grid.float_type if substep_floattype is None else substep_floattype).type
        if self.substep_floattype not in (np.float32, np.float64) or np.dtype(self.substep_floattype).itemsize > grid.ftype:
            raise NotImplementedError("substep_floattype: eltype(grid) or Float32 inside a Float64 model")
        for name, loc in self.FIELDS:
            setattr(self, name, Field(grid, _LOC[loc], device, float_type=self.substep_floattype if name in self.WORKING else None))
        self.linearization_exner = self.exner
        self.linearization_potential_temperature = self.potential_temperature
        self.linearization_gamma_R_mixture = self.gamma_R_mixture
        self.time_averaged_velocities = {"u": self.time_averaged_u, "v": self.time_averaged_v, "w": self.time_averaged_w}
        self.momentum_perturbation = {"u": self.momentum_perturbation_u, "v": self.momentum_perturbation_v,
                                      "w": self.momentum_perturbation_w}

    def struct(self):
        s = _lib.bz_acoustic_substepper()
        for name, _ in self.FIELDS:
            setattr(s, name, getattr(self, name).ptr())
        return s


class AcousticRungeKutta3:
    """Wicker-Skamarock RK3 with acoustic substepping: β = (1/3, 1/2, 1) (acoustic_runge_kutta_3.jl:64-103)."""

    def __init__(self, grid, prognostic_fields, dynamics, device, substep_floattype=None):
        self.β1, self.β2, self.β3 = 1.0 / 3.0, 1.0 / 2.0, 1.0
        self.U0 = {k: Field(grid, f.loc, device) for k, f in prognostic_fields.items()}
        self.Gn = {k: Field(grid, f.loc, device) for k, f in prognostic_fields.items()}
        self.substepper = AcousticSubstepper(grid, dynamics.time_discretization, device, substep_floattype=substep_floattype)


_ALIASES = {"θ": "θ", "theta": "θ", "θˡⁱ": "θ", "θli": "θ", "ρ": "ρ", "rho": "ρ", "u": "u", "v": "v", "w": "w",
            "qᵗ": "q", "qt": "q", "qᵛ": "q", "qv": "q", "qᶜˡ": "qcl", "qcl": "qcl", "qʳ": "qr", "qr": "qr"}


def _exner_reference_struct(T, dynamics):
    """-> (bz_exner_reference_state of the dynamics' reference state, the column arrays it points to; None without a reference state)."""
    ref, arrays = dynamics.reference_state, None
    br = T.bz_exner_reference_state()
    br.standard_pressure = dynamics.standard_pressure
    if ref is not None:
        arrays = [np.ascontiguousarray(a, dtype=T.np_real) for a in (ref.pressure, ref.density)]
        br.pressure, br.density = (a.ctypes.data_as(C.POINTER(T.real)) for a in arrays)
    return br, arrays


def _split_explicit_struct(T, grid, td, temperature_solver, substep_floattype, sponge=True):
    """-> bz_split_explicit of a SplitExplicitTimeDiscretization; sponge = False leaves the UpperSponge out (the adiabatic-balance twin)."""
    bt = T.bz_split_explicit()
    bt.substeps = 0 if td.substeps is None else td.substeps
    damp = td.damping
    bt.damp_vertical = int(isinstance(damp, ThermalDivergenceDamping) and damp.damp_vertical)
    bt.apply_first_substep_pressure_gradient = int(td.apply_first_substep_pressure_gradient)
    bt.newton_maxiter = temperature_solver.maxiter
    bt.acoustic_cfl, bt.forward_weight = td.acoustic_cfl, td.forward_weight
    bt.damping_coefficient = damp.coefficient if isinstance(damp, (ThermalDivergenceDamping, DirectDivergenceDamping)) else -1.0
    bt.direct_divergence_damping = int(isinstance(damp, DirectDivergenceDamping))
    bt.damping_length_scale = (damp.length_scale or 0.0) if isinstance(damp, ThermalDivergenceDamping) else 0.0
    bt.thermodynamic_tendency_factor = td.thermodynamic_tendency_factor
    bt.vertical_momentum_tendency_factor = td.vertical_momentum_tendency_factor
    bt.newton_abstol = temperature_solver.abstol
    bt.substep_distribution = td.substep_distribution.code
    bt.substep_float_bytes = 4 if (substep_floattype is np.float32 and grid.ftype == 8) else 0
    if sponge and td.sponge is not None:
        bt.sponge_ramp, bt.sponge_damping_rate, bt.sponge_depth = td.sponge.ramp.code, td.sponge.damping_rate, td.sponge.depth
    return bt


class CompressibleAtmosphereModel(_context.ContextOwner):
    """AtmosphereModel(grid; dynamics=CompressibleDynamics(SplitExplicitTimeDiscretization(...)), advection=WENO(order=5))
    — timestepper :AcousticRungeKutta3; coriolis = FPlane(f) and density-keyed Relaxation sponges on ρu, ρv, ρw, ρθ
    (examples/tropical_cyclone_with_rainband.jl:434-514) are the forcing terms built; closure = SmagorinskyLilly(), ScalarDiffusivity(ν, κ)
    or VerticalScalarDiffusivity(ν, κ) with the explicit time discretisation (benchmarking/run_benchmarks.jl:111-119;
    validation/DCMIP2016_TC/dcmip2016_tc.jl:277-292) on single-GPU models that are periodic in x and y; microphysics = SaturationAdjustment,
    DCMIP2016KesslerMicrophysics or — on those single-GPU periodic models — InstantaneousPrecipitation (src/Microphysics/instantaneous_precipitation.jl):
    microphysical_fields = {"qᵛ": the specific-moisture field, "precipitation_rate": a centre Field}, the once-per-step rain-out closes time_step.
    boundary_conditions = {"ρu": BulkDrag(...), "ρv": ..., "ρθ" | "ρe": BulkSensibleHeatFlux(...), "ρqᵛ" | "ρqᵉ" | "ρqᵗ": BulkVaporFlux(...)} — bottom
    bulk surface fluxes with a numeric coefficient, a gustiness and a surface temperature that is a number, an (Ny, Nx) array or T₀(x, y), on the
    single-GPU model that is periodic in x and y (validation/DCMIP2016_TC/dcmip2016_tc.jl:293-311): every stage adds them after its slow tendencies
    (compute_flux_bc_tendencies_); on a walled grid the keyword carries the open lateral sides (NormalFlowBoundaryCondition)."""

    def __init__(self, grid, dynamics, advection=None, thermodynamic_constants=None, temperature_solver=None,
                 closure=None, coriolis=None, microphysics=None, forcing=None, device="cuda:0", substep_floattype=None,
                 boundary_conditions=None):
        """substep_floattype: storage type of the acoustic substepper's working fields (the keyword of the reference's
        AcousticSubstepper constructor, acoustic_substepping.jl:181,199-235): None = eltype(grid); numpy.float32 inside a Float64
        model halves the bytes the substep kernels stream."""
        import torch
        if not isinstance(grid, RectilinearGrid):
            raise TypeError("grid must be a RectilinearGrid")
        # (Periodic, Flat, Bounded): the 2-D x-z cases of examples/acoustic_wave.jl:51 and inertia_gravity_wave.jl:70
        # a Bounded x and / or y (3-D): the acoustic substep loop with its lateral boundaries (refresh_linearization_, acoustic_rk3_substep_loop_).
        # (Periodic, Bounded, Bounded) with impenetrable south and north walls also runs the whole model — set, update_state_, the slow
        # tendencies and time_step (the reference's validation/cartesian_baroclinic_wave); on a Bounded x, or with an active open side, those
        # are not built (the library returns BZ_ERR_UNSUPPORTED)
        self.lateral_walls = Bounded in grid.topology[:2]
        if self.lateral_walls and (Flat in grid.topology or type(self) is not CompressibleAtmosphereModel):
            raise NotImplementedError("Bounded x / y of the compressible model: 3-D grids on one device")
        if not self.lateral_walls and grid.topology not in ((Periodic, Periodic, Bounded), (Periodic, Flat, Bounded)):
            raise NotImplementedError("the HIP path implements topology (Periodic, Periodic, Bounded) and (Periodic, Flat, Bounded)")
        self.boundary_conditions = boundary_conditions or {}
        # bottom bulk surface fluxes (BulkDrag, BulkSensibleHeatFlux, BulkVaporFlux with a numeric coefficient) on the single-device model that
        # is periodic in x and y; a lateral condition there, and every other flux condition, fails by name (forcings.py)
        from .forcings import compressible_surface_flux_conditions
        self._surface_fluxes = compressible_surface_flux_conditions(self.boundary_conditions, grid, type(self) is CompressibleAtmosphereModel,
                                                                    self.lateral_walls)
        if grid.topology[1] == Flat and not (isinstance(advection, WENO) and advection.bounds is None):
            raise NotImplementedError("(Periodic, Flat, Bounded): the WENO(order = 5 | 7 | 9) model is implemented")
        if isinstance(advection, WENO) and advection.order != 5:      # examples/splitting_supercell.jl:279 uses WENO(order = 9)
            need = (advection.order + 1) // 2
            if min(h for h, t in zip((grid.Hx, grid.Hy, grid.Hz), grid.topology) if t != Flat) < need:
                raise ValueError(f"WENO(order={advection.order}) needs halos of at least {need} cells in every direction")
            if advection.bounds is not None:
                raise NotImplementedError("bounds-preserving WENO is implemented for order 5")
        if not isinstance(dynamics, CompressibleDynamics):
            raise TypeError("dynamics must be CompressibleDynamics")
        self._diffusivity = _context.check_closure(closure, f"closure = {type(closure).__name__}")
        if closure is not None:
            if self._diffusivity and closure.vertically_implicit:
                raise NotImplementedError("closure with VerticallyImplicitTimeDiscretization: CompressibleDynamics runs the closures with "
                                          "ExplicitTimeDiscretization (the implicit substep of the reference is not built)")
            if self.lateral_walls:
                raise NotImplementedError("closure: not implemented on a compressible model between walls (Bounded x / Bounded y)")
            if Flat in grid.topology:
                raise NotImplementedError("closure: not implemented on a compressible model with a Flat y")
            if type(self) is not CompressibleAtmosphereModel:
                raise NotImplementedError("closure: not implemented on y-slab (distributed) compressible models")
        self.closure = closure
        from .forcings import FPlane, split_relaxation
        if coriolis is not None and not isinstance(coriolis, FPlane):
            raise NotImplementedError("coriolis: FPlane is implemented")
        forcing_rest, self._relaxation, self._field_forcing = split_relaxation(forcing)
        if forcing_rest:
            raise NotImplementedError("CompressibleDynamics: Relaxation sponges keyed ρu, ρv, ρw, ρθ and a 3-D Forcing on θ / ρθ are the forcings implemented")
        if set(self._relaxation) - {"ρu", "ρv", "ρw", "ρθ"}:
            raise NotImplementedError("CompressibleDynamics: Relaxation sponges keyed ρu, ρv, ρw, ρθ")
        if (coriolis is not None or self._relaxation or self._field_forcing) and type(self) is not CompressibleAtmosphereModel:
            raise NotImplementedError("Coriolis and sponges of the compressible model: single-GPU contexts")
        self.coriolis, self.forcing = coriolis, forcing
        # InstantaneousPrecipitation: the single-device model that is periodic in x and y (its own messages; the list below is for unknown types)
        ip_refused = ("InstantaneousPrecipitation: not implemented on a compressible model between walls (Bounded x / Bounded y)" if self.lateral_walls
                      else "InstantaneousPrecipitation: not implemented on y-slab (distributed) compressible models"
                      if type(self) is not CompressibleAtmosphereModel
                      else "InstantaneousPrecipitation: not implemented on a compressible model with a Flat y" if Flat in grid.topology else None)
        _context.refuse_bulk_microphysics(microphysics, type(self).__name__, "the moisture update of CompressibleDynamics is fused into the acoustic stage epilogue")
        # the constructor attaches the warm-phase adjustment; the density-based mixed-phase form is attached to the built model (set_mixed_phase_equilibrium_)
        _context.refuse_mixed_phase(microphysics, type(self).__name__, "the constructor attaches the warm-phase density-based adjustment; the mixed-phase "
                                    "form is attached to the built model by compressible.set_mixed_phase_equilibrium_(model, MixedPhaseEquilibrium(...))")
        self._kessler = _context.check_microphysics(microphysics, "compressible microphysics: DCMIP2016KesslerMicrophysics() and "
                                                                  "SaturationAdjustment(equilibrium = WarmPhaseEquilibrium()) are implemented",
                                                    instantaneous_precipitation_refused=ip_refused)
        # FlatauPolynomial constants: the single-device model; a bulk vapour flux evaluates the Clausius-Clapeyron qᵛ⁺ of the surface
        if type(self) is not CompressibleAtmosphereModel:
            _context.refuse_flatau_polynomial(thermodynamic_constants, type(self).__name__, "y-slab models evaluate the Clausius-Clapeyron expression")
        if "vapor" in self._surface_fluxes:
            _context.refuse_flatau_polynomial(thermodynamic_constants, type(self).__name__, "BulkVaporFlux evaluates the Clausius-Clapeyron qᵛ⁺ of the surface")
        self.microphysics = microphysics
        from .microphysics import InstantaneousPrecipitation
        self._ip = isinstance(microphysics, InstantaneousPrecipitation)
        self._sa = microphysics is not None and not self._kessler and not self._ip
        if self._kessler:
            _context.check_kessler_constants(thermodynamic_constants)
        if advection is None:
            from .model import Centered
            advection = Centered(order=2)          # the reference's default
        if not torch.cuda.is_available():
            raise RuntimeError("CompressibleAtmosphereModel needs a GPU: the HIP path has no CPU fallback")
        self.grid, self.advection, self.dynamics = grid, advection, dynamics
        self.thermodynamic_constants = c = thermodynamic_constants or ThermodynamicConstants()
        self.temperature_solver = temperature_solver or NewtonSolver()
        self.clock = Clock()
        self.device = torch.device(device)
        torch.cuda.set_device(self.device)
        self._T = T = _lib.types(grid.ftype)
        # eltype(grid) = Float32 (examples/splitting_supercell.jl:86): the Float32 twin of the library
        self._lib = lib = _context.load_library(grid, advection, "Float32 grids: WENO(order = 5 | 7 | 9) is wired up")
        dynamics.dry_density, dynamics.total_density, dynamics.pressure = (Field(grid, _LOC["ccc"], self.device) for _ in range(3))
        fld = _context.allocate_common_fields(self, grid)
        self.microphysical_fields = {}
        if self._kessler:
            _context.materialize_kessler_fields(self, fld)
        if dynamics._reference_given is not None:
            given = dynamics._reference_given
            if (given.Nz, given.Hz) != (grid.Nz, grid.Hz):
                raise ValueError("the ExnerReferenceState passed as `reference_state` was built on another vertical grid")
            dynamics.reference_state = given
        elif dynamics._reference_spec is not None:
            dynamics.reference_state = ExnerReferenceState(grid, c, surface_pressure=dynamics.surface_pressure,
                                                           potential_temperature=dynamics._reference_spec,
                                                           vapor_mass_fraction=dynamics._reference_vapor,
                                                           standard_pressure=dynamics.standard_pressure)
        self.timestepper = AcousticRungeKutta3(grid, self.prognostic_fields(), dynamics, self.device, substep_floattype=substep_floattype)
        self.U0, self.G = self.timestepper.U0, self.timestepper.Gn

        # ---- context ----
        bg, self._zf = _context.grid_struct(T, grid)
        ref = dynamics.reference_state
        br, self._ref_arrays = _exner_reference_struct(T, dynamics)
        bt = _split_explicit_struct(T, grid, dynamics.time_discretization, self.temperature_solver, self.timestepper.substepper.substep_floattype)
        td = dynamics.time_discretization
        self._open_context("bz_create_compressible", bg, _context.constants_struct(T, c), br, bt, advection.order)
        self._state = self._make_state()
        self._U0, self._G = self._make_prog(self.U0), self._make_prog(self.G)
        self._sub = self.timestepper.substepper.struct()
        if self._sa:
            _context.attach_saturation_adjustment(self, fld)
        if self._kessler:
            _context.attach_kessler(self, dynamics.standard_pressure)
        if self._ip:
            _context.attach_instantaneous_precipitation(self, fld)
        if self._sa or self._ip:
            _context.attach_flatau_polynomial(self)      # saturation_vapor_pressure = FlatauPolynomial() of the constants
        if coriolis is not None:      # the f-plane term of the slow momentum tendencies (bz_set_forcings with coriolis_f alone)
            Fc = T.bz_column_forcings()
            Fc.coriolis_f = coriolis.f
            self._check(lib.bz_set_forcings(self._ctx, C.byref(Fc)), "bz_set_forcings")
        _context.attach_relaxation(self, self._relaxation, "LiquidIcePotentialTemperature")
        _context.attach_field_forcing(self, self._field_forcing, "LiquidIcePotentialTemperature")
        _context.attach_closure(self, fld)      # (explicit only: the vertically implicit discretisation was refused above)
        if self._surface_fluxes:      # bulk surface fluxes: a stage adds them after its slow tendencies (bz_set_compressible_surface_fluxes)
            from .forcings import materialize_compressible_surface_fluxes
            Sf, self._surface_flux_arrays = materialize_compressible_surface_fluxes(grid, self._surface_fluxes, dynamics, c, T)
            self._check(lib.bz_set_compressible_surface_fluxes(self._ctx, C.byref(Sf)), "bz_set_compressible_surface_fluxes")
        if self.lateral_walls:      # is_active_open_bc of the four sides (acoustic_substepping.jl:1339-1361)
            bu, bv = self.boundary_conditions.get("ρu"), self.boundary_conditions.get("ρv")
            sides = [is_active_open_bc(getattr(b, k, None)) and grid.topology[d] == Bounded
                     for b, k, d in ((bu, "west", 0), (bu, "east", 0), (bv, "south", 1), (bv, "north", 1))]
            self._check(lib.bz_set_acoustic_lateral_boundaries(self._ctx, *(int(x) for x in sides), td.open_boundary_relaxation),
                        "bz_set_acoustic_lateral_boundaries")
            self._open_sides = tuple(k for k, on in zip(("west", "east", "south", "north"), sides) if on)
        # seed_pressure! (compressible_dynamics.jl:254-258)
        if ref is not None:
            Hz, Nz = grid.Hz, grid.Nz
            dynamics.pressure.set_interior(ref.pressure[Hz:Hz + Nz][:, None, None])
        else:
            dynamics.pressure.set_interior(dynamics.surface_pressure)

    def _create_context(self, lib, bg, bc, br, bt, order):
        return lib.bz_create_compressible(C.byref(self._ctx), C.byref(bg), C.byref(bc), C.byref(br), C.byref(bt), order)

    def _exchange(self, tensors):
        """y-halo exchange hook: nothing to do on a single GPU (the kernels wrap periodically)."""

    def prognostic_fields(self):
        out = {"ρᵈ": self.dynamics.dry_density, "ρu": self.momentum["ρu"], "ρv": self.momentum["ρv"],
               "ρw": self.momentum["ρw"], "ρθ": self.potential_temperature_density, "ρq": self.moisture_density}
        if getattr(self, "_kessler", False):
            out["ρqᶜˡ"], out["ρqʳ"] = self.microphysical_fields["ρqᶜˡ"], self.microphysical_fields["ρqʳ"]
        return out

    def _make_state(self):
        s = _lib.bz_compressible_state()
        d = self.dynamics
        s.rho_d, s.rho, s.p = d.dry_density.ptr(), d.total_density.ptr(), d.pressure.ptr()
        s.rho_u, s.rho_v, s.rho_w = (self.momentum[k].ptr() for k in ("ρu", "ρv", "ρw"))
        s.rho_theta, s.rho_q = self.potential_temperature_density.ptr(), self.moisture_density.ptr()
        s.u, s.v, s.w = (self.velocities[k].ptr() for k in ("u", "v", "w"))
        s.theta, s.q, s.T = self.potential_temperature.ptr(), self.specific_moisture.ptr(), self.temperature.ptr()
        return s

    @staticmethod
    def _make_prog(d):
        p = _lib.bz_compressible_prognostic()
        p.rho_d, p.rho_u, p.rho_v, p.rho_w, p.rho_theta, p.rho_q = (d[k].ptr() for k in ("ρᵈ", "ρu", "ρv", "ρw", "ρθ", "ρq"))
        return p

    def set(self, **kw):
        return set_(self, **kw)

    def time_step(self, Δt):
        return time_step_(self, Δt)

    def stage_substeps(self, Δt, β):
        n, dτ = C.c_int32(), self._T.real()
        self._check(self._lib.bz_stage_substeps(self._ctx, float(Δt), float(β), C.byref(n), C.byref(dτ)), "bz_stage_substeps")
        return n.value, dτ.value


# ---------------------------------------------------------------------------------------------------------------------
def update_state_(model, compute_tendencies=True):
    if getattr(model, "decomp", None) is not None:
        return model.update_state_slab(compute_tendencies)
    model._check(model._lib.bz_compressible_update_state(model._ctx, C.byref(model._state), C.byref(model._G),
                                                         C.byref(model._sub), 1 if compute_tendencies else 0),
                 "bz_compressible_update_state")


def compute_closure_fields_(model):
    """compute_closure_fields!(model.closure_fields, model.closure, model) (update_atmosphere_model_state.jl:218) alone; update_state_
    ends with it."""
    model._check(model._lib.bz_compressible_compute_closure_fields(model._ctx, C.byref(model._state)),
                 "bz_compressible_compute_closure_fields")


def refresh_linearization_(model):
    model._check(model._lib.bz_refresh_linearization(model._ctx, C.byref(model._state), C.byref(model._sub)),
                 "bz_refresh_linearization")


def seed_time_averaged_velocities_(model):
    model._check(model._lib.bz_seed_time_averaged_velocities(model._ctx, C.byref(model._state), C.byref(model._sub)),
                 "bz_seed_time_averaged_velocities")


def compute_slow_tendencies_(model):
    model._check(model._lib.bz_compute_slow_tendencies(model._ctx, C.byref(model._state), C.byref(model._G)),
                 "bz_compute_slow_tendencies")


def compute_flux_bc_tendencies_(model):
    """compute_flux_bc_tendencies!(model) of the compressible model (acoustic_runge_kutta_3.jl:190-193): the attached bulk surface fluxes are
    ADDED to the first level of Gρu, Gρv, Gρθ and the moisture tendency — after compute_slow_tendencies_, which overwrites the first three.
    acoustic_rk3_substep_ and time_step do this themselves, once per stage."""
    model._check(model._lib.bz_compressible_compute_flux_bc_tendencies(model._ctx, C.byref(model._state), C.byref(model._G)),
                 "bz_compressible_compute_flux_bc_tendencies")


def detach_surface_fluxes_(model):
    """bz_set_compressible_surface_fluxes(NULL): the model steps on as one built without bulk surface fluxes."""
    model._check(model._lib.bz_set_compressible_surface_fluxes(model._ctx, None), "bz_set_compressible_surface_fluxes")
    model._surface_fluxes = {}


def set_mixed_phase_equilibrium_(model, equilibrium):
    """equilibrium = MixedPhaseEquilibrium(Tᶠ, Tʰ) of the SaturationAdjustment of a built CompressibleAtmosphereModel: the density-based
    adjustment on the mixed surface (adjust_thermodynamic_state(::LiquidIceDensityState, ::SaturationAdjustment),
    src/Microphysics/saturation_adjustment.jl:241-293) through bz_set_compressible_mixed_phase_equilibrium.  The model is one built with
    SaturationAdjustment(equilibrium = WarmPhaseEquilibrium()); its `microphysics` becomes the adjustment with the given equilibrium (same
    solver) and microphysical_fields gains qⁱ (materialize_microphysical_fields(::MPSA), saturation_adjustment.jl:119), which update_state!
    and every stage epilogue diagnose from then on: call it before set!, or follow it with update_state_.  `equilibrium` a
    WarmPhaseEquilibrium (or None) returns the model to the warm phase.  What the mixed form does not run with raises NotImplementedError
    naming MixedPhaseEquilibrium before the context is touched: y-slabs, walls, bulk surface fluxes, TetensFormula constants."""
    from .microphysics import MixedPhaseEquilibrium, SaturationAdjustment, WarmPhaseEquilibrium
    current = getattr(model, "microphysics", None)
    if not isinstance(model, CompressibleAtmosphereModel):
        raise TypeError("set_mixed_phase_equilibrium_: `model` must be a CompressibleAtmosphereModel (AtmosphereModel takes the equilibrium in its constructor)")
    if not getattr(model, "_sa", False) or not isinstance(current, SaturationAdjustment):
        raise NotImplementedError("set_mixed_phase_equilibrium_: MixedPhaseEquilibrium belongs to a SaturationAdjustment, and the model was built with "
                                  f"microphysics = {type(current).__name__}; build it with SaturationAdjustment(equilibrium = WarmPhaseEquilibrium())")
    name = "bz_set_compressible_mixed_phase_equilibrium"
    if equilibrium is None or isinstance(equilibrium, WarmPhaseEquilibrium):
        model._check(getattr(model._lib, name)(model._ctx, None, None), name)
        model.microphysics = SaturationAdjustment(solver=current.solver, equilibrium=WarmPhaseEquilibrium())
        model.microphysical_fields.pop("qⁱ", None)
        return model
    if not isinstance(equilibrium, MixedPhaseEquilibrium):
        raise TypeError("set_mixed_phase_equilibrium_: `equilibrium` must be a MixedPhaseEquilibrium or a WarmPhaseEquilibrium")
    adjustment = SaturationAdjustment(solver=current.solver, equilibrium=equilibrium)
    _context.check_mixed_phase_compressible(adjustment, "set_mixed_phase_equilibrium_", model.thermodynamic_constants, model._surface_fluxes,
                                            slab=type(model) is not CompressibleAtmosphereModel, walls=model.lateral_walls)
    c, μ = model.thermodynamic_constants, model.microphysical_fields
    qi = μ["qⁱ"] if "qⁱ" in μ else Field(model.grid, _LOC["ccc"], model.device)
    mp = model._T.bz_mixed_phase_equilibrium(equilibrium.freezing_temperature, equilibrium.homogeneous_ice_nucleation_temperature,
                                             c.ice_reference_latent_heat, c.ice_heat_capacity)
    model._check(getattr(model._lib, name)(model._ctx, C.byref(mp), C.c_void_p(qi.ptr())), name)
    model.microphysical_fields = {"qᵛ": μ["qᵛ"], "qˡ": μ["qˡ"], "qⁱ": qi, "qᵉ": μ["qᵉ"]}
    model.microphysics = adjustment
    return model


def acoustic_rk3_substep_loop_(model, Δt, β):
    model._check(model._lib.bz_acoustic_substep_loop(model._ctx, C.byref(model._state), C.byref(model._U0), C.byref(model._G),
                                                     C.byref(model._sub), float(Δt), float(β)), "bz_acoustic_substep_loop")


def acoustic_rk3_substep_(model, Δt, β):
    model._check(model._lib.bz_acoustic_rk3_substep(model._ctx, C.byref(model._state), C.byref(model._U0), C.byref(model._G),
                                                    C.byref(model._sub), float(Δt), float(β)), "bz_acoustic_rk3_substep")


def store_initial_state_(model):
    for k, f in model.prognostic_fields().items():
        model.U0[k].parent.copy_(f.parent)


def _require_whole_model_on_walls(model, what):
    """What a model on lateral walls runs beyond its acoustic loop: (Periodic, Bounded, Bounded) with impenetrable south and north walls,
    WENO(order = 5), dry or vapour-carrying.  Everything else fails by name (the library's rejections say the same)."""
    if not getattr(model, "lateral_walls", False):
        return
    if model.grid.topology[0] == Bounded:
        raise NotImplementedError(f"{what}: a compressible model on a Bounded x runs the acoustic substep loop only (fill its fields directly)")
    if getattr(model, "_open_sides", ()):
        raise NotImplementedError(f"{what}: a Bounded y with an active open boundary (NormalFlowBoundaryCondition on ρv, sides "
                                  f"{', '.join(model._open_sides)}) runs the acoustic substep loop only")
    if not isinstance(model.advection, WENO):
        raise NotImplementedError(f"{what}: Centered(order = 2) is not built on a Bounded y (WENO(order = 5) is)")
    if model.advection.bounds is not None:
        raise NotImplementedError(f"{what}: bounds-preserving WENO (bounds = ...) is not built on a Bounded y")
    if model.advection.order != 5:
        raise NotImplementedError(f"{what}: WENO(order = {model.advection.order}) is not built on a Bounded y (WENO(order = 5) is)")
    if getattr(model, "_kessler", False):
        raise NotImplementedError(f"{what}: DCMIP2016KesslerMicrophysics is not built on a Bounded y")
    if getattr(model, "_sa", False):
        raise NotImplementedError(f"{what}: SaturationAdjustment is not built on a Bounded y")


def _require_balance_scope(model, what):
    """set_to_mean!, compute_reference_state and HydrostaticallyBalancedDensity: one device, (Periodic, Periodic | Flat, Bounded)."""
    if getattr(model, "lateral_walls", False):
        raise NotImplementedError(f"{what}: not implemented on a compressible model between walls (Bounded x / Bounded y)")
    if type(model) is not CompressibleAtmosphereModel:
        raise NotImplementedError(f"{what}: not implemented on y-slab (distributed) compressible models")
    # the balanced columns and the reference profiles are integrated with Rᵐ and cᵖᵐ of (qᵛ, qˡ): no ice fraction
    _context.refuse_mixed_phase(getattr(model, "microphysics", None), what, "the hydrostatic columns are integrated without qⁱ")


def specific_humidity(model):
    """specific_humidity(model) = model.microphysical_fields.qᵛ (microphysics_interface.jl:359); without microphysics the moisture is vapour."""
    return model.microphysical_fields["qᵛ"] if model.microphysics is not None else model.specific_moisture


def set_to_mean_(reference_state, model):
    """set_to_mean!(ref::ExnerReferenceState, model) (set_to_mean.jl:152-201): the reference columns again, by the constructor's integration,
    from the horizontal means of the model's θˡⁱ and qᵛ (bz_horizontal_average); the host object is updated in place, the context takes the
    new columns (bz_set_exner_reference_state) and update_state! follows.  No density is rescaled: the Exner reference is the base state of
    the perturbation form only."""
    _require_balance_scope(model, "set_to_mean!")
    if not isinstance(reference_state, ExnerReferenceState):
        raise TypeError("set_to_mean!: the compressible model carries an ExnerReferenceState")
    if reference_state is not model.dynamics.reference_state:
        raise ValueError("set_to_mean!: `reference_state` must be the model's own (model.dynamics.reference_state)")
    from .diagnostics import horizontal_average
    θ = horizontal_average(model, model.potential_temperature).astype(np.float64)
    qv = horizontal_average(model, specific_humidity(model)).astype(np.float64)
    reference_state.set_profiles_(θ, qv)
    br, model._ref_arrays = _exner_reference_struct(model._T, model.dynamics)
    model._check(model._lib.bz_set_exner_reference_state(model._ctx, C.byref(br)), "bz_set_exner_reference_state")
    update_state_(model, compute_tendencies=False)


def reset_reference_state_(model):
    """reset_reference_state!(model) (set_to_mean.jl:212-229): a no-op on a model without a reference state."""
    ref = model.dynamics.reference_state
    if ref is not None:
        set_to_mean_(ref, model)


def set_hydrostatically_balanced_density_(model, spec):
    """set_hydrostatically_balanced_density!(model, spec) (set_to_mean.jl:262-310) behind bz_set_hydrostatically_balanced_density."""
    _require_balance_scope(model, "HydrostaticallyBalancedDensity")
    p0 = model.dynamics.surface_pressure if spec.surface_pressure is None else spec.surface_pressure
    model._check(model._lib.bz_set_hydrostatically_balanced_density(model._ctx, C.byref(model._state), float(p0)),
                 "bz_set_hydrostatically_balanced_density")


def exner_columns_(model, potential_temperature, vapor_mass_fraction, surface_pressure, exner_function, pressure, density):
    """_compute_exner_reference_3d! on centre Fields of the model's grid (vapor_mass_fraction None: dry): one balanced column per (i, j)."""
    model._check(model._lib.bz_exner_columns(model._ctx, C.c_void_p(potential_temperature.ptr()),
                                             C.c_void_p(None if vapor_mass_fraction is None else vapor_mass_fraction.ptr()),
                                             float(surface_pressure), C.c_void_p(exner_function.ptr()), C.c_void_p(pressure.ptr()),
                                             C.c_void_p(density.ptr())), "bz_exner_columns")


def set_(model, compute_reference_state=False, balancer=None, **kw):
    """set!(model; ρ, θ, u, v, w, qᵗ, compute_reference_state): total density first, moisture, then establish_densities!, θ and velocities
    (set_atmosphere_model.jl:198-362; compressible_time_stepping.jl:105-150).  Walls in y: v given as a function is evaluated on the
    faces 0 … Ny-1, ρv takes the face-mean density through the no-flux halo row, and update_state! leaves exact zeros on the wall faces.
    ρ = HydrostaticallyBalancedDensity(p₀) is the reference's deferred density: a unit placeholder goes into ρᵈ, establish_densities! runs with
    neither density given, and the balanced density is computed after the closing update_state!; compute_reference_state = True recomputes
    the reference state from the horizontal means first (a no-op without one).  balancer = AdiabaticBalancer(...) | True:
    balance_adiabatically!(model, balancer) closes the call (balance.py)."""
    if balancer is not None and balancer is not False:      # refused by name before anything is set
        from .balance import require_balance_model
        require_balance_model(model, balancer, "set!(model; balancer)")
    balanced = next((v for n, v in kw.items() if _ALIASES.get(n) == "ρ" and isinstance(v, HydrostaticallyBalancedDensity)), None)
    if balanced is not None:
        _require_balance_scope(model, "HydrostaticallyBalancedDensity")
    if compute_reference_state:
        _require_balance_scope(model, "compute_reference_state")
    _require_whole_model_on_walls(model, "set!")
    d = model.dynamics
    g = model.grid
    keys = {}
    for name, value in kw.items():
        key = _ALIASES.get(name)
        if key is None and name in ("T", "ℋ", "H", "relative_humidity"):      # (set!(T | ℋ) is not built here; a mixed-phase model says why it could not be)
            _context.refuse_mixed_phase(model.microphysics, f"set!(model; {name})", "θ from T and qᵛ⁺ from ℋ are formed without qⁱ and over the liquid surface")
        if key is None:
            raise ValueError(f"Cannot set! {name} in AtmosphereModel because {name} is neither a prognostic variable, a "
                             "settable thermodynamic variable, nor a settable diagnostic variable!")
        keys[key] = value
    ρd, ρ = d.dry_density, d.total_density
    total_density_given = "ρ" in keys and balanced is None
    if "ρ" in keys:
        ρd.set_interior(1.0 if balanced is not None else keys["ρ"])
    if "q" in keys:
        model.specific_moisture.set_interior(keys["q"])
        model.moisture_density.interior.copy_(ρd.interior * model.specific_moisture.interior)
    condensate = 0.0
    if getattr(model, "_kessler", False):        # settable specific microphysical names: only ρq is set
        for key, dens in (("qcl", "ρqᶜˡ"), ("qr", "ρqʳ")):
            if key in keys:
                f = model.microphysical_fields[dens]
                f.set_interior(keys[key])
                f.interior.copy_(ρd.interior * f.interior)
        condensate = model.microphysical_fields["ρqᶜˡ"].interior + (model.microphysical_fields["ρqʳ"].interior + 0.0)
    elif "qcl" in keys or "qr" in keys:
        raise ValueError("Cannot set! qᶜˡ / qʳ: the model has no Kessler microphysics")
    if total_density_given:      # establish_densities!(total_density_given); neither given: update_state! diagnoses ρ = ρᵈ + Σρqˣ
        ρ.interior.copy_(ρd.interior)
        ρd.interior.copy_(ρ.interior - (model.moisture_density.interior + condensate))
    from .model import fill_halo_regions_
    fill_halo_regions_(model, ρd, 0)
    model._exchange([ρd.parent])
    if "θ" in keys:
        model.potential_temperature.set_interior(keys["θ"])
        model.potential_temperature_density.interior.copy_(ρd.interior * model.potential_temperature.interior)
    P = ρd.parent
    Hx, Hy, Hz, Nx, Ny, Nz = g.Hx, g.Hy, g.Hz, g.Nx, g.Ny, g.Nz
    if "u" in keys:
        model.velocities["u"].set_interior(keys["u"])
        ρx = (ρd.interior + P[Hz:Hz + Nz, Hy:Hy + Ny, Hx - 1:Hx - 1 + Nx]) / 2
        model.momentum["ρu"].interior.copy_(ρx * model.velocities["u"].interior)
    if "v" in keys:
        model.velocities["v"].set_interior(keys["v"])
        # ℑy of a Flat direction is the identity
        ρy = ρd.interior if g.topology[1] == Flat else (ρd.interior + P[Hz:Hz + Nz, Hy - 1:Hy - 1 + Ny, Hx:Hx + Nx]) / 2
        model.momentum["ρv"].interior.copy_(ρy * model.velocities["v"].interior)
    if "w" in keys:
        model.velocities["w"].set_interior(keys["w"])
        ρz = (P[Hz:Hz + Nz + 1, Hy:Hy + Ny, Hx:Hx + Nx] + P[Hz - 1:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx]) / 2
        model.momentum["ρw"].interior.copy_(ρz * model.velocities["w"].interior)
    update_state_(model, compute_tendencies=False)
    if compute_reference_state:
        reset_reference_state_(model)
    if balanced is not None:
        set_hydrostatically_balanced_density_(model, balanced)
    if balancer is not None and balancer is not False:
        from .balance import balance_adiabatically_
        balance_adiabatically_(model, balancer)


def time_step_(model, Δt, whole_step=True):
    """time_step!(model::CompressibleAcousticModel, Δt) (acoustic_runge_kutta_3.jl:264-319) without callbacks.
    whole_step=True keeps the step behind one C call; False issues the operator sequence of the reference."""
    Δt = float(Δt)
    _require_whole_model_on_walls(model, "time_step!")
    if model.clock.iteration == 0:                         # maybe_prepare_first_time_step!
        seed_time_averaged_velocities_(model)
        update_state_(model, compute_tendencies=True)
    if getattr(model, "decomp", None) is not None:
        model.time_step_slab(Δt)
    elif whole_step:
        model._check(model._lib.bz_time_step_compressible(model._ctx, C.byref(model._state), C.byref(model._U0),
                                                          C.byref(model._G), C.byref(model._sub), Δt),
                     "bz_time_step_compressible")
    else:
        store_initial_state_(model)
        refresh_linearization_(model)                      # freeze_linearization_state!
        seed_time_averaged_velocities_(model)
        for β in (model.timestepper.β1, model.timestepper.β2, model.timestepper.β3):
            acoustic_rk3_substep_(model, Δt, β)
            update_state_(model, compute_tendencies=True)
        if getattr(model, "_kessler", False):
            model._check(model._lib.bz_compressible_kessler_update(model._ctx, C.byref(model._state), C.byref(model._G),
                                                                   C.byref(model._sub), Δt), "bz_compressible_kessler_update")
        if getattr(model, "_ip", False):       # microphysics_model_update!(::InstantaneousPrecipitation, model) with Δt = this step's
            model._check(model._lib.bz_instantaneous_precipitation_update(model._ctx, C.byref(model._state), C.byref(model._G),
                                                                          C.byref(model._sub), Δt), "bz_instantaneous_precipitation_update")
    model.clock.time += Δt
    model.clock.last_Δt = Δt
    model.clock.iteration += 1


# ---------------------------------------------------------------------------------------------------------------------
# y-slab decomposition: one process per GPU, halo exchanges only — the acoustic column solve is rank-local
# ---------------------------------------------------------------------------------------------------------------------
class SlabCompressibleModel(CompressibleAtmosphereModel):
    """CompressibleAtmosphereModel on one y-slab of a (Periodic, Periodic, Bounded) global grid.  Same kernels as the
    single-GPU model; inside a stage the two perturbation fields the next substep reads across the slab edge
    ((ρθ)′ and (ρv)′) are exchanged with the ring neighbours, everything else once per stage
    (breeze.jl_amd/distributed.py: SlabDecomposition, torch.distributed; backend "nccl" = RCCL on ROCm)."""

    def __init__(self, global_grid, rank, world, dynamics, advection=None, group=None, device=None, decomp=None,
                 transport="torch", **kw):
        """transport: "torch" — exchanges issued from Python through torch.distributed (`decomp` / `group`); "rccl" or
        "local:<name>" — the library owns the communicator (csrc/bz_comm.hip) and `time_step` is one C call per step."""
        import torch
        from .distributed import LibraryComm, SlabDecomposition, attach_library_transport
        grid = _context.slab_grid(global_grid, rank, world)
        self.global_grid = G = global_grid
        self.rank, self.world = rank, world
        sft = kw.get("substep_floattype")
        if sft is not None and np.dtype(sft) == np.float32 and G.ftype == 8 and transport == "torch":
            # the library-owned step moves the Float32 rows of the working fields (csrc/bz_comm.hip: halo_exchange, half); the
            # Python-issued exchange assumes the grid's real
            raise NotImplementedError('substep_floattype = Float32 on y-slabs: transport "rccl" or "local:<name>"')
        self.decomp = None                     # set after construction: the constructor's set-up is rank-local
        self.transport = transport
        library = transport != "torch"
        self._pending_decomp = LibraryComm(self) if library else (decomp or SlabDecomposition(G.Nx, grid.Ny, G.Nz, G.Hy, rank, world, group))
        dev = device if device is not None else f"cuda:{torch.cuda.current_device()}"
        super().__init__(grid, dynamics, advection=advection, device=dev, **kw)
        if library:
            attach_library_transport(self, transport, group)
        self.decomp = self._pending_decomp
        if getattr(self.decomp, "rows", "absent") is None:      # one gather / scatter launch per direction for the halo rows
            self.decomp.rows = self._device_rows
        # second buffers of the (ρu)′, (ρv)′ ping-pong are owned here so that their halos can be exchanged (the library-owned
        # step exchanges the context's own scratch buffers)
        self._up2, self._vp2 = Field(grid, _LOC["fcc"], self.device), Field(grid, _LOC["cfc"], self.device)
        if not library:
            self._check(self._lib.bz_set_acoustic_scratch(self._ctx, C.c_void_p(self._up2.ptr()), C.c_void_p(self._vp2.ptr())),
                        "bz_set_acoustic_scratch")
        sub = self.timestepper.substepper
        self._th_buf = (sub.density_potential_temperature_perturbation.parent,
                        sub.previous_density_potential_temperature_perturbation.parent)
        self._v_buf = (sub.momentum_perturbation_v.parent, self._vp2.parent)
        self._u_buf = (sub.momentum_perturbation_u.parent, self._up2.parent)
        self._direct = isinstance(self.dynamics.time_discretization.damping, DirectDivergenceDamping)
        self._exchange([self.dynamics.pressure.parent])

    def _create_context(self, lib, bg, bc, br, bt, order):
        return lib.bz_create_compressible_slab(C.byref(self._ctx), C.byref(bg), C.byref(bc), C.byref(br), C.byref(bt), order,
                                               self.world, self.rank)

    def _exchange(self, tensors):
        d = self.decomp or self._pending_decomp
        d.exchange_y_halos(list(tensors))

    def _device_rows(self, fields, row0, nrows, buffer, unpack):
        n = len(fields)
        ptrs = (C.c_void_p * n)(*[f.data_ptr() for f in fields])
        levels = (C.c_int32 * n)(*[f.shape[0] for f in fields])
        self._check(self._lib.bz_pack_rows(self._ctx, ptrs, levels, n, int(row0), int(nrows), C.c_void_p(buffer.data_ptr()),
                                           1 if unpack else 0), "bz_pack_rows")

    # field groups ----------------------------------------------------------------------------------------------------
    def _prognostic_tensors(self):
        sub = self.timestepper.substepper
        return ([f.parent for f in self.prognostic_fields().values()] +
                [sub.time_averaged_u.parent, sub.time_averaged_v.parent, sub.time_averaged_w.parent])

    def _diagnostic_tensors(self):
        d = self.dynamics
        μ = [self.microphysical_fields[k].parent for k in ("qᵛ", "qᶜˡ", "qʳ")] if self._kessler else []
        if self._sa:       # the halo rows' linearisation reads the liquid fraction
            μ = [self.microphysical_fields[k].parent for k in ("qᵛ", "qˡ")]
        return ([d.total_density.parent, d.pressure.parent] + [self.velocities[k].parent for k in ("u", "v", "w")] +
                [self.potential_temperature.parent, self.specific_moisture.parent, self.temperature.parent] + μ)

    def update_state_slab(self, compute_tendencies=True):
        """update_state! with the neighbour exchanges of the slab decomposition.  The diagnosis needs ρᵈ of row -1 (face
        velocities); everything else is exchanged after it, when the x halos of the edge rows (written by the diagnosis
        kernel) are valid, so that the corner cells the WENO stencils touch arrive with the rows."""
        if self.transport != "torch":
            self._check(self._lib.bz_comm_compressible_update_state(self._ctx, C.byref(self._state), C.byref(self._G), C.byref(self._sub),
                                                                    1 if compute_tendencies else 0), "bz_comm_compressible_update_state")
            return
        self._exchange([self.dynamics.dry_density.parent])
        self._check(self._lib.bz_compressible_update_state(self._ctx, C.byref(self._state), C.byref(self._G), C.byref(self._sub), 0),
                    "bz_compressible_update_state")
        self._exchange(self._prognostic_tensors() + self._diagnostic_tensors())
        if compute_tendencies:
            self._check(self._lib.bz_compute_moisture_tendency(self._ctx, C.byref(self._state), C.byref(self._G), C.byref(self._sub)),
                        "bz_compute_moisture_tendency")

    def acoustic_rk3_substep_slab(self, Δt, β):
        """acoustic_rk3_substep!(model, Δt, β) on a slab (call order in include/breeze_hip.h, slab section)."""
        lib, ctx = self._lib, self._ctx
        st, U0, G, sub = C.byref(self._state), C.byref(self._U0), C.byref(self._G), C.byref(self._sub)
        refresh_linearization_(self)
        compute_slow_tendencies_(self)
        self._exchange([self.G["ρv"].parent])
        n, cur = C.c_int32(), C.c_int32()
        self._check(lib.bz_acoustic_stage_begin(ctx, st, U0, G, sub, float(Δt), float(β), C.byref(n), C.byref(cur)),
                    "bz_acoustic_stage_begin")
        for s in range(1, n.value + 1):
            self._exchange([self._th_buf[cur.value], self._v_buf[cur.value]])
            self._check(lib.bz_acoustic_substep(ctx, st, U0, G, sub, s, C.byref(cur)), "bz_acoustic_substep")
            if self._direct:      # apply_divergence_damping!(::DirectDivergenceDamping): needs the neighbours' freshly advanced rows
                self._exchange([self._u_buf[cur.value], self._v_buf[cur.value]])
                self._check(lib.bz_acoustic_direct_damping(ctx, st, U0, G, sub), "bz_acoustic_direct_damping")
        self._exchange([self._th_buf[cur.value]])
        self._check(lib.bz_acoustic_stage_end(ctx, st, U0, G, sub, float(Δt), float(β), 1), "bz_acoustic_stage_end")

    def time_step_slab(self, Δt):
        if self.transport != "torch":       # the whole distributed step behind one call (bz_comm.hip: bzi_dist_time_step_compressible)
            self._check(self._lib.bz_time_step_compressible(self._ctx, C.byref(self._state), C.byref(self._U0), C.byref(self._G),
                                                            C.byref(self._sub), float(Δt)), "bz_time_step_compressible")
            return
        store_initial_state_(self)
        for β in (self.timestepper.β1, self.timestepper.β2, self.timestepper.β3):
            self.acoustic_rk3_substep_slab(Δt, β)
            self.update_state_slab(compute_tendencies=True)
        if self._kessler:      # microphysics_model_update!: rank-local columns, then the exchanging update_state!
            self._check(self._lib.bz_compressible_kessler_update(self._ctx, C.byref(self._state), C.byref(self._G),
                                                                 C.byref(self._sub), float(Δt)), "bz_compressible_kessler_update")
            self.update_state_slab(compute_tendencies=True)
