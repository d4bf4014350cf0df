"""Host-side mirror of the forcing / Coriolis / boundary-flux interface of the BOMEX configuration (BASELINE configs[2]).

The reference assembles these from Oceananigans' `Forcing`, `FluxBoundaryCondition`, `FPlane` and Breeze's own
`SubsidenceForcing` / `geostrophic_forcings` (examples/bomex.jl:80-207).  Every one of them is a horizontally uniform
column profile (times the reference density, src/Forcings/specific_forcing.jl:61-74), so `materialize_forcings` reduces the
model's `forcing` / `coriolis` / `boundary_conditions` keywords to one `bz_column_forcings` struct for `bz_set_forcings`.
Nothing here computes on the CPU: the profiles are evaluated once at construction (as `set!` of a column Field is in the
reference) and the tendencies are HIP kernels (csrc/bz_forcing.hip).
"""
import ctypes as C
import unicodedata
from collections import namedtuple

import numpy as np

from . import _lib


class SmagorinskyLilly:
    """SmagorinskyLilly(; C = 0.16, Cb = 1.0, Pr = 1.0) (Oceananigans.TurbulenceClosures, re-exported src/Breeze.jl:186,220)."""

    def __init__(self, C=0.16, Cb=1.0, Pr=1.0):
        from .closures import ExplicitTimeDiscretization, VerticallyImplicitTimeDiscretization
        if isinstance(C, (ExplicitTimeDiscretization, VerticallyImplicitTimeDiscretization)) or C in (ExplicitTimeDiscretization, VerticallyImplicitTimeDiscretization):
            # SmagorinskyLilly(VerticallyImplicitTimeDiscretization()): Oceananigans' optional positional argument
            raise NotImplementedError("SmagorinskyLilly(time_discretization): only the explicit discretisation is implemented")
        self.C, self.Cb, self.Pr = float(C), float(Cb), float(Pr)


class FPlane:
    """FPlane(f=...) (Oceananigans.Coriolis)."""

    def __init__(self, f):
        self.f = float(f)


class SubsidenceForcing:
    """SubsidenceForcing(wˢ) (src/Forcings/subsidence_forcing.jl:14-58): wˢ a function of z or Nz+1 face values."""

    def __init__(self, subsidence_vertical_velocity):
        self.subsidence_vertical_velocity = subsidence_vertical_velocity


class GeostrophicForcing:
    """One component of geostrophic_forcings (src/Forcings/geostrophic_forcings.jl): direction "x": -f vᵍ, "y": +f uᵍ."""

    def __init__(self, geostrophic_velocity, direction):
        self.geostrophic_velocity, self.direction = geostrophic_velocity, direction


GeostrophicForcings = namedtuple("GeostrophicForcings", ("u", "v"))


def geostrophic_forcings(uᵍ, vᵍ):
    """geostrophic_forcings(uᵍ, vᵍ) -> (u = -f vᵍ, v = +f uᵍ); f comes from the model's coriolis at materialization."""
    return GeostrophicForcings(GeostrophicForcing(vᵍ, "x"), GeostrophicForcing(uᵍ, "y"))


class Forcing:
    """Forcing(profile): a column field / function of z added to the specific tendency (Oceananigans Forcing(field))."""

    def __init__(self, profile):
        self.profile = profile


class GaussianMask:
    """GaussianMask{:z}(center, width): exp(-(z - center)^2 / (2 width^2)) (Oceananigans; examples/rico.jl:104,
    examples/neutral_atmospheric_boundary_layer.jl:105)."""

    def __init__(self, center, width, direction="z"):
        if str(direction).lstrip(":") != "z":
            raise NotImplementedError("GaussianMask{:z}: sponges vary with height only")
        self.center, self.width = float(center), float(width)

    def __call__(self, z):
        return np.exp(-(z - self.center) ** 2 / (2 * self.width ** 2))


class Relaxation:
    """Relaxation(rate, mask, target): F = rate * mask(z) * (target(z) - field) (Oceananigans Relaxation; the sponge layers of
    examples/rico.jl:103-105,164, neutral_atmospheric_boundary_layer.jl:127, tropical_cyclone_world.jl).  mask: GaussianMask or a function
    of z (default 1); target: a number, a function of z or a column (default 0).  Keyed in `forcing` by a density name (ρu, ρv, ρw, ρθ / ρe,
    ρqᵉ ...: the density relaxes, as the reference's examples write it) or by u, v, w (specific forcing: ρᵣ F)."""

    def __init__(self, rate, mask=None, target=0.0):
        self.rate, self.mask, self.target = float(rate), mask, target


class FrictionVelocityDrag:
    """The example's bulk drag closure -ρ₀ u★² ρu / √(ρu² + ρv²) (examples/bomex.jl:95-99) as data."""

    def __init__(self, ρ0, ustar, epsilon=0.0):
        # epsilon: the ϵ under the square root of benchmarking/src/convective_boundary_layer.jl:142-146 (1e-10 there)
        self.ρ0, self.ustar, self.epsilon = float(ρ0), float(ustar), float(epsilon)


# default neutral polynomials (a₀, a₁, a₂) of Large & Yeager (2009) (polynomial_bulk_coefficient.jl:8-10)
default_neutral_drag_polynomial = (0.142, 0.076, 2.7)
default_neutral_sensible_heat_polynomial = (0.128, 0.068, 2.43)
default_neutral_latent_heat_polynomial = (0.120, 0.070, 2.55)


class StabilityFunctionParameters:
    """StabilityFunctionParameters(; γᴰ = 19.3, γᵀ = 11.6, a = 1, b = 2/3, c = 5, d = 0.35) (polynomial_bulk_coefficient.jl:56-64):
    Hogström (1996) unstable, Beljaars & Holtslag (1991) stable Ψ functions."""

    def __init__(self, γᴰ=19.3, γᵀ=11.6, a=1, b=2 / 3, c=5, d=0.35):
        self.γᴰ, self.γᵀ, self.a, self.b, self.c, self.d = (float(x) for x in (γᴰ, γᵀ, a, b, c, d))

    def values(self):
        return (self.γᴰ, self.γᵀ, self.a, self.b, self.c, self.d)


class RichardsonNumberMapping:
    """RichardsonNumberMapping(; ...) (polynomial_bulk_coefficient.jl:135-152): Li et al. (2010) regression coefficients of the
    Ri_B → ζ mapping with the reference's defaults; its keywords aᵘ₁₁, bʷ₂₂, ... are spelled au11, bw22, ... (subscript digits are not
    Python identifier characters)."""

    def __init__(self, stable_unstable_transition=0, strongly_stable_transition=0.2,
                 au11=0.0450, bu11=0.0030, bu12=0.0059, au21=-0.0828, au22=0.8845, bu31=0.1739, bu32=-0.9213, bu33=-0.1057,
                 aw11=0.5738, aw12=-0.4399, aw21=-4.901, aw22=52.50, bw11=-0.0539, bw12=1.540, bw21=-0.6690, bw22=-3.282,
                 as11=0.7529, as21=14.94, bs11=0.1569, bs21=-0.3091, bs22=-1.303):
        kw = dict(locals())
        kw.pop("self")
        for k, v in kw.items():
            setattr(self, k, float(v))

    def values(self):
        return tuple(getattr(self, n) for n in _lib._MAPPING_FIELDS)


class FittedStabilityFunction:
    """FittedStabilityFunction(scalar_roughness_length; richardson_number_mapping, stability_function_parameters)
    (polynomial_bulk_coefficient.jl:204-210)."""

    def __init__(self, scalar_roughness_length, richardson_number_mapping=None, stability_function_parameters=None):
        self.scalar_roughness_length = float(scalar_roughness_length)
        self.richardson_number_mapping = richardson_number_mapping or RichardsonNumberMapping()
        self.stability_function_parameters = stability_function_parameters or StabilityFunctionParameters()


_DEFAULT_STABILITY = object()


class PolynomialCoefficient:
    """PolynomialCoefficient(; polynomial = nothing, roughness_length = 1.5e-4, minimum_wind_speed = 0.1, stability_function =
    FittedStabilityFunction(roughness_length / 7.3), surface = PlanarLiquidSurface()) (polynomial_bulk_coefficient.jl:466-481).
    polynomial=None: the condition it is attached to picks its Large & Yeager polynomial; stability_function=None: no correction."""

    def __init__(self, polynomial=None, roughness_length=1.5e-4, minimum_wind_speed=0.1, stability_function=_DEFAULT_STABILITY,
                 surface=None, transfer_type=None):
        if surface is not None and str(surface) not in ("PlanarLiquidSurface", "PlanarLiquidSurface()"):
            raise NotImplementedError("PolynomialCoefficient: surface = PlanarLiquidSurface() is implemented")
        self.polynomial = None if polynomial is None else tuple(float(a) for a in polynomial)
        if self.polynomial is not None and len(self.polynomial) != 3:
            raise ValueError("polynomial = (a₀, a₁, a₂)")
        self.roughness_length, self.minimum_wind_speed = float(roughness_length), float(minimum_wind_speed)
        if stability_function is _DEFAULT_STABILITY:
            stability_function = FittedStabilityFunction(self.roughness_length / 7.3)
        if stability_function is not None and not isinstance(stability_function, FittedStabilityFunction):
            raise NotImplementedError("stability_function: FittedStabilityFunction or None")
        self.stability_function, self.transfer_type = stability_function, transfer_type


class FilteredSurfaceVelocities:
    """FilteredSurfaceVelocities(grid; height = nothing, filter_timescale = Inf) (filtered_surface_state.jl:66-73): exponentially
    time-filtered û, v̂, θ̂ᵥ (and, per condition, θ̂ / q̂) of the first level; the 2-D fields live in the library's context
    (model.filtered_surface_field(name) / model.set_filtered_surface_field(name, array)).  update_stages: after which stages'
    update_state! of a whole step the filter advances with ε = Δt / τ.  The default (1, 3) is a READING of the reference's
    (clock.iteration, clock.stage) key (its second stage does not tick the clock, ssp_runge_kutta_3.jl:249); a host that knows its
    clock passes what the clock says."""

    def __init__(self, grid=None, height=None, filter_timescale=float("inf"), update_stages=(1, 3)):
        self.grid, self.height, self.filter_timescale = grid, height, float(filter_timescale)
        self.update_stages = tuple(int(s) for s in update_stages)
        if any(s not in (1, 2, 3) for s in self.update_stages):
            raise ValueError("update_stages names stages 1, 2, 3")

    @property
    def stage_mask(self):
        return sum(1 << (s - 1) for s in set(self.update_stages))


def _coefficient(c):
    # (a function-valued coefficient — user code like the WindDependentDrag of validation/DCMIP2016_TC/dcmip2016_tc.jl — is kept as given: the
    # model constructors refuse it by name)
    return c if isinstance(c, PolynomialCoefficient) or callable(c) else float(c)


def _surface_temperature(T0):
    return T0 if (T0 is None or callable(T0) or np.ndim(T0) > 0) else float(T0)


class BulkDrag:
    """BulkDrag(; coefficient = 1e-3, gustiness = 0, surface_temperature = nothing, filtered_velocities = nothing)
    (src/BoundaryConditions/bulk_drag.jl:60-84); without a surface temperature the anelastic default Π₀ θ₀ of the reference state is
    used (src/AnelasticEquations/anelastic_dynamics.jl:99-105).  coefficient: a number or a PolynomialCoefficient;
    surface_temperature: a number, an (Ny, Nx) array or T₀(x) / T₀(x, y) evaluated at the cell centres."""
    default_polynomial, transfer_type = default_neutral_drag_polynomial, "momentum"

    def __init__(self, coefficient=1e-3, gustiness=0.0, surface_temperature=None, filtered_velocities=None):
        if isinstance(coefficient, PolynomialCoefficient) and surface_temperature is None:      # bulk_drag.jl:78-80
            raise ValueError("surface_temperature keyword argument must be provided when configuring BulkDrag with a PolynomialCoefficient")
        self.coefficient, self.gustiness = _coefficient(coefficient), float(gustiness)
        self.surface_temperature, self.filtered_velocities = _surface_temperature(surface_temperature), filtered_velocities


class BulkSensibleHeatFlux:
    """BulkSensibleHeatFlux(; coefficient, gustiness = 0, surface_temperature, filtered_velocities = nothing) (bulk_scalar_fluxes.jl:53-56)."""
    default_polynomial, transfer_type = default_neutral_sensible_heat_polynomial, "scalar"

    def __init__(self, coefficient, surface_temperature, gustiness=0.0, filtered_velocities=None):
        self.coefficient, self.gustiness = _coefficient(coefficient), float(gustiness)
        self.surface_temperature, self.filtered_velocities = _surface_temperature(surface_temperature), filtered_velocities


class BulkVaporFlux:
    """BulkVaporFlux(; coefficient, gustiness = 0, surface_temperature, filtered_velocities = nothing) (bulk_scalar_fluxes.jl:172-176)."""
    default_polynomial, transfer_type = default_neutral_latent_heat_polynomial, "scalar"

    def __init__(self, coefficient, surface_temperature, gustiness=0.0, filtered_velocities=None):
        self.coefficient, self.gustiness = _coefficient(coefficient), float(gustiness)
        self.surface_temperature, self.filtered_velocities = _surface_temperature(surface_temperature), filtered_velocities


class FluxBoundaryCondition:
    def __init__(self, condition):
        self.condition = condition


class FieldBoundaryConditions:
    def __init__(self, bottom=None, top=None, west=None, east=None, south=None, north=None):
        """bottom: the surface flux conditions of the anelastic model; west / east / south / north: NormalFlowBoundaryCondition on the
        wall-normal momentum of a compressible model with a Bounded x / y (the open lateral boundaries of the acoustic substep loop)."""
        if top is not None:
            raise NotImplementedError("only bottom flux boundary conditions are implemented (bulk surface fluxes and the constant fluxes are "
                                      "bottom conditions; a top flux condition is not built)")
        self.bottom = bottom
        self.west, self.east, self.south, self.north = west, east, south, north


def _key(name):
    return unicodedata.normalize("NFKC", str(name))


def _profile(value, z):
    if callable(value):
        return np.ascontiguousarray([float(value(zk)) for zk in z], dtype=np.float64)
    a = np.ascontiguousarray(value, dtype=np.float64)
    if a.shape != z.shape:
        raise ValueError(f"profile has shape {a.shape}, expected {z.shape}")
    return a


_RELAX_SLOTS = {"ρu": ("u", 0), "ρv": ("v", 0), "ρw": ("w", 0), "ρθ": ("theta", 0), "ρe": ("theta", 0), "ρqe": ("moisture", 0),
                "ρqv": ("moisture", 0), "ρqt": ("moisture", 0), "ρq": ("moisture", 0), "u": ("u", 1), "v": ("v", 2), "w": ("w", 4)}


def _is_field_forcing(item):
    """Forcing(f(x, y, z)) or Forcing(3-D array): a forcing that varies in the horizontal (the column stack takes functions of z)."""
    if not isinstance(item, Forcing):
        return False
    f = item.profile
    if callable(f):
        import inspect
        try:
            nargs = len(inspect.signature(f).parameters)
        except (TypeError, ValueError):
            return False
        if nargs == 4:      # Forcing(f(x, y, z, t)): nothing here re-evaluates a forcing field as the clock advances
            raise NotImplementedError("Forcing(f(x, y, z, t)): time-dependent 3-D forcings are not implemented — pass f(x, y, z) "
                                      "(evaluated once) or a 3-D array and refresh it yourself between steps")
        return nargs == 3
    return np.ndim(f) == 3


def split_relaxation(forcing):
    """-> (forcing without the entries below, {key: Relaxation}, {key: Forcing}): sponges go to bz_set_relaxation, 3-D forcings of the
    thermodynamic variable to bz_set_field_forcing, the rest to the column-forcing stack."""
    rest, relax, field = {}, {}, {}
    for name, entry in (forcing or {}).items():
        items = entry if isinstance(entry, (tuple, list)) else (entry,)
        keep = tuple(it for it in items if not isinstance(it, Relaxation) and not _is_field_forcing(it))
        mine = [it for it in items if isinstance(it, Relaxation)]
        fields = [it for it in items if _is_field_forcing(it)]
        if len(mine) > 1 or len(fields) > 1:
            raise NotImplementedError(f"one Relaxation and one 3-D Forcing per field ({name!r})")
        if mine:
            relax[_key(name)] = mine[0]
        if fields:
            if _key(name) not in ("θ", "ρθ", "e", "ρe"):
                raise NotImplementedError(f"3-D Forcing on {name!r}: the thermodynamic variable (θ / e, or ρθ / ρe) is implemented")
            if field:
                raise NotImplementedError("one 3-D Forcing of the thermodynamic variable")
            field[_key(name)] = fields[0]
        if keep:
            rest[name] = keep if len(keep) > 1 else keep[0]
    return (rest or None), relax, field


def materialize_field_forcing(grid, field, formulation, device):
    """{key: Forcing} -> (device Field holding F at the cell centres, specific flag) or (None, 0)."""
    if not field:
        return None, 0
    from .model import _LOC, Field
    (k, item), = field.items()
    if (k in ("e", "ρe")) != (formulation == "StaticEnergy"):
        raise ValueError(f"3-D Forcing on {k!r}: the thermodynamic variable of this formulation is {'e' if formulation == 'StaticEnergy' else 'θ'}")
    F = Field(grid, _LOC["ccc"], device)
    F.set_interior(item.profile)
    return F, 0 if k.startswith("ρ") else 1


def materialize_relaxation(grid, relax, formulation, T=None):
    """{key: Relaxation} -> (bz_column_relaxation, keepalive arrays) or (None, None)."""
    T = T or _lib.types(8)
    if not relax:
        return None, None
    zc, zf = np.asarray(grid.zᶜ, dtype=np.float64), np.asarray(grid.zᶠ, dtype=np.float64)
    S, keep, seen = T.bz_column_relaxation(), [], set()
    for k, r in relax.items():
        if k not in _RELAX_SLOTS:
            raise NotImplementedError(f"Relaxation on {k!r} is not implemented (ρu, ρv, ρw, ρθ / ρe, the moisture density; u, v, w)")
        if (k == "ρe") != (formulation == "StaticEnergy") and k in ("ρe", "ρθ"):
            raise ValueError(f"Relaxation on {k!r}: the thermodynamic density of this formulation is {'ρe' if formulation == 'StaticEnergy' else 'ρθ'}")
        slot, bit = _RELAX_SLOTS[k]
        if slot in seen:
            raise NotImplementedError(f"one Relaxation per field ({slot})")
        seen.add(slot)
        z = zf if slot == "w" else zc
        mask = np.ones_like(z) if r.mask is None else np.asarray([float(r.mask(zk)) for zk in z])
        rate = np.ascontiguousarray(r.rate * mask, dtype=T.np_real)
        target = np.ascontiguousarray(np.full_like(z, float(r.target)) if np.isscalar(r.target) else _profile(r.target, z), dtype=T.np_real)
        keep += [rate, target]
        setattr(S, "rate_" + slot, rate.ctypes.data_as(C.POINTER(T.real)))
        setattr(S, "target_" + slot, target.ctypes.data_as(C.POINTER(T.real)))
        S.specific_mask |= bit
    return S, keep


def materialize_forcings(grid, coriolis, forcing, boundary_conditions, T=None):
    """-> (bz_column_forcings, keepalive arrays) or (None, None) when nothing is attached.  T: _lib.types(grid.ftype) — the struct
    classes and scalar type of the grid's precision (profiles are evaluated in Float64 and stored in eltype(grid))."""
    T = T or _lib.types(8)
    if coriolis is None and not forcing and not boundary_conditions:
        return None, None
    if coriolis is not None and not isinstance(coriolis, FPlane):
        raise NotImplementedError("coriolis: FPlane is implemented")
    f = coriolis.f if coriolis is not None else 0.0
    zc, zf = np.asarray(grid.zᶜ, dtype=np.float64), np.asarray(grid.zᶠ, dtype=np.float64)
    slots = {"u": "u_forcing", "v": "v_forcing", "θ": "theta_forcing", "qe": "moisture_forcing", "qv": "moisture_forcing",
             "qt": "moisture_forcing", "e": "energy_forcing"}
    sub_flags = {"u": "subsidence_u", "v": "subsidence_v", "θ": "subsidence_theta", "qe": "subsidence_moisture",
                 "qv": "subsidence_moisture", "qt": "subsidence_moisture"}
    static, keep = {}, []
    S = T.bz_column_forcings()
    ws = None
    for name, entry in (forcing or {}).items():
        k = _key(name)
        if k.startswith("ρ"):
            raise ValueError("forcings are specific tendencies and must be supplied under the specific prognostic name "
                             "(e.g. `θ` instead of `ρθ`); the density factor is applied automatically")
        if k not in slots:
            raise NotImplementedError(f"forcing on {name!r} is not implemented")
        for item in (entry if isinstance(entry, (tuple, list)) else (entry,)):
            if isinstance(item, SubsidenceForcing):
                if k not in sub_flags:
                    raise NotImplementedError(f"SubsidenceForcing on {name!r} is not implemented")
                w = _profile(item.subsidence_vertical_velocity, zf)
                if ws is not None and not np.array_equal(ws, w):
                    raise NotImplementedError("one subsidence velocity profile per model")
                ws = w
                setattr(S, sub_flags[k], 1)
            elif isinstance(item, GeostrophicForcing):
                if coriolis is None:
                    raise ValueError("geostrophic forcings need the model's coriolis")
                if (item.direction, k) not in (("x", "u"), ("y", "v")):
                    raise ValueError("geostrophic.u belongs under `u`, geostrophic.v under `v`")
                prof = _profile(item.geostrophic_velocity, zc)
                prof = -f * prof if item.direction == "x" else f * prof
                static[slots[k]] = static.get(slots[k], 0.0) + prof
            elif isinstance(item, Forcing) or callable(item):
                prof = _profile(item.profile if isinstance(item, Forcing) else item, zc)
                static[slots[k]] = static.get(slots[k], 0.0) + prof
            else:
                raise NotImplementedError(f"forcing {item!r} is not implemented")
    for slot, prof in static.items():
        a = np.ascontiguousarray(prof, dtype=T.np_real)
        keep.append(a)
        setattr(S, slot, a.ctypes.data_as(C.POINTER(T.real)))
    if ws is not None:
        ws = np.ascontiguousarray(ws, dtype=T.np_real)
        keep.append(ws)
        S.subsidence_vertical_velocity = ws.ctypes.data_as(C.POINTER(T.real))
    S.coriolis_f = f
    drag = None
    for name, bcs in (boundary_conditions or {}).items():
        k = _key(name)
        bottom = bcs.bottom if isinstance(bcs, FieldBoundaryConditions) else bcs
        if bottom is None:
            continue
        cond = bottom.condition if isinstance(bottom, FluxBoundaryCondition) else bottom
        if isinstance(cond, (BulkDrag, BulkSensibleHeatFlux, BulkVaporFlux)):
            continue                      # collected by materialize_bulk_fluxes
        if k == "ρe":      # an energy flux keyed ρe in a potential-temperature model: Q / cᵖᵐ enters ρθ (BoundaryConditions.jl:218-227)
            if S.bottom_theta_flux:
                raise ValueError("Cannot specify boundary conditions on both ρθ and ρe")
            S.bottom_energy_flux = float(cond)
        elif k == "ρθ":
            if S.bottom_energy_flux:
                raise ValueError("Cannot specify boundary conditions on both ρθ and ρe")
            S.bottom_theta_flux = float(cond)
        elif k in ("ρqe", "ρqv", "ρqt"):
            S.bottom_moisture_flux = float(cond)
        elif k in ("ρu", "ρv"):
            if not isinstance(cond, FrictionVelocityDrag):
                raise NotImplementedError("momentum bottom flux: FrictionVelocityDrag(ρ₀, u★)")
            d = (cond.ρ0 * cond.ustar ** 2, cond.epsilon)
            if drag is not None and drag != d:
                raise NotImplementedError("ρu and ρv share one drag")
            drag = d
        else:
            raise NotImplementedError(f"boundary condition on {name!r} is not implemented")
    S.bottom_drag_rho0_ustar2, S.bottom_drag_epsilon = drag or (0.0, 0.0)
    if not static and ws is None and f == 0.0 and not (S.bottom_theta_flux or S.bottom_moisture_flux or S.bottom_drag_rho0_ustar2 or
                                                          S.bottom_energy_flux):
        return None, None                 # e.g. only bulk conditions were given
    return S, keep


def materialize_bulk_fluxes(boundary_conditions, reference_state, constants, T=None):
    """-> bz_bulk_surface_fluxes or None.  BulkDrag belongs on ρu / ρv (one coefficient for both), BulkSensibleHeatFlux on ρθ,
    BulkVaporFlux on the moisture density; anything else raises like the reference's regularization does."""
    if needs_surface_layer(boundary_conditions):
        return None                       # materialize_surface_layer
    B, found, drag = (T or _lib.types(8)).bz_bulk_surface_fluxes(), False, None
    for name, bcs in (boundary_conditions or {}).items():
        k = _key(name)
        bottom = bcs.bottom if isinstance(bcs, FieldBoundaryConditions) else bcs
        cond = bottom.condition if isinstance(bottom, FluxBoundaryCondition) else bottom
        if isinstance(cond, BulkDrag):
            if k not in ("ρu", "ρv"):
                raise ValueError("BulkDrag is a momentum boundary condition (ρu, ρv)")
            T0 = cond.surface_temperature
            if T0 is None:      # default_drag_surface_temperature(::AnelasticDynamics)
                from .thermodynamics import dry_air_gas_constant
                Π0 = (reference_state.surface_pressure / reference_state.standard_pressure) ** (
                    dry_air_gas_constant(constants) / constants.dry_air_heat_capacity)
                T0 = Π0 * reference_state.potential_temperature
            new = (cond.coefficient, cond.gustiness, float(T0))
            if drag is not None and drag != new:      # compared as given (the Float32 struct rounds what it stores)
                raise NotImplementedError("ρu and ρv share one BulkDrag")
            drag = new
            B.drag_coefficient, B.drag_gustiness, B.drag_surface_temperature = new
            found = True
        elif isinstance(cond, BulkSensibleHeatFlux):
            # keyed ρe in a potential-temperature model (examples/tropical_cyclone_world.jl:109-115) the condition is moved to ρθ with the
            # potential-temperature difference, unchanged (BoundaryConditions.jl:218-227, thermodynamic_variable_bcs.jl:283); bulk fluxes
            # are built for that formulation only (the model constructor says so for StaticEnergy)
            if k not in ("ρθ", "ρe"):
                raise ValueError("BulkSensibleHeatFlux belongs on ρθ (or ρe)")
            if B.heat_coefficient:
                raise ValueError("Cannot specify boundary conditions on both ρθ and ρe")
            B.heat_coefficient, B.heat_gustiness, B.heat_surface_temperature = cond.coefficient, cond.gustiness, cond.surface_temperature
            found = True
        elif isinstance(cond, BulkVaporFlux):
            if k not in ("ρqe", "ρqv", "ρqt"):
                raise ValueError("BulkVaporFlux belongs on the moisture density")
            B.vapor_coefficient, B.vapor_gustiness, B.vapor_surface_temperature = cond.coefficient, cond.gustiness, cond.surface_temperature
            found = True
    if not found:
        return None
    B.surface_pressure, B.standard_pressure = reference_state.surface_pressure, reference_state.standard_pressure
    c = constants
    B.liquid_latent_heat, B.liquid_heat_capacity = c.liquid_reference_latent_heat, c.liquid_heat_capacity
    B.energy_reference_temperature = c.energy_reference_temperature
    B.triple_point_temperature, B.triple_point_pressure = c.triple_point_temperature, c.triple_point_pressure
    return B


# ---- PolynomialCoefficient / FilteredSurfaceVelocities / T₀(x, y): bz_set_surface_layer -------------------------------------------------
def _bulk_conditions(boundary_conditions):
    for name, bcs in (boundary_conditions or {}).items():
        bottom = bcs.bottom if isinstance(bcs, FieldBoundaryConditions) else bcs
        cond = bottom.condition if isinstance(bottom, FluxBoundaryCondition) else bottom
        if isinstance(cond, (BulkDrag, BulkSensibleHeatFlux, BulkVaporFlux)):
            yield _key(name), cond


def needs_surface_layer(boundary_conditions):
    """True when a bulk condition carries what the constant-coefficient entry point cannot: a PolynomialCoefficient, a surface
    temperature that varies in the horizontal, or FilteredSurfaceVelocities."""
    return any(isinstance(c.coefficient, PolynomialCoefficient) or c.filtered_velocities is not None or
               callable(c.surface_temperature) or np.ndim(c.surface_temperature) > 0 for _, c in _bulk_conditions(boundary_conditions))


def surface_temperature_field(grid, T0):
    """A callable T₀(x) / T₀(x, y) evaluated at the cell centres, or an (Ny, Nx) array -> (Ny, Nx) Float64 array
    (materialize_surface_field: the reference sets a Center, Center, Nothing field from the function)."""
    if callable(T0):
        import inspect
        nargs = len(inspect.signature(T0).parameters)
        x, y = np.asarray(grid.xᶜ, dtype=np.float64)[None, :], np.asarray(grid.yᶜ, dtype=np.float64)[:, None]
        if nargs == 1:
            one = grid.xᶜ if grid.Nx > 1 or grid.Ny == 1 else grid.yᶜ
            v = np.array([float(T0(a)) for a in one], dtype=np.float64)
            a = np.broadcast_to(v[None, :] if one is grid.xᶜ else v[:, None], (grid.Ny, grid.Nx))
        elif nargs == 2:
            a = np.array([[float(T0(float(xi), float(yj))) for xi in x[0]] for yj in y[:, 0]], dtype=np.float64)
        else:
            raise ValueError("surface_temperature: T₀(x) or T₀(x, y)")
    else:
        a = np.asarray(T0, dtype=np.float64)
    if a.shape != (grid.Ny, grid.Nx):
        raise ValueError(f"surface_temperature has shape {a.shape}, expected {(grid.Ny, grid.Nx)}")
    return np.ascontiguousarray(a, dtype=np.float64)


def fill_polynomial_record(P, coef, cond):
    """bz_polynomial_coefficient from a PolynomialCoefficient attached to `cond` (defaults chosen by the condition's type:
    fill_polynomial, polynomial_bulk_coefficient.jl:714-721)."""
    P.a0, P.a1, P.a2 = coef.polynomial if coef.polynomial is not None else cond.default_polynomial
    P.roughness_length, P.minimum_wind_speed = coef.roughness_length, coef.minimum_wind_speed
    sf = coef.stability_function
    P.stability = 0 if sf is None else 1
    sf = sf or FittedStabilityFunction(coef.roughness_length / 7.3)      # (unused numbers of a switched-off correction)
    P.scalar_roughness_length = sf.scalar_roughness_length
    for n, v in zip(_lib._MAPPING_FIELDS, sf.richardson_number_mapping.values()):
        setattr(P, n, v)
    for n, v in zip(_lib._PSI_FIELDS, sf.stability_function_parameters.values()):
        setattr(P, n, v)
    return P


def materialize_surface_layer(grid, boundary_conditions, reference_state, constants, T=None):
    """-> (bz_surface_layer, keepalive arrays, FilteredSurfaceVelocities or None), or (None, None, None) when the constant-coefficient
    entry point serves every bulk condition.  Keys as materialize_bulk_fluxes: BulkDrag on ρu / ρv (one for both), BulkSensibleHeatFlux
    on ρθ / ρe, BulkVaporFlux on the moisture density."""
    if not needs_surface_layer(boundary_conditions):
        return None, None, None
    T = T or _lib.types(8)
    L, keep, fv, seen = T.bz_surface_layer(), [], [], {}
    for k, cond in _bulk_conditions(boundary_conditions):
        if isinstance(cond, BulkDrag):
            if k not in ("ρu", "ρv"):
                raise ValueError("BulkDrag is a momentum boundary condition (ρu, ρv)")
            slot = "drag"
        elif isinstance(cond, BulkSensibleHeatFlux):
            if k not in ("ρθ", "ρe"):
                raise ValueError("BulkSensibleHeatFlux belongs on ρθ (or ρe)")
            slot = "heat"
        else:
            if k not in ("ρqe", "ρqv", "ρqt"):
                raise ValueError("BulkVaporFlux belongs on the moisture density")
            slot = "vapor"
        if slot in seen:
            if slot == "drag" and _same_condition(seen[slot], cond):
                continue
            raise NotImplementedError("ρu and ρv share one BulkDrag" if slot == "drag" else "Cannot specify boundary conditions on both ρθ and ρe")
        seen[slot] = cond
        F = getattr(L, slot)
        F.enabled, F.gustiness = 1, cond.gustiness
        if isinstance(cond.coefficient, PolynomialCoefficient):
            F.polynomial = 1
            fill_polynomial_record(F.poly, cond.coefficient, cond)
        else:
            F.polynomial, F.coefficient = 0, cond.coefficient
        T0 = cond.surface_temperature
        if T0 is None:      # default_drag_surface_temperature(::AnelasticDynamics)
            from .thermodynamics import dry_air_gas_constant
            T0 = (reference_state.surface_pressure / reference_state.standard_pressure) ** (
                dry_air_gas_constant(constants) / constants.dry_air_heat_capacity) * reference_state.potential_temperature
        if callable(T0) or np.ndim(T0) > 0:
            a = np.ascontiguousarray(surface_temperature_field(grid, T0), dtype=T.np_real)
            keep.append(a)
            F.surface_temperature_field = a.ctypes.data_as(C.POINTER(T.real))
            F.surface_temperature = float(a.flat[0])
        else:
            F.surface_temperature = float(T0)
        if cond.filtered_velocities is not None:
            fv.append(cond.filtered_velocities)
    if fv and (len(fv) != len(seen) or any(f is not fv[0] for f in fv)):
        raise NotImplementedError("FilteredSurfaceVelocities: one filtered state shared by every bulk condition of the model")
    L.surface_pressure, L.standard_pressure = reference_state.surface_pressure, reference_state.standard_pressure
    c = constants
    L.liquid_latent_heat, L.liquid_heat_capacity = c.liquid_reference_latent_heat, c.liquid_heat_capacity
    L.energy_reference_temperature = c.energy_reference_temperature
    L.triple_point_temperature, L.triple_point_pressure = c.triple_point_temperature, c.triple_point_pressure
    if fv:
        f = fv[0]
        L.filtered, L.filter_timescale, L.filter_stage_mask = 1, f.filter_timescale, f.stage_mask
        if f.height is not None:
            L.filter_height_set, L.filter_height = 1, float(f.height)
    return L, keep, (fv[0] if fv else None)


def _same_condition(a, b):
    """ρu and ρv carry one BulkDrag (the example assigns the same object to both)."""
    if a is b:
        return True
    Ta, Tb = a.surface_temperature, b.surface_temperature
    same_T0 = Ta is Tb or (not callable(Ta) and not callable(Tb) and np.array_equal(Ta, Tb))
    same_C = a.coefficient is b.coefficient or (not isinstance(a.coefficient, PolynomialCoefficient) and a.coefficient == b.coefficient)
    return bool(same_T0 and same_C and a.gustiness == b.gustiness and a.filtered_velocities is b.filtered_velocities)


# ---- bulk surface fluxes on CompressibleDynamics: bz_set_compressible_surface_fluxes -------------------------------------------------------
_LATERAL_PINNED = "boundary_conditions: the open lateral boundaries of the acoustic substep loop on a Bounded x / y"


def compressible_surface_flux_conditions(boundary_conditions, grid, single_device, lateral_walls):
    """The `boundary_conditions` keyword of CompressibleAtmosphereModel, checked without a GPU -> {"drag" | "heat" | "vapor": condition}
    (empty: nothing but the open lateral conditions of a walled model).  Bottom conditions of the three bulk types with a numeric
    coefficient run on the single-device model that is periodic in x and y; everything else fails by name ("bulk surface fluxes").
    Keys as materialize_bulk_fluxes: BulkDrag on ρu / ρv (one for both), BulkSensibleHeatFlux on ρθ — or ρe, moved to ρθ with the
    potential-temperature difference (BoundaryConditions.jl:218-227) — and BulkVaporFlux on the moisture density."""
    from .compressible import NormalFlowBoundaryCondition
    from .grids import Flat
    entries = [(_key(name), bcs) for name, bcs in (boundary_conditions or {}).items()]
    laterals = [side for _, bcs in entries if isinstance(bcs, FieldBoundaryConditions)
                for side in (bcs.west, bcs.east, bcs.south, bcs.north) if side is not None]
    if not lateral_walls:
        if any(isinstance(side, NormalFlowBoundaryCondition) for side in laterals):
            raise NotImplementedError(_LATERAL_PINNED)
        if laterals:
            raise NotImplementedError("boundary_conditions: bulk surface fluxes are bottom conditions; a lateral flux condition is not implemented")
    seen = {}
    for k, bcs in entries:
        bottom = bcs.bottom if isinstance(bcs, FieldBoundaryConditions) else bcs
        if bottom is None:
            continue
        cond = bottom.condition if isinstance(bottom, FluxBoundaryCondition) else bottom
        if not isinstance(cond, (BulkDrag, BulkSensibleHeatFlux, BulkVaporFlux)):
            raise NotImplementedError(f"boundary_conditions[{k!r}]: CompressibleDynamics carries bulk surface fluxes (BulkDrag, BulkSensibleHeatFlux, "
                                      f"BulkVaporFlux) at the bottom; a plain FluxBoundaryCondition ({type(cond).__name__}) is not implemented")
        what = type(cond).__name__
        if isinstance(cond.coefficient, PolynomialCoefficient):
            raise NotImplementedError(f"{what}(coefficient = PolynomialCoefficient): bulk surface fluxes on CompressibleDynamics take a numeric coefficient")
        if callable(cond.coefficient):
            raise NotImplementedError(f"{what}: a function-valued coefficient is user code; bulk surface fluxes on CompressibleDynamics take a "
                                      "numeric coefficient")
        if cond.filtered_velocities is not None:
            raise NotImplementedError(f"{what}(filtered_velocities = FilteredSurfaceVelocities): bulk surface fluxes on CompressibleDynamics read "
                                      "the unfiltered first-level fields")
        if isinstance(cond, BulkDrag):
            if k not in ("ρu", "ρv"):
                raise ValueError("BulkDrag is a momentum boundary condition (ρu, ρv)")
            slot = "drag"
        elif isinstance(cond, BulkSensibleHeatFlux):
            if k not in ("ρθ", "ρe"):
                raise ValueError("BulkSensibleHeatFlux belongs on ρθ (or ρe)")
            slot = "heat"
        else:
            if k not in ("ρqe", "ρqv", "ρqt"):
                raise ValueError("BulkVaporFlux belongs on the moisture density")
            slot = "vapor"
        if slot in seen:
            if slot == "drag" and _same_condition(seen[slot], cond):
                continue
            if slot == "heat":      # validate_thermodynamic_bcs (BoundaryConditions.jl:200-209)
                raise ValueError("Cannot specify boundary conditions on both ρθ and ρe")
            raise NotImplementedError("ρu and ρv share one BulkDrag" if slot == "drag" else "one BulkVaporFlux per model")
        seen[slot] = cond
    if not seen:
        return seen
    if lateral_walls:
        raise NotImplementedError("boundary_conditions: bulk surface fluxes are not implemented on a compressible model between walls (Bounded x / Bounded y)")
    if Flat in grid.topology:
        raise NotImplementedError("boundary_conditions: bulk surface fluxes are not implemented on a compressible model with a Flat y")
    if not single_device:
        raise NotImplementedError("boundary_conditions: bulk surface fluxes are not implemented on y-slab (distributed) compressible models")
    if "drag" in seen and seen["drag"].surface_temperature is None:
        # default_drag_surface_temperature(::CompressibleDynamics, ...) (compressible_dynamics.jl:520-525) has no profile to draw from: it throws
        raise ValueError("BulkDrag under CompressibleDynamics requires `surface_temperature` to be provided explicitly: there is no default "
                         "surface temperature for compressible dynamics (no reference profile to draw from)")
    for cond in seen.values():
        T0 = cond.surface_temperature
        if not callable(T0) and np.ndim(T0) > 0 and np.shape(T0) != (grid.Ny, grid.Nx):
            raise ValueError(f"surface_temperature has shape {np.shape(T0)}, expected {(grid.Ny, grid.Nx)}")
    return seen


def materialize_compressible_surface_fluxes(grid, conditions, dynamics, constants, T=None):
    """{"drag" | "heat" | "vapor": condition} (compressible_surface_flux_conditions) -> (bz_compressible_surface_fluxes, keepalive arrays).
    p₀ is the dynamics' surface_pressure; the surface temperature is a number, an (Ny, Nx) array or T₀(x) / T₀(x, y)."""
    T = T or _lib.types(8)
    S, keep = T.bz_compressible_surface_fluxes(), []
    for slot, cond in conditions.items():
        F = getattr(S, slot)
        F.enabled, F.coefficient, F.gustiness = 1, cond.coefficient, cond.gustiness
        T0 = cond.surface_temperature
        if callable(T0) or np.ndim(T0) > 0:
            a = np.ascontiguousarray(surface_temperature_field(grid, T0), dtype=T.np_real)
            keep.append(a)
            F.surface_temperature_field = a.ctypes.data_as(C.POINTER(T.real))
            F.surface_temperature = float(a.flat[0])
        else:
            F.surface_temperature = float(T0)
    S.surface_pressure, S.standard_pressure = dynamics.surface_pressure, dynamics.standard_pressure
    c = constants
    S.liquid_latent_heat, S.liquid_heat_capacity = c.liquid_reference_latent_heat, c.liquid_heat_capacity
    S.energy_reference_temperature = c.energy_reference_temperature
    S.triple_point_temperature, S.triple_point_pressure = c.triple_point_temperature, c.triple_point_pressure
    return S, keep
