"""Host-side mirror of Breeze's AtmosphereModel API for the anelastic hot path.

Julia is not available in the build image, so this module plays the role of the Julia host code
above the C ABI (include/breeze_hip.h): same names, argument meaning and call order as
  AtmosphereModel(grid; dynamics, advection, ...)   src/AtmosphereModels/atmosphere_model.jl:114-314
  set!(model; θ=..., u=..., ...)                    src/AtmosphereModels/set_atmosphere_model.jl:198-362
  update_state!(model; compute_tendencies)          src/AtmosphereModels/update_atmosphere_model_state.jl:41-68
  time_step!(model, Δt)                             src/TimeSteppers/ssp_runge_kutta_3.jl:209-278
(paths relative to /root/reference).  Julia's `f!` is spelled `f_` here.

All field memory lives on the GPU (torch tensors are only the allocator/stream plumbing); every
numerical operation of the path is a HIP kernel behind libbreeze_hip.so.  There is no CPU fallback.
"""
import ctypes as C

import numpy as np

from . import _context, _lib
from .grids import Bounded, Center, Face, Flat, Periodic, RectilinearGrid
from .thermodynamics import ReferenceState, ThermodynamicConstants, dry_air_gas_constant, vapor_gas_constant


class Centered:
    """Centered(order = 2): the AtmosphereModel constructor's default advection in the reference."""

    def __init__(self, order=2):
        if order != 2:
            raise NotImplementedError("Centered(order = 2) is implemented")
        self.order = 2


class WENO:
    """WENO(order=5; bounds=nothing).  order = 5 is the tuned path; orders 7 and 9 (the examples' choice) run through generic
    kernels (csrc/bz_tendency_generic.hip) on single-GPU anelastic models (θ or StaticEnergy, 2-D Flat grids too) and on compressible
    models (single GPU or y-slabs, with Kessler) whose grid carries halos of at least (order + 1) / 2 cells, as Oceananigans requires.  `bounds = (lo, hi)` (order 5) makes it the
    bounds-preserving scheme (Oceananigans' BoundsPreservingWENO) that the reference's moist examples give their moisture
    densities (examples/rico.jl:184-190, examples/tropical_cyclone_world.jl:169); it is a per-scalar scheme:
    `advection = {"momentum": WENO(), "ρθ": WENO(), "ρqᵉ": WENO(bounds=(0, 1))}`."""

    def __init__(self, order=5, bounds=None, ft2_hypothesis=0):
        """ft2_hypothesis (0, 1, 2): which reading of Oceananigans' second float type FT2 = Float32 the reconstruction follows (SURVEY
        Appendix D.1; csrc/bz_weno.h: BZ_WENO_FT2) — 0 everything in the grid's type (shipped), 1 newton_div quotients, 2 weights in Float32.
        1 and 2 run from lib/libbreeze_hip_ft2_<level>.so (Float64 grids): parity instrumentation for the day reference goldens exist."""
        if order not in (5, 7, 9):
            raise NotImplementedError("WENO orders 5, 7 and 9 are implemented in the HIP path")
        if ft2_hypothesis not in (0, 1, 2):
            raise ValueError("ft2_hypothesis is 0, 1 or 2")
        self.ft2_hypothesis = ft2_hypothesis
        if order != 5 and bounds is not None:
            raise NotImplementedError("bounds-preserving WENO is implemented for order 5")
        self.order = order
        if bounds is not None:
            bounds = (float(bounds[0]), float(bounds[1]))
            if not bounds[1] > bounds[0]:
                raise ValueError("bounds must be (lower, upper) with upper > lower")
        self.bounds = bounds


_MOISTURE_KEYS = ("ρq", "ρqᵛ", "ρqᵉ", "ρqᵗ")
_SPECIES_KEYS = ("ρqᶜˡ", "ρqʳ")


def _merge_advection(advection, momentum_advection, scalar_advection):
    """atmosphere_model.jl:146-152: a single `advection` serves momentum and scalars; otherwise `momentum_advection` and `scalar_advection`
    (one scheme, or a NamedTuple keyed by scalar name) each default to Centered(order = 2).  Returns `advection` in the form
    `_split_advection` takes: one scheme, or a dict keyed by `momentum` and the scalar names (`scalars` = every scalar not named)."""
    if advection is not None:
        if momentum_advection is not None or scalar_advection is not None:
            raise ValueError("pass either `advection` or `momentum_advection` / `scalar_advection`")
        return advection
    if momentum_advection is None and scalar_advection is None:
        return None
    momentum_advection = momentum_advection or Centered(order=2)
    scalar_advection = scalar_advection or Centered(order=2)
    merged = {"momentum": momentum_advection}
    if isinstance(scalar_advection, dict):
        merged.update({str(k).lstrip(":"): v for k, v in scalar_advection.items()})
        merged.setdefault("scalars", Centered(order=2))      # validate_tracer_advection: scalars a NamedTuple does not name take the default
    else:
        merged["scalars"] = scalar_advection
    return merged


def _split_advection(advection, tracer_names):
    """The reference accepts one scheme or a NamedTuple of schemes keyed by `momentum` and the scalar names
    (atmosphere_model.jl advection keyword; examples/rico.jl:186-190).  Returns (momentum scheme, bounds-preserving request or None,
    order of the scalars' schemes, whether scalars the NamedTuple does not name would take a scheme of another order)."""
    if not isinstance(advection, dict):
        if getattr(advection, "bounds", None) is not None:
            raise NotImplementedError("bounds-preserving WENO is a scalar scheme: pass advection = {'momentum': WENO(), ..., 'ρqᵉ': WENO(bounds=(0, 1))}")
        return advection, None, advection.order, False
    advection = {str(k).lstrip(":"): v for k, v in advection.items()}
    base = advection.get("momentum") or next(iter(advection.values()))
    named = {k: v for k, v in advection.items() if k not in ("momentum", "scalars")}
    rest = advection.get("scalars")          # scheme of the scalars not named (_merge_advection); absent: the momentum scheme's order
    orders = {getattr(v, "order", None) for v in named.values()}
    if len(orders) > 1:
        raise NotImplementedError("every scalar must be advected with a scheme of one order")
    scalar_order = orders.pop() if orders else (rest.order if rest is not None else base.order)
    unnamed_differ = bool(named) and rest is not None and rest.order != scalar_order
    if (base.order == 2) != (scalar_order == 2):
        raise NotImplementedError("Centered(order = 2) for momentum with WENO scalars (or the reverse) is not implemented")
    bounded, lo_hi = {"moisture": 0, "microphysical_species": 0, "tracers": 0}, None
    for key, scheme in named.items():
        b = getattr(scheme, "bounds", None)
        if b is None:
            continue
        if key in ("ρθ", "ρe"):
            raise NotImplementedError(f"bounds-preserving advection of {key} is not implemented (moisture, microphysical species, tracers)")
        if lo_hi is not None and b != lo_hi:
            raise NotImplementedError("one pair of bounds for all bounds-preserving scalars")
        lo_hi = b
        if key in _MOISTURE_KEYS:
            bounded["moisture"] = 1
        elif key in _SPECIES_KEYS:
            bounded["microphysical_species"] = 1
        elif key.lstrip("ρ") in tracer_names or key in tracer_names:
            bounded["tracers"] = 1
        else:
            raise ValueError(f"advection key {key!r} names no prognostic scalar of this model")
    if getattr(base, "bounds", None) is not None or getattr(rest, "bounds", None) is not None:
        raise NotImplementedError("bounds-preserving WENO is given per scalar: scalar_advection = {'ρθ': WENO(), 'ρqᵉ': WENO(bounds=(0, 1))}")
    if lo_hi is None:
        return base, None, scalar_order, unnamed_differ
    return base, dict(bounded, lower=lo_hi[0], upper=lo_hi[1]), scalar_order, unnamed_differ


def _check_bounded_clients(advection, tracer_names, species_names):
    """The library limits scalars by class, one mask bit each for the moisture, the microphysical species and the tracers
    (csrc/bz_bounded.hip: bz_set_bounds_preserving_advection): bounds on some scalars of a class would limit all of them, and bounds on a
    species the model's microphysics does not carry would limit nothing.  Both are refused here, by name, before `_split_advection`
    folds the names into the three flags.  `species_names`: the prognostic species of the model (`_SPECIES_KEYS` with Kessler, else none)."""
    if not isinstance(advection, dict):
        return
    limited = {str(k).lstrip(":") for k, s in advection.items() if getattr(s, "bounds", None) is not None} - {"momentum", "scalars"}
    for key in _SPECIES_KEYS:
        if key in limited and key not in species_names:
            raise ValueError(f"advection key {key!r} names no prognostic scalar of this model: its microphysics has no such species, "
                             "and the scalar's bounds would be ignored")
    unnamed = [k for k in species_names if k not in limited] if limited & set(species_names) else []
    tracers_limited = [t for t in tracer_names if t in limited or "ρ" + t in limited]
    if tracers_limited:
        unnamed += [t for t in tracer_names if t not in tracers_limited]
    if unnamed:
        raise NotImplementedError("bounds-preserving advection is switched on for all microphysical species and for all tracers at once: "
                                  f"give {unnamed} the same WENO(bounds = ...) too (or none of their class)")


class AnelasticDynamics:
    """AnelasticDynamics(reference_state)  (src/AnelasticEquations/anelastic_dynamics.jl:5-8)."""

    def __init__(self, reference_state):
        self.reference_state = reference_state
        self.pressure_anomaly = None   # materialised by AtmosphereModel


class PrescribedDynamics:
    """PrescribedDynamics(reference_state; divergence_correction=false) (src/KinematicDriver/prescribed_dynamics.jl:27-84): the kinematic
    driver.  Density and pressure are the reference state's, the velocities are ordinary fields set with `model.set(u=..., v=..., w=...)`,
    and only the scalars (ρθ, moisture, tracers) advance; there is no momentum and no pressure solver.  With `divergence_correction` every
    scalar tendency carries `+ c ∇·(ρU)` (kinematic_driver_time_stepping.jl:66-73), for velocity fields that are not anelastically
    non-divergent."""

    def __init__(self, reference_state, divergence_correction=False):
        self.reference_state = reference_state
        self.divergence_correction = bool(divergence_correction)
        self.pressure_anomaly = None


class PrescribedVelocityFields:
    """PrescribedVelocityFields(u=f(x, y, z, t), ...) of the reference (functions of time): named so that the constructor can refuse it."""

    def __init__(self, u=None, v=None, w=None, parameters=None):
        self.u, self.v, self.w, self.parameters = u, v, w, parameters


def _check_kinematic_options(model_type, grid, dynamics, advection, formulation, closure, microphysics, forcing, boundary_conditions, velocities,
                             coriolis):
    """What AtmosphereModel(dynamics = PrescribedDynamics(...)) runs: (Periodic, Periodic | Flat, Bounded), Float64, WENO(order = 5), the
    potential-temperature formulation, microphysics nothing or warm-phase saturation adjustment, tracers, one GPU.  Everything else of the
    reference's kinematic driver says so here, by name."""
    from .microphysics import SaturationAdjustment
    _context.refuse_bulk_microphysics(microphysics, "AtmosphereModel(dynamics = PrescribedDynamics(...))", "the kinematic driver runs no negative moisture correction")

    def no(what):
        raise NotImplementedError(f"AtmosphereModel(dynamics = PrescribedDynamics(...)): {what} not implemented")
    if not isinstance(dynamics.reference_state, ReferenceState):
        no("prognostic density (PrescribedDynamics(ρ_field)) is")
    if model_type is not AtmosphereModel:
        no("y-slab (distributed) models are")
    if grid.topology not in ((Periodic, Periodic, Bounded), (Periodic, Flat, Bounded)):
        no(f"topology {grid.topology} is")
    if grid.ftype != 8:
        no("Float32 grids are")
    schemes = list(advection.values()) if isinstance(advection, dict) else [advection]
    for s in schemes:
        if s is None or isinstance(s, Centered):
            no("Centered advection is (pass advection = WENO(order = 5)); it is")
        if not isinstance(s, WENO):
            no(f"advection scheme {type(s).__name__} is")
        if s.bounds is not None:
            no("bounds-preserving advection (WENO(bounds = ...)) is")
        if s.order != 5:
            no(f"WENO(order = {s.order}) is")
        if s.ft2_hypothesis:
            no("WENO(ft2_hypothesis != 0) is")
    if str(formulation).lstrip(":") != "LiquidIcePotentialTemperature":
        no(f"the {str(formulation).lstrip(':')} formulation is")
    if microphysics is not None and not isinstance(microphysics, SaturationAdjustment):
        no(f"microphysics {type(microphysics).__name__} (Kessler) is")
    _context.refuse_mixed_phase(microphysics, "AtmosphereModel(dynamics = PrescribedDynamics(...))", "the kinematic driver diagnoses qᵛ and qˡ only")
    if closure is not None:
        no("a closure is")
    if forcing is not None or coriolis is not None:
        no("forcing (Forcing, Relaxation sponges, subsidence, Coriolis) is")
    if boundary_conditions is not None:
        w = boundary_conditions.get("w") if isinstance(boundary_conditions, dict) else None
        if w is not None:
            no("a NormalFlowBoundaryCondition (or any boundary condition) on w is")
        no("flux and value boundary conditions are")
    if velocities is not None:
        no("PrescribedVelocityFields (velocities as functions of time) is")


class Clock:
    def __init__(self):
        self.time, self.iteration, self.last_Δt = 0.0, 0, float("inf")


class Field:
    """A device-resident Oceananigans-style field: `.parent` is the halo-inclusive array
    ((z, y, x)-shaped, x fastest), `.interior` a view of the interior."""

    def __init__(self, grid, loc, device, float_type=None):
        import torch
        self.grid, self.loc = grid, loc
        self.zface = loc[2] is Face
        # float_type: CenterField(grid, FT) of another element type than eltype(grid) (the substepper's working fields)
        ft = getattr(grid, "ftype", 8) if float_type is None else np.dtype(float_type).itemsize
        self.dtype = torch.float32 if ft == 4 else torch.float64
        self.parent = torch.zeros(grid.parent_shape(self.zface), dtype=self.dtype, device=device)

    @property
    def interior(self):
        return self.parent[self.grid.interior_slices(self.zface)]

    def ptr(self):
        return self.parent.data_ptr()

    # u * w, w ** 3, ... are expressions for Average(...) (diagnostics.py); nothing is evaluated here
    def __mul__(self, other):
        from .diagnostics import _Product
        return _Product(self, other)

    def __pow__(self, p):
        from .diagnostics import _Power
        return _Power(self, p)

    def __add__(self, other):
        from .diagnostics import _Sum
        return _Sum(self, other)

    __sub__ = __radd__ = __rsub__ = __add__

    def set_interior(self, value):
        import torch
        g = self.grid
        if callable(value):
            x, y, z = g.nodes(self.loc)
            import inspect
            # functions of the non-Flat coordinates, as in Oceananigans: f(x, z) on a (Periodic, Flat, Bounded) grid
            two = g.topology[1] == "Flat" and len(inspect.signature(value).parameters) == 2
            value = value(x, z) if two else value(x, y, z)
        shape = tuple(self.interior.shape)
        arr = np.broadcast_to(np.asarray(value, dtype=np.float64), shape)
        self.interior.copy_(torch.from_numpy(np.array(arr, dtype=np.float64, order="C")).to(self.dtype))

    # diagnostic fields of a model (u, v, w, θ, qᵛ, T, pressure anomaly) know their owner: after time_steps(..., diagnose_last=False)
    # they are older than the prognostic state, and a host read rebuilds them first (update_state!) instead of returning stale values
    _owner = None

    def _fresh(self):
        m = self._owner() if self._owner is not None else None
        if m is not None and getattr(m, "_ctx", None) and diagnostics_stale(m):
            if getattr(m, "_collective_refresh", False):
                # slab models: rebuilding the diagnostics exchanges halos — a collective a single rank's read must not enter on its own
                # (a rank-0-only log line would wait for ranks that never come)
                raise RuntimeError("the diagnostic fields of this slab model are older than its prognostic state (time_steps(..., diagnose_last=False)): "
                                   "call model.refresh_diagnostics() on EVERY rank before reading them")
            m._refresh_diagnostics()

    def cpu(self):
        self._fresh()
        return self.parent.cpu().numpy()

    def interior_cpu(self):
        self._fresh()
        return self.interior.cpu().numpy()


_LOC = {"ccc": (Center, Center, Center), "fcc": (Face, Center, Center),
        "cfc": (Center, Face, Center), "ccf": (Center, Center, Face)}

# keyword spellings accepted by set_ (Julia names and ASCII transliterations)
_ALIASES = {"θ": "θ", "theta": "θ", "θˡⁱ": "θ", "ρθ": "ρθ", "rho_theta": "ρθ", "e": "e", "ρe": "ρe", "rho_e": "ρe",
            "u": "u", "v": "v", "w": "w", "ρu": "ρu", "ρv": "ρv", "ρw": "ρw",
            "rho_u": "ρu", "rho_v": "ρv", "rho_w": "ρw",
            "qᵗ": "q", "qt": "q", "qᵛ": "q", "qv": "q", "qᵉ": "q", "qe": "q", "ρqᵗ": "ρq", "ρqᵛ": "ρq", "ρqᵉ": "ρq", "ρqe": "ρq",
            "rho_q": "ρq", "qᶜˡ": "qcl", "qcl": "qcl", "qʳ": "qr", "qr": "qr", "T": "T", "ℋ": "ℋ", "H": "ℋ", "relative_humidity": "ℋ",      # Python NFKC-normalises the keyword ℋ to H
            # NFKC-normalised spellings (Python normalises identifiers used as keywords)
            "θli": "θ", "ρqt": "ρq", "ρqv": "ρq"}


class AtmosphereModel(_context.ContextOwner):
    """AtmosphereModel(grid; dynamics=AnelasticDynamics(ReferenceState(grid)), advection=WENO(order=5),
    formulation=:LiquidIcePotentialTemperature, thermodynamic_constants, timestepper=:SSPRungeKutta3).

    Dry anelastic dynamics without closure / Coriolis / forcing / microphysics — the configuration
    of BASELINE.json configs 1-2 and 4."""

    def __init__(self, grid, dynamics=None, advection=None, thermodynamic_constants=None,
                 formulation="LiquidIcePotentialTemperature", timestepper="SSPRungeKutta3",
                 closure=None, coriolis=None, microphysics=None, forcing=None, boundary_conditions=None,
                 tracers=(), device="cuda:0", momentum_advection=None, scalar_advection=None, velocities=None):
        import torch
        if not isinstance(grid, RectilinearGrid):
            raise TypeError("grid must be a RectilinearGrid")
        advection = _merge_advection(advection, momentum_advection, scalar_advection)
        # dynamics = PrescribedDynamics(reference_state): the kinematic driver (csrc/bz_kinematic.hip)
        self._kinematic = kin = isinstance(dynamics, PrescribedDynamics)
        if kin:
            _check_kinematic_options(type(self), grid, dynamics, advection, formulation, closure, microphysics, forcing, boundary_conditions,
                                     velocities, coriolis)
        elif velocities is not None:
            raise ValueError("`velocities` belongs to AtmosphereModel(dynamics = PrescribedDynamics(...))")
        bounded_x = grid.topology == (Bounded, Flat, Bounded)          # walls in x of a 2-D model: examples/cloudy_thermal_bubble.jl
        flat_y = grid.topology == (Periodic, Flat, Bounded) or bounded_x
        bounded_y = grid.topology == (Periodic, Bounded, Bounded)      # walls in y: the reference benchmark driver's PBB option
        if grid.topology != (Periodic, Periodic, Bounded) and not flat_y and not bounded_y:
            raise NotImplementedError("the HIP path implements topology (Periodic, Periodic, Bounded), (Periodic, Flat, Bounded), "
                                      "(Bounded, Flat, Bounded) and (Periodic, Bounded, Bounded)")
        if advection is None:
            advection = Centered(order=2)          # the reference's default (resolved before the Flat guard: ADVICE r02)
        _base = advection.get("momentum") or next(iter(advection.values())) if isinstance(advection, dict) else advection
        if flat_y and (not isinstance(_base, WENO) or _base.order not in (5, 7, 9)):
            # the reference's 2-D x-z cases (README.md:67-75, examples/dry_thermal_bubble.jl with WENO(order = 9)): the per-operator
            # kernels drop the y terms
            raise NotImplementedError("(Periodic, Flat, Bounded): WENO(order = 5 | 7 | 9) models are implemented")
        formulation = str(formulation).lstrip(":")
        _any_bounds = any(getattr(s, "bounds", None) is not None for s in (advection.values() if isinstance(advection, dict) else (advection,)))
        if bounded_x and (_any_bounds or grid.Nx % 2):
            raise NotImplementedError("(Bounded, Flat, Bounded): WENO(order = 5 | 7 | 9) models without bounds-preserving advection on an even "
                                      "number of columns are implemented")
        if bounded_y and (not isinstance(_base, WENO) or _base.order not in (5, 7, 9) or _any_bounds):
            # Coriolis, forcings, bottom flux boundary conditions and the closure reach their y neighbours through the halo rows (as on
            # y-slabs); microphysics, tracers and the StaticEnergy formulation are column- or cell-local
            raise NotImplementedError("(Periodic, Bounded, Bounded): WENO(order = 5 | 7 | 9) models without bounds-preserving advection "
                                      "are implemented")
        if formulation not in ("LiquidIcePotentialTemperature", "StaticEnergy"):
            raise NotImplementedError(f"formulation {formulation!r} is not implemented")
        self.formulation = formulation
        if timestepper not in ("SSPRungeKutta3", ":SSPRungeKutta3"):
            raise NotImplementedError("only SSPRungeKutta3 is implemented")
        self._diffusivity = _context.check_closure(closure)
        if self._diffusivity and any("Slab" in k.__name__ for k in type(self).__mro__):      # the y-slab models of distributed.py
            raise NotImplementedError("closure = ScalarDiffusivity / VerticalScalarDiffusivity: not implemented on y-slab (distributed) models")
        if self._diffusivity and (bounded_x or bounded_y):
            raise NotImplementedError("closure = ScalarDiffusivity / VerticalScalarDiffusivity: not implemented between walls in x or y "
                                      "(Bounded x / Bounded y)")
        self.closure = closure
        self.coriolis, self.forcing, self.boundary_conditions = coriolis, forcing, boundary_conditions
        if any("Slab" in k.__name__ for k in type(self).__mro__):      # the y-slab models of distributed.py
            _context.refuse_bulk_microphysics(microphysics, type(self).__name__, "y-slab models run no negative moisture correction")
        from .microphysics import cloud_formation
        self._kessler = _context.check_microphysics(cloud_formation(microphysics), "microphysics: SaturationAdjustment(equilibrium = WarmPhaseEquilibrium()) and "
                                                                  "DCMIP2016KesslerMicrophysics() are implemented",
                                                    instantaneous_precipitation_refused="InstantaneousPrecipitation: implemented on CompressibleDynamics "
                                                    "(CompressibleAtmosphereModel); not on the anelastic AtmosphereModel, the kinematic driver or their y-slab models")
        if microphysics is not None and formulation != "LiquidIcePotentialTemperature":
            raise NotImplementedError("microphysics is implemented for the potential-temperature formulation")
        if any("Slab" in k.__name__ for k in type(self).__mro__):      # the y-slab models of distributed.py
            _context.refuse_mixed_phase(microphysics, type(self).__name__, "the halo exchanges of y-slab models carry qᵛ and qˡ only")
        _context.check_mixed_phase_model(microphysics, thermodynamic_constants, forcing, boundary_conditions)
        # FlatauPolynomial constants: single-device anelastic models; the places that hard-wire Clausius-Clapeyron refuse by name
        if any("Slab" in k.__name__ for k in type(self).__mro__):
            _context.refuse_flatau_polynomial(thermodynamic_constants, type(self).__name__, "y-slab models evaluate the Clausius-Clapeyron expression")
        if kin:
            _context.refuse_flatau_polynomial(thermodynamic_constants, "AtmosphereModel(dynamics = PrescribedDynamics(...))",
                                              "the kinematic driver evaluates the Clausius-Clapeyron expression")
        _context.check_flatau_anelastic(thermodynamic_constants, boundary_conditions)
        self.microphysics = microphysics
        if self._kessler:
            _context.check_kessler_constants(thermodynamic_constants)
        _named = set(str(k).lstrip(":") for k in advection) if isinstance(advection, dict) else set()
        _tracer_names = tuple(str(n).lstrip(":") for n in ((tracers,) if isinstance(tracers, str) else tracers))
        _check_bounded_clients(advection, _tracer_names, _SPECIES_KEYS if self._kessler else ())
        advection, self._bounded_advection, self._scalar_order, _unnamed_differ = _split_advection(advection, _tracer_names)
        if _unnamed_differ:
            # scalar_advection was a NamedTuple: every scalar of the model it does not name takes Centered(order = 2) in the reference
            missing = {"ρe" if formulation == "StaticEnergy" else "ρθ"} - _named
            if not _named & set(_MOISTURE_KEYS):
                missing.add("moisture")
            if self._kessler:
                missing |= set(_SPECIES_KEYS) - _named
            missing |= {t for t in _tracer_names if t not in _named and "ρ" + t not in _named}
            if missing:
                raise NotImplementedError("scalar_advection names only some scalars: the others would take Centered(order = 2), and one order "
                                          f"for all scalars is implemented (unnamed: {sorted(missing)})")
        if not torch.cuda.is_available():
            raise RuntimeError("AtmosphereModel needs a GPU: the HIP path has no CPU fallback")
        self.grid = grid
        self.advection = advection
        if isinstance(advection, WENO) and max(advection.order, self._scalar_order) != 5:
            order = max(advection.order, self._scalar_order)
            need = (order + 1) // 2
            if min(h for h, t in zip((grid.Hx, grid.Hy, grid.Hz), grid.topology) if t != Flat) < need:
                raise ValueError(f"WENO(order={order}) needs halos of at least {need} cells in every direction "
                                 f"(got {(grid.Hx, grid.Hy, grid.Hz)}): RectilinearGrid(..., halo=({need}, {need}, {need}))")
        if self._bounded_advection is not None and self._scalar_order != 5:
            raise NotImplementedError(f"WENO(order={self._scalar_order}): bounds-preserving advection is implemented for order 5")
        self.thermodynamic_constants = c = thermodynamic_constants or ThermodynamicConstants()
        if dynamics is None:
            dynamics = AnelasticDynamics(ReferenceState(grid, c))      # default_dynamics
        self.dynamics = dynamics
        self.clock = Clock()
        self.device = torch.device(device)
        torch.cuda.set_device(self.device)
        self._T = T = _lib.types(grid.ftype)
        self._lib = lib = _context.load_library(grid, advection, "Float32 grids: WENO(order = 5 | 7 | 9) is wired up on the host side")
        fld = _context.allocate_common_fields(self, grid, momentum=not kin)      # a kinematic model has no prognostic momentum
        # :StaticEnergy keeps rho_e / e in the thermodynamic slots (energy_density, specific_energy)
        self.energy_density, self.specific_energy = self.potential_temperature_density, self.potential_temperature
        dynamics.pressure_anomaly = None if kin else fld("ccc")
        # the context owns the Fourier-tridiagonal solver of an anelastic model; a kinematic model has none
        self.pressure_solver = None if kin else "FourierTridiagonalPoissonSolver"
        import weakref
        # (the velocities of a kinematic model are the user's, not diagnostics: reading them never rebuilds anything)
        for _f in ((self.potential_temperature, self.specific_moisture, self.temperature) if kin else
                   (*self.velocities.values(), self.potential_temperature, self.specific_moisture, self.temperature, dynamics.pressure_anomaly)):
            _f._owner = weakref.ref(self)
        self.microphysical_fields = {}
        if self._kessler:
            _context.materialize_kessler_fields(self, fld)
        # tracers = (:a, :b): prognostic density fields model.tracers[name]; the specific field sits beside it
        tracers = (tracers,) if isinstance(tracers, str) else tuple(tracers)
        self.tracers = {str(n).lstrip(":"): fld("ccc") for n in tracers}
        self.specific_tracers = {n: fld("ccc") for n in self.tracers}
        prog = self.prognostic_fields()
        self.U0 = {k: Field(grid, f.loc, self.device) for k, f in prog.items()}     # timestepper.U⁰
        self.G = {k: Field(grid, f.loc, self.device) for k, f in prog.items()}      # timestepper.Gⁿ

        # ---- context: pressure solver, column tables ----
        ref = dynamics.reference_state
        bg, self._zf = _context.grid_struct(T, grid)
        br, self._ref_arrays = _context.reference_struct(T, ref)
        self._open_context("bz_create", bg, _context.constants_struct(T, c), br, advection.order)
        if kin:
            self._check(lib.bz_set_prescribed_dynamics(self._ctx, 1 if dynamics.divergence_correction else 0), "bz_set_prescribed_dynamics")
        if formulation == "StaticEnergy":
            self._check(lib.bz_set_formulation(self._ctx, 1), "bz_set_formulation")
        if self._scalar_order != advection.order:      # momentum_advection and scalar_advection of different orders
            self._check(lib.bz_set_scalar_advection_order(self._ctx, self._scalar_order), "bz_set_scalar_advection_order")
        if self._kessler:
            _context.attach_kessler(self, ref.standard_pressure)
        elif microphysics is not None:
            _context.attach_saturation_adjustment(self, fld)
            _context.attach_negative_moisture_correction(self)      # of a BulkMicrophysics
            _context.attach_flatau_polynomial(self)                 # saturation_vapor_pressure = FlatauPolynomial() of the constants
        if self.tracers:
            arr = (_lib.bz_tracer_fields * len(self.tracers))()
            for t, n in enumerate(self.tracers):
                arr[t].density, arr[t].specific = self.tracers[n].ptr(), self.specific_tracers[n].ptr()
                arr[t].U0, arr[t].G = self.U0[n].ptr(), self.G[n].ptr()
            self._check(lib.bz_set_tracers(self._ctx, len(self.tracers), arr), "bz_set_tracers")
        if self._bounded_advection is not None:
            ba = self._bounded_advection
            if ba["tracers"] and ba["tracers"] != 0 and len(self.tracers) == 0:
                raise ValueError("bounds-preserving tracer advection without tracers")
            bs = T.bz_bounds_preserving_advection(ba["lower"], ba["upper"], ba["moisture"], ba["microphysical_species"], ba["tracers"], 0)
            self._check(lib.bz_set_bounds_preserving_advection(self._ctx, C.byref(bs)), "bz_set_bounds_preserving_advection")
        _context.attach_closure(self, fld, smagorinsky_refused="SmagorinskyLilly is implemented for the potential-temperature formulation "
                                "without Kessler" if self._kessler or formulation != "LiquidIcePotentialTemperature" else None)
        # coriolis / forcing / boundary_conditions of the BOMEX configuration -> one column-forcing stack (forcings.py)
        from .forcings import materialize_forcings, split_relaxation
        forcing, _relax, _field = split_relaxation(forcing)      # Relaxation sponges and 3-D forcings: their own attachments
        _context.attach_relaxation(self, _relax, formulation)
        _context.attach_field_forcing(self, _field, formulation)
        F, self._forcing_keepalive = materialize_forcings(grid, coriolis, forcing, boundary_conditions, T)
        if F is not None:
            if self._kessler or formulation != "LiquidIcePotentialTemperature":
                raise NotImplementedError("forcings are implemented for the potential-temperature formulation without Kessler")
            self._check(lib.bz_set_forcings(self._ctx, C.byref(F)), "bz_set_forcings")
        from .forcings import materialize_bulk_fluxes
        Bk = materialize_bulk_fluxes(boundary_conditions, ref, c, T)
        if Bk is not None:
            if self._kessler or formulation != "LiquidIcePotentialTemperature":
                raise NotImplementedError("bulk surface fluxes are implemented for the potential-temperature formulation without Kessler")
            self._check(lib.bz_set_bulk_surface_fluxes(self._ctx, C.byref(Bk)), "bz_set_bulk_surface_fluxes")
        # PolynomialCoefficient / FilteredSurfaceVelocities / T₀(x, y) conditions: the surface-layer configuration (forcings.py)
        from .forcings import materialize_surface_layer
        Sl, self._surface_layer_keepalive, self.filtered_velocities = materialize_surface_layer(grid, boundary_conditions, ref, c, T)
        self._surface_filter_initialized = False
        if Sl is not None:
            if self._kessler or formulation != "LiquidIcePotentialTemperature":
                raise NotImplementedError("bulk surface fluxes are implemented for the potential-temperature formulation without Kessler")
            self._check(lib.bz_set_surface_layer(self._ctx, C.byref(Sl)), "bz_set_surface_layer")
        self._state = self._make_state()
        self._U0 = self._make_prog(self.U0)
        self._G = self._make_prog(self.G)
        # initialize_model_thermodynamics!: θ = θ₀  (anelastic_time_stepping.jl:15-19); nothing for a kinematic model
        # (kinematic_driver_time_stepping.jl:16)
        if not kin:
            set_(self, θ=ref.potential_temperature)

    def prognostic_fields(self):
        out = dict(self.momentum)
        out.update({"ρθ": self.potential_temperature_density, "ρq": self.moisture_density})
        if getattr(self, "_kessler", False):
            out["ρqᶜˡ"], out["ρqʳ"] = self.microphysical_fields["ρqᶜˡ"], self.microphysical_fields["ρqʳ"]
        out.update(getattr(self, "tracers", {}))
        return out

    def _make_state(self):
        s = _lib.bz_state()
        if self.momentum:
            s.rho_u, s.rho_v, s.rho_w = (self.momentum[k].ptr() for k in ("ρu", "ρv", "ρw"))
        s.rho_theta, s.rho_q = self.potential_temperature_density.ptr(), self.moisture_density.ptr()
        s.u, s.v, s.w = (self.velocities[k].ptr() for k in ("u", "v", "w"))
        s.theta, s.q, s.T = self.potential_temperature.ptr(), self.specific_moisture.ptr(), self.temperature.ptr()
        if self.dynamics.pressure_anomaly is not None:
            s.phi = self.dynamics.pressure_anomaly.ptr()
        return s

    @staticmethod
    def _make_prog(d):
        p = _lib.bz_prognostic()
        if "ρu" in d:
            p.rho_u, p.rho_v, p.rho_w = (d[k].ptr() for k in ("ρu", "ρv", "ρw"))
        p.rho_theta, p.rho_q = d["ρθ"].ptr(), d["ρq"].ptr()
        return p

    # method spellings of the module-level functions
    def _create_context(self, lib, bg, bc, br, order):
        return lib.bz_create(C.byref(self._ctx), C.byref(bg), C.byref(bc), C.byref(br), order)

    def set(self, **kw):
        return set_(self, **kw)

    def time_step(self, Δt):
        return time_step_(self, Δt)

    def time_steps(self, Δt, n, diagnose_last=True):
        """n × time_step!(model, Δt) in one C call (bz_time_steps_anelastic): the reference's many_time_steps! loop
        (/root/reference/benchmarking/src/timestepping.jl:11-16) and run!'s stretch between two callback iterations.  With
        diagnose_last=False the velocities / θ / qᵛ / T / pressure anomaly stay stale until update_state_(model) (stepping may go on)."""
        return many_time_steps_(self, Δt, n, diagnose_last)

    # -- filtered surface state (FilteredSurfaceVelocities) --------------------
    _FILTERED = {"u": 0, "v": 1, "θᵥ": 2, "θv": 2, "theta_v": 2, "θ": 3, "theta": 3, "q": 4}

    def initialize_(self):
        """initialize!(model) (update_boundary_conditions.jl:119-122): the filtered surface fields take the current first-level values.
        Runs by itself before the first step unless the fields were set."""
        self._check(self._lib.bz_surface_layer_initialize(self._ctx, C.byref(self._state)), "bz_surface_layer_initialize")
        self._surface_filter_initialized = True

    def update_filtered_surface_state_(self, Δt):
        """update!(fv, ..., Δt) of every filtered field, ε = Δt / τ (the per-operator sequence calls it at the filter's update_stages)."""
        self._check(self._lib.bz_surface_layer_update(self._ctx, C.byref(self._state), float(Δt) / self.filtered_velocities.filter_timescale),
                    "bz_surface_layer_update")

    def filtered_surface_field(self, name):
        """(Ny, Nx) host copy of a filtered 2-D field: "u" (x faces), "v" (y faces), "θᵥ", "θ", "q" (centres)."""
        a = np.empty((self.grid.Ny, self.grid.Nx), dtype=self._T.np_real)
        self._check(self._lib.bz_surface_layer_get_filtered(self._ctx, self._FILTERED[name], a.ctypes.data_as(C.POINTER(self._T.real))),
                    "bz_surface_layer_get_filtered")
        return a

    def set_filtered_surface_field(self, name, value):
        """set!(fv.u, ...): checkpoints and tests."""
        a = np.ascontiguousarray(np.broadcast_to(np.asarray(value, dtype=self._T.np_real), (self.grid.Ny, self.grid.Nx)))
        self._check(self._lib.bz_surface_layer_set_filtered(self._ctx, self._FILTERED[name], a.ctypes.data_as(C.POINTER(self._T.real))),
                    "bz_surface_layer_set_filtered")
        self._surface_filter_initialized = True

    def _refresh_diagnostics(self):
        """update_state!(model; compute_tendencies=false) after undiagnosed steps (slab models override it with the exchanging form)."""
        update_state_(self, compute_tendencies=False)

    def refresh_diagnostics(self):
        """Rebuild u, v, w, θ, qᵛ, T from the prognostic state if they are stale.  On slab models a collective: call it on every rank."""
        if diagnostics_stale(self):
            self._refresh_diagnostics()

    def graph_enable(self, on=True):
        """hipGraph replay of whole steps (csrc/bz_graph.hip); opt-in, bit-identical to launched steps."""
        if self._kinematic and on:
            raise NotImplementedError("AtmosphereModel(dynamics = PrescribedDynamics(...)): hipGraph replay is not implemented")
        super().graph_enable(on)

    def max_abs_divergence(self):
        if self._kinematic:
            raise ValueError("a kinematic model has no momentum")
        out = self._T.real()
        self._check(self._lib.bz_max_abs_divergence(self._ctx, C.byref(self._state), C.byref(out)),
                    "bz_max_abs_divergence")
        return out.value


# ---------------------------------------------------------------------------
# Julia-style generic functions on the model (f! -> f_)
# ---------------------------------------------------------------------------
def fill_halo_regions_(model, field, kind=None):
    if kind is None:
        kind = (1 if field.zface else 0) + (4 if field.loc[1] is Face else 0) + (8 if field.loc[0] is Face else 0)      # + 4 / + 8: y- / x-face field
    model._check(model._lib.bz_fill_halo_regions(model._ctx, C.c_void_p(field.ptr()), kind), "bz_fill_halo_regions")


def update_state_(model, compute_tendencies=True):
    model._check(model._lib.bz_update_state(model._ctx, C.byref(model._state), C.byref(model._G),
                                            1 if compute_tendencies else 0), "bz_update_state")


def fix_negative_moisture_(model):
    """fix_negative_moisture!(model) (negative_moisture_correction.jl:170-193): the attached correction once on the moisture density.  The
    whole steps and update_state_ run it themselves; this is the operator alone."""
    model._check(model._lib.bz_fix_negative_moisture(model._ctx, C.byref(model._state)), "bz_fix_negative_moisture")


def compute_tendencies_(model):
    model._check(model._lib.bz_compute_tendencies(model._ctx, C.byref(model._state), C.byref(model._G)),
                 "bz_compute_tendencies")


def compute_scalar_tendency_(model, c, Gc):
    """Gc = -div_rhoUc(c) for one centre field c (halo-filled) with the model's velocities: compute_scalar_tendency!
    (update_atmosphere_model_state.jl:390-393), the launch the reference's scalar_tendency micro-benchmark times."""
    v = model.velocities
    model._check(model._lib.bz_compute_scalar_tendency(model._ctx, v["u"].ptr(), v["v"].ptr(), v["w"].ptr(), c.ptr(), Gc.ptr()),
                 "bz_compute_scalar_tendency")


def compute_closure_fields_(model):
    """compute_closure_fields!(model.closure_fields, model.closure, model) (update_atmosphere_model_state.jl:218)."""
    model._check(model._lib.bz_compute_closure_fields(model._ctx, C.byref(model._state)), "bz_compute_closure_fields")


def implicit_step_(model, Δt):
    """implicit_step!(field, implicit_solver, closure, ..., Δt) of every prognostic field (ssp_runge_kutta_3.jl:124-161): a no-op
    without a vertically implicit closure."""
    model._check(model._lib.bz_implicit_step(model._ctx, C.byref(model._state), float(Δt)), "bz_implicit_step")


def compute_flux_bc_tendencies_(model):
    """compute_flux_bc_tendencies!(model) (update_atmosphere_model_state.jl:418-434)."""
    model._check(model._lib.bz_compute_flux_bc_tendencies(model._ctx, C.byref(model._state), C.byref(model._G)),
                 "bz_compute_flux_bc_tendencies")


def compute_velocities_(model):
    model._check(model._lib.bz_compute_velocities(model._ctx, C.byref(model._state)), "bz_compute_velocities")


def compute_auxiliary_thermodynamic_variables_(model):
    model._check(model._lib.bz_compute_auxiliary_thermodynamic_variables(model._ctx, C.byref(model._state)),
                 "bz_compute_auxiliary_thermodynamic_variables")


def compute_pressure_correction_(model, Δt):
    model._check(model._lib.bz_compute_pressure_correction(model._ctx, C.byref(model._state), float(Δt)),
                 "bz_compute_pressure_correction")


def make_pressure_correction_(model, Δt):
    model._check(model._lib.bz_make_pressure_correction(model._ctx, C.byref(model._state), float(Δt)),
                 "bz_make_pressure_correction")


def store_initial_state_(model):
    model._check(model._lib.bz_store_initial_state(model._ctx, C.byref(model._state), C.byref(model._U0)),
                 "bz_store_initial_state")


def ssp_rk3_substep_(model, Δt, α):
    model._check(model._lib.bz_ssp_rk3_substep(model._ctx, C.byref(model._state), C.byref(model._U0),
                                               C.byref(model._G), float(Δt), float(α)), "bz_ssp_rk3_substep")


def enforce_mass_conservation_(model):
    """set_atmosphere_model.jl:121-128: one projection with Δt = 1."""
    compute_pressure_correction_(model, 1.0)
    make_pressure_correction_(model, 1.0)
    update_state_(model, compute_tendencies=False)


def set_(model, enforce_mass_conservation=True, balancer=None, **kw):
    """set!(model; kw...): θ / ρθ, u v w / ρu ρv ρw, qᵗ / ρqᵗ from numbers, arrays or f(x, y, z).  balancer = AdiabaticBalancer(...) | True:
    balance_adiabatically!(model, balancer) after the fields are set (set_atmosphere_model.jl; balance.py)."""
    import torch
    if balancer is not None and balancer is not False:      # refused by name before anything is set
        from .balance import require_balance_model
        require_balance_model(model, balancer, "set!(model; balancer)")
    if getattr(model, "_kinematic", False):
        return _set_kinematic(model, **kw)
    g = model.grid
    ref = model.dynamics.reference_state
    Hz, Nz = g.Hz, g.Nz
    ρc = torch.from_numpy(ref.density[Hz:Hz + Nz].copy()).to(model.device)[:, None, None]
    ρf_host = 0.5 * (ref.density[Hz - 1:Hz + Nz] + ref.density[Hz:Hz + Nz + 1])
    ρf = torch.from_numpy(ρf_host).to(model.device)[:, None, None]
    order = {"q": 0, "ρq": 0, "ℋ": 2}        # moisture first; ℋ after everything else (it needs the diagnosed temperature)
    for name, value in sorted(kw.items(), key=lambda kv: order.get(_ALIASES.get(kv[0]), 1)):
        key = _ALIASES.get(name)
        if key in ("e", "ρe") and model.formulation != "StaticEnergy":
            key = None
        if key in ("T", "ℋ") and (model.formulation != "LiquidIcePotentialTemperature" or getattr(model, "_kessler", False)):
            raise NotImplementedError(f"set!(model; {name}) is implemented for the potential-temperature formulation "
                                      "(microphysics nothing or SaturationAdjustment)")
        if key in ("T", "ℋ"):      # set-up arithmetic on Clausius-Clapeyron constants (ℋ evaluates pᵛ⁺; T is refused with it: one rule for both)
            _context.refuse_flatau_polynomial(model.thermodynamic_constants, f"set!(model; {name})", "qᵛ⁺ from ℋ is the Clausius-Clapeyron expression")
        if key in ("T", "ℋ"):      # both conversions below know the liquid phase only
            _context.refuse_mixed_phase(model.microphysics, f"set!(model; {name})", "θ from T and qᵛ⁺ from ℋ are formed without qⁱ and over the liquid surface")
        if key == "T":
            # set_thermodynamic_variable!(model, Val(:T), value) (potential_temperature_tendency.jl:202-250): theta^li from the
            # in-situ temperature with the current moisture fractions, theta = (T - L q^l / c_pm) / Pi
            c = model.thermodynamic_constants
            Rd, Rv = dry_air_gas_constant(c), vapor_gas_constant(c)
            model.temperature.set_interior(value)
            if model.microphysics is not None:
                qv, ql = model.microphysical_fields["qᵛ"].interior, model.microphysical_fields["qˡ"].interior
                cl, Ll = c.liquid_heat_capacity, c.liquid_reference_latent_heat
            else:
                qv, ql, cl, Ll = model.specific_moisture.interior, 0.0, 0.0, 0.0
            qd = 1.0 - (qv + ql)
            Rm, cpm = qd * Rd + qv * Rv, qd * c.dry_air_heat_capacity + qv * c.vapor_heat_capacity + ql * cl
            pr = torch.from_numpy(ref.pressure[Hz:Hz + Nz].copy()).to(model.device)[:, None, None]
            Π = (pr / ref.standard_pressure) ** (Rm / cpm)
            model.potential_temperature.interior.copy_((model.temperature.interior - Ll * ql / cpm) / Π)
            model.potential_temperature_density.interior.copy_(ρc * model.potential_temperature.interior)
            continue
        if key == "ℋ":
            # set!(model; ℋ) (set_atmosphere_model.jl:280-297): update_state!, q^v+ = SaturationSpecificHumidity(model, :equilibrium)
            # (vapor_saturation.jl:216-230) materialised before the moisture is overwritten, q = ℋ q^v+, rho q = rho_r q
            update_state_(model, compute_tendencies=False)
            c = model.thermodynamic_constants
            Rd, Rv = dry_air_gas_constant(c), vapor_gas_constant(c)
            T, qt = model.temperature.interior, model.specific_moisture.interior
            pr = torch.from_numpy(ref.pressure[Hz:Hz + Nz].copy()).to(model.device)[:, None, None]
            dc = c.vapor_heat_capacity - c.liquid_heat_capacity
            L0 = c.liquid_reference_latent_heat - dc * c.energy_reference_temperature
            ps = c.triple_point_pressure * (T / c.triple_point_temperature) ** (dc / Rv) * \
                torch.exp((1.0 / c.triple_point_temperature - 1.0 / T) * L0 / Rv)
            q1 = (Rd / Rv) * (1.0 - qt) * ps / (pr - ps)
            ρ = pr / ((Rd * (1.0 - qt) + Rv * qt) * T)
            q0 = ps / (ρ * Rv * T)
            qsat = torch.where(qt >= q0, q1, q0)
            model.specific_moisture.set_interior(value)
            model.specific_moisture.interior.mul_(qsat)
            model.moisture_density.interior.copy_(ρc * model.specific_moisture.interior)
            continue
        if key is None:
            raise ValueError(f"Cannot set! {name} in AtmosphereModel because {name} is neither a prognostic "
                             "variable, a settable thermodynamic variable, nor a settable diagnostic variable!")
        if key == "θ" and model.formulation == "StaticEnergy":
            # _energy_density_from_potential_temperature! (static_energy_tendency.jl:93-140): host set-up arithmetic
            c = model.thermodynamic_constants
            Rd, Rv = dry_air_gas_constant(c), vapor_gas_constant(c)
            scratch = model.temperature
            scratch.set_interior(value)
            q = model.specific_moisture.interior
            qd = 1.0 - q
            Rm, cpm = qd * Rd + q * Rv, qd * c.dry_air_heat_capacity + q * c.vapor_heat_capacity
            pr = torch.from_numpy(ref.pressure[Hz:Hz + Nz].copy()).to(model.device)[:, None, None]
            z = torch.from_numpy(np.ascontiguousarray(g.zᶜ)).to(model.device)[:, None, None]
            T = (pr / ref.standard_pressure) ** (Rm / cpm) * scratch.interior
            model.specific_energy.interior.copy_(cpm * T + c.gravitational_acceleration * z)
            model.energy_density.interior.copy_(ρc * model.specific_energy.interior)
        elif key == "θ" or key == "e":
            model.potential_temperature.set_interior(value)
            model.potential_temperature_density.interior.copy_(ρc * model.potential_temperature.interior)
        elif key == "ρθ" or key == "ρe":
            model.potential_temperature_density.set_interior(value)
        elif key == "q":
            model.specific_moisture.set_interior(value)
            model.moisture_density.interior.copy_(ρc * model.specific_moisture.interior)
        elif key == "ρq":
            model.moisture_density.set_interior(value)
        elif key in ("qcl", "qr"):          # settable specific microphysical names (set_atmosphere_model.jl:247-253)
            if not getattr(model, "_kessler", False):
                raise ValueError(f"Cannot set! {name}: the model has no Kessler microphysics")
            # only ρq is set (set!(ρμ, value); set!(ρμ, ρ * ρμ)); the diagnostic field is refreshed by update_state!
            dens = model.microphysical_fields["ρqᶜˡ" if key == "qcl" else "ρqʳ"]
            dens.set_interior(value)
            dens.interior.copy_(ρc * dens.interior)
        elif key in ("u", "v"):
            model.velocities[key].set_interior(value)
            model.momentum["ρ" + key].interior.copy_(ρc * model.velocities[key].interior)
        elif key == "w":
            model.velocities["w"].set_interior(value)
            model.momentum["ρw"].interior.copy_(ρf * model.velocities["w"].interior)
        else:   # ρu, ρv, ρw
            model.momentum[key].set_interior(value)
    if hasattr(model, "_finish_set"):      # y-slab models: update_state! + exchanges + the distributed projection, inside the library
        model._finish_set(enforce_mass_conservation)
        return
    update_state_(model, compute_tendencies=False)
    if enforce_mass_conservation:
        enforce_mass_conservation_(model)
    if balancer is not None and balancer is not False:
        from .balance import balance_adiabatically_
        balance_adiabatically_(model, balancer)


def _set_kinematic(model, **kw):
    """set!(model; kw...) of a kinematic model: θ / ρθ, qᵗ / ρqᵗ, the tracers by name (their density fields, set_atmosphere_model.jl:236-238)
    and the velocities u, v, w (kinematic_driver_time_stepping.jl:28-42).  Momentum cannot be set; nothing is projected."""
    import torch
    g = model.grid
    ref = model.dynamics.reference_state
    Hz, Nz = g.Hz, g.Nz
    ρc = torch.from_numpy(ref.density[Hz:Hz + Nz].copy()).to(model.device)[:, None, None]
    velocities_set = False
    for name, value in sorted(kw.items(), key=lambda kv: 0 if _ALIASES.get(kv[0]) in ("q", "ρq") else 1):
        tracer = str(name).lstrip(":")
        if tracer in model.tracers or (tracer.startswith("ρ") and tracer[1:] in model.tracers):
            model.tracers[tracer if tracer in model.tracers else tracer[1:]].set_interior(value)
            continue
        key = _ALIASES.get(name)
        if key in ("ρu", "ρv", "ρw"):
            raise ValueError(f"Cannot set momentum component '{name}' of a KinematicModel.")
        if key in ("u", "v", "w"):
            model.velocities[key].set_interior(value)
            velocities_set = True
        elif key == "θ":
            model.potential_temperature.set_interior(value)
            model.potential_temperature_density.interior.copy_(ρc * model.potential_temperature.interior)
        elif key == "ρθ":
            model.potential_temperature_density.set_interior(value)
        elif key == "q":
            model.specific_moisture.set_interior(value)
            model.moisture_density.interior.copy_(ρc * model.specific_moisture.interior)
        elif key == "ρq":
            model.moisture_density.set_interior(value)
        elif key in ("T", "ℋ", "e", "ρe", "qcl", "qr"):
            raise NotImplementedError(f"set!(model; {name}) is not implemented for AtmosphereModel(dynamics = PrescribedDynamics(...))")
        else:
            raise ValueError(f"Cannot set! {name} in AtmosphereModel because {name} is neither a prognostic "
                             "variable, a settable thermodynamic variable, nor a settable diagnostic variable!")
    if velocities_set:
        # default boundary conditions: the faces k = 1 and k = Nz + 1 of w are impenetrable — zeros, as the halo fill of a wall-normal face
        # field leaves them; u, v, w get their periodic images.  Then the library is told that the velocities changed (∇·(ρU) is re-formed)
        w = model.velocities["w"].parent
        w[Hz].zero_()
        w[Hz + Nz].zero_()
        fill_halo_regions_(model, model.velocities["u"], kind=2 | 8)
        fill_halo_regions_(model, model.velocities["v"], kind=2 | 4)
        fill_halo_regions_(model, model.velocities["w"], kind=1)
        model._check(model._lib.bz_set_prescribed_dynamics(model._ctx, 1 if model.dynamics.divergence_correction else 0),
                     "bz_set_prescribed_dynamics")
    update_state_(model, compute_tendencies=False)


def compute_kinematic_tendencies_(model):
    """Gⁿ of every scalar of a kinematic model, G = −∇·(ρU c) [+ c ∇·(ρU)], from the fields of the last update_state!."""
    model._check(model._lib.bz_compute_kinematic_tendencies(model._ctx, C.byref(model._state), C.byref(model._G)),
                 "bz_compute_kinematic_tendencies")


def _kinematic_time_steps(model, Δt, n, diagnose_last=True):
    """n × time_step!(model, Δt) of a kinematic model (ssp_runge_kutta_3.jl:209-278 with the projection calls doing nothing)."""
    n = int(n)
    if n <= 0:
        return
    if model.clock.iteration == 0:       # maybe_prepare_first_time_step!
        update_state_(model, compute_tendencies=False)      # (the stage kernel evaluates the tendencies itself)
    model._check(model._lib.bz_time_steps_kinematic(model._ctx, C.byref(model._state), C.byref(model._U0), C.byref(model._G),
                                                    float(Δt), n, 1 if diagnose_last else 0), "bz_time_steps_kinematic")
    model.clock.time += n * Δt
    model.clock.last_Δt = float(Δt)
    model.clock.iteration += n


def time_step_(model, Δt, whole_step=True):
    """time_step!(model, Δt) with SSP-RK3.  whole_step=True uses the single-call device-resident seam
    (bz_time_step_anelastic); False replays the reference's call sequence through the per-operator
    entry points (same kernels, used by the parity tests)."""
    if getattr(model, "_kinematic", False):
        return _kinematic_time_steps(model, Δt, 1)
    if model.clock.iteration == 0:       # maybe_prepare_first_time_step!
        update_state_(model, compute_tendencies=True)
    fv = getattr(model, "filtered_velocities", None)
    if fv is not None and not model._surface_filter_initialized:      # initialize!(model), after set!
        model.initialize_()
    if whole_step:
        model._check(model._lib.bz_time_step_anelastic(model._ctx, C.byref(model._state), C.byref(model._U0),
                                                       C.byref(model._G), float(Δt)), "bz_time_step_anelastic")
    else:
        store_initial_state_(model)
        for stage, α in enumerate((1.0, 1.0 / 4.0, 2.0 / 3.0), start=1):
            compute_flux_bc_tendencies_(model)
            ssp_rk3_substep_(model, Δt, α)
            implicit_step_(model, α * Δt)      # ssp_runge_kutta_3.jl:124-161 (a no-op without a vertically implicit closure)
            compute_pressure_correction_(model, α * Δt)
            make_pressure_correction_(model, α * Δt)
            update_state_(model, compute_tendencies=True)
            if fv is not None and stage in fv.update_stages:      # update_boundary_conditions! inside update_state!
                model.update_filtered_surface_state_(Δt)
        if getattr(model, "_kessler", False):
            from .microphysics import microphysics_model_update_
            microphysics_model_update_(model.microphysics, model, Δt=Δt)
    model.clock.time += Δt
    model.clock.last_Δt = float(Δt)
    model.clock.iteration += 1


def many_time_steps_(model, Δt, n, diagnose_last=True):
    """many_time_steps!(model, Δt, n) of the reference's benchmark driver through the multi-step seam."""
    if getattr(model, "_kinematic", False):
        return _kinematic_time_steps(model, Δt, n, diagnose_last)
    n = int(n)
    if n <= 0:
        return
    if model.clock.iteration == 0:       # maybe_prepare_first_time_step!
        update_state_(model, compute_tendencies=True)
    if getattr(model, "filtered_velocities", None) is not None and not model._surface_filter_initialized:
        model.initialize_()
    model._check(model._lib.bz_time_steps_anelastic(model._ctx, C.byref(model._state), C.byref(model._U0), C.byref(model._G),
                                                    float(Δt), n, 1 if diagnose_last else 0), "bz_time_steps_anelastic")
    model.clock.time += n * Δt
    model.clock.last_Δt = float(Δt)
    model.clock.iteration += n


def diagnostics_stale(model):
    return bool(model._lib.bz_diagnostics_stale(model._ctx))


def cell_advection_timescale(model, formulation="ThreeDimensional"):
    """cell_advection_timescale(model) (src/AtmosphereModels/cell_advection_timescale.jl:47-66): the TimeStepWizard's
    advective timescale min 1/(|u|/Δx + |v|/Δy + |w|/Δz); formulation "Horizontal" drops the vertical term."""
    if diagnostics_stale(model):      # the velocities are diagnostics: rebuild them after undiagnosed steps (time_steps(..., diagnose_last=False))
        model._refresh_diagnostics()
    out = model._T.real()
    w = None if str(formulation).startswith("Horizontal") else C.c_void_p(model.velocities["w"].ptr())
    model._check(model._lib.bz_cell_advection_timescale(model._ctx, C.c_void_p(model.velocities["u"].ptr()),
                                                        C.c_void_p(model.velocities["v"].ptr()), w, C.byref(out)),
                 "bz_cell_advection_timescale")
    return out.value


def nan_checker(model):
    """default_nan_checker(model): NaN check of the first prognostic field (atmosphere_model.jl:561-572)."""
    name, field = next(iter(model.prognostic_fields().items()))
    out = C.c_int32()
    model._check(model._lib.bz_any_nan(model._ctx, C.c_void_p(field.ptr()), 1 if field.zface else 0, C.byref(out)), "bz_any_nan")
    return bool(out.value)
