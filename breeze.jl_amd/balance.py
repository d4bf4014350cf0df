"""Adiabatic initialisation (FV3 `na_init`): balance_adiabatically! and AdiabaticBalancer of the reference
(src/AtmosphereModels/adiabatic_balance.jl; Julia's `f!` is spelled `f_`).

An analysis carries ρ, ρu, ρv, ρθ and ρq but starts w at zero, so the nonhydrostatic state is out of balance with the rest and the first
minutes of a run ring.  Each cycle runs two symmetric excursions, 0 → +Δt → 0 and 0 → −Δt → 0, and after each nudges the initial fields —
every prognostic field but ρw — back towards their snapshot, x ← (x + weight·x₀) / (1 + weight); ρw keeps what the excursions imprint.

Two layers, as in the reference:
  balance_adiabatically_(model, Δt=..., cycles=1, weight=2)   the loop on the model as given (the caller passes a stripped model); one C call
                                                               (bz_balance_adiabatically_compressible / _anelastic, csrc/bz_adiabatic_balance.hip)
  balance_adiabatically_(model, AdiabaticBalancer(...) | True | False), set_(model, ..., balancer=...)
                                                               the same loop on a stripped TWIN context that steps the production model's
                                                               own arrays in place: same grid, constants, reference, advection and time
                                                               discretisation; no sponge, microphysics, closure, forcing, Relaxation or
                                                               surface flux; Coriolis stays.  The production context is not touched.
"""
import ctypes as C
import math

import numpy as np

from . import _context, _lib
from .grids import Bounded
from .model import AtmosphereModel, Clock, fill_halo_regions_
from .thermodynamics import dry_air_gas_constant

ACOUSTIC_CFL_SAFETY = 0.85      # acoustic_cfl_safety (adiabatic_balance.jl:139)


class DefaultTimeStepping:
    """Sentinel of AdiabaticBalancer's default `time_stepping`: in the reference the fully explicit twin of CompressibleDynamics, which this
    library does not have — on CompressibleDynamics the default is refused by name (pass time_stepping=None); AnelasticDynamics ignores it."""


class AdiabaticBalancer:
    """AdiabaticBalancer(Δt=None, cycles=1, weight=2, with_moisture=True, time_stepping=DefaultTimeStepping()) (adiabatic_balance.jl:126-136).
    Δt None: 0.85 Δz_min / sqrt(γᵈ Rᵈ max T); with_moisture False: the moisture density is saved before the balance and restored after it;
    time_stepping None: the model's own split-explicit scheme without its sponge (CompressibleDynamics only; ignored by AnelasticDynamics)."""

    def __init__(self, Δt=None, cycles=1, weight=2, with_moisture=True, time_stepping=DefaultTimeStepping()):
        if Δt is not None:
            Δt = float(Δt)
            if not math.isfinite(Δt) or Δt == 0.0:
                raise ValueError(f"`Δt` must be finite and non-zero, or None (got {Δt})")
        if isinstance(cycles, bool) or int(cycles) != cycles or int(cycles) < 1:
            raise ValueError(f"`cycles` must be a positive integer (got {cycles})")
        weight = float(weight)
        if not math.isfinite(weight) or weight <= -1.0:
            raise ValueError(f"`weight` must be finite and greater than -1 (got {weight})")
        if not isinstance(with_moisture, (bool, np.bool_)):
            raise TypeError("`with_moisture` must be a Bool")
        self.Δt, self.cycles, self.weight = Δt, int(cycles), weight
        self.with_moisture, self.time_stepping = bool(with_moisture), time_stepping


# ---- what runs where ------------------------------------------------------------------------------------------------------------------
def _is_compressible(model):
    from .compressible import CompressibleAtmosphereModel
    return isinstance(model, CompressibleAtmosphereModel)


def require_balance_scope(model, what="balance_adiabatically!"):
    """The single-device anelastic AtmosphereModel on (Periodic, Periodic | Flat, Bounded) and the single-device CompressibleAtmosphereModel
    that is periodic in x and y or has a Flat y.  Everything else is refused by name, before anything touches the device."""
    if any("Slab" in k.__name__ for k in type(model).__mro__):
        raise NotImplementedError(f"{what}: not implemented on y-slab (distributed) models")
    if not isinstance(model, AtmosphereModel) and not _is_compressible(model):
        raise TypeError(f"{what}: `model` must be an AtmosphereModel or a CompressibleAtmosphereModel")
    if getattr(model, "_kinematic", False):
        raise NotImplementedError(f"{what}: not implemented on the kinematic driver (AtmosphereModel(dynamics = PrescribedDynamics(...)) has "
                                  "no vertical momentum to spin up)")
    if Bounded in tuple(model.grid.topology[:2]):
        raise NotImplementedError(f"{what}: not implemented on a model between walls (Bounded x / Bounded y)")


def require_balance_model(model, balancer, what="balance_adiabatically!"):
    """require_balance_scope and, for an AdiabaticBalancer (or True) on CompressibleDynamics, its `time_stepping`."""
    require_balance_scope(model, what)
    if balancer is True:
        balancer = AdiabaticBalancer()
    if not isinstance(balancer, AdiabaticBalancer):
        if balancer is False or balancer is None:
            return None
        raise TypeError(f"{what}: `balancer` must be an AdiabaticBalancer or a Bool")
    if _is_compressible(model):
        if balancer.with_moisture:      # the twin steps the moisture with the vapour-only thermodynamics; its closing update_state! would re-partition it
            from ._context import refuse_mixed_phase
            refuse_mixed_phase(getattr(model, "microphysics", None), f"{what} (with_moisture = true)", "the balance of the moisture-carrying compressible state is "
                               "checked against the warm-phase adjustment only; pass with_moisture=False")
        ts = balancer.time_stepping
        if isinstance(ts, DefaultTimeStepping):
            raise NotImplementedError(f"{what}: the default time_stepping of AdiabaticBalancer is the fully explicit twin "
                                      "(CompressibleDynamics(ExplicitTimeStepping())), which is not built; pass time_stepping=None to "
                                      "balance with the model's own split-explicit scheme without its sponge")
        if ts is not None:
            raise NotImplementedError(f"{what}: time_stepping = {type(ts).__name__} is not implemented (ExplicitTimeStepping and swapped-in "
                                      "time discretisations are not built); pass time_stepping=None")
    return balancer


# ---- the initial fields ---------------------------------------------------------------------------------------------------------------
def initial_fields(model):
    """The fields nudged back towards the analysis: every prognostic field but ρw (adiabatic_balance.jl:72) — compressible (ρᵈ, ρu, ρv, ρθ,
    ρq), anelastic (ρu, ρv, ρθ | ρe, ρq, tracers...).  The species of a Kessler model are not among them: the balance runs without
    microphysics and neither steps nor nudges them."""
    return [f for k, f in model.prognostic_fields().items() if k not in ("ρw", "ρqᶜˡ", "ρqʳ")]


def snapshot_initial_fields(model):
    """Copies of the initial fields' whole parent arrays, halos included (adiabatic_balance.jl:75)."""
    return [f.parent.clone() for f in initial_fields(model)]


def _nudge(owner, fields, snapshot, weight):
    n = len(fields)
    ptrs = (C.c_void_p * n)(*[f.ptr() for f in fields])
    snaps = (C.c_void_p * n)(*[x0.data_ptr() for x0 in snapshot])
    count = (C.c_int64 * n)(*[f.parent.numel() for f in fields])
    owner._check(owner._lib.bz_nudge_fields(owner._ctx, n, ptrs, snaps, count, float(weight)), "bz_nudge_fields")


def nudge_initial_fields_(model, snapshot, weight):
    """x ← (x + weight·x₀) / (1 + weight) over the whole parent array of every initial field, in the grid's precision, then its halo fill
    (adiabatic_balance.jl:78-86): one launch for all fields (bz_nudge_fields)."""
    fields = initial_fields(model)
    if len(snapshot) != len(fields):
        raise ValueError(f"the snapshot holds {len(snapshot)} arrays, the model has {len(fields)} initial fields")
    for f, x0 in zip(fields, snapshot):
        if tuple(x0.shape) != tuple(f.parent.shape) or x0.dtype != f.parent.dtype or x0.device != f.parent.device or not x0.is_contiguous():
            raise ValueError("every snapshot array must be a contiguous copy of its field's parent array (snapshot_initial_fields)")
    _nudge(model, fields, snapshot, weight)
    for f in fields:
        fill_halo_regions_(model, f, 0)


# ---- Δt -------------------------------------------------------------------------------------------------------------------------------
def resolve_balance_Δt(balancer, model):
    """The balancer's Δt, or 0.85 Δz_min / sqrt(γᵈ Rᵈ max T) in the grid's precision (adiabatic_balance.jl:138-156): the vertical acoustic
    CFL on the thinnest layer with the warmest temperature of the model, taken by a reduction on the device."""
    Δt = balancer.Δt if isinstance(balancer, AdiabaticBalancer) else balancer
    if Δt is not None:
        return float(Δt)
    from .model import diagnostics_stale
    if hasattr(model, "_refresh_diagnostics") and diagnostics_stale(model):
        model._refresh_diagnostics()
    c = model.thermodynamic_constants
    Rd, cpd = dry_air_gas_constant(c), c.dry_air_heat_capacity
    γd = cpd / (cpd - Rd)
    Tmax = float(model.temperature.interior.max().item())
    Δz_min = float(np.min(np.diff(np.asarray(model.grid.zᶠ, dtype=np.float64))))
    return float(np.dtype(model._T.np_real).type(ACOUSTIC_CFL_SAFETY * Δz_min / math.sqrt(γd * Rd * Tmax)))


# ---- the loop -------------------------------------------------------------------------------------------------------------------------
def _update_state(owner, model, compressible):
    """update_state!(model) with tendencies through the context of `owner` on the arrays of `model`."""
    if compressible:
        owner._check(owner._lib.bz_compressible_update_state(owner._ctx, C.byref(model._state), C.byref(model._G), C.byref(model._sub), 1),
                     "bz_compressible_update_state")
    else:
        owner._check(owner._lib.bz_update_state(owner._ctx, C.byref(model._state), C.byref(model._G), 1), "bz_update_state")


def _run_balance(owner, model, clock, Δt, cycles, weight):
    """balance_adiabatically!(model; Δt, cycles, weight) (adiabatic_balance.jl:44-66) through the context of `owner` on the arrays of `model`;
    `clock` is the clock of whoever steps (the model's own, or the twin's fresh one) and is fully reset on exit."""
    compressible = _is_compressible(model)
    st = C.byref(model._state)
    if clock.iteration == 0:       # maybe_prepare_first_time_step! of the first excursion
        if compressible:
            owner._check(owner._lib.bz_seed_time_averaged_velocities(owner._ctx, st, C.byref(model._sub)), "bz_seed_time_averaged_velocities")
        _update_state(owner, model, compressible)
    if compressible:
        rc = owner._lib.bz_balance_adiabatically_compressible(owner._ctx, st, C.byref(model._U0), C.byref(model._G), C.byref(model._sub),
                                                              float(Δt), int(cycles), float(weight), 1)
        owner._check(rc, "bz_balance_adiabatically_compressible")
    else:
        rc = owner._lib.bz_balance_adiabatically_anelastic(owner._ctx, st, C.byref(model._U0), C.byref(model._G), float(Δt), int(cycles),
                                                           float(weight), 1)
        owner._check(rc, "bz_balance_adiabatically_anelastic")
    clock.time, clock.iteration, clock.last_Δt = 0.0, 0, float("inf")      # reset!(model.clock)


# ---- the twin -------------------------------------------------------------------------------------------------------------------------
class _TwinContext(_context.ContextOwner):
    """A stripped context on the production model's grid, constants, reference, advection and time discretisation.  It owns no field: every
    call takes the production model's argument structs, so it steps the production arrays in place.  close() destroys it."""

    def __init__(self, model):
        self._lib, self._T, self.device = model._lib, model._T, model.device
        self.clock = Clock()
        T, grid, c = model._T, model.grid, model.thermodynamic_constants
        bg, self._zf = _context.grid_struct(T, grid)
        bc = _context.constants_struct(T, c)
        if _is_compressible(model):
            from .compressible import _exner_reference_struct, _split_explicit_struct
            br, self._ref_arrays = _exner_reference_struct(T, model.dynamics)
            bt = _split_explicit_struct(T, grid, model.dynamics.time_discretization, model.temperature_solver,
                                        model.timestepper.substepper.substep_floattype, sponge=False)
            self._create = lambda lib: lib.bz_create_compressible(C.byref(self._ctx), C.byref(bg), C.byref(bc), C.byref(br), C.byref(bt),
                                                                  model.advection.order)
            self._open_context("bz_create_compressible (adiabatic twin)")
            if model.coriolis is not None:
                Fc = T.bz_column_forcings()
                Fc.coriolis_f = model.coriolis.f
                self._check(self._lib.bz_set_forcings(self._ctx, C.byref(Fc)), "bz_set_forcings")
            return
        br, self._ref_arrays = _context.reference_struct(T, model.dynamics.reference_state)
        self._create = lambda lib: lib.bz_create(C.byref(self._ctx), C.byref(bg), C.byref(bc), C.byref(br), model.advection.order)
        self._open_context("bz_create (adiabatic twin)")
        lib = self._lib
        if model.formulation == "StaticEnergy":
            self._check(lib.bz_set_formulation(self._ctx, 1), "bz_set_formulation")
        if model._scalar_order != model.advection.order:
            self._check(lib.bz_set_scalar_advection_order(self._ctx, model._scalar_order), "bz_set_scalar_advection_order")
        if model.tracers:
            arr = (_lib.bz_tracer_fields * len(model.tracers))()
            for t, n in enumerate(model.tracers):
                arr[t].density, arr[t].specific = model.tracers[n].ptr(), model.specific_tracers[n].ptr()
                arr[t].U0, arr[t].G = model.U0[n].ptr(), model.G[n].ptr()
            self._check(lib.bz_set_tracers(self._ctx, len(model.tracers), arr), "bz_set_tracers")
        ba = model._bounded_advection
        if ba is not None and (ba["moisture"] or ba["tracers"]):      # the advection schemes are the model's (its species are not stepped)
            bs = T.bz_bounds_preserving_advection(ba["lower"], ba["upper"], ba["moisture"], 0, ba["tracers"], 0)
            self._check(lib.bz_set_bounds_preserving_advection(self._ctx, C.byref(bs)), "bz_set_bounds_preserving_advection")
        if model.coriolis is not None:
            from .forcings import materialize_forcings
            F, self._forcing_keepalive = materialize_forcings(grid, model.coriolis, None, None, T)
            self._check(lib.bz_set_forcings(self._ctx, C.byref(F)), "bz_set_forcings")

    def _create_context(self, lib):
        return self._create(lib)

    def close(self):
        if self._ctx:
            self._lib.bz_sync(self._ctx)
            self._lib.bz_destroy(self._ctx)
            self._ctx = None


# ---- the public function ----------------------------------------------------------------------------------------------------------------
def balance_adiabatically_(model, balancer=None, Δt=None, cycles=1, weight=2):
    """balance_adiabatically!(model; Δt, cycles, weight): the loop on the model as given — pass a model built without microphysics, sponge,
    closure and forcing; its clock is fully reset (time 0, iteration 0, last_Δt inf).
    balance_adiabatically!(model, balancer): `balancer` an AdiabaticBalancer, True (the defaults) or False (a no-op): the loop on a stripped
    twin context that shares the model's fields, closed by update_state! of the model; the model's clock, context, attachments and
    recorded steps are left alone.  Returns the model."""
    if balancer is False:
        return model
    if balancer is None:
        require_balance_scope(model)
        if Δt is None:
            raise TypeError("balance_adiabatically!(model; Δt, cycles = 1, weight = 2): `Δt` is required (or pass an AdiabaticBalancer)")
        given = AdiabaticBalancer(Δt=Δt, cycles=cycles, weight=weight)      # the same argument checks
        _run_balance(model, model, model.clock, given.Δt, given.cycles, given.weight)
        return model
    balancer = require_balance_model(model, balancer)
    compressible = _is_compressible(model)
    step = resolve_balance_Δt(balancer, model)
    ρq0 = None if balancer.with_moisture else model.moisture_density.parent.clone()
    twin = _TwinContext(model)
    try:
        _update_state(twin, model, compressible)      # update_state!(twin)
        _run_balance(twin, model, twin.clock, step, balancer.cycles, balancer.weight)
    finally:
        twin.close()
    if ρq0 is not None:
        model.moisture_density.parent.copy_(ρq0)
    _update_state(model, model, compressible)      # update_state!(model)
    return model
