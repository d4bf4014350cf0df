"""Host-side mirror of Breeze.Microphysics.SaturationAdjustment (src/Microphysics/saturation_adjustment.jl:20-60) and the
solver vocabulary of Breeze.Solvers (src/Solvers.jl:55-136): warm-phase and mixed-phase equilibrium with the secant iteration."""


class WarmPhaseEquilibrium:
    pass


class MixedPhaseEquilibrium:
    """MixedPhaseEquilibrium(; freezing_temperature=273.15, homogeneous_ice_nucleation_temperature=233.15)
    (src/Thermodynamics/vapor_saturation.jl:146-176): the equilibrium liquid fraction of the condensate falls linearly from 1 at Tᶠ to 0 at Tʰ."""

    def __init__(self, freezing_temperature=273.15, homogeneous_ice_nucleation_temperature=233.15):
        if freezing_temperature < homogeneous_ice_nucleation_temperature:
            raise ValueError("`freezing_temperature` must be greater than `homogeneous_ice_nucleation_temperature`")
        if freezing_temperature == homogeneous_ice_nucleation_temperature:
            # the reference accepts this and divides 0 by 0 in equilibrated_surface: λ = (clamp(T, Tʰ, Tᶠ) - Tʰ) / (Tᶠ - Tʰ)
            raise ValueError("`freezing_temperature` must be greater than `homogeneous_ice_nucleation_temperature`: with equal temperatures the "
                             "liquid fraction (T - Tʰ) / (Tᶠ - Tʰ) is 0 / 0")
        self.freezing_temperature = float(freezing_temperature)
        self.homogeneous_ice_nucleation_temperature = float(homogeneous_ice_nucleation_temperature)


class SecantSolver:
    def __init__(self, reltol=0, abstol=1e-4, maxiter=20):
        if reltol != 0:
            raise NotImplementedError("SecantSolver(reltol != 0) is not implemented in the HIP path")
        self.reltol, self.abstol, self.maxiter = 0.0, float(abstol), int(maxiter)


class SaturationAdjustment:
    """SaturationAdjustment(; solver = SecantSolver(abstol=1e-4, maxiter=20), equilibrium = MixedPhaseEquilibrium())
    (saturation_adjustment.jl:55-70).  The mixed-phase equilibrium runs on the single-device anelastic AtmosphereModel (pressure form: qᵛ⁺ at
    the reference pressure) and on the single-device CompressibleAtmosphereModel that is periodic in x and y or Flat in y (density form,
    saturation_adjustment.jl:241-293: qᵛ⁺ = pᵛ⁺ / (ρ Rᵛ T) at the cell's own density, inside update_state! and the fused stage epilogue); both
    diagnose microphysical_fields["qⁱ"] beside qᵛ and qˡ.  The anelastic model takes the equilibrium in its constructor; the compressible
    constructor attaches the warm-phase adjustment and refuses the mixed one by name, and compressible.set_mixed_phase_equilibrium_(model,
    MixedPhaseEquilibrium(...)) attaches the mixed form to the built model.  Slab, walled and kinematic models, bulk surface fluxes, TetensFormula constants,
    set!(T | ℋ), the diagnostics operations and the hydrostatic balances refuse it by name."""

    def __init__(self, solver=None, equilibrium=None):
        if equilibrium is None:
            equilibrium = MixedPhaseEquilibrium()
        if not isinstance(equilibrium, (WarmPhaseEquilibrium, MixedPhaseEquilibrium)):
            raise NotImplementedError("the HIP path implements SaturationAdjustment(equilibrium = WarmPhaseEquilibrium() | MixedPhaseEquilibrium())")
        self.equilibrium = equilibrium
        self.solver = solver or SecantSolver()

    @property
    def mixed_phase(self):
        return isinstance(self.equilibrium, MixedPhaseEquilibrium)


class InstantaneousPrecipitation:
    """InstantaneousPrecipitation(; equilibrium = WarmPhaseEquilibrium(), solver = SecantSolver()) (src/Microphysics/
    instantaneous_precipitation.jl:39-55): the Reed–Jablonowski large-scale condensation.  It wraps a SaturationAdjustment
    (`saturation_adjustment`); once per step the vapour above saturation condenses at the cell's own density, its latent heat stays in the air
    and the condensate leaves as precipitation.  The prognostic moisture is ρqᵛ; there are no condensate fields.  CompressibleDynamics only."""

    def __init__(self, equilibrium=None, solver=None):
        if isinstance(equilibrium, MixedPhaseEquilibrium):
            raise NotImplementedError("InstantaneousPrecipitation(equilibrium = MixedPhaseEquilibrium()): the rain-out kernel runs the warm-phase "
                                      "density-based adjustment (it has no ice to precipitate); WarmPhaseEquilibrium() is implemented")
        self.saturation_adjustment = SaturationAdjustment(solver=solver, equilibrium=WarmPhaseEquilibrium() if equilibrium is None else equilibrium)


# ---------------------------------------------------------------------------------------------------------------------
# BulkMicrophysics and its negative moisture correction (src/Microphysics/bulk_microphysics.jl:26-40,208-265,
# src/AtmosphereModels/negative_moisture_correction.jl)
# ---------------------------------------------------------------------------------------------------------------------
class VerticalBorrowing:
    """VerticalBorrowing() (negative_moisture_correction.jl:45-60): a cell of the moisture prognostic with qᵛ < 0 is filled from the cell below
    (top to bottom, the mass deficit carried down the column), then the bottom cell borrows from the one above it."""


class SpeciesBorrowing:
    """SpeciesBorrowing(; vertical_borrowing = nothing) (negative_moisture_correction.jl:62-90): at every level a negative species borrows from the
    next lighter one, the lightest from the moisture prognostic; optionally followed by the vertical redistribution.  The non-precipitating
    scheme has no species: SpeciesBorrowing() alone has nothing to do."""

    def __init__(self, vertical_borrowing=None):
        if vertical_borrowing is not None and not isinstance(vertical_borrowing, VerticalBorrowing):
            raise TypeError("SpeciesBorrowing(vertical_borrowing = ...): nothing or VerticalBorrowing()")
        self.vertical_borrowing = vertical_borrowing


class NonEquilibriumCloudFormation:
    """NonEquilibriumCloudFormation(liquid, ice = nothing) (bulk_microphysics.jl:73-80): prognostic cloud condensate.  A name the host mirror
    knows in order to refuse it: no model here runs it."""

    def __init__(self, liquid=None, ice=None):
        self.liquid, self.ice = liquid, ice


class BulkMicrophysics:
    """BulkMicrophysics(; categories = nothing, cloud_formation = SaturationAdjustment(), precipitation_boundary_condition = nothing,
    negative_moisture_correction = nothing) (bulk_microphysics.jl:208-265).  Without categories this is the reference's non-precipitating bulk
    scheme: the wrapped SaturationAdjustment (warm or mixed phase) with, optionally, the negative moisture correction at the head of every
    update_state!.  Runs on the single-device anelastic AtmosphereModel; every other model refuses it by name."""

    def __init__(self, categories=None, cloud_formation=None, precipitation_boundary_condition=None, negative_moisture_correction=None):
        if categories is not None:
            raise NotImplementedError("BulkMicrophysics(categories = ...): precipitating categories (the CloudMicrophysics extension) are not "
                                      "implemented; categories = nothing is")
        if isinstance(cloud_formation, NonEquilibriumCloudFormation):
            raise NotImplementedError("BulkMicrophysics(cloud_formation = NonEquilibriumCloudFormation(...)) is not implemented; "
                                      "cloud_formation = SaturationAdjustment(...) is")
        if cloud_formation is None:
            cloud_formation = SaturationAdjustment()
        if not isinstance(cloud_formation, SaturationAdjustment):
            raise NotImplementedError("BulkMicrophysics(cloud_formation = ...): SaturationAdjustment(...) is implemented")
        if precipitation_boundary_condition is not None:
            raise NotImplementedError("BulkMicrophysics(precipitation_boundary_condition = ...): there are no precipitating categories whose "
                                      "sedimentation it would bound; precipitation_boundary_condition = nothing is implemented")
        if negative_moisture_correction is not None and not isinstance(negative_moisture_correction, (VerticalBorrowing, SpeciesBorrowing)):
            raise TypeError("BulkMicrophysics(negative_moisture_correction = ...): nothing, VerticalBorrowing() or SpeciesBorrowing(...)")
        self.cloud_formation = cloud_formation
        self.categories = None
        self.precipitation_boundary_condition = None
        self.negative_moisture_correction = negative_moisture_correction


def cloud_formation(microphysics):
    """The scheme that forms cloud: a BulkMicrophysics' cloud_formation, anything else is its own.  Every place that asks for the
    SaturationAdjustment, its solver or its equilibrium goes through here, so the wrapper is looked through everywhere alike."""
    return microphysics.cloud_formation if isinstance(microphysics, BulkMicrophysics) else microphysics


def vertical_borrowing(correction):
    """Whether a negative moisture correction redistributes vertically."""
    return isinstance(correction, VerticalBorrowing) or (isinstance(correction, SpeciesBorrowing) and correction.vertical_borrowing is not None)


# ---------------------------------------------------------------------------------------------------------------------
# DCMIP2016 Kessler warm-rain microphysics: the operator-split column update (src/Microphysics/dcmip2016_kessler.jl)
# ---------------------------------------------------------------------------------------------------------------------
class TetensFormula:
    """TetensFormula(; reference_saturation_vapor_pressure=610, reference_temperature=273.15, liquid_coefficient=17.27,
    liquid_temperature_offset=35.85, ...) (src/Thermodynamics/tetens_formula.jl:72-85); liquid surface only here."""

    def __init__(self, reference_saturation_vapor_pressure=610, reference_temperature=273.15, liquid_coefficient=17.27,
                 liquid_temperature_offset=35.85):
        self.reference_saturation_vapor_pressure = float(reference_saturation_vapor_pressure)
        self.reference_temperature = float(reference_temperature)
        self.liquid_coefficient = float(liquid_coefficient)
        self.liquid_temperature_offset = float(liquid_temperature_offset)


class DCMIP2016KesslerMicrophysics:
    """DCMIP2016KesslerMicrophysics(; ...) with the reference's defaults (dcmip2016_kessler.jl:154-169)."""

    DEFAULTS = dict(dcmip_temperature_scale=237.3, terminal_velocity_coefficient=36.34, density_scale=0.001,
                    terminal_velocity_exponent=0.1364, autoconversion_rate=0.001, autoconversion_threshold=0.001,
                    accretion_rate=2.2, accretion_exponent=0.875, evaporation_ventilation_coefficient_1=1.6,
                    evaporation_ventilation_coefficient_2=124.9, evaporation_ventilation_exponent_1=0.2046,
                    evaporation_ventilation_exponent_2=0.525, diffusivity_coefficient=2.55e8,
                    thermal_conductivity_coefficient=5.4e5, substep_cfl=0.8)

    def __init__(self, **kw):
        for k, v in self.DEFAULTS.items():
            setattr(self, k, float(kw.pop(k, v)))
        if kw:
            raise TypeError(f"unknown DCMIP2016KesslerMicrophysics parameters: {sorted(kw)}")


class KesslerMicrophysicalFields:
    """materialize_microphysical_fields(::DCMIP2016KesslerMicrophysics, grid, bcs) (dcmip2016_kessler.jl:255-290):
    prognostic rho q^cl, rho q^r and the diagnostic q^v, q^cl, q^r, W^r, precipitation_rate."""

    def __init__(self, model):
        import torch
        from .model import Field, _LOC
        g = model.grid
        # ASCII attribute names (Python normalises superscript identifiers): rho_qcl = ρqᶜˡ, rho_qr = ρqʳ, qv, qcl, qr, W = 𝕎ʳ
        for name in ("rho_qcl", "rho_qr", "qv", "qcl", "qr", "W"):
            setattr(self, name, Field(g, _LOC["ccc"], model.device))
        self.precipitation_rate = torch.zeros((g.Ny + 2 * g.Hy, g.Nx + 2 * g.Hx), dtype=self.qv.parent.dtype, device=model.device)      # eltype(grid): the Float32 library writes 4-byte reals


def kessler_parameter_struct(microphysics, constants, tetens=None, ftype=8):
    """bz_kessler_microphysics from DCMIP2016KesslerMicrophysics + the TetensFormula / liquid phase of the constants."""
    from . import _lib
    tf = tetens or getattr(constants, "saturation_vapor_pressure", None) or TetensFormula()
    P = _lib.types(ftype).bz_kessler_microphysics()
    for k in DCMIP2016KesslerMicrophysics.DEFAULTS:
        setattr(P, k, getattr(microphysics, k))
    P.tetens_reference_saturation_vapor_pressure = tf.reference_saturation_vapor_pressure
    P.tetens_reference_temperature = tf.reference_temperature
    P.tetens_liquid_coefficient = tf.liquid_coefficient
    P.tetens_liquid_temperature_offset = tf.liquid_temperature_offset
    P.liquid_latent_heat, P.liquid_heat_capacity = constants.liquid_reference_latent_heat, constants.liquid_heat_capacity
    return P


def microphysics_model_update_(microphysics, model, fields=None, Δt=None, tetens=None, density=None, pressure=None,
                               standard_pressure=None):
    """microphysics_model_update!(microphysics::DCMIP2016KesslerMicrophysics, model) (dcmip2016_kessler.jl:449-486) without
    the trailing update_state!: one launch of the column kernel.  `density` / `pressure`: 3-D Fields (compressible) or None
    for the anelastic reference columns of the model's context.
    microphysics_model_update!(microphysics::InstantaneousPrecipitation, model) (instantaneous_precipitation.jl:115-141): the rain-out kernel
    WITH the trailing update_state!; Δt = model.clock.last_Δt unless given; nothing happens for a Δt that is NaN, infinite or ≤ 0."""
    import ctypes as C
    from . import _lib
    if isinstance(microphysics, InstantaneousPrecipitation):
        Δt = model.clock.last_Δt if Δt is None else Δt
        model._check(model._lib.bz_instantaneous_precipitation_update(model._ctx, C.byref(model._state), C.byref(model._G), C.byref(model._sub),
                                                                      float(Δt)), "bz_instantaneous_precipitation_update")
        return
    if fields is None:          # the model owns the Kessler fields: microphysics_model_update!(microphysics, model)
        Δt = model.clock.last_Δt if Δt is None else Δt
        model._check(model._lib.bz_kessler_model_update(model._ctx, C.byref(model._state), C.byref(model._G), float(Δt)),
                     "bz_kessler_model_update")
        return
    P = kessler_parameter_struct(microphysics, model.thermodynamic_constants, tetens, ftype=getattr(model.grid, "ftype", 8))
    F = _lib.bz_kessler_fields()
    F.density = density.ptr() if density is not None else None
    F.pressure = pressure.ptr() if pressure is not None else None
    F.potential_temperature = model.potential_temperature.ptr()
    F.potential_temperature_density = model.potential_temperature_density.ptr()
    F.moisture_density = model.moisture_density.ptr()
    F.cloud_liquid_density, F.rain_density = fields.rho_qcl.ptr(), fields.rho_qr.ptr()
    F.vapor_mass_fraction, F.cloud_liquid_mass_fraction, F.rain_mass_fraction = fields.qv.ptr(), fields.qcl.ptr(), fields.qr.ptr()
    F.rain_terminal_velocity = fields.W.ptr()
    F.precipitation_rate = fields.precipitation_rate.data_ptr()
    if standard_pressure is None:
        ref = getattr(model.dynamics, "reference_state", None)
        standard_pressure = getattr(model.dynamics, "standard_pressure", None) or ref.standard_pressure
    model._check(model._lib.bz_kessler_microphysics_update(model._ctx, C.byref(P), C.byref(F), float(Δt), float(standard_pressure)),
                 "bz_kessler_microphysics_update")
