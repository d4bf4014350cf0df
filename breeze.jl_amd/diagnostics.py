"""Output diagnostics on the device: the operations the reference's examples build after the model — `RelativeHumidity(model)`,
`PotentialTemperature(model)`, `Average(..., dims=(1, 2))`, ... (src/AtmosphereModels/Diagnostics/, src/Microphysics/
microphysics_diagnostics.jl) — behind bz_compute_diagnostics / bz_horizontal_average of include/breeze_hip.h.

    ℋ = RelativeHumidity(model).compute()                       # a Field, halos filled
    θᵛ, θᵉ = compute_diagnostics(model, [VirtualPotentialTemperature(model), EquivalentPotentialTemperature(model)])   # one launch
    profile = Average(RelativeHumidity(model), dims=(1, 2)).compute()      # numpy, Nz values

    vθ = TangentialVelocity(model, center=(0, 0)).compute()     # (−y uᶜ + x vᶜ)/r at cell centres
    v̄θ = azimuthal_mean(vθ, radius=150e3, Nr=30)               # .data (Nr, Nz), .counts, .r, .z
    θ̄ = azimuthal_mean(LiquidIcePotentialTemperature(model), radius=150e3, Nr=30)      # same geometry: the ring plan is reused

Moisture fractions are picked from the model as grid_moisture_fractions does: no microphysics qᵛ = qᵗ and no liquid;
SaturationAdjustment the stored qᵛ, qˡ; Kessler qᵛ, qᶜˡ + qʳ.  Anelastic models read the reference-state columns; a compressible model
hands its own p and ρ fields to the potential temperatures and its dynamics.reference_state (required) to the other kinds.
"""
import ctypes as C

import numpy as np

from . import _lib
from .grids import Center
from .model import Field, fill_halo_regions_

_SPECIFIC_OR_DENSITY = ("specific", "density")


def _flavor(flavor, valid):
    flavor = str(flavor).lstrip(":")
    if flavor not in valid:      # the reference's ArgumentError
        raise ValueError(f"`flavor` must be one of {valid}, received {flavor!r}")
    return flavor


class _Operation:
    """A KernelFunctionOperation at (Center, Center, Center) of one model."""
    kind = None
    needs_saturation_pressure = False
    uses_model_pressure = False      # the potential temperatures: dynamics_pressure_for_potential_temperature

    def __init__(self, model):
        self.model = model
        self.code = _lib.BZ_DIAG[self.kind]

    def compute(self, out=None):
        """Evaluate into `out` (a centre Field of the model's grid; allocated when None) and fill its halos."""
        return compute_diagnostics(self.model, [self], out=None if out is None else [out])[0]

    def __repr__(self):
        return f"{type(self).__name__}(model)"


class _FlavoredPotentialTemperature(_Operation):
    uses_model_pressure = True

    def __init__(self, model, flavor="specific"):
        super().__init__(model)
        self.flavor = _flavor(flavor, _SPECIFIC_OR_DENSITY)
        if self.flavor == "density":
            self.code |= _lib.BZ_DIAG_DENSITY_WEIGHTED


class PotentialTemperature(_FlavoredPotentialTemperature):
    """θ = T / (p/pˢᵗ)^(Rᵐ/cᵖᵐ)"""
    kind = "POTENTIAL_TEMPERATURE"


class VirtualPotentialTemperature(_FlavoredPotentialTemperature):
    """θᵛ = T / (p/pˢᵗ)^(Rᵈ/cᵖᵈ) (1 + (Rᵛ/Rᵈ − 1) qᵛ − qˡ)"""
    kind = "VIRTUAL_POTENTIAL_TEMPERATURE"


class LiquidIcePotentialTemperature(_FlavoredPotentialTemperature):
    """θˡⁱ = θ (1 − ℒˡᵣ qˡ / (cᵖᵐ T))"""
    kind = "LIQUID_ICE_POTENTIAL_TEMPERATURE"


class EquivalentPotentialTemperature(_FlavoredPotentialTemperature):
    """θᵉ = T (pˢᵗ/p)^(Rᵈ/cᵖᵐ) exp(ℒˡ(T) qᵛ / (cᵖᵐ T)) ℋ^(−Rᵛ qᵛ / cᵖᵐ)"""
    kind = "EQUIVALENT_POTENTIAL_TEMPERATURE"
    needs_saturation_pressure = True


class StabilityEquivalentPotentialTemperature(_FlavoredPotentialTemperature):
    """θᵇ = θᵉ (T/Tᵣ)^(cˡ qˡ / cᵖᵐ)"""
    kind = "STABILITY_EQUIVALENT_POTENTIAL_TEMPERATURE"
    needs_saturation_pressure = True


class StaticEnergy(_Operation):
    """e = cᵖᵐ T + g z − ℒˡᵣ qˡ"""
    kind = "STATIC_ENERGY"

    def __init__(self, model, flavor="specific"):
        super().__init__(model)
        self.flavor = _flavor(flavor, _SPECIFIC_OR_DENSITY)
        if self.flavor == "density":
            self.code |= _lib.BZ_DIAG_DENSITY_WEIGHTED


class SaturationSpecificHumidity(_Operation):
    """qᵛ⁺ in one of three flavours: "prognostic" pᵛ⁺ / (ρ★ Rᵛ T) at the cell's own density, "equilibrium"
    equilibrium_saturation_specific_humidity(T, pᵣ, qᵛᵉ), "total_moisture" ϵ pᵛ⁺ / (pᵣ + (ϵ − 1) pᵛ⁺)."""
    needs_saturation_pressure = True
    _KINDS = {"prognostic": "SATURATION_SPECIFIC_HUMIDITY", "equilibrium": "SATURATION_SPECIFIC_HUMIDITY_EQUILIBRIUM",
              "total_moisture": "SATURATION_SPECIFIC_HUMIDITY_TOTAL_MOISTURE"}

    def __init__(self, model, flavor="prognostic"):
        self.flavor = _flavor(flavor, tuple(self._KINDS))
        self.kind = self._KINDS[self.flavor]
        super().__init__(model)


class RelativeHumidity(_Operation):
    """ℋ = pᵛ / max(pᵛ⁺(T), eps)"""
    kind = "RELATIVE_HUMIDITY"
    needs_saturation_pressure = True


class DewpointTemperature(_Operation):
    """T⁺ with pᵛ⁺(T⁺) = pᵛ: secant iteration, SecantSolver(reltol=1e-4, abstol=0, maxiter=10) scaled by pᵛ."""
    kind = "DEWPOINT_TEMPERATURE"
    needs_saturation_pressure = True


def _is_compressible(model):
    from .compressible import CompressibleAtmosphereModel
    return isinstance(model, CompressibleAtmosphereModel)


def _inputs(model, model_pressure):
    """bz_diagnostic_inputs of `model`; model_pressure: hand over the model's own p and ρ fields (compressible potential temperatures)."""
    T = model._T
    c = model.thermodynamic_constants
    μ = model.microphysical_fields
    I = T.bz_diagnostic_inputs()
    I.temperature = model.temperature.ptr()
    I.moisture = model.specific_moisture.ptr()
    if getattr(model, "_kessler", False):
        I.vapor, I.liquid, I.liquid_2 = μ["qᵛ"].ptr(), μ["qᶜˡ"].ptr(), μ["qʳ"].ptr()
    elif model.microphysics is not None:
        I.vapor, I.liquid = μ["qᵛ"].ptr(), μ["qˡ"].ptr()
    else:
        I.vapor = model.specific_moisture.ptr()
    if model_pressure:
        I.pressure, I.density = model.dynamics.pressure.ptr(), model.dynamics.total_density.ptr()
    I.liquid_latent_heat, I.liquid_heat_capacity = c.liquid_reference_latent_heat, c.liquid_heat_capacity
    I.energy_reference_temperature = c.energy_reference_temperature
    I.triple_point_temperature, I.triple_point_pressure = c.triple_point_temperature, c.triple_point_pressure
    return I


def _launch(model, ops, fields, model_pressure):
    T = model._T
    I = _inputs(model, model_pressure)
    n = len(ops)
    kinds = (C.c_int32 * n)(*[op.code for op in ops])
    outs = (C.c_void_p * n)(*[f.ptr() for f in fields])
    state = None if _is_compressible(model) else C.byref(model._state)      # bz_state: the call rebuilds stale diagnostics from it
    model._check(model._lib.bz_compute_diagnostics(model._ctx, state, C.byref(I), n, kinds, outs), "bz_compute_diagnostics")


def compute_diagnostics(model, operations, out=None):
    """Evaluate several operations of one model in one fused launch (the inputs are read once); returns their Fields, halos filled.
    On a compressible model the potential temperatures (own p, ρ) and the other kinds (reference state) are one launch each."""
    ops = list(operations)
    if not ops:
        return []
    if len(ops) > _lib.BZ_MAX_DIAGNOSTICS:
        raise ValueError(f"at most {_lib.BZ_MAX_DIAGNOSTICS} diagnostics per call")
    for op in ops:
        if not isinstance(op, _Operation):
            raise TypeError(f"{op!r} is not a diagnostic operation")
        if op.model is not model:
            raise ValueError("every operation must belong to `model`")
        formula = getattr(model.thermodynamic_constants, "saturation_vapor_pressure", None)
        if op.needs_saturation_pressure and formula is not None:
            raise NotImplementedError(f"{type(op).__name__}: the Clausius-Clapeyron saturation vapour pressure is implemented "
                                      f"(the model's constants carry {type(formula).__name__})")
    compressible = _is_compressible(model)
    if compressible and any(not op.uses_model_pressure for op in ops) and model.dynamics.reference_state is None:
        raise NotImplementedError("this CompressibleDynamics model has no reference_state: only the potential temperatures are defined")
    if out is None:
        out = [Field(model.grid, (Center, Center, Center), model.device) for _ in ops]
    if len(out) != len(ops):
        raise ValueError("one output field per operation")
    for f in out:
        if f.grid is not model.grid or f.zface or f.dtype != model.temperature.dtype:
            raise ValueError("outputs must be centre fields of the model's grid")
    if compressible:
        for own in (True, False):
            sel = [m for m, op in enumerate(ops) if op.uses_model_pressure == own]
            if sel:
                _launch(model, [ops[m] for m in sel], [out[m] for m in sel], own)
    else:
        _launch(model, ops, out, False)
    for f in out:
        fill_halo_regions_(model, f)
    return out


def horizontal_average(model, field):
    """Average(field, dims=(1, 2)) of one Field of the model: a numpy profile of Nz (z-face fields: Nz + 1) values."""
    if hasattr(field, "_fresh"):
        field._fresh()      # a stale diagnostic field of the model is rebuilt first
    nlev = model.grid.Nz + (1 if field.zface else 0)
    prof = np.empty(nlev, dtype=model._T.np_real)
    model._check(model._lib.bz_horizontal_average(model._ctx, C.c_void_p(field.ptr()), 1 if field.zface else 0,
                                                  prof.ctypes.data_as(C.POINTER(model._T.real))), "bz_horizontal_average")
    return prof


class Average:
    """Average(field_or_operation, dims=(1, 2)): the horizontal mean per level.  `model` is needed for a bare Field."""

    def __init__(self, operand, dims=(1, 2), model=None):
        if tuple(dims) != (1, 2):
            raise NotImplementedError("Average: dims = (1, 2) is implemented")
        self.operand, self.dims = operand, (1, 2)
        self.model = operand.model if isinstance(operand, _Operation) else model
        if self.model is None:
            owner = getattr(operand, "_owner", None)
            self.model = owner() if owner is not None else None
        if self.model is None:
            raise ValueError("Average(field): pass model=... for a field that does not know its model")

    def compute(self):
        field = self.operand.compute() if isinstance(self.operand, _Operation) else self.operand
        return horizontal_average(self.model, field)


# ---- azimuthal means and polar winds (csrc/bz_azimuthal.hip; src/AtmosphereModels/Diagnostics/azimuthal_mean.jl) ---------------------
MAX_RINGS, MAX_SUBCELLS = 1024, 16      # the limits of bz_azimuthal_mean (include/breeze_hip.h)


def _is_slab(model):
    from .compressible import SlabCompressibleModel
    from .distributed import LibrarySlabAtmosphereModel, SlabStepper
    return isinstance(model, (SlabCompressibleModel, LibrarySlabAtmosphereModel, SlabStepper))


def _resolve_model(operand, model, what):
    if isinstance(operand, (_Operation, _PolarVelocity)):
        return operand.model
    if model is None:
        owner = getattr(operand, "_owner", None)
        model = owner() if owner is not None else None
    if model is None:
        raise ValueError(f"{what}: pass model=... for a field that does not know its model")
    return model


def _horizontal_model(model, what):
    """The checks every polar operation makes on the host, before any device call."""
    if model.grid.topology[1] == "Flat":
        raise NotImplementedError(f"{what}: not defined on a Flat y")
    if _is_slab(model):
        raise NotImplementedError(f"{what}: not implemented on y-slab models (the rings span the ranks)")


def _set_nodes(model):
    """Hand the grid's own xᶜ, yᶜ to the context, once per model."""
    if getattr(model, "_horizontal_nodes", None) is None:
        T = model._T
        nodes = [np.ascontiguousarray(a, dtype=T.np_real) for a in (model.grid.xᶜ, model.grid.yᶜ)]
        model._check(model._lib.bz_set_horizontal_nodes(model._ctx, *[a.ctypes.data_as(C.POINTER(T.real)) for a in nodes]),
                     "bz_set_horizontal_nodes")
        model._horizontal_nodes = nodes


def _center(center):
    cx, cy = center
    return float(cx), float(cy)


class AzimuthalMean:
    """What azimuthal_mean returns: `.data` (Nr, nlev) as interior(c̄, :, 1, :), `.counts` samples per ring, `.r` ring centres, `.z`."""

    def __init__(self, data, counts, r, z):
        self.data, self.counts, self.r, self.z = data, counts, r, z

    def __repr__(self):
        return f"AzimuthalMean({self.data.shape[0]} rings × {self.data.shape[1]} levels)"


def azimuthal_mean(operand, radius, Nr, center=(0, 0), m=4, model=None):
    """azimuthal_mean(field_or_operation; radius, Nr, center=(0, 0), m=4): the mean over Nr uniform rings on [0, radius] about `center`, by
    binning m × m sub-cell centres per cell; a ring that catches no sample is NaN.  `model` is needed for a bare Field."""
    Nr, m, radius = int(Nr), int(m), float(radius)
    if not 1 <= Nr <= MAX_RINGS:
        raise ValueError(f"azimuthal_mean: Nr must be between 1 and {MAX_RINGS}, received {Nr}")
    if not 1 <= m <= MAX_SUBCELLS:
        raise ValueError(f"azimuthal_mean: m must be between 1 and {MAX_SUBCELLS}, received {m}")
    if not radius > 0 or not np.isfinite(radius):
        raise ValueError(f"azimuthal_mean: radius must be positive, received {radius}")
    cx, cy = _center(center)
    model = _resolve_model(operand, model, "azimuthal_mean")
    _horizontal_model(model, "azimuthal_mean")
    if isinstance(operand, (_Operation, _PolarVelocity)):      # evaluates to a centre field of the model's grid: nothing to validate
        field = operand.compute()
    else:
        field = operand
        if (not isinstance(field, Field) or field.grid is not model.grid or field.dtype != model.temperature.dtype
                or field.loc[0] is not Center or field.loc[1] is not Center):
            raise ValueError("azimuthal_mean: the field must be a Field at (Center, Center, ·) of the model's grid")
    if hasattr(field, "_fresh"):
        field._fresh()      # a stale diagnostic field of the model is rebuilt first
    _set_nodes(model)
    g, T = model.grid, model._T
    nlev = g.Nz + (1 if field.zface else 0)
    prof = np.empty((nlev, Nr), dtype=T.np_real)
    counts = np.empty(Nr, dtype=np.int64)
    model._check(model._lib.bz_azimuthal_mean(model._ctx, C.c_void_p(field.ptr()), 1 if field.zface else 0, cx, cy, radius, Nr, m,
                                              prof.ctypes.data_as(C.POINTER(T.real)), counts.ctypes.data_as(C.POINTER(C.c_int64))),
                 "bz_azimuthal_mean")
    Δr = radius / Nr
    return AzimuthalMean(prof.T, counts, Δr * (np.arange(Nr) + 0.5), np.asarray(g.zᶠ if field.zface else g.zᶜ))


class _PolarVelocity:
    """A wind component in polar coordinates about `center`, at (Center, Center, Center) of one model."""
    _slot = None

    def __init__(self, model, center=(0, 0)):
        _horizontal_model(model, type(self).__name__)
        self.model, self.center = model, _center(center)

    def compute(self, out=None):
        """Evaluate into `out` (a centre Field of the model's grid; allocated when None) and fill its halos."""
        model = self.model
        if out is None:
            out = Field(model.grid, (Center, Center, Center), model.device)
        if out.grid is not model.grid or out.zface or out.dtype != model.temperature.dtype:
            raise ValueError("the output must be a centre field of the model's grid")
        u, v = model.velocities["u"], model.velocities["v"]
        u._fresh()
        _set_nodes(model)
        ptrs = [None, None]
        ptrs[self._slot] = C.c_void_p(out.ptr())
        model._check(model._lib.bz_polar_winds(model._ctx, C.c_void_p(u.ptr()), C.c_void_p(v.ptr()), *self.center, *ptrs), "bz_polar_winds")
        fill_halo_regions_(model, out)
        return out

    def __repr__(self):
        return f"{type(self).__name__}(model, center={self.center})"


class TangentialVelocity(_PolarVelocity):
    """vθ = (−y uᶜ + x vᶜ)/r, (x, y) from `center`; NaN where a cell centre coincides with the centre, as the reference's Field."""
    _slot = 0


class RadialVelocity(_PolarVelocity):
    """vʳ = (x uᶜ + y vᶜ)/r"""
    _slot = 1
