"""Output diagnostics on the device: the operations the reference's examples build after the model — `RelativeHumidity(model)`,
`PotentialTemperature(model)`, `Average(..., dims=(1, 2))`, ... (src/AtmosphereModels/Diagnostics/, src/Microphysics/
microphysics_diagnostics.jl) — behind bz_compute_diagnostics / bz_horizontal_average of include/breeze_hip.h.

    ℋ = RelativeHumidity(model).compute()                       # a Field, halos filled
    θᵛ, θᵉ = compute_diagnostics(model, [VirtualPotentialTemperature(model), EquivalentPotentialTemperature(model)])   # one launch
    profile = Average(RelativeHumidity(model), dims=(1, 2)).compute()      # numpy, Nz values

    u, v, w = model.velocities.values(); θ = model.potential_temperature; CCC = (Center, Center, Center)
    profiles = compute_averages(model, {"uw": Average(at(CCC, u * w)), "w³": Average(at(CCC, w ** 3)), "θw": Average(θ * w),
                                        "u²w": Average(at(CCC, u ** 2 * w)), "∂z_u": Average(at(CCC, partial_z(u)))})
                                                                # one fused bz_horizontal_moments call: every field is read once

    vθ = TangentialVelocity(model, center=(0, 0)).compute()     # (−y uᶜ + x vᶜ)/r at cell centres
    v̄θ = azimuthal_mean(vθ, radius=150e3, Nr=30)               # .data (Nr, Nz), .counts, .r, .z
    θ̄ = azimuthal_mean(LiquidIcePotentialTemperature(model), radius=150e3, Nr=30)      # same geometry: the ring plan is reused

Moisture fractions are picked from the model as grid_moisture_fractions does: no microphysics qᵛ = qᵗ and no liquid;
SaturationAdjustment the stored qᵛ, qˡ; Kessler qᵛ, qᶜˡ + qʳ; InstantaneousPrecipitation qᵛ = ρqᵛ / ρ and no liquid.  Anelastic models read the reference-state columns; a compressible model
hands its own p and ρ fields to the potential temperatures and its dynamics.reference_state (required) to the other kinds.
"""
import ctypes as C

import numpy as np

from . import _lib
from .grids import Center, Face
from .model import Field, fill_halo_regions_

_SPECIFIC_OR_DENSITY = ("specific", "density")


def _flavor(flavor, valid):
    flavor = str(flavor).lstrip(":")
    if flavor not in valid:      # the reference's ArgumentError
        raise ValueError(f"`flavor` must be one of {valid}, received {flavor!r}")
    return flavor


class _Arithmetic:
    """`a * b`, `a ** p` on fields, pointwise operations and expressions: each returns a small expression object for Average(...)."""

    def __mul__(self, other):
        return _Product(self, other)

    def __pow__(self, p):
        return _Power(self, p)

    def __add__(self, other):
        return _Sum(self, other)

    __sub__ = __radd__ = __rsub__ = __add__


class _Operation(_Arithmetic):
    """A KernelFunctionOperation at (Center, Center, Center) of one model."""
    loc = (Center, Center, Center)
    kind = None
    needs_saturation_pressure = False
    uses_model_pressure = False      # the potential temperatures: dynamics_pressure_for_potential_temperature

    def __init__(self, model):
        from ._context import refuse_mixed_phase
        # the diagnostic kernels form Rᵐ, cᵖᵐ and the latent term from qᵛ and qˡ and saturate over the liquid surface
        refuse_mixed_phase(getattr(model, "microphysics", None), type(self).__name__, "the diagnostic kernels know no qⁱ and no mixed-phase surface")
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
    elif model.microphysics is not None and not getattr(model, "_ip", False):      # (InstantaneousPrecipitation keeps no condensate: vapour only)
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


# ---- precipitation of InstantaneousPrecipitation (csrc/bz_instant_precip.hip: bz_column_integral) ----------------------------------------
def _require_instantaneous_precipitation(model, what):
    if not getattr(model, "_ip", False):
        raise NotImplementedError(f"{what}: implemented for microphysics = InstantaneousPrecipitation(...) "
                                  f"(the model carries {type(getattr(model, 'microphysics', None)).__name__})")


class ColumnIntegral:
    """Field(Integral(field, dims = 3)) of a centre Field of the model: `.compute()` returns the (Ny, Nx) interior view of a device array of
    (Ny + 2 Hy, Nx + 2 Hx) values, Σₖ f[k] Δzᶜ[k] summed upward from k = 0 (deterministic).  The array is kept and rewritten by the next
    `.compute()`."""

    def __init__(self, model, field):
        if not isinstance(field, Field) or field.zface or field.grid is not model.grid or field.dtype != model.temperature.dtype:
            raise ValueError("ColumnIntegral: a centre Field of the model's grid and float type")
        self.model, self.field, self.parent = model, field, None

    def compute(self):
        import torch
        m, g = self.model, self.model.grid
        if self.parent is None:
            self.parent = torch.zeros((g.Ny + 2 * g.Hy, g.Nx + 2 * g.Hx), dtype=self.field.parent.dtype, device=m.device)
        m._check(m._lib.bz_column_integral(m._ctx, C.c_void_p(self.field.ptr()), C.c_void_p(self.parent.data_ptr())), "bz_column_integral")
        return self.parent[g.Hy:g.Hy + g.Ny, g.Hx:g.Hx + g.Nx]


class _StoredField:
    """A field the model already holds, behind the `.compute()` of the other diagnostics."""

    def __init__(self, field):
        self.field = field

    def compute(self):
        return self.field


def precipitation_rate(model, phase="liquid"):
    """precipitation_rate(model, :liquid | :ice) (instantaneous_precipitation.jl:88-89): `.compute()` gives microphysical_fields.
    precipitation_rate (kg m⁻³ s⁻¹, the centre Field the once-per-step update writes) for :liquid; None is returned for :ice."""
    _require_instantaneous_precipitation(model, "precipitation_rate")
    phase = str(phase).lstrip(":")
    if phase not in ("liquid", "ice"):
        raise ValueError(f"`phase` must be :liquid or :ice, received {phase!r}")
    return _StoredField(model.microphysical_fields["precipitation_rate"]) if phase == "liquid" else None


def surface_precipitation_flux(model):
    """surface_precipitation_flux(model) (instantaneous_precipitation.jl:99-102): the condensate leaves at once, so the surface flux is the
    column integral of the precipitation rate, kg m⁻² s⁻¹: a ColumnIntegral, `.compute()` gives the (Ny, Nx) device array."""
    _require_instantaneous_precipitation(model, "surface_precipitation_flux")
    return ColumnIntegral(model, model.microphysical_fields["precipitation_rate"])


# ---- Average of products, powers and ∂z (csrc/bz_moments.hip: bz_horizontal_moments) ----------------------------------------------------
# Oceananigans' BinaryOperation, ^, ∂z and @at as the reference's examples use them in their profile lists
# (examples/neutral_atmospheric_boundary_layer.jl:203-221): trees of small objects that Average lowers onto one bz_moment descriptor
class _Expression(_Arithmetic):
    def shape(self):
        raise NotImplementedError

    def __repr__(self):
        return self.shape()


def _shape(x):
    if isinstance(x, _Expression):
        return x.shape()
    if isinstance(x, _Operation):
        return type(x).__name__
    if isinstance(x, Field):
        return "field"
    return type(x).__name__


class _Product(_Expression):
    def __init__(self, a, b):
        self.a, self.b = a, b

    def shape(self):
        right = _shape(self.b)
        return f"{_shape(self.a)} * " + (f"({right})" if isinstance(self.b, (_Product, _Sum)) else right)


class _Power(_Expression):
    def __init__(self, a, p):
        self.a, self.p = a, p

    def shape(self):
        base = _shape(self.a)
        return (f"({base})" if isinstance(self.a, _Expression) else base) + f" ** {self.p}"


class _Sum(_Expression):
    def __init__(self, a, b):
        self.a, self.b = a, b

    def shape(self):
        return f"{_shape(self.a)} + {_shape(self.b)}"


class _Dz(_Expression):
    def __init__(self, a):
        self.a = a

    def shape(self):
        return f"∂z({_shape(self.a)})"


class _At(_Expression):
    def __init__(self, loc, a):
        self.loc, self.a = tuple(loc), a

    def shape(self):
        return f"at(({', '.join(getattr(l, '__name__', repr(l)) for l in self.loc)}), {_shape(self.a)})"


def partial_z(f):
    """∂z(f) of one field or pointwise operation: (f[k] − f[k−1]) / Δzᵃᵃᶠ[k] at the z location opposite to f's."""
    return _Dz(f)


def at(loc, expr):
    """@at(loc, expr): the expression interpolated to `loc`; (Center, Center, Center) is implemented."""
    return _At(loc, expr)


def _is_leaf(x):
    return isinstance(x, (Field, _Operation))


class Moment:
    """One bz_moment before its fields are numbered: `factors` [(leaf, power), ...], `dz`, `at_center`."""

    def __init__(self, factors, dz=False, at_center=False):
        self.factors, self.dz, self.at_center = factors, bool(dz), bool(at_center)

    @property
    def leaves(self):
        return [f for f, _ in self.factors]

    def needs_halos(self):
        """True if any neighbour of a point is read: ∂z, @at of a face location, or factors at different locations."""
        first = self.factors[0][0].loc
        return self.dz or (self.at_center and any(l is Face for l in first)) or any(tuple(f.loc) != tuple(first) for f in self.leaves)

    def descriptor(self, index):
        """The bz_moment with fields numbered by `index` (id(leaf) -> position in fields[])."""
        M = _lib.bz_moment()
        M.n_factors = len(self.factors)
        for q, (f, p) in enumerate(self.factors):
            M.field[q], M.power[q] = index[id(f)], p
        M.dz, M.at_center = int(self.dz), int(self.at_center)
        return M

    def key(self):
        """(((face_x, face_y, face_z), power), ...), dz, at_center: what the descriptor says, without pointers"""
        return (tuple((tuple(int(l is Face) for l in f.loc), p) for f, p in self.factors), self.dz, self.at_center)


def lower(expr):
    """The Moment of an accepted expression: a left-associated product of up to three leaves, each optionally raised to a power 1..3, or a
    single ∂z(leaf), optionally under at((Center, Center, Center), ·).  Anything else raises NotImplementedError naming the shape."""
    def refuse(why):
        raise NotImplementedError(f"Average: {why}: {_shape(expr)} (implemented: leaf ** p * leaf ** p * leaf ** p multiplied left to right "
                                  f"with powers 1..3, or ∂z(leaf), optionally under at((Center, Center, Center), ...))")

    at_center = False
    body = expr
    if isinstance(body, _At):
        if body.loc != (Center, Center, Center):
            refuse("at(loc, ...) is implemented for (Center, Center, Center)")
        at_center, body = True, body.a

    def factor(x):
        if _is_leaf(x):
            return (x, 1)
        if isinstance(x, _Power) and _is_leaf(x.a):
            if not isinstance(x.p, (int, np.integer)) or isinstance(x.p, bool) or not 1 <= x.p <= 3:
                refuse("a power must be an integer 1..3")
            return (x.a, int(x.p))
        if isinstance(x, _Power):
            refuse("a power of an expression is not implemented")
        if isinstance(x, _Product):
            refuse("a product is multiplied left to right, (a * b) * c; a product as the right factor is not implemented")
        if isinstance(x, _Sum):
            refuse("sums are not implemented")
        if isinstance(x, _Dz):
            refuse("∂z inside a product is not implemented")
        if isinstance(x, _At):
            refuse("at(...) is implemented as the outermost operation")
        refuse(f"{type(x).__name__} is not a field or a diagnostic operation")

    if isinstance(body, _Dz):
        if not _is_leaf(body.a):
            refuse("∂z takes one field or diagnostic operation")
        return Moment([(body.a, 1)], dz=True, at_center=at_center)
    factors = []
    while isinstance(body, _Product):
        factors.insert(0, factor(body.b))
        body = body.a
    factors.insert(0, factor(body))
    if len(factors) > _lib.BZ_MAX_MOMENT_FACTORS:
        refuse(f"at most {_lib.BZ_MAX_MOMENT_FACTORS} factors")
    return Moment(factors, at_center=at_center)


def _dims(dims, model):
    """dims = (1, 2); dims = 1 on a Flat y, where it is the same average (the reference's x-z examples)"""
    d = (dims,) if isinstance(dims, (int, np.integer)) else tuple(dims)
    if d == (1, 2):
        return d
    topology = getattr(getattr(model, "grid", None), "topology", None)
    if d == (1,) and topology is not None and topology[1] == "Flat":
        return d
    raise NotImplementedError("Average: dims = (1, 2) is implemented, and dims = 1 on a Flat y")


def _refuse_slab(model, what):
    if _is_slab(model):
        raise NotImplementedError(f"{what}: not implemented on y-slab models (the average needs an all-reduce over the ranks)")


class Average:
    """Average(field_or_operation_or_expression, dims=(1, 2)): the horizontal mean per level.  `model` is needed if no leaf knows it."""

    def __init__(self, operand, dims=(1, 2), model=None):
        self.operand = operand
        self.moment = lower(operand) if isinstance(operand, _Expression) else None
        if model is None:
            for leaf in (self.moment.leaves if self.moment else [operand]):
                model = leaf.model if isinstance(leaf, _Operation) else None
                if model is None:
                    owner = getattr(leaf, "_owner", None)
                    model = owner() if owner is not None else None
                if model is not None:
                    break
        if model is None:
            raise ValueError("Average(field): pass model=... for a field that does not know its model")
        self.model = model
        self.dims = _dims(dims, model)

    def compute(self):
        if self.moment is not None:
            return compute_averages(self.model, {"": self})[""]
        field = self.operand.compute() if isinstance(self.operand, _Operation) else self.operand
        return horizontal_average(self.model, field)


def _maintained_fields(model):
    """ids of the Fields the model itself holds (state, diagnostics, dynamics, microphysics, tracers): update_state! keeps their halos"""
    found = set()
    for holder in (model, getattr(model, "dynamics", None)):
        for value in vars(holder).values() if holder is not None else ():
            for f in (value.values() if isinstance(value, dict) else (value,)):
                if isinstance(f, Field):
                    found.add(id(f))
    return found


def _plan_calls(moments, max_fields=None, max_moments=None):
    """Greedy packing of moments (in order) into calls of at most max_moments moments over at most max_fields distinct leaves: a list of
    (leaves, [positions])."""
    max_fields = _lib.BZ_MAX_MOMENT_FIELDS if max_fields is None else max_fields
    max_moments = _lib.BZ_MAX_MOMENTS if max_moments is None else max_moments
    calls = []
    for pos, M in enumerate(moments):
        ids = {id(f): f for f in M.leaves}
        for leaves, members in calls:
            new = [f for i, f in ids.items() if i not in {id(x) for x in leaves}]
            if len(members) < max_moments and len(leaves) + len(new) <= max_fields:
                leaves.extend(new)
                members.append(pos)
                break
        else:
            calls.append((list(ids.values()), [pos]))
    return calls


def compute_averages(model, averages):
    """Evaluate {name: Average(...)} of one model in as few fused bz_horizontal_moments calls as its limits allow (every distinct field of
    a call is read once); returns {name: numpy profile}.  Pointwise operations among the leaves are computed first, in one
    compute_diagnostics launch; halos of leaves the model does not maintain are filled where a moment reads neighbours."""
    _refuse_slab(model, "compute_averages")
    names = list(averages)
    moments = []
    for name in names:
        A = averages[name]
        if not isinstance(A, Average):
            raise TypeError(f"{name!r}: {A!r} is not an Average")
        if A.model is not model:
            raise ValueError("every Average must belong to `model`")
        M = A.moment
        moments.append(Moment(list(M.factors), M.dz, M.at_center) if M is not None else Moment([(A.operand, 1)]))
    if not moments:
        return {}
    # pointwise operations -> centre fields, one launch for all of them
    ops = {}
    for M in moments:
        for f in M.leaves:
            if isinstance(f, _Operation):
                ops.setdefault(id(f), f)
    done = dict(zip(ops, compute_diagnostics(model, list(ops.values())))) if ops else {}
    for M in moments:
        M.factors = [(done.get(id(f), f), p) for f, p in M.factors]
    filled = {id(f) for f in done.values()} | _maintained_fields(model)
    real = model.temperature.dtype
    for M in moments:
        for f in M.leaves:
            if not isinstance(f, Field) or f.grid is not model.grid or f.dtype != real:
                raise ValueError("Average: every leaf must be a Field of the model's grid and float type")
            if hasattr(f, "_fresh"):
                f._fresh()      # a stale diagnostic field of the model is rebuilt first
            if M.needs_halos() and id(f) not in filled:
                fill_halo_regions_(model, f)      # not one of the fields the model maintains: its halos may be anything
                filled.add(id(f))
    T, Nz = model._T, model.grid.Nz
    out = {}
    for leaves, members in _plan_calls(moments):
        index = {id(f): n for n, f in enumerate(leaves)}
        fields = (_lib.bz_moment_field * len(leaves))()
        for n, f in enumerate(leaves):
            fields[n].data = f.ptr()
            fields[n].face_x, fields[n].face_y, fields[n].face_z = (int(l is Face) for l in f.loc)
        descs = (_lib.bz_moment * len(members))(*[moments[pos].descriptor(index) for pos in members])
        prof = np.zeros((len(members), Nz + 1), dtype=T.np_real)
        nlev = (C.c_int32 * len(members))()
        model._check(model._lib.bz_horizontal_moments(model._ctx, len(leaves), fields, len(members), descs,
                                                      prof.ctypes.data_as(C.POINTER(T.real)), nlev), "bz_horizontal_moments")
        for row, pos in enumerate(members):
            out[names[pos]] = prof[row, :nlev[row]].copy()
    return {name: out[name] for name in names}


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
