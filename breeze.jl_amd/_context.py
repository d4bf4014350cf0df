"""What the host constructors of the anelastic, compressible and slab models share (model.py, compressible.py, distributed.py): the
struct builders of the context, the base class of an object that owns a `bz_ctx`, the common field set, the rank-local slab grid, and
one function per attachment (`bz_set_*`) with the validation that goes with it.

The rule: a new attachment is ONE function here, called from each constructor that supports it.  Where two models legitimately differ
(a refusal, the wording of a message), the difference is an argument.  Each constructor keeps its own order of checks and of `bz_set_*`
calls; nothing here decides an order.  Nothing a time step executes lives here."""
import ctypes as C

import numpy as np

from . import _lib
from .grids import Bounded, Periodic, RectilinearGrid
from .thermodynamics import dry_air_gas_constant, vapor_gas_constant


# ---- struct builders -----------------------------------------------------------------------------------------------------------------
def grid_struct(T, grid):
    """-> (bz_grid of the precision T = _lib.types(grid.ftype), the z-face array it points to: keep it alive as long as the struct)."""
    zf = np.ascontiguousarray(grid.zᶠ, dtype=T.np_real)
    bg = T.bz_grid()
    bg.Nx, bg.Ny, bg.Nz = grid.Nx, grid.Ny, grid.Nz
    bg.Hx, bg.Hy, bg.Hz = grid.Hx, grid.Hy, grid.Hz
    for d, t in enumerate(grid.topology_codes()):
        bg.topo[d] = t
    bg.ftype = grid.ftype
    bg.dx, bg.dy = grid.Δx, grid.Δy
    bg.zf = zf.ctypes.data_as(C.POINTER(T.real))
    bg.regular_z = 1 if grid.regular_z else 0
    return bg, zf


def constants_struct(T, c):
    return T.bz_constants(c.gravitational_acceleration, dry_air_gas_constant(c), vapor_gas_constant(c),
                          c.dry_air_heat_capacity, c.vapor_heat_capacity)


def reference_struct(T, ref):
    """-> (bz_reference_state of an anelastic ReferenceState, the column arrays it points to)."""
    arrays = [np.ascontiguousarray(a, dtype=T.np_real) for a in (ref.density, ref.pressure, ref.temperature)]
    return T.bz_reference_state(ref.surface_pressure, ref.potential_temperature, ref.standard_pressure,
                                *[a.ctypes.data_as(C.POINTER(T.real)) for a in arrays]), arrays


def load_library(grid, advection, float32_message):
    """The build of the library a model runs: the Float32 twin for eltype(grid) = Float32 (WENO only), else the Centered(order = 2) build,
    the WENO build or one of its FT2 variants (WENO(ft2_hypothesis = 1 | 2))."""
    from .model import WENO
    if grid.ftype == 4:
        if not isinstance(advection, WENO):
            raise NotImplementedError(float32_message)
        return _lib.load_f32()
    return _lib.load(advection.order, getattr(advection, "ft2_hypothesis", 0))


# ---- the owner of a context ----------------------------------------------------------------------------------------------------------
class ContextOwner:
    """An object that owns a `bz_ctx`: `_lib` (the loaded library), `_T` (= _lib.types(ftype)), `device` and `_ctx`."""

    _ctx = None

    def _open_context(self, what, *structs):
        """`_create_context(lib, *structs)` of the class, then the context takes torch's current stream of the device."""
        import torch
        self._ctx = C.c_void_p()
        rc = self._create_context(self._lib, *structs)
        if rc != 0:
            raise _lib.BreezeHIPError(f"{what} failed with code {rc}")
        self._check(self._lib.bz_set_stream(self._ctx, C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)), "bz_set_stream")

    def _check(self, rc, what):
        _lib.check(self._lib, self._ctx, rc, what)

    def __del__(self):
        try:
            if getattr(self, "_ctx", None):
                self._lib.bz_destroy(self._ctx)
                self._ctx = None
        except Exception:
            pass

    def synchronize(self):
        self._check(self._lib.bz_sync(self._ctx), "bz_sync")

    def graph_enable(self, on=True):
        """hipGraph replay of whole steps (csrc/bz_graph.hip); opt-in, bit-identical to launched steps."""
        self._check(self._lib.bz_graph_enable(self._ctx, 1 if on else 0), "bz_graph_enable")

    def graph_info(self):
        """(enabled, steps recorded, steps replayed)"""
        en, cap, rep = C.c_int32(), C.c_int64(), C.c_int64()
        self._check(self._lib.bz_graph_info(self._ctx, C.byref(en), C.byref(cap), C.byref(rep)), "bz_graph_info")
        return bool(en.value), cap.value, rep.value

    def closure_marches(self):
        """Whether the SmagorinskyLilly kernels of this context run as the z-marching LDS-tiled kernels (whole 64 x 8 tiles) rather than
        cell per thread: the verdict of the library's one dispatch predicate (bz_closure_march_info).  Same bits either way."""
        m = C.c_int32()
        self._check(self._lib.bz_closure_march_info(self._ctx, C.byref(m)), "bz_closure_march_info")
        return bool(m.value)

    def profile_enable(self, on=True):
        self._check(self._lib.bz_profile_enable(self._ctx, 1 if on else 0), "bz_profile_enable")

    def profile_reset(self):
        self._check(self._lib.bz_profile_reset(self._ctx), "bz_profile_reset")

    def profile(self):
        """{kernel group: (total_ms, launches)} accumulated since the last reset."""
        out = {}
        for i in range(self._lib.bz_profile_count(self._ctx)):
            name, ms, n = C.c_char_p(), self._T.real(), C.c_int64()
            self._check(self._lib.bz_profile_get(self._ctx, i, C.byref(name), C.byref(ms), C.byref(n)), "bz_profile_get")
            out[name.value.decode()] = (ms.value, n.value)
        return out

    def comm_info(self):
        """(transport name, bytes this rank has sent, number of exchanges) of the library-owned communicator of a slab context; an error
        of the library on a context without one."""
        name, nbytes, nex = C.c_char_p(), C.c_int64(), C.c_int32()
        self._check(self._lib.bz_comm_info(self._ctx, C.byref(name), C.byref(nbytes), C.byref(nex)), "bz_comm_info")
        return name.value.decode(), nbytes.value, nex.value


# ---- fields and grids ----------------------------------------------------------------------------------------------------------------
def allocate_common_fields(model, grid, momentum=True):
    """materialize_momentum_and_velocities, formulation, moisture, temperature: the fields every model has, on `model.device`."""
    from .model import _LOC, Field

    def fld(loc):
        return Field(grid, _LOC[loc], model.device)

    model.momentum = {"ρu": fld("fcc"), "ρv": fld("cfc"), "ρw": fld("ccf")} if momentum else {}
    model.velocities = {"u": fld("fcc"), "v": fld("cfc"), "w": fld("ccf")}
    model.potential_temperature_density, model.potential_temperature = fld("ccc"), fld("ccc")
    model.moisture_density, model.specific_moisture = fld("ccc"), fld("ccc")
    model.temperature = fld("ccc")
    return fld


def check_slab_topology(global_grid):
    if global_grid.topology != (Periodic, Periodic, Bounded):
        raise NotImplementedError("slab decomposition implements topology (Periodic, Periodic, Bounded)")


def slab_grid(global_grid, rank, world):
    """The grid of rank `rank` of `world` y-slabs of a (Periodic, Periodic, Bounded) grid: rows [rank Ny / world, (rank + 1) Ny / world)."""
    G = global_grid
    check_slab_topology(G)
    if G.Ny % world:
        raise ValueError(f"Ny={G.Ny} is not divisible by {world} ranks")
    Ny = G.Ny // world
    y0 = G.yᶠ[0] + rank * Ny * G.Δy
    z = (G.zᶠ[0], G.zᶠ[-1]) if G.regular_z else G.zᶠ
    grid = RectilinearGrid((G.Nx, Ny, G.Nz), x=(G.xᶠ[0], G.xᶠ[0] + G.Nx * G.Δx), y=(y0, y0 + Ny * G.Δy), z=z,
                           halo=(G.Hx, G.Hy, G.Hz), float_type=G.float_type)      # eltype(grid) travels with the slab
    grid.Δx, grid.Δy = G.Δx, G.Δy          # bit-identical spacings on every rank
    return grid


# ---- validation shared by the constructors ---------------------------------------------------------------------------------------------
def check_closure(closure, what="closure"):
    """One closure, no tuples; SmagorinskyLilly or a ScalarDiffusivity.  -> whether it is a ScalarDiffusivity."""
    from .closures import ScalarDiffusivity
    from .forcings import SmagorinskyLilly
    if isinstance(closure, (tuple, list)):
        raise NotImplementedError("closure: one closure is implemented (no closure tuples)")
    if closure is not None and not isinstance(closure, (SmagorinskyLilly, ScalarDiffusivity)):
        raise NotImplementedError(f"{what}: SmagorinskyLilly(), ScalarDiffusivity(...) and VerticalScalarDiffusivity(...) are implemented")
    return isinstance(closure, ScalarDiffusivity)


def check_microphysics(microphysics, message, instantaneous_precipitation_refused="InstantaneousPrecipitation: not implemented on this model"):
    """Nothing, warm-phase saturation adjustment or Kessler; InstantaneousPrecipitation where the caller passes
    instantaneous_precipitation_refused = None (else that message is raised, at the place of this check).  -> whether it is Kessler."""
    from .microphysics import DCMIP2016KesslerMicrophysics, InstantaneousPrecipitation, SaturationAdjustment
    if isinstance(microphysics, InstantaneousPrecipitation):
        if instantaneous_precipitation_refused is not None:
            raise NotImplementedError(instantaneous_precipitation_refused)
        return False
    if microphysics is not None and not isinstance(microphysics, (SaturationAdjustment, DCMIP2016KesslerMicrophysics)):
        raise NotImplementedError(message)
    return isinstance(microphysics, DCMIP2016KesslerMicrophysics)


def is_mixed_phase(microphysics):
    from .microphysics import MixedPhaseEquilibrium, cloud_formation
    return isinstance(getattr(cloud_formation(microphysics), "equilibrium", None), MixedPhaseEquilibrium)      # (through a BulkMicrophysics)


def refuse_bulk_microphysics(microphysics, where, why):
    """BulkMicrophysics(...) runs on the single-device anelastic AtmosphereModel; every other model says so here, by name, before its
    generic microphysics type check."""
    from .microphysics import BulkMicrophysics
    if isinstance(microphysics, BulkMicrophysics):
        raise NotImplementedError(f"{where}: BulkMicrophysics is not implemented ({why}); it runs on the single-device anelastic AtmosphereModel")


def refuse_mixed_phase(microphysics, where, why):
    """SaturationAdjustment(equilibrium = MixedPhaseEquilibrium()) runs on the single-device anelastic AtmosphereModel (potential-temperature
    formulation) and, attached by compressible.set_mixed_phase_equilibrium_, on the single-device CompressibleAtmosphereModel that is
    periodic in x and y or Flat in y; every other place says so here, where the microphysics type is checked."""
    if is_mixed_phase(microphysics):
        raise NotImplementedError(f"{where}: SaturationAdjustment(equilibrium = MixedPhaseEquilibrium()) is not implemented ({why}); "
                                  "pass equilibrium = WarmPhaseEquilibrium()")


def check_mixed_phase_model(microphysics, thermodynamic_constants, forcing, boundary_conditions):
    """What a mixed-phase anelastic model does not attach: Tetens constants (its ice coefficients are not mirrored) and the attachments whose
    kernels form cᵖᵐ from qᵛ and qˡ alone: energy-keyed column forcings, a bottom energy flux, bulk surface fluxes and the surface layer."""
    if not is_mixed_phase(microphysics):
        return
    from .forcings import _bulk_conditions, _key
    from .microphysics import TetensFormula
    where = "AtmosphereModel"
    if isinstance(getattr(thermodynamic_constants, "saturation_vapor_pressure", None), TetensFormula):
        refuse_mixed_phase(microphysics, where, "TetensFormula constants: the ice coefficients of the Tetens formula are not mirrored")
    if any(_key(name) == "e" for name in (forcing or {})):
        refuse_mixed_phase(microphysics, where, "a forcing keyed `e`: the energy-to-θ conversion forms cᵖᵐ without qⁱ")
    if any(True for _ in _bulk_conditions(boundary_conditions)):
        refuse_mixed_phase(microphysics, where, "bulk surface fluxes and the surface layer form cᵖᵐ without qⁱ")
    if any(_key(name) == "ρe" for name in (boundary_conditions or {})):
        refuse_mixed_phase(microphysics, where, "a bottom flux keyed ρe: the energy-to-θ conversion forms cᵖᵐ without qⁱ")


def check_mixed_phase_compressible(microphysics, where, thermodynamic_constants, surface_fluxes, slab, walls):
    """What compressible.set_mixed_phase_equilibrium_ does not attach the mixed-phase form to: y-slabs (their halo exchanges carry qᵛ and qˡ),
    lateral walls, Tetens constants and the bulk surface fluxes, whose kernel forms cᵖᵐ from qᵛ and qˡ alone.  (The constructors refuse
    BulkMicrophysics, and InstantaneousPrecipitation(equilibrium = MixedPhaseEquilibrium()) refuses itself.)"""
    if not is_mixed_phase(microphysics):
        return
    from .microphysics import TetensFormula
    if slab:
        refuse_mixed_phase(microphysics, where, "the halo exchanges of y-slab models carry qᵛ and qˡ only")
    if walls:
        refuse_mixed_phase(microphysics, where, "SaturationAdjustment is not built on a compressible model between walls (Bounded x / Bounded y)")
    if isinstance(getattr(thermodynamic_constants, "saturation_vapor_pressure", None), TetensFormula):
        refuse_mixed_phase(microphysics, where, "TetensFormula constants: the ice coefficients of the Tetens formula are not mirrored")
    if surface_fluxes:
        refuse_mixed_phase(microphysics, where, "bulk surface fluxes form cᵖᵐ without qⁱ")


def flatau_polynomial(thermodynamic_constants):
    """The FlatauPolynomial of the constants, or None (Clausius-Clapeyron, Tetens)."""
    from .thermodynamics import FlatauPolynomial
    formula = getattr(thermodynamic_constants, "saturation_vapor_pressure", None)
    return formula if isinstance(formula, FlatauPolynomial) else None


def refuse_flatau_polynomial(thermodynamic_constants, where, why):
    """ThermodynamicConstants(saturation_vapor_pressure = FlatauPolynomial()) runs inside the saturation adjustments of the single-device
    AtmosphereModel (AnelasticDynamics) and CompressibleAtmosphereModel; every place whose kernels hard-wire the Clausius-Clapeyron expression
    says so here, where the constants are checked and before a GPU is asked for."""
    if flatau_polynomial(thermodynamic_constants) is not None:
        raise NotImplementedError(f"{where}: ThermodynamicConstants(saturation_vapor_pressure = FlatauPolynomial()) is not implemented ({why}); "
                                  "the default (Clausius-Clapeyron) constants run here")


def check_flatau_anelastic(thermodynamic_constants, boundary_conditions):
    """The bottom conditions of an anelastic model whose surface qᵛ⁺ is the Clausius-Clapeyron expression: BulkVaporFlux, and the surface layer
    (PolynomialCoefficient, FilteredSurfaceVelocities, T₀(x, y)), whose stability correction forms θᵥ₀ from qᵛ⁺(T₀) for every condition.  Forcings
    and bottom fluxes keyed e / ρe convert energy to θ with cᵖᵐ of the stored qᵛ, qˡ: they read no pᵛ⁺ and stay."""
    if flatau_polynomial(thermodynamic_constants) is None:
        return
    from .forcings import BulkVaporFlux, _bulk_conditions, needs_surface_layer
    if needs_surface_layer(boundary_conditions):
        refuse_flatau_polynomial(thermodynamic_constants, "AtmosphereModel", "the surface layer (PolynomialCoefficient, FilteredSurfaceVelocities, "
                                 "T₀(x, y)) evaluates the Clausius-Clapeyron qᵛ⁺ of the surface")
    if any(isinstance(cond, BulkVaporFlux) for _, cond in _bulk_conditions(boundary_conditions)):
        refuse_flatau_polynomial(thermodynamic_constants, "AtmosphereModel", "BulkVaporFlux evaluates the Clausius-Clapeyron qᵛ⁺ of the surface")


def attach_flatau_polynomial(model):
    """bz_set_saturation_vapor_pressure_polynomial from the constants of the model; nothing on Clausius-Clapeyron (and Tetens) constants."""
    fp = flatau_polynomial(model.thermodynamic_constants)
    if fp is None:
        return
    P = model._T.bz_flatau_polynomial()
    for n in range(9):
        P.liquid_coefficients[n], P.ice_coefficients[n] = fp.liquid_coefficients[n], fp.ice_coefficients[n]
    P.reference_temperature, P.minimum_temperature_offset = fp.reference_temperature, fp.minimum_temperature_offset
    model._check(model._lib.bz_set_saturation_vapor_pressure_polynomial(model._ctx, C.byref(P)), "bz_set_saturation_vapor_pressure_polynomial")


def check_kessler_constants(thermodynamic_constants):
    """validate_microphysics (dcmip2016_kessler.jl:196-207)"""
    from .microphysics import TetensFormula
    tcs = thermodynamic_constants
    if tcs is None or not isinstance(getattr(tcs, "saturation_vapor_pressure", None), TetensFormula):
        raise ValueError("DCMIP2016KesslerMicrophysics requires `thermodynamic_constants` with a `TetensFormula` "
                         "saturation vapor pressure formulation. Construct the model with, e.g., "
                         "`thermodynamic_constants = ThermodynamicConstants(saturation_vapor_pressure = TetensFormula())`.")


# ---- attachments: one function each, called by every constructor that supports it ----------------------------------------------------------
def materialize_kessler_fields(model, fld):
    """materialize_microphysical_fields(::DCMIP2016KM) (dcmip2016_kessler.jl:255-290); before the time stepper's U⁰ and Gⁿ are made."""
    import torch
    g = model.grid
    model.microphysical_fields = {k: fld("ccc") for k in ("ρqᶜˡ", "ρqʳ", "qᵛ", "qᶜˡ", "qʳ", "𝕎ʳ")}
    model.microphysical_fields["precipitation_rate"] = torch.zeros((g.Ny + 2 * g.Hy, g.Nx + 2 * g.Hx),
                                                                   dtype=model.potential_temperature.dtype, device=model.device)


def attach_kessler(model, standard_pressure):
    from .microphysics import kessler_parameter_struct
    μ = model.microphysical_fields
    P = kessler_parameter_struct(model.microphysics, model.thermodynamic_constants, ftype=model.grid.ftype)
    K = model._T.bz_kessler_model_fields()
    K.cloud_liquid_density, K.rain_density = μ["ρqᶜˡ"].ptr(), μ["ρqʳ"].ptr()
    K.U0_cloud_liquid_density, K.U0_rain_density = model.U0["ρqᶜˡ"].ptr(), model.U0["ρqʳ"].ptr()
    K.G_cloud_liquid_density, K.G_rain_density = model.G["ρqᶜˡ"].ptr(), model.G["ρqʳ"].ptr()
    K.vapor_mass_fraction, K.cloud_liquid_mass_fraction, K.rain_mass_fraction = μ["qᵛ"].ptr(), μ["qᶜˡ"].ptr(), μ["qʳ"].ptr()
    K.rain_terminal_velocity, K.precipitation_rate = μ["𝕎ʳ"].ptr(), μ["precipitation_rate"].data_ptr()
    model._check(model._lib.bz_set_kessler_microphysics(model._ctx, C.byref(P), C.byref(K), standard_pressure),
                 "bz_set_kessler_microphysics")


def attach_saturation_adjustment(model, fld):
    """materialize_microphysical_fields(::WarmPhaseSaturationAdjustment): (qᵛ, qˡ, qᵉ); (::MixedPhaseSaturationAdjustment): (qᵛ, qˡ, qⁱ, qᵉ)
    (saturation_adjustment.jl:118-119); qᵉ is the specific moisture slot."""
    from .microphysics import cloud_formation
    adjustment = cloud_formation(model.microphysics)
    c, solver = model.thermodynamic_constants, adjustment.solver
    mixed = is_mixed_phase(adjustment)
    μ = model.microphysical_fields = {"qᵛ": fld("ccc"), "qˡ": fld("ccc"), **({"qⁱ": fld("ccc")} if mixed else {}), "qᵉ": model.specific_moisture}
    sa = model._T.bz_saturation_adjustment(c.liquid_reference_latent_heat, c.liquid_heat_capacity, c.energy_reference_temperature,
                                           c.triple_point_temperature, c.triple_point_pressure, solver.abstol, solver.maxiter, 0)
    model._check(model._lib.bz_set_saturation_adjustment(model._ctx, C.byref(sa), C.c_void_p(μ["qᵛ"].ptr()), C.c_void_p(μ["qˡ"].ptr())),
                 "bz_set_saturation_adjustment")
    if mixed:
        eq = adjustment.equilibrium
        mp = model._T.bz_mixed_phase_equilibrium(eq.freezing_temperature, eq.homogeneous_ice_nucleation_temperature,
                                                 c.ice_reference_latent_heat, c.ice_heat_capacity)
        model._check(model._lib.bz_set_mixed_phase_equilibrium(model._ctx, C.byref(mp), C.c_void_p(μ["qⁱ"].ptr())),
                     "bz_set_mixed_phase_equilibrium")


def attach_negative_moisture_correction(model):
    """negative_moisture_correction(microphysics) of a BulkMicrophysics -> bz_set_negative_moisture_correction.  The non-precipitating scheme
    has no species (correction_moisture_fields, correction_number_mass_pairs and correction_number_fields are empty tuples): the lists of
    the descriptor stay empty, and SpeciesBorrowing() without vertical borrowing launches nothing."""
    from .microphysics import SpeciesBorrowing, vertical_borrowing
    correction = getattr(model.microphysics, "negative_moisture_correction", None)
    if correction is None:
        return
    d = _lib.bz_negative_moisture_correction()
    d.species_borrowing = 1 if isinstance(correction, SpeciesBorrowing) else 0
    d.vertical_borrowing = 1 if vertical_borrowing(correction) else 0
    model._check(model._lib.bz_set_negative_moisture_correction(model._ctx, C.byref(d)), "bz_set_negative_moisture_correction")


def attach_instantaneous_precipitation(model, fld):
    """materialize_microphysical_fields(::InstantaneousPrecipitation) (instantaneous_precipitation.jl:69-70): (qᵛ, precipitation_rate); qᵛ is
    the specific-moisture slot (update_microphysical_fields! stores the vapour fraction the state carries, which is ρqᵛ / ρ)."""
    c, solver = model.thermodynamic_constants, model.microphysics.saturation_adjustment.solver
    μ = model.microphysical_fields = {"qᵛ": model.specific_moisture, "precipitation_rate": fld("ccc")}
    sa = model._T.bz_saturation_adjustment(c.liquid_reference_latent_heat, c.liquid_heat_capacity, c.energy_reference_temperature,
                                           c.triple_point_temperature, c.triple_point_pressure, solver.abstol, solver.maxiter, 0)
    model._check(model._lib.bz_set_instantaneous_precipitation(model._ctx, C.byref(sa), C.c_void_p(μ["precipitation_rate"].ptr())),
                 "bz_set_instantaneous_precipitation")


def attach_closure(model, fld, smagorinsky_refused=None):
    """ScalarDiffusivity: no closure fields — ν and κ are numbers or the user's own centre fields (dcmip2016_tc.jl:277-292), checked here;
    SmagorinskyLilly: build_closure_fields, νₑ (atmosphere_model.jl:276).  smagorinsky_refused: the message of a model that is configured
    in a way SmagorinskyLilly does not run with (a model that refuses the vertically implicit discretisation has done so already)."""
    from .closures import ScalarDiffusivity
    from .model import Field
    closure, T = model.closure, model._T
    model.closure_fields = {}
    if isinstance(closure, ScalarDiffusivity):
        Kf = {}
        for name, value in (("ν", closure.ν), ("κ", closure.κ)):
            if isinstance(value, Field):
                if value.grid is not model.grid or value.parent.device != model.device or value.parent.dtype != model.potential_temperature.parent.dtype:
                    raise ValueError(f"closure {name}: the field must live on the model's grid, device and float type")
                Kf[name] = value
        sd = T.bz_scalar_diffusivity(closure.formulation, 1 if closure.vertically_implicit else 0,
                                     0.0 if "ν" in Kf else closure.ν, 0.0 if "κ" in Kf else closure.κ)
        model._diffusivity_fields = Kf      # keeps the arrays the context reads alive
        model._check(model._lib.bz_set_scalar_diffusivity(model._ctx, C.byref(sd), C.c_void_p(Kf["ν"].ptr() if "ν" in Kf else None),
                                                          C.c_void_p(Kf["κ"].ptr() if "κ" in Kf else None)), "bz_set_scalar_diffusivity")
    elif closure is not None:
        if smagorinsky_refused:
            raise NotImplementedError(smagorinsky_refused)
        model.closure_fields = {"νₑ": fld("ccc")}
        cl = T.bz_smagorinsky_lilly(closure.C, closure.Cb, closure.Pr)
        model._check(model._lib.bz_set_closure(model._ctx, C.byref(cl), C.c_void_p(model.closure_fields["νₑ"].ptr())), "bz_set_closure")


def attach_relaxation(model, relaxation, formulation):
    """{key: Relaxation} (forcings.split_relaxation) -> the sponge columns of the context."""
    from .forcings import materialize_relaxation
    Rx, model._relaxation_keepalive = materialize_relaxation(model.grid, relaxation, formulation, model._T)
    if Rx is not None:
        model._check(model._lib.bz_set_relaxation(model._ctx, C.byref(Rx)), "bz_set_relaxation")


def attach_field_forcing(model, field_forcing, formulation):
    """Forcing(f(x, y, z)) on θ / e (or ρθ / ρe): a centre field the library reads at every tendency evaluation; refresh it with
    model.thermodynamic_forcing_field.set_interior(...) when the forcing depends on time."""
    from .forcings import materialize_field_forcing
    model.thermodynamic_forcing_field, specific = materialize_field_forcing(model.grid, field_forcing, formulation, model.device)
    if model.thermodynamic_forcing_field is not None:
        model._check(model._lib.bz_set_field_forcing(model._ctx, C.c_void_p(model.thermodynamic_forcing_field.ptr()), specific),
                     "bz_set_field_forcing")
