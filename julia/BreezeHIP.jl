# BreezeHIP.jl — Julia-side glue for libbreeze_hip.so (UNTESTED: Julia is not available in the build image).
#
# A package extension in the style of ext/BreezeReactantExt/Timesteppers.jl:6-19: the hot-path generic functions are
# specialised on a marker architecture and forwarded to the C ABI of include/breeze_hip.h.  Fields stay ordinary
# Oceananigans fields whose storage lives on the GPU (e.g. ROCArray parents); only raw device pointers cross the boundary.
module BreezeHIP

using Breeze
using Breeze.AtmosphereModels: AtmosphereModel, AtmosphereModels
using Breeze.TimeSteppers: SSPRungeKutta3
using Oceananigans
using Oceananigans.TimeSteppers: TimeSteppers as OceananigansTimeSteppers, update_state!, tick!
using Oceananigans.Grids: topology, Periodic, Bounded, Flat, znodes, Face
using Oceananigans.Architectures: AbstractArchitecture

const libbreeze_hip = get(ENV, "BREEZE_HIP_LIB", "libbreeze_hip.so")

"Marker architecture: fields are allocated by `child` (a GPU architecture), the hot path runs in libbreeze_hip."
struct HIPNative{A} <: AbstractArchitecture
    child :: A
end

struct BzGrid
    Nx::Int32; Ny::Int32; Nz::Int32
    Hx::Int32; Hy::Int32; Hz::Int32
    topo::NTuple{3, Int32}
    ftype::Int32
    dx::Float64; dy::Float64
    zf::Ptr{Float64}
    regular_z::Int32; reserved::Int32
end
struct BzConstants
    g::Float64; Rd::Float64; Rv::Float64; cpd::Float64; cpv::Float64
end
struct BzReferenceState
    p0::Float64; θ0::Float64; pst::Float64
    density::Ptr{Float64}; pressure::Ptr{Float64}; temperature::Ptr{Float64}
end
struct BzState
    ρu::Ptr{Float64}; ρv::Ptr{Float64}; ρw::Ptr{Float64}; ρθ::Ptr{Float64}; ρq::Ptr{Float64}
    u::Ptr{Float64}; v::Ptr{Float64}; w::Ptr{Float64}; θ::Ptr{Float64}; q::Ptr{Float64}; T::Ptr{Float64}
    ϕ::Ptr{Float64}
end
struct BzPrognostic
    ρu::Ptr{Float64}; ρv::Ptr{Float64}; ρw::Ptr{Float64}; ρθ::Ptr{Float64}; ρq::Ptr{Float64}
end

devptr(f) = Ptr{Float64}(UInt(pointer(parent(f))))     # device pointer of the halo-inclusive parent array
topocode(::Type{Periodic}) = Int32(0); topocode(::Type{Bounded}) = Int32(1); topocode(::Type{Flat}) = Int32(2)

check(rc, what, ctx) = rc == 0 || error("$what failed with code $rc: ",
                                        unsafe_string(ccall((:bz_last_error, libbreeze_hip), Cstring, (Ptr{Cvoid},), ctx)))

"Build the context once per model (dynamics_pressure_solver + materialize_advection time)."
function create_context(model::AtmosphereModel)
    grid = model.grid
    Nx, Ny, Nz = size(grid); Hx, Hy, Hz = Oceananigans.Grids.halo_size(grid)
    zf = collect(Float64, znodes(grid, Face()))
    ref = model.dynamics.reference_state
    c = model.thermodynamic_constants
    hostcol(f) = collect(Float64, vec(Array(parent(f))))          # Nz + 2Hz values, halos filled
    ρ, p, T = hostcol(ref.density), hostcol(ref.pressure), hostcol(ref.temperature)
    ctx = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve zf ρ p T begin
        g = BzGrid(Nx, Ny, Nz, Hx, Hy, Hz, map(topocode, topology(grid)), 8, grid.Δxᶜᵃᵃ, grid.Δyᵃᶜᵃ, pointer(zf),
                   grid.z.Δᵃᵃᶜ isa Number ? 1 : 0, 0)
        k = BzConstants(c.gravitational_acceleration, c.molar_gas_constant / c.dry_air.molar_mass,
                        c.molar_gas_constant / c.vapor.molar_mass, c.dry_air.heat_capacity, c.vapor.heat_capacity)
        r = BzReferenceState(ref.surface_pressure, ref.potential_temperature, ref.standard_pressure,
                             pointer(ρ), pointer(p), pointer(T))
        rc = ccall((:bz_create, libbreeze_hip), Cint,
                   (Ref{Ptr{Cvoid}}, Ref{BzGrid}, Ref{BzConstants}, Ref{BzReferenceState}, Cint), ctx, g, k, r, weno_order(model.advection))
        rc == 0 || error("bz_create failed with code $rc (WENO orders 5, 7, 9 with halos >= (order + 1) / 2)")
    end
    so = scalar_weno_order(model.advection)      # model.advection = (; momentum, ρθ, ρqᵉ, ...) after the constructor merged the schemes
    so == weno_order(model.advection) || set_scalar_advection_order!(ctx[], so)
    return ctx[]
end

state(model) = BzState(devptr(model.momentum.ρu), devptr(model.momentum.ρv), devptr(model.momentum.ρw),
                       devptr(model.formulation.potential_temperature_density), devptr(model.moisture_density),
                       devptr(model.velocities.u), devptr(model.velocities.v), devptr(model.velocities.w),
                       devptr(model.formulation.potential_temperature), devptr(model.microphysical_fields.qᵛ),
                       devptr(model.temperature), devptr(model.dynamics.pressure_anomaly))
prognostic(nt) = BzPrognostic(devptr(nt.ρu), devptr(nt.ρv), devptr(nt.ρw), devptr(nt.ρθ), devptr(nt.ρqᵛ))

const CONTEXTS = IdDict{Any, Ptr{Cvoid}}()
context(model) = get!(() -> create_context(model), CONTEXTS, model)

const HIPModel = AtmosphereModel{<:Any, <:Any, <:HIPNative, <:SSPRungeKutta3}

# Whole-step seam (src/TimeSteppers/ssp_runge_kutta_3.jl:209-278)
function OceananigansTimeSteppers.time_step!(model::HIPModel, Δt; callbacks=[])
    ctx = context(model)
    model.clock.iteration == 0 && update_state!(model, callbacks; compute_tendencies=true)
    rc = ccall((:bz_time_step_anelastic, libbreeze_hip), Cint,
               (Ptr{Cvoid}, Ref{BzState}, Ref{BzPrognostic}, Ref{BzPrognostic}, Cdouble),
               ctx, state(model), prognostic(model.timestepper.U⁰), prognostic(model.timestepper.Gⁿ), Δt)
    check(rc, "bz_time_step_anelastic", ctx)
    tick!(model.clock, Δt)
    return nothing
end

# Multi-step seam: n steps with nothing reading the model in between — many_time_steps! of the benchmark driver
# (benchmarking/src/timestepping.jl:11-16) and the stretch of run!(simulation) up to the next callback / output-writer actuation.
# Every step but the last skips the projection + diagnosis pass (model.velocities, θ, qᵛ, T, pressure anomaly are host-side products);
# diagnose_last = true leaves exactly what n calls of time_step! leave.
function many_time_steps!(model::HIPModel, Δt, n::Integer; diagnose_last::Bool=true)
    n <= 0 && return nothing
    ctx = context(model)
    model.clock.iteration == 0 && update_state!(model; compute_tendencies=true)
    rc = ccall((:bz_time_steps_anelastic, libbreeze_hip), Cint,
               (Ptr{Cvoid}, Ref{BzState}, Ref{BzPrognostic}, Ref{BzPrognostic}, Cdouble, Cint, Cint),
               ctx, state(model), prognostic(model.timestepper.U⁰), prognostic(model.timestepper.Gⁿ), Δt, n, diagnose_last ? 1 : 0)
    check(rc, "bz_time_steps_anelastic", ctx)
    for _ in 1:n
        tick!(model.clock, Δt)
    end
    return nothing
end

# iterations until something scheduled on the simulation wants to look at the model (IterationInterval schedules; any other schedule: 1)
function iterations_to_next_actuation(sim)
    n = sim.stop_iteration - sim.model.clock.iteration
    for item in Iterators.flatten((values(sim.callbacks), values(sim.output_writers), values(sim.diagnostics)))
        sched = item.schedule
        n = sched isa IterationInterval ? min(n, sched.interval - mod(sim.model.clock.iteration - sched.offset, sched.interval)) : 1
    end
    return max(1, Int(min(n, typemax(Int32))))
end

# Simulation time_step! for the HIP model: fixed-Δt stretches between actuations go through the multi-step seam
function time_steps_to_next_actuation!(sim)
    n = iterations_to_next_actuation(sim)
    many_time_steps!(sim.model, sim.Δt, n; diagnose_last=true)
    return n
end

# Per-operator seams (src/AtmosphereModels/update_atmosphere_model_state.jl:41-68; src/AnelasticEquations/anelastic_time_stepping.jl:26-78)
function OceananigansTimeSteppers.update_state!(model::HIPModel, callbacks=[]; compute_tendencies=true)
    ctx = context(model)
    rc = ccall((:bz_update_state, libbreeze_hip), Cint, (Ptr{Cvoid}, Ref{BzState}, Ref{BzPrognostic}, Cint),
               ctx, state(model), prognostic(model.timestepper.Gⁿ), compute_tendencies ? 1 : 0)
    check(rc, "bz_update_state", ctx)
    return nothing
end
function AtmosphereModels.compute_pressure_correction!(model::HIPModel, Δt)
    ctx = context(model)
    check(ccall((:bz_compute_pressure_correction, libbreeze_hip), Cint, (Ptr{Cvoid}, Ref{BzState}, Cdouble),
                ctx, state(model), Δt), "bz_compute_pressure_correction", ctx)
end
function AtmosphereModels.make_pressure_correction!(model::HIPModel, Δt)
    ctx = context(model)
    check(ccall((:bz_make_pressure_correction, libbreeze_hip), Cint, (Ptr{Cvoid}, Ref{BzState}, Cdouble),
                ctx, state(model), Δt), "bz_make_pressure_correction", ctx)
end

# AtmosphereModel(grid; momentum_advection, scalar_advection) with schemes of different orders (atmosphere_model.jl:80-82,148-158):
# the context is created with the momentum order; this hands over the scalars' order (5, 7 or 9)
function set_scalar_advection_order!(ctx, order::Integer)
    check(ccall((:bz_set_scalar_advection_order, libbreeze_hip), Cint, (Ptr{Cvoid}, Cint), ctx, order), "bz_set_scalar_advection_order", ctx)
end

# Gc = -div_ρUc(c) of one centre field with the model's velocities: the launch of compute_scalar_tendency!
# (update_atmosphere_model_state.jl:390-393) and what benchmarking/src/scalar_tendency.jl:16-25 times
function compute_scalar_tendency!(Gc, model::HIPModel, c)
    ctx = context(model)
    U = model.velocities
    check(ccall((:bz_compute_scalar_tendency, libbreeze_hip), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
                ctx, pointer(parent(U.u)), pointer(parent(U.v)), pointer(parent(U.w)), pointer(parent(c)), pointer(parent(Gc))),
          "bz_compute_scalar_tendency", ctx)
end

##### ---------------------------------------------------------------------------------------------------------------
##### Physics attachments of the BOMEX / supercell configurations: the context builder calls these once, right after
##### bz_create, when the model carries the corresponding component (include/breeze_hip.h, same section names).
##### ---------------------------------------------------------------------------------------------------------------
struct BzSmagorinskyLilly
    smagorinsky_coefficient::Cdouble; reduction_factor::Cdouble; prandtl_number::Cdouble
end

struct BzColumnForcings
    u_forcing::Ptr{Cdouble}; v_forcing::Ptr{Cdouble}; theta_forcing::Ptr{Cdouble}; moisture_forcing::Ptr{Cdouble}
    energy_forcing::Ptr{Cdouble}; subsidence_vertical_velocity::Ptr{Cdouble}
    subsidence_u::Int32; subsidence_v::Int32; subsidence_theta::Int32; subsidence_moisture::Int32
    coriolis_f::Cdouble; bottom_theta_flux::Cdouble; bottom_moisture_flux::Cdouble; bottom_drag_rho0_ustar2::Cdouble; bottom_drag_epsilon::Cdouble
    bottom_energy_flux::Cdouble      # a constant flux keyed ρe in a θ model: Q / cᵖᵐ enters ρθ (EnergyFluxBoundaryCondition)
end

struct BzTracerFields
    density::Ptr{Cdouble}; specific::Ptr{Cdouble}; U0::Ptr{Cdouble}; G::Ptr{Cdouble}
end

"closure = SmagorinskyLilly(): νₑ is `model.closure_fields.νₑ` (src/AtmosphereModels/atmosphere_model.jl:272-276).  Anelastic and
compressible contexts alike (bz_create_compressible: one device, periodic in x and y)."
function attach_closure!(ctx, closure, νₑ)
    c = closure.coefficient              # LillyCoefficient(smagorinsky, reduction_factor); Pr from closure.Pr
    cl = BzSmagorinskyLilly(c.smagorinsky, c.reduction_factor, first(values(closure.Pr)))
    check(ccall((:bz_set_closure, libbreeze_hip), Cint, (Ptr{Cvoid}, Ref{BzSmagorinskyLilly}, Ptr{Cdouble}),
                ctx, cl, pointer(parent(νₑ))), "bz_set_closure", ctx)
end

struct BzScalarDiffusivity
    formulation::Int32; time_discretization::Int32
    nu::Cdouble; kappa::Cdouble
end

"""
closure = ScalarDiffusivity(ν, κ) / VerticalScalarDiffusivity(ν, κ): numbers or `(Center, Center, Center)` fields the caller keeps alive
and may rewrite between steps (validation/DCMIP2016_TC/dcmip2016_tc.jl:277-292); one κ for every scalar.  Compressible contexts take the
explicit discretisation only (the library returns BZ_ERR_UNSUPPORTED for the vertically implicit one).  NOT RUN: no Julia is installed
where this library is built.
"""
function attach_scalar_diffusivity!(ctx, closure, vertical::Bool, implicit::Bool)
    ν, κ = closure.ν, closure.κ isa NamedTuple ? first(values(closure.κ)) : closure.κ
    fieldptr(K) = K isa Number ? Ptr{Cdouble}(C_NULL) : pointer(parent(K))
    number(K) = K isa Number ? Cdouble(K) : 0.0
    sd = BzScalarDiffusivity(Int32(vertical), Int32(implicit), number(ν), number(κ))
    GC.@preserve ν κ check(ccall((:bz_set_scalar_diffusivity, libbreeze_hip), Cint, (Ptr{Cvoid}, Ref{BzScalarDiffusivity}, Ptr{Cdouble}, Ptr{Cdouble}),
                                 ctx, sd, fieldptr(ν), fieldptr(κ)), "bz_set_scalar_diffusivity", ctx)
end

"""
Column forcings of examples/bomex.jl:104-207.  `profiles` holds host `Vector{Float64}`s evaluated once from the model's
materialized forcings (Array(interior(field, 1, 1, :))): geostrophic -f vᵍ / +f uᵍ, Forcing(field) profiles, the subsidence wˢ
on faces; `flags` says which specific fields carry a SubsidenceForcing; fluxes are the bottom FluxBoundaryCondition values.
"""
function attach_forcings!(ctx, profiles::NamedTuple, flags::NamedTuple, f, Jθ, Jq, ρ₀u★², ϵ = 0.0, 𝒬 = 0.0)
    p(name) = haskey(profiles, name) ? pointer(profiles[name]) : Ptr{Cdouble}(C_NULL)
    F = BzColumnForcings(p(:u), p(:v), p(:θ), p(:q), p(:e), p(:wˢ),
                         flags.u, flags.v, flags.θ, flags.q, f, Jθ, Jq, ρ₀u★², ϵ, 𝒬)      # ϵ: the drag's regulariser (convective_boundary_layer.jl:142-146)
    GC.@preserve profiles check(ccall((:bz_set_forcings, libbreeze_hip), Cint, (Ptr{Cvoid}, Ref{BzColumnForcings}), ctx, F),
                                "bz_set_forcings", ctx)
end

struct BzColumnRelaxation
    rate_u::Ptr{Cdouble}; target_u::Ptr{Cdouble}; rate_v::Ptr{Cdouble}; target_v::Ptr{Cdouble}; rate_w::Ptr{Cdouble}; target_w::Ptr{Cdouble}
    rate_theta::Ptr{Cdouble}; target_theta::Ptr{Cdouble}; rate_moisture::Ptr{Cdouble}; target_moisture::Ptr{Cdouble}
    specific_mask::Int32
end

"""
Sponge layers: every `Relaxation(rate, mask::GaussianMask{:z}, target)` of `model.forcing` (examples/rico.jl:103-105,164;
neutral_atmospheric_boundary_layer.jl:103-136) as two host columns, `rate .* mask.(z)` and `target.(z)` at the field's vertical nodes
(ρw / w: the Nz + 1 faces).  `columns = (; u = (rate, target), w = ..., θ = ..., q = ...)`; `specific` lists the entries keyed by the
specific names u, v, w (their forcing is ρᵣ F).
"""
function attach_relaxation!(ctx, columns::NamedTuple, specific = ())
    p(name, i) = haskey(columns, name) ? pointer(columns[name][i]) : Ptr{Cdouble}(C_NULL)
    mask = Int32((:u in specific) + 2 * (:v in specific) + 4 * (:w in specific))
    R = BzColumnRelaxation(p(:u, 1), p(:u, 2), p(:v, 1), p(:v, 2), p(:w, 1), p(:w, 2), p(:θ, 1), p(:θ, 2), p(:q, 1), p(:q, 2), mask)
    GC.@preserve columns check(ccall((:bz_set_relaxation, libbreeze_hip), Cint, (Ptr{Cvoid}, Ref{BzColumnRelaxation}), ctx, R),
                               "bz_set_relaxation", ctx)
end

# ---- wind- and stability-dependent bulk fluxes on a filtered surface state (include/breeze_hip.h: bz_surface_layer) ----
# The structs mirror the header field by field.  NOTHING in this section has been run: no Julia is installed where this library is built.
struct BzPolynomialCoefficient
    a0::Cdouble; a1::Cdouble; a2::Cdouble
    roughness_length::Cdouble; minimum_wind_speed::Cdouble
    stability::Int32; reserved::Int32
    scalar_roughness_length::Cdouble
    stable_unstable_transition::Cdouble; strongly_stable_transition::Cdouble
    au11::Cdouble; bu11::Cdouble; bu12::Cdouble; au21::Cdouble; au22::Cdouble; bu31::Cdouble; bu32::Cdouble; bu33::Cdouble
    aw11::Cdouble; aw12::Cdouble; aw21::Cdouble; aw22::Cdouble; bw11::Cdouble; bw12::Cdouble; bw21::Cdouble; bw22::Cdouble
    as11::Cdouble; as21::Cdouble; bs11::Cdouble; bs21::Cdouble; bs22::Cdouble
    gamma_d::Cdouble; gamma_t::Cdouble; psi_a::Cdouble; psi_b::Cdouble; psi_c::Cdouble; psi_d::Cdouble
end

struct BzSurfaceFlux
    enabled::Int32; polynomial::Int32
    coefficient::Cdouble; gustiness::Cdouble
    surface_temperature::Cdouble
    surface_temperature_field::Ptr{Cdouble}      # HOST (Ny × Nx), copied by the call
    poly::BzPolynomialCoefficient
end

struct BzSurfaceLayer
    drag::BzSurfaceFlux; heat::BzSurfaceFlux; vapor::BzSurfaceFlux
    surface_pressure::Cdouble; standard_pressure::Cdouble
    liquid_latent_heat::Cdouble; liquid_heat_capacity::Cdouble; energy_reference_temperature::Cdouble
    triple_point_temperature::Cdouble; triple_point_pressure::Cdouble
    filtered::Int32; filter_height_set::Int32
    filter_height::Cdouble; filter_timescale::Cdouble
    filter_stage_mask::Int32; reserved::Int32
end

"""
`bz_polynomial_coefficient` of a materialized `PolynomialCoefficient` (polynomial filled by the condition's type).
"""
function polynomial_record(coef)
    sf = coef.stability_function
    on = !isnothing(sf)
    sf = on ? sf : Breeze.BoundaryConditions.FittedStabilityFunction(coef.roughness_length / 7.3)
    m, p = sf.richardson_number_mapping, sf.stability_function_parameters
    a₀, a₁, a₂ = coef.polynomial
    BzPolynomialCoefficient(a₀, a₁, a₂, coef.roughness_length, coef.minimum_wind_speed, Int32(on), Int32(0), sf.scalar_roughness_length,
                            m.stable_unstable_transition, m.strongly_stable_transition,
                            m.aᵘ₁₁, m.bᵘ₁₁, m.bᵘ₁₂, m.aᵘ₂₁, m.aᵘ₂₂, m.bᵘ₃₁, m.bᵘ₃₂, m.bᵘ₃₃,
                            m.aʷ₁₁, m.aʷ₁₂, m.aʷ₂₁, m.aʷ₂₂, m.bʷ₁₁, m.bʷ₁₂, m.bʷ₂₁, m.bʷ₂₂,
                            m.aˢ₁₁, m.aˢ₂₁, m.bˢ₁₁, m.bˢ₂₁, m.bˢ₂₂, p.γᴰ, p.γᵀ, p.a, p.b, p.c, p.d)
end

const NO_POLYNOMIAL = BzPolynomialCoefficient(ntuple(_ -> 0.0, 5)..., Int32(0), Int32(0), ntuple(_ -> 0.0, 30)...)
const NO_SURFACE_FLUX = BzSurfaceFlux(Int32(0), Int32(0), 0.0, 0.0, 0.0, Ptr{Cdouble}(C_NULL), NO_POLYNOMIAL)

"""
One bulk condition (`BulkDragFunction` / `BulkSensibleHeatFluxFunction` / `BulkVaporFluxFunction`, materialized) as a `BzSurfaceFlux`;
`T₀host` is `nothing` or the host copy `Array(interior(T₀, :, :, 1))` (x fastest), kept alive by the caller for the call.
"""
function surface_flux_record(bf, T₀host)
    C = bf.coefficient
    poly = C isa Number ? NO_POLYNOMIAL : polynomial_record(C)
    T₀ = isnothing(T₀host) ? Cdouble(bf.surface_temperature) : Cdouble(first(T₀host))
    BzSurfaceFlux(Int32(1), Int32(!(C isa Number)), C isa Number ? Cdouble(C) : 0.0, Cdouble(bf.gustiness), T₀,
                  isnothing(T₀host) ? Ptr{Cdouble}(C_NULL) : pointer(T₀host), poly)
end

"""
Attach the surface layer: `conditions = (; drag, heat, vapor)` of materialized condition functions (or `nothing`), `T₀ = (; drag, heat, vapor)`
host arrays or `nothing`, `fv` the shared `FilteredSurfaceVelocities` or `nothing`, `stage_mask` what the model's clock does: bit s - 1 set
when `update_state!` of stage s sees a new `(clock.iteration, clock.stage)` key.
"""
function attach_surface_layer!(ctx, conditions::NamedTuple, T₀::NamedTuple, p₀, pˢᵗ, constants, fv = nothing, stage_mask = 0b101)
    rec(name) = isnothing(conditions[name]) ? NO_SURFACE_FLUX : surface_flux_record(conditions[name], T₀[name])
    liq = constants.liquid
    L = BzSurfaceLayer(rec(:drag), rec(:heat), rec(:vapor), p₀, pˢᵗ, liq.reference_latent_heat, liq.heat_capacity,
                       constants.energy_reference_temperature, constants.triple_point_temperature, constants.triple_point_pressure,
                       Int32(!isnothing(fv)), Int32(!isnothing(fv) && !isnothing(fv.height)),
                       (isnothing(fv) || isnothing(fv.height)) ? 0.0 : Cdouble(fv.height), isnothing(fv) ? Inf : Cdouble(fv.filter_timescale),
                       Int32(stage_mask), Int32(0))
    GC.@preserve T₀ check(ccall((:bz_set_surface_layer, libbreeze_hip), Cint, (Ptr{Cvoid}, Ref{BzSurfaceLayer}), ctx, L), "bz_set_surface_layer", ctx)
end

detach_surface_layer!(ctx) =
    check(ccall((:bz_set_surface_layer, libbreeze_hip), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), ctx, C_NULL), "bz_set_surface_layer", ctx)

# initialize!(model) / update!(fv, …, Δt) with ϵ = Δt / τ; `s` is the Ref{BzState} of the model
initialize_surface_layer!(ctx, s) =
    check(ccall((:bz_surface_layer_initialize, libbreeze_hip), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), ctx, s), "bz_surface_layer_initialize", ctx)
update_surface_layer!(ctx, s, ϵ) =
    check(ccall((:bz_surface_layer_update, libbreeze_hip), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cdouble), ctx, s, ϵ), "bz_surface_layer_update", ctx)

# the filtered 2-D fields as host (Nx, Ny) arrays (x fastest); which = 0 û, 1 v̂, 2 θ̂ᵥ, 3 θ̂, 4 q̂
get_filtered_surface_field!(host::Array{Float64}, ctx, which) =
    check(ccall((:bz_surface_layer_get_filtered, libbreeze_hip), Cint, (Ptr{Cvoid}, Cint, Ptr{Cdouble}), ctx, which, host), "bz_surface_layer_get_filtered", ctx)
set_filtered_surface_field!(ctx, which, host::Array{Float64}) =
    check(ccall((:bz_surface_layer_set_filtered, libbreeze_hip), Cint, (Ptr{Cvoid}, Cint, Ptr{Cdouble}), ctx, which, host), "bz_surface_layer_set_filtered", ctx)

"""
`Forcing(f(x, y, z, t))` / `Forcing(field)` on θ / e (specific = true) or ρθ / ρe: `F` is a CenterField the extension fills from the forcing
(and refreshes from a callback when it depends on time); the library reads it at every tendency evaluation.
"""
attach_field_forcing!(ctx, F, specific::Bool) =
    check(ccall((:bz_set_field_forcing, libbreeze_hip), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Cint), ctx, pointer(parent(F)), specific),
          "bz_set_field_forcing", ctx)

"tracers = (:a, :b): density = model.tracers[n]; `specific` is an extra centre field owned by the extension."
function attach_tracers!(ctx, model, specific_fields)
    ts = model.timestepper
    t = [BzTracerFields(pointer(parent(model.tracers[n])), pointer(parent(specific_fields[n])),
                        pointer(parent(ts.U⁰[n])), pointer(parent(ts.Gⁿ[n]))) for n in keys(model.tracers)]
    check(ccall((:bz_set_tracers, libbreeze_hip), Cint, (Ptr{Cvoid}, Int32, Ptr{BzTracerFields}), ctx, length(t), t),
          "bz_set_tracers", ctx)
end

"compute_flux_bc_tendencies!(model) (src/AtmosphereModels/update_atmosphere_model_state.jl:418-434)"
function OceananigansTimeSteppers.compute_flux_bc_tendencies!(model::HIPModel)
    ctx = context(model)
    check(ccall((:bz_compute_flux_bc_tendencies, libbreeze_hip), Cint, (Ptr{Cvoid}, Ref{BzState}, Ref{BzPrognostic}),
                ctx, state(model), prognostic(model.timestepper.Gⁿ)), "bz_compute_flux_bc_tendencies", ctx)
    return nothing
end

##### ---------------------------------------------------------------------------------------------------------------
##### CompressibleDynamics + SplitExplicitTimeDiscretization (src/TimeSteppers/acoustic_runge_kutta_3.jl,
##### src/CompressibleEquations/acoustic_substepping.jl)
##### ---------------------------------------------------------------------------------------------------------------
using Breeze.TimeSteppers: AcousticRungeKutta3
using Breeze.CompressibleEquations: CompressibleDynamics, ThermalDivergenceDamping, ProportionalSubsteps, ConstantSubstepSize, MonolithicFirstStage
import Breeze.CompressibleEquations: acoustic_rk3_substep_loop!

struct BzCompressibleState
    ρᵈ::Ptr{Float64}; ρ::Ptr{Float64}; ρu::Ptr{Float64}; ρv::Ptr{Float64}; ρw::Ptr{Float64}; ρθ::Ptr{Float64}; ρq::Ptr{Float64}
    u::Ptr{Float64}; v::Ptr{Float64}; w::Ptr{Float64}; θ::Ptr{Float64}; q::Ptr{Float64}; T::Ptr{Float64}; p::Ptr{Float64}
end
struct BzCompressiblePrognostic
    ρᵈ::Ptr{Float64}; ρu::Ptr{Float64}; ρv::Ptr{Float64}; ρw::Ptr{Float64}; ρθ::Ptr{Float64}; ρq::Ptr{Float64}
end
struct BzAcousticSubstepper       # field order of include/breeze_hip.h: bz_acoustic_substepper
    Π::Ptr{Float64}; θ::Ptr{Float64}; γR::Ptr{Float64}
    ρ′::Ptr{Float64}; ρθ′::Ptr{Float64}; ρu′::Ptr{Float64}; ρv′::Ptr{Float64}; ρw′::Ptr{Float64}
    ρ′★::Ptr{Float64}; ρθ′★::Ptr{Float64}; ρθ′ˢ⁻::Ptr{Float64}
    ū::Ptr{Float64}; v̄::Ptr{Float64}; w̄::Ptr{Float64}
    Gˢρw::Ptr{Float64}; rhs::Ptr{Float64}
end
struct BzSplitExplicit
    substeps::Int32; damp_vertical::Int32; apply_first::Int32; newton_maxiter::Int32
    acoustic_cfl::Float64; forward_weight::Float64; damping_coefficient::Float64
    f_θ::Float64; f_w::Float64; newton_abstol::Float64
    direct_divergence_damping::Int32; sponge_ramp::Int32          # ramp: 0 none, 1 LinearRamp, 2 CubicRamp, 3 Sin2Ramp
    sponge_damping_rate::Float64; sponge_depth::Float64
    substep_distribution::Int32                                   # 0 ProportionalSubsteps, 1 ConstantSubstepSize, 2 MonolithicFirstStage
    substep_float_bytes::Int32                                    # 0: eltype(grid); 4: the substepper's working fields are Float32 arrays
    damping_length_scale::Float64                                 # ThermalDivergenceDamping(length_scale): 0 = nothing (local scale)
end
distcode(::ProportionalSubsteps) = Int32(0)
distcode(::ConstantSubstepSize) = Int32(1)
distcode(::MonolithicFirstStage) = Int32(2)
rampcode(::Nothing) = Int32(0)
rampcode(s::UpperSponge) = s.ramp isa LinearRamp ? Int32(1) : s.ramp isa CubicRamp ? Int32(2) : s.ramp isa Sin2Ramp ? Int32(3) :
                           error("BreezeHIP: custom sponge ramps are not supported")
struct BzExnerReference
    pst::Float64; pressure::Ptr{Float64}; density::Ptr{Float64}
end

const HIPAcousticModel = AtmosphereModel{<:CompressibleDynamics, <:Any, <:HIPNative, <:AcousticRungeKutta3}

cstate(m) = BzCompressibleState(devptr(m.dynamics.dry_density), devptr(m.dynamics.total_density),
                                devptr(m.momentum.ρu), devptr(m.momentum.ρv), devptr(m.momentum.ρw),
                                devptr(m.formulation.potential_temperature_density), devptr(m.moisture_density),
                                devptr(m.velocities.u), devptr(m.velocities.v), devptr(m.velocities.w),
                                devptr(m.formulation.potential_temperature), devptr(m.microphysical_fields.qᵛ),
                                devptr(m.temperature), devptr(m.dynamics.pressure))
cprognostic(nt) = BzCompressiblePrognostic(devptr(nt.ρᵈ), devptr(nt.ρu), devptr(nt.ρv), devptr(nt.ρw), devptr(nt.ρθ), devptr(nt.ρqᵛ))
substepper(a) = BzAcousticSubstepper(devptr(a.linearization_exner), devptr(a.linearization_potential_temperature),
                                     devptr(a.linearization_gamma_R_mixture), devptr(a.density_perturbation),
                                     devptr(a.density_potential_temperature_perturbation),
                                     devptr(a.momentum_perturbation.u), devptr(a.momentum_perturbation.v), devptr(a.momentum_perturbation.w),
                                     devptr(a.density_predictor), devptr(a.density_potential_temperature_predictor),
                                     devptr(a.previous_density_potential_temperature_perturbation),
                                     devptr(a.time_averaged_velocities.u), devptr(a.time_averaged_velocities.v), devptr(a.time_averaged_velocities.w),
                                     devptr(a.slow_vertical_momentum_tendency), devptr(a.vertical_solver_source_term))

function create_compressible_context(model)
    grid = model.grid
    Nx, Ny, Nz = size(grid); Hx, Hy, Hz = Oceananigans.Grids.halo_size(grid)
    zf = collect(Float64, znodes(grid, Face()))
    c = model.thermodynamic_constants
    a = model.timestepper.substepper
    ref = model.dynamics.reference_state
    hostcol(f) = collect(Float64, vec(Array(parent(f))))
    p, ρ = ref === nothing ? (Float64[], Float64[]) : (hostcol(ref.pressure), hostcol(ref.density))
    solver = model.formulation.temperature_solver                      # NewtonSolver(reltol = 0)
    damp = a.damping
    td = BzSplitExplicit(something(a.substeps, 0), damp isa ThermalDivergenceDamping && damp.damp_vertical,
                         a.apply_first_substep_pressure_gradient, solver.maxiter, a.acoustic_cfl, a.forward_weight,
                         damp isa Union{ThermalDivergenceDamping, DirectDivergenceDamping} ? damp.coefficient : -1.0,
                         a.thermodynamic_tendency_factor, a.vertical_momentum_tendency_factor, solver.abstol,
                         damp isa DirectDivergenceDamping, rampcode(a.sponge),
                         a.sponge === nothing ? 0.0 : a.sponge.damping_rate, a.sponge === nothing ? 0.0 : a.sponge.depth,
                         distcode(a.substep_distribution),
                         eltype(a.density_perturbation) === Float32 && eltype(grid) === Float64 ? Int32(4) : Int32(0),
                         damp isa ThermalDivergenceDamping && damp.length_scale !== nothing ? Float64(damp.length_scale) : 0.0)
    ctx = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve zf p ρ begin
        g = BzGrid(Nx, Ny, Nz, Hx, Hy, Hz, map(topocode, topology(grid)), 8, grid.Δxᶜᵃᵃ, grid.Δyᵃᶜᵃ, pointer(zf),
                   grid.z.Δᵃᵃᶜ isa Number ? 1 : 0, 0)
        k = BzConstants(c.gravitational_acceleration, c.molar_gas_constant / c.dry_air.molar_mass,
                        c.molar_gas_constant / c.vapor.molar_mass, c.dry_air.heat_capacity, c.vapor.heat_capacity)
        r = BzExnerReference(model.dynamics.standard_pressure, ref === nothing ? C_NULL : pointer(p), ref === nothing ? C_NULL : pointer(ρ))
        rc = ccall((:bz_create_compressible, libbreeze_hip), Cint,
                   (Ref{Ptr{Cvoid}}, Ref{BzGrid}, Ref{BzConstants}, Ref{BzExnerReference}, Ref{BzSplitExplicit}, Cint), ctx, g, k, r, td, 5)
        rc == 0 || error("bz_create_compressible failed with code $rc")
    end
    # Bounded x / y: which sides carry an active open boundary condition on the wall-normal momentum (is_active_open_bc,
    # src/CompressibleEquations/acoustic_substepping.jl:1318) and the relaxation factor of the substepper; the loop seam below then enforces the
    # lateral boundaries itself (_zero_{x,y}_wall_face!, _relax_open_boundary_{x,y}!, :1323-1395).  On such a grid only the loop seam is forwarded:
    # the fills with the model's boundary conditions and compute_velocities! after _recover_full_state! (:1584-1587) stay on the Julia side.
    TX, TY, _ = topology(grid)
    if TX === Bounded || TY === Bounded
        bu, bv = model.momentum.ρu.boundary_conditions, model.momentum.ρv.boundary_conditions
        active(bc) = (bc isa BoundaryCondition{<:NormalFlow}) && !(bc.condition isa Nothing)
        rc = ccall((:bz_set_acoustic_lateral_boundaries, libbreeze_hip), Cint, (Ptr{Cvoid}, Cint, Cint, Cint, Cint, Cdouble), ctx[],
                   TX === Bounded && active(bu.west), TX === Bounded && active(bu.east), TY === Bounded && active(bv.south),
                   TY === Bounded && active(bv.north), a.open_boundary_relaxation)
        check(rc, "bz_set_acoustic_lateral_boundaries", ctx[])
    end
    # closure terms are slow terms of the split-explicit step (src/TimeSteppers/acoustic_substep_helpers.jl:55-93); the library ends every
    # update_state! with compute_closure_fields!.  NOT RUN (no Julia where this library is built).
    cl = model.closure
    if cl isa Oceananigans.TurbulenceClosures.SmagorinskyLilly
        attach_closure!(ctx[], cl, model.closure_fields.νₑ)
    elseif cl isa Oceananigans.TurbulenceClosures.ScalarDiffusivity
        F = typeof(cl).parameters[2]                                    # ThreeDimensionalFormulation | VerticalFormulation
        attach_scalar_diffusivity!(ctx[], cl, F <: Oceananigans.TurbulenceClosures.VerticalFormulation,
                                   typeof(cl).parameters[1] <: Oceananigans.TurbulenceClosures.VerticallyImplicitTimeDiscretization)
    elseif cl !== nothing
        error("closure = $(typeof(cl).name.name) is not implemented on the HIP compressible path")
    end
    return ctx[]
end
ccontext(model) = get!(() -> create_compressible_context(model), CONTEXTS, model)

# Whole-step seam (src/TimeSteppers/acoustic_runge_kutta_3.jl:264-319)
function OceananigansTimeSteppers.time_step!(model::HIPAcousticModel, Δt; callbacks=[])
    ctx = ccontext(model)
    OceananigansTimeSteppers.maybe_prepare_first_time_step!(model, Δt, callbacks)
    ts = model.timestepper
    rc = ccall((:bz_time_step_compressible, libbreeze_hip), Cint,
               (Ptr{Cvoid}, Ref{BzCompressibleState}, Ref{BzCompressiblePrognostic}, Ref{BzCompressiblePrognostic}, Ref{BzAcousticSubstepper}, Cdouble),
               ctx, cstate(model), cprognostic(ts.U⁰), cprognostic(ts.Gⁿ), substepper(ts.substepper), Δt)
    check(rc, "bz_time_step_compressible", ctx)
    tick!(model.clock, Δt)
    return nothing
end

# Loop seam (src/CompressibleEquations/acoustic_substepping.jl:1404)
function acoustic_rk3_substep_loop!(model::HIPAcousticModel, a, Δt, β_stage, U⁰)
    ctx = ccontext(model)
    rc = ccall((:bz_acoustic_substep_loop, libbreeze_hip), Cint,
               (Ptr{Cvoid}, Ref{BzCompressibleState}, Ref{BzCompressiblePrognostic}, Ref{BzCompressiblePrognostic}, Ref{BzAcousticSubstepper}, Cdouble, Cdouble),
               ctx, cstate(model), cprognostic(U⁰), cprognostic(model.timestepper.Gⁿ), substepper(a), Δt, β_stage)
    check(rc, "bz_acoustic_substep_loop", ctx)
    return nothing
end

function OceananigansTimeSteppers.update_state!(model::HIPAcousticModel, callbacks=[]; compute_tendencies=true)
    ctx = ccontext(model)
    ts = model.timestepper
    rc = ccall((:bz_compressible_update_state, libbreeze_hip), Cint,
               (Ptr{Cvoid}, Ref{BzCompressibleState}, Ref{BzCompressiblePrognostic}, Ref{BzAcousticSubstepper}, Cint),
               ctx, cstate(model), cprognostic(ts.Gⁿ), substepper(ts.substepper), compute_tendencies ? 1 : 0)
    check(rc, "bz_compressible_update_state", ctx)
    return nothing
end

#####
##### microphysics = InstantaneousPrecipitation(...) (src/Microphysics/instantaneous_precipitation.jl).  Like the rest of this file these
##### three bindings have never been run (Julia is not available in the build image); the Python host (breeze.jl_amd/) drives the same
##### entry points in tests/test_instantaneous_precipitation.py.
#####
struct BzSaturationAdjustment
    liquid_latent_heat::Float64; liquid_heat_capacity::Float64; energy_reference_temperature::Float64
    triple_point_temperature::Float64; triple_point_pressure::Float64
    abstol::Float64
    maxiter::Int32; reserved::Int32
end

"Attach the scheme to a compressible context: the wrapped SaturationAdjustment's solver and the liquid-phase constants; `precipitation_rate` = model.microphysical_fields.precipitation_rate."
function attach_instantaneous_precipitation!(ctx, model)
    c = model.thermodynamic_constants
    solver = model.microphysics.saturation_adjustment.solver
    P = BzSaturationAdjustment(c.liquid.reference_latent_heat, c.liquid.heat_capacity, c.energy_reference_temperature,
                               c.triple_point_temperature, c.triple_point_pressure, solver.abstol, Int32(solver.maxiter), Int32(0))
    check(ccall((:bz_set_instantaneous_precipitation, libbreeze_hip), Cint, (Ptr{Cvoid}, Ref{BzSaturationAdjustment}, Ptr{Cdouble}),
                ctx, P, devptr(model.microphysical_fields.precipitation_rate)), "bz_set_instantaneous_precipitation", ctx)
    attach_saturation_vapor_pressure!(ctx, c)
    return nothing
end

# bz_flatau_polynomial: the isbits NTuples lay out as the C arrays
struct BzFlatauPolynomial
    liquid_coefficients::NTuple{9, Float64}; ice_coefficients::NTuple{9, Float64}
    reference_temperature::Float64; minimum_temperature_offset::Float64
end

"""saturation_vapor_pressure of the constants, after the adjustment that evaluates it is attached: a `FlatauPolynomial` goes to
bz_set_saturation_vapor_pressure_polynomial; every other formulation leaves the context on Clausius-Clapeyron, as before."""
function attach_saturation_vapor_pressure!(ctx, constants)
    formula = constants.saturation_vapor_pressure
    if formula isa Breeze.Thermodynamics.FlatauPolynomial
        P = BzFlatauPolynomial(map(Float64, formula.liquid_coefficients), map(Float64, formula.ice_coefficients),
                               Float64(formula.reference_temperature), Float64(formula.minimum_temperature_offset))
        check(ccall((:bz_set_saturation_vapor_pressure_polynomial, libbreeze_hip), Cint, (Ptr{Cvoid}, Ref{BzFlatauPolynomial}), ctx, P),
              "bz_set_saturation_vapor_pressure_polynomial", ctx)
    end
    return nothing
end

# microphysics_model_update!(::InstantaneousPrecipitation, model) (instantaneous_precipitation.jl:115-141); bz_time_step_compressible calls it itself
function AtmosphereModels.microphysics_model_update!(::Breeze.Microphysics.InstantaneousPrecipitation, model::HIPAcousticModel)
    ctx = ccontext(model)
    ts = model.timestepper
    rc = ccall((:bz_instantaneous_precipitation_update, libbreeze_hip), Cint,
               (Ptr{Cvoid}, Ref{BzCompressibleState}, Ref{BzCompressiblePrognostic}, Ref{BzAcousticSubstepper}, Cdouble),
               ctx, cstate(model), cprognostic(ts.Gⁿ), substepper(ts.substepper), model.clock.last_Δt)
    check(rc, "bz_instantaneous_precipitation_update", ctx)
    return nothing
end

# negative_moisture_correction of a bulk scheme (src/AtmosphereModels/negative_moisture_correction.jl): the descriptor of
# bz_set_negative_moisture_correction.  Pointers and counts only: the same struct binds both precisions.
struct BzNegativeMoistureCorrection
    species_borrowing::Int32; vertical_borrowing::Int32
    n_mass::Int32; n_pairs::Int32; n_clamp::Int32; reserved::Int32
    mass::NTuple{4, Ptr{Cvoid}}
    number::NTuple{4, Ptr{Cvoid}}
    pair_mass::NTuple{4, Ptr{Cvoid}}
    clamp::NTuple{4, Ptr{Cvoid}}
end

pad4(ptrs) = ntuple(i -> i <= length(ptrs) ? Ptr{Cvoid}(ptrs[i]) : Ptr{Cvoid}(C_NULL), 4)

"""
Attach negative_moisture_correction(model.microphysics) to an anelastic context with an attached SaturationAdjustment (after
bz_set_saturation_adjustment): the species chain correction_moisture_fields (heaviest first; the lightest borrows from model.moisture_density),
correction_number_mass_pairs and correction_number_fields, at most four each.  `nothing` detaches.  The one- and two-moment schemes of the
CloudMicrophysics extension keep their own kernels; this call hands their fields to the column kernel.
"""
function attach_negative_moisture_correction!(ctx, model)
    μp, μ = model.microphysics, model.microphysical_fields
    correction = AtmosphereModels.negative_moisture_correction(μp)
    if correction === nothing
        check(ccall((:bz_set_negative_moisture_correction, libbreeze_hip), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), ctx, C_NULL),
              "bz_set_negative_moisture_correction", ctx)
        return nothing
    end
    species = correction isa AtmosphereModels.SpeciesBorrowing
    vertical = correction isa AtmosphereModels.VerticalBorrowing || (species && correction.vertical_borrowing !== nothing)
    mass = species ? map(devptr, AtmosphereModels.correction_moisture_fields(μp, μ)) : ()
    pairs = species ? AtmosphereModels.correction_number_mass_pairs(μp, μ) : ()
    clamp = species ? map(devptr, AtmosphereModels.correction_number_fields(μp, μ)) : ()
    max(length(mass), length(pairs), length(clamp)) <= 4 || error("BreezeHIP: at most four species, pairs and clamped number fields")
    D = BzNegativeMoistureCorrection(Int32(species), Int32(vertical), Int32(length(mass)), Int32(length(pairs)), Int32(length(clamp)), Int32(0),
                                     pad4(mass), pad4(map(p -> devptr(p[1]), pairs)), pad4(map(p -> devptr(p[2]), pairs)), pad4(clamp))
    check(ccall((:bz_set_negative_moisture_correction, libbreeze_hip), Cint, (Ptr{Cvoid}, Ref{BzNegativeMoistureCorrection}), ctx, D),
          "bz_set_negative_moisture_correction", ctx)
    return nothing
end

"fix_negative_moisture!(model) as its own launch (update_state! and the whole steps of the library run it themselves)."
function fix_negative_moisture!(model::HIPModel)
    ctx = context(model)
    check(ccall((:bz_fix_negative_moisture, libbreeze_hip), Cint, (Ptr{Cvoid}, Ref{BzState}), ctx, state(model)), "bz_fix_negative_moisture", ctx)
    return nothing
end

"Field(Integral(field, dims = 3)) into `out`, a device array of (Nx + 2Hx) × (Ny + 2Hy) reals (interior positions are written)."
function column_integral!(out, model::HIPAcousticModel, field)
    ctx = ccontext(model)
    check(ccall((:bz_column_integral, libbreeze_hip), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}), ctx, devptr(field), Ptr{Float64}(UInt(pointer(out)))),
          "bz_column_integral", ctx)
    return out
end


#####
##### Multi-GPU: one process per GPU, y-slabs, the communicator lives inside libbreeze_hip (bz_comm.hip)
#####
##### The rank-local RectilinearGrid is this rank's y-slab of the global (Periodic, Periodic, Bounded) domain.  MPI.jl (or any
##### launcher) is used for exactly two things: starting the ranks and broadcasting RCCL's 128-byte unique id.
#####

const BZ_UNIQUE_ID_BYTES = 128

"WENO(order = N) of the model's momentum scheme -> the weno_order argument of bz_create (5: tuned kernels; 7, 9: generic kernels)."
weno_order(advection) = 2 * Oceananigans.Advection.required_halo_size_x(advection isa NamedTuple ? advection.momentum : advection) - 1

"The scalars' order of a merged advection NamedTuple (atmosphere_model.jl:279-284); every scalar must share it (bz_set_scalar_advection_order)."
function scalar_weno_order(advection)
    advection isa NamedTuple || return weno_order(advection)
    orders = unique(2 * Oceananigans.Advection.required_halo_size_x(s) - 1 for (k, s) in pairs(advection) if k != :momentum)
    length(orders) <= 1 || error("BreezeHIP: one advection order for all scalars (got $orders)")
    return isempty(orders) ? weno_order(advection) : first(orders)
end

"Create the slab context of this rank and attach the RCCL communicator to it."
function slab_context!(model, y_nranks::Integer, y_rank::Integer, bcast_bytes!::Function)
    ctx = Ref{Ptr{Cvoid}}(C_NULL)
    grid, constants, reference = bz_grid(model.grid), bz_constants(model), bz_reference_state(model)
    rc = ccall((:bz_create_slab, libbreeze_hip), Cint,
               (Ref{Ptr{Cvoid}}, Ref{BzGrid}, Ref{BzConstants}, Ref{BzReferenceState}, Cint, Cint, Cint),
               ctx, grid, constants, reference, weno_order(model.advection), y_nranks, y_rank)
    rc == 0 || error("bz_create_slab failed with code $rc")
    id = zeros(UInt8, BZ_UNIQUE_ID_BYTES)
    if y_rank == 0
        rc = ccall((:bz_comm_unique_id, libbreeze_hip), Cint, (Ptr{UInt8},), id)
        rc == 0 || error("bz_comm_unique_id failed with code $rc")
    end
    bcast_bytes!(id)                     # e.g. id -> MPI.Bcast!(id, 0, MPI.COMM_WORLD)
    rc = ccall((:bz_comm_init_rccl, libbreeze_hip), Cint, (Ptr{Cvoid}, Ptr{UInt8}), ctx[], id)
    rc == 0 || error(unsafe_string(ccall((:bz_last_error, libbreeze_hip), Cstring, (Ptr{Cvoid},), ctx[])))
    return ctx[]
end

"set!(model; ...) on slabs ends with update_state! + halo exchange + the initial projection, all inside the library."
function finish_set!(model, ctx; enforce_mass_conservation = true)
    rc = ccall((:bz_comm_update_state_and_project, libbreeze_hip), Cint,
               (Ptr{Cvoid}, Ref{BzState}, Ref{BzPrognostic}, Cdouble, Cint),
               ctx, state(model), prognostic(model.timestepper.Gⁿ), 1.0, enforce_mass_conservation ? 1 : 0)
    rc == 0 || error(unsafe_string(ccall((:bz_last_error, libbreeze_hip), Cstring, (Ptr{Cvoid},), ctx)))
    return nothing
end

# time_step! needs no distributed method: bz_time_step_anelastic on a slab context with a communicator is the distributed step.

"Compressible model on slabs: the same communicator calls on a context made by bz_create_compressible_slab; time_step! is then
bz_time_step_compressible (per-substep halo exchange of the acoustic loop inside the library), update_state! the call below."
function compressible_slab_context!(model, y_nranks::Integer, y_rank::Integer, bcast_bytes!::Function, g, k, r, td)
    ctx = Ref{Ptr{Cvoid}}(C_NULL)
    rc = ccall((:bz_create_compressible_slab, libbreeze_hip), Cint,
               (Ref{Ptr{Cvoid}}, Ref{BzGrid}, Ref{BzConstants}, Ref{BzExnerReference}, Ref{BzSplitExplicit}, Cint, Cint, Cint),
               ctx, g, k, r, td, weno_order(model.advection), y_nranks, y_rank)
    rc == 0 || error("bz_create_compressible_slab failed with code $rc")
    id = zeros(UInt8, BZ_UNIQUE_ID_BYTES)
    if y_rank == 0
        rc = ccall((:bz_comm_unique_id, libbreeze_hip), Cint, (Ptr{UInt8},), id)
        rc == 0 || error("bz_comm_unique_id failed with code $rc")
    end
    bcast_bytes!(id)
    rc = ccall((:bz_comm_init_rccl, libbreeze_hip), Cint, (Ptr{Cvoid}, Ptr{UInt8}), ctx[], id)
    rc == 0 || error(unsafe_string(ccall((:bz_last_error, libbreeze_hip), Cstring, (Ptr{Cvoid},), ctx[])))
    return ctx[]
end

function compressible_update_state!(model, ctx; compute_tendencies = true)
    rc = ccall((:bz_comm_compressible_update_state, libbreeze_hip), Cint,
               (Ptr{Cvoid}, Ref{BzCompressibleState}, Ref{BzCompressiblePrognostic}, Ref{BzAcousticSubstepper}, Cint),
               ctx, cstate(model), cprognostic(model.timestepper.Gⁿ), substepper(model.timestepper.substepper), compute_tendencies ? 1 : 0)
    rc == 0 || error(unsafe_string(ccall((:bz_last_error, libbreeze_hip), Cstring, (Ptr{Cvoid},), ctx)))
    return nothing
end

# ---- output diagnostics (csrc/bz_diagnostics.hip): the operations of src/AtmosphereModels/Diagnostics/ and RelativeHumidity evaluated by one
# pointwise kernel, and Average(field, dims = (1, 2)).  An extension specialises `compute!(::Field{<:Any, <:Any, <:Any, <:KernelFunctionOperation{...}})`
# on the kernel-function types below and forwards here; `kinds` are bz_diagnostic_kind codes (| BZ_DIAG_DENSITY_WEIGHTED for the :density flavours).
struct BzDiagnosticInputs
    temperature::Ptr{Cvoid}; vapor::Ptr{Cvoid}; liquid::Ptr{Cvoid}; liquid_2::Ptr{Cvoid}; moisture::Ptr{Cvoid}
    pressure::Ptr{Cvoid}; density::Ptr{Cvoid}
    liquid_latent_heat::Cdouble; liquid_heat_capacity::Cdouble
    energy_reference_temperature::Cdouble; triple_point_temperature::Cdouble; triple_point_pressure::Cdouble
end
const BZ_DIAG_DENSITY_WEIGHTED = Int32(0x100)

"n diagnostics into n centre fields from one read of T, q^v, q^l (p, rho); `s` lets the library rebuild stale diagnostics first."
function compute_diagnostics!(ctx, s::BzState, inputs::BzDiagnosticInputs, kinds::Vector{Int32}, outputs::Vector{Ptr{Cvoid}})
    check(ccall((:bz_compute_diagnostics, libbreeze_hip), Cint,
                (Ptr{Cvoid}, Ref{BzState}, Ref{BzDiagnosticInputs}, Int32, Ptr{Int32}, Ptr{Ptr{Cvoid}}),
                ctx, s, inputs, length(kinds), kinds, outputs), "bz_compute_diagnostics", ctx)
end

# ---- discrete hydrostatic balance of the initial and the base state (csrc/bz_balance.hip).  Written against the header; this file has
# not been run (no Julia in the build environment). ----
"_compute_exner_reference_3d!: one balanced column per (i, j) of the device parent arrays θ and qᵛ (C_NULL: dry), upward from p₀."
function exner_columns!(ctx, θ::Ptr{Cvoid}, qᵛ::Ptr{Cvoid}, p₀::Real, π::Ptr{Cvoid}, p::Ptr{Cvoid}, ρ::Ptr{Cvoid})
    check(ccall((:bz_exner_columns, libbreeze_hip), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cdouble, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                ctx, θ, qᵛ, p₀, π, p, ρ), "bz_exner_columns", ctx)
    return nothing
end

"set_hydrostatically_balanced_density!(model, spec) (src/AtmosphereModels/set_to_mean.jl:271-310) on the state arrays, after update_state!."
function set_hydrostatically_balanced_density!(model::HIPAcousticModel, p₀::Real)
    ctx = ccontext(model)
    check(ccall((:bz_set_hydrostatically_balanced_density, libbreeze_hip), Cint, (Ptr{Cvoid}, Ref{BzCompressibleState}, Cdouble),
                ctx, cstate(model), p₀), "bz_set_hydrostatically_balanced_density", ctx)
    return nothing
end

"The context's reference columns again, from host arrays of Nz + 2Hz levels (parent(field)[1, 1, :] of the recomputed ExnerReferenceState,
halos filled): the tail of set_to_mean!(::ExnerReferenceState, model); update_state! follows."
function set_exner_reference_state!(model::HIPAcousticModel, p::Vector{Float64}, ρ::Vector{Float64})
    ctx = ccontext(model)
    GC.@preserve p ρ begin
        r = BzExnerReference(model.dynamics.standard_pressure, pointer(p), pointer(ρ))
        check(ccall((:bz_set_exner_reference_state, libbreeze_hip), Cint, (Ptr{Cvoid}, Ref{BzExnerReference}), ctx, r),
              "bz_set_exner_reference_state", ctx)
    end
    OceananigansTimeSteppers.update_state!(model; compute_tendencies=false)
    return nothing
end

"Average(field, dims = (1, 2)) of one centre or z-face parent array into a host profile of Nz (Nz + 1) values."
function horizontal_average!(profile::Vector{Float64}, ctx, field::Ptr{Cvoid}, z_face::Bool)
    check(ccall((:bz_horizontal_average, libbreeze_hip), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Cdouble}), ctx, field, z_face, profile),
          "bz_horizontal_average", ctx)
    return profile
end

# ---- turbulence statistics: Average(expression, dims = (1, 2)) of products, powers and ∂z (bz_horizontal_moments) ----
const BZ_MAX_MOMENT_FIELDS, BZ_MAX_MOMENTS, BZ_MAX_MOMENT_FACTORS = 8, 24, 3
"A field of a moment list: the device parent array and its location (0: Center, 1: Face)."
struct BzMomentField
    data::Ptr{Cvoid}
    face_x::Int32; face_y::Int32; face_z::Int32
end
"One moment: f[field[1]]^power[1] * ℑ(f[field[2]]^power[2]) * ℑ(f[field[3]]^power[3]) (0-based field indices), or ∂z of the single factor; at_center: @at((Center, Center, Center), ·)."
struct BzMoment
    n_factors::Int32
    field::NTuple{3, Int32}
    power::NTuple{3, Int32}
    dz::Int32
    at_center::Int32
end

"""
horizontal_moments!(profiles, nlev, ctx, fields, moments): every profile of the list from one pass over the fields;
`profiles` is (Nz + 1) × length(moments) (a column per moment, nlev[m] valid levels), host memory.
"""
function horizontal_moments!(profiles::Matrix{Float64}, nlev::Vector{Int32}, ctx, fields::Vector{BzMomentField}, moments::Vector{BzMoment})
    check(ccall((:bz_horizontal_moments, libbreeze_hip), Cint,
                (Ptr{Cvoid}, Int32, Ptr{BzMomentField}, Int32, Ptr{BzMoment}, Ptr{Cdouble}, Ptr{Int32}),
                ctx, length(fields), fields, length(moments), moments, profiles, nlev), "bz_horizontal_moments", ctx)
    return profiles
end

"Hand the grid's own cell-centre coordinates (xnodes / ynodes at Center, host vectors) to the context: needed once before azimuthal_mean / polar_winds!."
function set_horizontal_nodes!(ctx, xc::Vector{Float64}, yc::Vector{Float64})
    check(ccall((:bz_set_horizontal_nodes, libbreeze_hip), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}), ctx, xc, yc),
          "bz_set_horizontal_nodes", ctx)
end

"""
azimuthal_mean!(profile, counts, ctx, field, z_face; radius, center = (0, 0), m = 4): the reference's azimuthal_mean of one centre or z-face
parent array into `profile` (Nr × nlev host matrix, ring index fastest, as `interior(c̄, :, 1, :)`) and the samples per ring into `counts`.
Call `set_horizontal_nodes!(ctx, xnodes, ynodes)` once on the context first: without the grid's own cell-centre coordinates the library
returns BZ_ERR_INVALID.
"""
function azimuthal_mean!(profile::Matrix{Float64}, counts::Vector{Int64}, ctx, field::Ptr{Cvoid}, z_face::Bool; radius, center = (0, 0), m = 4)
    Nr = size(profile, 1)
    length(counts) == Nr || throw(ArgumentError("counts must have one entry per ring"))
    check(ccall((:bz_azimuthal_mean, libbreeze_hip), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cdouble, Cdouble, Cdouble, Int32, Int32, Ptr{Cdouble}, Ptr{Int64}),
                ctx, field, z_face, center[1], center[2], radius, Nr, m, profile, counts), "bz_azimuthal_mean", ctx)
    return profile
end

"azimuthal_mean(ctx, field, z_face, nlev; radius, Nr, center = (0, 0), m = 4) -> (profile (Nr × nlev), counts); needs set_horizontal_nodes! first"
function azimuthal_mean(ctx, field::Ptr{Cvoid}, z_face::Bool, nlev::Integer; radius, Nr, center = (0, 0), m = 4)
    profile, counts = Matrix{Float64}(undef, Nr, nlev), Vector{Int64}(undef, Nr)
    azimuthal_mean!(profile, counts, ctx, field, z_face; radius, center, m)
    return profile, counts
end

"""
Tangential and radial wind about `center` at cell centres from the velocity parent arrays (filled halos); either output may be C_NULL.
Needs `set_horizontal_nodes!(ctx, xnodes, ynodes)` once on the context first (else BZ_ERR_INVALID); NaN where a cell centre is the centre.
"""
function polar_winds!(tangential::Ptr{Cvoid}, radial::Ptr{Cvoid}, ctx, u::Ptr{Cvoid}, v::Ptr{Cvoid}; center = (0, 0))
    check(ccall((:bz_polar_winds, libbreeze_hip), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cdouble, Cdouble, Ptr{Cvoid}, Ptr{Cvoid}),
                ctx, u, v, center[1], center[2], tangential, radial), "bz_polar_winds", ctx)
end

# hipGraph replay of whole steps (csrc/bz_graph.hip): opt-in, pays with a fixed Δt on launch-bound grids; Oceananigans fields keep
# their device arrays for the life of the model, which is what a recorded step relies on
graph_replay!(ctx, on::Bool = true) = check(ccall((:bz_graph_enable, libbreeze_hip), Cint, (Ptr{Cvoid}, Cint), ctx, on), "bz_graph_enable", ctx)

end # module
