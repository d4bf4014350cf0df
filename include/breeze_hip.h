/*
 * breeze_hip.h — C ABI of libbreeze_hip.so: the MI355X-native (gfx950) replacement for the
 * inner time-stepping hot path of Breeze.jl's anelastic AtmosphereModel.
 *
 * The reference has no FFI for this path: every operator is a Julia method chosen by multiple
 * dispatch and executed as KernelAbstractions kernels.  Each entry point below replaces one of
 * the Julia generic functions a package extension would specialise on a marker architecture
 * (precedent: /root/reference/ext/BreezeReactantExt/Timesteppers.jl:6-19) and forward with
 * `ccall((:bz_..., libbreeze_hip), ...)`; see INTEGRATION.md for the Julia stub.
 *
 * Conventions
 *  - Plain C types only.  All field pointers are DEVICE pointers to the *parent*
 *    (halo-inclusive) array of an Oceananigans Field, column-major, i fastest:
 *        element (i,j,k) [1-based interior] at p[(i-1+Hx) + Sx*((j-1+Hy) + Sy*(k-1+Hz))]
 *        Sx = Nx+2Hx, Sy = Ny+2Hy;  z-Face fields on Bounded z have Nz+1 levels.
 *    Column (reference-state) and grid arrays passed to bz_create are HOST pointers; they are
 *    copied at creation.
 *  - Every call returns 0 on success, a BZ_ERR_* code or a negated hipError_t / hipfftResult
 *    otherwise; nothing throws; bz_last_error() returns a message for the calling thread's ctx.
 *  - Calls are asynchronous and stream-ordered on the stream set by bz_set_stream (default: the
 *    HIP null stream).  bz_sync() blocks until the stream is idle.  No internal host threads.
 *  - The caller owns all field memory; the ctx owns FFT plans, column tables and scratch.
 *  - One ctx per device/stream.  Float64 only (ftype = 8) in this version.
 */
#ifndef BREEZE_HIP_H
#define BREEZE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BZ_PERIODIC 0
#define BZ_BOUNDED 1
#define BZ_FLAT 2

#define BZ_OK 0
#define BZ_ERR_INVALID 1      /* null pointer / inconsistent sizes */
#define BZ_ERR_UNSUPPORTED 2  /* topology, float type, halo or scheme not implemented */
#define BZ_ERR_ALLOC 3

/* Oceananigans RectilinearGrid (regular x, y; regular or stretched z). */
typedef struct bz_grid {
    int32_t Nx, Ny, Nz;
    int32_t Hx, Hy, Hz;   /* halo sizes (>= 3 for WENO order 5) */
    int32_t topo[3];      /* BZ_PERIODIC / BZ_BOUNDED / BZ_FLAT per direction */
    int32_t ftype;        /* sizeof(eltype(grid)): 8 */
    double dx, dy;        /* regular horizontal spacings */
    const double *zf;     /* HOST: Nz+1 z-face heights */
    int32_t regular_z;    /* 1: use dz = (zf[Nz]-zf[0])/Nz exactly, as Oceananigans regular grids do */
    int32_t reserved;
} bz_grid;

/* Breeze ThermodynamicConstants subset used on the dry/vapour path
 * (src/Thermodynamics/thermodynamics_constants.jl:182-217). */
typedef struct bz_constants {
    double gravitational_acceleration;
    double dry_air_gas_constant;      /* R / Md */
    double vapor_gas_constant;        /* R / Mv */
    double dry_air_heat_capacity;
    double vapor_heat_capacity;
} bz_constants;

/* Breeze ReferenceState columns (src/Thermodynamics/reference_states.jl:18-28, 402-445):
 * HOST arrays of length Nz+2Hz holding parent(field)[1,1,:] including filled halos. */
typedef struct bz_reference_state {
    double surface_pressure, potential_temperature, standard_pressure;
    const double *density;
    const double *pressure;
    const double *temperature;
} bz_reference_state;

/* model.momentum, formulation/moisture prognostics, velocities, diagnostics, pressure_anomaly
 * (src/AtmosphereModels/atmosphere_model.jl:37-61; src/AnelasticEquations/anelastic_dynamics.jl:5-8). */
typedef struct bz_state {
    double *rho_u, *rho_v, *rho_w;   /* model.momentum            (XFace, YFace, ZFace) */
    double *rho_theta;               /* formulation.potential_temperature_density        */
    double *rho_q;                   /* model.moisture_density                           */
    double *u, *v, *w;               /* model.velocities                                 */
    double *theta;                   /* formulation.potential_temperature                */
    double *q;                       /* specific_prognostic_moisture (qv)                */
    double *T;                       /* model.temperature                                */
    double *phi;                     /* dynamics.pressure_anomaly  (p'/rho_r)            */
} bz_state;

/* A NamedTuple of prognostic-shaped fields: timestepper.Gn or timestepper.U0
 * (src/TimeSteppers/ssp_runge_kutta_3.jl:53-60, 87-88). */
typedef struct bz_prognostic {
    double *rho_u, *rho_v, *rho_w, *rho_theta, *rho_q;
} bz_prognostic;

typedef struct bz_ctx bz_ctx;

/* dynamics_pressure_solver + materialize_advection: builds FFT plans, tridiagonal factors and
 * column tables.  weno_order: 5 (the tuned kernels), or 7 / 9 (WENO(order = 7 | 9), the examples' scheme: generic kernels, halos >=
 * (order + 1) / 2, anelastic or compressible model without bounds-preserving advection, operator-by-operator anelastic stepping; Centered(order = 2)
 * is weno_order = 2 of libbreeze_hip_centered2.so); topology (Periodic, Periodic, Bounded) or — single-GPU contexts —
 * (Periodic, Flat, Bounded) with Ny = 1, Hy = 0 (the reference's 2-D x-z cases, anelastic and compressible), (Bounded, Flat, Bounded) — the same
 * with walls in x (examples/cloudy_thermal_bubble.jl:20-24; anelastic, even Nx <= 4096, u / rho u with wall faces i = 0 and Nx, cosine transform
 * along x) — or (Periodic, Bounded, Bounded) —
 * walls in y, the reference benchmark driver's PBB option (benchmarking/run_benchmarks.jl:130): anelastic WENO(order = 5 | 7 | 9) contexts (no bounds-preserving
 * advection) stepped operator by operator, rho v / v with impenetrable wall faces j = 0 and Ny (face Ny in the first upper halo row), cosine transform along
 * y in the pressure solve (Nx a power of two in [16, 1024] or 3 * 2^m, Ny a multiple of 8 up to 4096); halos >= 3, Float64; every extent at least its
 * halo (Oceananigans' own N >= H rule — the reference's 4 x 4 x 4 smoke-test boxes work, odd extents too); anything else returns
 * BZ_ERR_UNSUPPORTED.  Grids with Nx < 2 Hx or Ny < 2 Hy run the per-operator kernels instead of the fused tiers.
 * Replaces: AtmosphereModels.dynamics_pressure_solver (src/AnelasticEquations/anelastic_pressure_solver.jl:11-24)
 *           and compute_main_diagonal!/compute_lower_diagonal! (:32-78). */
int bz_create(bz_ctx **ctx, const bz_grid *grid, const bz_constants *constants,
              const bz_reference_state *reference_state, int weno_order);
void bz_destroy(bz_ctx *ctx);
/* Thermodynamic formulation of the anelastic model (AtmosphereModel(...; formulation)): 0 = :LiquidIcePotentialTemperature
 * (default), 1 = :StaticEnergy (src/StaticEnergyFormulations/static_energy_formulation.jl:18-21,70-95,
 * static_energy_tendency.jl:39-72).  With 1 the `rho_theta` / `theta` slots of bz_state and bz_prognostic carry
 * energy_density (rho e) / specific_energy (e): T = (e - g z)/c_pm and G_rho_e = -div_rhoUc(e) - Iz(w * Iz(buoyancy)). */
int bz_set_formulation(bz_ctx *ctx, int formulation);
/* microphysics = SaturationAdjustment(equilibrium = WarmPhaseEquilibrium(), solver = SecantSolver(abstol, maxiter))
 * (src/Microphysics/saturation_adjustment.jl:20-60,82-86,168-235): the moisture prognostic is the equilibrium moisture
 * rho q^e (bz_state.rho_q / q), T comes from the secant iteration on the adjusted state, and q^v, q^l are diagnosed into
 * model.microphysical_fields.q^v / q^l (device parent arrays given here), which the buoyancy then reads
 * (grid_moisture_fractions, :127-131).  Constants: liquid CondensedPhase, energy reference temperature and triple point of
 * ThermodynamicConstants (src/Thermodynamics/thermodynamics_constants.jl:92,182-194).  params == NULL: microphysics = nothing.
 * On a CompressibleDynamics context (bz_create_compressible) the same call attaches the density-based adjustment
 * (adjust_thermodynamic_state(::LiquidIceDensityState, ::SaturationAdjustment), src/Microphysics/saturation_adjustment.jl:236-301):
 * saturation at the cell's own total density, one Newton temperature for dynamics and microphysics. */
typedef struct bz_saturation_adjustment {
    double liquid_latent_heat, liquid_heat_capacity;
    double energy_reference_temperature, triple_point_temperature, triple_point_pressure;
    double abstol;            /* SecantSolver abstol (default 1e-4), reltol = 0 */
    int32_t maxiter;          /* default 20 */
    int32_t reserved;
} bz_saturation_adjustment;
int bz_set_saturation_adjustment(bz_ctx *ctx, const bz_saturation_adjustment *params, double *q_vapor, double *q_liquid);
/* equilibrium = MixedPhaseEquilibrium(freezing_temperature, homogeneous_ice_nucleation_temperature) of the SaturationAdjustment attached
 * by bz_set_saturation_adjustment (src/Thermodynamics/vapor_saturation.jl:146-176, src/Microphysics/saturation_adjustment.jl:92-100,
 * 128-149,193-231), called AFTER it: the condensate q^c = max(0, q^t - q^v+) is split q^l = lambda q^c, q^i = (1 - lambda) q^c with
 * lambda(T) = (clamp(T, T^h, T^f) - T^h) / (T^f - T^h), the saturation surface is the PlanarMixedPhaseSurface(lambda) of the temperature it is
 * evaluated at, T carries both latent heats, q^i is diagnosed into model.microphysical_fields.q^i (device parent array given here) and the
 * buoyancy reads q^l + q^i as condensate.  Constants: the ice CondensedPhase of ThermodynamicConstants.  params == NULL returns the context
 * to the warm phase; bz_set_saturation_adjustment (NULL or a new attachment) and bz_set_kessler_microphysics clear the ice state too.
 * Anelastic single-device contexts only: BZ_ERR_UNSUPPORTED, bz_last_error naming the reason, on CompressibleDynamics, y-slab and
 * kinematic contexts and on a context without an attached SaturationAdjustment.  Every call invalidates recorded steps. */
typedef struct bz_mixed_phase_equilibrium {
    double freezing_temperature, homogeneous_ice_nucleation_temperature;
    double ice_latent_heat, ice_heat_capacity;
} bz_mixed_phase_equilibrium;
int bz_set_mixed_phase_equilibrium(bz_ctx *ctx, const bz_mixed_phase_equilibrium *params, double *q_ice);
/* The same equilibrium on a CompressibleDynamics context, called AFTER bz_set_saturation_adjustment: the density-based adjustment
 * (src/Microphysics/saturation_adjustment.jl:241-293) saturates at the cell's own total density over the surface equilibrated at the
 * temperature of each evaluation, q^v+ = p^v+ / (rho R^v T), splits the condensate by lambda(T), and the residual, the Newton temperature
 * (src/Thermodynamics/dynamic_states.jl:197-232), the pressure p = rho R_m T and the acoustic linearisation
 * (src/CompressibleEquations/acoustic_substepping.jl:390-410) carry both latent heats and c_i q^i.  q^i is diagnosed into `q_ice` (device
 * parent array) by update_state! and by the fused stage epilogue.  params == NULL returns the context to the warm phase: its steps are then
 * those of a context that never had the equilibrium attached.  Single-device compressible contexts that are periodic in x and y:
 * BZ_ERR_UNSUPPORTED, bz_last_error naming the function and the reason, on anelastic, kinematic, y-slab and walled contexts, with
 * DCMIP2016KesslerMicrophysics or InstantaneousPrecipitation attached, with bulk surface fluxes attached (they form c_pm without q^i; in the
 * other order bz_set_compressible_surface_fluxes refuses) and without an attached SaturationAdjustment.  Every call invalidates recorded steps. */
int bz_set_compressible_mixed_phase_equilibrium(bz_ctx *ctx, const bz_mixed_phase_equilibrium *params, double *q_ice);
/* ThermodynamicConstants(saturation_vapor_pressure = FlatauPolynomial(...)) (src/Thermodynamics/flatau_polynomial.jl): the eighth-order
 * polynomial fits of Flatau et al. (1992), p^v+ = sum_n a_n x^n, n = 0..8, x = max(T - reference_temperature, -minimum_temperature_offset),
 * over liquid and over ice, coefficients in Pa, a_0 first; on the mixed-phase surface lambda p^v+l + (1 - lambda) p^v+i.  While attached,
 * every saturation adjustment of the context evaluates it in the place of the Clausius-Clapeyron expression: the anelastic adjustment (warm
 * and mixed phase), the density-based adjustment of CompressibleDynamics and the one InstantaneousPrecipitation wraps.  The call may come
 * before or after bz_set_saturation_adjustment / bz_set_mixed_phase_equilibrium / bz_set_instantaneous_precipitation and outlives them.
 * params == NULL returns the context to Clausius-Clapeyron.  BZ_ERR_UNSUPPORTED, bz_last_error naming the function and the reason: y-slab and
 * kinematic contexts, and a context with a surface layer or a bulk vapour flux attached (their surface q^v+ is Clausius-Clapeyron; in the
 * other order bz_set_surface_layer, and bz_set_bulk_surface_fluxes / bz_set_compressible_surface_fluxes with a vapour flux, refuse).  The
 * Kessler scheme and the diagnostics keep their own expressions.  Every call invalidates recorded steps. */
typedef struct bz_flatau_polynomial {
    double liquid_coefficients[9], ice_coefficients[9];
    double reference_temperature, minimum_temperature_offset;
} bz_flatau_polynomial;
int bz_set_saturation_vapor_pressure_polynomial(bz_ctx *ctx, const bz_flatau_polynomial *params);
/* negative_moisture_correction of BulkMicrophysics (src/Microphysics/bulk_microphysics.jl:26-40; src/AtmosphereModels/
 * negative_moisture_correction.jl:199-347): fix_negative_moisture!(model), the first call of update_state!
 * (update_atmosphere_model_state.jl:42), on the moisture prognostic rho_q and a species chain.  Per column, k = 1 the bottom, rho the
 * reference density column:
 *   species_borrowing: at every level, along mass[0] (heaviest) .. mass[n_mass - 1] -> rho_q, each neighbouring pair (h, l):
 *     sink = q_h < 0 ? min(-q_h, max(0, q_l)) : 0 with q = rho q / rho;  rho q_h += rho sink, rho q_l -= rho sink.  Then number[p] = 0 where
 *     pair_mass[p] <= 0 (after the borrowing), then clamp[c] = max(0, clamp[c]).  The lists are used under species_borrowing only.
 *   vertical_borrowing (rho_q only): for k = Nz .. 2: deficit = rho_q[k] / rho[k] < 0 ? -rho_q[k] dz[k] : 0, rho_q[k] += deficit / dz[k],
 *     rho_q[k - 1] -= deficit / dz[k - 1]; then the bottom borrows from level 2: dq = (q[1] < 0 & q[2] > 0) ? min(-rho_q[1] dz[1],
 *     rho_q[2] dz[2]) : 0, rho_q[1] += dq / dz[1], rho_q[2] -= dq / dz[2].
 * The operations are IEEE +, -, *, / in this order, uncontracted; a NaN passes through.  Interior cells only: the halo fill of
 * bz_update_state or the projection + diagnosis kernel of a whole step writes the images afterwards.
 * Every array is a DEVICE centre parent array of the grid; SpeciesBorrowing() of the non-precipitating scheme has empty lists.
 * While attached, the correction runs once per update_state! of the reference: at the head of bz_update_state and, in the whole-step
 * tiers, before the projection + diagnosis of every stage (profile slot "fix_negative_moisture"); nothing is launched when the scheme has
 * nothing to do (no vertical borrowing and empty lists).  The tier a step takes does not depend on it.  c == NULL detaches.
 * BZ_ERR_UNSUPPORTED, bz_last_error naming the function and the reason: CompressibleDynamics, kinematic and y-slab contexts and contexts
 * without an attached SaturationAdjustment (bz_set_saturation_adjustment first; detaching it detaches the correction).  BZ_ERR_INVALID:
 * a count outside 0 .. 4, a null array, an array given twice in a list or in two lists that may not share it (number fields may also be
 * clamped, pair_mass may name a member of mass), a non-empty list with neither phase selected.  An array equal to the rho_q it is run on
 * is refused by the run (BZ_ERR_INVALID).  Every call invalidates recorded steps. */
typedef struct bz_negative_moisture_correction {
    int32_t species_borrowing, vertical_borrowing;
    int32_t n_mass, n_pairs, n_clamp, reserved;
    double *mass[4];
    double *number[4], *pair_mass[4];
    double *clamp[4];
} bz_negative_moisture_correction;
int bz_set_negative_moisture_correction(bz_ctx *ctx, const bz_negative_moisture_correction *c);
/* The attached correction once on s->rho_q (only that member of s is read): the per-operator entry point.  BZ_ERR_INVALID with a message
 * when nothing is attached. */
int bz_fix_negative_moisture(bz_ctx *ctx, const bz_state *s);
int bz_set_stream(bz_ctx *ctx, void *hip_stream);
int bz_sync(bz_ctx *ctx);
const char *bz_last_error(const bz_ctx *ctx);

/* fill_halo_regions! for one field (Oceananigans.BoundaryConditions; call sites
 * src/AtmosphereModels/update_atmosphere_model_state.jl:48,135-136,152,241-243).
 * kind: 0 = centre-in-z field, default (no-flux) z BCs;  1 = z-face field, impenetrable walls;
 *       2 = `nothing` z BCs (diagnostic velocities): periodic wrap only; 3 = as 2 for a z-face field.
 *       + 4 for a field on y faces (rho v, v): on a Bounded y its wall faces j = 0, Ny are set to 0, where a centre-in-y field takes
 *       its first halo row from the adjacent interior row (ignored on a Periodic y); + 8 likewise for a field on x faces (rho u, u). */
int bz_fill_halo_regions(bz_ctx *ctx, double *field, int kind);

/* AtmosphereModels.compute_velocities! (update_atmosphere_model_state.jl:122-155, kernel :248-254). */
int bz_compute_velocities(bz_ctx *ctx, const bz_state *s);
/* compute_auxiliary_thermodynamic_variables! (:225-246, kernel :256-292). */
int bz_compute_auxiliary_thermodynamic_variables(bz_ctx *ctx, const bz_state *s);
/* AtmosphereModels.compute_tendencies! (:294-387): G.rho_u, rho_v, rho_w, rho_theta, rho_q. */
int bz_compute_tendencies(bz_ctx *ctx, const bz_state *s, const bz_prognostic *G);
/* scalar_tendency of ONE field: Gc = -div_rhoUc(c) from the velocities u, v, w (all halo-filled) — compute_scalar_tendency!
 * (update_atmosphere_model_state.jl:390-393, dynamics_kernel_functions.jl:132-159 without forcing), the kernel group the reference's
 * own micro-benchmark times (benchmarking/src/scalar_tendency.jl:16-25: Gc = -div_Uc; here with the reference density of the
 * anelastic model, rho_r = const on that benchmark's 1 m deep box).  WENO order of the context (5, 7 or 9). */
int bz_compute_scalar_tendency(bz_ctx *ctx, const double *u, const double *v, const double *w, const double *c, double *Gc);
/* AtmosphereModel(grid; momentum_advection, scalar_advection) with schemes of different orders (atmosphere_model.jl:80-82,126-127,148-158;
 * examples/tropical_cyclone_world.jl:167-169 and examples/prescribed_sea_surface_temperature.jl:72-73: momentum WENO(order = 9), every
 * scalar WENO(order = 5)): bz_create's weno_order is the momentum scheme, this sets the order (5, 7 or 9) of every scalar — rho theta /
 * rho e, moisture, microphysical species, tracers.  Halos must cover both schemes.  Orders that differ run operator by operator (one
 * kernel per field, the reference's own launch list) on anelastic contexts (y-slabs: the operator-by-operator distributed step);
 * bounds-preserving advection stays a WENO(order = 5)
 * scalar scheme.  Call before the first step. */
int bz_set_scalar_advection_order(bz_ctx *ctx, int order);
/* TimeSteppers.update_state!(model; compute_tendencies) (:41-68); G may be NULL iff compute_tendencies == 0. */
int bz_update_state(bz_ctx *ctx, const bz_state *s, const bz_prognostic *G, int compute_tendencies);

/* store_initial_state! (src/TimeSteppers/ssp_runge_kutta_3.jl:180-186). */
int bz_store_initial_state(bz_ctx *ctx, const bz_state *s, const bz_prognostic *U0);
/* ssp_rk3_substep! (:114-173): u = (1-alpha) u0 + alpha (u + dt G) for the five prognostic fields. */
int bz_ssp_rk3_substep(bz_ctx *ctx, const bz_state *s, const bz_prognostic *U0,
                       const bz_prognostic *G, double dt, double alpha);

/* AtmosphereModels.compute_pressure_correction!(model, dt)
 * (src/AnelasticEquations/anelastic_time_stepping.jl:26-39 -> anelastic_pressure_solver.jl:84-105):
 * momentum halos, source term, Fourier-tridiagonal solve into s->phi, phi halos. */
int bz_compute_pressure_correction(bz_ctx *ctx, const bz_state *s, double dt);
/* AtmosphereModels.make_pressure_correction!(model, dt) (anelastic_time_stepping.jl:45-78). */
int bz_make_pressure_correction(bz_ctx *ctx, const bz_state *s, double dt);

/* OceananigansTimeSteppers.time_step!(model::AtmosphereModel{..SSPRungeKutta3}, dt)
 * (src/TimeSteppers/ssp_runge_kutta_3.jl:209-278) for dry anelastic dynamics without callbacks:
 * the whole step stays on the device (preferred seam).  The state must be consistent
 * (bz_update_state with compute_tendencies=1 called once after set!, as
 * maybe_prepare_first_time_step! does).
 * NOTE: this seam folds each ssp_rk3_substep! into the preceding tendency evaluation, so on return the G arrays hold
 * the last stage's predictor momentum instead of tendencies (they are scratch of the time stepper in the reference as
 * well); bz_compute_tendencies / bz_update_state rebuild them, and bz_ssp_rk3_substep does so automatically.
 * U0 CONTRACT: the U0 arrays are the time stepper's scratch and their contents are UNDEFINED after a step.  The reference fills them
 * with the step-start state (store_initial_state!) and nothing outside time_step! reads them; the lean tier never copies the state into
 * them (the state arrays stay intact as U0 until the last writer of the step) and parks stage-1/2 momentum and stage-2 scalars there,
 * the compressible step stores interior cells only.  No entry point of this library reads U0 (or its halos) across calls. */
int bz_time_step_anelastic(bz_ctx *ctx, const bz_state *s, const bz_prognostic *U0,
                           const bz_prognostic *G, double dt);

/* n calls of time_step!(model, dt) with nothing reading the model in between: the loop of the reference's benchmark driver,
 * many_time_steps! (benchmarking/src/timestepping.jl:11-16), and of run!(simulation) between two callback / output iterations
 * (an IterationInterval- / TimeInterval-aware host calls it with n = the distance to the next actuation).
 * On the lean whole-step tier (dry / vapour-only theta-formulation models, WENO order 5) the tendency kernels derive u, v, w, theta,
 * q^v, T from the prognostic fields, so every step but the last ends with the momentum-only projection and skips the projection +
 * diagnosis pass whose 13 output words per cell only host consumers read; the other tiers diagnose every step.
 *   diagnose_last != 0: on return every field and halo of `s` holds the bits n calls of bz_time_step_anelastic leave.
 *   diagnose_last == 0: the prognostic state is current but the diagnostics (and pressure_anomaly) are stale and rho_theta / rho_q may be
 *     parked in G->rho_theta / G->rho_q (the kernels' ping-pong partner).  Stepping may simply continue (either entry point);
 *     before anything else reads `s`, call bz_update_state(ctx, s, G, 0).  bz_diagnostics_stale(ctx) reports the flag.
 *     Entry points of this library that read the diagnostics and are handed the state rebuild them first (bz_compute_tendencies,
 *     bz_compute_closure_fields, bz_compute_forcings, bz_compute_flux_bc_tendencies, bz_kessler_model_update); bz_cell_advection_timescale,
 *     which takes bare velocity pointers, returns BZ_ERR_INVALID while the flag is set; bz_sync joins a pending halo exchange of a slab context. */
int bz_time_steps_anelastic(bz_ctx *ctx, const bz_state *s, const bz_prognostic *U0,
                            const bz_prognostic *G, double dt, int n, int diagnose_last);
int bz_diagnostics_stale(const bz_ctx *ctx);

/* ---- Kinematic driver: AtmosphereModel(grid; dynamics = PrescribedDynamics(reference_state; divergence_correction)) ----------------
 * (src/KinematicDriver/prescribed_dynamics.jl:27-84, kinematic_driver_time_stepping.jl:16-73).  The velocities s->u, s->v, s->w are GIVEN:
 * ordinary halo-filled fields the host writes (periodic images in x, y; w as stored on the wall faces k = 0 and k = Nz — the host keeps
 * zeros there for impenetrable walls), never written by the library.  Density and pressure are the reference state's; there is no
 * momentum (s->rho_u, rho_v, rho_w, phi and their U0 / G slots may be NULL) and no pressure solve.  Every scalar c of {theta, moisture,
 * tracers} advances with
 *     G = -div_rhoUc(c) [+ c div_rhoU],   div_rhoU = 1/V [dx(Ax Ix(rho) u) + dy(Ay Iy(rho) v) + dz(Az Iz(rho) w)]
 * (dynamics_kernel_functions.jl:155-156; the second term with divergence_correction != 0: a uniform c then stays uniform in a divergent
 * flow), all scalars of a Runge-Kutta stage in one launch.
 * bz_set_prescribed_dynamics marks an anelastic single-device context ((Periodic, Periodic | Flat, Bounded)) kinematic; compressible,
 * y-slab and walled contexts return BZ_ERR_UNSUPPORTED.  EVERY call also declares that the velocity fields may have changed (the
 * host's set path calls it again): the library re-forms div_rhoU before its next use.
 * On a kinematic context bz_update_state skips the velocity computation (update_state! with compute_velocities! = nothing) and, with
 * compute_tendencies != 0, ends with bz_compute_kinematic_tendencies; the momentum / projection entry points (bz_time_step(s)_anelastic,
 * bz_compute_tendencies, bz_compute_velocities, bz_ssp_rk3_substep, bz_store_initial_state, bz_compute_pressure_correction,
 * bz_make_pressure_correction, bz_tendencies_fused_rk, bz_ssp_rk3_substep_fused, bz_max_abs_divergence) return BZ_ERR_UNSUPPORTED with
 * bz_last_error set, and so do the two entry points below on a context that is not kinematic.
 * Implemented: WENO(order = 5), the potential-temperature formulation, microphysics nothing or warm-phase saturation adjustment, user
 * tracers; anything else attached to the context (closure, forcings, sponges, bulk fluxes, bounds-preserving advection, Kessler, graph
 * replay) makes the two entry points return BZ_ERR_UNSUPPORTED naming it. */
int bz_set_prescribed_dynamics(bz_ctx *ctx, int divergence_correction);
/* G->rho_theta, G->rho_q and the tracers' G arrays from the stored specific fields (stale diagnostics are rebuilt first). */
int bz_compute_kinematic_tendencies(bz_ctx *ctx, const bz_state *s, const bz_prognostic *G);
/* n x time_step!(model, dt): per stage the substep of every rho c (stage 1 also stores U0), then update_state!.  The caller has run
 * bz_update_state once after the last set!.  diagnose_last as in bz_time_steps_anelastic: with 0 the update_state! after the very last
 * stage is skipped, the prognostic scalars are current, theta / q / T / the specific tracers are stale (bz_diagnostics_stale) until
 * bz_update_state(ctx, s, G, 0) — which a following call of this function runs by itself.  The G arrays are not written. */
int bz_time_steps_kinematic(bz_ctx *ctx, const bz_state *s, const bz_prognostic *U0, const bz_prognostic *G, double dt, int n,
                            int diagnose_last);

/* ---- y-slab decomposition: one process per GPU --------------------------------------------------
 * The reference re-exports Oceananigans' Distributed architecture (src/Breeze.jl:172,183,209) and has no
 * distributed code of its own; these entry points are the rank-local kernels of this repo's decomposition.
 * `local_grid` describes this rank's slab: Ny = rows owned (global Ny = Ny * y_nranks), y halos are filled by the
 * caller's neighbour exchange instead of a periodic wrap.  The caller also performs the horizontal transforms of
 * the Poisson solve (x-FFT, all-to-all to kx slabs, y-FFT and back); this rank's spectral block is
 * [Nz][nkx][Ny_global] complex (ky fastest, so the y transform is contiguous) for kx in [kx0, kx0+nkx) of the
 * zero-padded half spectrum. */
int bz_create_slab(bz_ctx **ctx, const bz_grid *local_grid, const bz_constants *constants,
                   const bz_reference_state *reference_state, int weno_order, int y_nranks, int y_rank);
int bz_slab_info(bz_ctx *ctx, int32_t *y_nranks, int32_t *y_rank, int32_t *nkx, int32_t *kx0, int32_t *ny_global);
/* ssp_rk3_substep! with store_initial_state! folded into the first stage (first != 0 requires alpha == 1). */
int bz_ssp_rk3_substep_fused(bz_ctx *ctx, const bz_state *s, const bz_prognostic *U0, const bz_prognostic *G,
                             double dt, double alpha, int first);
/* compute_anelastic_source_term! into rhs (device, contiguous Nx*Ny*Nz); in slab mode row Ny of rho_v must hold
 * the neighbour's first row. */
int bz_poisson_source_term(bz_ctx *ctx, const bz_state *s, double dt, double *rhs);
/* Thomas solve along z of every horizontal wavenumber of this rank's spectral block, in place; `scale` multiplies
 * the right-hand side (inverse-transform normalisation); the (0,0) column gets its z-mean removed. */
int bz_spectral_tridiagonal_solve(bz_ctx *ctx, double *hat, double scale);
/* Transposing pack of the distributed transform (complex Float64, interleaved re/im): in is (Nz, A, ld), out (Nz, B, A),
 * out[k][b][a] = in[k][a][c0 + b], zero where c0 + b >= valid.  One call per destination rank builds its send block. */
int bz_pack_transpose(bz_ctx *ctx, const double *in, double *out, int32_t Nz, int32_t A, int32_t ld, int32_t c0, int32_t B,
                      int32_t valid);
/* The local transforms of the distributed Poisson solve (1-D batched rocFFT plans, unnormalised): which = 0 x forward
 * (real (Nz, Ny, Nx) -> complex (Nz, Ny, Nx/2+1)), 1 / 2 y forward / backward in place on this rank's (Nz, nkx, Ny_global) block,
 * 3 x backward (complex (Nz, Ny, ld), ld >= Nx/2+1 -> real (Nz, Ny, Nx); overwrites its input).  ld is read for which = 3 only. */
int bz_slab_transform(bz_ctx *ctx, int32_t which, double *in, double *out, int32_t ld);
/* y-halo exchange helper of the slab drivers: gathers (unpack = 0) or scatters (unpack != 0) parent rows [row0, row0 + nrows) of n
 * parent arrays (levels[m] z-levels each: Nz + 2 Hz for centre fields, Nz + 1 + 2 Hz for z-face fields; full x width) into / out of
 * one contiguous device buffer, field-major then (level, row, x).  n <= 24. */
int bz_pack_rows(bz_ctx *ctx, double *const *fields, const int32_t *levels, int32_t n, int32_t row0, int32_t nrows, double *buffer,
                 int32_t unpack);
/* make_pressure_correction! + compute_velocities! + thermodynamic diagnosis + x/z halo fills in one pass from the
 * contiguous solution phi_c (Nx*Ny*Nz); phi_below = phi of row j = -1, layout [k][i] (slab mode; else NULL). */
int bz_project_and_diagnose(bz_ctx *ctx, const bz_state *s, const double *phi_c, const double *phi_below, double dt);

/* compute_tendencies! with the next ssp_rk3_substep! folded into the kernels' store: predictor momentum goes to
 * G->rho_u/v/w (to be projected by bz_project_and_diagnose_from), rho_theta / rho_q advance in place, U0 is filled when
 * first != 0 (alpha must then be 1).  The *_from variants take the momentum predictor from `predictor` instead of s. */
int bz_tendencies_fused_rk(bz_ctx *ctx, const bz_state *s, const bz_prognostic *U0, const bz_prognostic *G,
                           double dt, double alpha, int first);
int bz_poisson_source_term_from(bz_ctx *ctx, const bz_state *s, const bz_prognostic *predictor, double dt, double *rhs);
int bz_project_and_diagnose_from(bz_ctx *ctx, const bz_state *s, const bz_prognostic *predictor, const double *phi_c,
                                 const double *phi_below, double dt);

/* ---- communication of the y-slab decomposition inside the library (BASELINE.json north_star: RCCL halo exchange and FFT
 * all-to-all behind the C ABI).  With a communicator attached to a slab context, bz_time_step_anelastic IS the distributed step:
 * the lean whole-step seam with, per stage, one row of predictor rho_v from the upper neighbour, the Poisson solve as local x
 * transform -> all-to-all of transposed blocks -> y transform + Thomas solve -> all-to-all back -> x transform, one row of phi
 * from the lower neighbour, and the Hy-row halo exchange of (rho_u, rho_v, rho_w, rho_theta, rho_q) on a side stream while the
 * next stage's interior tile rows compute.  Every exchange is a group of point-to-point messages (one per xGMI link).
 *   bz_comm_unique_id      rank 0: a 128-byte id (ncclGetUniqueId) that the host hands to every rank (MPI.Bcast, a file, ...)
 *   bz_comm_init_rccl      every rank, on its own device: ncclCommInitRank(y_nranks, id, y_rank); librccl is dlopen'ed
 *   bz_comm_init_local     the ranks are contexts of this process (one host thread each): peer copies ordered by events — the
 *                          transport the distributed step is tested with on a single GPU, and a single-process multi-GPU option
 *   bz_comm_exchange_y_halos            Hy halo rows of n parent arrays (levels[m] z levels each), both directions
 *   bz_comm_update_state_and_project    set!'s update_state!(compute_tendencies = false) + halo exchange and, if project != 0, the
 *                                       initial projection with dt (set_atmosphere_model.jl:121-128) and the exchange after it
 *   bz_comm_info           transport name, bytes sent by this rank so far, number of exchanges
 * Dry / vapour anelastic model (the configuration of BASELINE configs[1] and [3]); other physics return BZ_ERR_UNSUPPORTED. */
#define BZ_UNIQUE_ID_BYTES 128
int bz_comm_unique_id(void *id_out);
int bz_comm_init_rccl(bz_ctx *ctx, const void *id);
int bz_comm_init_local(bz_ctx *ctx, const char *group_name);
int bz_comm_destroy(bz_ctx *ctx);
int bz_comm_exchange_y_halos(bz_ctx *ctx, double *const *fields, const int32_t *levels, int32_t n);
int bz_comm_update_state_and_project(bz_ctx *ctx, const bz_state *s, const bz_prognostic *G, double dt, int project);
int bz_comm_info(bz_ctx *ctx, const char **transport, int64_t *bytes_sent, int32_t *exchanges);
/* Compressible y-slab contexts (bz_create_compressible_slab) take the same communicators: bz_time_step_compressible then runs
 * the whole distributed WS-RK3 step in the library (per-substep exchange of (rho theta)' and (rho v)', per-stage exchange of
 * G_rho_v, prognostics, diagnostics and time-averaged velocities; the Kessler column update stays rank-local), and
 * bz_comm_compressible_update_state is update_state! with those exchanges (for set! and drivers stepping operator by operator). */
struct bz_compressible_state; struct bz_compressible_prognostic; struct bz_acoustic_substepper;
int bz_comm_compressible_update_state(bz_ctx *ctx, const struct bz_compressible_state *s, const struct bz_compressible_prognostic *G,
                                      const struct bz_acoustic_substepper *sub, int compute_tendencies);

/* ==== CompressibleDynamics + SplitExplicitTimeDiscretization ==================================
 * Fully compressible dynamics advanced by the Wicker-Skamarock RK3 outer loop with the linearised acoustic substep
 * loop (src/TimeSteppers/acoustic_runge_kutta_3.jl, src/CompressibleEquations/acoustic_substepping.jl).
 * Scope: (Periodic, Periodic, Bounded), microphysics = nothing (vapour is a passive mass fraction entering R_m, c_p,m),
 * ProportionalSubsteps, ThermalDivergenceDamping (optionally damp_vertical) or NoDivergenceDamping, no sponge,
 * LiquidIcePotentialTemperature formulation with the NewtonSolver temperature inversion. */

/* model.dynamics.{dry_density,total_density,pressure}, model.momentum, formulation / moisture prognostics and the
 * diagnostics (src/CompressibleEquations/compressible_dynamics.jl:44-55; atmosphere_model.jl:37-61). */
typedef struct bz_compressible_state {
    double *rho_d;                   /* dynamics.dry_density (prognostic)                */
    double *rho;                     /* dynamics.total_density = rho_d + rho q (diagnosed) */
    double *rho_u, *rho_v, *rho_w;   /* model.momentum                                   */
    double *rho_theta;               /* formulation.potential_temperature_density        */
    double *rho_q;                   /* model.moisture_density                           */
    double *u, *v, *w;               /* model.velocities (default boundary conditions)   */
    double *theta, *q, *T;           /* theta = rho_theta/rho_d, q = rho_q/rho, temperature */
    double *p;                       /* dynamics.pressure = rho R_m T                    */
} bz_compressible_state;

/* timestepper.Gn / timestepper.U0 of AcousticRungeKutta3 (acoustic_runge_kutta_3.jl:64-72): prognostic order
 * (rho_d, rho_u, rho_v, rho_w, rho_theta, rho_q). */
typedef struct bz_compressible_prognostic {
    double *rho_d, *rho_u, *rho_v, *rho_w, *rho_theta, *rho_q;
} bz_compressible_prognostic;

/* AcousticSubstepper fields (acoustic_substepping.jl:91-134); all caller-owned parent arrays. */
typedef struct bz_acoustic_substepper {
    double *exner, *potential_temperature, *gamma_R_mixture;     /* linearization_* (centre)                  */
    double *density_perturbation;                                /* rho'                                       */
    double *density_potential_temperature_perturbation;          /* (rho theta)'                               */
    double *momentum_perturbation_u, *momentum_perturbation_v;   /* (rho u)', (rho v)'                         */
    double *momentum_perturbation_w;                             /* (rho w)'  (z-face)                         */
    double *density_predictor, *density_potential_temperature_predictor;
    double *previous_density_potential_temperature_perturbation;
    double *time_averaged_u, *time_averaged_v, *time_averaged_w; /* time_averaged_velocities (w: z-face)       */
    double *slow_vertical_momentum_tendency;                     /* G^s_rho_w (z-face)                         */
    double *vertical_solver_source_term;                         /* tridiagonal right-hand side (z-face)       */
} bz_acoustic_substepper;

/* SplitExplicitTimeDiscretization (src/CompressibleEquations/time_discretizations.jl:535-562). */
typedef struct bz_split_explicit {
    int32_t substeps;                 /* acoustic substeps per dt; 0 = adaptive from acoustic_cfl (nothing)   */
    int32_t damp_vertical;            /* ThermalDivergenceDamping(damp_vertical)                              */
    int32_t apply_first_substep_pressure_gradient;
    int32_t newton_maxiter;           /* NewtonSolver maxiter (default 8)                                     */
    double acoustic_cfl;              /* default 0.5                                                          */
    double forward_weight;            /* omega, default 0.65                                                  */
    double damping_coefficient;       /* ThermalDivergenceDamping alpha (default 0.1); < 0: NoDivergenceDamping */
    double thermodynamic_tendency_factor, vertical_momentum_tendency_factor;   /* default 1                   */
    double newton_abstol;             /* NewtonSolver abstol (default 1e-4), reltol = 0                       */
    int32_t direct_divergence_damping; /* != 0: DirectDivergenceDamping(damping_coefficient) (time_discretizations.jl:269-274,
                                         acoustic_substepping.jl:1146-1188) instead of ThermalDivergenceDamping; horizontal only  */
    int32_t sponge_ramp;              /* UpperSponge (time_discretizations.jl:381-512; acoustic_substepping.jl:584-602,639,948):
                                         0 = sponge = nothing, 1 LinearRamp, 2 CubicRamp (the default ramp), 3 Sin2Ramp                 */
    double sponge_damping_rate;       /* peak rate at the lid, 1/s (default 0.2)                                                       */
    double sponge_depth;              /* layer thickness below z = grid.Lz, m (default 5e3)                                            */
    int32_t substep_distribution;     /* stage substep counts and sizes (acoustic_substepping.jl:468-508): 0 ProportionalSubsteps (default:
                                         ceil(beta N) substeps tiling beta dt), 1 ConstantSubstepSize (N rounded up to a multiple of 6,
                                         round(beta N) substeps of dt / N), 2 MonolithicFirstStage (stage 1: one substep of dt / 3)          */
    int32_t substep_float_bytes;      /* substep_floattype (acoustic_substepping.jl:199-235): storage type of the substepper's working fields
                                         — exner, potential_temperature, gamma_R_mixture, density_perturbation,
                                         density_potential_temperature_perturbation, momentum_perturbation_u / _v, density_predictor,
                                         density_potential_temperature_predictor, previous_density_potential_temperature_perturbation —
                                         0 = eltype(grid); 4 = Float32 (those ten pointers of bz_acoustic_substepper then address float arrays;
                                         (rho w)', the solver's right-hand side and the time-averaged velocities stay eltype(grid)).
                                         Thermal or no divergence damping; single-device contexts and y-slab contexts with a library-owned
                                         communicator (the per-substep halo messages then carry the Float32 rows). */
    double damping_length_scale;      /* ThermalDivergenceDamping(length_scale = l) (time_discretizations.jl:215-218,235-247): <= 0 = nothing,
                                         the local scale kappa = alpha min(dx, dy)^2 / dtau (acoustic_substepping.jl:1100-1110); > 0 the fixed
                                         diffusivity (alpha l^2) / dtau in both horizontal directions (:1085-1092).  The vertical part of
                                         damp_vertical keeps alpha dz^2 / dtau. */
} bz_split_explicit;

/* ExnerReferenceState columns (src/Thermodynamics/reference_states.jl:717-815): HOST arrays of length Nz+2Hz
 * (parent(field)[1,1,:], halos filled); both NULL for reference_state = nothing. */
typedef struct bz_exner_reference_state {
    double standard_pressure;
    const double *pressure;
    const double *density;
} bz_exner_reference_state;

/* materialize_dynamics(::CompressibleDynamics) + AcousticRungeKutta3/AcousticSubstepper construction
 * (compressible_dynamics.jl:205-252; acoustic_runge_kutta_3.jl:82-103; acoustic_substepping.jl:180-270). */
int bz_create_compressible(bz_ctx **ctx, const bz_grid *grid, const bz_constants *constants,
                           const bz_exner_reference_state *reference_state, const bz_split_explicit *time_discretization,
                           int weno_order);

/* update_state!(model; compute_tendencies) for CompressibleDynamics (update_atmosphere_model_state.jl:41-68 with
 * compressible_time_stepping.jl:83-103,191-242): total density, prognostic halos, velocities, theta, q, T (Newton), p,
 * and — when compute_tendencies != 0 — the moisture tendency G->rho_q built with the total density and the substepper's
 * time-averaged transport velocities (acoustic_runge_kutta_3.jl:352-358).  The momentum / rho_theta / rho_d tendencies
 * that the reference also computes here are overwritten by compute_slow_*_tendencies! before use and are not formed.
 * The stepping entry points of a compressible context need Nx >= 2 Hx and Ny >= 2 Hy and return BZ_ERR_UNSUPPORTED otherwise.  This call
 * (and bz_instantaneous_precipitation_update) also runs on narrower grids (Hx <= Nx, Hy <= Ny: the reference's 8 x 8 x 8 test grids under a
 * halo of 5) of a single-device context that is periodic in x and y and carries neither microphysics species nor a closure: the halos
 * are then filled by the generic halo kernels after the diagnosis. */
int bz_compressible_update_state(bz_ctx *ctx, const bz_compressible_state *s, const bz_compressible_prognostic *G,
                                 const bz_acoustic_substepper *sub, int compute_tendencies);

/* refresh_linearization_basic_state! / prepare_acoustic_cache! (acoustic_substepping.jl:318-399,412-413). */
int bz_refresh_linearization(bz_ctx *ctx, const bz_compressible_state *s, const bz_acoustic_substepper *sub);
/* seed_time_averaged_velocities! (acoustic_substepping.jl:303-314). */
int bz_seed_time_averaged_velocities(bz_ctx *ctx, const bz_compressible_state *s, const bz_acoustic_substepper *sub);
/* compute_slow_momentum_tendencies! + compute_slow_scalar_tendencies! (acoustic_substep_helpers.jl:55-93,117-149):
 * G->rho_u, rho_v, rho_w (advection only, SlowTendencyMode), G->rho_d = -div(momentum), G->rho_theta. */
int bz_compute_slow_tendencies(bz_ctx *ctx, const bz_compressible_state *s, const bz_compressible_prognostic *G);
/* acoustic_substepping.jl:451-508 (ProportionalSubsteps): substep count and size of the stage covering beta*dt. */
int bz_stage_substeps(bz_ctx *ctx, double dt, double beta, int32_t *n_substeps, double *dtau);
/* acoustic_rk3_substep_loop!(model, substepper, dt, beta, U0) (acoustic_substepping.jl:1404-1590): slow rho_w assembly,
 * rewind initialisation, the substep loop, time-averaged velocities, recovery of the full state, halos, velocities. */
int bz_acoustic_substep_loop(bz_ctx *ctx, const bz_compressible_state *s, const bz_compressible_prognostic *U0,
                             const bz_compressible_prognostic *G, const bz_acoustic_substepper *sub, double dt, double beta);
/* acoustic_rk3_substep!(model, dt, beta) (acoustic_runge_kutta_3.jl:172-186): linearisation refresh, slow tendencies,
 * substep loop, WS-RK3 update of the moisture density. */
int bz_acoustic_rk3_substep(bz_ctx *ctx, const bz_compressible_state *s, const bz_compressible_prognostic *U0,
                            const bz_compressible_prognostic *G, const bz_acoustic_substepper *sub, double dt, double beta);
/* time_step!(model::CompressibleAcousticModel, dt) (acoustic_runge_kutta_3.jl:264-319) without callbacks; the state
 * must be consistent (bz_seed_time_averaged_velocities + bz_compressible_update_state(compute_tendencies=1) once
 * after set!, as maybe_prepare_first_time_step! does). */
int bz_time_step_compressible(bz_ctx *ctx, const bz_compressible_state *s, const bz_compressible_prognostic *U0,
                              const bz_compressible_prognostic *G, const bz_acoustic_substepper *sub, double dt);

/* ---- discrete hydrostatic balance of the initial and the base state (csrc/bz_balance.hip) ----
 * set!(model; rho = HydrostaticallyBalancedDensity(p0)) and set!(model; compute_reference_state = true) / set_to_mean!(::ExnerReferenceState,
 * model) of the reference (src/AtmosphereModels/set_to_mean.jl:152-229,243-310; src/Thermodynamics/reference_states.jl:572-677,835-838).
 * One device, (Periodic, Periodic | Flat, Bounded): contexts with a Bounded x or y and y-slab contexts return BZ_ERR_UNSUPPORTED from all
 * three, with bz_last_error naming the function.
 *
 * bz_exner_columns — _compute_exner_reference_3d!: one discrete-balance Exner integration per column (i, j) of the DEVICE parent arrays
 * theta and qv (NULL = dry), upward from the surface pressure p0: half a continuous step to level 1, then for k = 2 .. Nz a continuous first
 * guess and exactly five Newton iterations on F(p) = p / dz_f + A p^(1 - kappa) - C with the level's moist constants, so that
 * (p[k] - p[k-1]) / dz_f[k] + g (rho[k] + rho[k-1]) / 2 = 0 holds to rounding at every interior face.  Writes the interior of exner, pressure,
 * density (DEVICE parent arrays of centre fields); reads only interior cells, halos are neither read nor written.  Asynchronous. */
int bz_exner_columns(bz_ctx *ctx, const double *theta, const double *qv, double p0, double *exner, double *pressure, double *density);
/* set_hydrostatically_balanced_density!(model, spec) on the state arrays, after the update_state! that closes set! (s->theta and the halos
 * of s->rho_d are those it left): (1) q^v = rho_q / rho_d_old, (2) the column integration of bz_exner_columns with s->theta and that q^v gives
 * the balanced total density, (3) rho_q and the Kessler species are scaled by rho / rho_d_old, (4) rho_d = rho - (rho_q + species), (5) its
 * halos are filled, (6) rho_u, rho_v, rho_w (ratio of the face means of new and old dry density; the wall faces of rho_w keep their values)
 * and rho_theta are scaled by rho_d_new / rho_d_old, (7) update_state!(compute_tendencies = false).  Specific theta and q are preserved to
 * rounding, velocities up to the face means.  Two parent-shaped scratch arrays are allocated by the first call. */
int bz_set_hydrostatically_balanced_density(bz_ctx *ctx, const bz_compressible_state *s, double p0);
/* Replace the reference columns of a compressible context (what set_to_mean!(::ExnerReferenceState, model) changes for the time step):
 * HOST arrays as in bz_create_compressible — Nz + 2 Hz entries, halo levels included, taken as they are (the host fills them with the
 * boundary conditions the reference's fields were built with: pressure and density by the bottom values of construction, no-flux on top).
 * Every column table bzi_create derives from them is rebuilt by the function that built it: rho_r, 1 / rho_r, p_r, ln(p_r / p_st) at centres,
 * Iz(rho_r) and 1 / Iz(rho_r) at faces; grid metrics and the (unused) reference temperature are untouched.  The stream is drained first and
 * the configuration epoch is bumped: no recorded step (bz_graph_enable) survives.  standard_pressure must be the one of creation.  A context
 * created without a reference (both pointers NULL at creation) returns BZ_ERR_INVALID.  Afterwards the caller redoes what depends on the
 * reference: update_state! (bz_compressible_update_state) and, before per-operator substeps, bz_refresh_linearization. */
int bz_set_exner_reference_state(bz_ctx *ctx, const bz_exner_reference_state *reference_state);

/* ---- y-slab decomposition of the compressible path (halo exchanges only, the column solve is local) ----
 * `local_grid` is this rank's slab as in bz_create_slab.  The caller's neighbour exchange fills the y halos (Hy rows) at the
 * points listed below; x and z halos stay the library's business.  Sequence of one WS-RK3 stage:
 *   [state halos valid: rho_d, rho, momentum, rho_theta, rho_q, u, v, w, theta, q, T, p, time-averaged velocities; the U0 arrays are
 *    whole-array copies of the step-start state, halo rows included (the stage's first sweeps form U0 - U on the halo rows too)]
 *   bz_refresh_linearization            (also linearises one halo row on each side)
 *   bz_compute_slow_tendencies          -> exchange G->rho_v
 *   bz_acoustic_stage_begin             returns N_tau and which buffer pair is current (0: the substepper's own
 *                                       (rho theta)', (rho u)', (rho v)' fields, 1: previous_(rho theta)' / the scratch pair)
 *   for n = 1..N_tau:  exchange current (rho theta)' and (rho v)'  ->  bz_acoustic_substep(n)
 *                      [DirectDivergenceDamping: -> exchange the (rho u)', (rho v)' buffers bz_acoustic_substep made current
 *                       -> bz_acoustic_direct_damping]
 *   exchange current (rho theta)'  ->  bz_acoustic_stage_end
 *   exchange rho_d, momentum, rho_theta, rho_q, time-averaged velocities  ->  bz_compressible_update_state(compute_tendencies = 0)
 *   exchange rho, u, v, w, theta, q, T, p  ->  bz_compute_moisture_tendency */
int bz_create_compressible_slab(bz_ctx **ctx, const bz_grid *local_grid, const bz_constants *constants,
                                const bz_exner_reference_state *reference_state, const bz_split_explicit *time_discretization,
                                int weno_order, int y_nranks, int y_rank);
/* The three pieces of acoustic_rk3_substep_loop! (acoustic_substepping.jl:1404-1590): :1437-1441 | one iteration of
 * :1448-1555 | :1557-1590 without the trailing halo fills / compute_velocities! (done by the next update_state!). */
int bz_acoustic_stage_begin(bz_ctx *ctx, const bz_compressible_state *s, const bz_compressible_prognostic *U0,
                            const bz_compressible_prognostic *G, const bz_acoustic_substepper *sub, double dt, double beta,
                            int32_t *n_substeps, int32_t *current_buffer);
int bz_acoustic_substep(bz_ctx *ctx, const bz_compressible_state *s, const bz_compressible_prognostic *U0,
                        const bz_compressible_prognostic *G, const bz_acoustic_substepper *sub, int32_t substep,
                        int32_t *current_buffer);
int bz_acoustic_stage_end(bz_ctx *ctx, const bz_compressible_state *s, const bz_compressible_prognostic *U0,
                          const bz_compressible_prognostic *G, const bz_acoustic_substepper *sub, double dt, double beta,
                          int update_moisture);
/* apply_divergence_damping!(::DirectDivergenceDamping) (acoustic_substepping.jl:1158-1188) of the substep that just ran, on a y-slab
 * context: the divergence of the theta-weighted momentum perturbations reads (rho v)' of the neighbour's first row and the gradient
 * reads it one row below the slab, so the driver exchanges the current (rho u)', (rho v)' buffers between bz_acoustic_substep and this
 * call.  Single-GPU contexts damp inside bz_acoustic_substep; there, and without DirectDivergenceDamping, this is a no-op. */
int bz_acoustic_direct_damping(bz_ctx *ctx, const bz_compressible_state *s, const bz_compressible_prognostic *U0,
                               const bz_compressible_prognostic *G, const bz_acoustic_substepper *sub);
/* Lateral boundaries of the acoustic substep loop (acoustic_substepping.jl:1300-1395: apply_open_boundary_relaxation!,
 * enforce_wall_impenetrability!), compressible contexts on a grid with a Bounded x and / or y — (Bounded, Periodic, Bounded),
 * (Periodic, Bounded, Bounded), (Bounded, Bounded, Bounded); single device.  Such a context runs bz_refresh_linearization,
 * bz_acoustic_substep_loop and the three-piece stage interface.  With a Bounded x, bz_compressible_update_state,
 * bz_compute_slow_tendencies, bz_compute_moisture_tendency, bz_acoustic_rk3_substep and bz_time_step_compressible return BZ_ERR_UNSUPPORTED
 * (bz_last_error names the function that was called).  (Periodic, Bounded, Bounded) runs them too — whole steps between impenetrable south
 * and north walls, WENO(order = 5), no microphysics: rho v and v carry exact zeros on their wall faces j = 0 and j = Ny (face Ny is the
 * first upper halo row), every field that is a centre in y the no-flux copy in its first halo rows, and the wall row j = 0 of the slow
 * rho v tendency is not written; with an active open side, WENO 7 / 9 or microphysics they return BZ_ERR_UNSUPPORTED naming the option.
 * The substepper's own fields take the zero-gradient halo of their default boundary conditions from the library; the model's fields
 * (rho_d, rho_theta, p, the slow tendencies) are read with the one halo row / column the caller's boundary conditions filled.
 * *_open != 0: that side carries an active open (normal-flow) boundary condition on the wall-normal momentum — the outermost cells of rho',
 * (rho theta)' are relaxed every substep towards (c^L[halo] - c^L[cell]) / 2 with factor open_boundary_relaxation in (0, 1]
 * (SplitExplicitTimeDiscretization(open_boundary_relaxation = 0.5)) and the west / south wall face of the momentum perturbation is advanced
 * by the substep like any other face; 0 (the default of every side): an impenetrable wall, whose face is held at zero.  The east / north
 * wall face (index N + 1 of the reference's face field) is written by no kernel of the reference's loop and is an exact zero here.
 * bz_acoustic_substep_loop ends with _recover_full_state! on such a context: the halo fills with the model's boundary conditions and
 * compute_velocities! (:1584-1587) are the caller's. */
int bz_set_acoustic_lateral_boundaries(bz_ctx *ctx, int west_open, int east_open, int south_open, int north_open,
                                       double open_boundary_relaxation);
/* Caller-owned second buffers of the (rho u)', (rho v)' ping-pong (XFace / YFace parent arrays), so that the slab driver can
 * exchange their halos; NULL, NULL returns to the context's own scratch. */
int bz_set_acoustic_scratch(bz_ctx *ctx, double *momentum_u_second_buffer, double *momentum_v_second_buffer);
/* The moisture part of compute_tendencies! alone (update_atmosphere_model_state.jl:330-343 with the time-averaged
 * transport velocities), for drivers that exchange halos between the diagnosis and the tendency. */
int bz_compute_moisture_tendency(bz_ctx *ctx, const bz_compressible_state *s, const bz_compressible_prognostic *G,
                                 const bz_acoustic_substepper *sub);
/* compute_closure_fields!(model.closure_fields, model.closure, model) of a compressible context alone (bz_set_closure: nu_e and its
 * halos; bz_set_scalar_diffusivity: the halos of a field-valued K; no closure: nothing), from the state the last update_state! left. */
int bz_compressible_compute_closure_fields(bz_ctx *ctx, const bz_compressible_state *s);

/* ---- DCMIP2016 Kessler warm-rain microphysics: the operator-split column kernel ----
 * microphysics_model_update!(::DCMIP2016KesslerMicrophysics, model) (src/Microphysics/dcmip2016_kessler.jl:449-486, kernel
 * :618-858): autoconversion, accretion, saturation adjustment (Tetens), rain evaporation and sedimentation with per-column
 * subcycling, in place on theta / rho_theta / rho_qv / rho_qcl / rho_qr; q^v, q^cl, q^r, W^r are diagnosed (they double
 * as the column workspace, as in the reference); the caller follows with update_state!.  density / pressure: 3-D parents
 * (CompressibleDynamics) or NULL for the context's reference columns (AnelasticDynamics).  precipitation_rate: the
 * horizontal parent (Sx x Sy) of mu.precipitation_rate. */
typedef struct bz_kessler_microphysics {      /* DCMIP2016KesslerMicrophysics (:40-70,154-169) */
    double dcmip_temperature_scale;
    double terminal_velocity_coefficient, density_scale, terminal_velocity_exponent;
    double autoconversion_rate, autoconversion_threshold;
    double accretion_rate, accretion_exponent;
    double evaporation_ventilation_coefficient_1, evaporation_ventilation_coefficient_2;
    double evaporation_ventilation_exponent_1, evaporation_ventilation_exponent_2;
    double diffusivity_coefficient, thermal_conductivity_coefficient;
    double substep_cfl;
    /* TetensFormula (src/Thermodynamics/tetens_formula.jl:72-85) and the liquid CondensedPhase of the constants */
    double tetens_reference_saturation_vapor_pressure, tetens_reference_temperature;
    double tetens_liquid_coefficient, tetens_liquid_temperature_offset;
    double liquid_latent_heat, liquid_heat_capacity;
} bz_kessler_microphysics;
typedef struct bz_kessler_fields {
    const double *density, *pressure;
    double *potential_temperature, *potential_temperature_density;
    double *moisture_density, *cloud_liquid_density, *rain_density;                     /* rho q^v, mu.rho q^cl, mu.rho q^r */
    double *vapor_mass_fraction, *cloud_liquid_mass_fraction, *rain_mass_fraction;      /* mu.q^v, mu.q^cl, mu.q^r          */
    double *rain_terminal_velocity;                                                     /* mu.W^r                          */
    double *precipitation_rate;
} bz_kessler_fields;
int bz_kessler_microphysics_update(bz_ctx *ctx, const bz_kessler_microphysics *params, const bz_kessler_fields *fields,
                                   double dt, double standard_pressure);
/* AtmosphereModel(...; microphysics = DCMIP2016KesslerMicrophysics()) for AnelasticDynamics: rho q^cl and rho q^r join the
 * prognostic fields (prognostic_field_names, dcmip2016_kessler.jl:216) with their U0 / Gn storage; the specific moisture slot
 * of bz_state is q^v; update_state! diagnoses q^cl, q^r, q^v and T = Pi(q) theta + L q^l/c_pm with q = (q^v, q^cl + q^r)
 * (:222-227,298-303,860-865); compute_tendencies! adds -div_rhoUc of both species; ssp_rk3_substep! / store_initial_state!
 * include them; bz_time_step_anelastic ends with the column update + update_state! (ssp_runge_kutta_3.jl:262-263).
 * params == NULL detaches.  bz_kessler_model_update is microphysics_model_update!(microphysics, model) for per-operator drivers. */
typedef struct bz_kessler_model_fields {
    double *cloud_liquid_density, *rain_density;                 /* mu.rho q^cl, mu.rho q^r (prognostic) */
    double *U0_cloud_liquid_density, *U0_rain_density;           /* timestepper.U0                        */
    double *G_cloud_liquid_density, *G_rain_density;             /* timestepper.Gn                        */
    double *vapor_mass_fraction, *cloud_liquid_mass_fraction, *rain_mass_fraction;     /* mu.q^v, q^cl, q^r */
    double *rain_terminal_velocity;                              /* mu.W^r                                */
    double *precipitation_rate;                                  /* horizontal parent (Sx x Sy)           */
} bz_kessler_model_fields;
int bz_set_kessler_microphysics(bz_ctx *ctx, const bz_kessler_microphysics *params, const bz_kessler_model_fields *fields,
                                double standard_pressure);
int bz_kessler_model_update(bz_ctx *ctx, const bz_state *s, const bz_prognostic *G, double dt);
/* The same attachment works for a CompressibleDynamics context (bz_create_compressible): the total density then includes the
 * condensates (compressible_time_stepping.jl:83-103 with condensate_field_names), the Newton temperature inversion carries the
 * latent term, gamma R_m of the linearisation includes the liquid fraction, the species ride the time-averaged transport
 * velocities and the WS-RK3 scalar update, and bz_time_step_compressible ends with the column update (density = rho_d,
 * pressure = dynamics.pressure) + update_state! (acoustic_runge_kutta_3.jl:315-316).  On a y-slab context
 * (bz_create_compressible_slab) the call runs the rank-local column kernel only and the driver's exchanging update_state! follows. */
int bz_compressible_kessler_update(bz_ctx *ctx, const bz_compressible_state *s, const bz_compressible_prognostic *G,
                                   const bz_acoustic_substepper *sub, double dt);

/* ---- microphysics = InstantaneousPrecipitation(equilibrium = WarmPhaseEquilibrium(), solver) on CompressibleDynamics ----
 * The Reed-Jablonowski large-scale condensation of validation/DCMIP2016_TC/dcmip2016_tc.jl:292
 * (src/Microphysics/instantaneous_precipitation.jl:39-185).  The scheme wraps a SaturationAdjustment.  The prognostic moisture is the vapour
 * density rho q^v (bz_compressible_state::rho_q); there are no condensate fields; the microphysical fields are q^v — the specific moisture
 * rho q^v / rho that update_state! diagnoses (bz_compressible_state::q) — and a centre field precipitation_rate in kg m^-3 s^-1.
 * Inside a stage nothing condenses (maybe_adjust_thermodynamic_state returns the state, the moisture fractions are vapour only, :73-86): a
 * stage is the stage of a context without microphysics, and the attachment does not change what any stage kernel computes.
 * Once per step, after the update_state! that follows stage 3 (src/TimeSteppers/acoustic_runge_kutta_3.jl:307-316),
 * microphysics_model_update! (:115-185) does in every interior cell, with dt = clock.last_dt:
 *     rho = total density (as that update_state! left it), rho_d = dry density, q^t = rho q^v / rho, theta_0 = rho theta / rho_d
 *     (T, q^v+, q^l) = adjust_thermodynamic_state(LiquidIceDensityState(theta_0, q^t, p_st, rho), SaturationAdjustment) — the density-based
 *                      warm-phase adjustment of bz_set_saturation_adjustment on a compressible context
 *                      (src/Microphysics/saturation_adjustment.jl:236-301); a subsaturated cell short-circuits with q^v+ = q^t
 *     R_m = (1 - q^v+) R_d + q^v+ R_v,  c_pm = (1 - q^v+) c_pd + q^v+ c_pv
 *     theta_f = T (p_st / (rho R_m T))^(R_m / c_pm)        with_temperature of the vapour-only state (src/Thermodynamics/dynamic_states.jl:251-264):
 *                                                          the condensate leaves, its latent warming stays
 *     c = rho max(0, q^t - q^v+)
 *     rho q^v <- rho q^v+,   rho theta <- rho_d theta_f,   precipitation_rate <- c / dt where c > 0 (a cell that does not condense keeps its rate)
 * and then update_state!(model) with tendencies: rho = rho_d + rho q^v (the total density drops by the rain), T, p, velocities, halos, closure
 * fields and the moisture tendency of the next step's first stage.  The whole update, update_state! included, is skipped when dt is NaN,
 * infinite or <= 0 (:121).  The Newton settings of the temperature inversions are the context's (bz_split_explicit::newton_abstol / _maxiter).
 *
 * bz_set_instantaneous_precipitation: params = the wrapped SaturationAdjustment (constants of the liquid phase and SecantSolver(abstol,
 *   maxiter)), precipitation_rate = the centre field (parent with halos; written at interior cells only).  NULL params detaches.  Every call
 *   invalidates recorded steps.  BZ_ERR_UNSUPPORTED with bz_last_error naming the function: contexts not created by bz_create_compressible
 *   (the anelastic model), contexts with Kessler or saturation adjustment attached, y-slab contexts, contexts with a Bounded x or y or a Flat y.
 * bz_instantaneous_precipitation_update: microphysics_model_update!(microphysics, model) for per-operator drivers;
 *   bz_time_step_compressible calls it after its third stage (a recorded step contains it).
 * bz_column_integral: Field(Integral(field, dims = 3)) of any centre field of the context's grid: out2d[j + Hy][i + Hx] = sum_k field[k] dz_c[k],
 *   summed from k = 0 upward (deterministic); out2d is a device array of (Ny + 2 Hy) x (Nx + 2 Hx) reals, written at interior positions
 *   (the layout of the Kessler scheme's surface precipitation_rate).  surface_precipitation_flux(model) (:99-102) is this of
 *   precipitation_rate, in kg m^-2 s^-1.  Runs on the context's stream without synchronising.  y-slab contexts return BZ_ERR_UNSUPPORTED. */
int bz_set_instantaneous_precipitation(bz_ctx *ctx, const bz_saturation_adjustment *params, double *precipitation_rate);
int bz_instantaneous_precipitation_update(bz_ctx *ctx, const bz_compressible_state *s, const bz_compressible_prognostic *G,
                                          const bz_acoustic_substepper *sub, double dt);
int bz_column_integral(bz_ctx *ctx, const double *field, double *out2d);

/* ---- forcing, f-plane Coriolis and bottom-flux stack of the BOMEX configuration (BASELINE configs[2]) ----
 * Every forcing of examples/bomex.jl:104-196 is a horizontally uniform specific profile multiplied by the reference density
 * (SpecificForcing, src/Forcings/specific_forcing.jl:61-74), so the model's `forcing` NamedTuple reduces to columns:
 *   u_forcing / v_forcing        geostrophic_forcings: -f v_g(z), +f u_g(z) (src/Forcings/geostrophic_forcings.jl)
 *   theta_forcing, moisture_forcing   Forcing(field) profiles keyed under theta / q^e (q^v)
 *   energy_forcing               profile keyed under `e`; enters G_rho_theta as rho F_e / (c_pm Pi)
 *                                (src/PotentialTemperatureFormulations/potential_temperature_tendency.jl:86-104)
 *   subsidence_vertical_velocity SubsidenceForcing(w_s) on the flagged fields: F = -zb-average(w_s dz(horizontal average))
 *                                (src/Forcings/subsidence_forcing.jl:75-91), averages recomputed at every compute_forcings!
 *   coriolis_f                   FPlane(f): -x_f_cross_U, -y_f_cross_U (src/AtmosphereModels/dynamics_kernel_functions.jl:79,99)
 *   bottom_*_flux                FluxBoundaryCondition values on rho theta / rho q (examples/bomex.jl:80-87)
 *   bottom_drag_rho0_ustar2      rho0 u*^2 of the bulk drag FluxBoundaryCondition on rho u, rho v (examples/bomex.jl:95-101)
 *   bottom_drag_epsilon          the regulariser under the square root, J = -rho0 u*^2 rho_u / sqrt(rho_u^2 + rho_v^2 + eps)
 *                                (benchmarking/src/convective_boundary_layer.jl:142-146 uses 1e-10; the BOMEX example none)
 *   bottom_energy_flux           see the member
 * All pointers are HOST arrays (cell centres, length Nz; the subsidence velocity Nz+1 faces), copied by the call; NULL = absent.
 * With a stack attached bz_compute_tendencies adds the forcing + Coriolis terms, and bz_time_step_anelastic calls
 * bz_compute_flux_bc_tendencies before every RK substep (src/TimeSteppers/ssp_runge_kutta_3.jl:229,243,257).
 * Anelastic potential-temperature contexts (microphysics nothing or SaturationAdjustment; single device, or y-slabs through the library-owned
 * distributed step); a single-device CompressibleDynamics context accepts a stack whose only non-zero member is coriolis_f (the f-plane term
 * of its slow momentum tendencies, examples/tropical_cyclone_with_rainband.jl:508-514). */
typedef struct bz_column_forcings {
    const double *u_forcing;
    const double *v_forcing;
    const double *theta_forcing;
    const double *moisture_forcing;
    const double *energy_forcing;
    const double *subsidence_vertical_velocity;
    int32_t subsidence_u, subsidence_v, subsidence_theta, subsidence_moisture;
    double coriolis_f;
    double bottom_theta_flux, bottom_moisture_flux;
    double bottom_drag_rho0_ustar2;
    double bottom_drag_epsilon;
    double bottom_energy_flux;       /* a constant FluxBoundaryCondition keyed rho e in a potential-temperature model: the energy flux Q (W m^-2)
                                        enters rho theta as Q / c_pm with the mixture heat capacity of the lowest cell
                                        (EnergyFluxBoundaryCondition, src/BoundaryConditions/thermodynamic_variable_bcs.jl; BoundaryConditions.jl:218-227) */
} bz_column_forcings;
int bz_set_forcings(bz_ctx *ctx, const bz_column_forcings *forcings);       /* NULL detaches the stack */
/* ---- sponge layers: Relaxation(rate, mask, target) forcings with a horizontally uniform mask and target ----
 * Oceananigans' Relaxation — F = rate * mask(x, y, z) * (target(x, y, z, t) - field) — is how the reference's examples damp the top of
 * the domain: examples/rico.jl:103-105,164 (w = Relaxation(rate, GaussianMask{:z})), examples/neutral_atmospheric_boundary_layer.jl:103-136
 * (rho w relaxed to 0, rho theta to a reference profile), examples/tropical_cyclone_world.jl, tropical_cyclone_with_rainband.jl:434-490.
 * With mask and target functions of z alone the forcing is two columns per field:
 *   rate_*    rate * mask(z) at the field's vertical location (centres, length Nz; rho w: faces, length Nz + 1)
 *   target_*  target(z) there (NULL = 0)
 * for rho u, rho v, rho w, the thermodynamic density (rho theta or rho e) and the moisture density; NULL rate = no relaxation of that field.
 * Keyed by the density name (rho w = ...) the forcing enters the density tendency as is, G += rate (target - rho phi); keyed by the specific
 * name (w = ..., bit set in specific_mask: 1 u, 2 v, 4 w) it is a specific forcing (src/Forcings/specific_forcing.jl:61-74):
 * G += rho_r rate (target - phi) with the reference density at the field's location.  HOST arrays, copied by the call.  bz_compute_tendencies adds the terms
 * after the forcing stack; bz_time_step_anelastic then steps with the tendencies evaluated per operator (fused RK update, projection and
 * diagnosis; y-slab contexts: the operator-by-operator distributed step).  On a single-device CompressibleDynamics context (examples/tropical_cyclone_with_rainband.jl:434-514) the density-keyed
 * sponges of rho u, rho v, rho w, rho theta join the slow tendencies (bz_compute_slow_tendencies), and bz_set_forcings accepts coriolis_f alone. */
typedef struct bz_column_relaxation {
    const double *rate_u, *target_u;
    const double *rate_v, *target_v;
    const double *rate_w, *target_w;
    const double *rate_theta, *target_theta;
    const double *rate_moisture, *target_moisture;
    int32_t specific_mask;
} bz_column_relaxation;
int bz_set_relaxation(bz_ctx *ctx, const bz_column_relaxation *relaxation);      /* NULL detaches */
/* Forcing(f(x, y, z, t)) / Forcing(field) on the thermodynamic variable (examples/tropical_cyclone_with_rainband.jl:419-432,511-514: the
 * prescribed rainband heating keyed `theta`): a DEVICE array at cell centres in the parent layout of the fields, read at every tendency
 * evaluation — the caller owns it and refreshes its contents when the forcing depends on time.  specific = 1 (keyed theta / e): a specific
 * forcing, G_rho_theta += rho F with the coupling density (rho_r(z) of AnelasticDynamics, the prognostic dry density of CompressibleDynamics;
 * src/Forcings/specific_forcing.jl:61-74, compressible_dynamics.jl:385); specific = 0 (keyed rho theta / rho e): G += F.  NULL detaches.
 * On a y-slab the array is the slab's own parent array.  Compressible y-slabs: not built. */
int bz_set_field_forcing(bz_ctx *ctx, const double *thermodynamic_forcing, int specific);
/* compute_forcings!(model) (src/AtmosphereModels/update_atmosphere_model_state.jl:81-86) */
int bz_compute_forcings(bz_ctx *ctx, const bz_state *s);
/* compute_flux_bc_tendencies!(model) (src/AtmosphereModels/update_atmosphere_model_state.jl:418-434) */
int bz_compute_flux_bc_tendencies(bz_ctx *ctx, const bz_state *s, const bz_prognostic *G);
/* Bulk aerodynamic bottom conditions with constant transfer coefficients on unfiltered fields:
 *   BulkDrag on rho u, rho v               J^u = -rho0 C^D U~ u          (src/BoundaryConditions/bulk_drag.jl:114-135)
 *   BulkSensibleHeatFlux on rho theta      J^th = -rho0 C^T U~ (theta - theta0)  (bulk_scalar_fluxes.jl:82-90,123-137)
 *   BulkVaporFlux on the moisture density  J^v = -rho0 C^v U~ (q^v - q^v+(T0, rho0))  (bulk_scalar_fluxes.jl:206-232)
 * with U~ = sqrt(U^2 + gustiness^2), U^2 interpolated to the flux location (BoundaryConditions.jl:64-85), rho0 = p0 / (R^d T0)
 * (src/Thermodynamics/reference_states.jl:73-76), theta0 = T0 / (p0/p_st)^(R^d/c_pd).  A coefficient <= 0 switches that
 * condition off.  Applied by bz_compute_flux_bc_tendencies (and inside bz_time_step_anelastic) next to the constant fluxes of
 * bz_column_forcings.  PolynomialCoefficient and FilteredSurfaceVelocities: bz_set_surface_layer below. */
typedef struct bz_bulk_surface_fluxes {
    double drag_coefficient, drag_gustiness, drag_surface_temperature;
    double heat_coefficient, heat_gustiness, heat_surface_temperature;
    double vapor_coefficient, vapor_gustiness, vapor_surface_temperature;
    double surface_pressure, standard_pressure;
    /* liquid CondensedPhase + triple point of ThermodynamicConstants, for q^v+ of the vapour flux */
    double liquid_latent_heat, liquid_heat_capacity, energy_reference_temperature, triple_point_temperature, triple_point_pressure;
} bz_bulk_surface_fluxes;
int bz_set_bulk_surface_fluxes(bz_ctx *ctx, const bz_bulk_surface_fluxes *fluxes);      /* NULL detaches */

/* ---- wind- and stability-dependent bulk fluxes on a filtered surface state (examples/prescribed_sea_surface_temperature.jl:39-72) ----
 * The same three bottom conditions with, per condition, either a constant coefficient or a PolynomialCoefficient
 * (src/BoundaryConditions/polynomial_bulk_coefficient.jl), a surface temperature that is a number or a (Ny x Nx) centre array, and
 * optionally FilteredSurfaceVelocities (filtered_surface_state.jl).  Per surface cell and condition:
 *   T0 = surface temperature at index (i, j) (the drag at an x or y face reads the centre array at its own index: surface_value(i, j, .)),
 *   rho0 = p0 / (R^d T0), theta0 = T0 / (p0/p_st)^(R^d/c_pd), q^v+ = p^v+(T0) / (rho0 R^v T0)           (per cell)
 *   U~ = sqrt(U^2 + gustiness^2) with U^2 at the flux's own location multiplies the flux (BoundaryConditions.jl:64-124),
 *   C = polynomial: C10 (ln(10/l) / ln(h/l))^2 [x stability factor], C10 = (a0 + a1 Us + a2 / Us) 1e-3, Us = max(U, U_min), where U is
 *       the un-gusted wind speed at the CENTRE (i, j) for all three conditions (bulk_coefficient, :687-707) and h the first centre height;
 *       stability (FittedStabilityFunction): Ri_B from theta_v of the first cell, theta_v0 = T0 (1 + delta q^v+_t(T0, p0)) (the
 *       pressure-based saturation_total_specific_moisture) and the literal g = 9.81 of bulk_richardson_number; Li et al. (2010) three-regime
 *       zeta mapping, Hogstrom / Beljaars-Holtslag Psi functions, momentum or scalar correction factor.  Every branch is a select.
 * With filtering every velocity, theta_v, theta and the vapour flux's moisture come from context-owned 2-D fields
 *   f^ <- (f^ + eps f) / (1 + eps)   (u^ at x faces, v^ at y faces, theta_v^, theta^, q^ at centres; first-level values; the moisture is
 *   the specific PROGNOSTIC moisture s->q (update_boundary_conditions.jl:47), while the unfiltered vapour flux reads q^v),
 * whose neighbour reads wrap periodically and collapse onto the cell in a Flat direction.
 * One launch per flux evaluation over the Nx x Ny surface, one launch per filter update; no synchronisation, no allocation per call;
 * captured steps (bz_graph_enable) replay both.  The lean seam never carries these fluxes: with a configuration attached
 * bz_time_step_anelastic / bz_time_steps_anelastic take the tiers that diagnose after every stage (every step of an n-step call),
 * so the filter always reads current first-level diagnostics.
 * Inside the library-owned whole steps the filter advances with eps = dt / filter_timescale after update_state! of the stages named by
 * filter_stage_mask (bit 0: first stage ... bit 2: third stage): the reference advances it once per new (clock.iteration, clock.stage)
 * key, which is the host clock's business.  The per-operator sequence calls bz_surface_layer_update itself.
 * BZ_ERR_UNSUPPORTED (with bz_last_error naming the reason): compressible, StaticEnergy and Kessler contexts, y-slab contexts, a filter
 * reference height other than the first cell centre (filter_height_set != 0), filtering on a Bounded x or y.  PlanarIceSurface: not built. */
typedef struct bz_polynomial_coefficient {
    double a0, a1, a2;                       /* polynomial (the host fills the defaults per condition type) */
    double roughness_length, minimum_wind_speed;
    int32_t stability, reserved;             /* 1: FittedStabilityFunction, 0: stability_function = nothing */
    double scalar_roughness_length;
    /* RichardsonNumberMapping, in the reference's field order */
    double stable_unstable_transition, strongly_stable_transition;
    double au11, bu11, bu12, au21, au22, bu31, bu32, bu33;
    double aw11, aw12, aw21, aw22, bw11, bw12, bw21, bw22;
    double as11, as21, bs11, bs21, bs22;
    /* StabilityFunctionParameters */
    double gamma_d, gamma_t, psi_a, psi_b, psi_c, psi_d;
} bz_polynomial_coefficient;
typedef struct bz_surface_flux {
    int32_t enabled, polynomial;             /* polynomial = 0: `coefficient` is used */
    double coefficient, gustiness;
    double surface_temperature;              /* used when the field is NULL */
    const double *surface_temperature_field; /* HOST (Ny x Nx), row j column i; copied by the call */
    bz_polynomial_coefficient poly;
} bz_surface_flux;
typedef struct bz_surface_layer {
    bz_surface_flux drag, heat, vapor;
    double surface_pressure, standard_pressure;
    double liquid_latent_heat, liquid_heat_capacity, energy_reference_temperature, triple_point_temperature, triple_point_pressure;
    int32_t filtered, filter_height_set;
    double filter_height, filter_timescale;
    int32_t filter_stage_mask, reserved;
} bz_surface_layer;
int bz_set_surface_layer(bz_ctx *ctx, const bz_surface_layer *layer);      /* NULL detaches and frees the 2-D fields */
/* initialize!(model): the filtered fields take the first-level values of `s` (diagnostics current) */
int bz_surface_layer_initialize(bz_ctx *ctx, const bz_state *s);
/* update!(fv, ..., dt) with epsilon = dt / tau */
int bz_surface_layer_update(bz_ctx *ctx, const bz_state *s, double epsilon);
/* the filtered 2-D fields as HOST (Ny x Nx) arrays; which = 0 u^, 1 v^, 2 theta_v^, 3 theta^, 4 q^.  get synchronises. */
int bz_surface_layer_get_filtered(bz_ctx *ctx, int which, double *host);
int bz_surface_layer_set_filtered(bz_ctx *ctx, int which, const double *host);

/* ---- bulk surface fluxes on CompressibleDynamics (csrc/bz_cmp_surface_flux.hip; validation/DCMIP2016_TC/dcmip2016_tc.jl:293-311) ----
 * The three bottom conditions of bz_bulk_surface_fluxes above — same formulas, same sources — with a constant coefficient, a gustiness
 * and, per condition, a surface temperature that is a number or a HOST (Ny x Nx) centre array (row j, column i; copied by the call):
 *   rho0 = p0 / (R^d T0), theta0 = T0 / (p0/p_st)^(R^d/c_pd), q^v+ = p^v+(T0) / (rho0 R^v T0) over a planar liquid surface, per cell;
 *   the drag at an x or y face reads the centre array at its own index.  p0 is the dynamics' surface_pressure.  p^v+ is the
 *   Clausius-Clapeyron form of the constants below; on a context with DCMIP2016 Kessler microphysics, whose constants carry a
 *   TetensFormula, it is that formula with the attached scheme's parameters (src/Thermodynamics/tetens_formula.jl:110-117).
 * Fields read: the first level of the state's u, v, theta and of q^v — the diagnosed vapour fraction while a SaturationAdjustment is
 * attached, else the specific prognostic moisture s->q (InstantaneousPrecipitation, Kessler, no microphysics).  Neighbours of u, v by
 * periodic wrap indexing.  Fluxes enter where the reference adds them (src/TimeSteppers/acoustic_runge_kutta_3.jl:187-196): after the slow
 * tendencies of a stage and before its substep loop, once per stage, in bz_acoustic_rk3_substep and in every stage of
 * bz_time_step_compressible — G_rho_u, G_rho_v, G_rho_theta and the moisture tendency the previous update_state! left take J / dz_1 at the
 * first level, by ONE launch over the Nx x Ny surface (no allocation, no synchronisation; captured steps replay it).  While a vapour flux
 * is attached the dry shortcut of the step (bz_moisture.hip) is off: evaporation into a dry model is a moisture source.
 * bz_compressible_compute_flux_bc_tendencies is compute_flux_bc_tendencies!(model) alone, for per-operator drivers: it ADDS to G.
 * BZ_ERR_UNSUPPORTED (bz_last_error names the function and the reason): anelastic and kinematic contexts, y-slab contexts, a Bounded x or
 * y, a Flat y.  PolynomialCoefficient and FilteredSurfaceVelocities are not built on CompressibleDynamics (bz_set_surface_layer refuses). */
typedef struct bz_compressible_surface_flux {
    int32_t enabled, reserved;
    double coefficient, gustiness;
    double surface_temperature;              /* used when the field is NULL */
    const double *surface_temperature_field; /* HOST (Ny x Nx), row j column i; copied by the call */
} bz_compressible_surface_flux;
typedef struct bz_compressible_surface_fluxes {
    bz_compressible_surface_flux drag, heat, vapor;
    double surface_pressure, standard_pressure;
    /* liquid CondensedPhase + triple point of ThermodynamicConstants, for q^v+ of the vapour flux */
    double liquid_latent_heat, liquid_heat_capacity, energy_reference_temperature, triple_point_temperature, triple_point_pressure;
} bz_compressible_surface_fluxes;
int bz_set_compressible_surface_fluxes(bz_ctx *ctx, const bz_compressible_surface_fluxes *fluxes);      /* NULL detaches */
int bz_compressible_compute_flux_bc_tendencies(bz_ctx *ctx, const bz_compressible_state *s, const bz_compressible_prognostic *G);

/* ---- user tracers of the anelastic model: AtmosphereModel(grid; tracers = (:a, :b)) ----
 * density = model.tracers.c (prognostic rho c), specific = c = rho c / rho_r (the reference converts in place around the tendency
 * evaluation, src/AtmosphereModels/update_atmosphere_model_state.jl:43,65,88-112; here it is a separate centre array), U0 / G the
 * timestepper mirrors.  Each tracer gets the WENO-5 scalar tendency -div_rhoUc(c) (:352-372) and the SSP-RK3 update.  At most
 * BZ_MAX_TRACERS; n = 0 detaches.  Single-device anelastic contexts; not combined with a closure in this build. */
#define BZ_MAX_TRACERS 8
typedef struct bz_tracer_fields {
    double *density;
    double *specific;
    double *U0;
    double *G;
} bz_tracer_fields;
int bz_set_tracers(bz_ctx *ctx, int32_t n, const bz_tracer_fields *tracers);

/* ---- bounds-preserving WENO for moisture-like scalars (second half) ----
 * advection = (; rho_q^e = WENO(order = 5, bounds = (0, 1)), ...) (examples/rico.jl:184-190, examples/tropical_cyclone_world.jl:169):
 * div_rhoUc(i, j, k, grid, ::BoundsPreservingWENO, rho, U, c) = V^-1 (bounded_tracer_flux_divergence_x + _y + _z)
 * (src/Advection.jl:42-47); the three divergences are Oceananigans' positivity-preserving limiter (not vendored; restated in
 * oracle/breeze_oracle.c: parity unpinned).  Flags select the scalars that use it: the moisture density (rho q^v / rho q^e), the
 * prognostic species of the attached microphysics (rho q^cl, rho q^r), the user tracers.  With any flag set bz_compute_tendencies
 * replaces those scalars' advective tendencies and bz_time_step_anelastic runs its operator-sequence tier.  Single-device anelastic
 * contexts of the WENO build; NULL detaches. */
typedef struct bz_bounds_preserving_advection {
    double lower, upper;
    int32_t moisture, microphysical_species, tracers, reserved;
} bz_bounds_preserving_advection;
int bz_set_bounds_preserving_advection(bz_ctx *ctx, const bz_bounds_preserving_advection *bounds);

/* ---- closure = SmagorinskyLilly() (BASELINE configs[2]) ----
 * Breeze's part — density-weighted stress and flux divergences (src/TurbulenceClosures/TurbulenceClosures.jl:44-101), their place
 * in the tendencies (src/AtmosphereModels/dynamics_kernel_functions.jl:80,100,128,157), N^2 = g dz(log theta_v)
 * (src/AtmosphereModels/atmosphere_model_buoyancy.jl:46-68) and compute_closure_fields! at the end of
 * compute_auxiliary_variables! (src/AtmosphereModels/update_atmosphere_model_state.jl:218) — is followed line by line; the eddy
 * viscosity and kinematic fluxes are Oceananigans' SmagorinskyLilly (0.110.14, not vendored), restated from its published form
 * (oracle/closure.py: parity unpinned).  eddy_viscosity is model.closure_fields.nu_e (centre field parent, caller-owned).
 * With a closure attached bz_compute_tendencies subtracts the divergences after the advective terms.  Anelastic potential-temperature
 * contexts, and compressible contexts (bz_create_compressible) on one device that are periodic in x and y: there the closure terms are
 * slow terms of the split-explicit step (src/TimeSteppers/acoustic_substep_helpers.jl:55-93) —
 *   bz_compute_slow_tendencies subtracts d_j T_ij from G_rho_u, G_rho_v, G_rho_w and div J from G_rho_theta (c = theta) with the 3-D
 *     dynamics density rho_d at the flux locations: the cell value at ccc, the two-point means of the field at the faces, the four-point
 *     means at ffc / fcf / cff in the order of the nu averages, through the field's own halos; G_rho_d gets nothing;
 *   bz_compute_moisture_tendency (and the update_state! of whole steps) subtracts div J from the tendencies of rho q and, with Kessler,
 *     rho q^cl and rho q^r with the TOTAL density at the faces, one launch for all of them;
 *   every update_state! (bz_compressible_update_state, the stage ends of bz_time_step_compressible, bz_compressible_kessler_update) ends with
 *     compute_closure_fields!: N^2 = g dz(log theta_v) with theta_v from the model's 3-D pressure at each cell (dynamics_pressure) and
 *     q^v = specific_humidity(model), then the halos of nu_e (periodic in x / y, zero gradient in z).  T and p carry zero-gradient z halos,
 *     so the bottom and top face values of dz(log theta_v) are exact zeros.  The slow tendencies of a stage use the nu_e of the
 *     update_state! before it.
 * Compressible contexts with a Bounded x or y, a Flat y or on a y-slab return BZ_ERR_UNSUPPORTED naming the option. */
typedef struct bz_smagorinsky_lilly {
    double smagorinsky_coefficient;   /* C  = 0.16 */
    double reduction_factor;          /* Cb = 1.0: varsigma = sqrt(1 - min(1, Cb N^2+ / Sigma^2)) */
    double prandtl_number;            /* Pr = 1.0 (every scalar) */
} bz_smagorinsky_lilly;
int bz_set_closure(bz_ctx *ctx, const bz_smagorinsky_lilly *closure, double *eddy_viscosity);   /* NULL detaches */
int bz_compute_closure_fields(bz_ctx *ctx, const bz_state *s);
/* Which kernels the closure of this context launches (read-only; no reference counterpart).  *marches = 1: the z-marching LDS-tiled
 * kernels (k_smagorinsky_march, k_closure_march) — SmagorinskyLilly attached, x periodic, y periodic or a y-slab, Nx a multiple of 64, the
 * (local) Ny a multiple of 8, Nz >= 4, Hz >= 2, and BZ_NO_CLOSURE_MARCH unset when the context was created; 0: the cell-per-thread kernels
 * (or no SmagorinskyLilly closure).  Both compute the same expressions in the same order: the choice changes no bit of nu_e or of a
 * tendency.  It is the verdict of the one host predicate every launch site of csrc/bz_closure.hip asks. */
int bz_closure_march_info(bz_ctx *ctx, int32_t *marches);

/* ---- closure = ScalarDiffusivity(...) / VerticalScalarDiffusivity(...), explicit or vertically implicit (csrc/bz_diffusivity.hip) ----
 * Breeze's part is followed line by line: dynamic fluxes = rho_r at the flux location x Oceananigans' kinematic flux, with the
 * closure's time discretisation passed into every flux (src/TurbulenceClosures/TurbulenceClosures.jl:48-101), and
 * implicit_step!(field, solver, closure, ..., alpha dt) after the RK update of every prognostic field
 * (src/TimeSteppers/ssp_runge_kutta_3.jl:124-161; order inside a stage :229-236: flux-BC tendencies, RK update, implicit step,
 * pressure correction, update_state!).  Oceananigans (0.110.14) is not vendored: what follows is the reading — PARITY UNPINNED, pinned
 * only by closed forms and the reference's own known answers (test/vertical_diffusion.jl, test/turbulence_closures.jl:14-50;
 * tests/scalar_diffusivity_reference.py restates it on the CPU).
 *   formulation 0 (isotropic): the SmagorinskyLilly fluxes with the given nu in place of nu_e and an independent kappa: stresses
 *     -2 nu Sigma_ij with nu averaged to ccc / ffc / fcf / cff, scalar fluxes -kappa grad c with kappa averaged to the face.
 *   formulation 1 (vertical): only tau_uz = -nu_fcf dz u, tau_vz = -nu_cff dz v, tau_wz = -nu_ccc dz w, J_z = -kappa_ccf dz c.
 *   time_discretization 1 (vertically implicit): the explicit tendency drops what the solve covers — vertical formulation: all four
 *     z fluxes; isotropic: tau_uz -> -nu_fcf dx w, tau_vz -> -nu_cff dy w (the cross terms stay explicit), tau_wz -> 0, J_z -> 0,
 *     horizontal fluxes unchanged.  The fluxes on the boundary faces k = 1 and Nz + 1 stay explicit in Oceananigans; they vanish
 *     under the default no-flux / impenetrable conditions (the only ones here), so there is no code for them.
 *   implicit step: (I - dtau dz K dz) phi = phi* on the density-weighted prognostic field itself (rho u, rho v, rho w, rho theta or
 *     rho e, the moisture density, Kessler species, tracer densities); no density in the operator — the reference's own asymmetry
 *     (test/turbulence_closures.jl:38-50 accepts rtol 1e-5 for a uniform e).  Rows of z-centre fields, k = 1 .. Nz, K^f = K at the
 *     z face of the field's own column (nu_fcf, nu_cff, kappa_ccf): upper(k) = -dtau K^f[k+1] / (dz^c[k] dz^f[k+1]) (0 at Nz),
 *     lower(k) = -dtau K^f[k] / (dz^c[k] dz^f[k]) (0 at 1), diag = 1 - upper - lower.  Rows of rho w, faces k = 2 .. Nz, nu at
 *     centres: upper(k) = -dtau nu[k] / (dz^f[k] dz^c[k]), lower(k) = -dtau nu[k-1] / (dz^f[k] dz^c[k-1]), diag = 1 - upper - lower;
 *     the wall value w = 0 enters rows 2 and Nz through the diagonal only; faces 1 and Nz + 1 are never written
 *     (src/AtmosphereModels/implicit_vertical_advection.jl:202-214,270-292 documents the same z-Face convention).  K = 0 gives
 *     identity rows; a closure whose nu (kappa) is the number 0 skips the momentum (the scalars) altogether.
 * nu_field / kappa_field: centre field parents with the model's halos (caller-owned; NULL: the number in the struct).  The library
 * fills their halos — periodic in x and y, zero gradient in z — before every use (bz_compute_closure_fields, bz_compute_tendencies,
 * bz_implicit_step), because the user may have rewritten them.  Mutually exclusive with bz_set_closure: the second attach returns
 * BZ_ERR_UNSUPPORTED.  Single-device contexts, periodic in x and y (or, anelastic, Flat y); y-slab, walled and kinematic contexts return
 * BZ_ERR_UNSUPPORTED naming the option.  With one attached bz_compute_tendencies subtracts the explicit
 * divergences where it subtracts SmagorinskyLilly's, and bz_time_step(s)_anelastic run the implicit step of every stage (never on
 * the lean tier).  Compressible contexts take the explicit discretisation only (time_discretization 1, or a Flat y, returns
 * BZ_ERR_UNSUPPORTED naming the option): the divergences enter where SmagorinskyLilly's do — rho_d at the flux locations for momentum and
 * rho theta, the total density for the water scalars — and the halos of a field-valued K are refilled before every use.  NULL detaches. */
typedef struct bz_scalar_diffusivity {
    int32_t formulation;           /* 0: ScalarDiffusivity (isotropic), 1: VerticalScalarDiffusivity */
    int32_t time_discretization;   /* 0: ExplicitTimeDiscretization, 1: VerticallyImplicitTimeDiscretization */
    double nu;                     /* used where nu_field == NULL */
    double kappa;                  /* used where kappa_field == NULL (every scalar) */
} bz_scalar_diffusivity;
int bz_set_scalar_diffusivity(bz_ctx *ctx, const bz_scalar_diffusivity *c, double *nu_field, double *kappa_field);
/* implicit_step! of every prognostic field of the context with dtau = dt (a stage passes alpha dt): one launch.  Interior cells only:
 * the halos are left to the operators that follow (bz_compute_pressure_correction and bz_update_state fill what they read).  A no-op
 * without a vertically implicit closure. */
int bz_implicit_step(bz_ctx *ctx, const bz_state *s, double dt);

/* ---- the reductions of the run! loop around the step ---- */
/* cell_advection_timescale(model) (src/AtmosphereModels/cell_advection_timescale.jl:47-66): minimum over the interior of
 * 1 / (|u|/dx + |v|/dy + |w|/dz) into *out (host; +Inf for a fluid at rest); w == NULL gives the HorizontalFormulation.
 * Synchronises the stream.  u, v, w: velocity parent arrays (a slab rank reduces its own slab; combine with a min). */
int bz_cell_advection_timescale(bz_ctx *ctx, const double *u, const double *v, const double *w, double *out);
/* NaNChecker on one field (default_nan_checker, src/AtmosphereModels/atmosphere_model.jl:561-572): *out = 1 if any
 * interior value is NaN.  Synchronises. */
int bz_any_nan(bz_ctx *ctx, const double *field, int z_face, int32_t *out);

/* ---- output diagnostics: what the run! loop evaluates between steps for its output writers (csrc/bz_diagnostics.hip) ----
 * KernelFunctionOperations of src/AtmosphereModels/Diagnostics/ and src/Microphysics/microphysics_diagnostics.jl, evaluated by one
 * pointwise kernel.  Notation: q = (q^v, q^l, q^i = 0), R_m = q^d R^d + q^v R^v, c_pm = q^d c_pd + q^v c_pv + q^l c_l,
 * rho* = p / (R_m T), p^v = rho* q^v R^v T, p^v+(T) the Clausius-Clapeyron pressure over a planar liquid surface, H = p^v / p^v+.
 *   POTENTIAL_TEMPERATURE                      theta = T / (p/p_st)^(R_m/c_pm)                      (potential_temperatures.jl:538-616)
 *   LIQUID_ICE_POTENTIAL_TEMPERATURE           theta (1 - L_lr q^l / (c_pm T))
 *   VIRTUAL_POTENTIAL_TEMPERATURE              T / (p/p_st)^(R^d/c_pd) (1 + (R^v/R^d - 1) q^v - q^l)
 *   EQUIVALENT_POTENTIAL_TEMPERATURE           T (p_st/p)^(R^d/c_pm) exp(L_l(T) q^v / (c_pm T)) H^(-R^v q^v / c_pm),
 *                                              L_l(T) = L_lr + (c_pv - c_l)(T - T_r)
 *   STABILITY_EQUIVALENT_POTENTIAL_TEMPERATURE theta^e (T/T_r)^(c_l q^l / c_pm)
 *   STATIC_ENERGY                              c_pm T + g z_c[k] - L_lr q^l                         (static_energy.jl:94-120)
 *   RELATIVE_HUMIDITY                          p^v / max(p^v+(T), eps)                              (microphysics_diagnostics.jl:139-170)
 *   SATURATION_SPECIFIC_HUMIDITY               :prognostic, p^v+ / (rho* R^v T)                     (saturation_specific_humidity.jl:124-149)
 *   SATURATION_SPECIFIC_HUMIDITY_EQUILIBRIUM   :equilibrium, equilibrium_saturation_specific_humidity(T, p, q^ve) (vapor_saturation.jl:216-230)
 *   SATURATION_SPECIFIC_HUMIDITY_TOTAL_MOISTURE :total_moisture, eps p^v+ / (p + (eps - 1) p^v+), eps = R^d / R^v
 *   DEWPOINT_TEMPERATURE                       secant inversion of p^v+(T+) = p^v: T where p^v+(T) - p^v <= 0, else from the guesses T and
 *                                              T - 20 (1 - H) with SecantSolver(reltol = 1e-4, abstol = 0, maxiter = 10) scaled by p^v
 *                                              (vapor_saturation.jl:313-331)
 * kind | BZ_DIAG_DENSITY_WEIGHTED is the density-weighted flavour (rho x) of a potential temperature or of the static energy. */
typedef enum bz_diagnostic_kind {
    BZ_DIAG_POTENTIAL_TEMPERATURE = 0,
    BZ_DIAG_LIQUID_ICE_POTENTIAL_TEMPERATURE = 1,
    BZ_DIAG_VIRTUAL_POTENTIAL_TEMPERATURE = 2,
    BZ_DIAG_EQUIVALENT_POTENTIAL_TEMPERATURE = 3,
    BZ_DIAG_STABILITY_EQUIVALENT_POTENTIAL_TEMPERATURE = 4,
    BZ_DIAG_STATIC_ENERGY = 5,
    BZ_DIAG_RELATIVE_HUMIDITY = 6,
    BZ_DIAG_SATURATION_SPECIFIC_HUMIDITY = 7,
    BZ_DIAG_SATURATION_SPECIFIC_HUMIDITY_EQUILIBRIUM = 8,
    BZ_DIAG_SATURATION_SPECIFIC_HUMIDITY_TOTAL_MOISTURE = 9,
    BZ_DIAG_DEWPOINT_TEMPERATURE = 10,
    BZ_DIAG_KIND_COUNT = 11
} bz_diagnostic_kind;
#define BZ_DIAG_DENSITY_WEIGHTED 0x100
#define BZ_MAX_DIAGNOSTICS 24
/* The inputs are passed explicitly (the kernel knows no model): DEVICE parent arrays at cell centres.
 *   temperature, vapor   T and q^v (grid_moisture_fractions: q^t without microphysics, the stored q^v otherwise)
 *   liquid, liquid_2     q^l; either may be NULL (read as 0); liquid_2 is added to liquid (Kessler: q^cl + q^r, dcmip2016_kessler.jl:298-303)
 *   moisture             q^ve, the specific prognostic moisture: read by the :equilibrium flavour only
 *   pressure, density    3-D fields (CompressibleDynamics: dynamics_pressure_for_potential_temperature); if either is NULL the
 *                        context's reference-state columns p_r[k], rho_r[k] are used
 * and the liquid CondensedPhase, energy reference temperature and triple point of ThermodynamicConstants
 * (src/Thermodynamics/thermodynamics_constants.jl:92,182-194), which a context without microphysics does not hold. */
typedef struct bz_diagnostic_inputs {
    const double *temperature, *vapor, *liquid, *liquid_2, *moisture, *pressure, *density;
    double liquid_latent_heat, liquid_heat_capacity;
    double energy_reference_temperature, triple_point_temperature, triple_point_pressure;
} bz_diagnostic_inputs;
/* n >= 1 diagnostics (kinds[m], at most BZ_MAX_DIAGNOSTICS) into n cell-centred parent arrays outputs[m] from ONE read of the inputs; only
 * the interior is written (fill halos with bz_fill_halo_regions).  Asynchronous on the context's stream.  If the context's diagnostics are
 * stale (bz_diagnostics_stale) they are rebuilt first from `s` (NULL is accepted while they are current, and on compressible contexts).
 * Works on y-slab contexts as on any other: the kernel is pointwise. */
int bz_compute_diagnostics(bz_ctx *ctx, const bz_state *s, const bz_diagnostic_inputs *inputs, int32_t n, const int32_t *kinds,
                           double *const *outputs);
/* Average(field, dims = (1, 2)): the mean over the interior Nx x Ny cells of every level of one centre (z_face = 0: Nz levels) or z-face
 * (z_face != 0: Nz + 1 levels) parent array, into `profile` (HOST).  Halos are never read.  Deterministic: fixed block and summation order,
 * no floating-point atomics; the level sum is divided by Nx Ny.  Synchronises.  y-slab contexts (bz_create_slab,
 * bz_create_compressible_slab) return BZ_ERR_UNSUPPORTED. */
int bz_horizontal_average(bz_ctx *ctx, const double *field, int z_face, double *profile);

/* ---- turbulence statistics: Average(expression, dims = (1, 2)) of products, powers and vertical derivatives (csrc/bz_moments.hip) ----
 * The profiles the reference's LES examples average every step inside an AveragedTimeInterval window
 * (examples/neutral_atmospheric_boundary_layer.jl:203-221: u^2, u*w, θ*w, u^2*w, w^3, νₑ^3, ∂z(u), ... under @at((Center, Center, Center), ·);
 * rico.jl:281-282; tropical_cyclone_world.jl:244-249), all of one list from ONE pass over the fields they are functions of.
 * The semantics are those of Oceananigans' BinaryOperation, ^, ∂z and @at as the example's comments describe them.  Oceananigans is not
 * vendored with the reference, so this is a READING of it, not a checked parity:
 *   location   The location L of a moment is that of its first factor; with `dz` its z location is flipped.  On a Flat y there is no y
 *              location (face_y is ignored) and no y interpolation.
 *   value      At a point of L:  f0^p0 · ℑ_L(f1^p1) · ℑ_L(f2^p2), multiplied left to right.  A power is repeated multiplication and is
 *              applied BEFORE the interpolation, as in a * (b^p).  ℑ_L is the two-point mean (a + b) / 2 in every direction in which
 *              the factor's location differs from L, composed with x outermost and z innermost: centre -> face at index i uses the
 *              centres i - 1 and i, face -> centre at i the faces i and i + 1.
 *   dz         ∂z of the single factor (n_factors == 1, power == 1): centre -> face k is (f[k] - f[k-1]) / Δzᵃᵃᶠ[k], face -> centre k is
 *              (f[k+1] - f[k]) / Δzᵃᵃᶜ[k], with the grid's own spacings (true divisions).
 *   at_center  The field of values at L is interpolated to (Center, Center, Center) with the same ℑ rules before it is averaged.
 *   profile    profiles[m (Nz + 1) + k], k < nlev[m]: the sum over the Nx × Ny interior points of level k divided by Nx Ny, in the
 *              context's float type.  nlev[m] = Nz + 1 if L is a z face and at_center == 0, else Nz; the remaining entries of a row are 0.
 * Halo reads: at most ONE halo cell in each direction, corners included (the ℑxy of u*v; the z halo under the bottom and above the top
 * face for θ*w and ∂z).  The caller provides filled halos; cells further out are never read.  Contexts need Hx, Hy (unless Flat), Hz >= 1.
 * Deterministic: fixed summation order (that of bz_horizontal_average: a plain field gives the same bits as that call), no floating-point
 * atomics; the bits of a moment's profile depend neither on the other moments of the call nor on their order.  Runs on the context's
 * stream, makes one device -> host copy and synchronises once.  The kernel knows no model: anelastic, compressible, Flat-y and Float32
 * contexts alike.  The caller rebuilds stale diagnostics first if a field is one of them (bz_diagnostics_stale).
 * BZ_ERR_UNSUPPORTED: y-slab contexts; on contexts with walls in x or y any moment with a field or L at a horizontal face (moments of
 * horizontally centred fields run: nothing there is wall-specific).  BZ_ERR_INVALID: counts outside the limits below, a null array, a face
 * flag other than 0 / 1, a field index out of range, a power outside 1 .. 3, dz with more than one factor or a power.  bz_last_error names
 * the argument; nothing is launched. */
#define BZ_MAX_MOMENT_FIELDS 8
#define BZ_MAX_MOMENTS 24
#define BZ_MAX_MOMENT_FACTORS 3
typedef struct bz_moment_field {
    const double *data;      /* DEVICE parent array */
    int32_t face_x, face_y, face_z;      /* 0: Center, 1: Face */
} bz_moment_field;
typedef struct bz_moment {
    int32_t n_factors;                          /* 1 .. 3 */
    int32_t field[BZ_MAX_MOMENT_FACTORS];       /* index into fields[] */
    int32_t power[BZ_MAX_MOMENT_FACTORS];       /* 1 .. 3 */
    int32_t dz;                                 /* 1: ∂z of the single factor */
    int32_t at_center;                          /* 1: interpolate the result to (Center, Center, Center) before averaging */
} bz_moment;
int bz_horizontal_moments(bz_ctx *ctx, int32_t n_fields, const bz_moment_field *fields, int32_t n_moments, const bz_moment *moments,
                          double *profiles /* HOST, n_moments rows of Nz + 1 */, int32_t *nlev /* HOST, n_moments */);

/* ---- azimuthal means and polar winds (csrc/bz_azimuthal.hip; src/AtmosphereModels/Diagnostics/azimuthal_mean.jl of the reference) ---- */
/* The cell-centre coordinates of the grid, x^c[0 .. Nx) and y^c[0 .. Ny) (HOST arrays, copied; xnodes / ynodes of the caller's grid at
 * Center).  bz_grid carries spacings only, and the ring membership of a sample must be formed from the very coordinates the caller's grid
 * holds, not from ones re-derived from extents.  Required once before bz_azimuthal_mean / bz_polar_winds.  Synchronises. */
int bz_set_horizontal_nodes(bz_ctx *ctx, const double *xc, const double *yc);
/* azimuthal_mean(field; radius, Nr, center = (center_x, center_y), m): the mean of one centre (z_face = 0: Nz levels) or z-face
 * (z_face != 0: Nz + 1 levels) DEVICE parent array over Nr uniform rings on [0, radius], dr = radius / Nr, by binning an m x m block of
 * sub-cell centres per cell:
 *     x = (x^c[i] - center_x) + (2 si - m - 1) dx / (2 m),  y likewise,  1 <= si, sj <= m      (product, then quotient, then sum)
 *     the sample is in ring ir (1-based) iff trunc(sqrt(x x + y y) / dr) + 1 == ir; samples past the radius fall in no ring
 *     profile[k Nr + ir - 1] = sum of field[i, j, k] over the ring's samples / their number, NaN for a ring without samples
 * all in the context's float type, without FMA contraction and with correctly rounded divide and sqrt, so that the ring of every sample is
 * the one the reference's expression gives.  `profile` (HOST) has nlev x Nr entries, ring index fastest; `counts` (HOST, Nr entries, may
 * be NULL) receives the number of samples per ring, the same for every level.  Halos are never read; the value of a cell without a sample
 * inside the radius is not used at all.  A centre outside the domain is legal.
 * Deterministic: the ring geometry is worked out once per (center, radius, Nr, m) and kept on the context; a ring's sum is accumulated in
 * a fixed order (cell order within a wave's share, waves, then row slices), no floating-point atomics: two calls return the same bits.
 * Runs on the context's stream and synchronises.  The caller rebuilds stale diagnostics first if `field` is one of them
 * (bz_diagnostics_stale).
 * Limits: 1 <= Nr <= 1024, 1 <= m <= 16, radius > 0, else BZ_ERR_INVALID with bz_last_error naming the argument.  Flat-y contexts and
 * y-slab contexts (bz_create_slab, bz_create_compressible_slab) return BZ_ERR_UNSUPPORTED. */
int bz_azimuthal_mean(bz_ctx *ctx, const double *field, int z_face, double center_x, double center_y, double radius, int32_t Nr, int32_t m,
                      double *profile, int64_t *counts);
/* Tangential and radial wind about (center_x, center_y) at cell centres, from the velocity parent arrays u (x faces) and v (y faces) with
 * FILLED halos (the faces i + 1 = Nx and j + 1 = Ny are read):
 *     u^c = (u[i] + u[i + 1]) / 2,  v^c = (v[j] + v[j + 1]) / 2,  x = x^c[i] - center_x,  y = y^c[j] - center_y,  r = sqrt(x x + y y)
 *     tangential = (-y u^c + x v^c) / r,   radial = (x u^c + y v^c) / r
 * Either output (DEVICE centre parent arrays) may be NULL; only the interior is written (fill halos with bz_fill_halo_regions).  There is no
 * guard at r = 0: a cell centre that coincides with the centre gives NaN, as the reference's Field((-y u + x v) / r) does.  Asynchronous on
 * the context's stream.  Flat-y contexts return BZ_ERR_UNSUPPORTED. */
int bz_polar_winds(bz_ctx *ctx, const double *u, const double *v, double center_x, double center_y, double *tangential, double *radial);

/* ---- adiabatic initialisation (csrc/bz_adiabatic_balance.hip) ----
 * balance_adiabatically!(model; dt, cycles, weight) of the reference (src/AtmosphereModels/adiabatic_balance.jl:44-86), FV3's na_init: the
 * initial fields — every prognostic field but rho_w — are snapshotted as whole parent arrays; each of `cycles` cycles runs, for s = +1 and
 * then s = -1, time_step(s dt), time_step(-s dt), the nudge x <- (x + weight x0) / (1 + weight) of every initial field over its whole parent
 * array, the halo fills of the nudged fields and update_state! with tendencies.  rho_w is never snapshotted or nudged.
 *
 * bz_nudge_fields — nudge_initial_fields!: one launch blends `n` <= 16 DEVICE arrays fields[i] of count[i] elements each towards snapshots[i],
 * in the arrays' own precision; counts may differ (centre and z-face parents) and may be odd.  Asynchronous on the context's stream; any context.
 *
 * bz_balance_adiabatically_compressible / _anelastic — the whole loop behind one call, on the context it is given: the caller passes a
 * context WITHOUT sponge, microphysics, closure, forcings and surface fluxes (the excursions must be reversible), with the state made
 * consistent as before a first time step (compressible: bz_seed_time_averaged_velocities + bz_compressible_update_state(.., 1); anelastic:
 * bz_update_state(.., 1)).  Initial fields: rho_d, rho_u, rho_v, rho_theta [, rho_q] — anelastic: rho_u, rho_v, rho_theta [, rho_q] and the
 * user tracers; rho_q is left out of the list with nudge_moisture = 0; Kessler species are never nudged.  The snapshot memory is allocated
 * and freed by the call; everything between is enqueued on the context's stream without a host synchronisation, the steps are launched,
 * never replayed from a recorded graph, and nothing of the context's configuration changes (recorded steps stay valid).  The moisture scan
 * is not run: the steps treat the moisture as present (same bits).  Negative dt steps are the ordinary steps with the sign of dt carried
 * through: the substep count takes |dt| and the UpperSponge terms |dtau|.  BZ_ERR_INVALID: cycles < 1, dt zero or not finite, weight not
 * finite or <= -1.  BZ_ERR_UNSUPPORTED with bz_last_error naming the reason: y-slab, kinematic and walled (Bounded x / y) contexts. */
int bz_nudge_fields(bz_ctx *ctx, int32_t n, double *const *fields, const double *const *snapshots, const int64_t *count, double weight);
int bz_balance_adiabatically_compressible(bz_ctx *ctx, const bz_compressible_state *s, const bz_compressible_prognostic *U0,
                                          const bz_compressible_prognostic *G, const bz_acoustic_substepper *sub, double dt, int32_t cycles,
                                          double weight, int32_t nudge_moisture);
int bz_balance_adiabatically_anelastic(bz_ctx *ctx, const bz_state *s, const bz_prognostic *U0, const bz_prognostic *G, double dt,
                                       int32_t cycles, double weight, int32_t nudge_moisture);

/* ---- instrumentation (not part of the reference interface) ---- */
/* When enabled, every kernel group is bracketed by hipEvents on the ctx stream. */
int bz_profile_enable(bz_ctx *ctx, int on);
int bz_profile_reset(bz_ctx *ctx);
/* number of instrumented kernel groups; name/total milliseconds/launch count of group idx
 * (synchronises the stream). */
int bz_profile_count(bz_ctx *ctx);
int bz_profile_get(bz_ctx *ctx, int idx, const char **name, double *total_ms, int64_t *launches);
/* divergence of momentum, max-abs over the interior, into *out (host); diagnostic for tests
 * (test/anelastic_pressure_solver_nonhydrostatic.jl:45-46). Fills the momentum halos itself; non-finite momentum reports +Inf,
 * never a finite value (a NaN in any cell, or an infinite momentum, cannot pass an `assert div < tol`). Synchronises. */
int bz_max_abs_divergence(bz_ctx *ctx, const bz_state *s, double *out);

/* hipGraph replay of whole time steps (csrc/bz_graph.hip).  bz_time_step_anelastic / bz_time_step_compressible are pure functions of
 * (argument structs, dt, configuration); on launch-bound grids the second call with the same arguments records the step with stream
 * capture and later calls replay it with one hipGraphLaunch.  Opt-in (bz_graph_enable, or BZ_GRAPH=1 in the environment): measured gain
 * on MI355X is 0-5 % on launch-bound grids and recording costs ~1 ms, so it pays only with a fixed dt.  Inactive while profiling is
 * enabled and on contexts with a communicator.  The arrays named by the structs must stay where they are, as
 * Oceananigans fields do.  No reference counterpart. */
int bz_graph_enable(bz_ctx *ctx, int on);
int bz_graph_info(bz_ctx *ctx, int32_t *enabled, int64_t *captures, int64_t *replays);

#ifdef __cplusplus
}
#endif
#endif /* BREEZE_HIP_H */
