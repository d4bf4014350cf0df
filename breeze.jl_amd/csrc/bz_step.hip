// bz_step.hip — host-side orchestration of the device-resident anelastic SSP-RK3 step.
//   update_state!  /root/reference/src/AtmosphereModels/update_atmosphere_model_state.jl:41-68
//   time_step!     /root/reference/src/TimeSteppers/ssp_runge_kutta_3.jl:209-278
// Everything is enqueued on ctx->stream; there is no host synchronisation inside a step.  One tier decision (bzi_anelastic_tier), one
// function per tier (step_lean, step_fused_rk, step_fused, step_operators), and the pieces the slab drivers of bz_comm.hip share.
#include <cstdlib>

#include "bz_internal.h"

extern "C" int bz_update_state(bz_ctx *ctx, const bz_state *s, const bz_prognostic *G, int compute_tendencies)
{
    if (!ctx || !s || (compute_tendencies && !G)) return BZ_ERR_INVALID;
    if (ctx->kinematic) return bzi_kinematic_update_state(ctx, s, G, compute_tendencies);      // compute_velocities! is a no-op there (bz_kinematic.hip)
    int rc;
    if (ctx->comm && (rc = bzi_comm_join_pending(ctx))) return rc;      // an undiagnosed last stage leaves its halo exchange on the side stream
    ctx->diagnostics_stale = false;
    if (ctx->d_qstate) BZ_HIP(hipMemsetAsync(ctx->d_qstate, 0, sizeof(int), ctx->stream));      // the moisture may have been set!: unknown (= moist) until the next scan
    bzi_moisture_unknown(ctx);
    if ((rc = bzi_fix_negative_moisture(ctx, s->rho_q))) return rc;      // fix_negative_moisture!(model)  (:42)
    // fill_halo_regions!(prognostic_fields(model))  (:48) — momentum halos are filled inside bz_compute_velocities (:135-136), the scalars here.
    double *sf[4] = {s->rho_theta, s->rho_q, ctx->dg.rqcl_field, ctx->dg.rqr_field};
    int sk[4] = {0, 0, 0, 0};
    if ((rc = bzi_fill_halos_multi(ctx, sf, sk, ctx->dg.microphysics == 2 ? 4 : 2))) return rc;
    // compute_auxiliary_variables!  (:207-223)
    if ((rc = bz_compute_velocities(ctx, s))) return rc;
    if ((rc = bz_compute_auxiliary_thermodynamic_variables(ctx, s))) return rc;
    // compute_tendencies!  (:63)
    if (compute_tendencies && (rc = bz_compute_tendencies(ctx, s, G))) return rc;
    return BZ_OK;
}

// ---- which tier a step takes -------------------------------------------------------------------------------------------------------
// The one statement of tier eligibility, for single-device contexts and for y-slab contexts with a communicator (bz_comm.hip).  Where the
// slab rule differs, the difference is a named condition; DESIGN §4 "which tier runs where" lists them.  (No walls on slabs: bzi_create.)
bz_tier bzi_anelastic_tier(const bz_ctx *ctx)
{
    const DevGrid &g = ctx->dg;
    const bool slab = ctx->slab_mode;
    // walls in y ((Periodic, Bounded, Bounded)) ride the lean seam too (WY kernels, wall rows in the projection kernels); the generic
    // order-7 / 9 kernels of the fused-RK tier are wall-aware, its LDS-tiled order-5 kernels are not
    const bool walls_lean = g.bounded_y && ctx->walls_lean_ok;
    const bool order5 = ctx->weno_R == 3 && ctx->scalar_R == 3;
    const bool theta_model = g.formulation == 0;
    const bool lean_switches = slab || (ctx->fuse_rk && ctx->lean);                       // slab: BZ_NO_LEAN / BZ_NO_FUSE_RK are not consulted
    const bool lean_anelastic = slab || !ctx->compressible;                               // slab: the context's model is not looked at
    const bool lean_forcings = !ctx->has_forcings || (!slab && bzi_lean_forcings_ok(ctx));      // slab: every forcing stack is refused
    const bool rk_orders = slab ? order5                                                  // slab: order 5 only
                                : ctx->scalar_R == ctx->weno_R && (ctx->weno_R == 3 || ctx->n_tracers == 0);
    const bool rk_forcings = slab || !(ctx->has_forcings && ctx->tune.no_fuse_forcing);   // slab: BZ_NO_FUSE_FORCING is not consulted
    const bool fused_tier = !slab;                                                        // slab: no fused tier, operators instead
    // lean seam: dry / vapour WENO5 theta model without closure (SmagorinskyLilly or a ScalarDiffusivity), bulk fluxes, relaxation, tracers, microphysics
    if ((ctx->fused_ok || walls_lean) && lean_switches && order5 && lean_anelastic && theta_model && g.microphysics == 0 && lean_forcings &&
        !ctx->has_bulk && !ctx->has_closure && !ctx->has_diffusivity && !ctx->has_relaxation && ctx->n_tracers == 0 && !ctx->bounded_mask &&
        (long long)g.Sxy * (g.Nz + 2 * g.Hz + 1) < (1LL << 32))
        return BZ_TIER_LEAN;
    if ((ctx->fused_ok || (walls_lean && ctx->weno_R != 3)) && ctx->fuse_rk && rk_orders && theta_model && g.microphysics != 2 &&
        !ctx->bounded_mask && !ctx->has_relaxation && rk_forcings)
        return BZ_TIER_FUSED_RK;
    return ctx->fused_ok && fused_tier ? BZ_TIER_FUSED : BZ_TIER_OPERATORS;
}

// ---- pieces shared with the slab drivers (bz_comm.hip) and the per-operator entry points (bz_slab.hip) -------------------------------
// the wall faces of the predictor rho w in the G slots stay 0 — and, for the lean seam, those of the projected momentum of stages 1-2 (U0)
int bzi_zero_wall_faces(bz_ctx *ctx, const bz_prognostic *G, const bz_prognostic *U0)
{
    const DevGrid &g = ctx->dg;
    for (const long long face : {g.Sxy * g.Hz, g.Sxy * (g.Hz + g.Nz)})
        BZ_HIP(hipMemsetAsync(G->rho_w + face, 0, g.Sxy * sizeof(double), ctx->stream));
    return U0 ? bzi_zero_wall_faces(ctx, U0, nullptr) : BZ_OK;
}

// The scalar-pair kernel feeds nothing of the pressure solve: it runs on the side stream beside the source term, the transforms and the Thomas
// solve (issue-bound stencil kernel next to bandwidth-bound streaming kernels); it joins before the projection (z-halo images of rho theta / rho q)
int bzi_scalar_pair_fork(bz_ctx *ctx, const LeanStage &L, const bz_prognostic *G, double dt, double alpha, bool first)
{
    BZ_HIP(hipEventRecord(ctx->ev_fork, ctx->stream));
    BZ_HIP(hipStreamWaitEvent(ctx->side_stream, ctx->ev_fork, 0));
    hipStream_t keep = ctx->stream;
    ctx->stream = ctx->side_stream;
    const int rc = bzi_lean_tendencies(ctx, L, G, dt, alpha, first, 0, 2);
    ctx->stream = keep;
    if (rc) return rc;
    BZ_HIP(hipEventRecord(ctx->ev_join, ctx->side_stream));
    return BZ_OK;
}

int bzi_scalar_pair_join(bz_ctx *ctx) { BZ_HIP(hipStreamWaitEvent(ctx->stream, ctx->ev_join, 0)); return BZ_OK; }

// The physics beside the fused-RK kernels of a stage: evaluated from the still-intact previous-stage state and added, weighted alpha dt, to what
// the fused RK update just wrote (G slots, rho theta / rho q in place).  fold: the stack's momentum terms went into the momentum kernels' epilogues
int bzi_fused_rk_physics(bz_ctx *ctx, const bz_state *s, const bz_prognostic *G, double dt, double alpha, bool first, bool fold)
{
    int rc;
    if (ctx->n_tracers) {       // tracers ride beside the fused kernels: tendency from the previous-stage state, RK in place
        if ((rc = bzi_tracer_tendencies(ctx, s))) return rc;
        if ((rc = bzi_tracer_rk3(ctx, dt, alpha, first))) return rc;
    }
    if (ctx->has_closure && (rc = bzi_apply_closure(ctx, s, G->rho_u, G->rho_v, G->rho_w, s->rho_theta, s->rho_q, alpha * dt))) return rc;
    if (ctx->has_diffusivity && (rc = bzi_apply_diffusivity(ctx, s, G->rho_u, G->rho_v, G->rho_w, s->rho_theta, s->rho_q, alpha * dt))) return rc;
    if (ctx->has_forcings && (rc = bzi_apply_forcings(ctx, s, G->rho_u, G->rho_v, s->rho_theta, s->rho_q, alpha * dt, fold))) return rc;
    if ((ctx->has_forcings || ctx->has_bulk) && (rc = bzi_flux_bc(ctx, s, G->rho_u, G->rho_v, s->rho_theta, s->rho_q, alpha * dt))) return rc;
    return BZ_OK;
}

// host-side bookkeeping at the end of a lean step (single-device and slab drivers): where the ping-pong pair sits now
void bzi_lean_step_done(bz_ctx *ctx, bool diagnosed)
{
    ctx->lean_step_last = true;
    ctx->G_is_predictor = true;
    ctx->diagnostics_stale = !diagnosed;
}

// Buffer rotation of the lean seam (round 4).  Three sets of prognostic arrays take part: A = the state `s`, B = the G slots,
// C = the U0 slots.  Nothing is ever copied into U0 (store_initial_state!, ssp_runge_kutta_3.jl:180-186, has no pass and no store
// of its own): the state arrays stay intact as "U0" until the last writer of the step.
//   momentum   tendency + RK kernels: stencils from A (stage 1) / C (stages 2, 3), u0 from A, predictor -> B;
//              projection: B -> C (stages 1, 2), B -> A (stage 3, when nothing reads A any more)
//   scalars    stage 1: A -> B;  stage 2: stencils from B, u0 from A -> C;  stage 3: stencils from C, u0 from A -> A in place
//              (a thread reads A only at its own cell, before it writes it)
// so every step ends with the whole prognostic state in `s`, diagnosed or not.  The U0 arrays are the time stepper's scratch
// (as in the reference, where nothing reads U0 outside time_step!).
void bzi_lean_stage(const bz_state *s, const bz_prognostic *U0, const bz_prognostic *G, int stage, LeanStage *L)
{
    L->sin = *s; L->sout = *s;
    if (stage > 0) { L->sin.rho_u = U0->rho_u; L->sin.rho_v = U0->rho_v; L->sin.rho_w = U0->rho_w; }
    if (stage < 2) { L->sout.rho_u = U0->rho_u; L->sout.rho_v = U0->rho_v; L->sout.rho_w = U0->rho_w; }
    L->u0.rho_u = s->rho_u; L->u0.rho_v = s->rho_v; L->u0.rho_w = s->rho_w; L->u0.rho_theta = s->rho_theta; L->u0.rho_q = s->rho_q;
    L->pa = stage == 0 ? s->rho_theta : stage == 1 ? G->rho_theta : U0->rho_theta;
    L->pb = stage == 0 ? s->rho_q : stage == 1 ? G->rho_q : U0->rho_q;
    L->oa = stage == 0 ? G->rho_theta : stage == 1 ? U0->rho_theta : s->rho_theta;
    L->ob = stage == 0 ? G->rho_q : stage == 1 ? U0->rho_q : s->rho_q;
}

// Lean tier.  full: projection + diagnosis into `s` (the last stage of a diagnosed step); else the momentum-only projection
static int lean_project(bz_ctx *ctx, const bz_state *s, const LeanStage &L, const bz_prognostic *G, double adt, bool full)
{
    return full ? bzi_project_diagnose(ctx, s, adt, nullptr, nullptr, G, true, L.oa, L.ob) : bzi_project_lean(ctx, &L.sout, adt, nullptr, nullptr, G, L.oa, L.ob);
}

// Pressure solve from the predictor in the G slots and the projection of a lean stage: the hand-written x transforms or the library's 2-D plans
static int lean_solve_and_project(bz_ctx *ctx, const bz_state *s, const LeanStage &L, const bz_prognostic *G, double adt, bool full)
{
    int rc = BZ_OK;
    if (ctx->xf) {
        // hand-written x transforms (bz_xfft_kernels.h): the source term is evaluated inside the forward x pass; y transforms
        // (contiguous) and vertical solves on the transposed spectrum
        {
            ProfileScope ps(ctx, "poisson_source_term+fft_x");
            if ((rc = bzi_xf_forward(ctx, s, adt, G))) return rc;
        }
        if ((rc = bzi_xf_middle(ctx))) return rc;
        ProfileScope ps(ctx, "poisson_fft_x_inverse");
        if ((rc = bzi_xf_inverse(ctx))) return rc;
    } else {
        if ((rc = bzi_poisson_source_fused(ctx, s, adt, nullptr, G))) return rc;
        if ((rc = bzi_poisson_spectral(ctx))) return rc;
    }
    return lean_project(ctx, s, L, G, adt, full);
}

// Lean seam (bz_tendency5_kernels.h): the tendency kernels read the prognostic fields only and derive u, v, w, theta, q^v, T on the
// fly (bit-identical to the stored diagnostics), rho theta / rho q ping-pong between their own arrays and the G slots, the projection
// of stages 1-2 writes momentum only; stage 3 of a diagnosed step runs the full projection + diagnosis kernel, so on return every
// field of `s` (halos included) is what the per-operator sequence leaves.
static int step_lean(bz_ctx *ctx, const bz_state *s, const bz_prognostic *U0, const bz_prognostic *G, double dt, bool diagnose)
{
    int rc;
    if ((rc = bzi_zero_wall_faces(ctx, G, U0))) return rc;
    for (int stage = 0; stage < 3; ++stage) {
        const double alpha = BZ_SSP_RK3_ALPHA[stage];
        LeanStage L;
        bzi_lean_stage(s, U0, G, stage, &L);
        if ((rc = bzi_lean_tendencies(ctx, L, G, dt, alpha, stage == 0, 0, 3))) return rc;
        // the bottom fluxes of the stage (bzi_lean_forcings_ok), evaluated from the intact previous-stage momentum and added, weighted alpha dt, to
        // what the fused RK updates just wrote: the predictor momentum in the G slots and rho theta / rho q in the stage's output buffers (the Coriolis /
        // profile terms went into the RK epilogues: Lean5::mforce, bz_tendency5.hip; T is no stored field here: the next stage derives it from oa, ob)
        if (ctx->has_forcings && (rc = bzi_flux_bc(ctx, &L.sin, G->rho_u, G->rho_v, L.oa, L.ob, alpha * dt))) return rc;
        if ((rc = lean_solve_and_project(ctx, s, L, G, alpha * dt, diagnose && stage == 2))) return rc;
    }
    bzi_lean_step_done(ctx, diagnose);
    return BZ_OK;
}

// Fused-RK tier: tendencies and the following RK update in one pass (bz_tendency.hip: bzi_tendencies_fused_rk).  The tendency of stage s is
// evaluated where the reference applies it (at the start of stage s, from the state left by stage s-1), the predictor momentum goes to the G arrays
// and is projected from there into the state arrays, rho_theta / rho_q advance in place.  G never makes the round trip through HBM.
// lsum_in: the level sums the previous step of this call left are fresh (one_anelastic_step).
static int step_fused_rk(bz_ctx *ctx, const bz_state *s, const bz_prognostic *U0, const bz_prognostic *G, double dt, bool lsum_in)
{
    int rc;
    if ((rc = bzi_zero_wall_faces(ctx, G))) return rc;
    // momentum terms of the forcing stack in the epilogues of the stored-velocity momentum kernels (round 5): the stage's subsidence
    // profiles are built first (from the stored u, v, theta, q of the stage start, which the tendency kernels do not touch)
    const bool fold = ctx->has_forcings && ctx->weno_R == 3 && bzi_k6_stored_ok(ctx) && ctx->tiled_tendencies && !ctx->tune.no_fuse_forcing && !ctx->tune.no_fold_forcing;
    for (int stage = 0; stage < 3; ++stage) {
        const double alpha = BZ_SSP_RK3_ALPHA[stage];
        if (stage == 0) ctx->lsum_fresh = lsum_in;
        if (fold && (rc = bzi_compute_forcings(ctx, s))) return rc;
        ctx->fold_momentum_forcing = fold;
        rc = bzi_tendencies_fused_rk(ctx, s, U0, G, dt, alpha, stage == 0);
        ctx->fold_momentum_forcing = false;
        if (rc) return rc;
        if ((rc = bzi_fused_rk_physics(ctx, s, G, dt, alpha, stage == 0, fold))) return rc;
        // implicit_step! of the stage (:124-161): the predictor momentum in the G slots, the scalars in place
        if ((rc = bzi_implicit_step(ctx, G->rho_u, G->rho_v, G->rho_w, s->rho_theta, s->rho_q, alpha * dt))) return rc;
        if (ctx->dg.bounded_y && (rc = bzi_fill_halo(ctx, G->rho_v, BZ_HALO_YFACE))) return rc;      // wall faces j = 0, Ny of the predictor (the source term reads face Ny)
        if ((rc = bzi_poisson_from_momentum(ctx, s, alpha * dt, G))) return rc;
        // pressure_anomaly is a diagnostic nobody reads inside the step: only the last stage scatters it
        // (the horizontal sums of the u, v, theta, q it stores ride along: the next stage's subsidence profiles, bz_forcing.hip)
        const bool ride = bzi_level_sums_ride(ctx) && ctx->d_lsum_rows;
        // fix_negative_moisture! of the stage's update_state! (:42): the RK update wrote rho q in place, the projection touches momentum only
        if ((rc = bzi_fix_negative_moisture(ctx, s->rho_q))) return rc;
        if ((rc = bzi_project_diagnose(ctx, s, alpha * dt, nullptr, nullptr, G, stage == 2, nullptr, nullptr, ride))) return rc;
        ctx->lsum_fresh = ride;
        if ((rc = bzi_tracer_specific(ctx))) return rc;
        if ((rc = bzi_surface_layer_stage(ctx, s, stage, dt))) return rc;      // update_boundary_conditions! of the stage's update_state!
    }
    ctx->lsum_step_last = ctx->lsum_fresh;
    ctx->G_is_predictor = true;
    return BZ_OK;
}

// Fused tier: same arithmetic as the operators, fewer passes over HBM (bz_fused.hip): store_initial_state! rides on the first RK update, the source
// term uses wrap indexing instead of a halo fill, and the projection, velocity / thermodynamic diagnosis and every halo fill of
// update_state! are one kernel.
static int step_fused(bz_ctx *ctx, const bz_state *s, const bz_prognostic *U0, const bz_prognostic *G, double dt)
{
    int rc;
    if (ctx->G_is_predictor && (rc = bz_compute_tendencies(ctx, s, G))) return rc;
    for (int stage = 0; stage < 3; ++stage) {
        const double alpha = BZ_SSP_RK3_ALPHA[stage];
        if ((rc = bz_compute_flux_bc_tendencies(ctx, s, G))) return rc;          // :229,243,257
        if ((rc = bzi_rk3_fused(ctx, s, U0, G, dt, alpha, stage == 0))) return rc;
        if (ctx->dg.microphysics == 2 && (rc = bzi_kessler_rk3(ctx, dt, alpha, stage == 0))) return rc;
        if ((rc = bzi_tracer_rk3(ctx, dt, alpha, stage == 0))) return rc;
        if ((rc = bz_implicit_step(ctx, s, alpha * dt))) return rc;
        if ((rc = bzi_poisson_from_momentum(ctx, s, alpha * dt, nullptr))) return rc;
        if ((rc = bzi_fix_negative_moisture(ctx, s->rho_q))) return rc;      // fix_negative_moisture! of the stage's update_state! (:42)
        if ((rc = bzi_project_diagnose(ctx, s, alpha * dt))) return rc;
        if ((rc = bzi_tracer_specific(ctx))) return rc;
        if ((rc = bzi_surface_layer_stage(ctx, s, stage, dt))) return rc;
        if ((rc = bz_compute_tendencies(ctx, s, G))) return rc;
    }
    // microphysics_model_update!(model.microphysics, model) closes the step (ssp_runge_kutta_3.jl:262-263)
    if (ctx->dg.microphysics == 2 && (rc = bzi_kessler_update(ctx, s, G, dt))) return rc;
    return BZ_OK;
}

// Operators tier: the reference's own call order
static int step_operators(bz_ctx *ctx, const bz_state *s, const bz_prognostic *U0, const bz_prognostic *G, double dt)
{
    int rc;
    if (ctx->G_is_predictor && (rc = bz_compute_tendencies(ctx, s, G))) return rc;
    if ((rc = bz_store_initial_state(ctx, s, U0))) return rc;               // :223
    for (int stage = 0; stage < 3; ++stage) {
        const double alpha = BZ_SSP_RK3_ALPHA[stage];
        if ((rc = bz_compute_flux_bc_tendencies(ctx, s, G))) return rc;              // :229,243,257
        if ((rc = bz_ssp_rk3_substep(ctx, s, U0, G, dt, alpha))) return rc;          // :230,244,258
        if ((rc = bz_implicit_step(ctx, s, alpha * dt))) return rc;                  // :124-161 (a no-op without a vertically implicit closure)
        if ((rc = bz_compute_pressure_correction(ctx, s, alpha * dt))) return rc;    // :232,246,260
        if ((rc = bz_make_pressure_correction(ctx, s, alpha * dt))) return rc;       // :233,247,261
        if ((rc = bz_update_state(ctx, s, G, 1))) return rc;                         // :236,250,270
        if ((rc = bzi_surface_layer_stage(ctx, s, stage, dt))) return rc;
    }
    if (ctx->dg.microphysics == 2 && (rc = bzi_kessler_update(ctx, s, G, dt))) return rc;
    return BZ_OK;
}

// One step on a single-device context.  A hipGraph records this body (one_anelastic_step): nothing below allocates or synchronises,
// and G_is_predictor, lean_step_last, lsum_step_last are what the recording saves after it (bz_graph.hip).
static int anelastic_step_body(bz_ctx *ctx, bz_tier tier, const bz_state *s, const bz_prognostic *U0, const bz_prognostic *G, double dt, bool diagnose)
{
    ctx->lean_step_last = false;
    ctx->lsum_step_last = false;
    const bool lsum_in = ctx->lsum_fresh;      // every tier but the fused-RK one leaves no sums behind
    ctx->lsum_fresh = false;
    if (tier == BZ_TIER_LEAN) return step_lean(ctx, s, U0, G, dt, diagnose);
    if (tier == BZ_TIER_FUSED_RK) return step_fused_rk(ctx, s, U0, G, dt, lsum_in);
    if (tier == BZ_TIER_FUSED) return step_fused(ctx, s, U0, G, dt);
    return step_operators(ctx, s, U0, G, dt);
}

static int one_anelastic_step(bz_ctx *ctx, const bz_state *s, const bz_prognostic *U0, const bz_prognostic *G, double dt, bool diagnose)
{
    if (ctx->slab_mode) {
        if (ctx->comm) return bzi_dist_time_step(ctx, s, U0, G, dt, diagnose);      // the library owns the exchanges (bz_comm.hip)
        ctx->last_error = "bz_time_step_anelastic: a y-slab context needs a communicator (bz_comm_init_rccl / bz_comm_init_local) "
                          "or a host-side distributed driver";
        return BZ_ERR_UNSUPPORTED;
    }
    const bz_tier tier = bzi_anelastic_tier(ctx);
    // the tiers other than the lean seam start from the stored diagnostics: if undiagnosed lean steps came before (the configuration
    // changed in between), rebuild them — here, outside the region a graph records (a rebuild baked into a recorded step would run, and
    // reset the moisture scan's word, on every replay)
    if (ctx->diagnostics_stale && tier != BZ_TIER_LEAN) { const int rcs = bz_update_state(ctx, s, G, 0); if (rcs) return rcs; }
    // launch-bound grids replay the recorded step (bz_graph.hip); a failed recording has executed nothing and falls through
    // (the host's view of the moisture scan selects the kernels a recording holds; so does the source of the first stage's level sums)
    const int kind = 1 + (diagnose ? 0 : 16) + 32 * ctx->q_host + (ctx->lsum_fresh ? 128 : 0);
    const uint64_t key = bzi_graph_key(ctx, kind, dt, s, sizeof(*s), U0, sizeof(*U0), G, sizeof(*G), nullptr, 0);
    bool capture = false;
    int rc;
    if (bzi_graph_begin(ctx, key, &capture) == 1) {
        if (ctx->lean_step_last) ctx->diagnostics_stale = !diagnose;      // the host-side bookkeeping of the recorded body
        ctx->lsum_fresh = ctx->lsum_step_last;
        return BZ_OK;
    }
    const bool lsum_in = ctx->lsum_fresh;
    if (capture) {
        rc = anelastic_step_body(ctx, tier, s, U0, G, dt, diagnose);
        if ((rc = bzi_graph_end(ctx, key, rc)) != -1) return rc;
        ctx->lsum_fresh = lsum_in;      // nothing ran
    }
    return anelastic_step_body(ctx, tier, s, U0, G, dt, diagnose);
}

// The level sums of SubsidenceForcing ride on the projection + diagnosis kernel (bz_fused.hip) from one stage to the next INSIDE a call;
// the first stage of a call takes them from its own pass (the host may have written the fields), and nothing is trusted after it.
static void level_sums_open(bz_ctx *ctx)
{
    ctx->lsum_fresh = false;
    long long P;
    (void)bzi_level_sum_rows(ctx, &P);      // allocated here: not inside a region a graph records
}

// initialize!(model) of a filtered surface state that nobody initialised or set: before the first step, outside any recorded region
static int surface_layer_first_step(bz_ctx *ctx, const bz_state *s)
{
    if (!ctx->sl_on || !ctx->sl.filtered || ctx->sl_initialized) return BZ_OK;
    return bz_surface_layer_initialize(ctx, s);
}

// A sequence of steps of a caller that opens the call itself (bz_adiabatic_balance.hip).  open: what bz_time_step_anelastic does before its
// step, with the moisture scan's word put to "unknown" instead of a scan (the kernels then skip nothing: same bits, and no read-back);
// launched: one step that is never replayed from, or recorded into, a graph of the context.
int bzi_anelastic_steps_open(bz_ctx *ctx, const bz_state *s)
{
    level_sums_open(ctx);
    if (ctx->d_qstate) BZ_HIP(hipMemsetAsync(ctx->d_qstate, 0, sizeof(int), ctx->stream));
    bzi_moisture_unknown(ctx);
    return surface_layer_first_step(ctx, s);
}

int bzi_anelastic_step_launched(bz_ctx *ctx, const bz_state *s, const bz_prognostic *U0, const bz_prognostic *G, double dt)
{
    const int mode = ctx->graph_mode;
    ctx->graph_mode = 0;
    const int rc = one_anelastic_step(ctx, s, U0, G, dt, true);
    ctx->graph_mode = mode;
    ctx->lsum_fresh = false;
    return rc;
}

extern "C" int bz_time_step_anelastic(bz_ctx *ctx, const bz_state *s, const bz_prognostic *U0, const bz_prognostic *G, double dt)
{
    if (!ctx || !s || !U0 || !G) return BZ_ERR_INVALID;
    BZ_REJECT_KINEMATIC(ctx, "bz_time_step_anelastic");
    level_sums_open(ctx);
    int rc = bzi_scan_moisture(ctx, s);
    if (!rc) rc = surface_layer_first_step(ctx, s);
    if (!rc) rc = one_anelastic_step(ctx, s, U0, G, dt, true);
    ctx->lsum_fresh = false;
    return rc;
}

// n steps of time_step!(model, dt) in one call — the loop of the reference's benchmark driver, many_time_steps!
// (/root/reference/benchmarking/src/timestepping.jl:11-16) and of run!(simulation) between two callback / output iterations: nothing
// reads model.velocities, theta, q^v, T or the pressure anomaly in between, and the lean tendency kernels derive what they need from the
// prognostic fields.  So every step but (optionally) the last ends its third stage with the momentum-only projection instead of the
// projection + diagnosis pass (13 words per cell written for host consumers only).  diagnose_last != 0: on return every field and halo
// of `s` carries the bits n calls of bz_time_step_anelastic leave.  diagnose_last == 0: the prognostic fields of `s` are current, the
// diagnostics are stale until bz_update_state(ctx, s, G, 0) — which bz_time_step(s)_anelastic do NOT need: stepping can simply go
// on.  Tiers other than the lean seam diagnose every step.
extern "C" int bz_time_steps_anelastic(bz_ctx *ctx, const bz_state *s, const bz_prognostic *U0, const bz_prognostic *G, double dt, int n,
                                       int diagnose_last)
{
    if (!ctx || !s || !U0 || !G || n < 0) return BZ_ERR_INVALID;
    BZ_REJECT_KINEMATIC(ctx, "bz_time_steps_anelastic");
    level_sums_open(ctx);
    if (n > 0) { const int rc = bzi_scan_moisture(ctx, s); if (rc) return rc; }
    if (n > 0) { const int rc = surface_layer_first_step(ctx, s); if (rc) return rc; }
    for (int it = 0; it < n; ++it) {
        const int rc = one_anelastic_step(ctx, s, U0, G, dt, it == n - 1 && diagnose_last);
        if (rc) { ctx->lsum_fresh = false; return rc; }
    }
    ctx->lsum_fresh = false;
    return BZ_OK;
}

int bzi_refresh_diagnostics(bz_ctx *ctx, const bz_state *s, const char *who)
{
    if (!ctx->diagnostics_stale) return BZ_OK;
    if (!s) {
        ctx->last_error = std::string(who) + ": the diagnostics are stale (bz_time_steps_anelastic ended without the last diagnosis); call bz_update_state first";
        return BZ_ERR_INVALID;
    }
    if (ctx->comm) return bz_comm_update_state_and_project(ctx, s, nullptr, 1.0, 0);
    return bz_update_state(ctx, s, nullptr, 0);
}

extern "C" int bz_diagnostics_stale(const bz_ctx *ctx) { return ctx ? (ctx->diagnostics_stale ? 1 : 0) : BZ_ERR_INVALID; }
