// bz_compressible.hip — CompressibleDynamics + SplitExplicitTimeDiscretization on gfx950:
// the Wicker-Skamarock RK3 outer loop with the linearised acoustic substep loop.
//
//   time_step! / acoustic_rk3_substep!     /root/reference/src/TimeSteppers/acoustic_runge_kutta_3.jl:172-319
//   compute_slow_*_tendencies!             /root/reference/src/TimeSteppers/acoustic_substep_helpers.jl:55-149
//   acoustic_rk3_substep_loop! and kernels /root/reference/src/CompressibleEquations/acoustic_substepping.jl:318-1590
//   update_state! (compressible)           /root/reference/src/AtmosphereModels/update_atmosphere_model_state.jl:41-68
//                                          /root/reference/src/CompressibleEquations/compressible_time_stepping.jl:83-242
//
// This file is the outer loop: bz_acoustic_substep_loop, bz_acoustic_rk3_substep and the whole step with its buffer rotation.  The rest:
//   bz_cmp_state.hip                update_state! (k_cmp_diagnose), the linearisation refresh, context creation, the Kessler update
//   bz_cmp_scalar.hip               slow tendencies: the 3-D-density scalar flux divergence (the WENO reconstructions of the model)
//   bz_acoustic.hip                 one stage of the substep loop in three pieces, walls / open boundaries, direct damping
//   bz_acoustic_kernels.h           its kernels (k_ac_*)
//   bz_compressible_internal.h      what these share: field bundles, the stage in flight, argument checks, launch-selection helpers
//
// Kernel structure of one acoustic substep (the reference launches 5 kernels + 8 halo fills per substep and moves
// ~58 words/cell; here 3 kernels, no halo fills, ~39 words/cell):
//   k_ac_horizontal        pointwise.  Klemp-2018 divergence damping of the PREVIOUS substep (it only needs the two
//                          (rho theta)' levels that are still in memory) followed by the explicit horizontal step of
//                          this substep; accumulates the time-averaged horizontal momentum.  Neighbours by periodic
//                          wrap indexing, so the perturbation fields never need halos inside the loop.
//   k_ac_column_forward    one thread per column marching upward: predictors rho'*, (rho theta)'* of cell k, right-hand
//                          side of face k, forward elimination of the tridiagonal system with the coefficients built on
//                          the fly from registers (the Thomas factors t_k are stored by the first substep of a stage and
//                          reused: they depend only on the linearisation and d tau).
//   k_ac_column_backward   one thread per column marching downward: back substitution for (rho w)', post-solve recovery
//                          of rho', (rho theta)', accumulation of the time-averaged vertical momentum.
// Stage prologue / epilogue are single pointwise kernels (k_ac_stage_init, k_ac_finalize, k_ac_recover) and the whole
// update_state! is k_cmp_diagnose, which also writes every periodic halo image and z-halo copy of what it produces.
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "bz_compressible_internal.h"

__global__ __launch_bounds__(256) void k_ws_rk3_scalar(DevGrid g, double *__restrict__ u, const double *__restrict__ u0,
                                                       const double *__restrict__ G, double dt_stage)
{
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long long)g.Ny * g.Sx) return;
    const int k = blockIdx.y;
    const long long n = g.Sxy * (k + g.Hz) + (long long)g.Hy * g.Sx + t;
    u[n] = u0[n] + dt_stage * G[n];
}

// acoustic_rk3_substep_loop!; moist: fold the WS-RK3 moisture update into the recovery kernel; velocities: finish with the
// halo fills + compute_velocities! of the reference (skipped when a full update_state! follows immediately).
static int bzi_acoustic_substep_loop(bz_ctx *ctx, const bz_compressible_state *s, const bz_compressible_prognostic *U0,
                                     const bz_compressible_prognostic *G, const bz_acoustic_substepper *sub, double dt,
                                     double beta, bool moist, bool velocities)
{
    int rc = bzi_acoustic_stage_begin(ctx, s, U0, G, sub, dt, beta);
    if (rc) return rc;
    const int ntau = stage_of(ctx).ntau;
    for (int sstep = 1; sstep <= ntau; ++sstep)
        if ((rc = bzi_acoustic_substep(ctx, s, U0, G, sub, sstep))) return rc;
    return bzi_acoustic_stage_end(ctx, s, U0, G, sub, dt, beta, moist, velocities);
}

// Walls in y: what acoustic_rk3_substep_loop! does after the loop's last kernel and bz_acoustic_substep_loop leaves to its caller there
// (acoustic_substepping.jl:1560-1587).  The fills of rho_d, rho theta, rho u, rho v, rho w with the model's conditions, compute_velocities! and
// the fills of u, v, w are one launch of k_cmp_diagnose<.., WY> (bzi_compressible_velocities, or the full update_state! that follows a stage
// of a whole step); left are the fills of the time-averaged velocities: no-flux rows for <u> and <w>, wall faces 0 and Ny for the y-face
// field <v> (the moisture tendency reads <v> of face Ny in the first upper halo row).
static int fill_walled_averages(bz_ctx *ctx, const bz_acoustic_substepper *sub)
{
    double *f[3] = {sub->time_averaged_u, sub->time_averaged_v, sub->time_averaged_w};
    const int kinds[3] = {0, BZ_HALO_YFACE, 1};
    return bzi_fill_halos_multi(ctx, f, kinds, 3);
}

extern "C" int bz_acoustic_substep_loop(bz_ctx *ctx, const bz_compressible_state *s, const bz_compressible_prognostic *U0,
                                        const bz_compressible_prognostic *G, const bz_acoustic_substepper *sub, double dt,
                                        double beta)
{
    BZ_REQUIRE_COMPRESSIBLE();
    int rc = check_loop_args(ctx, s, U0, G, sub);
    if (rc) return rc;
    if ((rc = require_no_slab(ctx, "bz_acoustic_substep_loop"))) return rc;
    // Bounded x / y: the loop ends with _recover_full_state!; the halo fills with the model's boundary conditions and compute_velocities! that
    // close the reference's function (acoustic_substepping.jl:1584-1587) are the caller's
    return bzi_acoustic_substep_loop(ctx, s, U0, G, sub, dt, beta, false, !ac_walls(ctx));
}

extern "C" int bz_acoustic_rk3_substep(bz_ctx *ctx, const bz_compressible_state *s, const bz_compressible_prognostic *U0,
                                       const bz_compressible_prognostic *G, const bz_acoustic_substepper *sub, double dt,
                                       double beta)
{
    BZ_REQUIRE_COMPRESSIBLE();
    BZ_REJECT_WALLS("bz_acoustic_rk3_substep");
    BZ_REJECT_Y_WALL_OPTIONS("bz_acoustic_rk3_substep");
    int rc = check_loop_args(ctx, s, U0, G, sub);
    if (rc) return rc;
    if ((rc = require_no_slab(ctx, "bz_acoustic_rk3_substep"))) return rc;
    rc = bz_refresh_linearization(ctx, s, sub);
    if (rc) return rc;
    rc = bz_compute_slow_tendencies(ctx, s, G);
    if (rc) return rc;
    // compute_flux_bc_tendencies! (acoustic_runge_kutta_3.jl:190-193): after the slow tendencies, which overwrite G, and before the loop
    if ((rc = bzi_cmp_surface_fluxes(ctx, s, G))) return rc;
    rc = bzi_acoustic_substep_loop(ctx, s, U0, G, sub, dt, beta, true, true);
    if (rc || !ctx->dg.bounded_y) return rc;
    return fill_walled_averages(ctx, sub);
}

// buffer rotation of the whole-step seam: the z-halo levels of the six prognostic fields (the step's kernels write the first one of the centre
// fields and none of rho w's; the deeper ones never), state arrays -> U0 arrays; blockIdx.y: level pair (below / above), blockIdx.z: field
// (5 = rho w, whose upper halo sits one level higher)
struct RotPtrs { double *dst[6]; const double *src[6]; };
__global__ __launch_bounds__(256) void k_copy_deep_zhalo(DevGrid g, RotPtrs R)
{
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= g.Sxy) return;
    const int h = (int)(blockIdx.y >> 1), f = blockIdx.z;
    const bool up = blockIdx.y & 1;
    const long long lev = up ? (long long)(g.Hz + g.Nz + h + (f == 5 ? 1 : 0)) : (long long)(g.Hz - 1 - h);
    R.dst[f][lev * g.Sxy + t] = R.src[f][lev * g.Sxy + t];
}

// store_initial_state! (prognostic fields incl. the Kessler species into timestepper.U0)
int bzi_compressible_store_initial_state(bz_ctx *ctx, const bz_compressible_state *s, const bz_compressible_prognostic *U0)
{
    const DevGrid &g = ctx->dg;
    ProfileScope ps(ctx, "store_initial_state");
    const size_t nc = (size_t)g.Sxy * (size_t)(g.Nz + 2 * g.Hz) * sizeof(double);
    const size_t nf = (size_t)g.Sxy * (size_t)(g.Nz + 1 + 2 * g.Hz) * sizeof(double);
    BZ_HIP(hipMemcpyAsync(U0->rho_d, s->rho_d, nc, hipMemcpyDeviceToDevice, ctx->stream));
    BZ_HIP(hipMemcpyAsync(U0->rho_u, s->rho_u, nc, hipMemcpyDeviceToDevice, ctx->stream));
    BZ_HIP(hipMemcpyAsync(U0->rho_v, s->rho_v, nc, hipMemcpyDeviceToDevice, ctx->stream));
    BZ_HIP(hipMemcpyAsync(U0->rho_w, s->rho_w, nf, hipMemcpyDeviceToDevice, ctx->stream));
    BZ_HIP(hipMemcpyAsync(U0->rho_theta, s->rho_theta, nc, hipMemcpyDeviceToDevice, ctx->stream));
    BZ_HIP(hipMemcpyAsync(U0->rho_q, s->rho_q, nc, hipMemcpyDeviceToDevice, ctx->stream));
    if (g.microphysics == 2) {
        const bz_kessler_model_fields &K = ctx->kessler;
        BZ_HIP(hipMemcpyAsync(K.U0_cloud_liquid_density, K.cloud_liquid_density, nc, hipMemcpyDeviceToDevice, ctx->stream));
        BZ_HIP(hipMemcpyAsync(K.U0_rain_density, K.rain_density, nc, hipMemcpyDeviceToDevice, ctx->stream));
    }
    return BZ_OK;
}

static int compressible_step_body(bz_ctx *ctx, const bz_compressible_state *s, const bz_compressible_prognostic *U0,
                                  const bz_compressible_prognostic *G, const bz_acoustic_substepper *sub, double dt)
{
    int rc;
    const DevGrid &g = ctx->dg;
    BZ_REJECT_WALLS("bz_time_step_compressible");
    // round 4: on single-device contexts the stage epilogue is one pass (k_ac_stage_end) and store_initial_state! rides on the first
    // stage's initialisation kernel (the state IS U0 there); BZ_NO_AC_END_FUSE=1 restores the separate passes
    const bool fuse_end = bzi_acoustic_stage_end_fusable(ctx);
    const bool store0 = fuse_end && ctx->ac_fused;
    // Round 6, buffer rotation (the anelastic lean seam's scheme, bz_step.hip: bzi_lean_stage): nothing is copied into U0.  The state arrays
    // stay intact as "U0" until the last writer of the step: stage 1 reads them as U^L and writes its recovered state into the U0 ARRAYS
    // (out of place: k_ac_stage_end writes rho_d with the other fields, no separate density pass), stages 2 and 3 run on those with
    // U0 := the state arrays, and stage 3's epilogue writes the final state back into the state arrays (a thread reads U0 only at its own
    // cell, before it writes it).  12 words of store_initial_state! and two density passes less per step; the U0 arrays are the time
    // stepper's scratch (as in the reference, where nothing reads U0 outside time_step!).  Kessler species keep their copies.
    const bool rotate = store0 && ctx->tune.ac_rotate;
    bz_compressible_state sB = *s;                 // the state with its six prognostic fields living in the U0 arrays
    bz_compressible_prognostic uS = *U0;           // "U0" = the state arrays
    if (rotate) {
        sB.rho_d = U0->rho_d; sB.rho_theta = U0->rho_theta; sB.rho_u = U0->rho_u; sB.rho_v = U0->rho_v; sB.rho_w = U0->rho_w; sB.rho_q = U0->rho_q;
        uS.rho_d = s->rho_d; uS.rho_theta = s->rho_theta; uS.rho_u = s->rho_u; uS.rho_v = s->rho_v; uS.rho_w = s->rho_w; uS.rho_q = s->rho_q;
        // z-halo levels the step's kernels do not write: the U0 arrays get the state's, once per step
        {
            ProfileScope ps(ctx, "store_initial_state");
            RotPtrs R;
            R.dst[0] = U0->rho_d; R.dst[1] = U0->rho_theta; R.dst[2] = U0->rho_u; R.dst[3] = U0->rho_v; R.dst[4] = U0->rho_q; R.dst[5] = U0->rho_w;
            R.src[0] = s->rho_d; R.src[1] = s->rho_theta; R.src[2] = s->rho_u; R.src[3] = s->rho_v; R.src[4] = s->rho_q; R.src[5] = s->rho_w;
            hipLaunchKernelGGL(k_copy_deep_zhalo, dim3((unsigned)((g.Sxy + 255) / 256), 2 * g.Hz, 6), dim3(256), 0, ctx->stream, g, R);
        }
    }
    if (store0) {
        if (g.microphysics == 2) {      // the species' U0 copies stay copies (k_ac_stage_init does not know them)
            const bz_kessler_model_fields &K = ctx->kessler;
            const size_t nc = (size_t)g.Sxy * (size_t)(g.Nz + 2 * g.Hz) * sizeof(double);
            ProfileScope ps(ctx, "store_initial_state");
            BZ_HIP(hipMemcpyAsync(K.U0_cloud_liquid_density, K.cloud_liquid_density, nc, hipMemcpyDeviceToDevice, ctx->stream));
            BZ_HIP(hipMemcpyAsync(K.U0_rain_density, K.rain_density, nc, hipMemcpyDeviceToDevice, ctx->stream));
        }
    } else if ((rc = bzi_compressible_store_initial_state(ctx, s, U0))) return rc;
    // freeze_linearization_state! (acoustic_substepping.jl:288-292): the linearisation of stage 1 (refreshed again by
    // prepare_acoustic_cache! from the same state).  Its second half, seed_time_averaged_velocities!, is deliberately not
    // issued here: nothing between this point and stage 1's substep loop reads the time-averaged velocities (the slow
    // rho theta tendency of stage 1 uses model.velocities, the stage-1 moisture tendency was built by the previous
    // update_state!), and the first substep of the loop assigns the three accumulators — the seed is
    // unobservable inside a whole step (tests/test_gpu_compressible.py::test_whole_step_matches_operator_sequence runs the
    // per-operator sequence WITH the seed against this seam).  Per-operator drivers call bz_seed_time_averaged_velocities.
    rc = bz_refresh_linearization(ctx, s, sub);
    if (rc) return rc;
    const double betas[3] = {1.0 / 3.0, 1.0 / 2.0, 1.0};
    const bz_compressible_state *s_step = s;
    const bz_compressible_prognostic *U0_step = U0;
    for (int st = 0; st < 3; ++st) {
        // rotation: stage 1 runs on the state arrays (U0 = the same arrays), stages 2 and 3 on the U0 arrays (U0 = the state arrays)
        const bz_compressible_state *s = (rotate && st > 0) ? &sB : s_step;
        const bz_compressible_prognostic *U0 = rotate ? &uS : U0_step;
        const bz_compressible_state *s_next = !rotate ? s : (st == 2 ? s_step : &sB);
        rc = bz_compute_slow_tendencies(ctx, s, G);
        if (rc) return rc;
        // compute_flux_bc_tendencies! (acoustic_runge_kutta_3.jl:190-193) on both stage paths: G_rho_u, G_rho_v, G_rho_theta are complete
        // before the stage's first sweeps fold the gradient of p^L into them, and G_rho_q — left by the previous update_state! (the diagnostics
        // u, v, theta, q of `s` do not rotate) — before the stage epilogue forms U0_rho_q + dt G_rho_q
        if ((rc = bzi_cmp_surface_fluxes(ctx, s, G))) return rc;
        if (!fuse_end) {
            rc = bzi_acoustic_substep_loop(ctx, s, U0, G, sub, dt, betas[st], true, false);
            if (rc) return rc;
            if (g.bounded_y && (rc = fill_walled_averages(ctx, sub))) return rc;      // walls in y take this unfused path (bzi_acoustic_stage_end_fusable)
            // update_state! (+ prepare_acoustic_cache! of the next stage: same inputs, folded into the diagnosis kernel)
            rc = bzi_compressible_update_state(ctx, s, G, sub, true, st < 2);
            if (rc) return rc;
            continue;
        }
        ctx->ac_skip_avg = st < 2;      // the averages of stages 1 and 2 feed only the (skipped) moisture tendency of a dry model
        ctx->ac_whole_step = true;
        ctx->ac_rotate = rotate;
        rc = bzi_acoustic_stage_begin(ctx, s, U0, G, sub, dt, betas[st], store0 && st == 0);
        ctx->ac_rotate = false;
        ctx->ac_skip_avg = false;
        ctx->ac_whole_step = false;
        if (rc) return rc;
        const int ntau = stage_of(ctx).ntau;
        for (int sstep = 1; sstep <= ntau; ++sstep)
            if ((rc = bzi_acoustic_substep(ctx, s, U0, G, sub, sstep))) return rc;
        if ((rc = bzi_acoustic_stage_end_fused(ctx, s, U0, G, sub, dt, betas[st], st < 2, s_next))) return rc;
        // compute_closure_fields! of the update_state! the fused epilogue stands for: a launch of its own after it (velocities, T, p and their
        // halos are final), on the arrays the next stage reads
        if ((ctx->has_closure || ctx->has_diffusivity) && (rc = bzi_cmp_closure_fields(ctx, s_next))) return rc;
        if ((rc = bz_compute_moisture_tendency(ctx, s_next, G, sub))) return rc;
    }
    s = s_step;
    if (g.microphysics == 2) return bz_compressible_kessler_update(ctx, s, G, sub, dt);     // microphysics_model_update! (:316)
    if (ctx->has_instant_precip) return bz_instantaneous_precipitation_update(ctx, s, G, sub, dt);      // the same slot (bz_instant_precip.hip)
    return BZ_OK;
}

// the step body for a caller that has checked the arguments and opens the call itself (bz_adiabatic_balance.hip): launched, never replayed,
// and without the moisture scan — the scan's word must say "unknown" (the stage kernels then skip nothing; same bits)
int bzi_compressible_step_launched(bz_ctx *ctx, const bz_compressible_state *s, const bz_compressible_prognostic *U0,
                                   const bz_compressible_prognostic *G, const bz_acoustic_substepper *sub, double dt)
{
    return compressible_step_body(ctx, s, U0, G, sub, dt);
}

extern "C" int bz_time_step_compressible(bz_ctx *ctx, const bz_compressible_state *s, const bz_compressible_prognostic *U0,
                                         const bz_compressible_prognostic *G, const bz_acoustic_substepper *sub, double dt)
{
    BZ_REQUIRE_COMPRESSIBLE();
    BZ_REJECT_WALLS("bz_time_step_compressible");
    BZ_REJECT_Y_WALL_OPTIONS("bz_time_step_compressible");
    int rc = check_loop_args(ctx, s, U0, G, sub);
    if (rc) return rc;
    if ((rc = bzi_scan_moisture_field(ctx, s->rho_q))) return rc;      // dry models: the moisture tendency kernels write exact zeros without reading
    if (ctx->slab_mode && ctx->comm) return bzi_dist_time_step_compressible(ctx, s, U0, G, sub, dt);     // bz_comm.hip owns the exchanges
    if ((rc = require_no_slab(ctx, "bz_time_step_compressible"))) return rc;
    // launch-bound grids replay the recorded step (bz_graph.hip); a failed recording has executed nothing and falls through
    const uint64_t key = bzi_graph_key(ctx, 2, dt, s, sizeof(*s), U0, sizeof(*U0), G, sizeof(*G), sub, sizeof(*sub));
    bool capture = false;
    if (bzi_graph_begin(ctx, key, &capture) == 1) return BZ_OK;
    if (capture) {
        rc = compressible_step_body(ctx, s, U0, G, sub, dt);
        if ((rc = bzi_graph_end(ctx, key, rc)) != -1) return rc;
    }
    return compressible_step_body(ctx, s, U0, G, sub, dt);
}
