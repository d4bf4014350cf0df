// bz_kinematic.hip — AtmosphereModel(dynamics = PrescribedDynamics(reference_state)): the kinematic driver.
//   PrescribedDynamics, PrescribedDensity                   /root/reference/src/KinematicDriver/prescribed_dynamics.jl:27-84
//   compute_velocities!, pressure correction: no-ops        /root/reference/src/KinematicDriver/kinematic_driver_time_stepping.jl:16-49
//   div_rhoU, c_div_rhoU                                    /root/reference/src/KinematicDriver/kinematic_driver_time_stepping.jl:55-73
//   scalar_tendency = -div_rhoUc + c_div_rhoU               /root/reference/src/AtmosphereModels/dynamics_kernel_functions.jl:132-159,
//                                                           /root/reference/src/PotentialTemperatureFormulations/potential_temperature_tendency.jl:66-106
//   time_step! (SSP-RK3; the projection calls do nothing)   /root/reference/src/TimeSteppers/ssp_runge_kutta_3.jl:209-278
// The velocities u, v, w are given (ordinary halo-filled fields the host sets), density and pressure are the reference state's, and only
// the scalars rho theta, rho q and the user tracers advance.  A stage is ONE launch of k_kin_scalar_stage over all scalars — it reads the
// specific fields c the previous update_state! diagnosed and halo-filled and writes the densities rho c, so it never reads what it writes —
// followed by update_state! without the velocity computation (halo fill, k_thermo, tracer_density_to_specific!: the kernels of the anelastic
// model, bz_state.hip / bz_tracers.hip).  No step writes u, v or w.
//
// Kernel shape: k_scalar_tendency's (bz_tendency.hip) — a block owns a 64 x 4 tile of columns and marches upward through a chunk of levels,
// six-value vertical ring and the carried lower-face flux in registers per scalar, horizontal stencils through the L1 — with up to
// KIN_GROUP scalars marched side by side: u, v, w at the cell's six faces and D are loaded once per level and reused by every scalar of the
// group.  The arithmetic of -div_rhoUc is k_scalar_tendency's, operation for operation.
#include "bz_internal.h"
#include "bz_weno.h"

#define KTX 64
#define KTY 4
#define KIN_GROUP 4
#define KIN_MAX_SCALARS (2 + BZ_MAX_TRACERS)

struct KinScalars {
    int n;
    const double *c[KIN_MAX_SCALARS];      // specific fields (halo-filled)
    double *rc[KIN_MAX_SCALARS];           // densities rho c: read and written at the thread's own cell (MODE 1, 2)
    double *u0[KIN_MAX_SCALARS];           // step-start densities: written in MODE 1 (store_initial_state!), read in MODE 2
    double *G[KIN_MAX_SCALARS];            // tendencies (MODE 0)
};

// D = div_rhoU at cell centres (kinematic_driver_time_stepping.jl:55-73) with the face areas of the flux divergence it corrects, in the
// reference's order: interpolate rho, times the velocity, times the area, difference, times 1 / V.  rho is a column, so Ix(rho) = Iy(rho) =
// rho[k] exactly and Iz(rho) at face k is the tabulated rho_f[k].  w is multiplied as stored: the host keeps zeros on the wall faces.
__global__ __launch_bounds__(KTX *KTY) void k_kin_mass_divergence(DevGrid g, double *__restrict__ D, const double *__restrict__ u,
                                                                 const double *__restrict__ v, const double *__restrict__ w)
{
    const int i = blockIdx.x * KTX + threadIdx.x, j = blockIdx.y * KTY + threadIdx.y, k = blockIdx.z;
    if (i >= g.Nx || j >= g.Ny) return;
    const long long n = g.idx(i, j, k);
    const double rho = g.rho[k], Ax = g.Ax[k], Ay = g.Ay[k], Az = g.Az;
    const double dx = Ax * (rho * u[n + 1]) - Ax * (rho * u[n]);
    const double dy = g.flat_y ? 0.0 : Ay * (rho * v[n + g.Sx]) - Ay * (rho * v[n]);
    const double dz = Az * (g.rho_f[k + 1] * w[n + g.Sxy]) - Az * (g.rho_f[k] * w[n]);
    D[n] = g.Vinv_c[k] * (dx + dy + dz);
}

__device__ __forceinline__ double kin_flux_z(const DevGrid &g, double wt, double m3, double m2, double m1, double p0, double p1, double p2,
                                             int kface)
{
    const double cR = bz_upB(m3, m2, m1, p0, p1, p2, wt > 0.0, bz_buffer_face(kface, g.Nz));
    return g.rho_f[kface] * ((g.Az * wt) * cR);
}

// All scalars of the model through one RK stage.  blockIdx.z = level chunk + nchunks * scalar group.
//   MODE 0: G <- tendency;  1: first stage, u0 <- rho c, rho c <- (1 - alpha) u0 + alpha (rho c + dt G);  2: later stages (reads u0)
//   (the RKEpilogue semantics of bzi_tendencies_fused_rk, ssp_runge_kutta_3.jl:167-186).  CORR: G = -div_rhoUc + c D.
template <int MODE, bool CORR>
__global__ __launch_bounds__(KTX *KTY) void k_kin_scalar_stage(DevGrid g, KinScalars P, const double *__restrict__ u,
                                                              const double *__restrict__ v, const double *__restrict__ w,
                                                              const double *__restrict__ D, int kchunk, int nchunks, double dt, double alpha)
{
    const int i = blockIdx.x * KTX + threadIdx.x, j = blockIdx.y * KTY + threadIdx.y;
    if (i >= g.Nx || j >= g.Ny) return;
    const int grp = blockIdx.z / nchunks, chunk = blockIdx.z - grp * nchunks;
    const int s0 = grp * KIN_GROUP, ns = min(KIN_GROUP, P.n - s0);      // block-uniform: the guards below are scalar branches
    const int k0 = chunk * kchunk, k1 = min(k0 + kchunk, g.Nz);
    const long long sy = g.Sx, sz = g.Sxy;
    long long n = g.idx(i, j, k0);
    const double oma = 1.0 - alpha;

    const double *c[KIN_GROUP];
    double zm3[KIN_GROUP], zm2[KIN_GROUP], zm1[KIN_GROUP], z0[KIN_GROUP], zp1[KIN_GROUP], zp2[KIN_GROUP], Fz_lo[KIN_GROUP];
    {
        const double w_lo = w[n];
#pragma unroll
        for (int s = 0; s < KIN_GROUP; ++s) {
            if (s >= ns) continue;
            const double *cs = c[s] = P.c[s0 + s];
            zm3[s] = cs[n - 3 * sz]; zm2[s] = cs[n - 2 * sz]; zm1[s] = cs[n - sz]; z0[s] = cs[n]; zp1[s] = cs[n + sz]; zp2[s] = cs[n + 2 * sz];
            Fz_lo[s] = kin_flux_z(g, w_lo, zm3[s], zm2[s], zm1[s], z0[s], zp1[s], zp2[s], k0);
        }
    }

    for (int k = k0; k < k1; ++k, n += sz) {
        // the advecting velocities of the cell's faces and D: once per level, for every scalar of the group
        const double w_hi = w[n + sz], u_lo = u[n], u_hi = u[n + 1];
        double v_lo = 0.0, v_hi = 0.0;
        if (!g.flat_y) { v_lo = v[n]; v_hi = v[n + sy]; }      // a Flat y direction has no faces
        const double Dn = CORR ? D[n] : 0.0;
        const double rho = g.rho[k], Ax = g.Ax[k], Ay = g.Ay[k], Vinv = g.Vinv_c[k];
#pragma unroll
        for (int s = 0; s < KIN_GROUP; ++s) {
            if (s >= ns) continue;
            const double *cs = c[s];
            const double zp3 = cs[n + 3 * sz], cc = z0[s];
            const double Fz_hi = kin_flux_z(g, w_hi, zm2[s], zm1[s], cc, zp1[s], zp2[s], zp3, k + 1);

            const double xm3 = cs[n - 3], xm2 = cs[n - 2], xm1 = cs[n - 1], xp1 = cs[n + 1], xp2 = cs[n + 2], xp3 = cs[n + 3];
            const double Fx_lo = rho * ((Ax * u_lo) * bz_upB(xm3, xm2, xm1, cc, xp1, xp2, u_lo > 0.0, 3));
            const double Fx_hi = rho * ((Ax * u_hi) * bz_upB(xm2, xm1, cc, xp1, xp2, xp3, u_hi > 0.0, 3));

            double Fy_lo = 0.0, Fy_hi = 0.0;
            if (!g.flat_y) {
                const double ym3 = cs[n - 3 * sy], ym2 = cs[n - 2 * sy], ym1 = cs[n - sy], yp1 = cs[n + sy], yp2 = cs[n + 2 * sy], yp3 = cs[n + 3 * sy];
                Fy_lo = rho * ((Ay * v_lo) * bz_upB(ym3, ym2, ym1, cc, yp1, yp2, v_lo > 0.0, 3));
                Fy_hi = rho * ((Ay * v_hi) * bz_upB(ym2, ym1, cc, yp1, yp2, yp3, v_hi > 0.0, 3));
            }

            double Gc = -(Vinv * ((Fx_hi - Fx_lo) + (Fy_hi - Fy_lo) + (Fz_hi - Fz_lo[s])));
            if (CORR) Gc = Gc + cc * Dn;      // + c div_rhoU (dynamics_kernel_functions.jl:155-156)

            if (MODE == 0) {
                P.G[s0 + s][n] = Gc;
            } else {
                double *rc = P.rc[s0 + s];
                const double uold = rc[n];
                double u0v;
                if (MODE == 1) { P.u0[s0 + s][n] = uold; u0v = uold; }
                else u0v = P.u0[s0 + s][n];
                rc[n] = oma * u0v + alpha * (uold + dt * Gc);
            }

            zm3[s] = zm2[s]; zm2[s] = zm1[s]; zm1[s] = cc; z0[s] = zp1[s]; zp1[s] = zp2[s]; zp2[s] = zp3;
            Fz_lo[s] = Fz_hi;
        }
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------
static int kin_require(bz_ctx *ctx, const char *who)
{
    if (ctx->kinematic) return BZ_OK;
    ctx->last_error = std::string(who) + ": the context has no PrescribedDynamics (bz_set_prescribed_dynamics); anelastic contexts step with "
                                         "bz_time_step_anelastic";
    return BZ_ERR_UNSUPPORTED;
}

// what a kinematic context runs: the WENO(order = 5) theta model with microphysics nothing or warm-phase saturation adjustment and tracers
static int kin_configuration(bz_ctx *ctx, const char *who)
{
    const DevGrid &g = ctx->dg;
    const char *what = nullptr;
    if (ctx->weno_R != 3 || ctx->scalar_R != 3) what = "WENO(order = 5) is implemented";
    else if (g.formulation != 0) what = "the StaticEnergy formulation is not implemented";
    else if (g.microphysics == 2) what = "Kessler microphysics is not implemented";
    else if (ctx->has_closure || ctx->has_diffusivity) what = "closures are not implemented";
    else if (ctx->has_forcings || ctx->has_relaxation || ctx->field_forcing) what = "forcings and sponges are not implemented";
    else if (ctx->has_bulk) what = "flux boundary conditions are not implemented";
    else if (ctx->bounded_mask) what = "bounds-preserving advection is not implemented";
    else if (ctx->graph_mode) what = "hipGraph replay is not implemented";
    if (!what) return BZ_OK;
    ctx->last_error = std::string(who) + " (PrescribedDynamics): " + what;
    return BZ_ERR_UNSUPPORTED;
}

extern "C" int bz_set_prescribed_dynamics(bz_ctx *ctx, int divergence_correction)
{
    if (!ctx) return BZ_ERR_INVALID;
    ++ctx->config_epoch;
    ++ctx->velocity_epoch;      // every call says: the velocity fields may have changed
    const DevGrid &g = ctx->dg;
    if (ctx->compressible) { ctx->last_error = "bz_set_prescribed_dynamics: compressible contexts have prognostic momentum"; return BZ_ERR_UNSUPPORTED; }
    if (ctx->slab_mode || g.bounded_x || g.bounded_y) {
        ctx->last_error = "bz_set_prescribed_dynamics: single-device (Periodic, Periodic, Bounded) and (Periodic, Flat, Bounded) contexts";
        return BZ_ERR_UNSUPPORTED;
    }
    if (divergence_correction && !ctx->d_kin_div) {
        const size_t bytes = (size_t)g.Sxy * (size_t)(g.Nz + 2 * g.Hz) * sizeof(double);
        BZ_HIP(hipMalloc(&ctx->d_kin_div, bytes));
        BZ_HIP(hipMemsetAsync(ctx->d_kin_div, 0, bytes, ctx->stream));
    }
    ctx->kinematic = true;
    ctx->kin_correction = divergence_correction != 0;
    return BZ_OK;
}

void bzi_kinematic_teardown(bz_ctx *ctx)
{
    if (ctx->d_kin_div) hipFree(ctx->d_kin_div);
    ctx->d_kin_div = nullptr;
}

static void kin_scalars(const bz_ctx *ctx, const bz_state *s, const bz_prognostic *U0, const bz_prognostic *G, KinScalars *P)
{
    P->n = 2 + ctx->n_tracers;
    for (int t = 0; t < KIN_MAX_SCALARS; ++t) { P->c[t] = nullptr; P->rc[t] = P->u0[t] = P->G[t] = nullptr; }
    P->c[0] = s->theta; P->rc[0] = s->rho_theta; P->u0[0] = U0 ? U0->rho_theta : nullptr; P->G[0] = G ? G->rho_theta : nullptr;
    P->c[1] = s->q; P->rc[1] = s->rho_q; P->u0[1] = U0 ? U0->rho_q : nullptr; P->G[1] = G ? G->rho_q : nullptr;
    for (int t = 0; t < ctx->n_tracers; ++t) {
        const bz_tracer_fields &T = ctx->tracers[t];
        P->c[2 + t] = T.specific; P->rc[2 + t] = T.density; P->u0[2 + t] = T.U0; P->G[2 + t] = T.G;
    }
}

// D is formed when the correction is on and the velocities changed since it was last formed (velocity epoch, or other arrays)
static int kin_mass_divergence(bz_ctx *ctx, const bz_state *s)
{
    if (!ctx->kin_correction) return BZ_OK;
    if (ctx->kin_div_epoch == ctx->velocity_epoch && ctx->kin_div_u == s->u && ctx->kin_div_v == s->v && ctx->kin_div_w == s->w) return BZ_OK;
    const DevGrid &g = ctx->dg;
    ProfileScope ps(ctx, "kinematic_mass_divergence");
    hipLaunchKernelGGL(k_kin_mass_divergence, dim3((g.Nx + KTX - 1) / KTX, (g.Ny + KTY - 1) / KTY, g.Nz), dim3(KTX, KTY), 0, ctx->stream, g,
                       ctx->d_kin_div, s->u, s->v, s->w);
    BZ_LAUNCH_CHECK();
    ctx->kin_div_epoch = ctx->velocity_epoch;
    ctx->kin_div_u = s->u; ctx->kin_div_v = s->v; ctx->kin_div_w = s->w;
    return BZ_OK;
}

// mode 0: tendencies into G; 1 / 2: first / later RK stage
static int kin_stage(bz_ctx *ctx, const bz_state *s, const bz_prognostic *U0, const bz_prognostic *G, int mode, double dt, double alpha)
{
    int rc;
    if ((rc = kin_mass_divergence(ctx, s))) return rc;
    const DevGrid &g = ctx->dg;
    KinScalars P;
    kin_scalars(ctx, s, U0, G, &P);
    const int groups = (P.n + KIN_GROUP - 1) / KIN_GROUP;
    // level chunks: at least 8 levels each, enough blocks to fill the device (as bz_tendency.hip: pick_kchunk)
    const long long tiles = (long long)((g.Nx + KTX - 1) / KTX) * ((g.Ny + KTY - 1) / KTY) * groups;
    long long want = (4096 + tiles - 1) / tiles;
    const long long maxchunks = g.Nz / 8 > 0 ? g.Nz / 8 : 1;
    if (want > maxchunks) want = maxchunks;
    const int kchunk = (int)((g.Nz + want - 1) / want), nchunks = (g.Nz + kchunk - 1) / kchunk;
    const dim3 grid((g.Nx + KTX - 1) / KTX, (g.Ny + KTY - 1) / KTY, nchunks * groups), block(KTX, KTY);
    const double *D = ctx->d_kin_div;
    ProfileScope ps(ctx, mode ? "kinematic_scalar_stage" : "kinematic_scalar_tendencies");
#define KIN_LAUNCH(M, C) hipLaunchKernelGGL((k_kin_scalar_stage<M, C>), grid, block, 0, ctx->stream, g, P, s->u, s->v, s->w, D, kchunk, nchunks, dt, alpha)
    if (ctx->kin_correction) {
        if (mode == 0) KIN_LAUNCH(0, true); else if (mode == 1) KIN_LAUNCH(1, true); else KIN_LAUNCH(2, true);
    } else {
        if (mode == 0) KIN_LAUNCH(0, false); else if (mode == 1) KIN_LAUNCH(1, false); else KIN_LAUNCH(2, false);
    }
#undef KIN_LAUNCH
    BZ_LAUNCH_CHECK();
    return BZ_OK;
}

static int kin_check_state(bz_ctx *ctx, const bz_state *s, const bz_prognostic *U0, const bz_prognostic *G)
{
    if (!s || !s->u || !s->v || !s->w || !s->theta || !s->q || !s->T || !s->rho_theta || !s->rho_q) return BZ_ERR_INVALID;
    if (U0 && (!U0->rho_theta || !U0->rho_q)) return BZ_ERR_INVALID;
    if (G && (!G->rho_theta || !G->rho_q)) return BZ_ERR_INVALID;
    return BZ_OK;
}

// update_state! of a kinematic model (update_atmosphere_model_state.jl:41-68 with compute_velocities! = nothing): halo fill of the
// prognostic scalars, theta / q / T (+ saturation adjustment) and tracer_density_to_specific! with their halo fills, tendencies on request
int bzi_kinematic_update_state(bz_ctx *ctx, const bz_state *s, const bz_prognostic *G, int compute_tendencies)
{
    int rc;
    if ((rc = kin_check_state(ctx, s, nullptr, compute_tendencies ? G : nullptr))) return rc;
    ctx->diagnostics_stale = false;
    double *sf[2] = {s->rho_theta, s->rho_q};
    int sk[2] = {0, 0};
    if ((rc = bzi_fill_halos_multi(ctx, sf, sk, 2))) return rc;
    if ((rc = bz_compute_auxiliary_thermodynamic_variables(ctx, s))) return rc;
    if (!compute_tendencies) return BZ_OK;
    if ((rc = kin_configuration(ctx, "bz_update_state"))) return rc;
    return kin_stage(ctx, s, nullptr, G, 0, 0.0, 0.0);
}

extern "C" int bz_compute_kinematic_tendencies(bz_ctx *ctx, const bz_state *s, const bz_prognostic *G)
{
    if (!ctx || !s || !G) return BZ_ERR_INVALID;
    int rc;
    if ((rc = kin_require(ctx, "bz_compute_kinematic_tendencies"))) return rc;
    if ((rc = kin_configuration(ctx, "bz_compute_kinematic_tendencies"))) return rc;
    if ((rc = kin_check_state(ctx, s, nullptr, G))) return rc;
    if (ctx->diagnostics_stale && (rc = bzi_kinematic_update_state(ctx, s, nullptr, 0))) return rc;
    return kin_stage(ctx, s, nullptr, G, 0, 0.0, 0.0);
}

// n steps.  The stage kernel reads the specific fields of the previous update_state!, so every stage is followed by one — except, with
// diagnose_last == 0, the very last: the prognostic scalars are current then, theta / q / T and the specific tracers are stale
// (bz_diagnostics_stale) and the next call of this function, or bz_update_state, rebuilds them first.
extern "C" int bz_time_steps_kinematic(bz_ctx *ctx, const bz_state *s, const bz_prognostic *U0, const bz_prognostic *G, double dt, int n,
                                       int diagnose_last)
{
    if (!ctx || !s || !U0 || !G || n < 0) return BZ_ERR_INVALID;
    int rc;
    if ((rc = kin_require(ctx, "bz_time_steps_kinematic"))) return rc;
    if ((rc = kin_configuration(ctx, "bz_time_steps_kinematic"))) return rc;
    if ((rc = kin_check_state(ctx, s, U0, G))) return rc;
    if (n > 0 && ctx->diagnostics_stale && (rc = bzi_kinematic_update_state(ctx, s, nullptr, 0))) return rc;
    for (int it = 0; it < n; ++it) {
        for (int stage = 0; stage < 3; ++stage) {
            if ((rc = kin_stage(ctx, s, U0, G, stage == 0 ? 1 : 2, dt, BZ_SSP_RK3_ALPHA[stage]))) return rc;
            if (it == n - 1 && stage == 2 && !diagnose_last) { ctx->diagnostics_stale = true; break; }
            if ((rc = bzi_kinematic_update_state(ctx, s, nullptr, 0))) return rc;
        }
    }
    return BZ_OK;
}
