// bz_instant_precip.hip — microphysics = InstantaneousPrecipitation(equilibrium = WarmPhaseEquilibrium()) on CompressibleDynamics: the
// Reed-Jablonowski large-scale condensation with immediate rain-out, and the column integral of its precipitation diagnostic.
//
//   InstantaneousPrecipitation, its fields and interface   /root/reference/src/Microphysics/instantaneous_precipitation.jl:39-102
//   microphysics_model_update! and its kernel              /root/reference/src/Microphysics/instantaneous_precipitation.jl:115-185
//   adjust_thermodynamic_state(::LiquidIceDensityState)    /root/reference/src/Microphysics/saturation_adjustment.jl:236-301 (bz_ds_adjust, bz_internal.h)
//   with_temperature(::LiquidIceDensityState, T)           /root/reference/src/Thermodynamics/dynamic_states.jl:251-264
//   where the step calls it                                /root/reference/src/TimeSteppers/acoustic_runge_kutta_3.jl:307-316
//
// Inside a stage the scheme does nothing (maybe_adjust_thermodynamic_state returns the state, the moisture fractions are vapour only,
// :73-86): every stage kernel sees a plain vapour-carrying model, DevGrid::microphysics stays 0.  Once per step, after the update_state!
// that follows stage 3, k_instantaneous_precipitation condenses what is above saturation at the cell's own total density, leaves the
// latent heat in the air and removes the condensate; update_state! with tendencies follows (total density, T, p, velocities, halos,
// closure fields, the moisture tendency of the next step's first stage).
#include <cmath>

#include "bz_compressible_internal.h"

// One thread per interior cell, lanes along x; a ragged Nx is a predicate on the lane.  Reads rho, rho_d, rho theta, rho q^v of its own cell,
// writes rho theta, rho q^v and (where water condensed) precipitation_rate in place: 7 compulsory words per cell.  No LDS, no barrier, no
// halo writes (the update_state! that follows fills them).  A subsaturated cell leaves bz_ds_adjust before the secant loop.  q^v of the
// microphysical fields is the model's specific-moisture array: update_state! refreshes it (rho q^v / rho with the new total density).
// FL: the FlatauPolynomial instantiation (bz_set_saturation_vapor_pressure_polynomial), selected by the host
template <bool FL = false>
__global__ __launch_bounds__(256) void k_instantaneous_precipitation(DevGrid g, const double *__restrict__ rho, const double *__restrict__ rho_d,
                                                                     double *__restrict__ rth, double *__restrict__ rq,
                                                                     double *__restrict__ prate, double dt, double nabstol, int nmaxiter, const double *fl)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= g.Nx) return;
    const long long n = g.idx(i, blockIdx.y, blockIdx.z);
    const double r = rho[n], rd = rho_d[n];
    const double qt = rq[n] / r;              // total water = the prognostic vapour (no condensate is kept between steps)
    const double th0 = rth[n] / rd;           // rho theta is dry-coupled
    if (th0 == 0.0) return;                   // is_absolute_zero: nothing to adjust (and no temperature to divide by)
    double qv, ql;
    const double T = bz_ds_adjust<FL>(g, th0, qt, r, nabstol, nmaxiter, qv, ql, ColPtr(fl));
    // rain-out: the vapour-only parcel keeps T (with_temperature of the state without condensate, L = 0)
    const double qd = 1.0 - qv;
    const double Rm = qd * g.Rd + qv * g.Rv;
    const double cpm = qd * g.cpd + qv * g.cpv;
    const double thf = T * pow(g.pst / (r * Rm * T), Rm / cpm);
    const double c = r * fmax(0.0, qt - qv);  // exactly 0 in a subsaturated cell (q^v+ = q^t)
    rq[n] = r * qv;
    rth[n] = rd * thf;
    if (c > 0.0) prate[n] = c / dt;           // a cell that does not condense keeps the rate it had
}

// Field(Integral(f, dims = 3)): a lane owns a column, lanes along x, sum of f[k] dz_c[k] from k = 0 upward in that order (deterministic, no
// atomics); out: horizontal parent (Ny + 2 Hy) x (Nx + 2 Hx), interior positions only
__global__ __launch_bounds__(256) void k_column_integral(DevGrid g, const double *__restrict__ f, double *__restrict__ out)
{
    const int i = blockIdx.x * 256 + threadIdx.x, j = blockIdx.y;
    if (i >= g.Nx) return;
    const double *col = f + g.idx(i, j, 0);
    double a = 0.0;
    for (int k = 0; k < g.Nz; ++k) a += col[(long long)k * g.Sxy] * g.dzc[k];
    out[(long long)(j + g.Hy) * g.Sx + (i + g.Hx)] = a;
}

extern "C" int bz_set_instantaneous_precipitation(bz_ctx *ctx, const bz_saturation_adjustment *params, double *precipitation_rate)
{
    if (ctx) ++ctx->config_epoch;      // captured steps (bz_graph.hip) belong to one configuration
    if (!ctx) return BZ_ERR_INVALID;
    DevGrid &g = ctx->dg;
    if (!params) { ctx->has_instant_precip = false; ctx->ip_precipitation_rate = nullptr; return BZ_OK; }
    const char *why = !ctx->compressible     ? "the context was not created by bz_create_compressible (the anelastic model does not carry the scheme)"
                      : g.microphysics == 2  ? "DCMIP2016KesslerMicrophysics is attached"
                      : g.microphysics == 1  ? "SaturationAdjustment is attached"
                      : ctx->slab_mode       ? "not implemented on y-slab contexts"
                      : (g.bounded_x || g.bounded_y) ? "not implemented on a Bounded x or y"
                      : g.flat_y             ? "not implemented on a Flat y"
                                             : nullptr;
    if (why) {
        ctx->last_error = std::string("bz_set_instantaneous_precipitation: ") + why;
        return BZ_ERR_UNSUPPORTED;
    }
    if (!precipitation_rate || params->maxiter < 0) return BZ_ERR_INVALID;
    // what bz_ds_adjust reads; the standard pressure g.pst is the context's (bz_exner_reference_state::standard_pressure)
    g.sa_Ll = params->liquid_latent_heat;
    g.sa_cl = params->liquid_heat_capacity;
    g.sa_dc = ctx->constants.vapor_heat_capacity - params->liquid_heat_capacity;
    g.sa_L0 = params->liquid_latent_heat - g.sa_dc * params->energy_reference_temperature;
    g.sa_Ttr = params->triple_point_temperature;
    g.sa_ptr = params->triple_point_pressure;
    g.sa_abstol = params->abstol;
    g.sa_maxiter = params->maxiter;
    ctx->has_instant_precip = true;
    ctx->ip_precipitation_rate = precipitation_rate;
    return BZ_OK;
}

// the rain-out kernel alone on the state's own arrays (the caller has checked the state and that the scheme is attached)
int bzi_instantaneous_precipitation(bz_ctx *ctx, const bz_compressible_state *s, double dt)
{
    const DevGrid &g = ctx->dg;
    ProfileScope ps(ctx, "instantaneous_precipitation");
    const double *fl = bzi_flatau(ctx);
    if (fl)
        hipLaunchKernelGGL(k_instantaneous_precipitation<true>, dim3((g.Nx + 255) / 256, g.Ny, g.Nz), dim3(256), 0, ctx->stream, g, s->rho, s->rho_d,
                           s->rho_theta, s->rho_q, ctx->ip_precipitation_rate, dt, ctx->se.newton_abstol, ctx->se.newton_maxiter, fl);
    else
        hipLaunchKernelGGL(k_instantaneous_precipitation<false>, dim3((g.Nx + 255) / 256, g.Ny, g.Nz), dim3(256), 0, ctx->stream, g, s->rho, s->rho_d,
                           s->rho_theta, s->rho_q, ctx->ip_precipitation_rate, dt, ctx->se.newton_abstol, ctx->se.newton_maxiter, fl);
    BZ_LAUNCH_CHECK();
    return BZ_OK;
}

// microphysics_model_update!(::InstantaneousPrecipitation, model): the kernel, then update_state!(model) with tendencies
extern "C" int bz_instantaneous_precipitation_update(bz_ctx *ctx, const bz_compressible_state *s, const bz_compressible_prognostic *G,
                                                     const bz_acoustic_substepper *sub, double dt)
{
    BZ_REQUIRE_COMPRESSIBLE();
    if (!valid_state(s) || !valid_prog(G) || !valid_sub(sub)) return BZ_ERR_INVALID;
    if (!ctx->has_instant_precip) {
        ctx->last_error = "bz_instantaneous_precipitation_update: no InstantaneousPrecipitation attached";
        return BZ_ERR_INVALID;
    }
    if (!ctx->fused_ok && !small_grid_update_ok(ctx)) { ctx->last_error = "compressible path needs Nx >= 2Hx and Ny >= 2Hy"; return BZ_ERR_UNSUPPORTED; }
    if (!std::isfinite(dt) || !(dt > 0.0)) return BZ_OK;      // instantaneous_precipitation.jl:121: the whole update is skipped
    const int rc = bzi_instantaneous_precipitation(ctx, s, dt);
    return rc ? rc : bzi_compressible_update_state(ctx, s, G, sub, true, false);
}

extern "C" int bz_column_integral(bz_ctx *ctx, const double *field, double *out2d)
{
    if (!ctx || !field || !out2d) return BZ_ERR_INVALID;
    if (ctx->slab_mode) {
        ctx->last_error = "bz_column_integral: not implemented on y-slab contexts";
        return BZ_ERR_UNSUPPORTED;
    }
    const DevGrid &g = ctx->dg;
    ProfileScope ps(ctx, "column_integral");
    hipLaunchKernelGGL(k_column_integral, dim3((g.Nx + 255) / 256, g.Ny), dim3(256), 0, ctx->stream, g, field, out2d);
    BZ_LAUNCH_CHECK();
    return BZ_OK;
}
