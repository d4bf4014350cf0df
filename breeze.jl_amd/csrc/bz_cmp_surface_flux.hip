// bz_cmp_surface_flux.hip — BulkDrag / BulkSensibleHeatFlux / BulkVaporFlux bottom conditions of a CompressibleDynamics context
// (include/breeze_hip.h: bz_compressible_surface_fluxes).  The formulas are those of k_bulk_bottom_flux (bz_forcing.hip):
//   /root/reference/src/BoundaryConditions/bulk_drag.jl:114-135            J^u = -rho0 C^D U~ u at the x face (J^v at the y face)
//   /root/reference/src/BoundaryConditions/bulk_scalar_fluxes.jl:82-90,123-137,206-232   J^th, J^v at centres
//   /root/reference/src/BoundaryConditions/BoundaryConditions.jl:64-85     U^2 interpolated to the flux location
//   /root/reference/src/TimeSteppers/acoustic_runge_kutta_3.jl:187-196     where a stage adds them: after the slow tendencies, before the loop
// with a surface temperature per surface cell, so rho0 = p0 / (R^d T0), theta0 = T0 / Pi0 and q^v+(T0, rho0) are per cell too (a number
// is stored as a constant array: one code path).  The x / y neighbours of u, v are reached by periodic wrap indexing (wrap_of), so the
// kernel does not depend on which halo images the stage's earlier kernels have refreshed.
#include <cmath>
#include <vector>

#include "bz_compressible_internal.h"

struct CmpSfParams {
    double drag_c, drag_g2, heat_c, heat_g2, vap_c, vap_g2;
    double p0, Pi0;                 // surface pressure; (p0 / p_st)^(R^d / c_pd)
    double dc_Rv, L0_Rv, Ttr, ptr;  // saturation vapour pressure over a planar liquid surface: (c_pv - c_l) / R^v, L0 / R^v, triple point
    double tet_p, tet_a, tet_T, tet_dT;      // TetensFormula constants (the constants of a DCMIP2016 Kessler model): p_ref exp(a (T - T_ref) / (T - dT))
    int drag, heat, vapor, tetens;
    const double *T0_drag, *T0_heat, *T0_vap;      // (Ny x Nx) each
};

// one lane per surface column, j = blockIdx.y; the three conditions are wave-uniform switches
__global__ __launch_bounds__(256) void k_cmp_surface_flux(DevGrid g, CmpSfParams B, double *__restrict__ Gu, double *__restrict__ Gv,
                                                          double *__restrict__ Gth, double *__restrict__ Gq,
                                                          const double *__restrict__ u, const double *__restrict__ v,
                                                          const double *__restrict__ th, const double *__restrict__ qv)
{
    const int i = blockIdx.x * 256 + threadIdx.x, j = blockIdx.y;
    if (i >= g.Nx) return;
    const long long n = g.idx(i, j, 0);
    const long long c = (long long)j * g.Nx + i;
    const WrapIdx w = wrap_of(g, i, j);
    const double dz = g.dzc[0];
    auto sq = [](double a) { return a * a; };
    const double u0 = u[n], v0 = v[n];
    const double u_ip = u[n + w.ip], v_jp = v[n + w.jp];
    if (B.drag) {
        const double v2 = ((sq(v[n + w.im]) + sq(v[n + w.im + w.jp])) / 2 + (sq(v0) + sq(v_jp)) / 2) / 2;
        const double u2 = ((sq(u[n + w.jm]) + sq(u[n + w.jm + w.ip])) / 2 + (sq(u0) + sq(u_ip)) / 2) / 2;
        const double rho0 = B.p0 / (g.Rd * B.T0_drag[c]);
        const double Ju = -rho0 * B.drag_c * sqrt(sq(u0) + v2 + B.drag_g2) * u0;
        const double Jv = -rho0 * B.drag_c * sqrt(u2 + sq(v0) + B.drag_g2) * v0;
        Gu[n] += Ju / dz;
        Gv[n] += Jv / dz;
    }
    const double U2 = (sq(u0) + sq(u_ip)) / 2 + (sq(v0) + sq(v_jp)) / 2;
    if (B.heat) {
        const double T0 = B.T0_heat[c];
        const double rho0 = B.p0 / (g.Rd * T0), theta0 = T0 / B.Pi0;
        Gth[n] += (-rho0 * B.heat_c * sqrt(U2 + B.heat_g2) * (th[n] - theta0)) / dz;
    }
    if (B.vapor) {      // saturation_specific_humidity(T0, rho0, constants, PlanarLiquidSurface()): Clausius-Clapeyron, or the TetensFormula of
                        // the constants a Kessler model is built with (src/Thermodynamics/tetens_formula.jl:110-117)
        const double T0 = B.T0_vap[c];
        const double rho0 = B.p0 / (g.Rd * T0);
        const double ps = B.tetens ? B.tet_p * exp(B.tet_a * (T0 - B.tet_T) / (T0 - B.tet_dT))
                                   : B.ptr * pow(T0 / B.Ttr, B.dc_Rv) * exp((1.0 / B.Ttr - 1.0 / T0) * B.L0_Rv);
        const double q0 = ps / (rho0 * g.Rv * T0);
        Gq[n] += (-rho0 * B.vap_c * sqrt(U2 + B.vap_g2) * (qv[n] - q0)) / dz;
    }
}

void bzi_cmp_surface_flux_teardown(bz_ctx *ctx)
{
    if (ctx->d_cmp_sf_T0) (void)hipFree(ctx->d_cmp_sf_T0);
    ctx->d_cmp_sf_T0 = nullptr;
    ctx->cmp_sf_on = false;
}

// why this context does not carry the fluxes (nullptr: it does)
static const char *cmp_sf_refusal(const bz_ctx *ctx)
{
    if (ctx->kinematic) return "the context has PrescribedDynamics (kinematic driver): no momentum, no bottom fluxes of this kind";
    if (!ctx->compressible) return "the context is anelastic (bz_set_bulk_surface_fluxes and bz_set_surface_layer serve it)";
    if (ctx->slab_mode) return "not implemented on y-slab (distributed) compressible contexts";
    if (ctx->dg.bounded_x || ctx->dg.bounded_y) return "not implemented on a compressible context between walls (Bounded x / Bounded y)";
    if (ctx->dg.flat_y) return "not implemented on a compressible context with a Flat y";
    return nullptr;
}

extern "C" int bz_set_compressible_surface_fluxes(bz_ctx *ctx, const bz_compressible_surface_fluxes *f)
{
    if (ctx) ++ctx->config_epoch;      // captured steps (bz_graph.hip) belong to one configuration
    if (!ctx) return BZ_ERR_INVALID;
    if (const char *why = cmp_sf_refusal(ctx)) {
        ctx->last_error = std::string("bz_set_compressible_surface_fluxes: ") + why;
        return BZ_ERR_UNSUPPORTED;
    }
    if (!f) { ctx->cmp_sf_on = false; return BZ_OK; }
    if (ctx->dg.sa_mixed) {      // (the reverse order is refused by bz_set_compressible_mixed_phase_equilibrium)
        ctx->last_error = "bz_set_compressible_surface_fluxes: the bulk surface fluxes form c_pm without q^i, and the context's saturation adjustment "
                          "runs on MixedPhaseEquilibrium (bz_set_compressible_mixed_phase_equilibrium)";
        return BZ_ERR_UNSUPPORTED;
    }
    if (ctx->fl_on && f->vapor.enabled) {      // (the reverse order is refused by bz_set_saturation_vapor_pressure_polynomial)
        ctx->last_error = "bz_set_compressible_surface_fluxes: a bulk vapour flux evaluates the Clausius-Clapeyron q^v+ of the surface, and the context's "
                          "saturation adjustment runs on a FlatauPolynomial (bz_set_saturation_vapor_pressure_polynomial)";
        return BZ_ERR_UNSUPPORTED;
    }
    const DevGrid &g = ctx->dg;
    const size_t cells = (size_t)g.Nx * (size_t)g.Ny;
    const bz_compressible_surface_flux *cond[3] = {&f->drag, &f->heat, &f->vapor};
    if (!(f->surface_pressure > 0.0) || !(f->standard_pressure > 0.0)) {
        ctx->last_error = "bz_set_compressible_surface_fluxes: surface_pressure and standard_pressure must be positive";
        return BZ_ERR_INVALID;
    }
    std::vector<double> h(3 * cells, 1.0);      // (a switched-off condition keeps a harmless constant)
    for (int k = 0; k < 3; ++k) {
        if (!cond[k]->enabled) continue;
        for (size_t n = 0; n < cells; ++n) {
            const double T0 = cond[k]->surface_temperature_field ? cond[k]->surface_temperature_field[n] : cond[k]->surface_temperature;
            if (!(T0 > 0.0) || !std::isfinite(T0)) {
                ctx->last_error = "bz_set_compressible_surface_fluxes: every surface temperature of an enabled condition must be positive and finite";
                return BZ_ERR_INVALID;
            }
            h[(size_t)k * cells + n] = T0;
        }
        if (!std::isfinite(cond[k]->coefficient) || !std::isfinite(cond[k]->gustiness)) {
            ctx->last_error = "bz_set_compressible_surface_fluxes: coefficient and gustiness of an enabled condition must be finite";
            return BZ_ERR_INVALID;
        }
    }
    if (!ctx->d_cmp_sf_T0) BZ_HIP(hipMalloc(&ctx->d_cmp_sf_T0, 3 * cells * sizeof(double)));
    BZ_HIP(hipMemcpyAsync(ctx->d_cmp_sf_T0, h.data(), 3 * cells * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    BZ_HIP(hipStreamSynchronize(ctx->stream));      // the staging copy goes away with this call
    ctx->cmp_sf = *f;
    ctx->cmp_sf.drag.surface_temperature_field = ctx->cmp_sf.heat.surface_temperature_field = ctx->cmp_sf.vapor.surface_temperature_field = nullptr;
    ctx->cmp_sf_on = f->drag.enabled || f->heat.enabled || f->vapor.enabled;
    return BZ_OK;
}

// compute_flux_bc_tendencies!(model): G[.., 1] += J / dz_1, one launch over the surface; nothing to do without an attached set
int bzi_cmp_surface_fluxes(bz_ctx *ctx, const bz_compressible_state *s, const bz_compressible_prognostic *G)
{
    if (!ctx->cmp_sf_on) return BZ_OK;
    const DevGrid &g = ctx->dg;
    const bz_compressible_surface_fluxes &f = ctx->cmp_sf;
    const size_t cells = (size_t)g.Nx * (size_t)g.Ny;
    CmpSfParams B;
    B.drag = f.drag.enabled != 0; B.heat = f.heat.enabled != 0; B.vapor = f.vapor.enabled != 0;
    B.drag_c = f.drag.coefficient; B.drag_g2 = f.drag.gustiness * f.drag.gustiness;
    B.heat_c = f.heat.coefficient; B.heat_g2 = f.heat.gustiness * f.heat.gustiness;
    B.vap_c = f.vapor.coefficient; B.vap_g2 = f.vapor.gustiness * f.vapor.gustiness;
    B.p0 = f.surface_pressure;
    B.Pi0 = std::pow(f.surface_pressure / f.standard_pressure, g.Rd / g.cpd);
    const double dc = ctx->constants.vapor_heat_capacity - f.liquid_heat_capacity;
    B.dc_Rv = dc / g.Rv;
    B.L0_Rv = (f.liquid_latent_heat - dc * f.energy_reference_temperature) / g.Rv;
    B.Ttr = f.triple_point_temperature; B.ptr = f.triple_point_pressure;
    const bz_kessler_microphysics &K = ctx->kessler_params;
    B.tetens = g.microphysics == 2;
    B.tet_p = B.tetens ? K.tetens_reference_saturation_vapor_pressure : 0.0; B.tet_a = B.tetens ? K.tetens_liquid_coefficient : 0.0;
    B.tet_T = B.tetens ? K.tetens_reference_temperature : 0.0; B.tet_dT = B.tetens ? K.tetens_liquid_temperature_offset : 0.0;
    B.T0_drag = ctx->d_cmp_sf_T0; B.T0_heat = ctx->d_cmp_sf_T0 + cells; B.T0_vap = ctx->d_cmp_sf_T0 + 2 * cells;
    ProfileScope ps(ctx, "compressible_surface_fluxes");
    const double *qv = (g.microphysics == 1) ? g.qv_field : s->q;      // saturation adjustment: the diagnosed vapour; else the prognostic moisture
    hipLaunchKernelGGL(k_cmp_surface_flux, dim3((g.Nx + 255) / 256, g.Ny), dim3(256), 0, ctx->stream, g, B, G->rho_u, G->rho_v, G->rho_theta,
                       G->rho_q, s->u, s->v, s->theta, qv);
    BZ_LAUNCH_CHECK();
    return BZ_OK;
}

extern "C" int bz_compressible_compute_flux_bc_tendencies(bz_ctx *ctx, const bz_compressible_state *s, const bz_compressible_prognostic *G)
{
    if (!ctx) return BZ_ERR_INVALID;
    if (const char *why = cmp_sf_refusal(ctx)) {
        ctx->last_error = std::string("bz_compressible_compute_flux_bc_tendencies: ") + why;
        return BZ_ERR_UNSUPPORTED;
    }
    if (!valid_state(s) || !valid_prog(G)) return BZ_ERR_INVALID;
    return bzi_cmp_surface_fluxes(ctx, s, G);
}
