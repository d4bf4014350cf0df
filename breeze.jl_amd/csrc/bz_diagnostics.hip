// bz_diagnostics.hip — the output diagnostics the reference's examples write every output interval, evaluated on the device:
//   PotentialTemperature, LiquidIce-, Virtual-, Equivalent-, StabilityEquivalentPotentialTemperature
//                                         /root/reference/src/AtmosphereModels/Diagnostics/potential_temperatures.jl:538-616
//   StaticEnergy                          /root/reference/src/AtmosphereModels/Diagnostics/static_energy.jl:94-120
//   RelativeHumidity                      /root/reference/src/Microphysics/microphysics_diagnostics.jl:139-170
//   SaturationSpecificHumidity            /root/reference/src/AtmosphereModels/Diagnostics/saturation_specific_humidity.jl:111-149
//                                         (:equilibrium: /root/reference/src/Thermodynamics/vapor_saturation.jl:216-230)
//   DewpointTemperature                   /root/reference/src/AtmosphereModels/Diagnostics/dewpoint_temperature.jl:97-119,
//                                         /root/reference/src/Thermodynamics/vapor_saturation.jl:313-331, src/Solvers.jl:243-262
//   Average(field, dims = (1, 2))         Oceananigans' horizontal average of one field
// bz_compute_diagnostics is ONE pointwise kernel for a caller-given list of kinds: T, q^v, q^l (p, rho) are read once however many
// outputs are requested, and flavours requested together share ln(p / p_st), p^v+(T) and theta^e.  The list is a kernel argument, so
// every branch on it is wave-uniform; the only per-lane divergence is the dewpoint's iteration count.  Each quantity is formed at one
// place of the kernel, so a fused call and n single calls store the same bits.
// bz_horizontal_average sums each level in a fixed order (rows of a slice thread-strided, an LDS tree, then the slices in index order)
// and divides the level sum by Nx Ny: no floating-point atomics, two calls give the same bits.
#include "bz_internal.h"

#define DG_NEED_LNP 1          // ln(p / p_st): every potential temperature
#define DG_NEED_PSAT 2         // p^v+(T), rho* = p / (R_m T), p^v = rho* q^v R_v T
#define DG_NEED_THETA 4        // theta = T / Pi_m
#define DG_NEED_THETA_E 8      // theta^e
#define HSLICES 16             // row slices per level of the horizontal average

struct DiagArgs {
    const double *T, *qv, *ql, *ql2, *qe, *p, *rho;
    double Ll, cl, Tr, Ttr, ptr, dc, L0;      // dc = c_pv - c_l, L0 = L_lr - dc T_r (clausius_clapeyron.jl:59-68)
    int n, need;
    int kind[BZ_MAX_DIAGNOSTICS];
    double *out[BZ_MAX_DIAGNOSTICS];
};

// saturation vapour pressure over a planar liquid surface: p_tr (T / T_tr)^(dc / R_v) exp((1 / T_tr - 1 / T) L0 / R_v), the power as
// the exponential of its logarithm so that the whole is one log and one exp
__device__ __forceinline__ double dg_psat(const DevGrid &g, const DiagArgs &A, double T)
{
    return A.ptr * exp((A.dc / g.Rv) * log(T / A.Ttr) + (1.0 / A.Ttr - 1.0 / T) * A.L0 / g.Rv);
}

// x^y from ln x; y == 0 gives 1 for every x, as pow does (a cell without vapour has H = 0 and the exponent -R_v q^v / c_pm = -0)
__device__ __forceinline__ double dg_lnpow_arg(double lnx, double y) { return y == 0.0 ? 0.0 : y * lnx; }

// dewpoint_temperature(p^v, T, constants, PlanarLiquidSurface(), SecantSolver(reltol = 1e-4, abstol = 0, maxiter = 10))
__device__ __forceinline__ double dg_dewpoint(const DevGrid &g, const DiagArgs &A, double T, double pv, double ps)
{
    double r1 = ps - pv;
    if (r1 <= 0.0) return T;
    const double H = pv / ps;
    double x1 = T, x2 = T - (1.0 - H) * 20.0;
    double r2 = dg_psat(g, A, x2) - pv;
    const double tol = fmax(0.0, 1e-4 * fabs(pv));
    for (int it = 0; it < 10 && fabs(r2) > tol; ++it) {
        double s = (x2 - x1) / (r2 - r1);
        const bool valid = isfinite(s);
        s = valid ? s : 0.0;
        x1 = x2; r1 = r2;
        x2 -= r2 * s;
        r2 = valid ? dg_psat(g, A, x2) - pv : 0.0;
    }
    return x2;
}

__global__ __launch_bounds__(256) void k_diagnostics(DevGrid g, DiagArgs A)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y, k = blockIdx.z;
    if (i >= g.Nx) return;
    const long long n = g.idx(i, j, k);
    const double T = A.T[n], qv = A.qv[n];
    double ql = A.ql ? A.ql[n] : 0.0;
    if (A.ql2) ql += A.ql2[n];
    const bool cols = !A.p || !A.rho;      // reference columns: p, rho and ln(p / p_st) are constants of the level
    const double p = cols ? g.p_r[k] : A.p[n];
    const double rho = cols ? g.rho[k] : A.rho[n];
    const double qd = 1.0 - (qv + ql);
    const double Rm = qd * g.Rd + qv * g.Rv;
    const double cpm = qd * g.cpd + qv * g.cpv + ql * A.cl;

    double lnp = 0.0, ps = 0.0, rhos = 0.0, pv = 0.0, theta = 0.0, theta_e = 0.0;
    if (A.need & DG_NEED_LNP) lnp = cols ? g.lnpi[k] : log(p / g.pst);
    if (A.need & DG_NEED_PSAT) {
        ps = dg_psat(g, A, T);
        rhos = p / (Rm * T);
        pv = rhos * qv * g.Rv * T;
    }
    if (A.need & DG_NEED_THETA) theta = T / exp((Rm / cpm) * lnp);
    if (A.need & DG_NEED_THETA_E) {
        const double H = pv / ps;
        const double Lv = A.Ll + A.dc * (T - A.Tr);
        theta_e = T * exp(-(g.Rd / cpm) * lnp + Lv * qv / (cpm * T) + dg_lnpow_arg(log(H), -g.Rv * qv / cpm));
    }

    for (int m = 0; m < A.n; ++m) {
        const int kd = A.kind[m] & 0xff;
        double v;
        switch (kd) {
        case BZ_DIAG_POTENTIAL_TEMPERATURE: v = theta; break;
        case BZ_DIAG_LIQUID_ICE_POTENTIAL_TEMPERATURE: v = theta * (1.0 - A.Ll * ql / (cpm * T)); break;
        case BZ_DIAG_VIRTUAL_POTENTIAL_TEMPERATURE:
            v = T / exp((g.Rd / g.cpd) * lnp) * (1.0 + (g.Rv / g.Rd - 1.0) * qv - ql);
            break;
        case BZ_DIAG_EQUIVALENT_POTENTIAL_TEMPERATURE: v = theta_e; break;
        case BZ_DIAG_STABILITY_EQUIVALENT_POTENTIAL_TEMPERATURE:
            v = theta_e * exp(dg_lnpow_arg(log(T / A.Tr), A.cl * ql / cpm));
            break;
        case BZ_DIAG_STATIC_ENERGY: v = cpm * T + g.g * g.zc[k] - A.Ll * ql; break;
        case BZ_DIAG_RELATIVE_HUMIDITY: v = pv / fmax(ps, 2.220446049250313e-16); break;
        case BZ_DIAG_SATURATION_SPECIFIC_HUMIDITY: v = ps / (rhos * g.Rv * T); break;
        case BZ_DIAG_SATURATION_SPECIFIC_HUMIDITY_EQUILIBRIUM: {
            const double qt = A.qe[n], eps = g.Rd / g.Rv;
            const double q1 = eps * (1.0 - qt) * ps / (p - ps);
            const double re = p / ((g.Rd * (1.0 - qt) + g.Rv * qt) * T);
            const double q0 = ps / (re * g.Rv * T);
            v = qt >= q0 ? q1 : q0;
            break;
        }
        case BZ_DIAG_SATURATION_SPECIFIC_HUMIDITY_TOTAL_MOISTURE: {
            const double eps = g.Rd / g.Rv;
            v = eps * ps / (p + (eps - 1.0) * ps);
            break;
        }
        default: v = dg_dewpoint(g, A, T, pv, ps); break;      // BZ_DIAG_DEWPOINT_TEMPERATURE (the host rejects every other value)
        }
        if (A.kind[m] & BZ_DIAG_DENSITY_WEIGHTED) v *= rho;
        A.out[m][n] = v;
    }
}

static bool diag_has_density_flavour(int kd)
{
    return kd <= BZ_DIAG_STABILITY_EQUIVALENT_POTENTIAL_TEMPERATURE || kd == BZ_DIAG_STATIC_ENERGY;
}

extern "C" int bz_compute_diagnostics(bz_ctx *ctx, const bz_state *s, const bz_diagnostic_inputs *in, int32_t n, const int32_t *kinds,
                                      double *const *outputs)
{
    if (!ctx || !in || !kinds || !outputs) return BZ_ERR_INVALID;
    if (n < 1 || n > BZ_MAX_DIAGNOSTICS) { ctx->last_error = "bz_compute_diagnostics: 1 <= n <= BZ_MAX_DIAGNOSTICS"; return BZ_ERR_INVALID; }
    if (!in->temperature || !in->vapor) { ctx->last_error = "bz_compute_diagnostics: temperature and vapor are required"; return BZ_ERR_INVALID; }
    { const int rcs = bzi_refresh_diagnostics(ctx, s, "bz_compute_diagnostics"); if (rcs) return rcs; }
    const DevGrid &g = ctx->dg;
    DiagArgs A;
    A.T = in->temperature; A.qv = in->vapor; A.ql = in->liquid; A.ql2 = in->liquid_2; A.qe = in->moisture;
    A.p = in->pressure; A.rho = in->density;
    if ((!A.p || !A.rho) && ctx->compressible && !ctx->has_reference) {
        ctx->last_error = "bz_compute_diagnostics: this compressible context has no reference state: pass pressure and density fields";
        return BZ_ERR_INVALID;
    }
    A.Ll = in->liquid_latent_heat; A.cl = in->liquid_heat_capacity; A.Tr = in->energy_reference_temperature;
    A.Ttr = in->triple_point_temperature; A.ptr = in->triple_point_pressure;
    A.dc = g.cpv - A.cl;
    A.L0 = A.Ll - A.dc * A.Tr;
    A.n = n; A.need = 0;
    for (int m = 0; m < BZ_MAX_DIAGNOSTICS; ++m) { A.kind[m] = 0; A.out[m] = nullptr; }
    for (int m = 0; m < n; ++m) {
        const int kd = kinds[m] & 0xff;
        if (kd < 0 || kd >= BZ_DIAG_KIND_COUNT || (kinds[m] & ~(0xff | BZ_DIAG_DENSITY_WEIGHTED))) {
            ctx->last_error = "bz_compute_diagnostics: unknown diagnostic kind";
            return BZ_ERR_INVALID;
        }
        if ((kinds[m] & BZ_DIAG_DENSITY_WEIGHTED) && !diag_has_density_flavour(kd)) {
            ctx->last_error = "bz_compute_diagnostics: only the potential temperatures and the static energy have a density-weighted flavour";
            return BZ_ERR_INVALID;
        }
        if (!outputs[m]) { ctx->last_error = "bz_compute_diagnostics: null output"; return BZ_ERR_INVALID; }
        if (kd == BZ_DIAG_SATURATION_SPECIFIC_HUMIDITY_EQUILIBRIUM && !in->moisture) {
            ctx->last_error = "bz_compute_diagnostics: the :equilibrium flavour needs the `moisture` input";
            return BZ_ERR_INVALID;
        }
        A.kind[m] = kinds[m];
        A.out[m] = outputs[m];
        if (kd <= BZ_DIAG_STABILITY_EQUIVALENT_POTENTIAL_TEMPERATURE) A.need |= DG_NEED_LNP;
        if (kd <= BZ_DIAG_LIQUID_ICE_POTENTIAL_TEMPERATURE) A.need |= DG_NEED_THETA;
        if (kd == BZ_DIAG_EQUIVALENT_POTENTIAL_TEMPERATURE || kd == BZ_DIAG_STABILITY_EQUIVALENT_POTENTIAL_TEMPERATURE)
            A.need |= DG_NEED_THETA_E | DG_NEED_PSAT;
        if (kd >= BZ_DIAG_RELATIVE_HUMIDITY) A.need |= DG_NEED_PSAT;
    }
    if ((A.need & DG_NEED_PSAT) && !(A.Ttr > 0.0 && A.ptr > 0.0)) {
        ctx->last_error = "bz_compute_diagnostics: the liquid-phase constants of bz_diagnostic_inputs are not set";
        return BZ_ERR_INVALID;
    }
    ProfileScope ps(ctx, "diagnostics");
    const int bs = g.Nx <= 64 ? 64 : (g.Nx <= 128 ? 128 : 256);      // a block is a row segment of one level
    hipLaunchKernelGGL(k_diagnostics, dim3((g.Nx + bs - 1) / bs, g.Ny, g.Nz), dim3(bs), 0, ctx->stream, g, A);
    BZ_LAUNCH_CHECK();
    return BZ_OK;
}

// ---- Average(field, dims = (1, 2)) ----------------------------------------------------------------------------------------------
// stage 1: block (level, slice) adds the interior cells of its rows — a thread owns the columns i = t, t + 256, ... of every row, in row
// order — then an LDS tree; stage 2 adds the HSLICES partial sums of a level in index order and divides by Nx Ny
__global__ __launch_bounds__(256) void k_havg_partial(DevGrid g, const double *__restrict__ f, double *__restrict__ partial)
{
    const int k = blockIdx.x, s = blockIdx.y;
    const int j0 = (int)((long long)g.Ny * s / HSLICES), j1 = (int)((long long)g.Ny * (s + 1) / HSLICES);
    double a = 0.0;
    for (int j = j0; j < j1; ++j) {
        const double *row = f + g.idx(0, j, k);
        for (int i = threadIdx.x; i < g.Nx; i += 256) a += row[i];
    }
    __shared__ double red[256];
    red[threadIdx.x] = a;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[(long long)k * HSLICES + s] = red[0];
}

__global__ __launch_bounds__(256) void k_havg_finish(const double *__restrict__ partial, double *__restrict__ profile, int nlev, double count)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= nlev) return;
    double sum = 0.0;
    for (int s = 0; s < HSLICES; ++s) sum += partial[(long long)k * HSLICES + s];
    profile[k] = sum / count;
}

void bzi_diagnostics_teardown(bz_ctx *ctx)
{
    if (ctx->d_havg) hipFree(ctx->d_havg);
    ctx->d_havg = nullptr;
}

extern "C" int bz_horizontal_average(bz_ctx *ctx, const double *field, int z_face, double *profile)
{
    if (!ctx || !field || !profile) return BZ_ERR_INVALID;
    if (ctx->slab_mode) {
        ctx->last_error = "bz_horizontal_average: not implemented on y-slab contexts (the average needs an all-reduce over the ranks)";
        return BZ_ERR_UNSUPPORTED;
    }
    const DevGrid &g = ctx->dg;
    const int nlev = g.Nz + (z_face ? 1 : 0);
    if (!ctx->d_havg) BZ_HIP(hipMalloc(&ctx->d_havg, (size_t)(g.Nz + 1) * (HSLICES + 1) * sizeof(double)));
    double *partial = ctx->d_havg, *result = ctx->d_havg + (size_t)(g.Nz + 1) * HSLICES;
    ProfileScope ps(ctx, "horizontal_average");
    hipLaunchKernelGGL(k_havg_partial, dim3(nlev, HSLICES), dim3(256), 0, ctx->stream, g, field, partial);
    BZ_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_havg_finish, dim3((nlev + 255) / 256), dim3(256), 0, ctx->stream, partial, result, nlev,
                       (double)((long long)g.Nx * g.Ny));
    BZ_LAUNCH_CHECK();
    BZ_HIP(hipMemcpyAsync(profile, result, (size_t)nlev * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    BZ_HIP(hipStreamSynchronize(ctx->stream));
    return BZ_OK;
}
