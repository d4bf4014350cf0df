// bz_balance.hip — discrete hydrostatic balance of the compressible model's initial and base state:
//
//   bz_exner_columns                          _compute_exner_reference_3d!      src/Thermodynamics/reference_states.jl:572-677,835-838
//   bz_set_hydrostatically_balanced_density   set_hydrostatically_balanced_density!  src/AtmosphereModels/set_to_mean.jl:53-110,271-310
//   bz_set_exner_reference_state              what set_to_mean!(::ExnerReferenceState, model) does to the context (set_to_mean.jl:165-201)
//
// Three kernels:
//   k_exner_columns               one lane per column, lanes along x (the layout of k_implicit_step, bz_diffusivity.hip): every level is one
//                                 coalesced row segment, a ragged Nx is a lane predicate.  Per level: three pow() for the first guess and the
//                                 closing Exner function, five more in the Newton iterations — ~8 pow of ~150 FP64 instructions each against
//                                 5 words of traffic.  The kernel is pow-bound, not memory-bound: no LDS, no barrier, no tiling, no limit on Nz.
//   k_rescale_density_weighted    one launch over a descriptor list: every listed field is multiplied by new / old of the two densities at its
//                                 own location (cell ratio for centres, ratio of the face means for rho u, rho v, rho w); both densities are read
//                                 once per thread (own cell and the three lower neighbours, through their halos).
//   k_dry_from_total              rho_d = rho - (rho q + rho q^cl + rho q^r), the sum in total_condensate_density's order.
// Scope: one device, (Periodic, Periodic | Flat, Bounded).  Walls and y-slabs return BZ_ERR_UNSUPPORTED.
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "bz_compressible_internal.h"

// moist_reference_constants (reference_states.jl:572-577): exactly the dry constants for q^v = 0
__device__ __forceinline__ void bal_moist_constants(const DevGrid &g, double qv, double &Rm, double &cpm, double &kap)
{
    const double qd = 1.0 - qv;
    Rm = qd * g.Rd + qv * g.Rv;
    cpm = qd * g.cpd + qv * g.cpv;
    kap = Rm / cpm;
}

// _compute_exner_column! + integrate_exner_column! (reference_states.jl:611-672) in the reference's order of operations.
// qv == nullptr: a dry column (ZeroField).  qv_den != nullptr: the vapour fraction is qv[n] / qv_den[n] (step 1 of the balanced set,
// _dry_weighted_specific_moisture!, formed where it is read).  Pi_out, p_out may be nullptr (the balanced set keeps the density only).
// Only interior cells are read and written: whatever the halos of theta and q^v hold does not reach the output.
__global__ __launch_bounds__(64) void k_exner_columns(DevGrid g, const double *th, const double *qv, const double *qv_den, double p0, double *Pi_out,
                                                      double *p_out, double *rho_out)
{
    const int i = blockIdx.x * 64 + threadIdx.x, j = blockIdx.y;
    if (i >= g.Nx) return;
    const long long sz = g.Sxy;
    long long n = g.idx(i, j, 0);
    const double pst = g.pst, grav = g.g;
    double Rm, cpm, kap;
    // anchor: half a step of the continuous Exner integration from the surface (face 1 is the impenetrable boundary: no balance constraint there)
    double q = !qv ? 0.0 : (qv_den ? qv[n] / qv_den[n] : qv[n]);
    bal_moist_constants(g, q, Rm, cpm, kap);
    const double Pi_surface = pow(p0 / pst, kap);
    double thm = th[n];
    double Pim = Pi_surface - grav * g.dzc[0] / (2 * cpm * thm);
    double pm = pst * pow(Pim, 1 / kap);
    double rhom = pm / (Rm * thm * Pim);
    if (Pi_out) Pi_out[n] = Pim;
    if (p_out) p_out[n] = pm;
    rho_out[n] = rhom;
    for (int k = 1; k < g.Nz; ++k) {
        n += sz;
        const double dzf = g.dzf[k];
        const double thk = th[n];
        q = !qv ? 0.0 : (qv_den ? qv[n] / qv_den[n] : qv[n]);
        bal_moist_constants(g, q, Rm, cpm, kap);
        // first guess: one face step of the continuous Exner integration
        const double th_face = (thk + thm) / 2;
        const double Pi_init = Pim - grav * dzf / (cpm * th_face);
        double pk = pst * pow(Pi_init, 1 / kap);
        // newton_hydrostatic_pressure, FixedIterations(5): F(p) = p / dzf + A p^(1 - kappa) - C
        const double A = grav * pow(pst, kap) / (2 * Rm * thk);
        const double Cc = pm / dzf - grav * rhom / 2;
#pragma unroll 1
        for (int it = 0; it < 5; ++it) {
            const double rp = pow(pk, -kap);
            const double f = pk / dzf + A * pk * rp - Cc;
            const double df = 1 / dzf + A * (1 - kap) * rp;
            pk -= f / df;
        }
        const double Pik = pow(pk / pst, kap);
        const double rhok = pk / (Rm * thk * Pik);
        if (Pi_out) Pi_out[n] = Pik;
        if (p_out) p_out[n] = pk;
        rho_out[n] = rhok;
        pm = pk; rhom = rhok; Pim = Pik; thm = thk;
    }
}

// _rescale_momentum! + the centre-field broadcasts of rescale_dry_density_weighted_fields! / scale_total_density_weighted_fields!
// (set_to_mean.jl:53-99): f *= num / den at the field's location.  Face ratios take the face means (a + b) / 2 of both densities through
// their halos (x, y: periodic images; a Flat y mean is the identity); rho w is rescaled on its interior faces 1 .. Nz - 1 — the wall faces
// keep what they hold.  Centre-only lists read neither density outside the interior.
#define BAL_MAX_FIELDS 8
#define BAL_CENTER 0
#define BAL_XFACE 1
#define BAL_YFACE 2
#define BAL_ZFACE 3
struct RescaleList {
    double *f[BAL_MAX_FIELDS];
    int loc[BAL_MAX_FIELDS];
    int n, mask;      // mask: bit l set = some field sits at location l
};
__global__ __launch_bounds__(256) void k_rescale_density_weighted(DevGrid g, RescaleList L, const double *__restrict__ num, const double *__restrict__ den)
{
    const int i = blockIdx.x * 256 + threadIdx.x, j = blockIdx.y, k = blockIdx.z;
    if (i >= g.Nx) return;
    const long long n = g.idx(i, j, k);
    const double a = num[n], b = den[n];
    double r[4];
    r[BAL_CENTER] = a / b;
    r[BAL_XFACE] = r[BAL_YFACE] = r[BAL_CENTER];
    r[BAL_ZFACE] = 1.0;
    if (L.mask & (1 << BAL_XFACE)) r[BAL_XFACE] = ((a + num[n - 1]) / 2) / ((b + den[n - 1]) / 2);
    if ((L.mask & (1 << BAL_YFACE)) && !g.flat_y) r[BAL_YFACE] = ((a + num[n - g.Sx]) / 2) / ((b + den[n - g.Sx]) / 2);
    const bool zface = (L.mask & (1 << BAL_ZFACE)) && k > 0;
    if (zface) r[BAL_ZFACE] = ((a + num[n - g.Sxy]) / 2) / ((b + den[n - g.Sxy]) / 2);
    for (int fi = 0; fi < L.n; ++fi) {
        const int loc = L.loc[fi];
        if (loc == BAL_ZFACE && !zface) continue;
        const double ratio = loc == BAL_CENTER ? r[BAL_CENTER] : loc == BAL_XFACE ? r[BAL_XFACE] : loc == BAL_YFACE ? r[BAL_YFACE] : r[BAL_ZFACE];
        L.f[fi][n] *= ratio;
    }
}

// _set_dry_density_from_total_density! (set_to_mean.jl:101-105) with total_condensate_density (microphysics_interface.jl:635-639): the
// moisture density plus, with Kessler, rho q^cl + rho q^r — the association k_cmp_diagnose uses for the total density
__global__ __launch_bounds__(256) void k_dry_from_total(DevGrid g, double *__restrict__ rho_d, const double *__restrict__ rho, const double *__restrict__ rq)
{
    const int i = blockIdx.x * 256 + threadIdx.x, j = blockIdx.y, k = blockIdx.z;
    if (i >= g.Nx) return;
    const long long n = g.idx(i, j, k);
    const double S = (g.microphysics == 2) ? rq[n] + (g.rqcl_field[n] + (g.rqr_field[n] + 0.0)) : rq[n] + 0.0;
    rho_d[n] = rho[n] - S;
}

// ---------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------
static int balance_scope(bz_ctx *ctx, const char *what)
{
    if (ctx->dg.bounded_x || ctx->dg.bounded_y) {
        ctx->last_error = std::string(what) + ": not implemented on a Bounded x or y (compressible contexts with lateral walls)";
        return BZ_ERR_UNSUPPORTED;
    }
    if (ctx->slab_mode) {
        ctx->last_error = std::string(what) + ": not implemented on a y-slab context";
        return BZ_ERR_UNSUPPORTED;
    }
    return BZ_OK;
}

static int launch_exner_columns(bz_ctx *ctx, const double *th, const double *qv, const double *qv_den, double p0, double *Pi, double *p, double *rho)
{
    const DevGrid &g = ctx->dg;
    ProfileScope ps(ctx, "exner_columns");
    hipLaunchKernelGGL(k_exner_columns, dim3((g.Nx + 63) / 64, g.Ny), dim3(64), 0, ctx->stream, g, th, qv, qv_den, p0, Pi, p, rho);
    BZ_LAUNCH_CHECK();
    return BZ_OK;
}

static int launch_rescale(bz_ctx *ctx, RescaleList &L, const double *num, const double *den)
{
    const DevGrid &g = ctx->dg;
    L.mask = 0;
    for (int fi = 0; fi < L.n; ++fi) L.mask |= 1 << L.loc[fi];
    ProfileScope ps(ctx, "rescale_density_weighted");
    hipLaunchKernelGGL(k_rescale_density_weighted, dim3((g.Nx + 255) / 256, g.Ny, g.Nz), dim3(256), 0, ctx->stream, g, L, num, den);
    BZ_LAUNCH_CHECK();
    return BZ_OK;
}

extern "C" int bz_exner_columns(bz_ctx *ctx, const double *theta, const double *qv, double p0, double *exner, double *pressure, double *density)
{
    BZ_REQUIRE_COMPRESSIBLE();
    int rc = balance_scope(ctx, "bz_exner_columns");
    if (rc) return rc;
    if (!theta || !exner || !pressure || !density || !(p0 > 0.0)) return BZ_ERR_INVALID;
    return launch_exner_columns(ctx, theta, qv, nullptr, p0, exner, pressure, density);
}

extern "C" int bz_set_hydrostatically_balanced_density(bz_ctx *ctx, const bz_compressible_state *s, double p0)
{
    BZ_REQUIRE_COMPRESSIBLE();
    int rc = balance_scope(ctx, "bz_set_hydrostatically_balanced_density");
    if (rc) return rc;
    if (!valid_state(s) || !(p0 > 0.0)) return BZ_ERR_INVALID;
    if (!ctx->fused_ok) { ctx->last_error = "compressible path needs Nx >= 2Hx and Ny >= 2Hy"; return BZ_ERR_UNSUPPORTED; }
    const DevGrid &g = ctx->dg;
    if (g.microphysics == 2 && (!g.rqcl_field || !g.rqr_field)) return BZ_ERR_INVALID;
    const size_t ncell = (size_t)g.Sxy * (size_t)(g.Nz + 2 * g.Hz);
    // scratch: the old dry density (a copy of the parent array, halos included) and the balanced total density; allocated by the first call —
    // this entry point is part of set!, never of a recorded step
    if (!ctx->d_balance) BZ_HIP(hipMalloc(&ctx->d_balance, 2 * ncell * sizeof(double)));
    double *rd_old = ctx->d_balance, *rho = ctx->d_balance + ncell;
    BZ_HIP(hipMemcpyAsync(rd_old, s->rho_d, ncell * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    // steps 1 + 2: q^v = rho q^v / rho_d_old, column integration -> balanced total density
    if ((rc = launch_exner_columns(ctx, s->theta, s->rho_q, rd_old, p0, nullptr, nullptr, rho))) return rc;
    // step 3: total-density-weighted constituents *= rho / rho_d_old
    RescaleList L;
    L.n = 0;
    L.f[L.n] = s->rho_q; L.loc[L.n++] = BAL_CENTER;
    if (g.microphysics == 2) {
        L.f[L.n] = g.rqcl_field; L.loc[L.n++] = BAL_CENTER;
        L.f[L.n] = g.rqr_field; L.loc[L.n++] = BAL_CENTER;
    }
    if ((rc = launch_rescale(ctx, L, rho, rd_old))) return rc;
    // steps 4 + 5: the dry density as the residual, its halos
    {
        ProfileScope ps(ctx, "dry_from_total");
        hipLaunchKernelGGL(k_dry_from_total, dim3((g.Nx + 255) / 256, g.Ny, g.Nz), dim3(256), 0, ctx->stream, g, s->rho_d, rho, s->rho_q);
        BZ_LAUNCH_CHECK();
    }
    if ((rc = bzi_fill_halo(ctx, s->rho_d, 0))) return rc;
    // step 6: dry-density-weighted prognostics *= rho_d_new / rho_d_old
    L.n = 0;
    L.f[L.n] = s->rho_u; L.loc[L.n++] = BAL_XFACE;
    L.f[L.n] = s->rho_v; L.loc[L.n++] = BAL_YFACE;
    L.f[L.n] = s->rho_w; L.loc[L.n++] = BAL_ZFACE;
    L.f[L.n] = s->rho_theta; L.loc[L.n++] = BAL_CENTER;
    if ((rc = launch_rescale(ctx, L, s->rho_d, rd_old))) return rc;
    // step 7: update_state!(model; compute_tendencies = false)
    return bz_compressible_update_state(ctx, s, nullptr, nullptr, 0);
}

extern "C" int bz_set_exner_reference_state(bz_ctx *ctx, const bz_exner_reference_state *ref)
{
    BZ_REQUIRE_COMPRESSIBLE();
    int rc = balance_scope(ctx, "bz_set_exner_reference_state");
    if (rc) return rc;
    if (!ctx->has_reference) {
        ctx->last_error = "bz_set_exner_reference_state: the context was created without a reference state (reference_state = nothing)";
        return BZ_ERR_INVALID;
    }
    if (!ref || !ref->pressure || !ref->density) return BZ_ERR_INVALID;
    if (ref->standard_pressure != ctx->dg.pst) {
        ctx->last_error = "bz_set_exner_reference_state: the standard pressure is fixed at creation";
        return BZ_ERR_INVALID;
    }
    ++ctx->config_epoch;      // captured steps (bz_graph.hip) belong to one configuration
    return bzi_refresh_reference_columns(ctx, ref->density, ref->pressure);
}

void bzi_balance_teardown(bz_ctx *ctx)
{
    if (ctx->d_balance) (void)hipFree(ctx->d_balance);
    ctx->d_balance = nullptr;
}
