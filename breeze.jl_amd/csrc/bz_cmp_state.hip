// bz_cmp_state.hip — update_state! of CompressibleDynamics (k_cmp_diagnose), the linearisation refresh of the acoustic loop
// (k_cmp_linearization), the compressible context and the Kessler update that ends in update_state!.
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "bz_compressible_internal.h"

// ---------------------------------------------------------------------------------------------------------------------
// update_state!: total density, halos, velocities, theta, q, T (Newton), p   [+ linearisation when LIN]
// ---------------------------------------------------------------------------------------------------------------------
// FULL: everything; !FULL: halos of rho_d, rho_theta, momentum + velocities only (tail of acoustic_rk3_substep_loop!)
// KES: DCMIP2016 Kessler species — total density includes rho q^cl + rho q^r, q = (q^v, q^cl + q^r) in R_m, c_pm and the
// latent term of the temperature inversion, q^cl / q^r / q^v diagnosed (dcmip2016_kessler.jl:222-227,298-303,860-865)
// MP = 1: SaturationAdjustment(WarmPhaseEquilibrium) on the density-based state — rho q is the total moisture, q^v / q^l are
// diagnosed by bz_ds_adjust at the cell's own total density and the temperature is the same Newton inversion with the latent
// term (compressible_time_stepping.jl:191-250; saturation_adjustment.jl:236-301)
// MP = 3: MP = 1 with saturation_vapor_pressure = FlatauPolynomial (bz_set_saturation_vapor_pressure_polynomial): bz_ds_adjust<true>
// MP = 4: SaturationAdjustment(MixedPhaseEquilibrium(T^f, T^h)) (bz_set_compressible_mixed_phase_equilibrium): bz_ds_adjust_mixed diagnoses
// q^v, q^l and q^i; R_m, c_pm, the pressure and (LIN) the linearisation carry the ice fraction (acoustic_substepping.jl:390-410);
// MP = 5: MP = 4 on the FlatauPolynomial surface.  The host picks the instantiation (bzi_cmp_mp): MP <= 3 read no mixed-phase member.
// WY: walls in y (topology (Periodic, Bounded, Bounded), dry or vapour-carrying models).  The halo writes follow the conventions of
// DESIGN section 6 "Walls in y" instead of periodic images: a field that is a centre in y gets the no-flux copy of rows 0 and Ny - 1 in its
// first halo rows (oy = one row down / up for those two rows), rho v and v get exact zeros on their wall faces 0 and Ny (face Ny is the first
// upper halo row).  Row 0 reads no y neighbour: its face density is the no-flux mean (rho_d itself) and its v the wall's zero — the halo row
// below it is written by this launch.  x stays periodic, z is unchanged.  WY = false compiles to the code it replaced.
template <bool FULL, bool LIN, int MP = 0, bool WY = false>
__global__ __launch_bounds__(256) void k_cmp_diagnose(DevGrid g, DiagFields F, double abstol, int maxiter, const double *fl)
{
    constexpr bool KES = (MP == 2), MIX = (MP == 4 || MP == 5), SA = (MP == 1 || MP == 3 || MIX), FL = (MP == 3 || MP == 5);
    static_assert(!WY || (MP == 0 && !LIN), "walls in y: no microphysics; the linearisation is refreshed by its own kernel (halo rows)");
    const int i = blockIdx.x * 256 + threadIdx.x, j = blockIdx.y, k = blockIdx.z;
    if (i >= g.Nx) return;
    const long long sz = g.Sxy;
    const WrapIdx W = wrap_of(g, i, j);
    const bool south = WY && j == 0, north = WY && j == g.Ny - 1;
    const long long ox = W.ox, oy = !WY ? W.oy : south ? -(long long)g.Sx : north ? (long long)g.Sx : 0;
    const long long n = g.idx(i, j, k);
    const bool bot = (k == 0), top = (k == g.Nz - 1);

    const double rd = F.rho_d[n];
    const double rdx = (rd + F.rho_d[n + W.im]) / 2.0;
    const double rdy = south ? rd : (rd + F.rho_d[n + W.jm]) / 2.0;
    const double ru = F.ru[n], rv = south ? 0.0 : F.rv[n];
    const double u = ru / rdx, v = south ? 0.0 : rv / rdy;
    const double rth = F.rth[n];
    st_img_only(F.rho_d, n, rd, ox, oy);
    st_img_only(F.ru, n, ru, ox, oy);
    if constexpr (WY) st_yface_w(g, F.rv, n, rv, ox, south, north);
    else st_img_only(F.rv, n, rv, ox, oy);
    st_img_only(F.rth, n, rth, ox, oy);
    st_img(F.u, n, u, ox, oy);
    if constexpr (WY) st_yface_w(g, F.v, n, v, ox, true, north);
    else st_img(F.v, n, v, ox, oy);
    if (!bot) {
        const double rw = F.rw[n];
        const double rdz = (rd + F.rho_d[n - sz]) / 2.0;
        st_img_only(F.rw, n, rw, ox, oy);
        st_img(F.w, n, rw / rdz, ox, oy);
    } else {
        st_img(F.rw, n, 0.0, ox, oy);      // impenetrable walls
        st_img(F.w, n, 0.0, ox, oy);
    }
    if (top) {
        st_img(F.rw, n + sz, 0.0, ox, oy);
        st_img(F.w, n + sz, 0.0, ox, oy);
    }
    double r = 0.0, q = 0.0, th = 0.0, T = 0.0, p = 0.0, rq = 0.0, qcl_v = 0.0, qr_v = 0.0, sa_qv = 0.0, sa_ql = 0.0, sa_qi = 0.0;
    if (FULL) {
        rq = F.rq[n];
        double rqcl = 0.0, rqr = 0.0, ql = 0.0;
        if (KES) {
            rqcl = g.rqcl_field[n];
            rqr = g.rqr_field[n];
            r = rd + (rq + (rqcl + (rqr + 0.0)));
        } else {
            r = rd + (rq + 0.0);
        }
        th = rth / rd;
        q = rq / r;
        if (KES) {
            qcl_v = rqcl / r;
            qr_v = rqr / r;
            ql = qcl_v + qr_v;
        }
        double qvap = q;        // vapour fraction of the mixture constants (q itself unless the adjustment partitions it)
        if constexpr (MIX) {
            T = bz_ds_adjust_mixed<FL>(g, th, q, r, abstol, maxiter, qvap, ql, sa_qi, ColPtr(fl));
            st_img(g.qv_field, n, qvap, ox, oy);
            st_img(g.ql_field, n, ql, ox, oy);
            st_img(g.qi_field, n, sa_qi, ox, oy);
            sa_qv = qvap; sa_ql = ql;
        } else if (SA) {
            T = bz_ds_adjust<FL>(g, th, q, r, abstol, maxiter, qvap, ql, ColPtr(fl));
            st_img(g.qv_field, n, qvap, ox, oy);
            st_img(g.ql_field, n, ql, ox, oy);
            sa_qv = qvap; sa_ql = ql;
        }
        const double qd = MIX ? 1.0 - (qvap + ql + sa_qi) : 1.0 - (qvap + ql);
        const double Rm = qd * g.Rd + qvap * g.Rv;
        const double cpm = MIX ? qd * g.cpd + qvap * g.cpv + ql * g.sa_cl + sa_qi * g.sa_ci
                               : (KES || SA) ? qd * g.cpd + qvap * g.cpv + ql * g.sa_cl : qd * g.cpd + qvap * g.cpv;
        if (!SA) {
            const double kap = Rm / cpm;
            const double gam = cpm / (cpm - Rm);
            const double Lt = KES ? (g.sa_Ll * ql) / cpm : 0.0;
            T = pow(th, gam) * pow(r * Rm / g.pst, gam - 1.0) + Lt;
            double dT = T;
            for (int it = 0; it < maxiter && fabs(dT) > abstol; ++it) {
                const double Phi = pow(r * Rm * T / g.pst, kap) * th;
                dT = -(T - Phi - Lt) / (1.0 - kap * Phi / T);
                T += dT;
            }
        }
        p = r * Rm * T;
        if (KES) {
            st_img_only(g.rqcl_field, n, rqcl, ox, oy);
            st_img_only(g.rqr_field, n, rqr, ox, oy);
            st_img(g.qcl_field, n, qcl_v, ox, oy);
            st_img(g.qr_field, n, qr_v, ox, oy);
            st_img(g.qv_field, n, q, ox, oy);
        }
        st_img_only(F.rq, n, rq, ox, oy);
        st_img(F.rho, n, r, ox, oy);
        st_img(F.theta, n, th, ox, oy);
        st_img(F.q, n, q, ox, oy);
        st_img(F.T, n, T, ox, oy);
        st_img(F.p, n, p, ox, oy);
        if (LIN) {
            const double Pi = pow(p / g.pst, g.Rd / g.cpd);
            const double thl = rth / ((rd == 0.0) ? 1.0 : rd);
            const double gr = cpm * Rm / (cpm - Rm);
            st_store(F.Pi, n, Pi, F.st32);
            st_store(F.thL, n, thl, F.st32);
            st_store(F.gR, n, gr, F.st32);
            st_store(F.Clin, n, gr * Pi, F.st32);
        }
    }
    if (bot || top) {     // first z-halo cell of the no-flux centre fields
        const long long h = bot ? -sz : sz;
        st_img(F.rho_d, n + h, rd, ox, oy);
        st_img(F.ru, n + h, ru, ox, oy);
        if constexpr (WY) st_yface_w(g, F.rv, n + h, rv, ox, true, north);
        else st_img(F.rv, n + h, rv, ox, oy);
        st_img(F.rth, n + h, rth, ox, oy);
        st_img(F.u, n + h, u, ox, oy);
        if constexpr (WY) st_yface_w(g, F.v, n + h, v, ox, true, north);
        else st_img(F.v, n + h, v, ox, oy);
        if (FULL) {
            st_img(F.rq, n + h, rq, ox, oy);
            st_img(F.rho, n + h, r, ox, oy);
            st_img(F.theta, n + h, th, ox, oy);
            st_img(F.q, n + h, q, ox, oy);
            st_img(F.T, n + h, T, ox, oy);
            st_img(F.p, n + h, p, ox, oy);
            if (SA) {
                st_img(g.qv_field, n + h, sa_qv, ox, oy);
                st_img(g.ql_field, n + h, sa_ql, ox, oy);
            }
            if constexpr (MIX) st_img(g.qi_field, n + h, sa_qi, ox, oy);
            if (KES) {
                st_img(g.rqcl_field, n + h, g.rqcl_field[n], ox, oy);
                st_img(g.rqr_field, n + h, g.rqr_field[n], ox, oy);
                st_img(g.qcl_field, n + h, qcl_v, ox, oy);
                st_img(g.qr_field, n + h, qr_v, ox, oy);
                st_img(g.qv_field, n + h, q, ox, oy);
            }
        }
    }
}

// refresh_linearization_basic_state! (acoustic_substepping.jl:318-399); MIX: the mixed-phase instantiation, q^d = 1 - q^v - q^l - q^i and
// c_pm with c_i q^i (acoustic_substepping.jl:390-410) — the host selects it by DevGrid::sa_mixed, MIX = false reads no ice member
template <bool MIX>
__global__ __launch_bounds__(256) void k_cmp_linearization(DevGrid g, double *__restrict__ Pi, double *__restrict__ thL,
                                                           double *__restrict__ gR, double *__restrict__ Clin,
                                                           const double *__restrict__ p, const double *__restrict__ rho_d,
                                                           const double *__restrict__ rth, const double *__restrict__ qv, int st32, int hrows,
                                                           int hcols)
{
    // y-slab mode: hrows halo rows on each side are linearised locally (their inputs arrive with the state's halo exchange): one for
    // the substep kernels, two with DirectDivergenceDamping, whose delta of row -1 averages theta_L of rows -2 and -1
    // Bounded x / y: one halo column / row each side holds the zero-gradient copy of the adjacent interior cell — the fill_halo_regions! of
    // acoustic_substepping.jl:365-367 on fields with default boundary conditions: the value is formed from the state of that interior cell
    const int i = (int)(blockIdx.x * 256 + threadIdx.x) - hcols, j = (int)blockIdx.y - hrows, k = blockIdx.z;
    if (i >= g.Nx + hcols) return;
    const long long nd = g.idx(i, j, k);
    const int is = g.bounded_x ? min(max(i, 0), g.Nx - 1) : i, js = g.bounded_y ? min(max(j, 0), g.Ny - 1) : j;
    const long long n = g.idx(is, js, k);
    const double rd = rho_d[n];
    const double q = (g.microphysics == 1) ? g.qv_field[n] : qv[n];
    const double ql = (g.microphysics == 2) ? g.qcl_field[n] + g.qr_field[n] : ((g.microphysics == 1) ? g.ql_field[n] : 0.0);
    double qi = 0.0;
    if constexpr (MIX) qi = g.qi_field[n];
    const double qd = MIX ? 1.0 - q - ql - qi : 1.0 - q - ql;
    const double Rm = qd * g.Rd + q * g.Rv;
    const double cpm = MIX ? qd * g.cpd + q * g.cpv + ql * g.sa_cl + qi * g.sa_ci
                           : g.microphysics ? qd * g.cpd + q * g.cpv + ql * g.sa_cl : qd * g.cpd + q * g.cpv;
    const double P = pow(p[n] / g.pst, g.Rd / g.cpd);
    const double gr = cpm * Rm / (cpm - Rm);
    st_store(Pi, nd, P, st32);
    st_store(thL, nd, rth[n] / ((rd == 0.0) ? 1.0 : rd), st32);
    st_store(gR, nd, gr, st32);
    st_store(Clin, nd, gr * P, st32);
}

// ---------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------
static int bzi_create_compressible(bz_ctx **out, const bz_grid *grid, const bz_constants *constants,
                                   const bz_exner_reference_state *ref, const bz_split_explicit *td, int weno_order,
                                   int y_nranks, int y_rank, bool slab)
{
    if (!out || !grid || !constants || !ref || !td) return BZ_ERR_INVALID;
    if ((ref->pressure == nullptr) != (ref->density == nullptr)) return BZ_ERR_INVALID;
    if (td->substeps < 0 || !(td->acoustic_cfl > 0.0) || td->newton_maxiter < 0) return BZ_ERR_INVALID;
    if (td->sponge_ramp < 0 || td->sponge_ramp > 3 || (td->sponge_ramp && !(td->sponge_depth > 0.0))) return BZ_ERR_INVALID;
    if (td->substep_distribution < 0 || td->substep_distribution > 2) return BZ_ERR_INVALID;
    // substep_floattype: 0 = eltype(grid); 4 = Float32 working fields (inside a Float64 model: half the bytes; in the Float32 library: eltype)
    if (td->substep_float_bytes != 0 && td->substep_float_bytes != 4 && td->substep_float_bytes != (int32_t)sizeof(double)) return BZ_ERR_UNSUPPORTED;
    if (td->substep_float_bytes == 4 && sizeof(double) == 8 && td->direct_divergence_damping) return BZ_ERR_UNSUPPORTED;   // its two kernels read the working fields as the grid's real
    const int nc = grid->Nz + 2 * grid->Hz;
    std::vector<double> zeros((size_t)nc, 0.0);
    bz_reference_state r;
    r.surface_pressure = 0.0;
    r.potential_temperature = 0.0;
    r.standard_pressure = ref->standard_pressure;
    r.density = ref->density ? ref->density : zeros.data();
    r.pressure = ref->pressure ? ref->pressure : zeros.data();
    r.temperature = zeros.data();
    int rc = bzi_create(out, grid, constants, &r, weno_order, y_nranks, y_rank, slab, true);
    if (rc != BZ_OK) return rc;
    bz_ctx *ctx = *out;
    ctx->se = *td;
    ctx->has_reference = ref->density != nullptr;
    const size_t ncell = (size_t)ctx->dg.Sxy * (size_t)nc;
    ctx->ac_fused = !ctx->tune.no_ac_fuse;
    ctx->substep_f32 = (td->substep_float_bytes == 4) && sizeof(double) == 8;
    if (hipMalloc(&ctx->d_Clin, ncell * sizeof(double)) != hipSuccess ||
        hipMalloc(&ctx->d_tfac_ac, ncell * sizeof(double)) != hipSuccess ||
        hipMalloc(&ctx->d_up2, ncell * sizeof(double)) != hipSuccess ||
        hipMalloc(&ctx->d_thL2, ncell * sizeof(double)) != hipSuccess ||
        hipMalloc(&ctx->d_vp2, ncell * sizeof(double)) != hipSuccess ||
        (ctx->tune.ac_pfold && (hipMalloc(&ctx->d_Gp_ru, ncell * sizeof(double)) != hipSuccess ||
                                hipMalloc(&ctx->d_Gp_rv, ncell * sizeof(double)) != hipSuccess))) {
        bz_destroy(ctx);
        *out = nullptr;
        return BZ_ERR_ALLOC;
    }
    if (ctx->d_Gp_ru) {
        (void)hipMemset(ctx->d_Gp_ru, 0, ncell * sizeof(double));
        (void)hipMemset(ctx->d_Gp_rv, 0, ncell * sizeof(double));
    }
    (void)hipMemset(ctx->d_Clin, 0, ncell * sizeof(double));
    (void)hipMemset(ctx->d_tfac_ac, 0, ncell * sizeof(double));
    (void)hipMemset(ctx->d_up2, 0, ncell * sizeof(double));
    (void)hipMemset(ctx->d_thL2, 0, ncell * sizeof(double));
    (void)hipMemset(ctx->d_vp2, 0, ncell * sizeof(double));
    // UpperSponge profile on the faces: rate * ramp(z, grid.Lz, depth), ramp = 0 below Lz - depth and 1 at z = Lz
    // (time_discretizations.jl:398-433; the reference passes grid.Lz as the sponge top, whatever z[0] is)
    std::vector<double> sp((size_t)grid->Nz + 1, 0.0);
    if (td->sponge_ramp) {
        const double Lz = grid->zf[grid->Nz] - grid->zf[0], depth = td->sponge_depth, pi = 3.14159265358979323846;
        for (int k = 0; k <= grid->Nz; ++k) {
            double sN = (grid->zf[k] - (Lz - depth)) / depth;
            sN = sN < 0.0 ? 0.0 : (sN > 1.0 ? 1.0 : sN);
            const double ramp = td->sponge_ramp == 1 ? sN : td->sponge_ramp == 2 ? sN * sN * (3.0 - 2.0 * sN) : std::sin(pi / 2.0 * sN) * std::sin(pi / 2.0 * sN);
            sp[k] = td->sponge_damping_rate * ramp;
        }
    }
    if (hipMalloc(&ctx->d_sponge, sp.size() * sizeof(double)) != hipSuccess) {
        bz_destroy(ctx);
        *out = nullptr;
        return BZ_ERR_ALLOC;
    }
    BZ_HIP(hipMemcpy(ctx->d_sponge, sp.data(), sp.size() * sizeof(double), hipMemcpyHostToDevice));
    return BZ_OK;
}

extern "C" int bz_create_compressible(bz_ctx **out, const bz_grid *grid, const bz_constants *constants,
                                      const bz_exner_reference_state *ref, const bz_split_explicit *td, int weno_order)
{
    return bzi_create_compressible(out, grid, constants, ref, td, weno_order, 1, 0, false);
}

extern "C" int bz_create_compressible_slab(bz_ctx **out, const bz_grid *local_grid, const bz_constants *constants,
                                           const bz_exner_reference_state *ref, const bz_split_explicit *td, int weno_order,
                                           int y_nranks, int y_rank)
{
    // substep_floattype = Float32 inside a Float64 model: the per-substep halo messages carry the Float32 rows as Sx / 2 doubles (bz_comm.hip:
    // halo_exchange, half) — the row length must be even; library-owned communicators only (the host-driven exchange moves the grid's real)
    if (td && td->substep_float_bytes == 4 && sizeof(double) == 8 && local_grid && ((local_grid->Nx + 2 * local_grid->Hx) & 1)) return BZ_ERR_UNSUPPORTED;
    if (y_nranks < 1 || y_rank < 0 || y_rank >= y_nranks) return BZ_ERR_INVALID;
    return bzi_create_compressible(out, local_grid, constants, ref, td, weno_order, y_nranks, y_rank, true);
}

void bzi_compressible_teardown(bz_ctx *ctx)
{
    if (ctx->d_Clin) (void)hipFree(ctx->d_Clin);
    if (ctx->d_tfac_ac) (void)hipFree(ctx->d_tfac_ac);
    if (ctx->d_up2) (void)hipFree(ctx->d_up2);
    if (ctx->d_thL2) (void)hipFree(ctx->d_thL2);
    ctx->d_thL2 = nullptr;
    if (ctx->d_vp2) (void)hipFree(ctx->d_vp2);
    if (ctx->d_sponge) (void)hipFree(ctx->d_sponge);
    if (ctx->d_Gp_ru) (void)hipFree(ctx->d_Gp_ru);
    if (ctx->d_Gp_rv) (void)hipFree(ctx->d_Gp_rv);
    ctx->d_Gp_ru = ctx->d_Gp_rv = nullptr;
    ctx->d_Clin = ctx->d_tfac_ac = ctx->d_up2 = ctx->d_vp2 = ctx->d_sponge = nullptr;
    bzi_cmp_surface_flux_teardown(ctx);
}

// update_state! with the linearisation refresh of the next stage optionally folded in
int bzi_compressible_update_state(bz_ctx *ctx, const bz_compressible_state *s, const bz_compressible_prognostic *G,
                                  const bz_acoustic_substepper *sub, bool compute_tendencies, bool with_linearization)
{
    const DevGrid &g = ctx->dg;
    {
        ProfileScope ps(ctx, with_linearization ? "update_state+linearization" : "update_state");
        DiagFields F = diag_fields(ctx, s, sub);
        if (with_linearization) ctx->thL_alt = false;      // theta_L of the next stage goes to the caller's array
        dim3 grid((g.Nx + 255) / 256, g.Ny, g.Nz), block(256);
        const double na = ctx->se.newton_abstol;
        const int nm = ctx->se.newton_maxiter;
        if (g.bounded_y) hipLaunchKernelGGL((k_cmp_diagnose<true, false, 0, true>), grid, block, 0, ctx->stream, g, F, na, nm, bzi_flatau(ctx));
        else bz_bools([&](auto lin) {
            constexpr bool LIN = lin();
            bz_static_int<6>(bzi_cmp_mp(ctx), [&](auto mp) { hipLaunchKernelGGL((k_cmp_diagnose<true, LIN, mp()>), grid, block, 0, ctx->stream, g, F, na, nm, bzi_flatau(ctx)); });
        }, with_linearization);
        BZ_LAUNCH_CHECK();
    }
    // Nx < 2 Hx or Ny < 2 Hy (small_grid_update_ok): k_cmp_diagnose has stored one periodic image per direction where a cell has two; what it
    // computed in the interior is complete, the halos of everything it produced are filled again by the generic kernels
    if (!ctx->fused_ok && small_grid(g) && !g.bounded_y && !ctx->slab_mode) {
        double *fa[7] = {s->rho_d, s->rho, s->rho_u, s->rho_v, s->rho_w, s->rho_theta, s->rho_q};
        const int ka[7] = {0, 0, 0, 0, 1, 0, 0};
        double *fb[7] = {s->u, s->v, s->w, s->theta, s->q, s->T, s->p};
        const int kb[7] = {0, 0, 3, 0, 0, 0, 0};
        int rc = bzi_fill_halos_multi(ctx, fa, ka, 7);
        if (!rc) rc = bzi_fill_halos_multi(ctx, fb, kb, 7);
        if (rc) return rc;
    }
    // walls in y: the linearisation of the next stage by its own kernel, which also forms the zero-gradient halo rows the substeps read
    if (g.bounded_y && with_linearization) {
        const int rc = bz_refresh_linearization(ctx, s, sub);
        if (rc) return rc;
    }
    // compute_closure_fields! closes compute_auxiliary_variables! (update_atmosphere_model_state.jl:218): after velocities, T and p and their
    // halos, before the tendencies of this update_state!
    if (ctx->has_closure || ctx->has_diffusivity) {
        const int rc = bzi_cmp_closure_fields(ctx, s);
        if (rc) return rc;
    }
    if (compute_tendencies) return bz_compute_moisture_tendency(ctx, s, G, sub);
    return BZ_OK;
}

// the tail of acoustic_rk3_substep_loop!: halo images of rho_d, rho theta and the momentum + compute_velocities!
int bzi_compressible_velocities(bz_ctx *ctx, const bz_compressible_state *s, const bz_acoustic_substepper *sub)
{
    const DevGrid &g = ctx->dg;
    ProfileScope ps(ctx, "acoustic_velocities");
    DiagFields D = diag_fields(ctx, s, sub);
    if (g.bounded_y) hipLaunchKernelGGL((k_cmp_diagnose<false, false, 0, true>), dim3((g.Nx + 255) / 256, g.Ny, g.Nz), dim3(256), 0, ctx->stream, g, D, 0.0, 0, nullptr);
    else hipLaunchKernelGGL((k_cmp_diagnose<false, false>), dim3((g.Nx + 255) / 256, g.Ny, g.Nz), dim3(256), 0, ctx->stream, g, D, 0.0, 0, nullptr);
    BZ_LAUNCH_CHECK();
    return BZ_OK;
}

extern "C" int bz_compressible_update_state(bz_ctx *ctx, const bz_compressible_state *s, const bz_compressible_prognostic *G,
                                            const bz_acoustic_substepper *sub, int compute_tendencies)
{
    BZ_REQUIRE_COMPRESSIBLE();
    BZ_REJECT_WALLS("bz_compressible_update_state");
    BZ_REJECT_Y_WALL_OPTIONS("bz_compressible_update_state");
    if (!valid_state(s)) return BZ_ERR_INVALID;
    if (compute_tendencies && (!valid_prog(G) || !valid_sub(sub))) return BZ_ERR_INVALID;
    if (!ctx->fused_ok && !small_grid_update_ok(ctx)) { ctx->last_error = "compressible path needs Nx >= 2Hx and Ny >= 2Hy"; return BZ_ERR_UNSUPPORTED; }
    if (ctx->d_qstate) BZ_HIP(hipMemsetAsync(ctx->d_qstate, 0, sizeof(int), ctx->stream));      // moisture scan: unknown again (set! ends here)
    bzi_moisture_unknown(ctx);
    return bzi_compressible_update_state(ctx, s, G, sub, compute_tendencies != 0, false);
}

extern "C" int bz_refresh_linearization(bz_ctx *ctx, const bz_compressible_state *s, const bz_acoustic_substepper *sub)
{
    BZ_REQUIRE_COMPRESSIBLE();
    if (!valid_state(s) || !valid_sub(sub)) return BZ_ERR_INVALID;
    const DevGrid &g = ctx->dg;
    ProfileScope ps(ctx, "refresh_linearization");
    ctx->thL_alt = false;
    const int hrows = g.wrap_y ? 0 : g.bounded_y ? 1 : ((ctx->se.direct_divergence_damping && ctx->se.damping_coefficient >= 0.0) ? 2 : 1);
    const int hcols = g.bounded_x ? 1 : 0;
    dim3 grid((g.Nx + 2 * hcols + 255) / 256, g.Ny + 2 * hrows, g.Nz), block(256);
    bz_bools([&](auto mix) {
        hipLaunchKernelGGL(k_cmp_linearization<mix()>, grid, block, 0, ctx->stream, g, sub->exner, sub->potential_temperature,
                           sub->gamma_R_mixture, ctx->d_Clin, s->p, s->rho_d, s->rho_theta, s->q, ctx->substep_f32 ? 1 : 0, hrows, hcols);
    }, g.sa_mixed != 0);
    BZ_LAUNCH_CHECK();
    return BZ_OK;
}

extern "C" int bz_seed_time_averaged_velocities(bz_ctx *ctx, const bz_compressible_state *s, const bz_acoustic_substepper *sub)
{
    BZ_REQUIRE_COMPRESSIBLE();
    if (!valid_state(s) || !valid_sub(sub)) return BZ_ERR_INVALID;
    const DevGrid &g = ctx->dg;
    const size_t nc = (size_t)g.Sxy * (size_t)(g.Nz + 2 * g.Hz) * sizeof(double);
    const size_t nf = (size_t)g.Sxy * (size_t)(g.Nz + 1 + 2 * g.Hz) * sizeof(double);
    BZ_HIP(hipMemcpyAsync(sub->time_averaged_u, s->u, nc, hipMemcpyDeviceToDevice, ctx->stream));
    BZ_HIP(hipMemcpyAsync(sub->time_averaged_v, s->v, nc, hipMemcpyDeviceToDevice, ctx->stream));
    BZ_HIP(hipMemcpyAsync(sub->time_averaged_w, s->w, nf, hipMemcpyDeviceToDevice, ctx->stream));
    return BZ_OK;
}

// microphysics_model_update!(::DCMIP2016KesslerMicrophysics, model) for CompressibleDynamics: density = dynamics_density
// (rho_d), pressure = dynamics.pressure (dcmip2016_kessler.jl:460-485), then update_state!(model)
extern "C" int bz_compressible_kessler_update(bz_ctx *ctx, const bz_compressible_state *s, const bz_compressible_prognostic *G,
                                              const bz_acoustic_substepper *sub, double dt)
{
    BZ_REQUIRE_COMPRESSIBLE();
    BZ_REJECT_WALLS("bz_compressible_kessler_update");
    if (!valid_state(s) || !valid_prog(G) || !valid_sub(sub)) return BZ_ERR_INVALID;
    if (ctx->dg.microphysics != 2) { ctx->last_error = "bz_compressible_kessler_update: no Kessler microphysics attached"; return BZ_ERR_INVALID; }
    const int rc = bzi_kessler_columns(ctx, s->theta, s->rho_theta, s->rho_q, s->rho_d, s->p, dt);
    if (rc) return rc;
    // the columns are rank-local; on a y-slab the update_state! that follows needs the neighbour exchanges of the driver
    if (ctx->slab_mode) return BZ_OK;
    return bzi_compressible_update_state(ctx, s, G, sub, true, false);
}
