// bz_acoustic.hip — host side of the acoustic substep loop: substep counts, the stage in three pieces (begin / substep / end, which the y-slab
// driver interleaves with its halo exchanges), lateral walls and open boundaries, DirectDivergenceDamping and the per-stage C entry points.
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "bz_acoustic_kernels.h"

// compute_acoustic_substeps / stage_substep_count_and_size(::ProportionalSubsteps) (acoustic_substepping.jl:451-495)
static int acoustic_substeps_for(const bz_ctx *ctx, double dt)
{
    const double Rd = ctx->constants.dry_air_gas_constant, cpd = ctx->constants.dry_air_heat_capacity;
    const double gam = cpd / (cpd - Rd);
    const double cs = std::sqrt(gam * Rd * 300.0);
    const double dmin = ctx->dg.flat_y ? ctx->dg.dx : std::fmin(ctx->dg.dx, ctx->dg.dy);      // Flat directions do not bound the acoustic CFL (acoustic_substepping.jl:458-465)
    const double n = std::ceil(std::fabs(dt) * cs / (ctx->se.acoustic_cfl * dmin));
    return (int)std::fmax(1.0, n);
}

extern "C" int bz_stage_substeps(bz_ctx *ctx, double dt, double beta, int32_t *n_substeps, double *dtau)
{
    BZ_REQUIRE_COMPRESSIBLE();
    const double dt_stage = beta * dt;
    int n;
    double dtau_v;
    const int dist = ctx->se.substep_distribution;
    if (dist == 2 && beta < (1.0 / 3.0 + 1.0 / 2.0) / 2.0) {      // MonolithicFirstStage: stage 1 collapses to one substep of dt / 3 (:503-508)
        n = 1;
        dtau_v = dt / 3.0;
    } else if (dist == 1 || dist == 2) {      // ConstantSubstepSize (:497-501): one size dt / N for all stages, N a multiple of 6 so that beta N is integral
        const int n_raw = ctx->se.substeps > 0 ? ctx->se.substeps : acoustic_substeps_for(ctx, dt);
        const int N = std::max(6, 6 * ((n_raw + 5) / 6));
        n = std::max(1, (int)std::lround(beta * (double)N));
        dtau_v = dt / (double)N;
    } else {                                  // ProportionalSubsteps (:491-495)
        if (ctx->se.substeps > 0) n = (int)std::fmax(1.0, std::ceil(beta * (double)ctx->se.substeps));
        else n = acoustic_substeps_for(ctx, dt_stage);
        dtau_v = dt_stage / (double)n;
    }
    if (n_substeps) *n_substeps = n;
    if (dtau) *dtau = dtau_v;
    return BZ_OK;
}

static AcFields ac_fields(bz_ctx *ctx, const bz_compressible_state *s, const bz_compressible_prognostic *U0,
                          const bz_compressible_prognostic *G, const bz_acoustic_substepper *a)
{
    AcFields F;
    F.rho_d = s->rho_d; F.rth = s->rho_theta; F.ru = s->rho_u; F.rv = s->rho_v; F.rw = s->rho_w; F.rq = s->rho_q;
    F.rho = s->rho; F.p = s->p;
    F.U0_rho_d = U0->rho_d; F.U0_rth = U0->rho_theta; F.U0_ru = U0->rho_u; F.U0_rv = U0->rho_v; F.U0_rw = U0->rho_w; F.U0_rq = U0->rho_q;
    F.G_rho_d = G->rho_d; F.G_rth = G->rho_theta; F.G_ru = G->rho_u; F.G_rv = G->rho_v; F.G_rw = G->rho_w; F.G_rq = G->rho_q;
    F.thL = ctx->thL_alt ? ctx->d_thL2 : a->potential_temperature; F.Clin = ctx->d_Clin;
    F.rp = a->density_perturbation; F.rthp = a->density_potential_temperature_perturbation;
    F.rup = a->momentum_perturbation_u; F.rvp = a->momentum_perturbation_v; F.rwp = a->momentum_perturbation_w;
    F.rs = a->density_predictor; F.rths = a->density_potential_temperature_predictor;
    F.rth_old = a->previous_density_potential_temperature_perturbation;
    F.au = a->time_averaged_u; F.av = a->time_averaged_v; F.aw = a->time_averaged_w;
    F.Gs = a->slow_vertical_momentum_tendency; F.phi = a->vertical_solver_source_term;
    F.tfac = ctx->d_tfac_ac;
    F.sponge = ctx->d_sponge;
    F.rup_in = F.rup; F.rvp_in = F.rvp; F.rthp_out = F.rthp;
    F.Gp_ru = ctx->d_Gp_ru; F.Gp_rv = ctx->d_Gp_rv;
    const bz_kessler_model_fields &K = ctx->kessler;
    F.rqcl = K.cloud_liquid_density; F.rqr = K.rain_density;
    F.U0_rqcl = K.U0_cloud_liquid_density; F.U0_rqr = K.U0_rain_density;
    F.G_rqcl = K.G_cloud_liquid_density; F.G_rqr = K.G_rain_density;
    return F;
}

// k_ac_forward2 addresses every array by a 32-bit byte offset from its base and fetches the outer x neighbours of a row's two edge lanes
// with one load: arrays below 4 GB, two z halo levels (its ring words are requested two levels ahead), no row whose first lane is its last
static bool ac_forward2_ok(const bz_ctx *ctx)
{
    const DevGrid &g = ctx->dg;
    const unsigned long long bytes = (unsigned long long)g.Sxy * (unsigned long long)(g.Nz + 2 * g.Hz + 1) * sizeof(double);
    return ctx->tune.ac_forward2 && bytes < (1ull << 32) && g.Hz >= 1 && g.Nx >= 2 && (g.Nx % 64) != 1 && !g.bounded_x && !g.bounded_y;
}
// ---- lateral walls / open boundaries (Bounded x and / or y) ----
// fill_halo_regions! of a substepper field that is a centre along the Bounded directions: one zero-gradient halo row / column
template <class T>
static void fill_walls(bz_ctx *ctx, T *f)
{
    const DevGrid &g = ctx->dg;
    const int n = (g.bounded_y ? 2 * g.Nx : 0) + (g.bounded_x ? 2 * g.Ny : 0);
    if (!n) return;
    hipLaunchKernelGGL((k_ac_fill_walls<T>), dim3((n + 255) / 256, g.Nz), dim3(256), 0, ctx->stream, g, f);
}
static void fill_walls_st(bz_ctx *ctx, double *f)      // a working field in the substep storage type
{
    ac_storage(ctx, [&](auto st) { fill_walls(ctx, (typename decltype(st)::type *)f); });
}
// apply_open_boundary_relaxation! (acoustic_substepping.jl:1339-1361) on rho' and the current (rho theta)'
static void relax_open_boundaries(bz_ctx *ctx, const AcFields &F, double *rthp_cur)
{
    const DevGrid &g = ctx->dg;
    const double a = ctx->ac_open_relax;
    auto launch = [&](int dir, int cb, int ch) {
        const int n = dir ? g.Nx : g.Ny;
        dim3 grid((n + 255) / 256, g.Nz), block(256);
        ac_storage(ctx, [&](auto st) {
            using ST = typename decltype(st)::type;
            hipLaunchKernelGGL((k_ac_relax_open_boundary<ST>), grid, block, 0, ctx->stream, g, (ST *)F.rp, (ST *)rthp_cur, F.rho_d, F.rth, dir, cb, ch, a);
        });
    };
    if (g.bounded_x && ctx->ac_open[0]) launch(0, 0, -1);
    if (g.bounded_x && ctx->ac_open[1]) launch(0, g.Nx - 1, g.Nx);
    if (g.bounded_y && ctx->ac_open[2]) launch(1, 0, -1);
    if (g.bounded_y && ctx->ac_open[3]) launch(1, g.Ny - 1, g.Ny);
}
static void stage_buffers(bz_ctx *ctx, const AcFields &F, double *th_buf[2], double *u_buf[2], double *v_buf[2])
{
    // ping-pong buffers of the fused substep: the start buffers are chosen by the parity of N_tau so that the final
    // (rho theta)', (rho u)', (rho v)' land in the substepper's own fields (and the previous (rho theta)' in
    // previous_density_potential_temperature_perturbation, as in the reference).
    th_buf[0] = F.rthp; th_buf[1] = F.rth_old;
    u_buf[0] = F.rup; u_buf[1] = ctx->up2_user ? ctx->up2_user : ctx->d_up2;
    v_buf[0] = F.rvp; v_buf[1] = ctx->vp2_user ? ctx->vp2_user : ctx->d_vp2;
}

// apply_divergence_damping!(::DirectDivergenceDamping) on the current perturbation buffers
static int direct_damping(bz_ctx *ctx, const AcFields &F, const bz_acoustic_substepper *sub)
{
    const DevGrid &g = ctx->dg;
    const AcStage &S = stage_of(ctx);
    ProfileScope ps(ctx, "acoustic_direct_damping");
    double *th_buf[2], *u_buf[2], *v_buf[2];
    stage_buffers(ctx, F, th_buf, u_buf, v_buf);
    double *up = S.fused ? u_buf[S.cur] : (double *)F.rup, *vp = S.fused ? v_buf[S.cur] : (double *)F.rvp;
    const int extra = ctx->slab_mode ? 1 : 0;      // slab: delta from row -1
    dim3 rows((g.Nx + 255) / 256, g.Ny, g.Nz), rows_d((g.Nx + 255) / 256, g.Ny + extra, g.Nz), b256(256);
    hipLaunchKernelGGL(k_ac_direct_delta, rows_d, b256, 0, ctx->stream, g, sub->density_predictor, sub->potential_temperature, up, vp, -extra);
    if (ac_walls(ctx)) fill_walls(ctx, sub->density_predictor);      // fill_halo_regions!(delta) (acoustic_substepping.jl:1168)
    hipLaunchKernelGGL(k_ac_direct_apply, rows, b256, 0, ctx->stream, g, sub->density_predictor, sub->potential_temperature, up, vp,
                       ctx->se.damping_coefficient, S.P.wall_w, S.P.wall_s);
    BZ_LAUNCH_CHECK();
    return BZ_OK;
}

// assemble_slow_vertical_momentum_tendency! + initialize_stage_perturbations!
int bzi_acoustic_stage_begin(bz_ctx *ctx, const bz_compressible_state *s, const bz_compressible_prognostic *U0,
                             const bz_compressible_prognostic *G, const bz_acoustic_substepper *sub, double dt, double beta, bool store0)
{
    const DevGrid &g = ctx->dg;
    AcStage &S = stage_of(ctx);
    int32_t ntau = 1;
    double dtau = 0.0;
    bz_stage_substeps(ctx, dt, beta, &ntau, &dtau);
    const double om = ctx->se.forward_weight;
    AcParams &P = S.P;
    P.dtau = dtau; P.dtn = om * dtau; P.dto = (1.0 - om) * dtau;
    P.d_new = 0.0; P.d_old = 0.0;
    S.direct = ctx->se.damping_coefficient >= 0.0 && ctx->se.direct_divergence_damping != 0;
    S.damping = ctx->se.damping_coefficient >= 0.0 && !S.direct;      // the thermal form, folded into the substep kernels
    if (S.damping && ctx->se.damp_vertical) {
        const double base = ctx->se.damping_coefficient * (ctx->dz_min * ctx->dz_min);
        P.d_new = om * base;
        P.d_old = (1.0 - om) * base;
    }
    P.f_theta = ctx->se.thermodynamic_tendency_factor;
    P.f_w = ctx->se.vertical_momentum_tendency_factor;
    const double lmin = g.flat_y ? g.dx : std::fmin(g.dx, g.dy);                             // acoustic_substepping.jl:1102-1110
    const double lfix = ctx->se.damping_length_scale;                                        // ThermalDivergenceDamping(length_scale): :1085-1092
    P.kdamp = !S.damping ? 0.0 : (lfix > 0.0) ? (ctx->se.damping_coefficient * (lfix * lfix)) / dtau : ctx->se.damping_coefficient * (lmin * lmin) / dtau;
    P.inv_N = 1.0 / (double)ntau;
    P.gate = 1.0;
    P.xcd = 0;
    P.skip_avg_if_dry = nullptr;
    P.dry_q = nullptr;
    P.wall_w = ctx->ac_open[0] ? 0 : 1;
    P.wall_s = ctx->ac_open[2] ? 0 : 1;
    P.acc_mode = 0;
    P.out_of_place = 0;
    S.ntau = ntau;
    S.done = 0;
    S.fused = ctx->ac_fused;
    S.cur = S.fused ? (ntau & 1) : 0;       // index of the buffer holding the current perturbations
    AcFields F = ac_fields(ctx, s, U0, G, sub);
    double *th_buf[2], *u_buf[2], *v_buf[2];
    stage_buffers(ctx, F, th_buf, u_buf, v_buf);
    ProfileScope ps(ctx, "acoustic_stage_init");
    AcFields Fi = F;
    Fi.rthp_out = th_buf[S.cur]; Fi.rup = u_buf[S.cur]; Fi.rvp = v_buf[S.cur];
    dim3 rows((g.Nx + 255) / 256, g.Ny, g.Nz), b256(256);
    // first stage of a whole step (the caller passes store0): the state is U0 — store_initial_state! rides along
    S.fwd2 = S.fused && ac_forward2_ok(ctx);
    // stages 1 and 2 of a whole step on a single device (the caller says so through ctx->ac_skip_avg): see AcParams::skip_avg_if_dry
    if (ctx->ac_skip_avg && S.fwd2 && !ctx->slab_mode) P.skip_avg_if_dry = bzi_moisture_state(ctx);
    if (ctx->ac_whole_step && S.fwd2 && !ctx->slab_mode) P.dry_q = bzi_moisture_state(ctx);
    // the fold costs a stage four words per cell (R G_ru, G_rv; W Gp_ru, Gp_rv) and saves every substep one (p^L): stages of >= 5 substeps
    // (the 512 x 512 x 256 benchmark: 6, 9, 18; the supercell shape of configs[4]: 2, 3, 5 — its first two stages keep p^L in the substep)
    S.pfold = S.fwd2 && ctx->d_Gp_ru && (ntau >= 5 || ctx->tune.ac_pfold > 1);      // (y-slabs: the kernel folds the row above the slab too)
    // the stage's first sweeps (k_ac_forward2, k_ac_column_backward) form its initial perturbations themselves
    S.init_mode = (S.fwd2 && ctx->tune.ac_init_fold) ? (store0 ? 2 : 1) : 0;      // (y-slabs too: U0 and U carry exchanged halo rows)
    // buffer rotation (compressible_step_body): the caller passed the state arrays themselves as U0 — nothing to copy; the perturbations
    // U0 - U are (+0) by subtraction where a kernel forms them, and known zeros to the folded first sweeps
    const bool copy0 = store0 && !ctx->ac_rotate;
    if (S.pfold && ctx->slab_mode) rows.y = g.Ny + 1;
    ac_storage(ctx, [&](auto st) {
        using ST = typename decltype(st)::type;
        const AcFieldsT<ST> Fc = ac_cast<ST>(Fi);
        // ZERO: without the fused substep only; STORE0, PF, NOPERT: with it only — 9 of the 16 variants exist
        if (!S.fused) hipLaunchKernelGGL((k_ac_stage_init<true, false, false, false, ST>), rows, b256, 0, ctx->stream, g, Fc);
        else bz_bools([&](auto store, auto pf, auto nopert) {
            hipLaunchKernelGGL((k_ac_stage_init<false, store(), pf(), nopert(), ST>), rows, b256, 0, ctx->stream, g, Fc);
        }, copy0, S.pfold, S.init_mode != 0);
    });
    BZ_LAUNCH_CHECK();
    return BZ_OK;
}

// the forward sweep of a fused substep through k_ac_forward2: first substep of the stage (init: it forms the stage's initial perturbations
// itself, S.init_mode) / damping of the previous substep / folded p^L gradient
static void launch_forward2(bz_ctx *ctx, const AcFields &Fs, const AcParams &P, dim3 cols, dim3 bcol, bool first, bool damp, bool pfold, int init)
{
    const DevGrid &g = ctx->dg;
    ac_storage(ctx, [&](auto st) {
        using ST = typename decltype(st)::type;
        const AcFieldsT<ST> F = ac_cast<ST>(Fs);
        bz_bools([&](auto pf) {
            constexpr bool PF = pf();
            if (first && init == 2) hipLaunchKernelGGL((k_ac_forward2<true, false, PF, ST, 2>), cols, bcol, 0, ctx->stream, g, F, P);
            else if (first && init) hipLaunchKernelGGL((k_ac_forward2<true, false, PF, ST, 1>), cols, bcol, 0, ctx->stream, g, F, P);
            else if (first) hipLaunchKernelGGL((k_ac_forward2<true, false, PF, ST>), cols, bcol, 0, ctx->stream, g, F, P);
            else if (damp) hipLaunchKernelGGL((k_ac_forward2<false, true, PF, ST>), cols, bcol, 0, ctx->stream, g, F, P);
            else hipLaunchKernelGGL((k_ac_forward2<false, false, PF, ST>), cols, bcol, 0, ctx->stream, g, F, P);
        }, pfold);
    });
}

// substep `sstep` (1-based) of the stage opened by bzi_acoustic_stage_begin
int bzi_acoustic_substep(bz_ctx *ctx, const bz_compressible_state *s, const bz_compressible_prognostic *U0,
                         const bz_compressible_prognostic *G, const bz_acoustic_substepper *sub, int sstep)
{
    const DevGrid &g = ctx->dg;
    AcStage &S = stage_of(ctx);
    if (sstep != S.done + 1 || sstep > S.ntau) {
        ctx->last_error = "bz_acoustic_substep: substeps must be issued in order 1..N_tau after bz_acoustic_stage_begin";
        return BZ_ERR_INVALID;
    }
    AcParams P = S.P;
    const int ntau = S.ntau;
    const bool gate = ctx->se.apply_first_substep_pressure_gradient || (sstep != 1) || (ntau == 1);
    P.gate = gate ? 1.0 : 0.0;
    const bool damp = S.damping && sstep > 1;
    AcFields F = ac_fields(ctx, s, U0, G, sub);
    dim3 rows((g.Nx + 255) / 256, g.Ny, g.Nz), b256(256);
    dim3 cols((g.Nx + ACX - 1) / ACX, (g.Ny + ACY - 1) / ACY), bcol(ACX, ACY);
    P.xcd = (ctx->tune.ac_xcd && cols.y % 8 == 0) ? 1 : 0;
    dim3 colsb((g.Nx + ABX - 1) / ABX, (g.Ny + ABY - 1) / ABY), bcolb(ABX, ABY);
    const bool walls = ac_walls(ctx);
    ac_storage(ctx, [&](auto st) {      // every kernel of the substep in the storage type of the working fields
        using ST = typename decltype(st)::type;
        if (S.fused) {
            double *th_buf[2], *u_buf[2], *v_buf[2];
            stage_buffers(ctx, F, th_buf, u_buf, v_buf);
            const int cur = S.cur;
            // Bounded x / y: fill_halo_regions! of the current (rho theta)' (acoustic_substepping.jl:798,1538); the previous one, read by the
            // damping, is the buffer that was current — and filled — one substep ago
            if (walls) fill_walls_st(ctx, th_buf[cur]);
            AcFields Fs = F;
            Fs.rthp = th_buf[cur]; Fs.rth_old = th_buf[cur ^ 1]; Fs.rthp_out = th_buf[cur ^ 1];
            Fs.rup_in = u_buf[cur]; Fs.rup = u_buf[cur ^ 1];
            Fs.rvp_in = v_buf[cur]; Fs.rvp = v_buf[cur ^ 1];
            {
                ProfileScope ps(ctx, "acoustic_horizontal+column_forward");
                if (S.fwd2) {
                    const int bx = ctx->tune.ac_bx;      // 512 threads as fx columns of fy rows
                    const int fx = (bx == 128 || bx == 256 || bx == 512) ? bx : 64, fy = 512 / fx;
                    dim3 cols2((g.Nx + fx - 1) / fx, (g.Ny + fy - 1) / fy), bcol2(fx, fy);
                    P.xcd = (ctx->tune.ac_xcd && cols2.y % 8 == 0) ? 1 : 0;
                    // <u>, <v> in pairs counted from the stage's last substep (AcParams::acc_mode): substep 1 starts the accumulators, an odd
                    // substep out (substep 2) is added alone
                    if (ctx->tune.ac_pair_avg && !S.direct && !ctx->substep_f32 && sstep >= 2)      // (y-slabs too: a row accumulates its own faces)
                        P.acc_mode = ((ntau - sstep) & 1) ? 1 : (sstep >= 3 ? 2 : 0);
                    launch_forward2(ctx, Fs, P, cols2, bcol2, sstep == 1, damp, S.pfold, S.init_mode);
                }
                else if (sstep == 1)
                    hipLaunchKernelGGL((k_ac_column_forward<true, true, false, ST>), cols, bcol, 0, ctx->stream, g, ac_cast<ST>(Fs), P);
                else if (damp)
                    hipLaunchKernelGGL((k_ac_column_forward<false, true, true, ST>), cols, bcol, 0, ctx->stream, g, ac_cast<ST>(Fs), P);
                else
                    hipLaunchKernelGGL((k_ac_column_forward<false, true, false, ST>), cols, bcol, 0, ctx->stream, g, ac_cast<ST>(Fs), P);
            }
            {
                ProfileScope ps(ctx, "acoustic_column_backward");
                if (sstep == 1 && S.init_mode == 2) hipLaunchKernelGGL((k_ac_column_backward<true, ST, 2>), colsb, bcolb, 0, ctx->stream, g, ac_cast<ST>(Fs), P);
                else if (sstep == 1 && S.init_mode) hipLaunchKernelGGL((k_ac_column_backward<true, ST, 1>), colsb, bcolb, 0, ctx->stream, g, ac_cast<ST>(Fs), P);
                else if (sstep == 1) hipLaunchKernelGGL((k_ac_column_backward<true, ST>), colsb, bcolb, 0, ctx->stream, g, ac_cast<ST>(Fs), P);
                else hipLaunchKernelGGL((k_ac_column_backward<false, ST>), colsb, bcolb, 0, ctx->stream, g, ac_cast<ST>(Fs), P);
            }
            if (walls) relax_open_boundaries(ctx, F, th_buf[cur ^ 1]);
            S.cur ^= 1;
        } else {
            if (walls) { fill_walls_st(ctx, (double *)F.rthp); fill_walls_st(ctx, (double *)F.rth_old); }
            {
                ProfileScope ps(ctx, "acoustic_horizontal");
                if (damp)
                    hipLaunchKernelGGL((k_ac_horizontal<true, true, ST>), rows, b256, 0, ctx->stream, g, ac_cast<ST>(F), P);
                else
                    hipLaunchKernelGGL((k_ac_horizontal<false, true, ST>), rows, b256, 0, ctx->stream, g, ac_cast<ST>(F), P);
            }
            {
                ProfileScope ps(ctx, "acoustic_column_forward");
                if (sstep == 1)
                    hipLaunchKernelGGL((k_ac_column_forward<true, false, false, ST>), cols, bcol, 0, ctx->stream, g, ac_cast<ST>(F), P);
                else
                    hipLaunchKernelGGL((k_ac_column_forward<false, false, false, ST>), cols, bcol, 0, ctx->stream, g, ac_cast<ST>(F), P);
            }
            {
                ProfileScope ps(ctx, "acoustic_column_backward");
                hipLaunchKernelGGL((k_ac_column_backward<false, ST>), colsb, bcolb, 0, ctx->stream, g, ac_cast<ST>(F), P);
            }
            if (walls) relax_open_boundaries(ctx, F, (double *)F.rthp);
        }
    });
    S.done = sstep;
    // DirectDivergenceDamping closes every substep (also the last one) on the current perturbation buffers; on a y-slab the driver
    // exchanges (rho u)', (rho v)' first and then calls bz_acoustic_direct_damping
    if (S.direct && !ctx->slab_mode) return direct_damping(ctx, F, sub);
    BZ_LAUNCH_CHECK();
    return BZ_OK;
}

extern "C" int bz_acoustic_direct_damping(bz_ctx *ctx, const bz_compressible_state *s, const bz_compressible_prognostic *U0,
                                          const bz_compressible_prognostic *G, const bz_acoustic_substepper *sub)
{
    BZ_REQUIRE_COMPRESSIBLE();
    if (!valid_state(s) || !valid_prog(U0) || !valid_prog(G) || !valid_sub(sub)) return BZ_ERR_INVALID;
    AcStage &S = stage_of(ctx);
    if (!S.direct || !ctx->slab_mode) return BZ_OK;      // single-GPU contexts damp inside bz_acoustic_substep
    if (S.done < 1) { ctx->last_error = "bz_acoustic_direct_damping: no substep has run in this stage"; return BZ_ERR_INVALID; }
    AcFields F = ac_fields(ctx, s, U0, G, sub);
    return direct_damping(ctx, F, sub);
}

// last substep's damping + time-averaged velocities + recovery of the full state [+ WS-RK3 moisture update]
// [+ the halo fills / compute_velocities! that close the reference's loop]
int bzi_acoustic_stage_end(bz_ctx *ctx, const bz_compressible_state *s, const bz_compressible_prognostic *U0,
                           const bz_compressible_prognostic *G, const bz_acoustic_substepper *sub, double dt, double beta, bool moist,
                           bool velocities)
{
    const DevGrid &g = ctx->dg;
    AcStage &S = stage_of(ctx);
    if (S.done != S.ntau) {
        ctx->last_error = "bz_acoustic_stage_end: the stage still has substeps to run";
        return BZ_ERR_INVALID;
    }
    AcFields F = ac_fields(ctx, s, U0, G, sub);
    dim3 rows((g.Nx + 255) / 256, g.Ny, g.Nz), b256(256);
    if (ac_walls(ctx)) { fill_walls_st(ctx, (double *)F.rthp); if (!S.fused) fill_walls_st(ctx, (double *)F.rth_old); }
    ac_storage(ctx, [&](auto st) {
        using ST = typename decltype(st)::type;
        const AcFieldsT<ST> Fc = ac_cast<ST>(F);
        {
            ProfileScope ps(ctx, "acoustic_finalize");
            bz_bools([&](auto da) { hipLaunchKernelGGL((k_ac_finalize<da(), ST>), rows, b256, 0, ctx->stream, g, Fc, S.P); }, S.damping);
        }
        {
            ProfileScope ps(ctx, "acoustic_recover");
            const long long per_level = (long long)g.Ny * g.Sx;
            dim3 grid((unsigned)((per_level + 255) / 256), g.Nz);
            // MOIST 0: no moisture update; 1: rho q^v; 2: + the Kessler species
            bz_static_int<3>(!moist ? 0 : g.microphysics == 2 ? 2 : 1, [&](auto mo) {
                hipLaunchKernelGGL((k_ac_recover<mo(), ST>), grid, b256, 0, ctx->stream, g, Fc, beta * dt);
            });
        }
    });
    S.ntau = 0;
    if (velocities) return bzi_compressible_velocities(ctx, s, sub);
    BZ_LAUNCH_CHECK();
    return BZ_OK;
}

// The stage epilogue of the whole-step seam as k_ac_stage_end + k_ac_recover_density: finalize + recover (with the WS-RK3 moisture
// update) + update_state! [+ the next stage's linearisation].  Single-device contexts, thermal or no divergence damping.
bool bzi_acoustic_stage_end_fusable(const bz_ctx *ctx)
{
    return !ctx->slab_mode && !ac_walls(ctx) && !ctx->tune.no_ac_end_fuse && !(ctx->se.damping_coefficient >= 0.0 && ctx->se.direct_divergence_damping != 0);
}
int bzi_acoustic_stage_end_fused(bz_ctx *ctx, const bz_compressible_state *s, const bz_compressible_prognostic *U0,
                                 const bz_compressible_prognostic *G, const bz_acoustic_substepper *sub, double dt, double beta,
                                 bool with_linearization, const bz_compressible_state *s_out)
{
    // s_out: the recovered prognostic fields go to this state's arrays instead of in place (buffer rotation of compressible_step_body)
    const bool oop = s_out && s_out->rho_d != s->rho_d;
    const DevGrid &g = ctx->dg;
    AcStage &S = stage_of(ctx);
    if (S.done != S.ntau) {
        ctx->last_error = "bz_acoustic_stage_end: the stage still has substeps to run";
        return BZ_ERR_INVALID;
    }
    AcFields F = ac_fields(ctx, s, U0, G, sub);      // F.thL: the linearisation this stage ran on
    DiagFields D = diag_fields(ctx, oop ? s_out : s, sub);
    AcParams Pe = S.P;
    Pe.out_of_place = oop ? 1 : 0;
    double *thL_out = ctx->thL_alt ? sub->potential_temperature : ctx->d_thL2;
    dim3 rows((g.Nx + 255) / 256, g.Ny, g.Nz), b256(256);
    const double na = ctx->se.newton_abstol, dts = beta * dt;
    const int nm = ctx->se.newton_maxiter;
    ac_storage(ctx, [&](auto st) {
        using ST = typename decltype(st)::type;
        {
            ProfileScope ps(ctx, with_linearization ? "acoustic_stage_end+update_state+linearization" : "acoustic_stage_end+update_state");
            bz_bools([&](auto da, auto lin) {
                constexpr bool DAMP = da(), LIN = lin();
                bz_static_int<6>(bzi_cmp_mp(ctx), [&](auto mp) {
                    hipLaunchKernelGGL((k_ac_stage_end<DAMP, LIN, mp(), ST>), rows, b256, 0, ctx->stream, g, ac_cast<ST>(F), D, Pe, dts, (ST *)thL_out, na, nm, bzi_flatau(ctx));
                });
            }, S.damping, with_linearization);
        }
        if (!oop) {      // (out of place the density went out with the other fields: nothing reads the output set)
            ProfileScope ps(ctx, "acoustic_recover_density");
            hipLaunchKernelGGL((k_ac_recover_density<ST>), rows, b256, 0, ctx->stream, g, s->rho_d, (const ST *)F.rp);
        }
    });
    if (with_linearization) ctx->thL_alt = !ctx->thL_alt;
    S.ntau = 0;
    BZ_LAUNCH_CHECK();
    return BZ_OK;
}

extern "C" int bz_acoustic_stage_begin(bz_ctx *ctx, const bz_compressible_state *s, const bz_compressible_prognostic *U0,
                                       const bz_compressible_prognostic *G, const bz_acoustic_substepper *sub, double dt,
                                       double beta, int32_t *n_substeps, int32_t *current_buffer)
{
    BZ_REQUIRE_COMPRESSIBLE();
    int rc = check_loop_args(ctx, s, U0, G, sub);
    if (rc) return rc;
    // a caller that drives the slab exchanges itself packs rows with the grid's row and plane strides (bz_pack_rows): the Float32 working
    // fields of substep_floattype = Float32 have half-width rows, which only the library-owned communicator's packer knows
    if (ctx->slab_mode && ctx->substep_f32 && !ctx->comm) {
        ctx->last_error = "bz_acoustic_stage_begin: substep_float_bytes = 4 on a y-slab needs the library-owned communicator (bz_comm_init_*): the per-substep "
                          "halo rows of the Float32 working fields are packed by it";
        return BZ_ERR_UNSUPPORTED;
    }
    rc = bzi_acoustic_stage_begin(ctx, s, U0, G, sub, dt, beta);
    if (n_substeps) *n_substeps = stage_of(ctx).ntau;
    if (current_buffer) *current_buffer = stage_of(ctx).cur;
    return rc;
}

extern "C" int bz_acoustic_substep(bz_ctx *ctx, const bz_compressible_state *s, const bz_compressible_prognostic *U0,
                                   const bz_compressible_prognostic *G, const bz_acoustic_substepper *sub, int32_t substep,
                                   int32_t *current_buffer)
{
    BZ_REQUIRE_COMPRESSIBLE();
    int rc = check_loop_args(ctx, s, U0, G, sub);
    if (rc) return rc;
    rc = bzi_acoustic_substep(ctx, s, U0, G, sub, substep);
    if (current_buffer) *current_buffer = stage_of(ctx).cur;
    return rc;
}

extern "C" int bz_acoustic_stage_end(bz_ctx *ctx, const bz_compressible_state *s, const bz_compressible_prognostic *U0,
                                     const bz_compressible_prognostic *G, const bz_acoustic_substepper *sub, double dt,
                                     double beta, int update_moisture)
{
    BZ_REQUIRE_COMPRESSIBLE();
    int rc = check_loop_args(ctx, s, U0, G, sub);
    if (rc) return rc;
    return bzi_acoustic_stage_end(ctx, s, U0, G, sub, dt, beta, update_moisture != 0, false);
}

// Which lateral sides of a Bounded x / y carry an active open boundary condition on the wall-normal momentum (is_active_open_bc,
// acoustic_substepping.jl:1318): their outermost cells of rho', (rho theta)' are relaxed every substep with factor
// open_boundary_relaxation in (0, 1] (SplitExplicitTimeDiscretization(open_boundary_relaxation = 0.5)), and their west / south wall face
// is not zeroed; every other side of a Bounded direction is an impenetrable wall (the default).
extern "C" int bz_set_acoustic_lateral_boundaries(bz_ctx *ctx, int west_open, int east_open, int south_open, int north_open,
                                                  double open_boundary_relaxation)
{
    if (ctx) ++ctx->config_epoch;
    BZ_REQUIRE_COMPRESSIBLE();
    if (!(open_boundary_relaxation > 0.0) || open_boundary_relaxation > 1.0) {
        ctx->last_error = "bz_set_acoustic_lateral_boundaries: open_boundary_relaxation must be in (0, 1]";
        return BZ_ERR_INVALID;
    }
    const DevGrid &g = ctx->dg;
    if (((west_open || east_open) && !g.bounded_x) || ((south_open || north_open) && !g.bounded_y)) {
        ctx->last_error = "bz_set_acoustic_lateral_boundaries: an open side needs a Bounded topology in its direction";
        return BZ_ERR_INVALID;
    }
    ctx->ac_open[0] = west_open != 0; ctx->ac_open[1] = east_open != 0; ctx->ac_open[2] = south_open != 0; ctx->ac_open[3] = north_open != 0;
    ctx->ac_open_relax = open_boundary_relaxation;
    return BZ_OK;
}

extern "C" int bz_set_acoustic_scratch(bz_ctx *ctx, double *momentum_u_second_buffer, double *momentum_v_second_buffer)
{
    if (ctx) ++ctx->config_epoch;      // captured steps (bz_graph.hip) belong to one configuration
    BZ_REQUIRE_COMPRESSIBLE();
    if ((momentum_u_second_buffer == nullptr) != (momentum_v_second_buffer == nullptr)) return BZ_ERR_INVALID;
    ctx->up2_user = momentum_u_second_buffer;
    ctx->vp2_user = momentum_v_second_buffer;
    return BZ_OK;
}
