// bz_compressible_internal.h — what more than one unit of the compressible model needs (bz_cmp_state.hip, bz_cmp_scalar.hip,
// bz_acoustic.hip with bz_acoustic_kernels.h, bz_compressible.hip): the periodic wrap indexing, the field bundles of update_state! and of
// the acoustic loop, the stage in flight, argument checks, the launch-selection helpers and the bzi_* functions that cross these units.
#pragma once
#include <string>
#include <type_traits>

#include "bz_internal.h"

struct WrapIdx {
    long long im, ip, jm, jp;    // offsets to the periodic x / y neighbours of (i, j)
    long long ox, oy;            // offsets of this cell's periodic halo images (0: none)
};
__device__ __forceinline__ WrapIdx wrap_of(const DevGrid &g, int i, int j)
{
    WrapIdx w;
    // Bounded x (lateral walls of the acoustic loop, round 6): columns -1 and Nx are halo columns — filled by k_ac_fill_walls for the
    // substepper's own fields (their default zero-gradient boundary condition), by the caller for the model's
    w.im = (i > 0 || g.bounded_x) ? -1 : g.Nx - 1;
    w.ip = (i + 1 < g.Nx || g.bounded_x) ? 1 : 1 - g.Nx;
    // y-slab mode (wrap_y == 0): rows -1 and Ny are halo rows delivered by the caller's neighbour exchange (Bounded y: as Bounded x above)
    w.jm = (j > 0 || !g.wrap_y) ? -(long long)g.Sx : (long long)g.Sx * (g.Ny - 1);
    w.jp = (j + 1 < g.Ny || !g.wrap_y) ? (long long)g.Sx : (long long)g.Sx * (1 - g.Ny);
    w.ox = g.bounded_x ? 0 : (i < g.Hx) ? g.Nx : (i >= g.Nx - g.Hx) ? -(long long)g.Nx : 0;
    w.oy = !g.wrap_y ? 0 : (j < g.Hy) ? (long long)g.Ny * g.Sx : (j >= g.Ny - g.Hy) ? -(long long)g.Ny * g.Sx : 0;
    return w;
}

// update_state!: what k_cmp_diagnose (bz_cmp_state.hip) and the tail of k_ac_stage_end (bz_acoustic_kernels.h) read and write
struct DiagFields {
    double *rho_d, *rho, *ru, *rv, *rw, *rth, *rq;
    double *u, *v, *w, *theta, *q, *T, *p;
    double *Pi, *thL, *gR, *Clin;       // LIN
    int st32;                           // LIN: the four linearisation arrays are stored as float (substep_floattype = Float32)
};
// store into a working array of the substepper in its storage type (wave-uniform branch)
__device__ __forceinline__ void st_store(double *p, long long n, double v, int st32)
{
    if (st32) ((float *)p)[n] = (float)v;
    else p[n] = v;
}

struct AcParams {
    double dtau, dtn, dto;        // substep size, omega*dtau, (1-omega)*dtau
    double d_new, d_old;          // implicit vertical damping prefactors (0 unless damp_vertical)
    double f_theta, f_w;          // thermodynamic / vertical-momentum tendency factors
    double gate;                  // 1: perturbation horizontal PGF applied this substep, 0: skipped (first small step)
    double kdamp;                 // alpha * min(dx,dy)^2 / dtau   (0: no damping)
    double inv_N;                 // 1 / N_tau
    int xcd;                      // forward sweep: 1 = every XCD owns a band of tile rows (see k_ac_column_forward), 0 = launch order
    // Round 6, dry runs inside bz_time_step_compressible: the time-averaged velocities of a stage feed one thing, the moisture (tracer)
    // tendency the NEXT stage's update uses (acoustic_runge_kutta_3.jl:189-192) — which a model whose rho q is identically zero skips
    // (bz_moisture.hip: moisture scan; exact zeros either way).  Where this points at the scan's word and the word says "identically zero,
    // verified by the scan that opened this call", the substep kernels of stages 1 and 2 neither read nor write the three accumulators
    // (6 of a substep's 32 words) and the stage epilogue does not form the averages; stage 3 accumulates as ever, so after the step the
    // substepper holds the averages the reference leaves.  nullptr: always accumulate (per-operator entry points, slabs, moist models).
    const int *skip_avg_if_dry;
    // every stage of a dry whole step (same word): rho q and q are identically zero and stay so (the skipped moisture tendency is an exact
    // zero): the stage epilogue neither reads U0_rho_q, G_rho_q nor writes rho q, q (4 of its 41 words)
    const int *dry_q;
    // Bounded lateral topology (round 6): 1 = the west / south face of (rho u)' / (rho v)' is an impenetrable wall (the model's momentum boundary
    // condition there is the default one) and is held at zero — enforce_wall_impenetrability! (acoustic_substepping.jl:1378-1395); 0 = an
    // active open boundary, whose face the substep kernels advance like any other.  The east / north wall face (index N + 1 of the
    // reference's face field) is written by no kernel of the reference's loop — all of them are launched over :xyz — and keeps the zero the
    // field was built with: here it is an exact zero in every flux that reads it, whatever the boundary condition.
    int wall_w, wall_s;
    // Round 6: <u>, <v> accumulated two substeps at a time (k_ac_forward2).  The forward sweep of substep n reads the stored (rho u)' of
    // substep n - 1 anyway (it advances it), so a pair (n - 1, n) is added in substep n as  a += (u'_{n-1} + u'_n)  and substep n - 1 neither
    // reads nor writes the accumulators: 4 of a sweep's 22 words in every other substep.  0: a += u'_n (the reference's order); 1: this substep
    // leaves the accumulators alone (the next one takes the pair); 2: this substep adds the pair.  The sum differs from the reference's
    // ((a + u'_{n-1}) + u'_n) by one rounding of a per pair.  Thermal or no damping only (the stored u'_{n-1} is then the accumulated value:
    // its damping is applied by the sweep that reads it; DirectDivergenceDamping changes the stored field after the accumulation), working
    // fields in the grid's type (a Float32-stored u' is the rounded value of what was accumulated).
    int acc_mode;
    // Round 6: the stage epilogue writes the recovered state into ANOTHER set of arrays than it reads (compressible_step_body: buffer rotation
    // — the state arrays stay intact as U0, nothing is copied into U0): rho_d goes out with the other fields (no thread reads the output set)
    // and rho q is stored also on the dry path (the output set may hold anything)
    int out_of_place;
};

// ST = substep_floattype (acoustic_substepping.jl:199-235): the storage type of the acoustic perturbation / predictor / linearisation
// working fields.  Kernels read ST, promote to the grid's real, compute there and store ST; (rho w)', the tridiagonal right-hand side and
// factors, the time-averaged velocities and every model field stay in the grid's type.  ST = float inside a Float64 model halves the
// bytes of 12 of the arrays the substep kernels stream.
template <class ST>
struct AcFieldsT {
    // model state (stage-entry U^L; untouched by the loop)
    double *rho_d, *rth, *ru, *rv, *rw, *rq;
    const double *rho, *p;
    // outer-step start and slow tendencies
    const double *U0_rho_d, *U0_rth, *U0_ru, *U0_rv, *U0_rw, *U0_rq;
    const double *G_rho_d, *G_rth, *G_ru, *G_rv, *G_rw, *G_rq;
    double *Gp_ru, *Gp_rv;        // G_ru - dx p^L, G_rv - dy p^L of the stage (k_ac_stage_init<.., PF>; read by k_ac_forward2<.., PF>)
    // substepper
    const ST *thL, *Clin;
    ST *rp, *rthp, *rup, *rvp;
    double *rwp;
    ST *rs, *rths, *rth_old;
    // fused substep (k_ac_column_forward<.., FUSED = true>): (rho u)', (rho v)' ping-pong between rup_in (read) and rup
    // (written); (rho theta)' ping-pongs between rthp (current, read) / rth_old (previous, read) and rthp_out (written
    // by the backward sweep), so no thread reads a location another thread of the same launch writes.
    const ST *rup_in, *rvp_in;
    ST *rthp_out;
    double *au, *av, *aw;
    double *rqcl, *rqr;           // Kessler species (k_ac_recover<2>)
    const double *U0_rqcl, *U0_rqr, *G_rqcl, *G_rqr;
    double *Gs, *phi;             // slow vertical momentum tendency; forward-eliminated right-hand side
    double *tfac;                 // Thomas factors t_k
    const double *sponge;         // UpperSponge: damping_rate * ramp(z_face) per face k = 0 .. Nz (all zero without a sponge)
};
typedef AcFieldsT<double> AcFields;
// the same fields with the working arrays seen as ST (the host allocated them in that type; every other member is copied)
template <class ST>
static AcFieldsT<ST> ac_cast(const AcFields &F)
{
    AcFieldsT<ST> R;
    R.rho_d = F.rho_d; R.rth = F.rth; R.ru = F.ru; R.rv = F.rv; R.rw = F.rw; R.rq = F.rq; R.rho = F.rho; R.p = F.p;
    R.U0_rho_d = F.U0_rho_d; R.U0_rth = F.U0_rth; R.U0_ru = F.U0_ru; R.U0_rv = F.U0_rv; R.U0_rw = F.U0_rw; R.U0_rq = F.U0_rq;
    R.G_rho_d = F.G_rho_d; R.G_rth = F.G_rth; R.G_ru = F.G_ru; R.G_rv = F.G_rv; R.G_rw = F.G_rw; R.G_rq = F.G_rq;
    R.Gp_ru = F.Gp_ru; R.Gp_rv = F.Gp_rv;
    R.thL = (const ST *)F.thL; R.Clin = (const ST *)F.Clin;
    R.rp = (ST *)F.rp; R.rthp = (ST *)F.rthp; R.rup = (ST *)F.rup; R.rvp = (ST *)F.rvp; R.rwp = F.rwp;
    R.rs = (ST *)F.rs; R.rths = (ST *)F.rths; R.rth_old = (ST *)F.rth_old;
    R.rup_in = (const ST *)F.rup_in; R.rvp_in = (const ST *)F.rvp_in; R.rthp_out = (ST *)F.rthp_out;
    R.au = F.au; R.av = F.av; R.aw = F.aw; R.rqcl = F.rqcl; R.rqr = F.rqr;
    R.U0_rqcl = F.U0_rqcl; R.U0_rqr = F.U0_rqr; R.G_rqcl = F.G_rqcl; R.G_rqr = F.G_rqr;
    R.Gs = F.Gs; R.phi = F.phi; R.tfac = F.tfac; R.sponge = F.sponge;
    return R;
}

// ---- launch selection: runtime switches become template arguments once, inside a generic lambda --------------------------------
// The callee receives tags (bz_tag<T>, std::bool_constant, std::integral_constant) by value and reads them as constants
// (typename decltype(st)::type, da(), mp()).  A helper walks the full product of what it is given: where only some combinations of a
// kernel's template arguments are built (k_ac_stage_init, k_ac_forward2, k_ac_column_forward), the call site names them one by one.
template <class T>
struct bz_tag { typedef T type; };
// the context's substep storage type (AcFieldsT; ac_cast<ST> gives the fields in it)
template <class Fn>
static void ac_storage(const bz_ctx *ctx, Fn &&f)
{
    if (ctx->substep_f32) f(bz_tag<float>());
    else f(bz_tag<double>());
}
// f(std::bool_constant<b>()...) for the runtime bools b...
template <class Fn>
static void bz_bools(Fn &&f) { f(); }
template <class Fn, class... Bs>
static void bz_bools(Fn &&f, bool b, Bs... rest)
{
    if (b) bz_bools([&](auto... cs) { f(std::true_type(), cs...); }, rest...);
    else bz_bools([&](auto... cs) { f(std::false_type(), cs...); }, rest...);
}
// f(std::integral_constant<int, v>()) for v = 1 .. N - 1, any other v as 0 (g.microphysics: 0 none, 1 saturation adjustment, 2 Kessler)
template <int N, class Fn>
static void bz_static_int(int v, Fn &&f)
{
    if constexpr (N > 1) {
        if (v == N - 1) f(std::integral_constant<int, N - 1>());
        else bz_static_int<N - 1>(v, f);
    } else f(std::integral_constant<int, 0>());
}

// the MP instantiation of k_cmp_diagnose and k_ac_stage_end: g.microphysics, or for a saturation adjustment 3 on FlatauPolynomial constants,
// 4 with MixedPhaseEquilibrium (bz_set_compressible_mixed_phase_equilibrium) and 5 with both
static inline int bzi_cmp_mp(const bz_ctx *ctx)
{
    if (ctx->dg.microphysics != 1) return ctx->dg.microphysics;
    return ctx->dg.sa_mixed ? (ctx->fl_on ? 5 : 4) : (ctx->fl_on ? 3 : 1);
}

// ---- one WS-RK3 stage of the acoustic loop in three pieces (the y-slab driver exchanges halos between them) ---------
struct AcStage {
    int ntau = 0, cur = 0, done = 0;
    bool damping = false, fused = true, direct = false;
    bool fwd2 = false, pfold = false;      // k_ac_forward2 runs the forward sweeps of this stage; with the p^L gradient folded into Gp_ru / Gp_rv
    int init_mode = 0;                     // 1 / 2: the first sweeps of the stage form the initial perturbations (U0 - U / zeros) instead of reading stored ones
    AcParams P;
};
static AcStage &stage_of(bz_ctx *ctx)
{
    static_assert(sizeof(AcStage) <= sizeof(ctx->ac_stage_storage), "AcStage does not fit its storage in bz_ctx");
    return *reinterpret_cast<AcStage *>(ctx->ac_stage_storage);
}

// ---------------------------------------------------------------------------------------------------------------------
// host side: argument checks
// ---------------------------------------------------------------------------------------------------------------------
static bool valid_state(const bz_compressible_state *s)
{
    return s && s->rho_d && s->rho && s->rho_u && s->rho_v && s->rho_w && s->rho_theta && s->rho_q && s->u && s->v &&
           s->w && s->theta && s->q && s->T && s->p;
}
static bool valid_prog(const bz_compressible_prognostic *P)
{
    return P && P->rho_d && P->rho_u && P->rho_v && P->rho_w && P->rho_theta && P->rho_q;
}
static bool valid_sub(const bz_acoustic_substepper *a)
{
    return a && a->exner && a->potential_temperature && a->gamma_R_mixture && a->density_perturbation &&
           a->density_potential_temperature_perturbation && a->momentum_perturbation_u && a->momentum_perturbation_v &&
           a->momentum_perturbation_w && a->density_predictor && a->density_potential_temperature_predictor &&
           a->previous_density_potential_temperature_perturbation && a->time_averaged_u && a->time_averaged_v &&
           a->time_averaged_w && a->slow_vertical_momentum_tendency && a->vertical_solver_source_term;
}
// Contexts with a Bounded x run the acoustic loop only (bz_refresh_linearization, bz_acoustic_substep_loop, bz_acoustic_stage_begin /
// _substep / _stage_end); the rest of the compressible model — wall-aware slow tendencies, update_state! with the model's boundary
// conditions — is built for walls in y alone ((Periodic, Bounded, Bounded), impenetrable sides: BZ_REJECT_Y_WALL_OPTIONS)
#define BZ_REJECT_WALLS(what)                                                                                                          \
    do {                                                                                                                               \
        if (ctx->dg.bounded_x) {                                                                                                       \
            ctx->last_error = what ": not implemented on a Bounded x or y (compressible contexts with lateral walls run the acoustic substep loop only)"; \
            return BZ_ERR_UNSUPPORTED;                                                                                                 \
        }                                                                                                                              \
    } while (0)
// what whole steps on walls in y do not carry: an active open side (the loop alone relaxes it), WENO orders 7 / 9, microphysics
#define BZ_REJECT_Y_WALL_OPTIONS(what)                                                                                                 \
    do {                                                                                                                               \
        if (ctx->dg.bounded_y) {                                                                                                       \
            const char *why_ = (ctx->ac_open[2] || ctx->ac_open[3]) ? "an active open boundary (NormalFlowBoundaryCondition on rho v)"  \
                               : ctx->weno_R != 3                    ? "WENO(order = 7 | 9)"                                              \
                               : ctx->dg.microphysics == 2           ? "DCMIP2016KesslerMicrophysics"                                     \
                               : ctx->dg.microphysics == 1           ? "SaturationAdjustment"                                             \
                                                                     : nullptr;                                                          \
            if (why_) {                                                                                                                \
                ctx->last_error = std::string(what ": not implemented on a Bounded y with ") + why_;                                   \
                return BZ_ERR_UNSUPPORTED;                                                                                             \
            }                                                                                                                          \
        }                                                                                                                              \
    } while (0)
#define BZ_REQUIRE_COMPRESSIBLE()                                                      \
    do {                                                                               \
        if (!ctx) return BZ_ERR_INVALID;                                               \
        if (!ctx->compressible) {                                                      \
            ctx->last_error = "context was not created by bz_create_compressible";    \
            return BZ_ERR_INVALID;                                                     \
        }                                                                              \
    } while (0)

static int check_loop_args(bz_ctx *ctx, const bz_compressible_state *s, const bz_compressible_prognostic *U0,
                           const bz_compressible_prognostic *G, const bz_acoustic_substepper *sub)
{
    if (!valid_state(s) || !valid_prog(U0) || !valid_prog(G) || !valid_sub(sub)) return BZ_ERR_INVALID;
    if (!ctx->fused_ok) { ctx->last_error = "compressible path needs Nx >= 2Hx and Ny >= 2Hy"; return BZ_ERR_UNSUPPORTED; }
    return BZ_OK;
}

static int require_no_slab(bz_ctx *ctx, const char *what)
{
    if (ctx->slab_mode) {
        ctx->last_error = std::string(what) + ": a y-slab context needs the distributed driver (halo exchanges between the pieces)";
        return BZ_ERR_UNSUPPORTED;
    }
    return BZ_OK;
}

static DiagFields diag_fields(bz_ctx *ctx, const bz_compressible_state *s, const bz_acoustic_substepper *sub)
{
    DiagFields F;
    F.rho_d = s->rho_d; F.rho = s->rho; F.ru = s->rho_u; F.rv = s->rho_v; F.rw = s->rho_w; F.rth = s->rho_theta; F.rq = s->rho_q;
    F.u = s->u; F.v = s->v; F.w = s->w; F.theta = s->theta; F.q = s->q; F.T = s->T; F.p = s->p;
    F.Pi = sub ? sub->exner : nullptr;
    F.thL = sub ? sub->potential_temperature : nullptr;
    F.gR = sub ? sub->gamma_R_mixture : nullptr;
    F.Clin = ctx->d_Clin;
    F.st32 = ctx->substep_f32 ? 1 : 0;
    return F;
}

static bool ac_walls(const bz_ctx *ctx) { return ctx->dg.bounded_x || ctx->dg.bounded_y; }

// Grids with Hx <= Nx < 2 Hx or Hy <= Ny < 2 Hy (the reference's 8 x 8 x 8 test grids under a halo of 5, test/instantaneous_precipitation.jl:133):
// a cell can have two periodic images in a direction and the fused image stores of the step's kernels write one, so the acoustic loop and
// whole steps stay refused there (check_loop_args).  update_state! (set!) and the once-per-step update of InstantaneousPrecipitation run on a
// single-device periodic context without microphysics species and closures: k_cmp_diagnose reaches its neighbours through wrap offsets and
// the generic halo kernels fill what it produced (bzi_compressible_update_state).
static bool small_grid(const DevGrid &g) { return g.Nx < 2 * g.Hx || g.Ny < 2 * g.Hy; }
static bool small_grid_update_ok(const bz_ctx *ctx)
{
    return small_grid(ctx->dg) && ctx->dg.microphysics == 0 && !ctx->has_closure && !ctx->has_diffusivity && !ctx->slab_mode && !ac_walls(ctx);
}

// Walls in y, a y-face field (rho v, v): the x image; the south wall face (row 0) stored as the zero it is; next to the north wall also the
// wall face j = Ny, which lives in the first upper halo row ("Walls in y")
#ifdef __HIPCC__
__device__ __forceinline__ void st_yface_w(const DevGrid &g, double *__restrict__ f, long long n, double v, long long ox, bool store, bool north)
{
    if (store) f[n] = v;
    if (ox) f[n + ox] = v;
    if (north) {
        f[n + g.Sx] = 0.0;
        if (ox) f[n + g.Sx + ox] = 0.0;
    }
}
#endif

// ---- functions that cross the units ---------------------------------------------------------------------------------
// bz_cmp_state.hip: update_state! [+ the moisture tendencies] [+ the linearisation of the next stage]; the velocities-only tail of
// acoustic_rk3_substep_loop! (halo images of the acoustic prognostics + compute_velocities!)
int bzi_compressible_update_state(bz_ctx *ctx, const bz_compressible_state *s, const bz_compressible_prognostic *G,
                                  const bz_acoustic_substepper *sub, bool compute_tendencies, bool with_linearization);
int bzi_compressible_velocities(bz_ctx *ctx, const bz_compressible_state *s, const bz_acoustic_substepper *sub);
// bz_acoustic.hip: one WS-RK3 stage of the acoustic loop in its pieces
int bzi_acoustic_stage_begin(bz_ctx *ctx, const bz_compressible_state *s, const bz_compressible_prognostic *U0,
                             const bz_compressible_prognostic *G, const bz_acoustic_substepper *sub, double dt, double beta,
                             bool store0 = false);
int bzi_acoustic_substep(bz_ctx *ctx, const bz_compressible_state *s, const bz_compressible_prognostic *U0,
                         const bz_compressible_prognostic *G, const bz_acoustic_substepper *sub, int sstep);
int bzi_acoustic_stage_end(bz_ctx *ctx, const bz_compressible_state *s, const bz_compressible_prognostic *U0,
                           const bz_compressible_prognostic *G, const bz_acoustic_substepper *sub, double dt, double beta, bool moist,
                           bool velocities);
// bz_instant_precip.hip: the once-per-step rain-out kernel of InstantaneousPrecipitation on the state's own arrays (bz_ctx::has_instant_precip);
// bz_instantaneous_precipitation_update (public) is this followed by update_state! with tendencies
int bzi_instantaneous_precipitation(bz_ctx *ctx, const bz_compressible_state *s, double dt);
// bz_compressible.hip: the whole-step body, launched (no moisture scan, no recorded graph)
int bzi_compressible_step_launched(bz_ctx *ctx, const bz_compressible_state *s, const bz_compressible_prognostic *U0,
                                   const bz_compressible_prognostic *G, const bz_acoustic_substepper *sub, double dt);
bool bzi_acoustic_stage_end_fusable(const bz_ctx *ctx);
int bzi_acoustic_stage_end_fused(bz_ctx *ctx, const bz_compressible_state *s, const bz_compressible_prognostic *U0,
                                 const bz_compressible_prognostic *G, const bz_acoustic_substepper *sub, double dt, double beta,
                                 bool with_linearization, const bz_compressible_state *s_out = nullptr);

