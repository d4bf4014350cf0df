// bz_adiabatic_balance.hip — adiabatic initialisation (FV3 na_init) of the anelastic and the compressible model:
//
//   bz_nudge_fields                           nudge_initial_fields!      src/AtmosphereModels/adiabatic_balance.jl:77-86
//   bz_balance_adiabatically_compressible     balance_adiabatically!     src/AtmosphereModels/adiabatic_balance.jl:44-66
//   bz_balance_adiabatically_anelastic        (the same function on the anelastic model)
//
// One kernel:
//   k_nudge_fields   x <- (x + w x0) / (1 + w) over whole parent arrays, one launch for every listed field (pointer table by value, the field
//                    in blockIdx.y).  Two loads and one store per element and a division: memory-bound.  Where both arrays of a field are
//                    16-byte aligned the body moves 16 bytes per lane and access (2 Float64 / 4 Float32 elements) and a scalar tail takes the
//                    rest of an odd count; an unaligned field runs scalar.  The quotient is a true division, so the result is the correctly
//                    rounded (x + w x0) / (1 + w) up to the one contraction of x + w x0 into an FMA.
// The drivers enqueue everything on the context's stream: snapshot copies, the whole-step bodies with +dt and -dt (launched; no moisture
// scan, no recorded graph), the nudge, the halo fills of the nudged fields and update_state! with tendencies.  The only host waits are
// the allocation of the snapshot block before the loop and its release after it.
// Scope: one device, (Periodic, Periodic | Flat, Bounded).  Walls, y-slabs and kinematic contexts return BZ_ERR_UNSUPPORTED.
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "bz_compressible_internal.h"

#define BZ_NUDGE_MAX_FIELDS 16
constexpr int NUDGE_LANES = 16 / (int)sizeof(double);      // elements of a 16-byte access
typedef double nudge_vec __attribute__((ext_vector_type(NUDGE_LANES)));

struct NudgeTable {
    double *x[BZ_NUDGE_MAX_FIELDS];
    const double *x0[BZ_NUDGE_MAX_FIELDS];
    long long n[BZ_NUDGE_MAX_FIELDS];       // elements of the field
    long long nv[BZ_NUDGE_MAX_FIELDS];      // 16-byte groups its vector body covers (0: unaligned, all scalar)
};

__global__ __launch_bounds__(256) void k_nudge_fields(NudgeTable T, double w, double den)
{
    const int f = blockIdx.y;
    double *__restrict__ x = T.x[f];
    const double *__restrict__ x0 = T.x0[f];
    const long long n = T.n[f], nv = T.nv[f];
    const long long t0 = (long long)blockIdx.x * 256 + threadIdx.x, stride = (long long)gridDim.x * 256;
    nudge_vec *__restrict__ xv = (nudge_vec *)x;
    const nudge_vec *__restrict__ x0v = (const nudge_vec *)x0;
    for (long long t = t0; t < nv; t += stride) {
        const nudge_vec a = xv[t], b = x0v[t];
        xv[t] = (a + w * b) / den;
    }
    for (long long t = nv * NUDGE_LANES + t0; t < n; t += stride) x[t] = (x[t] + w * x0[t]) / den;
}

static bool nudge_weight_ok(double weight) { return std::isfinite(weight) && weight > -1.0; }

// the launch of bz_nudge_fields: one table, at most BZ_NUDGE_MAX_FIELDS fields (the longest list of the drivers below: four fields and
// BZ_MAX_TRACERS tracers)
static int nudge_fields(bz_ctx *ctx, int n, double *const *fields, const double *const *snapshots, const long long *count, double weight)
{
    ProfileScope ps(ctx, "nudge_initial_fields");
    NudgeTable T;
    long long work = 0;
    for (int i = 0; i < n; ++i) {
        T.x[i] = fields[i]; T.x0[i] = snapshots[i]; T.n[i] = count[i];
        const bool aligned = (((uintptr_t)T.x[i] | (uintptr_t)T.x0[i]) & 15) == 0;
        T.nv[i] = aligned ? T.n[i] / NUDGE_LANES : 0;
        const long long items = T.nv[i] + (T.n[i] - T.nv[i] * NUDGE_LANES);
        if (items > work) work = items;
    }
    if (n == 0 || work == 0) return BZ_OK;
    const long long cap = (long long)ctx->num_cus * 16;      // grid-stride: enough blocks to fill the device, no more
    const long long blocks = (work + 255) / 256;
    hipLaunchKernelGGL(k_nudge_fields, dim3((unsigned)(blocks < cap ? blocks : cap), n), dim3(256), 0, ctx->stream, T, weight, 1.0 + weight);
    BZ_LAUNCH_CHECK();
    return BZ_OK;
}

extern "C" int bz_nudge_fields(bz_ctx *ctx, int32_t n, double *const *fields, const double *const *snapshots, const int64_t *count, double weight)
{
    if (!ctx || n < 0 || (n > 0 && (!fields || !snapshots || !count))) return BZ_ERR_INVALID;
    if (!nudge_weight_ok(weight)) { ctx->last_error = "bz_nudge_fields: weight must be finite and > -1"; return BZ_ERR_INVALID; }
    if (n > BZ_NUDGE_MAX_FIELDS) { ctx->last_error = "bz_nudge_fields: more than 16 fields"; return BZ_ERR_INVALID; }
    long long cnt[BZ_NUDGE_MAX_FIELDS];
    for (int i = 0; i < n; ++i) {
        if (!fields[i] || !snapshots[i] || count[i] < 0) return BZ_ERR_INVALID;
        cnt[i] = (long long)count[i];
    }
    return nudge_fields(ctx, n, fields, snapshots, cnt, weight);
}

// ---------------------------------------------------------------------------------------------------------------------
// the balance loop
// ---------------------------------------------------------------------------------------------------------------------
static int balance_arguments(bz_ctx *ctx, const char *what, double dt, int cycles, double weight)
{
    if (cycles < 1) { ctx->last_error = std::string(what) + ": cycles must be >= 1"; return BZ_ERR_INVALID; }
    if (!std::isfinite(dt) || dt == 0.0) { ctx->last_error = std::string(what) + ": dt must be finite and non-zero"; return BZ_ERR_INVALID; }
    if (!nudge_weight_ok(weight)) { ctx->last_error = std::string(what) + ": weight must be finite and > -1"; return BZ_ERR_INVALID; }
    return BZ_OK;
}

static int balance_scope(bz_ctx *ctx, const char *what)
{
    if (ctx->slab_mode) {
        ctx->last_error = std::string(what) + ": not implemented on a y-slab context (the nudge and its update_state! would need the neighbour exchanges)";
        return BZ_ERR_UNSUPPORTED;
    }
    if (ctx->kinematic) {
        ctx->last_error = std::string(what) + ": the context has PrescribedDynamics (no vertical momentum to spin up)";
        return BZ_ERR_UNSUPPORTED;
    }
    if (ctx->dg.bounded_x || ctx->dg.bounded_y) {
        ctx->last_error = std::string(what) + ": not implemented between walls (Bounded x / Bounded y)";
        return BZ_ERR_UNSUPPORTED;
    }
    return BZ_OK;
}

// the initial fields of a model: centre-shaped parents all (rho_w is not among them)
struct InitialFields {
    double *f[BZ_NUDGE_MAX_FIELDS];
    int n = 0;
};
static_assert(4 + BZ_MAX_TRACERS <= 12 && 12 <= BZ_NUDGE_MAX_FIELDS, "the initial fields fit one nudge table and one halo-fill list (bz_halo.hip)");

// snapshot_initial_fields: one block for all copies (whole parent arrays, halos included), on the context's stream
static int snapshot_fields(bz_ctx *ctx, const InitialFields &I, size_t ncell, double **block, const double **snap)
{
    *block = nullptr;
    if (hipMalloc(block, (size_t)I.n * ncell * sizeof(double)) != hipSuccess || !*block) {
        (void)hipGetLastError();
        *block = nullptr;
        ctx->last_error = "balance_adiabatically: the snapshot of the initial fields could not be allocated";
        return BZ_ERR_ALLOC;
    }
    for (int i = 0; i < I.n; ++i) {
        snap[i] = *block + (size_t)i * ncell;
        BZ_HIP(hipMemcpyAsync(*block + (size_t)i * ncell, I.f[i], ncell * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    }
    return BZ_OK;
}

// nudge + fill_halo_regions! of every initial field (adiabatic_balance.jl:78-86)
static int nudge_and_fill(bz_ctx *ctx, const InitialFields &I, const double *const *snap, size_t ncell, double weight)
{
    long long count[BZ_NUDGE_MAX_FIELDS];
    int kinds[BZ_NUDGE_MAX_FIELDS];
    for (int i = 0; i < I.n; ++i) { count[i] = (long long)ncell; kinds[i] = 0; }
    const int rc = nudge_fields(ctx, I.n, I.f, snap, count, weight);
    return rc ? rc : bzi_fill_halos_multi(ctx, I.f, kinds, I.n);
}

// the snapshot block is released when the stream has run everything that reads it
static int release_snapshot(bz_ctx *ctx, double *block, int rc)
{
    if (!block) return rc;
    const hipError_t e = hipStreamSynchronize(ctx->stream);
    (void)hipFree(block);
    if (!rc && e != hipSuccess) { ctx->last_error = std::string("balance_adiabatically: ") + hipGetErrorString(e); return -(int)e; }
    return rc;
}

static int balance_compressible(bz_ctx *ctx, const bz_compressible_state *s, const bz_compressible_prognostic *U0,
                                const bz_compressible_prognostic *G, const bz_acoustic_substepper *sub, double dt, int cycles, double weight,
                                const InitialFields &I, const double *const *snap, size_t ncell)
{
    int rc;
    // the moisture scan's word: unknown, so that no stage skips the moisture on the word of an earlier call's scan
    if (ctx->d_qstate) BZ_HIP(hipMemsetAsync(ctx->d_qstate, 0, sizeof(int), ctx->stream));
    bzi_moisture_unknown(ctx);
    for (int c = 0; c < cycles; ++c)
        for (const double sdt : {dt, -dt}) {      // 0 -> +dt -> 0, nudge; 0 -> -dt -> 0, nudge
            if ((rc = bzi_compressible_step_launched(ctx, s, U0, G, sub, sdt))) return rc;
            if ((rc = bzi_compressible_step_launched(ctx, s, U0, G, sub, -sdt))) return rc;
            if ((rc = nudge_and_fill(ctx, I, snap, ncell, weight))) return rc;
            if ((rc = bz_compressible_update_state(ctx, s, G, sub, 1))) return rc;
        }
    return BZ_OK;
}

extern "C" int bz_balance_adiabatically_compressible(bz_ctx *ctx, const bz_compressible_state *s, const bz_compressible_prognostic *U0,
                                                     const bz_compressible_prognostic *G, const bz_acoustic_substepper *sub, double dt,
                                                     int32_t cycles, double weight, int32_t nudge_moisture)
{
    const char *what = "bz_balance_adiabatically_compressible";
    BZ_REQUIRE_COMPRESSIBLE();
    int rc = balance_scope(ctx, what);
    if (rc) return rc;
    if ((rc = check_loop_args(ctx, s, U0, G, sub))) return rc;
    if ((rc = balance_arguments(ctx, what, dt, cycles, weight))) return rc;
    const DevGrid &g = ctx->dg;
    const size_t ncell = (size_t)g.Sxy * (size_t)(g.Nz + 2 * g.Hz);
    InitialFields I;
    I.f[I.n++] = s->rho_d; I.f[I.n++] = s->rho_u; I.f[I.n++] = s->rho_v; I.f[I.n++] = s->rho_theta;
    if (nudge_moisture) I.f[I.n++] = s->rho_q;
    double *block;
    const double *snap[BZ_NUDGE_MAX_FIELDS];
    rc = snapshot_fields(ctx, I, ncell, &block, snap);
    if (!rc) rc = balance_compressible(ctx, s, U0, G, sub, dt, cycles, weight, I, snap, ncell);
    return release_snapshot(ctx, block, rc);
}

static int balance_anelastic(bz_ctx *ctx, const bz_state *s, const bz_prognostic *U0, const bz_prognostic *G, double dt, int cycles, double weight,
                             const InitialFields &I, const double *const *snap, size_t ncell)
{
    int rc = bzi_anelastic_steps_open(ctx, s);
    if (rc) return rc;
    for (int c = 0; c < cycles; ++c)
        for (const double sdt : {dt, -dt}) {
            if ((rc = bzi_anelastic_step_launched(ctx, s, U0, G, sdt))) return rc;
            if ((rc = bzi_anelastic_step_launched(ctx, s, U0, G, -sdt))) return rc;
            if ((rc = nudge_and_fill(ctx, I, snap, ncell, weight))) return rc;
            if ((rc = bz_update_state(ctx, s, G, 1))) return rc;
        }
    return BZ_OK;
}

extern "C" int bz_balance_adiabatically_anelastic(bz_ctx *ctx, const bz_state *s, const bz_prognostic *U0, const bz_prognostic *G, double dt,
                                                  int32_t cycles, double weight, int32_t nudge_moisture)
{
    const char *what = "bz_balance_adiabatically_anelastic";
    if (!ctx) return BZ_ERR_INVALID;
    if (ctx->compressible) { ctx->last_error = std::string(what) + ": the context was created by bz_create_compressible"; return BZ_ERR_INVALID; }
    int rc = balance_scope(ctx, what);
    if (rc) return rc;
    if (!s || !U0 || !G || !s->rho_u || !s->rho_v || !s->rho_w || !s->rho_theta || !s->rho_q) return BZ_ERR_INVALID;
    if ((rc = balance_arguments(ctx, what, dt, cycles, weight))) return rc;
    const DevGrid &g = ctx->dg;
    const size_t ncell = (size_t)g.Sxy * (size_t)(g.Nz + 2 * g.Hz);
    InitialFields I;
    I.f[I.n++] = s->rho_u; I.f[I.n++] = s->rho_v; I.f[I.n++] = s->rho_theta;
    if (nudge_moisture) I.f[I.n++] = s->rho_q;
    for (int t = 0; t < ctx->n_tracers; ++t) I.f[I.n++] = (double *)ctx->tracers[t].density;
    double *block;
    const double *snap[BZ_NUDGE_MAX_FIELDS];
    rc = snapshot_fields(ctx, I, ncell, &block, snap);
    if (!rc) rc = balance_anelastic(ctx, s, U0, G, dt, cycles, weight, I, snap, ncell);
    return release_snapshot(ctx, block, rc);
}
