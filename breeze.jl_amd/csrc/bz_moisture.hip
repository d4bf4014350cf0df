// bz_moisture.hip — the moisture scan that opens every anelastic step call: is rho q identically zero?
#include "bz_internal.h"

// The reference advects rho q^v in every model, dry ones included (update_atmosphere_model_state.jl:333-343).  In a dry run the field
// is identically zero and stays so: every flux of it is an exact zero, its update is 0 -> 0.  Every step call opens with one pass over
// rho q (1 word per cell, once per CALL — bz_time_steps_anelastic amortises it over its n steps) that leaves *d_qstate = 1 if every
// element is zero (2 otherwise); the lean scalar-pair and z-momentum kernels read that word and, where it is 1, skip every load, store and
// flux of rho q (4.6 of the scalar kernel's 13 words per cell, a fifth of its instructions).  The result carries the same bits either
// way.  2 is sticky (a moist model is scanned once, later calls return at once) until bz_update_state — what set! ends with — resets it;
// a dry model is scanned at every call, so a moisture field written behind the library's back is seen.  Contexts with a moisture
// source (bottom moisture flux, moisture forcing, subsidence of q) or with microphysics never take the shortcut.
// state[0]: 0 unknown (treated as moist: nothing is skipped), 1 identically zero (verified by the scan that opened this call),
//           2 moist (sticky until bz_update_state puts 0 back);  state[1]: "some block found a non-zero element" of the scan in flight
__global__ __launch_bounds__(256) void k_scan_moisture(const double *__restrict__ rq, long long n, int *__restrict__ state)
{
    if (state[0] == 2) return;
    bool found = false;
    for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < n; t += (long long)gridDim.x * 256) found = found || (rq[t] != 0.0);
    if (__any(found) && (threadIdx.x & 63) == 0) state[1] = 1;
}
__global__ void k_scan_moisture_close(int *__restrict__ state)
{
    if (state[0] != 2) state[0] = state[1] ? 2 : 1;
    state[1] = 0;
}
// y-slab contexts: the verdict must be the DOMAIN's, not the slab's (a rank whose slab is dry while its neighbour's is not would drop
// the moisture that arrives through its halo rows for the rest of the call): every rank contributes "found" (0 / 1, also a
// rank that already knows it is moist) to a sum over the communicator and closes the scan on the sum
__global__ void k_scan_moisture_flag(const int *__restrict__ state, double *__restrict__ flag) { flag[0] = (state[0] == 2 || state[1]) ? 1.0 : 0.0; }
__global__ void k_scan_moisture_close_global(int *__restrict__ state, const double *__restrict__ flag)
{
    state[0] = flag[0] != 0.0 ? 2 : 1;
    state[1] = 0;
}

static bool moisture_sources(const bz_ctx *ctx)
{
    return ctx->tune.no_dry_shortcut || ctx->dg.microphysics != 0 || ctx->has_bulk || ctx->has_relaxation || ctx->field_forcing != nullptr ||
           (ctx->has_forcings && (ctx->forcing_flux_q != 0.0 || (ctx->forcing_static_mask & 8) || (ctx->forcing_subsidence_mask & 8))) ||
           (ctx->cmp_sf_on && ctx->cmp_sf.vapor.enabled) ||      // BulkVaporFlux on a compressible context: evaporation into a dry model
           (ctx->slab_mode && !ctx->comm);      // slabs driven from the host: the library cannot ask the other ranks, so nothing is skipped
}

// the word the lean kernels read (nullptr: no shortcut on this context)
const int *bzi_moisture_state(const bz_ctx *ctx) { return (ctx->d_qstate && !moisture_sources(ctx)) ? ctx->d_qstate : nullptr; }

int bzi_scan_moisture(bz_ctx *ctx, const bz_state *s) { return ctx->compressible ? BZ_OK : bzi_scan_moisture_field(ctx, s->rho_q); }

void bzi_moisture_unknown(bz_ctx *ctx) { ctx->q_host = 0; ctx->q_pending = false; }

int bzi_scan_moisture_field(bz_ctx *ctx, const double *rho_q)
{
    if (moisture_sources(ctx)) return BZ_OK;
    const DevGrid &g = ctx->dg;
    int rc;
    if (!ctx->d_qstate) {
        BZ_HIP(hipMalloc(&ctx->d_qstate, 2 * sizeof(int) + 2 * sizeof(double)));      // [state, found] + the flag of the slab all-reduce
        BZ_HIP(hipMemsetAsync(ctx->d_qstate, 0, 2 * sizeof(int) + 2 * sizeof(double), ctx->stream));
        BZ_HIP(hipHostMalloc(&ctx->h_qstate, sizeof(int)));
        BZ_HIP(hipEventCreateWithFlags(&ctx->ev_q, hipEventDisableTiming));
        ctx->q_host = 0;
    }
    // the verdict of the previous call's scan, if it has landed (asynchronous copy, never waited for)
    if (ctx->q_pending && !ctx->comm && hipEventQuery(ctx->ev_q) == hipSuccess) { ctx->q_host = *ctx->h_qstate; ctx->q_pending = false; }
    if (ctx->q_host == 2) return BZ_OK;      // moist is sticky on the device (until bz_update_state) and on every rank of a slab communicator alike: nothing to scan
    // an undiagnosed last stage leaves the halo exchange of rho q on the side stream: the scan reads those rows
    if (ctx->comm && (rc = bzi_comm_join_pending(ctx))) return rc;
    const long long n = (long long)g.Sxy * (g.Nz + 2 * g.Hz);
    {
    ProfileScope ps(ctx, "moisture_scan");
    hipLaunchKernelGGL(k_scan_moisture, dim3(ctx->num_cus * 8), dim3(256), 0, ctx->stream, rho_q, n, ctx->d_qstate);
    if (ctx->comm) {
        double *flag = (double *)(ctx->d_qstate + 2);
        hipLaunchKernelGGL(k_scan_moisture_flag, dim3(1), dim3(1), 0, ctx->stream, ctx->d_qstate, flag);
        BZ_LAUNCH_CHECK();
        if ((rc = bzi_comm_allreduce_sum(ctx, flag, 1))) return rc;      // a collective: every rank of the communicator scans at every call
        hipLaunchKernelGGL(k_scan_moisture_close_global, dim3(1), dim3(1), 0, ctx->stream, ctx->d_qstate, flag);
    } else
        hipLaunchKernelGGL(k_scan_moisture_close, dim3(1), dim3(1), 0, ctx->stream, ctx->d_qstate);
    BZ_LAUNCH_CHECK();
    }
    if (ctx->graph_capturing) return BZ_OK;      // (never: the scan precedes the recorded region)
    BZ_HIP(hipMemcpyAsync(ctx->h_qstate, ctx->d_qstate, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    if (ctx->q_host == 0 || ctx->comm) {
        // first scan since update_state!: read the verdict back before the first tendency launch — one host wait per set! / first step —
        // so that from here on the host launches the body that applies (separate kernels, separate rocprofv3 rows).
        // Slab communicators read it back at EVERY call: the asynchronous path below lands at a rank-dependent time, and a rank that has
        // learnt "moist" stops scanning — its peers would wait for it in the scan's all-reduce.  Read synchronously, the (all-reduced)
        // verdict is the same on every rank at the same call
        BZ_HIP(hipStreamSynchronize(ctx->stream));
        ctx->q_host = *ctx->h_qstate;
        ctx->q_pending = false;
    } else {
        BZ_HIP(hipEventRecord(ctx->ev_q, ctx->stream));
        ctx->q_pending = true;
    }
    return BZ_OK;
}
