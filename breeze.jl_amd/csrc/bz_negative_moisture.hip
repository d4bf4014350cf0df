// bz_negative_moisture.hip — fix_negative_moisture!(model), the head of update_state! (line references: the reference's sources)
//   src/AtmosphereModels/update_atmosphere_model_state.jl:42
//   src/AtmosphereModels/negative_moisture_correction.jl:199-221 (column kernel), :225-228,290-321 (species borrowing),
//   :328-336 (orphaned numbers), :343-347 (clamp), :242-283 (vertical borrowing)
// One kernel, a lane per column with x fastest (the launch shape of k_implicit_step, bz_diffusivity.hip): every load and store is a coalesced
// row segment.  One downward pass per column: at level k the species borrowing, the orphan zeroing and the clamp of that level (they touch
// level k only), then the deficit handed down from k + 1, then this level's deficit, carried in a register — the reference's order of
// operations per cell, each field read once and written at most once.  Levels 2 and 1 (1-based) stay in registers for the upward step at the
// bottom.  The carry is the only dependence between levels: the loads of NMC_U levels are issued before the first of them is worked on.
// Interior cells only; the halo fill (bz_update_state) or the projection + diagnosis kernel (bz_fused.hip) that follows writes the images.
#include "bz_internal.h"

// rho q +- rho * sink stays a multiply and an add (the reference does not contract), and the vertical path has a division between every
// multiply and add: the result is a pure function of IEEE +, -, *, / in the stated order, which tests/negative_moisture_reference.py restates
#pragma clang fp contract(off)

#define NMC_MAX 4      // species of the chain, (number, mass) pairs, clamped number fields
#define NMC_U 8        // levels whose loads are in flight together

struct NmcLists {
    double *mass[NMC_MAX];            // heaviest first; the last borrows from the moisture prognostic
    double *number[NMC_MAX];
    const double *pair_mass[NMC_MAX];
    int pair_idx[NMC_MAX];            // pair_mass[p] is mass[pair_idx[p]] (its value after the borrowing is in a register), -1: another array
    double *clamp[NMC_MAX];
    int n_mass, n_pairs, n_clamp;
};

// the reference's max(0, x) and min(a, b) on floats: a NaN comes back as a NaN, max(0, -0) is +0
__device__ __forceinline__ double nmc_max0(double x) { return x > 0.0 ? x : (x != x ? x : 0.0); }
__device__ __forceinline__ double nmc_min(double a, double b) { return b != b ? b : (a < b ? a : b); }
__device__ __forceinline__ bool nmc_same_bits(double a, double b) { return bz_real_bits(a) == bz_real_bits(b); }
// a cell is stored where its bits changed ("Store policy")
__device__ __forceinline__ void nmc_store(double *__restrict__ f, long long n, double v, double v_loaded)
{
    if (!nmc_same_bits(v, v_loaded)) f[n] = v;
}

// Species borrowing, orphaned numbers and the clamp of one cell; v is rho q^ve of the cell (read by the caller, stored by the caller).
__device__ __forceinline__ double nmc_species_cell(const NmcLists &L, long long n, double rho, double v)
{
    double m[NMC_MAX], m0[NMC_MAX];
#pragma unroll
    for (int c = 0; c < NMC_MAX; ++c) m0[c] = m[c] = (c < L.n_mass) ? L.mass[c][n] : 0.0;
#pragma unroll
    for (int c = 0; c < NMC_MAX; ++c) {
        if (c < L.n_mass) {
            const bool last = c == L.n_mass - 1;
            double light = v;
            if (c + 1 < NMC_MAX) light = last ? v : m[c + 1];
            const double qh = m[c] / rho, ql = light / rho;
            const double sink = qh < 0.0 ? nmc_min(-qh, nmc_max0(ql)) : 0.0;
            const double t = rho * sink;
            m[c] = m[c] + t;
            light = light - t;
            if (last) v = light;
            else if (c + 1 < NMC_MAX) m[c + 1] = light;
        }
    }
#pragma unroll
    for (int c = 0; c < NMC_MAX; ++c)
        if (c < L.n_mass) nmc_store(L.mass[c], n, m[c], m0[c]);
#pragma unroll
    for (int p = 0; p < NMC_MAX; ++p) {
        if (p < L.n_pairs) {
            const int pi = L.pair_idx[p];
            const double mv = pi == 0 ? m[0] : pi == 1 ? m[1] : pi == 2 ? m[2] : pi == 3 ? m[3] : L.pair_mass[p][n];
            const double nv = L.number[p][n];
            nmc_store(L.number[p], n, mv <= 0.0 ? 0.0 : nv, nv);
        }
    }
#pragma unroll
    for (int c = 0; c < NMC_MAX; ++c) {
        if (c < L.n_clamp) {
            const double nv = L.clamp[c][n];      // may be a number field stored just above: the same lane, the same address
            nmc_store(L.clamp[c], n, nmc_max0(nv), nv);
        }
    }
    return v;
}

// One level k >= 1 of the downward sweep on the value v of the cell: receive the carry, form and remove this level's deficit.
__device__ __forceinline__ double nmc_down(const DevGrid &g, int k, double v, double &carry)
{
    const double dz = g.dzc[k];
    v = v - carry / dz;
    const double q = v / g.rho[k];
    const double deficit = q < 0.0 ? -v * dz : 0.0;
    v = v + deficit / dz;
    carry = deficit;
    return v;
}

// grid (ceil(Nx / 64), Ny), block 64: one wave, one row, 64 columns; ragged Nx through the predicate.
// SPECIES: a non-empty chain / pair / clamp list under SpeciesBorrowing; VERT: vertical borrowing.
template <bool SPECIES, bool VERT>
__global__ __launch_bounds__(64) void k_fix_negative_moisture(DevGrid g, NmcLists L, double *__restrict__ rq)
{
    const int i = blockIdx.x * 64 + threadIdx.x, j = blockIdx.y;
    if (i >= g.Nx) return;      // a lane reads and writes its own column only
    const long long sz = g.Sxy, n0 = g.idx(i, j, 0);
    const int Nz = g.Nz;
    if (!VERT) {
        for (int k = Nz - 1; k >= 0; --k) {
            const long long n = n0 + (long long)k * sz;
            const double v0 = rq[n];
            nmc_store(rq, n, nmc_species_cell(L, n, g.rho[k], v0), v0);
        }
        return;
    }
    // the two bottom levels are read first: the upward step at the end needs both
    const double b0_in = rq[n0], b1_in = Nz >= 2 ? rq[n0 + sz] : 0.0;
    double carry = 0.0;
    int k = Nz - 1;
    for (; k - (NMC_U - 1) >= 2; k -= NMC_U) {
        double v[NMC_U], vin[NMC_U];
        bool work = SPECIES || carry != 0.0;
#pragma unroll
        for (int u = 0; u < NMC_U; ++u) {
            vin[u] = v[u] = rq[n0 + (long long)(k - u) * sz];
            // a value with a clear sign bit, or a NaN, on a positive density: no deficit, and +- 0 / dz leaves its bits alone
            work = work || (__builtin_signbit(v[u]) && v[u] == v[u]) || !(g.rho[k - u] > 0.0);
        }
        if (!__any(work)) continue;
#pragma unroll
        for (int u = 0; u < NMC_U; ++u) {
            const long long n = n0 + (long long)(k - u) * sz;
            if (SPECIES) v[u] = nmc_species_cell(L, n, g.rho[k - u], v[u]);
            v[u] = nmc_down(g, k - u, v[u], carry);
            nmc_store(rq, n, v[u], vin[u]);
        }
    }
    for (; k >= 2; --k) {
        const long long n = n0 + (long long)k * sz;
        const double vin = rq[n];
        double v = vin;
        if (SPECIES) v = nmc_species_cell(L, n, g.rho[k], v);
        v = nmc_down(g, k, v, carry);
        nmc_store(rq, n, v, vin);
    }
    double b0 = b0_in, b1 = b1_in;
    if (Nz >= 2) {
        if (SPECIES) b1 = nmc_species_cell(L, n0 + sz, g.rho[1], b1);
        b1 = nmc_down(g, 1, b1, carry);
    }
    if (SPECIES) b0 = nmc_species_cell(L, n0, g.rho[0], b0);
    const double dz0 = g.dzc[0];
    if (Nz >= 2) {
        // the bottom receives the last deficit, then borrows upward from level 2 what it lacks and level 2 has
        const double dz1 = g.dzc[1];
        b0 = b0 - carry / dz0;
        const double qb = b0 / g.rho[0], qt = b1 / g.rho[1];
        const double dq = (qb < 0.0 && qt > 0.0) ? nmc_min(-b0 * dz0, b1 * dz1) : 0.0;
        b0 = b0 + dq / dz0;
        b1 = b1 - dq / dz1;
        nmc_store(rq, n0 + sz, b1, b1_in);
    } else {
        // Nz = 1: k_top = k_bot, dq = 0 is added to and subtracted from the one cell
        b0 = b0 + 0.0 / dz0;
        b0 = b0 - 0.0 / dz0;
    }
    nmc_store(rq, n0, b0, b0_in);
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
static bool nmc_species_active(const bz_negative_moisture_correction &c)
{
    return c.species_borrowing && (c.n_mass > 0 || c.n_pairs > 0 || c.n_clamp > 0);
}

extern "C" int bz_set_negative_moisture_correction(bz_ctx *ctx, const bz_negative_moisture_correction *c)
{
    if (!ctx) return BZ_ERR_INVALID;
    ++ctx->config_epoch;      // captured steps (bz_graph.hip) belong to one configuration
    if (!c) { ctx->has_nmc = false; return BZ_OK; }
    const char *refused = ctx->compressible  ? "CompressibleDynamics contexts update the moisture inside the acoustic stage epilogue"
                      : (ctx->slab_mode || ctx->comm) ? "y-slab contexts are not built"
                      : ctx->kinematic   ? "the kinematic driver is not built"
                      : ctx->dg.microphysics != 1 ? "no SaturationAdjustment is attached (call bz_set_saturation_adjustment first)"
                                         : nullptr;
    if (refused) {
        ctx->last_error = std::string("bz_set_negative_moisture_correction: ") + refused;
        return BZ_ERR_UNSUPPORTED;
    }
    auto invalid = [&](const char *why) {
        ctx->last_error = std::string("bz_set_negative_moisture_correction: ") + why;
        return BZ_ERR_INVALID;
    };
    if (c->n_mass < 0 || c->n_mass > NMC_MAX) return invalid("n_mass is outside 0 .. 4");
    if (c->n_pairs < 0 || c->n_pairs > NMC_MAX) return invalid("n_pairs is outside 0 .. 4");
    if (c->n_clamp < 0 || c->n_clamp > NMC_MAX) return invalid("n_clamp is outside 0 .. 4");
    if (!c->species_borrowing && !c->vertical_borrowing && (c->n_mass || c->n_pairs || c->n_clamp))
        return invalid("neither species_borrowing nor vertical_borrowing is selected, with a non-empty list");
    for (int a = 0; a < c->n_mass; ++a) {
        if (!c->mass[a]) return invalid("a null array in mass");
        for (int b = 0; b < a; ++b)
            if (c->mass[a] == c->mass[b]) return invalid("an array is given twice in mass");
    }
    for (int a = 0; a < c->n_pairs; ++a) {
        if (!c->number[a] || !c->pair_mass[a]) return invalid("a null array in number / pair_mass");
        if (c->number[a] == c->pair_mass[a]) return invalid("a number field is its own mass field");
        for (int b = 0; b < a; ++b)
            if (c->number[a] == c->number[b]) return invalid("an array is given twice in number");
        for (int b = 0; b < c->n_mass; ++b)
            if (c->number[a] == c->mass[b]) return invalid("an array is given in number and in mass");
        for (int b = 0; b < c->n_pairs; ++b)
            if (c->number[a] == c->pair_mass[b]) return invalid("an array is given in number and in pair_mass");
    }
    for (int a = 0; a < c->n_clamp; ++a) {
        if (!c->clamp[a]) return invalid("a null array in clamp");
        for (int b = 0; b < a; ++b)
            if (c->clamp[a] == c->clamp[b]) return invalid("an array is given twice in clamp");
        for (int b = 0; b < c->n_mass; ++b)
            if (c->clamp[a] == c->mass[b]) return invalid("an array is given in clamp and in mass");
        for (int b = 0; b < c->n_pairs; ++b)
            if (c->clamp[a] == c->pair_mass[b]) return invalid("an array is given in clamp and in pair_mass");
    }
    ctx->nmc = *c;
    ctx->has_nmc = true;
    return BZ_OK;
}

// fix_negative_moisture!(model) on rho_q: once per update_state! of the reference (bz_update_state; step_fused_rk and step_fused before
// their projection + diagnosis).  Nothing is launched when nothing is attached or the scheme has nothing to do.
int bzi_fix_negative_moisture(bz_ctx *ctx, double *rho_q)
{
    if (!ctx->has_nmc || ctx->dg.microphysics != 1) return BZ_OK;
    const bz_negative_moisture_correction &c = ctx->nmc;
    const bool species = nmc_species_active(c), vert = c.vertical_borrowing != 0;
    if (!species && !vert) return BZ_OK;
    if (!rho_q) return BZ_ERR_INVALID;
    NmcLists L = {};
    if (species) {
        L.n_mass = c.n_mass; L.n_pairs = c.n_pairs; L.n_clamp = c.n_clamp;
        for (int a = 0; a < c.n_mass; ++a) L.mass[a] = c.mass[a];
        for (int a = 0; a < c.n_clamp; ++a) L.clamp[a] = c.clamp[a];
        for (int a = 0; a < c.n_pairs; ++a) {
            L.number[a] = c.number[a]; L.pair_mass[a] = c.pair_mass[a]; L.pair_idx[a] = -1;
            for (int b = 0; b < c.n_mass; ++b)
                if (c.pair_mass[a] == c.mass[b]) L.pair_idx[a] = b;
        }
        bool alias = false;
        for (int a = 0; a < NMC_MAX; ++a)
            alias = alias || (a < c.n_mass && c.mass[a] == rho_q) || (a < c.n_pairs && (c.number[a] == rho_q || c.pair_mass[a] == rho_q)) ||
                    (a < c.n_clamp && c.clamp[a] == rho_q);
        if (alias) {
            ctx->last_error = "bz_fix_negative_moisture: an array of the correction is the moisture prognostic rho_q";
            return BZ_ERR_INVALID;
        }
    }
    const DevGrid &g = ctx->dg;
    ProfileScope ps(ctx, "fix_negative_moisture");
    const dim3 grid((g.Nx + 63) / 64, g.Ny), block(64);
#define NMC_LAUNCH(S, V) hipLaunchKernelGGL((k_fix_negative_moisture<S, V>), grid, block, 0, ctx->stream, g, L, rho_q)
    if (species && vert) NMC_LAUNCH(true, true);
    else if (species) NMC_LAUNCH(true, false);
    else NMC_LAUNCH(false, true);
#undef NMC_LAUNCH
    BZ_LAUNCH_CHECK();
    return BZ_OK;
}

extern "C" int bz_fix_negative_moisture(bz_ctx *ctx, const bz_state *s)
{
    if (!ctx || !s) return BZ_ERR_INVALID;
    if (!ctx->has_nmc) {
        ctx->last_error = "bz_fix_negative_moisture: no negative moisture correction is attached (bz_set_negative_moisture_correction)";
        return BZ_ERR_INVALID;
    }
    return bzi_fix_negative_moisture(ctx, s->rho_q);
}
