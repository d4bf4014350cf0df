// bz_tendency4.hip — launcher of the fourth-generation (LDS-tiled) tendency kernels of bz_tendency4_kernels.h: k_{u,v,w}_tend_lds and
// k_scalar_pair_lds.  The momentum launchers forward to the stored-velocity kernels of the fifth generation where those apply
// (bzi_k6_stored_ok, bz_tendency5.hip); the tiles are what runs between x walls, under BZ_NO_K6_STORED and in the compressible model.
#include <cstdlib>

#include "bz_tendency4_kernels.h"

// LDS-tiled kernels amortise a per-block prologue (tile + ring fill): prefer chunks of >= 128 levels while keeping
// >= 2 blocks per CU in flight
static int pick_chunk_lds(const DevGrid &g, int nlev, int rows_per_block)
{
    long long tiles = (long long)((g.Nx + 63) / 64) * ((g.Ny + rows_per_block - 1) / rows_per_block);
    long long want = (1024 + tiles - 1) / tiles;
    long long maxchunks = nlev / 128 > 0 ? nlev / 128 : 1;
    if (want > maxchunks) want = maxchunks;
    if (want < 1) want = 1;
    // small grids (BOMEX 256 x 256 x 128: 128 tiles; the 168 x 168 x 40 supercell box: 63): filling the 256 CUs matters more
    // than the prologue, go down to 8-level chunks until there are two blocks per CU (measured: supercell box 3.3 -> 2.5 ms/step,
    // BOMEX 128 x 128 x 96 2.6 -> 1.7 ms/step against a 32-level floor; 512^3 is not affected)
    if (tiles * want < 512) {
        long long fill = (512 + tiles - 1) / tiles;
        const int minlev = 8;
        long long cap = nlev / minlev > 0 ? nlev / minlev : 1;
        if (fill > cap) fill = cap;
        if (fill > want) want = fill;
    }
    return (int)((nlev + want - 1) / want);
}

// launch shape of every kernel here: 64 x 8 tiles, nlev levels in chunks of pick_chunk_lds
struct TileLaunch {
    int kc;
    dim3 block, grid;
    TileLaunch(const DevGrid &g, int nlev) : kc(pick_chunk_lds(g, nlev, 8)), block(64, 8), grid((g.Nx + 63) / 64, (g.Ny + 7) / 8, (nlev + kc - 1) / kc) {}
};

// inputs of a momentum tile kernel: advected velocity c, tendency (or, with an RK epilogue, predictor) array G
static Tend3Fields momentum_fields(const bz_state *s, const double *c, double *G)
{
    Tend3Fields F;
    F.ru = s->rho_u; F.rv = s->rho_v; F.rw = s->rho_w;
    F.u = s->u; F.v = s->v; F.w = s->w; F.T = s->T; F.q = s->q;
    F.c = c; F.G = G;
    return F;
}

// the caller's RK epilogue with the step-start array of this component (in the first stage the kernel fills it)
static RKEpilogue momentum_epilogue(const RKEpilogue *Ein, double *u0)
{
    RKEpilogue E;
    if (Ein) { E = *Ein; E.u0 = u0; E.u0_out = u0; }
    return E;
}

// potential temperature + moisture in one pass (k_scalar_pair_lds)
// With an RK epilogue (E != nullptr) rho_theta and rho_q are advanced in place and, in the first stage, U0 is filled.
int bzi_scalar_pair_tendency(bz_ctx *ctx, const bz_state *s, const bz_prognostic *G, const bz_prognostic *U0,
                             const RKEpilogue *Ein)
{
    const DevGrid &g = ctx->dg;
    ProfileScope ps(ctx, Ein ? "scalar_tendencies+rk3" : "scalar_tendencies");
    const TileLaunch L(g, g.Nz);
    RKEpilogue E;
    double *outa = G->rho_theta, *outb = G->rho_q;
    if (Ein) {
        E = *Ein;
        E.u0 = U0->rho_theta; E.u0_out = U0->rho_theta; E.u0b = U0->rho_q; E.u0b_out = U0->rho_q;
        outa = s->rho_theta; outb = s->rho_q;
    }
    hipLaunchKernelGGL((k_scalar_pair_lds<8>), L.grid, L.block, 0, ctx->stream, g, s->u, s->v, s->w, s->theta, s->q,
                       outa, outb, L.kc, E, s->rho_theta, s->rho_q);
    BZ_LAUNCH_CHECK();
    return BZ_OK;
}

// z-momentum tendency with the w y-stencil in an LDS tile (k_w_tend_lds); in situ (512^3 bubble) the tile with 8 rows took 2.9 ms
// per launch, with 4 rows 3.9 ms
int bzi_w_tendency_lds(bz_ctx *ctx, const bz_state *s, const bz_prognostic *G, const bz_prognostic *U0,
                       const RKEpilogue *Ein, int buoyancy_mode)
{
    const DevGrid &g = ctx->dg;
    const int bm = (buoyancy_mode == 0 && g.microphysics) ? (g.sa_mixed ? 5 : 3) : buoyancy_mode;      // 5: the mixed-phase instantiation of 3
    if (bzi_k6_stored_ok(ctx)) return bzi_k6_stored(ctx, 2, s, G, U0, Ein, bm);
    ProfileScope ps(ctx, Ein ? "z_momentum_tendency+rk3" : "z_momentum_tendency");
    const RKEpilogue E = momentum_epilogue(Ein, U0 ? U0->rho_w : nullptr);
    const Tend3Fields F = momentum_fields(s, s->w, G->rho_w);
    const TileLaunch L(g, g.Nz - 1);
    if (bm == 3) hipLaunchKernelGGL((k_w_tend_lds<8, 3>), L.grid, L.block, 0, ctx->stream, g, F, L.kc, E);
    else if (bm == 5) hipLaunchKernelGGL((k_w_tend_lds<8, 5>), L.grid, L.block, 0, ctx->stream, g, F, L.kc, E);
    else if (bm == 0) hipLaunchKernelGGL((k_w_tend_lds<8>), L.grid, L.block, 0, ctx->stream, g, F, L.kc, E);
    else if (bm == 1) hipLaunchKernelGGL((k_w_tend_lds<8, 1>), L.grid, L.block, 0, ctx->stream, g, F, L.kc, E);
    else hipLaunchKernelGGL((k_w_tend_lds<8, 2>), L.grid, L.block, 0, ctx->stream, g, F, L.kc, E);
    BZ_LAUNCH_CHECK();
    return BZ_OK;
}

// x-momentum tendency with the u y-stencil in an LDS tile (k_u_tend_lds)
int bzi_u_tendency_lds(bz_ctx *ctx, const bz_state *s, const bz_prognostic *G, const bz_prognostic *U0, const RKEpilogue *Ein)
{
    const DevGrid &g = ctx->dg;
    if (bzi_k6_stored_ok(ctx)) return bzi_k6_stored(ctx, 0, s, G, U0, Ein, 0);
    ProfileScope ps(ctx, Ein ? "x_momentum_tendency+rk3" : "x_momentum_tendency");
    const RKEpilogue E = momentum_epilogue(Ein, U0 ? U0->rho_u : nullptr);
    const Tend3Fields F = momentum_fields(s, s->u, G->rho_u);
    const TileLaunch L(g, g.Nz);
    hipLaunchKernelGGL((k_u_tend_lds<8>), L.grid, L.block, 0, ctx->stream, g, F, L.kc, E);
    BZ_LAUNCH_CHECK();
    return BZ_OK;
}

// y-momentum tendency with every y-stencil in LDS tiles (k_v_tend_lds)
int bzi_v_tendency_lds(bz_ctx *ctx, const bz_state *s, const bz_prognostic *G, const bz_prognostic *U0, const RKEpilogue *Ein)
{
    const DevGrid &g = ctx->dg;
    if (bzi_k6_stored_ok(ctx)) return bzi_k6_stored(ctx, 1, s, G, U0, Ein, 0);
    ProfileScope ps(ctx, Ein ? "y_momentum_tendency+rk3" : "y_momentum_tendency");
    const RKEpilogue E = momentum_epilogue(Ein, U0 ? U0->rho_v : nullptr);
    const Tend3Fields F = momentum_fields(s, s->v, G->rho_v);
    const TileLaunch L(g, g.Nz);
    hipLaunchKernelGGL((k_v_tend_lds<8>), L.grid, L.block, 0, ctx->stream, g, F, L.kc, E);
    BZ_LAUNCH_CHECK();
    return BZ_OK;
}
