// bz_moments.hip — Average(expression, dims = (1, 2)) for the expressions the reference's LES examples write as turbulence statistics:
//   u^2, u*w, θ*w, u^2*w, w^3, ∂z(u), each optionally wrapped in @at((Center, Center, Center), ...)
//                                         examples/neutral_atmospheric_boundary_layer.jl:203-221, rico.jl:281-282,
//                                         tropical_cyclone_world.jl:244-249 of the reference
// Semantics (a READING of Oceananigans' BinaryOperation, ^, ∂z and @at, stated in include/breeze_hip.h): the location L of a moment is its
// first factor's; the other factors are raised to their powers, then brought to L by two-point means (z innermost, x outermost); ∂z is a
// difference over the grid's own spacing; @at brings the field of values at L to the cell centres with the same means.
// bz_horizontal_moments is ONE kernel for a caller-given list of moments: a block owns a (level, row slice) pair as k_havg_partial does, a
// thread the columns i = t, t + 256, ... of every row of the slice, and every moment of the list is evaluated at a group of four of the
// thread's points before the thread moves on, so the neighbour reads that the moments share (a handful of cache lines of at most three
// levels of each field) are served by the L1 / L2 while each field's interior comes from HBM once.  The list is a kernel argument:
// descriptors are decoded with scalar instructions (one decode serves the four points, whose loads are independent; the next descriptor is
// fetched while the current one is evaluated), every branch on them is wave-uniform and the stencil offsets are scalar addends to the
// per-point vector indices.
// A moment is evaluated by the same instructions whatever else is in the list and its sums run in the order of bz_horizontal_average
// (columns of a thread in row order, an LDS tree, the slices in index order): no floating-point atomics, and the bits of a profile do not
// depend on the other moments of the call or on their order.
#include "bz_internal.h"

#define MSLICES 16             // row slices per level: the summation order of bz_horizontal_average (HSLICES of bz_diagnostics.hip)
#define MOM_THREADS 256
#define MOM_POINTS 4           // points a thread evaluates side by side: their loads are independent and one decode of a descriptor serves all

// one factor: the field's parent array, already advanced to the first cell of the factor's stencil, and
// code = power << 4 | x mean << 8 | y mean << 10 | z mean << 12; a mean is 0 (same location), 1 (centre -> face: cells i - 1, i) or
// 2 (face -> centre: faces i, i + 1)
// head of a moment: n_factors | dz << 2 | @at means in x, y, z (faces i, i + 1) << 3, 4, 5 | L is a z face << 6 | levels << 8
struct MomDesc {
    unsigned head;
    unsigned code[BZ_MAX_MOMENT_FACTORS];
    const double *f[BZ_MAX_MOMENT_FACTORS];
};
struct MomArgs {
    MomDesc mom[BZ_MAX_MOMENTS];
    int n;
};
struct MomLevels {
    int nlev[BZ_MAX_MOMENTS];
};

__device__ __forceinline__ double mom_power(double v, int p)
{
    double r = v;
    if (p >= 2) r *= v;
    if (p >= 3) r *= v;
    return r;
}

// ℑ_L(f^p) at the points whose parent indices are n[] + o: the two-point means composed with x outermost and z innermost
__device__ __forceinline__ void mom_factor(const DevGrid &g, const double *__restrict__ f, unsigned code, const long long (&n)[MOM_POINTS],
                                           long long o, double (&out)[MOM_POINTS])
{
    const int p = (int)((code >> 4) & 3u);
    const int mx = (int)((code >> 8) & 3u), my = (int)((code >> 10) & 3u), mz = (int)((code >> 12) & 3u);
    const int nx = mx ? 2 : 1, ny = my ? 2 : 1, nz = mz ? 2 : 1;
    double sx[MOM_POINTS], sy[MOM_POINTS], sz[MOM_POINTS];
#pragma unroll
    for (int u = 0; u < MOM_POINTS; ++u) sx[u] = 0.0;
    for (int a = 0; a < nx; ++a) {
#pragma unroll
        for (int u = 0; u < MOM_POINTS; ++u) sy[u] = 0.0;
        for (int b = 0; b < ny; ++b) {
#pragma unroll
            for (int u = 0; u < MOM_POINTS; ++u) sz[u] = 0.0;
            for (int c = 0; c < nz; ++c) {
                const long long oc = o + (a + (long long)g.Sx * b + g.Sxy * c);
#pragma unroll
                for (int u = 0; u < MOM_POINTS; ++u) sz[u] += mom_power(f[n[u] + oc], p);
            }
#pragma unroll
            for (int u = 0; u < MOM_POINTS; ++u) { if (mz) sz[u] *= 0.5; sy[u] += sz[u]; }
        }
#pragma unroll
        for (int u = 0; u < MOM_POINTS; ++u) { if (my) sy[u] *= 0.5; sx[u] += sy[u]; }
    }
#pragma unroll
    for (int u = 0; u < MOM_POINTS; ++u) out[u] = mx ? sx[u] * 0.5 : sx[u];
}

// the moment's values at the points of L with parent indices n[] + o; dzv: the spacing under a ∂z at these points' level
__device__ __forceinline__ void mom_value(const DevGrid &g, const MomDesc &D, const long long (&n)[MOM_POINTS], long long o, double dzv,
                                          double (&v)[MOM_POINTS])
{
    if (D.head & 4u) {      // ∂z of the single factor: centre -> face k over Δzᵃᵃᶠ[k], face -> centre k over Δzᵃᵃᶜ[k]
        const double *__restrict__ f = D.f[0];
        const long long lo = (D.head & 64u) ? o - g.Sxy : o, hi = lo + g.Sxy;
#pragma unroll
        for (int u = 0; u < MOM_POINTS; ++u) v[u] = (f[n[u] + hi] - f[n[u] + lo]) / dzv;
        return;
    }
    const int nf = (int)(D.head & 3u);
    mom_factor(g, D.f[0], D.code[0], n, o, v);
    double w[MOM_POINTS];      // (static factor indices: the descriptor is a copy in scalar registers)
    if (nf >= 2) {
        mom_factor(g, D.f[1], D.code[1], n, o, w);
#pragma unroll
        for (int u = 0; u < MOM_POINTS; ++u) v[u] *= w[u];
    }
    if (nf >= 3) {
        mom_factor(g, D.f[2], D.code[2], n, o, w);
#pragma unroll
        for (int u = 0; u < MOM_POINTS; ++u) v[u] *= w[u];
    }
}

// stage 1: block (level, slice).  A thread owns the columns i = t, t + 256, ... of every row of the slice and takes its points in that
// order (row by row), MOM_POINTS at a time; acc[m][t] in LDS is its running sum of moment m; then one tree per moment
__global__ __launch_bounds__(MOM_THREADS) void k_moments_partial(DevGrid g, MomArgs A, double *__restrict__ partial)
{
    extern __shared__ double mom_acc[];
    const int k = blockIdx.x, s = blockIdx.y, t = threadIdx.x;
    const int j0 = (int)((long long)g.Ny * s / MSLICES), j1 = (int)((long long)g.Ny * (s + 1) / MSLICES);
    const int cols = (g.Nx + MOM_THREADS - 1) / MOM_THREADS, npts = cols * (j1 - j0);
    const double dzf0 = g.dzf[k], dzf1 = g.dzf[k + 1], dzc0 = g.dzc[k];
    for (int m = 0; m < A.n; ++m) mom_acc[m * MOM_THREADS + t] = 0.0;
    for (int p0 = 0; p0 < npts; p0 += MOM_POINTS) {
        long long n[MOM_POINTS];
        bool valid[MOM_POINTS];
#pragma unroll
        for (int u = 0; u < MOM_POINTS; ++u) {
            const int p = p0 + u, r = p / cols, i = t + MOM_THREADS * (p - r * cols);
            valid[u] = p < npts && i < g.Nx;
            n[u] = valid[u] ? g.idx(i, j0 + r, k) : g.idx(0, j0, k);      // a lane without a point re-reads a valid cell and adds nothing
        }
        MomDesc D = A.mom[0];
        for (int m = 0; m < A.n; ++m) {
            const MomDesc N = A.mom[m + 1 < A.n ? m + 1 : m];      // the next descriptor travels while this one is evaluated
            if (k < (int)(D.head >> 8)) {
                const int cx = (D.head >> 3) & 1u, cy = (D.head >> 4) & 1u, cz = (D.head >> 5) & 1u;
                double vx[MOM_POINTS], vy[MOM_POINTS], vz[MOM_POINTS], v[MOM_POINTS];
#pragma unroll
                for (int u = 0; u < MOM_POINTS; ++u) vx[u] = 0.0;      // @at: faces i, i + 1 -> centre i in every direction where L is a face
                for (int a = 0; a <= cx; ++a) {
#pragma unroll
                    for (int u = 0; u < MOM_POINTS; ++u) vy[u] = 0.0;
                    for (int b = 0; b <= cy; ++b) {
#pragma unroll
                        for (int u = 0; u < MOM_POINTS; ++u) vz[u] = 0.0;
                        for (int c = 0; c <= cz; ++c) {
                            mom_value(g, D, n, a + (long long)g.Sx * b + g.Sxy * c, (D.head & 64u) ? (c ? dzf1 : dzf0) : dzc0, v);
#pragma unroll
                            for (int u = 0; u < MOM_POINTS; ++u) vz[u] += v[u];
                        }
#pragma unroll
                        for (int u = 0; u < MOM_POINTS; ++u) { if (cz) vz[u] *= 0.5; vy[u] += vz[u]; }
                    }
#pragma unroll
                    for (int u = 0; u < MOM_POINTS; ++u) { if (cy) vy[u] *= 0.5; vx[u] += vy[u]; }
                }
                double acc = mom_acc[m * MOM_THREADS + t];
#pragma unroll
                for (int u = 0; u < MOM_POINTS; ++u)
                    if (valid[u]) acc += cx ? vx[u] * 0.5 : vx[u];
                mom_acc[m * MOM_THREADS + t] = acc;
            }
            D = N;
        }
    }
    __syncthreads();
    for (int w = MOM_THREADS / 2; w > 0; w >>= 1) {
        if (t < w)
            for (int m = 0; m < A.n; ++m) mom_acc[m * MOM_THREADS + t] += mom_acc[m * MOM_THREADS + t + w];
        __syncthreads();
    }
    if (t < A.n) partial[((long long)t * (g.Nz + 1) + k) * MSLICES + s] = mom_acc[t * MOM_THREADS];
}

// stage 2: the slices of a (moment, level) in index order, divided by Nx Ny; levels a moment does not have are stored as 0
__global__ __launch_bounds__(256) void k_moments_finish(MomLevels V, int n, const double *__restrict__ partial, double *__restrict__ profiles,
                                                        int nrow, double count)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n * nrow) return;
    const int m = e / nrow, k = e - m * nrow;
    double sum = 0.0;
    if (k < V.nlev[m])
        for (int s = 0; s < MSLICES; ++s) sum += partial[(long long)e * MSLICES + s];
    profiles[e] = sum / count;
}

void bzi_moments_teardown(bz_ctx *ctx)
{
    if (ctx->d_moments) hipFree(ctx->d_moments);
    ctx->d_moments = nullptr;
}

static int mom_mean(int from_face, int to_face) { return from_face == to_face ? 0 : (to_face ? 1 : 2); }

extern "C" int bz_horizontal_moments(bz_ctx *ctx, int32_t n_fields, const bz_moment_field *fields, int32_t n_moments, const bz_moment *moments,
                                     double *profiles, int32_t *nlev)
{
    if (!ctx) return BZ_ERR_INVALID;
    if (!fields || !moments || !profiles || !nlev) { ctx->last_error = "bz_horizontal_moments: null argument"; return BZ_ERR_INVALID; }
    if (ctx->slab_mode) {
        ctx->last_error = "bz_horizontal_moments: not implemented on y-slab contexts (the average needs an all-reduce over the ranks)";
        return BZ_ERR_UNSUPPORTED;
    }
    if (n_fields < 1 || n_fields > BZ_MAX_MOMENT_FIELDS) {
        ctx->last_error = "bz_horizontal_moments: 1 <= n_fields <= BZ_MAX_MOMENT_FIELDS";
        return BZ_ERR_INVALID;
    }
    if (n_moments < 1 || n_moments > BZ_MAX_MOMENTS) {
        ctx->last_error = "bz_horizontal_moments: 1 <= n_moments <= BZ_MAX_MOMENTS";
        return BZ_ERR_INVALID;
    }
    const DevGrid &g = ctx->dg;
    const bool walls = g.bounded_x || g.bounded_y;
    MomArgs A;
    MomLevels levels;
    A.n = n_moments;
    int loc[BZ_MAX_MOMENT_FIELDS][3];
    for (int f = 0; f < n_fields; ++f) {
        if (!fields[f].data) { ctx->last_error = "bz_horizontal_moments: fields[].data is null"; return BZ_ERR_INVALID; }
        const int32_t fl[3] = {fields[f].face_x, fields[f].face_y, fields[f].face_z};
        for (int d = 0; d < 3; ++d) {
            if (fl[d] != 0 && fl[d] != 1) { ctx->last_error = "bz_horizontal_moments: fields[].face_x / face_y / face_z must be 0 or 1"; return BZ_ERR_INVALID; }
            loc[f][d] = fl[d];
        }
        if (g.flat_y) loc[f][1] = 0;      // a Flat y has no location
    }
    for (int m = 0; m < BZ_MAX_MOMENTS; ++m) {
        A.mom[m].head = 0u;
        for (int q = 0; q < BZ_MAX_MOMENT_FACTORS; ++q) { A.mom[m].code[q] = 0u; A.mom[m].f[q] = nullptr; }
        levels.nlev[m] = 0;
    }
    for (int m = 0; m < n_moments; ++m) {
        const bz_moment &M = moments[m];
        if (M.n_factors < 1 || M.n_factors > BZ_MAX_MOMENT_FACTORS) {
            ctx->last_error = "bz_horizontal_moments: moments[].n_factors must be 1 .. BZ_MAX_MOMENT_FACTORS";
            return BZ_ERR_INVALID;
        }
        if ((M.dz != 0 && M.dz != 1) || (M.at_center != 0 && M.at_center != 1)) {
            ctx->last_error = "bz_horizontal_moments: moments[].dz and moments[].at_center must be 0 or 1";
            return BZ_ERR_INVALID;
        }
        for (int q = 0; q < M.n_factors; ++q) {
            if (M.field[q] < 0 || M.field[q] >= n_fields) {
                ctx->last_error = "bz_horizontal_moments: moments[].field is not an index into fields[]";
                return BZ_ERR_INVALID;
            }
            if (M.power[q] < 1 || M.power[q] > 3) { ctx->last_error = "bz_horizontal_moments: moments[].power must be 1 .. 3"; return BZ_ERR_INVALID; }
        }
        if (M.dz && (M.n_factors != 1 || M.power[0] != 1)) {
            ctx->last_error = "bz_horizontal_moments: moments[].dz takes a single factor of power 1";
            return BZ_ERR_INVALID;
        }
        int L[3] = {loc[M.field[0]][0], loc[M.field[0]][1], loc[M.field[0]][2]};
        if (M.dz) L[2] = 1 - L[2];
        unsigned head = (unsigned)M.n_factors | (M.dz ? 4u : 0u) | (L[2] ? 64u : 0u);
        if (M.at_center) head |= (L[0] ? 8u : 0u) | (L[1] ? 16u : 0u) | (L[2] ? 32u : 0u);
        nlev[m] = g.Nz + ((L[2] && !M.at_center) ? 1 : 0);
        head |= (unsigned)nlev[m] << 8;
        A.mom[m].head = head;
        levels.nlev[m] = nlev[m];
        for (int q = 0; q < M.n_factors; ++q) {
            const int *G = loc[M.field[q]];
            if (walls && (G[0] || G[1] || L[0] || L[1])) {
                ctx->last_error = "bz_horizontal_moments: moments at or of horizontal faces are not implemented on a context with walls in x or y";
                return BZ_ERR_UNSUPPORTED;
            }
            const int mx = M.dz ? 0 : mom_mean(G[0], L[0]), my = M.dz ? 0 : mom_mean(G[1], L[1]), mz = M.dz ? 0 : mom_mean(G[2], L[2]);
            // the first cell of the stencil: one cell back in every direction of a centre -> face mean
            const long long first = (mx == 1 ? -1LL : 0LL) + (my == 1 ? -(long long)g.Sx : 0LL) + (mz == 1 ? -g.Sxy : 0LL);
            A.mom[m].f[q] = fields[M.field[q]].data + first;
            A.mom[m].code[q] = ((unsigned)M.power[q] << 4) | ((unsigned)mx << 8) | ((unsigned)my << 10) | ((unsigned)mz << 12);
        }
    }
    // every stencil reaches one cell past the interior at most
    if (g.Hx < 1 || g.Hz < 1 || (!g.flat_y && g.Hy < 1)) {
        ctx->last_error = "bz_horizontal_moments: needs a halo of at least one cell";
        return BZ_ERR_UNSUPPORTED;
    }
    const int nrow = g.Nz + 1;
    if (!ctx->d_moments) BZ_HIP(hipMalloc(&ctx->d_moments, (size_t)BZ_MAX_MOMENTS * nrow * (MSLICES + 1) * sizeof(double)));
    double *partial = ctx->d_moments, *result = ctx->d_moments + (size_t)BZ_MAX_MOMENTS * nrow * MSLICES;
    ProfileScope ps(ctx, "horizontal_moments");
    hipLaunchKernelGGL(k_moments_partial, dim3(nrow, MSLICES), dim3(MOM_THREADS), (size_t)n_moments * MOM_THREADS * sizeof(double), ctx->stream,
                       g, A, partial);
    BZ_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_moments_finish, dim3((n_moments * nrow + 255) / 256), dim3(256), 0, ctx->stream, levels, (int)n_moments, partial, result,
                       nrow, (double)((long long)g.Nx * g.Ny));
    BZ_LAUNCH_CHECK();
    BZ_HIP(hipMemcpyAsync(profiles, result, (size_t)n_moments * nrow * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    BZ_HIP(hipStreamSynchronize(ctx->stream));
    return BZ_OK;
}
