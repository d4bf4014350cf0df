// bz_azimuthal.hip — the analysis of the reference's tropical-cyclone examples on the device:
//   azimuthal_mean(field; radius, Nr, center, m)      src/AtmosphereModels/Diagnostics/azimuthal_mean.jl:36-92 of the reference
//   the polar wind components v_theta, v_r at cell centres (examples/tropical_cyclone_with_rainband.jl: Field((-y u + x v) / r))
// The reference's kernel is one thread per (ring, level) that walks all Nx Ny m^2 samples.  Ring membership depends on (i, j) only, so
// here it is worked out ONCE per geometry (k_az_plan): per cell the first ring it touches and how many of its m^2 samples fall into
// each of the W consecutive rings from there (W from the cell diagonal and the ring width, on the host).  The plan stays on the context,
// keyed on (center, radius, Nr, m): the example reduces v_theta and theta with one geometry.
// The sums (k_az_partial) use f n(cell, ring) instead of n repeated additions.  A block owns (level, slice of rows); a wave loads 64
// consecutive cells of a row coalesced and walks them in order, broadcasting (f, first ring) from lane to scalar registers; lane l owns the
// rings l + 64 q and adds its share, so a ring's partial sum is accumulated by ONE lane in cell order.  The four waves of a block are
// added in wave order, the slices in index order (k_az_finish), then one division by the count: no floating-point atomics, nothing depends
// on scheduling, two calls give the same bits.  Counts are integers (LDS histogram + integer atomics).
// Bin membership is the reference's expression in the reference's operation order with FMA contraction off (az_ring); divide and sqrt are
// the correctly rounded ones (no fast-math flag in any build of this file; -fhip-fp32-correctly-rounded-divide-sqrt is the default).
#include "bz_internal.h"

#include <cmath>

#define AZ_SLICES 16           // row slices per level
#define AZ_MAX_NR 1024         // rings: lane l of a wave owns the rings l + 64 q, q < 16
#define AZ_MAX_M 16            // m^2 <= 256 samples per cell

struct AzPlan {
    double *d_xc = nullptr, *d_yc = nullptr;      // x^c[0 .. Nx), y^c[0 .. Ny) as the host's grid holds them (bz_set_horizontal_nodes)
    // the cached geometry
    bool valid = false;
    double cx = 0.0, cy = 0.0, radius = 0.0;
    int Nr = 0, m = 0, W = 0;
    int *d_first = nullptr;                        // per cell: first ring touched, -1 when no sample lies inside the radius
    unsigned short *d_cnt = nullptr;               // per cell: samples in ring first + o, o < W (rows of max(W, 4) entries)
    unsigned long long *d_counts = nullptr;        // per ring: samples; entry Nr: set when a cell spans more than W rings (never, by construction)
    double *d_partial = nullptr, *d_result = nullptr;
    size_t cap_first = 0, cap_cnt = 0, cap_counts = 0, cap_partial = 0, cap_result = 0;
    std::vector<unsigned long long> h_counts;
};

// ring (0-based) of sample (si, sj), 1 <= si, sj <= m, of the cell whose centre is (x0, y0) from the centre of the rings; -1 past the radius.
// azimuthal_mean.jl:82-84: x = x0 + (2 si - m - 1) dx / (2 m), in_ring = unsafe_trunc(Int, sqrt(x^2 + y^2) / dr) + 1 == ir
__device__ __forceinline__ int az_ring(double x0, double y0, double dx, double dy, int si, int sj, int m, double dr, int Nr)
{
#pragma clang fp contract(off)
    const double x = x0 + (double)(2 * si - m - 1) * dx / (double)(2 * m);
    const double y = y0 + (double)(2 * sj - m - 1) * dy / (double)(2 * m);
    const double q = sqrt(x * x + y * y) / dr;
    return q < (double)Nr ? (int)q : -1;
}

__global__ __launch_bounds__(256) void k_az_plan(DevGrid g, const double *__restrict__ xc, const double *__restrict__ yc, double cx, double cy,
                                                 double dr, int Nr, int m, int W, int S, int *__restrict__ first, unsigned short *__restrict__ cnt,
                                                 unsigned long long *__restrict__ counts)
{
    extern __shared__ unsigned int az_hist[];      // Nr
    for (int r = threadIdx.x; r < Nr; r += 256) az_hist[r] = 0u;
    __syncthreads();
    const int i = blockIdx.x * 256 + threadIdx.x, j = blockIdx.y;
    if (i < g.Nx) {
        const double x0 = xc[i] - cx, y0 = yc[j] - cy;
        int lo = Nr;
        for (int sj = 1; sj <= m; ++sj)
            for (int si = 1; si <= m; ++si) {
                const int b = az_ring(x0, y0, g.dx, g.dy, si, sj, m, dr, Nr);
                if (b >= 0 && b < lo) lo = b;
            }
        const long long cell = (long long)j * g.Nx + i;
        first[cell] = lo < Nr ? lo : -1;
        unsigned short *row = cnt + cell * S;      // S >= W: the row stride (padded to 4 entries = one 64-bit word when W <= 4)
        for (int o = 0; o < S; ++o) row[o] = 0;
        if (lo < Nr)
            for (int sj = 1; sj <= m; ++sj)
                for (int si = 1; si <= m; ++si) {
                    const int b = az_ring(x0, y0, g.dx, g.dy, si, sj, m, dr, Nr);
                    if (b < 0) continue;
                    if (b - lo < W) row[b - lo] += 1;
                    else atomicOr(&counts[Nr], 1ull);
                    atomicAdd(&az_hist[b], 1u);
                }
    }
    __syncthreads();
    for (int r = threadIdx.x; r < Nr; r += 256)
        if (az_hist[r]) atomicAdd(&counts[r], (unsigned long long)az_hist[r]);
}

// lane l's value in a scalar register (l wave-uniform), for either float width
template <typename T> __device__ __forceinline__ T az_readlane(T v, int l)
{
    int w[sizeof(T) / 4];
    __builtin_memcpy(w, &v, sizeof(T));
    for (int n = 0; n < (int)(sizeof(T) / 4); ++n) w[n] = __builtin_amdgcn_readlane(w[n], l);
    __builtin_memcpy(&v, w, sizeof(T));
    return v;
}

// Q: accumulators per lane (Nr <= 64 Q).  PACK: W <= 4, a cell's counts are one 64-bit word that its lane loads with the chunk and the walk
// broadcasts like f, so the loop over the cells touches no memory; otherwise the owning lanes read their count from the cell's row.
template <int Q, bool PACK>
__global__ __launch_bounds__(256) void k_az_partial(DevGrid g, const double *__restrict__ f, const int *__restrict__ first,
                                                    const unsigned short *__restrict__ cnt, int W, int Nr, double *__restrict__ partial)
{
    const int k = blockIdx.x, s = blockIdx.y;
    const int j0 = (int)((long long)g.Ny * s / AZ_SLICES), j1 = (int)((long long)g.Ny * (s + 1) / AZ_SLICES);
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int nch = (g.Nx + 63) >> 6, nchunks = (j1 - j0) * nch;
    double acc[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) acc[q] = 0.0;
    for (int c = wave; c < nchunks; c += 4) {
        const int j = j0 + c / nch, i0 = (c % nch) << 6;
        const int n = g.Nx - i0 < 64 ? g.Nx - i0 : 64;
        const long long cell0 = (long long)j * g.Nx + i0;
        double fv = 0.0;
        int fr = -1;
        unsigned long long pk = 0ull;
        if (lane < n) {
            fv = f[g.idx(i0 + lane, j, k)];
            fr = first[cell0 + lane];
            if (PACK) pk = reinterpret_cast<const unsigned long long *>(cnt)[cell0 + lane];
        }
        for (int l = 0; l < n; ++l) {
            const int fl = __builtin_amdgcn_readlane(fr, l);
            if (fl < 0) continue;                  // no sample of this cell inside the radius: its value is not used at all
            const double fs = az_readlane(fv, l);
            const unsigned long long ps = PACK ? az_readlane(pk, l) : 0ull;
            const unsigned short *row = cnt + (cell0 + l) * W;
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                if (fl + W <= 64 * q || fl >= 64 * q + 64) continue;      // wave-uniform
                const int o = 64 * q + lane - fl;
                if ((unsigned)o < (unsigned)W) {
                    // W is an upper bound: most cells have zero entries at the end of their row.  A zero count adds nothing — not even
                    // f * 0, which would be NaN for a non-finite f in a ring the reference's membership test keeps it out of
                    const unsigned nsamp = PACK ? (unsigned)((ps >> (16 * o)) & 0xffffull) : (unsigned)row[o];
                    if (nsamp) acc[q] += fs * (double)nsamp;
                }
            }
        }
    }
    __shared__ double red[4 * Q * 64];
#pragma unroll
    for (int q = 0; q < Q; ++q) red[(wave * Q + q) * 64 + lane] = acc[q];
    __syncthreads();
    for (int r = threadIdx.x; r < Nr; r += 256) {
        double sum = red[r];
        for (int w = 1; w < 4; ++w) sum += red[w * Q * 64 + r];
        partial[((long long)k * AZ_SLICES + s) * Nr + r] = sum;
    }
}

__global__ __launch_bounds__(256) void k_az_finish(const double *__restrict__ partial, const unsigned long long *__restrict__ counts,
                                                   double *__restrict__ profile, int nlev, int Nr)
{
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= nlev * Nr) return;
    const int k = n / Nr, r = n % Nr;
    double sum = 0.0;
    for (int s = 0; s < AZ_SLICES; ++s) sum += partial[((long long)k * AZ_SLICES + s) * Nr + r];
    const unsigned long long c = counts[r];
    profile[n] = c ? sum / (double)c : (double)NAN;
}

__global__ __launch_bounds__(256) void k_polar_winds(DevGrid g, const double *__restrict__ u, const double *__restrict__ v,
                                                     const double *__restrict__ xc, const double *__restrict__ yc, double cx, double cy,
                                                     double *__restrict__ vt, double *__restrict__ vr)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y, k = blockIdx.z;
    if (i >= g.Nx) return;
    const long long n = g.idx(i, j, k);
    const double uc = (u[n] + u[n + 1]) / 2.0, vc = (v[n] + v[n + g.Sx]) / 2.0;
    const double x = xc[i] - cx, y = yc[j] - cy;
    const double r = sqrt(x * x + y * y);
    if (vt) vt[n] = (-y * uc + x * vc) / r;
    if (vr) vr[n] = (x * uc + y * vc) / r;
}

static AzPlan *az_get(bz_ctx *ctx)
{
    if (!ctx->az) ctx->az = new AzPlan();
    return ctx->az;
}

void bzi_azimuthal_teardown(bz_ctx *ctx)
{
    AzPlan *P = ctx->az;
    if (!P) return;
    void *bufs[] = {P->d_xc, P->d_yc, P->d_first, P->d_cnt, P->d_counts, P->d_partial, P->d_result};
    for (void *b : bufs)
        if (b) hipFree(b);
    delete P;
    ctx->az = nullptr;
}

extern "C" int bz_set_horizontal_nodes(bz_ctx *ctx, const double *xc, const double *yc)
{
    if (!ctx || !xc || !yc) return BZ_ERR_INVALID;
    AzPlan *P = az_get(ctx);
    const DevGrid &g = ctx->dg;
    if (!P->d_xc) BZ_HIP(hipMalloc(&P->d_xc, (size_t)g.Nx * sizeof(double)));
    if (!P->d_yc) BZ_HIP(hipMalloc(&P->d_yc, (size_t)g.Ny * sizeof(double)));
    P->valid = false;
    BZ_HIP(hipMemcpyAsync(P->d_xc, xc, (size_t)g.Nx * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    BZ_HIP(hipMemcpyAsync(P->d_yc, yc, (size_t)g.Ny * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    BZ_HIP(hipStreamSynchronize(ctx->stream));      // the host arrays are the caller's
    return BZ_OK;
}

#define AZ_GROW(ptr, cap, bytes)                                                            \
    do {                                                                                    \
        if ((cap) < (size_t)(bytes)) {                                                      \
            if (ptr) hipFree(ptr);                                                          \
            (ptr) = nullptr; (cap) = 0;                                                     \
            BZ_HIP(hipMalloc(&(ptr), (size_t)(bytes)));                                     \
            (cap) = (size_t)(bytes);                                                        \
        }                                                                                   \
    } while (0)

extern "C" int bz_azimuthal_mean(bz_ctx *ctx, const double *field, int z_face, double center_x, double center_y, double radius, int32_t Nr,
                                 int32_t m, double *profile, int64_t *counts)
{
    if (!ctx || !field || !profile) return BZ_ERR_INVALID;
    if (ctx->slab_mode) {
        ctx->last_error = "bz_azimuthal_mean: not implemented on y-slab contexts (the ring sums need an all-reduce over the ranks)";
        return BZ_ERR_UNSUPPORTED;
    }
    if (ctx->dg.flat_y) {
        ctx->last_error = "bz_azimuthal_mean: not defined on a Flat y (topology (Periodic, Flat, Bounded))";
        return BZ_ERR_UNSUPPORTED;
    }
    if (Nr < 1 || Nr > AZ_MAX_NR) { ctx->last_error = "bz_azimuthal_mean: Nr must be between 1 and 1024"; return BZ_ERR_INVALID; }
    if (m < 1 || m > AZ_MAX_M) { ctx->last_error = "bz_azimuthal_mean: m must be between 1 and 16"; return BZ_ERR_INVALID; }
    if (!(radius > 0.0) || !std::isfinite(radius)) { ctx->last_error = "bz_azimuthal_mean: radius must be positive and finite"; return BZ_ERR_INVALID; }
    AzPlan *P = az_get(ctx);
    if (!P->d_xc || !P->d_yc) {
        ctx->last_error = "bz_azimuthal_mean: the cell-centre coordinates are not set (bz_set_horizontal_nodes)";
        return BZ_ERR_INVALID;
    }
    const DevGrid &g = ctx->dg;
    const int nlev = g.Nz + (z_face ? 1 : 0);
    const double dr = radius / (double)Nr;
    const size_t cells = (size_t)g.Nx * g.Ny;
    ProfileScope ps(ctx, "azimuthal_mean");
    if (!(P->valid && P->cx == center_x && P->cy == center_y && P->radius == radius && P->Nr == Nr && P->m == m)) {
        P->valid = false;
        // rings one cell can touch: two samples of a cell are less than its diagonal apart, so their ring indices differ by at most
        // floor(diagonal / dr) + 1; one more for the rounding of the two quotients
        const double span = std::sqrt(g.dx * g.dx + g.dy * g.dy) / dr;
        const int W = span < (double)Nr ? ((int)span + 3 < Nr ? (int)span + 3 : Nr) : Nr;
        const int S = W <= 4 ? 4 : W;      // row stride of the table: one 64-bit word per cell when it fits (k_az_partial<Q, true>)
        if (cells * (size_t)S * sizeof(unsigned short) > ((size_t)1 << 31)) {
            ctx->last_error = "bz_azimuthal_mean: Nr is too fine for this grid (the per-cell ring table would exceed 2 GiB)";
            return BZ_ERR_UNSUPPORTED;
        }
        AZ_GROW(P->d_first, P->cap_first, cells * sizeof(int));
        AZ_GROW(P->d_cnt, P->cap_cnt, cells * (size_t)S * sizeof(unsigned short));
        AZ_GROW(P->d_counts, P->cap_counts, (size_t)(AZ_MAX_NR + 1) * sizeof(unsigned long long));
        BZ_HIP(hipMemsetAsync(P->d_counts, 0, (size_t)(Nr + 1) * sizeof(unsigned long long), ctx->stream));
        hipLaunchKernelGGL(k_az_plan, dim3((g.Nx + 255) / 256, g.Ny), dim3(256), (size_t)Nr * sizeof(unsigned int), ctx->stream, g, P->d_xc,
                           P->d_yc, center_x, center_y, dr, (int)Nr, (int)m, W, S, P->d_first, P->d_cnt, P->d_counts);
        BZ_LAUNCH_CHECK();
        P->h_counts.assign((size_t)Nr + 1, 0ull);
        BZ_HIP(hipMemcpyAsync(P->h_counts.data(), P->d_counts, (size_t)(Nr + 1) * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
        BZ_HIP(hipStreamSynchronize(ctx->stream));
        if (P->h_counts[Nr]) {
            // an invariant of the library, not a fault of the arguments: reported like a device-side failure (a negated hipError_t)
            ctx->last_error = "bz_azimuthal_mean: internal error: a cell spans more rings than its table holds";
            return -(int)hipErrorAssert;
        }
        P->cx = center_x; P->cy = center_y; P->radius = radius; P->Nr = Nr; P->m = m; P->W = W;
        P->valid = true;
    }
    AZ_GROW(P->d_partial, P->cap_partial, (size_t)nlev * AZ_SLICES * Nr * sizeof(double));
    AZ_GROW(P->d_result, P->cap_result, (size_t)nlev * Nr * sizeof(double));
    const dim3 grid(nlev, AZ_SLICES), block(256);
    const bool pack = P->W <= 4;
#define AZ_LAUNCH(Q, PACK)                                                                                                         \
    hipLaunchKernelGGL((k_az_partial<Q, PACK>), grid, block, 0, ctx->stream, g, field, P->d_first, P->d_cnt, P->W, (int)Nr, P->d_partial)
    if (Nr <= 64) { if (pack) AZ_LAUNCH(1, true); else AZ_LAUNCH(1, false); }
    else if (Nr <= 256) { if (pack) AZ_LAUNCH(4, true); else AZ_LAUNCH(4, false); }
    else { if (pack) AZ_LAUNCH(16, true); else AZ_LAUNCH(16, false); }
#undef AZ_LAUNCH
    BZ_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_az_finish, dim3((nlev * Nr + 255) / 256), dim3(256), 0, ctx->stream, P->d_partial, P->d_counts, P->d_result, nlev,
                       (int)Nr);
    BZ_LAUNCH_CHECK();
    BZ_HIP(hipMemcpyAsync(profile, P->d_result, (size_t)nlev * Nr * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    BZ_HIP(hipStreamSynchronize(ctx->stream));
    if (counts)
        for (int r = 0; r < Nr; ++r) counts[r] = (int64_t)P->h_counts[r];
    return BZ_OK;
}

extern "C" int bz_polar_winds(bz_ctx *ctx, const double *u, const double *v, double center_x, double center_y, double *tangential,
                              double *radial)
{
    if (!ctx || !u || !v) return BZ_ERR_INVALID;
    if (!tangential && !radial) { ctx->last_error = "bz_polar_winds: both outputs are NULL"; return BZ_ERR_INVALID; }
    const DevGrid &g = ctx->dg;
    if (g.flat_y) {
        ctx->last_error = "bz_polar_winds: not defined on a Flat y (topology (Periodic, Flat, Bounded))";
        return BZ_ERR_UNSUPPORTED;
    }
    if (g.Hx < 1 || g.Hy < 1) { ctx->last_error = "bz_polar_winds: needs halos >= 1 in x and y"; return BZ_ERR_UNSUPPORTED; }
    AzPlan *P = az_get(ctx);
    if (!P->d_xc || !P->d_yc) {
        ctx->last_error = "bz_polar_winds: the cell-centre coordinates are not set (bz_set_horizontal_nodes)";
        return BZ_ERR_INVALID;
    }
    ProfileScope ps(ctx, "polar_winds");
    const int bs = g.Nx <= 64 ? 64 : (g.Nx <= 128 ? 128 : 256);
    hipLaunchKernelGGL(k_polar_winds, dim3((g.Nx + bs - 1) / bs, g.Ny, g.Nz), dim3(bs), 0, ctx->stream, g, u, v, P->d_xc, P->d_yc, center_x,
                       center_y, tangential, radial);
    BZ_LAUNCH_CHECK();
    return BZ_OK;
}
