// bz_cmp_scalar.hip — slow scalar tendencies of CompressibleDynamics: the WENO-5 flux divergence with the 3-D carrier density in its three
// generations (the only reconstructions of the compressible units) and the entry points that launch it.
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "bz_compressible_internal.h"

// ---------------------------------------------------------------------------------------------------------------------
// slow scalar tendencies: G_rho_theta = -div_rhoUc(theta) with the 3-D carrier density (src/Advection.jl:20-35) and,
// when Grho != nullptr, G_rho_d = -div(momentum) (compressible_density_tendency.jl:52-55)
// ---------------------------------------------------------------------------------------------------------------------
#include "bz_weno.h"

// Walls in y (topology (Periodic, Bounded, Bounded)): the WY instantiations of the ragged and of the LDS-tiled kernel reconstruct the scalar in
// y with the buffer that fits at the face's row — WENO5 at faces 3 .. Ny-3, WENO3 at faces 2 and Ny-2, first-order upwind at faces 1 and
// Ny-1 and at the wall faces 0 and Ny, whose flux is the exact zero of their v — the rule of the per-operator kernels (bz_tendency.hip: by_face).
// A wavefront is one row: the buffer is wave-uniform and sits in a scalar register.  The density at a y face is the same two-point mean, read
// through the no-flux halo row; G_rho takes rho v of face Ny from the first upper halo row (a zero).  WY = false compiles to the code it replaced.
template <bool WY>
__device__ __forceinline__ int by_face_c(const DevGrid &g, int j)
{
    if constexpr (WY) return __builtin_amdgcn_readfirstlane(bz_buffer_face(j, g.Ny));
    else return 3;
}
template <bool WY>
__device__ __forceinline__ double bz_up5y_c(double m3, double m2, double m1, double p0, double p1, double p2, bool left, int B)
{
    if constexpr (WY) return bz_upB(m3, m2, m1, p0, p1, p2, left, B);
    else return bz_up5(m3, m2, m1, p0, p1, p2, left);
}

#define CTY 4
template <bool WY>
__global__ __launch_bounds__(64 * CTY) void k_scalar_tendency_rho3d(DevGrid g, double *__restrict__ Gc, double *__restrict__ Grho,
                                                                   const double *__restrict__ rho, const double *__restrict__ u,
                                                                   const double *__restrict__ v, const double *__restrict__ w,
                                                                   const double *__restrict__ c, const double *__restrict__ ru,
                                                                   const double *__restrict__ rv, const double *__restrict__ rw,
                                                                   int kchunk, const int *__restrict__ zero_if_dry)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    const int j = blockIdx.y * CTY + threadIdx.y;
    if (i >= g.Nx || j >= g.Ny) return;
    const int k0 = blockIdx.z * kchunk;
    const int k1 = min(k0 + kchunk, g.Nz);
    const long long sy = g.Sx, sz = g.Sxy;
    long long n = g.idx(i, j, k0);
    const int Bylo = by_face_c<WY>(g, j), Byhi = by_face_c<WY>(g, j + 1);
    // moisture launch of a dry model (the moisture scan's word, bz_moisture.hip: bzi_scan_moisture): the advected field is identically zero,
    // every flux an exact zero — the tendency is written as such without reading anything
    if (zero_if_dry && __builtin_amdgcn_readfirstlane(*zero_if_dry) == 1) {
        for (int k = k0; k < k1; ++k, n += sz) Gc[n] = 0.0;
        return;
    }

    double zm3 = c[n - 3 * sz], zm2 = c[n - 2 * sz], zm1 = c[n - sz], z0 = c[n], zp1 = c[n + sz], zp2 = c[n + 2 * sz];
    double r_lo = rho[n - sz], r0 = rho[n];
    double Fz_lo;
    {
        const double wt = w[n];
        const double cR = bz_upB(zm3, zm2, zm1, z0, zp1, zp2, wt > 0.0, bz_buffer_face(k0, g.Nz));
        Fz_lo = ((r0 + r_lo) / 2.0) * ((g.Az * wt) * cR);
    }
    for (int k = k0; k < k1; ++k, n += sz) {
        const double zp3 = c[n + 3 * sz];
        const double r_hi = rho[n + sz];
        double Fz_hi;
        {
            const double wt = w[n + sz];
            const double cR = bz_upB(zm2, zm1, z0, zp1, zp2, zp3, wt > 0.0, bz_buffer_face(k + 1, g.Nz));
            Fz_hi = ((r_hi + r0) / 2.0) * ((g.Az * wt) * cR);
        }
        const double Ax = g.Ax[k], Ay = g.Ay[k];
        const double xm3 = c[n - 3], xm2 = c[n - 2], xm1 = c[n - 1], xp1 = c[n + 1], xp2 = c[n + 2], xp3 = c[n + 3];
        const double u0 = u[n], u1 = u[n + 1];
        const double Fx_lo = ((r0 + rho[n - 1]) / 2.0) * ((Ax * u0) * bz_up5(xm3, xm2, xm1, z0, xp1, xp2, u0 > 0.0));
        const double Fx_hi = ((rho[n + 1] + r0) / 2.0) * ((Ax * u1) * bz_up5(xm2, xm1, z0, xp1, xp2, xp3, u1 > 0.0));
        double Fy_lo = 0.0, Fy_hi = 0.0;
        if (!g.flat_y) {
            const double ym3 = c[n - 3 * sy], ym2 = c[n - 2 * sy], ym1 = c[n - sy], yp1 = c[n + sy], yp2 = c[n + 2 * sy], yp3 = c[n + 3 * sy];
            const double v0 = v[n], v1 = v[n + sy];
            Fy_lo = ((r0 + rho[n - sy]) / 2.0) * ((Ay * v0) * bz_up5y_c<WY>(ym3, ym2, ym1, z0, yp1, yp2, v0 > 0.0, Bylo));
            Fy_hi = ((rho[n + sy] + r0) / 2.0) * ((Ay * v1) * bz_up5y_c<WY>(ym2, ym1, z0, yp1, yp2, yp3, v1 > 0.0, Byhi));
        }
        Gc[n] = -(g.Vinv_c[k] * ((Fx_hi - Fx_lo) + (Fy_hi - Fy_lo) + (Fz_hi - Fz_lo)));
        if (Grho) {
            const double a = Ax * ru[n + 1] - Ax * ru[n];
            const double b = g.flat_y ? 0.0 : Ay * rv[n + sy] - Ay * rv[n];
            const double cc = g.Az * rw[n + sz] - g.Az * rw[n];
            Grho[n] = -(g.Vinv_c[k] * (a + b + cc));
        }
        zm3 = zm2; zm2 = zm1; zm1 = z0; z0 = zp1; zp1 = zp2; zp2 = zp3;
        Fz_lo = Fz_hi;
        r_lo = r0; r0 = r_hi;
    }
}

// The same tendency with every face flux evaluated ONCE (round 4).  The kernel above evaluates both x faces, both y faces and the upper
// z face of its cell: five order-5 reconstructions per cell where three are needed.  Here a thread evaluates the fluxes through its
// low x face and low y face and through the upper z face; the high x-face flux comes from the next lane (the one beyond the tile edge:
// one evaluation per lane for the 64 levels of the march, read back with a second shuffle), the high y-face flux through an LDS row
// exchange of CTY levels at a time in which wave l evaluates the row outside the tile for level l (every wave: 3 CTY + 1 reconstructions
// per group).  Same expressions per flux; the differences see rounded fluxes (bz_sub_rounded_c), where the kernel above lets the compiler
// contract one of each pair into an fma — results differ from it by an ulp of a flux, both within 1e-12 of the oracle.
// grid (Nx / 64, Ny / CTY, ceil(Nz / 64)): rows of a multiple of 64 cells, Ny a multiple of CTY, not Flat; halo rows in y are read as
// they are (periodic images or a slab neighbour's rows).
__device__ __forceinline__ double bz_sub_rounded_c(double a, double b)
{
#pragma clang fp contract(off)
    return a - b;
}
__global__ __launch_bounds__(64 * CTY) void k_scalar_tendency_rho3d_x(DevGrid g, double *__restrict__ Gc, double *__restrict__ Grho,
                                                                     const double *__restrict__ rho, const double *__restrict__ u,
                                                                     const double *__restrict__ v, const double *__restrict__ w,
                                                                     const double *__restrict__ c, const double *__restrict__ ru,
                                                                     const double *__restrict__ rv, const double *__restrict__ rw,
                                                                     const int *__restrict__ zero_if_dry, int kchunk)
{
    __shared__ double FY[2][CTY][CTY + 1][64];
    __shared__ double AX[CTY][CTY][64], AZ[CTY][CTY][64];
    const int tx = threadIdx.x, ty = threadIdx.y;
    // Round 6: every XCD owns a band of tile rows (gridDim.y a multiple of 8).  A 64 x 4 tile reads nine rows of c for its four (y stencil)
    // and the row below of rho; in launch order (x fastest, round-robin over the eight XCDs) the tiles above and below sit behind other
    // L2s and every tile fetched its frame itself: PMC 1.4 x the compulsory bytes at 5.4 TB/s of real traffic — the kernel was
    // bandwidth-bound on re-reads.  (A pipelined form — next level's loads in flight — was measured equal and removed.)
    int bxr = blockIdx.x, byr = blockIdx.y;
    if ((gridDim.y & 7u) == 0) {
        const unsigned wv = blockIdx.y * gridDim.x + blockIdx.x, cx = wv & 7u, rr = wv >> 3;
        bxr = (int)(rr % gridDim.x);
        byr = (int)(cx * (gridDim.y >> 3) + rr / gridDim.x);
    }
    const int i0 = bxr * 64, j0 = byr * CTY, i = i0 + tx, j = j0 + ty;
    const int k0 = blockIdx.z * kchunk, k1 = min(k0 + kchunk, g.Nz);      // kchunk <= 64: one edge flux per lane
    const long long sy = g.Sx, sz = g.Sxy;
    long long n = g.idx(i, j, k0);
    if (zero_if_dry && __builtin_amdgcn_readfirstlane(*zero_if_dry) == 1) {
        for (int k = k0; k < k1; ++k, n += sz) Gc[n] = 0.0;
        return;
    }
    auto FX = [&](long long m, int k) {      // flux through the low x face of cell m
        const double u0 = u[m];
        return ((rho[m] + rho[m - 1]) / 2.0) * ((g.Ax[k] * u0) * bz_up5(c[m - 3], c[m - 2], c[m - 1], c[m], c[m + 1], c[m + 2], u0 > 0.0));
    };
    auto FYf = [&](long long m, int k) {     // low y face
        const double v0 = v[m];
        return ((rho[m] + rho[m - sy]) / 2.0) *
               ((g.Ay[k] * v0) * bz_up5(c[m - 3 * sy], c[m - 2 * sy], c[m - sy], c[m], c[m + sy], c[m + 2 * sy], v0 > 0.0));
    };
    double edge;
    {
        const int kk = min(k0 + tx, k1 - 1);
        edge = FX(g.idx(i0 + 64, j, kk), kk);
    }
    const long long nx0 = g.idx(i, j0 + CTY, k0);
    double zm3 = c[n - 3 * sz], zm2 = c[n - 2 * sz], zm1 = c[n - sz], z0 = c[n], zp1 = c[n + sz], zp2 = c[n + 2 * sz];
    double r_lo = rho[n - sz], r0 = rho[n];
    double Fz_lo;
    {
        const double wt = w[n];
        const double cR = bz_upB(zm3, zm2, zm1, z0, zp1, zp2, wt > 0.0, bz_buffer_face(k0, g.Nz));
        Fz_lo = ((r0 + r_lo) / 2.0) * ((g.Az * wt) * cR);
    }
    int buf = 0;
    for (int k = k0; k < k1; k += CTY, n += CTY * sz) {
        const int nl = min(CTY, k1 - k);
#pragma unroll 1
        for (int l = 0; l < nl; ++l) {
            const int kl = k + l;
            const long long m = n + l * sz;
            // Round 6: every load of the level first.  The reconstructions branch on the wave's upwind direction (bz_up5), so a load written
            // inside a flux expression stays in that flux's basic block: the ISA of the round-4 form drained the memory counter four
            // times per level (z, x, y, outside row).  Same expressions, same bits.
            const double zp3 = c[m + 3 * sz];
            const double r_hi = rho[m + sz];
            const double wt = w[m + sz];
            const double u0 = u[m], rxm = rho[m - 1];
            const double xm3 = c[m - 3], xm2 = c[m - 2], xm1 = c[m - 1], xp1 = c[m + 1], xp2 = c[m + 2];
            const double v0 = v[m], rym = rho[m - sy];
            const double ym3 = c[m - 3 * sy], ym2 = c[m - 2 * sy], ym1 = c[m - sy], yp1 = c[m + sy], yp2 = c[m + 2 * sy];
            const double cR = bz_upB(zm2, zm1, z0, zp1, zp2, zp3, wt > 0.0, bz_buffer_face(kl + 1, g.Nz));
            const double Fz_hi = ((r_hi + r0) / 2.0) * ((g.Az * wt) * cR);
            AZ[l][ty][tx] = bz_sub_rounded_c(Fz_hi, Fz_lo);
            // (z0 = c[m] and r0 = rho[m]: the ring values of this level)
            const double fx = ((r0 + rxm) / 2.0) * ((g.Ax[kl] * u0) * bz_up5(xm3, xm2, xm1, z0, xp1, xp2, u0 > 0.0));
            // neighbour lane's flux by a DPP move, the out-of-wave one by v_readlane (bz_internal.h; kl - k0 is wave-uniform); whole rows only,
            // so lane 63, which the shift leaves at 0, is always replaced
            double nb = bz_lane_down(fx);
            const double e = bz_lane_read(edge, kl - k0);
            if (tx == 63) nb = e;
            AX[l][ty][tx] = bz_sub_rounded_c(nb, fx);
            FY[buf][l][ty][tx] = ((r0 + rym) / 2.0) * ((g.Ay[kl] * v0) * bz_up5(ym3, ym2, ym1, z0, yp1, yp2, v0 > 0.0));
            if (ty == l) FY[buf][l][CTY][tx] = FYf(nx0 + (long long)(kl - k0) * sz, kl);      // the row outside the tile: one wave per level
            zm3 = zm2; zm2 = zm1; zm1 = z0; z0 = zp1; zp1 = zp2; zp2 = zp3;
            Fz_lo = Fz_hi;
            r_lo = r0; r0 = r_hi;
        }
        __syncthreads();
#pragma unroll 1
        for (int l = 0; l < nl; ++l) {
            const int kl = k + l;
            const long long m = n + l * sz;
            const double dy = bz_sub_rounded_c(FY[buf][l][ty + 1][tx], FY[buf][l][ty][tx]);
            Gc[m] = -(g.Vinv_c[kl] * (AX[l][ty][tx] + dy + AZ[l][ty][tx]));
            if (Grho) {
                const double Ax = g.Ax[kl], Ay = g.Ay[kl];
                const double a = Ax * ru[m + 1] - Ax * ru[m];
                const double b = Ay * rv[m + sy] - Ay * rv[m];
                const double cc = g.Az * rw[m + sz] - g.Az * rw[m];
                Grho[m] = -(g.Vinv_c[kl] * (a + b + cc));
            }
        }
        buf ^= 1;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Round 6: the same tendency with every stencil read from LDS tiles (the structure of k6_u, bz_tendency5_kernels.h).  The kernel above
// issues 22 vector-memory instructions per wave and level (stencils straight from the L1) and keeps a CU's address path 84 - 95 % busy
// (tools/gpu_sq_one_kernel.sh: ~32 TA cycles per 64-lane 8-byte load) at 1.3 x its compulsory bytes; here a 64 x SLT tile stages c with
// its three-cell frame and rho with its low-side frame once per level (double-buffered; every global load of an iteration is a prefetch
// for the NEXT level: ring tops, the thread's frame cells, its u, v, w), the x and y stencils are ds_reads, the high x-face flux comes
// from the next lane (beyond the tile: one evaluation per lane for 64 levels), the high y-face flux from the row above through LDS (the
// row outside the tile: wave 0).  7 loads per thread and level (13 with G_rho).  Same expressions per flux as k_scalar_tendency_rho3d_x:
// same bits.  grid (Nx / 64, Ny / SLT, chunks): Nx a multiple of 64, Ny of SLT; XCD bands of tile rows where gridDim.y is a multiple of 8.
// ---------------------------------------------------------------------------------------------------------------------
#define SLT 8      // tile rows
template <bool GRHO, bool WY = false>
__global__ __launch_bounds__(64 * SLT, 2) void k_scalar_rho3d_lds(DevGrid g, double *__restrict__ Gc, double *__restrict__ Grho,
                                                                const double *__restrict__ rho, const double *__restrict__ u,
                                                                const double *__restrict__ v, const double *__restrict__ w,
                                                                const double *__restrict__ c, const double *__restrict__ ru,
                                                                const double *__restrict__ rv, const double *__restrict__ rw,
                                                                const int *__restrict__ zero_if_dry, int kchunk)
{
    constexpr int TY = SLT, TR = TY + 6, TC = 72, RR = TY + 2, RC = 68, NT = 64 * TY;
    constexpr int NHC = TR * 70 - TY * 64;      // frame cells of the c tile (468 for TY = 8)
    constexpr int NHR = RR * 65 - TY * 64;      // frame cells of the rho tile: row -1, row TY (cols -1 .. 63), column -1 of rows 0 .. TY-1 (138)
    static_assert(NHC <= NT && NHR <= NT, "one frame cell of each tile per thread");
    __shared__ double C[2][TR][TC];             // c:   tile row r (-3 .. TY+2) at [r + 3], column q (-3 .. 66) at [q + 3]
    __shared__ double R[2][RR][RC];             // rho: tile row r (-1 .. TY)   at [r + 1], column q (-1 .. 63) at [q + 1]
    __shared__ double FY[2][TY + 1][64];
    const int tx = threadIdx.x, ty = threadIdx.y, t = ty * 64 + tx, tc = tx + 3;
    int bxr = blockIdx.x, byr = blockIdx.y;
    if ((gridDim.y & 7u) == 0) {
        const unsigned wv = blockIdx.y * gridDim.x + blockIdx.x, cx = wv & 7u, rr = wv >> 3;
        bxr = (int)(rr % gridDim.x);
        byr = (int)(cx * (gridDim.y >> 3) + rr / gridDim.x);
    }
    const int i0 = bxr * 64, j0 = byr * TY, i = i0 + tx, j = j0 + ty;
    const int k0 = blockIdx.z * kchunk, k1 = min(k0 + kchunk, g.Nz);      // kchunk <= 64: one edge flux per lane
    if (k0 >= k1) return;
    const long long sy = g.Sx, sz = g.Sxy;
    long long n = g.idx(i, j, k0);
    if (zero_if_dry && __builtin_amdgcn_readfirstlane(*zero_if_dry) == 1) {
        for (int k = k0; k < k1; ++k, n += sz) Gc[n] = 0.0;
        return;
    }
    // frame cell of the c tile
    const bool hc = t < NHC;
    int hcr = 0, hcc = 0;
    {
        const int h = hc ? t : 0;
        if (h < 6 * 70) { const int rr = h / 70; hcc = h - rr * 70; hcr = (rr < 3) ? rr : TY + rr; }      // rows -3 .. -1 and TY .. TY+2, whole width
        else { const int hh = h - 6 * 70, rr = hh / 6, cc = hh - rr * 6; hcr = 3 + rr; hcc = (cc < 3) ? cc : 64 + cc; }      // side columns of the interior rows
    }
    const long long hcn = g.idx(i0 - 3 + hcc, j0 - 3 + hcr, k0);
    // frame cell of the rho tile
    const bool hr = t < NHR;
    int hrr = 0, hrc = 0;
    {
        const int h = hr ? t : 0;
        if (h < 2 * 65) { const int rr = h / 65; hrc = h - rr * 65; hrr = rr ? TY + 1 : 0; }      // rows -1 and TY
        else { hrr = 1 + (h - 2 * 65); hrc = 0; }                                                  // column -1 of rows 0 .. TY-1
    }
    const long long hrn = g.idx(i0 - 1 + hrc, j0 - 1 + hrr, k0);
    // x flux beyond the tile (column i0 + 64), one level per lane, straight from memory
    auto FXg = [&](long long m, int k) {
        const double u0 = u[m];
        return ((rho[m] + rho[m - 1]) / 2.0) * ((g.Ax[k] * u0) * bz_up5(c[m - 3], c[m - 2], c[m - 1], c[m], c[m + 1], c[m + 2], u0 > 0.0));
    };
    double edge;
    {
        const int kk = min(k0 + tx, k1 - 1);
        edge = FXg(g.idx(i0 + 64, j, kk), kk);
    }
    // z ring of the own column, densities of the levels k-1, k, k+1, lower z flux
    double zm3 = c[n - 3 * sz], zm2 = c[n - 2 * sz], zm1 = c[n - sz], z0 = c[n], zp1 = c[n + sz], zp2 = c[n + 2 * sz];
    double r0 = rho[n], r_hi = rho[n + sz];
    double Fz_lo;
    {
        const double wt = w[n], r_lo = rho[n - sz];
        const double cR = bz_upB(zm3, zm2, zm1, z0, zp1, zp2, wt > 0.0, bz_buffer_face(k0, g.Nz));
        Fz_lo = ((r0 + r_lo) / 2.0) * ((g.Az * wt) * cR);
    }
    double u0 = u[n], v0 = v[n], wt = w[n + sz];
    double grw_lo = GRHO ? rw[n] : 0.0;
    const long long nvt = g.idx(i, j0 + TY, k0);      // v of the row outside the tile (wave 0)
    const int Byj = by_face_c<WY>(g, j), Byt = by_face_c<WY>(g, j0 + TY);      // walls in y: the buffers of the own low face and of the face above the tile
    double vT = (ty == 0) ? v[nvt] : 0.0;
    // tiles of level k0
    C[0][ty + 3][tc] = z0;
    R[0][ty + 1][tx + 1] = r0;
    if (hc) C[0][hcr][hcc] = c[hcn];
    if (hr) R[0][hrr][hrc] = rho[hrn];
    __syncthreads();
    int buf = 0;
    for (int k = k0; k < k1; ++k, n += sz) {
        const long long lev1 = (long long)(k + 1 - k0) * sz;
        // ---- prefetch for level k + 1 (consumed at the end of this iteration) ----
        const double p_zp3 = c[n + 3 * sz];
        const double p_rn = rho[n + 2 * sz];
        const double p_w = w[n + 2 * sz];
        const double p_u = u[n + sz], p_v = v[n + sz];
        const double p_hc = hc ? c[hcn + lev1] : 0.0;
        const double p_hr = hr ? rho[hrn + lev1] : 0.0;
        const double p_vT = (ty == 0) ? v[nvt + lev1] : 0.0;
        const double Ax = g.Ax[k], Ay = g.Ay[k];
        if (GRHO) {      // G_rho = -div(rho u) of the cell: the x neighbour from the next lane, the lower z face carried from the level below
            const double gru0 = ru[n], grv0 = rv[n], grv1 = rv[n + sy], grw1 = rw[n + sz];
            double gru1 = bz_lane_down(gru0);
            if (tx == 63) gru1 = ru[n + 1];
            const double a = Ax * gru1 - Ax * gru0;
            const double b = Ay * grv1 - Ay * grv0;
            const double cc = g.Az * grw1 - g.Az * grw_lo;
            Grho[n] = -(g.Vinv_c[k] * (a + b + cc));
            grw_lo = grw1;
        }
        const double(*Ck)[TC] = C[buf];
        const double(*Rk)[RC] = R[buf];
        // ---- z: upper face ----
        const double cR = bz_upB(zm2, zm1, z0, zp1, zp2, p_zp3, wt > 0.0, bz_buffer_face(k + 1, g.Nz));
        const double Fz_hi = ((r_hi + r0) / 2.0) * ((g.Az * wt) * cR);
        const double dz = bz_sub_rounded_c(Fz_hi, Fz_lo);
        // ---- x: low face of the own cell ----
        const double *cr = Ck[ty + 3] + tc;
        const double fx = ((r0 + Rk[ty + 1][tx]) / 2.0) * ((Ax * u0) * bz_up5(cr[-3], cr[-2], cr[-1], z0, cr[1], cr[2], u0 > 0.0));
        // ---- y: low face of the own cell; wave 0 also takes the row outside the tile ----
        const double fy = ((r0 + Rk[ty][tx + 1]) / 2.0) * ((Ay * v0) * bz_up5y_c<WY>(Ck[ty][tc], Ck[ty + 1][tc], Ck[ty + 2][tc], z0, Ck[ty + 4][tc], Ck[ty + 5][tc], v0 > 0.0, Byj));
        FY[buf][ty][tx] = fy;
        if (ty == 0)
            FY[buf][TY][tx] = ((Rk[TY + 1][tx + 1] + Rk[TY][tx + 1]) / 2.0) *
                              ((Ay * vT) * bz_up5y_c<WY>(Ck[TY][tc], Ck[TY + 1][tc], Ck[TY + 2][tc], Ck[TY + 3][tc], Ck[TY + 4][tc], Ck[TY + 5][tc], vT > 0.0, Byt));
        // ---- stage level k + 1 ----
        C[buf ^ 1][ty + 3][tc] = zp1;
        R[buf ^ 1][ty + 1][tx + 1] = r_hi;
        if (hc) C[buf ^ 1][hcr][hcc] = p_hc;
        if (hr) R[buf ^ 1][hrr][hrc] = p_hr;
        // neighbour lane's flux by a DPP move, the out-of-wave one by v_readlane (bz_internal.h; k - k0 is wave-uniform), ahead of the barrier;
        // whole rows only, so lane 63, which the shift leaves at 0, is always replaced
        double nb = bz_lane_down(fx);
        const double e = bz_lane_read(edge, k - k0);
        if (tx == 63) nb = e;
        __syncthreads();
        {
            const double dx = bz_sub_rounded_c(nb, fx);
            const double dy = bz_sub_rounded_c(FY[buf][ty + 1][tx], fy);
            Gc[n] = -(g.Vinv_c[k] * (dx + dy + dz));
        }
        zm3 = zm2; zm2 = zm1; zm1 = z0; z0 = zp1; zp1 = zp2; zp2 = p_zp3;
        Fz_lo = Fz_hi;
        r0 = r_hi; r_hi = p_rn;
        u0 = p_u; v0 = p_v; wt = p_w; vT = p_vT;
        buf ^= 1;
    }
}

static int pick_kchunk_c(const DevGrid &g, int nlev)
{
    long long tiles = (long long)((g.Nx + 63) / 64) * ((g.Ny + CTY - 1) / CTY);
    long long want = (4096 + tiles - 1) / tiles;
    if (want < 1) want = 1;
    long long maxchunks = nlev / 8 > 0 ? nlev / 8 : 1;
    if (want > maxchunks) want = maxchunks;
    return (int)((nlev + want - 1) / want);
}

static int launch_scalar_rho3d(bz_ctx *ctx, const char *name, double *Gc, double *Grho, const double *rho, const double *u,
                               const double *v, const double *w, const double *c, const double *ru, const double *rv,
                               const double *rw, const int *zero_if_dry = nullptr)
{
    const DevGrid &g = ctx->dg;
    ProfileScope ps(ctx, name);
    if (ctx->weno_R != 3) return bzi_scalar_rho3d_generic(ctx, Gc, Grho, rho, u, v, w, c, ru, rv, rw);
    // walls in y: the WY instantiations of the tiled and of the ragged kernel (the exchange kernel between them is periodic only)
    if (!ctx->tune.no_rho3d_exchange && ctx->tune.scalar_lds && !g.flat_y && !g.bounded_x && g.Nx % 64 == 0 && g.Ny % SLT == 0 && g.Hx >= 3 &&
        g.Hy >= 3 && g.Hz >= 3) {
        int kc = 64;
        while (kc > 8 && (long long)(g.Nx / 64) * (g.Ny / SLT) * ((g.Nz + kc - 1) / kc) < 2048) kc >>= 1;
        dim3 block(64, SLT), grid(g.Nx / 64, g.Ny / SLT, (g.Nz + kc - 1) / kc);
        bz_bools([&](auto grho, auto wy) {
            hipLaunchKernelGGL((k_scalar_rho3d_lds<grho(), wy()>), grid, block, 0, ctx->stream, g, Gc, Grho, rho, u, v, w, c, ru, rv, rw, zero_if_dry, kc);
        }, Grho != nullptr, g.bounded_y != 0);
        BZ_LAUNCH_CHECK();
        return BZ_OK;
    }
    if (!ctx->tune.no_rho3d_exchange && !g.flat_y && !g.bounded_x && !g.bounded_y && g.Nx % 64 == 0 && g.Ny % CTY == 0) {
        int kc = 64;      // levels per workgroup: >= 8 wavefronts per SIMD (see march_chunk in bz_tendency_generic.hip)
        while (kc > 8 && (long long)(g.Nx / 64) * g.Ny * ((g.Nz + kc - 1) / kc) < 8192) kc >>= 1;
        dim3 block(64, CTY), grid(g.Nx / 64, g.Ny / CTY, (g.Nz + kc - 1) / kc);
        hipLaunchKernelGGL(k_scalar_tendency_rho3d_x, grid, block, 0, ctx->stream, g, Gc, Grho, rho, u, v, w, c, ru, rv, rw, zero_if_dry, kc);
        BZ_LAUNCH_CHECK();
        return BZ_OK;
    }
    const int kc = pick_kchunk_c(g, g.Nz);
    dim3 block(64, CTY), grid((g.Nx + 63) / 64, (g.Ny + CTY - 1) / CTY, (g.Nz + kc - 1) / kc);
    if (g.bounded_y) hipLaunchKernelGGL(k_scalar_tendency_rho3d<true>, grid, block, 0, ctx->stream, g, Gc, Grho, rho, u, v, w, c, ru, rv, rw, kc, zero_if_dry);
    else hipLaunchKernelGGL(k_scalar_tendency_rho3d<false>, grid, block, 0, ctx->stream, g, Gc, Grho, rho, u, v, w, c, ru, rv, rw, kc, zero_if_dry);
    BZ_LAUNCH_CHECK();
    return BZ_OK;
}

extern "C" int bz_compute_slow_tendencies(bz_ctx *ctx, const bz_compressible_state *s, const bz_compressible_prognostic *G)
{
    BZ_REQUIRE_COMPRESSIBLE();
    BZ_REJECT_WALLS("bz_compute_slow_tendencies");
    BZ_REJECT_Y_WALL_OPTIONS("bz_compute_slow_tendencies");
    if (!valid_state(s) || !valid_prog(G)) return BZ_ERR_INVALID;
    bz_state a;
    std::memset(&a, 0, sizeof(a));
    a.rho_u = s->rho_u; a.rho_v = s->rho_v; a.rho_w = s->rho_w;
    a.u = s->u; a.v = s->v; a.w = s->w; a.T = s->p; a.q = s->rho;
    a.rho_theta = s->rho_theta; a.rho_q = s->rho_q; a.theta = s->theta;
    bz_prognostic Ga;
    Ga.rho_u = G->rho_u; Ga.rho_v = G->rho_v; Ga.rho_w = G->rho_w; Ga.rho_theta = G->rho_theta; Ga.rho_q = G->rho_q;
    int rc;
    if (ctx->weno_R != 3) {      // WENO(order = 7 / 9): generic kernels (bz_tendency_generic.hip)
        if ((rc = bzi_momentum_advection_generic(ctx, &a, &Ga))) return rc;
    } else if (ctx->dg.flat_y || ctx->dg.bounded_y) {
        // walls in y: the per-operator kernels carry the row-wise buffers (bz_tendency.hip: by_face, by_center, symm_y); the wall row j = 0 of
        // G_rho_v is not written (the acoustic loop holds that face at zero)
        if ((rc = bzi_momentum_advection_gen1(ctx, &a, &Ga))) return rc;
    } else {
        rc = bzi_u_tendency_lds(ctx, &a, &Ga);
        if (rc) return rc;
        rc = bzi_v_tendency_lds(ctx, &a, &Ga);
        if (rc) return rc;
        rc = bzi_w_tendency_lds(ctx, &a, &Ga, nullptr, nullptr, 1);
        if (rc) return rc;
    }
    if ((rc = launch_scalar_rho3d(ctx, "density+potential_temperature_tendency", G->rho_theta, G->rho_d, s->rho_d, s->u, s->v,
                                  s->w, s->theta, s->rho_u, s->rho_v, s->rho_w))) return rc;
    // - f x (rho U) of an FPlane and the density-keyed sponges are slow terms too (dynamics_kernel_functions.jl:79,99 through the same
    // x / y_momentum_tendency; examples/tropical_cyclone_with_rainband.jl:434-514)
    if (ctx->has_forcings && (rc = bzi_apply_forcings(ctx, &a, G->rho_u, G->rho_v, G->rho_theta, G->rho_q, 1.0))) return rc;
    // - d_j T_ij and - div J^theta of the closure, rho_d at the flux locations, between the Coriolis term and the forcings as in
    // x / y / z_momentum_tendency (dynamics_kernel_functions.jl:77-81; acoustic_substep_helpers.jl:55-93)
    if ((ctx->has_closure || ctx->has_diffusivity) && (rc = bzi_cmp_closure_slow(ctx, s, G))) return rc;
    return bzi_apply_relaxation(ctx, &a, &Ga, s->rho_d);
}

extern "C" int bz_compute_moisture_tendency(bz_ctx *ctx, const bz_compressible_state *s, const bz_compressible_prognostic *G,
                                            const bz_acoustic_substepper *sub)
{
    BZ_REQUIRE_COMPRESSIBLE();
    BZ_REJECT_WALLS("bz_compute_moisture_tendency");
    BZ_REJECT_Y_WALL_OPTIONS("bz_compute_moisture_tendency");
    if (!valid_state(s) || !valid_prog(G) || !valid_sub(sub)) return BZ_ERR_INVALID;
    // (WENO order 5 kernels; the generic order 7 / 9 path evaluates the field whatever it holds)
    const int *dry = ctx->weno_R == 3 ? bzi_moisture_state(ctx) : nullptr;
    int rc = launch_scalar_rho3d(ctx, "moisture_tendency", G->rho_q, nullptr, s->rho, sub->time_averaged_u, sub->time_averaged_v,
                                 sub->time_averaged_w, s->q, nullptr, nullptr, nullptr, dry);
    if (rc) return rc;
    if (ctx->dg.microphysics == 2) {
        const bz_kessler_model_fields &K = ctx->kessler;      // the Kessler species ride the same transport velocities
        rc = launch_scalar_rho3d(ctx, "kessler_species_tendencies", K.G_cloud_liquid_density, nullptr, s->rho, sub->time_averaged_u,
                                 sub->time_averaged_v, sub->time_averaged_w, K.cloud_liquid_mass_fraction, nullptr, nullptr, nullptr);
        if (rc) return rc;
        rc = launch_scalar_rho3d(ctx, "kessler_species_tendencies", K.G_rain_density, nullptr, s->rho, sub->time_averaged_u,
                                 sub->time_averaged_v, sub->time_averaged_w, K.rain_mass_fraction, nullptr, nullptr, nullptr);
        if (rc) return rc;
    }
    // - div J^c of the closure for every water scalar, the TOTAL density at the faces (scalar_tendency, dynamics_kernel_functions.jl:152-157)
    return bzi_cmp_water_closure(ctx, s, G, dry);
}
