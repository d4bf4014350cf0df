// bz_diffusivity.hip — closure = ScalarDiffusivity(...) / VerticalScalarDiffusivity(...) on the anelastic model, explicit or with
// VerticallyImplicitTimeDiscretization, nu and kappa each a number or a centre field.
//   Breeze side (followed line by line):
//     dynamic stresses / scalar fluxes = rho_r at the flux location x Oceananigans' kinematic flux, the closure's time discretisation
//     passed into every flux                /root/reference/src/TurbulenceClosures/TurbulenceClosures.jl:48-101
//     implicit_step!(field, solver, closure, ..., alpha dt) after the RK update of every prognostic field
//                                           /root/reference/src/TimeSteppers/ssp_runge_kutta_3.jl:124-161
//     order inside a stage                  /root/reference/src/TimeSteppers/ssp_runge_kutta_3.jl:229-236
//     z-Face rows of a vertical implicit solve   /root/reference/src/AtmosphereModels/implicit_vertical_advection.jl:202-214,270-292
//     the reference's own tests             /root/reference/test/turbulence_closures.jl:14-50, /root/reference/test/vertical_diffusion.jl
//   Oceananigans side (0.110.14, not vendored) — PARITY UNPINNED, the reading that include/breeze_hip.h states in full:
//     isotropic: stresses -2 nu Sigma_ij with nu averaged to ccc / ffc / fcf / cff, scalar fluxes -kappa grad c with kappa averaged
//     to the face (the SmagorinskyLilly path of bz_closure.hip with the given nu and an independent kappa);  vertical: only
//     tau_uz = -nu_fcf dz u, tau_vz = -nu_cff dz v, tau_wz = -nu_ccc dz w, J_z = -kappa_ccf dz c;  vertically implicit: the explicit
//     tendency keeps tau_uz = -nu_fcf dx w, tau_vz = -nu_cff dy w (isotropic) and drops tau_wz, J_z; the solve is
//     (I - dtau dz K dz) phi = phi* on the density-weighted prognostic field itself, no density in the operator.  The fluxes on the
//     boundary faces k = 1 and Nz + 1 stay explicit in Oceananigans; they vanish under the default no-flux / impenetrable
//     conditions, the only ones these closures run with here, so there is no code for them.
// Kernels: the explicit divergences one thread per cell (momentum; one launch per scalar), and the implicit step of a stage as ONE
// launch over every prognostic field of the context: a lane owns a column, lanes run along x (every level's access is coalesced), the
// Thomas sweep marches up and back.  Constant K: the elimination factors depend on the level only and come from a table a one-block
// prologue forms per (dtau, field class) — no division per cell.  Field K: factors on the fly, the modified upper diagonal through a
// scratch array per field (c' in LDS, 64 columns x Nz words per wave, leaves two waves on a CU at Nz = 128 and one at 256 and measured
// 6.5 x the table form).  A lane touches its own column only, so the kernel has no barrier.  The modified right-hand side
// goes through the field in place in both forms ("ScalarDiffusivity": words per cell and field).
#include "bz_closure_carriers.h"
#include "bz_compressible_internal.h"

// K at a cell: the centre field (halos: periodic x / y, zero gradient in z — bzi_diffusivity_halos) or the number
struct KSource {
    const double *f;
    double c;
    __device__ __forceinline__ double at(long long n) const { return f ? f[n] : c; }
};
// kappa = nu_e / Pr of SmagorinskyLilly at a cell (nu_e with its halos filled), for the water scalars of the compressible model
struct KScaled {
    const double *f;
    double mul;
    __device__ __forceinline__ double at(long long n) const { return f[n] * mul; }
};

// same block order as bz_closure.hip: every XCD gets a contiguous slab of (row, level / field) space
__device__ __forceinline__ void dif_xcd_block(int &bx, int &by, int &bz)
{
    const int nb = gridDim.x * gridDim.y * gridDim.z;
    int b = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);
    if (nb % 8 == 0) b = (b % 8) * (nb / 8) + b / 8;
    bx = b % gridDim.x;
    by = (b / gridDim.x) % gridDim.y;
    bz = b / (gridDim.x * gridDim.y);
}

// ---- explicit tendencies ------------------------------------------------------------------------------------------------------------
// VERT: the vertical formulation (every x and y flux is zero).  IMPL: the remainder a vertically implicit discretisation leaves explicit.
// Same expressions and order of operations as k_closure_tendencies (bz_closure.hip) where the two overlap; u, v, w carry periodic halos
// in x / y, nu its own (bzi_diffusivity_halos).
// RHO: the density of the flux locations (bz_closure_carriers.h): the reference column, or rho_d of the compressible model.
template <bool VERT, bool IMPL, class RHO>
__global__ __launch_bounds__(256) void k_diffusivity_momentum(DevGrid g, KSource NUs, RHO R, const double *__restrict__ u, const double *__restrict__ v,
                                                              const double *__restrict__ w, double *__restrict__ Gu, double *__restrict__ Gv,
                                                              double *__restrict__ Gw, double scale)
{
    int bx, by, bz;
    dif_xcd_block(bx, by, bz);
    const int i = bx * 256 + threadIdx.x, j = by, k = bz;
    if (i >= g.Nx) return;
    const long long n = g.idx(i, j, k), sx = 1, sy = g.flat_y ? 0 : g.Sx, sz = g.Sxy;      // Flat y: the neighbour rows coincide with the row
    const double dx = g.dx, dy = g.dy, dz = g.dzc[k];
    const double rVc = g.rdx * (1.0 / dy) * g.rdzc[k];
    const double Ax = dy * dz, Ay = dx * dz, Az = dx * dy;
    auto NU = [&](int di, int dj, int dk) { return NUs.at(n + di * sx + dj * sy + dk * sz); };
    auto nu_ffc = [&](int di, int dj) { return ((NU(di - 1, dj - 1, 0) + NU(di, dj - 1, 0)) / 2 + (NU(di - 1, dj, 0) + NU(di, dj, 0)) / 2) / 2; };
    auto nu_fcf = [&](int di, int dk) { return ((NU(di - 1, 0, dk - 1) + NU(di, 0, dk - 1)) / 2 + (NU(di - 1, 0, dk) + NU(di, 0, dk)) / 2) / 2; };
    auto nu_cff = [&](int dj, int dk) { return ((NU(0, dj - 1, dk - 1) + NU(0, dj, dk - 1)) / 2 + (NU(0, dj - 1, dk) + NU(0, dj, dk)) / 2) / 2; };
    auto wall = [&](int dk) { return k + dk <= 0 || k + dk >= g.Nz; };
    // the four derivatives of the off-diagonal vertical strains at (x face i + di | y face j + dj, z face k + dk); zero on the walls
    auto dzu = [&](int di, int dk) { const long long m = n + di * sx + dk * sz; return wall(dk) ? 0.0 : (u[m] - u[m - sz]) * g.rdzf[k + dk]; };
    auto dxw = [&](int di, int dk) { const long long m = n + di * sx + dk * sz; return wall(dk) ? 0.0 : (w[m] - w[m - 1]) * g.rdx; };
    auto dzv = [&](int dj, int dk) { const long long m = n + dj * sy + dk * sz; return wall(dk) ? 0.0 : (v[m] - v[m - sz]) * g.rdzf[k + dk]; };
    auto dyw = [&](int dj, int dk) { const long long m = n + dj * sy + dk * sz; return wall(dk) ? 0.0 : (w[m] - w[m - sy]) * g.rdy; };
    auto s11 = [&](int di) { const long long m = n + di * sx; return (u[m + 1] - u[m]) * g.rdx; };
    auto s22 = [&](int dj) { const long long m = n + dj * sy; return (v[m + sy] - v[m]) * g.rdy; };
    auto s33 = [&](int dk) { const long long m = n + dk * sz; return (w[m + sz] - w[m]) * g.rdzc[k + dk]; };
    auto s12 = [&](int di, int dj) { const long long m = n + di * sx + dj * sy; return ((u[m] - u[m - sy]) * g.rdy + (v[m] - v[m - 1]) * g.rdx) * 0.5; };
    // horizontal fluxes (isotropic formulation only; the time discretisation does not touch them)
    auto rfcf = [&](int di, int dk) { return R.fcf(g, n + di * sx + dk * sz, k + dk); };      // density at (x face i + di, z face k + dk)
    auto rcff = [&](int dj, int dk) { return R.cff(g, n + dj * sy + dk * sz, k + dk); };
    auto rccc = [&](int dk) { return R.ccc(g, n + dk * sz, k + dk); };
    auto T11 = [&](int di) { return R.ccc(g, n + di * sx, k) * (-2 * NU(di, 0, 0) * s11(di)); };
    auto T22 = [&](int dj) { return R.ccc(g, n + dj * sy, k) * (-2 * NU(0, dj, 0) * s22(dj)); };
    auto T12 = [&](int di, int dj) { return R.ffc(g, n + di * sx + dj * sy, k) * (-2 * nu_ffc(di, dj) * s12(di, dj)); };
    auto Twx = [&](int di) { return rfcf(di, 0) * (-2 * nu_fcf(di, 0) * ((dzu(di, 0) + dxw(di, 0)) * 0.5)); };      // x flux of z momentum at (x face i + di, z face k)
    auto Twy = [&](int dj) { return rcff(dj, 0) * (-2 * nu_cff(dj, 0) * ((dzv(dj, 0) + dyw(dj, 0)) * 0.5)); };
    // vertical fluxes: what the discretisation leaves explicit
    auto Tuz = [&](int dk) {
        if (VERT) return IMPL ? 0.0 : rfcf(0, dk) * (-nu_fcf(0, dk) * dzu(0, dk));
        return IMPL ? rfcf(0, dk) * (-nu_fcf(0, dk) * dxw(0, dk)) : rfcf(0, dk) * (-2 * nu_fcf(0, dk) * ((dzu(0, dk) + dxw(0, dk)) * 0.5));
    };
    auto Tvz = [&](int dk) {
        if (VERT) return IMPL ? 0.0 : rcff(0, dk) * (-nu_cff(0, dk) * dzv(0, dk));
        return IMPL ? rcff(0, dk) * (-nu_cff(0, dk) * dyw(0, dk)) : rcff(0, dk) * (-2 * nu_cff(0, dk) * ((dzv(0, dk) + dyw(0, dk)) * 0.5));
    };
    auto Twz = [&](int dk) {
        if (IMPL) return 0.0;
        return VERT ? rccc(dk) * (-NU(0, 0, dk) * s33(dk)) : rccc(dk) * (-2 * NU(0, 0, dk) * s33(dk));
    };
    {
        double div = Az * Tuz(1) - Az * Tuz(0);
        if (!VERT) div = (Ax * T11(0) - Ax * T11(-1)) + (g.flat_y ? 0.0 : Ay * T12(0, 1) - Ay * T12(0, 0)) + div;
        Gu[n] -= scale * (div * rVc);
    }
    {
        double div = Az * Tvz(1) - Az * Tvz(0);
        if (!VERT) div = (Ax * T12(1, 0) - Ax * T12(0, 0)) + (g.flat_y ? 0.0 : Ay * T22(0) - Ay * T22(-1)) + div;
        Gv[n] -= scale * (div * rVc);
    }
    if (k >= 1) {   // z momentum at the interior face k (between centres k-1 and k)
        const double dzf = g.dzf[k];
        const double Axf = dy * dzf, Ayf = dx * dzf;
        double div = Az * Twz(0) - Az * Twz(-1);
        if (!VERT) div = (Axf * Twx(1) - Axf * Twx(0)) + (g.flat_y ? 0.0 : Ayf * Twy(1) - Ayf * Twy(0)) + div;
        Gw[n] -= scale * (div * (g.rdx * (1.0 / dy) * g.rdzf[k]));
    }
}

// - div J^c of NS scalars that share their diffusivity and their density: J = rho x (-kappa grad c) with kappa and rho averaged to the
// face.  The face coefficients are formed once per cell.  div[q] is the flux divergence times 1 / V of scalar q.
template <bool VERT, bool IMPL, int NS, class RHO, class KS>
__device__ __forceinline__ void dif_scalar_divergences(const DevGrid &g, const KS &Ks, const RHO &R, long long n, int k, const double *const (&c)[NS],
                                                       double (&out)[NS])
{
    const long long sy = g.flat_y ? 0 : g.Sx, sz = g.Sxy;
    const double dx = g.dx, dy = g.dy, dz = g.dzc[k];
    const double rVc = g.rdx * (1.0 / dy) * g.rdzc[k];
    const double Ax = dy * dz, Ay = dx * dz, Az = dx * dy;
    const double kc = Ks.at(n);
    double kzm = 0.0, kzp = 0.0, rzm = 0.0, rzp = 0.0, kxm = 0.0, kxp = 0.0, kym = 0.0, kyp = 0.0, rxm = 0.0, rxp = 0.0, rym = 0.0, ryp = 0.0;
    if (!IMPL) {
        kzm = (Ks.at(n - sz) + kc) / 2; kzp = (kc + Ks.at(n + sz)) / 2;
        rzm = R.ccf(g, n, k); rzp = R.ccf(g, n + sz, k + 1);
    }
    if (!VERT) {
        kxm = (Ks.at(n - 1) + kc) / 2; kxp = (kc + Ks.at(n + 1)) / 2;
        kym = (Ks.at(n - sy) + kc) / 2; kyp = (kc + Ks.at(n + sy)) / 2;
        rxm = R.fcc(g, n, k); rxp = R.fcc(g, n + 1, k); rym = R.cfc(g, n, k); ryp = R.cfc(g, n + sy, k);
    }
#pragma unroll
    for (int q = 0; q < NS; ++q) {
        const double *__restrict__ cq = c[q];
        const double c0 = cq[n];
        double div = 0.0;
        if (!IMPL) {
            const double Jzm = (k == 0) ? 0.0 : rzm * (-kzm * ((c0 - cq[n - sz]) * g.rdzf[k]));
            const double Jzp = (k == g.Nz - 1) ? 0.0 : rzp * (-kzp * ((cq[n + sz] - c0) * g.rdzf[k + 1]));
            div = Az * Jzp - Az * Jzm;
        }
        if (!VERT) {
            const double Jxm = rxm * (-kxm * ((c0 - cq[n - 1]) * g.rdx)), Jxp = rxp * (-kxp * ((cq[n + 1] - c0) * g.rdx));
            const double Jym = rym * (-kym * ((c0 - cq[n - sy]) * g.rdy)), Jyp = ryp * (-kyp * ((cq[n + sy] - c0) * g.rdy));
            div = (Ax * Jxp - Ax * Jxm) + (Ay * Jyp - Ay * Jym) + div;
        }
        out[q] = div * rVc;
    }
}

template <bool VERT, bool IMPL, class RHO>
__global__ __launch_bounds__(256) void k_diffusivity_scalar(DevGrid g, KSource Ks, RHO R, const double *__restrict__ c, double *__restrict__ G, double scale)
{
    int bx, by, bz;
    dif_xcd_block(bx, by, bz);
    const int i = bx * 256 + threadIdx.x, j = by, k = bz;
    if (i >= g.Nx) return;
    const long long n = g.idx(i, j, k);
    const double *const cs[1] = {c};
    double div[1];
    dif_scalar_divergences<VERT, IMPL, 1>(g, Ks, R, n, k, cs, div);
    G[n] -= scale * div[0];
}

// The water scalars of the compressible model in one launch: rho q and, with Kessler, rho q^cl and rho q^r diffuse with one kappa
// (kappa of the closure, or nu_e / Pr) and the TOTAL density at the faces, both read once per cell.
// A dry model (the moisture scan's word, bz_moisture.hip) returns before reading: its moisture tendency is the exact zero the advection wrote.
struct WaterList { const double *c[3]; double *G[3]; };
template <bool VERT, int NS, class KS>
__global__ __launch_bounds__(256) void k_water_closure(DevGrid g, KS Ks, RhoField R, WaterList L, const int *__restrict__ skip_if_dry)
{
    int bx, by, bz;
    dif_xcd_block(bx, by, bz);
    const int i = bx * 256 + threadIdx.x, j = by, k = bz;
    if (i >= g.Nx) return;
    if (skip_if_dry && __builtin_amdgcn_readfirstlane(*skip_if_dry) == 1) return;
    const long long n = g.idx(i, j, k);
    const double *cs[NS];
    double div[NS];
#pragma unroll
    for (int q = 0; q < NS; ++q) cs[q] = L.c[q];
    dif_scalar_divergences<VERT, false, NS>(g, Ks, R, n, k, cs, div);
#pragma unroll
    for (int q = 0; q < NS; ++q) L.G[q][n] -= div[q];
}

// ---- implicit step ------------------------------------------------------------------------------------------------------------------
// field classes: where the field sits decides which average of K its rows take
#define DIF_CLASS_U 0        // centre rows, K = nu_fcf
#define DIF_CLASS_V 1        // centre rows, K = nu_cff
#define DIF_CLASS_W 2        // face rows 2 .. Nz (1-based), K = nu_ccc
#define DIF_CLASS_C 3        // centre rows, K = kappa_ccf
#define DIF_MAX_FIELDS (7 + BZ_MAX_TRACERS)
struct ImplicitList {
    double *f[DIF_MAX_FIELDS];
    int cls[DIF_MAX_FIELDS];
};

// Rows (0-based r; level kk = r for centre rows, r + 1 for the face rows of rho w; nr = Nz or Nz - 1):
//   centre  lower = -dtau Kf[kk] / (dzc[kk] dzf[kk]) (0 at kk = 0), upper = -dtau Kf[kk+1] / (dzc[kk] dzf[kk+1]) (0 at kk = Nz - 1)
//   face    lower = -dtau nu[kk-1] / (dzf[kk] dzc[kk-1]),           upper = -dtau nu[kk] / (dzf[kk] dzc[kk])
//   diag = (1 - upper) - lower; the first face row's lower and the last one's upper multiply the wall value w = 0: they stay in the
//   diagonal and leave the elimination.
// Thomas: m = 1 / (diag - lower c'[r-1]), c'[r] = upper m, d'[r] = (d[r] - lower d'[r-1]) m; back: x[r] = d'[r] - c'[r] x[r+1].
// table[(3 cls + {0: lower, 1: c', 2: m}) Nz + r]: constant K (one thread per class; Nz sequential divisions, once per launch)
// The recurrence runs in Float64 in both builds (double_t of <cmath>: the one spelling of the type the Float32 generator leaves alone), so
// the Float32 twin's table holds correctly rounded factors instead of Nz levels of accumulated Float32 rounding, at no cost: one thread
// per class, once per launch.
typedef double_t dif_wide_t;
__global__ void k_implicit_table(DevGrid g, double nu0, double kappa0, double dtau, double *__restrict__ table)
{
    const int cls = threadIdx.x;
    if (cls > 3) return;
    const bool face = cls == DIF_CLASS_W;
    const dif_wide_t K = (cls == DIF_CLASS_C) ? kappa0 : nu0, dt = dtau, one = 1.0;
    const int nr = face ? g.Nz - 1 : g.Nz;
    double *lo_t = table + (size_t)(3 * cls) * g.Nz, *cp_t = lo_t + g.Nz, *m_t = cp_t + g.Nz;
    dif_wide_t cp = 0.0;
    for (int r = 0; r < nr; ++r) {
        const int kk = r + (face ? 1 : 0);
        dif_wide_t lo, up;
        if (face) {
            lo = -dt * K / ((dif_wide_t)g.dzf[kk] * (dif_wide_t)g.dzc[kk - 1]);
            up = -dt * K / ((dif_wide_t)g.dzf[kk] * (dif_wide_t)g.dzc[kk]);
        } else {
            lo = (kk == 0) ? (dif_wide_t)0.0 : -dt * K / ((dif_wide_t)g.dzc[kk] * (dif_wide_t)g.dzf[kk]);
            up = (kk == g.Nz - 1) ? (dif_wide_t)0.0 : -dt * K / ((dif_wide_t)g.dzc[kk] * (dif_wide_t)g.dzf[kk + 1]);
        }
        const dif_wide_t diag = (one - up) - lo;
        const dif_wide_t lo_e = (r == 0) ? (dif_wide_t)0.0 : lo, up_e = (r == nr - 1) ? (dif_wide_t)0.0 : up;
        const dif_wide_t m = one / (diag - lo_e * cp);
        cp = up_e * m;
        lo_t[r] = (double)lo_e; cp_t[r] = (double)cp; m_t[r] = (double)m;
    }
}

// grid (ceil(Nx / 64), Ny, fields), block 64: one wave, one row, 64 columns; ragged Nx through the predicate.
// FIELDK: any of nu, kappa is a field — the factors are formed per column (a number among them is read as a number) and c' goes through a
// scratch array shaped like the field (one per field of the launch); else the table.
template <bool FIELDK>
__global__ __launch_bounds__(64) void k_implicit_step(DevGrid g, ImplicitList L, KSource NUs, KSource KAs, double dtau, const double *__restrict__ table,
                                                      double *__restrict__ scratch, long long scratch_stride)
{
    int bx, by, bz;
    dif_xcd_block(bx, by, bz);
    const int tx = threadIdx.x, i = bx * 64 + tx, j = by, fi = bz;
    if (i >= g.Nx) return;      // a lane reads and writes its own column of the field and of the scratch array only
    const int cls = L.cls[fi];
    const bool face = cls == DIF_CLASS_W;
    const int nr = face ? g.Nz - 1 : g.Nz;
    if (nr < 1) return;
    double *__restrict__ f = L.f[fi];
    const long long sz = g.Sxy, sy = g.flat_y ? 0 : g.Sx;
    const long long n0 = g.idx(i, j, face ? 1 : 0);      // row 0 of the column
    if (!FIELDK) {
        const double *lo_t = table + (size_t)(3 * cls) * g.Nz, *cp_t = lo_t + g.Nz, *m_t = cp_t + g.Nz;
        double dp = 0.0;
        long long n = n0;
        for (int r = 0; r < nr; ++r, n += sz) {
            dp = (f[n] - lo_t[r] * dp) * m_t[r];
            f[n] = dp;
        }
        double x = dp;
        n -= 2 * sz;
        for (int r = nr - 2; r >= 0; --r, n -= sz) {
            x = f[n] - cp_t[r] * x;
            f[n] = x;
        }
        return;
    }
    const KSource Ks = (cls == DIF_CLASS_C) ? KAs : NUs;
    double *__restrict__ cpg = scratch + (long long)fi * scratch_stride;      // c' of this field, at the field's own indices
    // K at the z face kk of the field's own column (centre rows), from the two levels around it
    const long long c0 = g.idx(i, j, 0);
    auto level_avg = [&](int kk) -> double {      // horizontal part of the average at level kk
        const long long m = c0 + (long long)kk * sz;
        if (cls == DIF_CLASS_U) return (Ks.at(m - 1) + Ks.at(m)) / 2;
        if (cls == DIF_CLASS_V) return (Ks.at(m - sy) + Ks.at(m)) / 2;
        return Ks.at(m);
    };
    double cp = 0.0, dp = 0.0;
    long long n = n0;
    if (face) {
        double nu_lo = Ks.at(c0);      // nu_ccc[kk - 1]
        for (int r = 0; r < nr; ++r, n += sz) {
            const int kk = r + 1;
            const double nu_hi = Ks.at(c0 + (long long)kk * sz);
            const double lo = -dtau * nu_lo / (g.dzf[kk] * g.dzc[kk - 1]), up = -dtau * nu_hi / (g.dzf[kk] * g.dzc[kk]);
            const double diag = (1.0 - up) - lo;
            const double lo_e = (r == 0) ? 0.0 : lo, up_e = (r == nr - 1) ? 0.0 : up;
            const double m = 1.0 / (diag - lo_e * cp);
            cp = up_e * m;
            dp = (f[n] - lo_e * dp) * m;
            cpg[n] = cp;
            f[n] = dp;
            nu_lo = nu_hi;
        }
    } else {
        double a_lo = level_avg(0), Kf_lo = 0.0;      // level kk's horizontal average; K at face kk (the wall face carries no flux)
        for (int r = 0; r < nr; ++r, n += sz) {
            const int kk = r;
            double a_hi = 0.0, Kf_hi = 0.0;
            if (kk < g.Nz - 1) { a_hi = level_avg(kk + 1); Kf_hi = (a_lo + a_hi) / 2; }
            const double lo = (kk == 0) ? 0.0 : -dtau * Kf_lo / (g.dzc[kk] * g.dzf[kk]);
            const double up = (kk == g.Nz - 1) ? 0.0 : -dtau * Kf_hi / (g.dzc[kk] * g.dzf[kk + 1]);
            const double diag = (1.0 - up) - lo;
            const double m = 1.0 / (diag - lo * cp);
            cp = up * m;
            dp = (f[n] - lo * dp) * m;
            cpg[n] = cp;
            f[n] = dp;
            a_lo = a_hi; Kf_lo = Kf_hi;
        }
    }
    double x = dp;
    n -= 2 * sz;
    for (int r = nr - 2; r >= 0; --r, n -= sz) {
        x = f[n] - cpg[n] * x;
        f[n] = x;
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
static int dif_field_count(const bz_ctx *ctx) { return 5 + (ctx->dg.microphysics == 2 ? 2 : 0) + ctx->n_tracers; }

// c' of the field-K solve: one parent-shaped array per field of the launch.  Grown here (attach time, and by the first solve after more
// fields were attached), never inside a recorded step.
static int dif_ensure_scratch(bz_ctx *ctx, int nf)
{
    const DevGrid &g = ctx->dg;
    const long long stride = g.Sxy * (long long)(g.Nz + 2 * g.Hz + 1);
    if (ctx->diff_scratch_fields >= nf) return BZ_OK;
    if (ctx->graph_capturing) { ctx->last_error = "bz_implicit_step: the scratch of the field-valued solve cannot grow inside a recorded step"; return BZ_ERR_UNSUPPORTED; }
    if (ctx->d_diff_scratch) { BZ_HIP(hipStreamSynchronize(ctx->stream)); BZ_HIP(hipFree(ctx->d_diff_scratch)); ctx->d_diff_scratch = nullptr; ctx->diff_scratch_fields = 0; }
    BZ_HIP(hipMalloc(&ctx->d_diff_scratch, (size_t)nf * (size_t)stride * sizeof(double)));
    ctx->diff_scratch_fields = nf;
    return BZ_OK;
}

extern "C" int bz_set_scalar_diffusivity(bz_ctx *ctx, const bz_scalar_diffusivity *c, double *nu_field, double *kappa_field)
{
    if (!ctx) return BZ_ERR_INVALID;
    ++ctx->config_epoch;      // captured steps (bz_graph.hip) belong to one configuration
    if (!c) { ctx->has_diffusivity = false; ctx->diff_nu = ctx->diff_kappa = nullptr; return BZ_OK; }
    const DevGrid &g = ctx->dg;
    const char *what = nullptr;
    if (ctx->has_closure) what = "a SmagorinskyLilly closure is attached (bz_set_closure): one closure per context";
    else if (ctx->compressible && c->time_discretization == 1)
        what = "VerticallyImplicitTimeDiscretization is not implemented on a compressible context (CompressibleDynamics): the explicit discretisation is";
    else if (ctx->compressible && g.flat_y) what = "not implemented on a compressible context with a Flat y";
    else if (ctx->kinematic) what = "not implemented on a kinematic context (PrescribedDynamics)";
    else if (ctx->slab_mode) what = "not implemented on a y-slab context";
    else if (g.bounded_x || g.bounded_y) what = "not implemented between walls in x or y (Bounded x / Bounded y)";
    else if (c->formulation < 0 || c->formulation > 1) what = "formulation: 0 (isotropic, ScalarDiffusivity) or 1 (VerticalScalarDiffusivity)";
    else if (c->time_discretization < 0 || c->time_discretization > 1) what = "time_discretization: 0 (explicit) or 1 (vertically implicit)";
    else if (g.Hx < 1 || (g.Hy < 1 && !g.flat_y) || g.Hz < 1) what = "needs halos >= 1";
    else if (!(c->nu >= 0.0) || !(c->kappa >= 0.0)) what = "nu and kappa must be finite and not negative";
    if (what) { ctx->last_error = std::string("bz_set_scalar_diffusivity: ") + what; return BZ_ERR_UNSUPPORTED; }
    if (c->time_discretization == 1) {
        if (!ctx->d_diff_table) BZ_HIP(hipMalloc(&ctx->d_diff_table, (size_t)12 * g.Nz * sizeof(double)));
        if (nu_field || kappa_field) { const int rcs = dif_ensure_scratch(ctx, dif_field_count(ctx)); if (rcs) return rcs; }
    }
    ctx->diffusivity = *c;
    ctx->diff_nu = nu_field;
    ctx->diff_kappa = kappa_field;
    ctx->has_diffusivity = true;
    return BZ_OK;
}

void bzi_diffusivity_teardown(bz_ctx *ctx)
{
    if (ctx->d_diff_table) hipFree(ctx->d_diff_table);
    if (ctx->d_diff_scratch) hipFree(ctx->d_diff_scratch);
    ctx->d_diff_table = ctx->d_diff_scratch = nullptr;
    ctx->diff_scratch_fields = 0;
}

// The user may have rewritten a field-valued K: periodic in x and y, zero gradient in z (as the eddy viscosity of bz_closure.hip is read)
int bzi_diffusivity_halos(bz_ctx *ctx)
{
    if (!ctx->has_diffusivity) return BZ_OK;
    double *f[2];
    int kinds[2] = {0, 0}, n = 0;
    if (ctx->diff_nu) f[n++] = ctx->diff_nu;
    if (ctx->diff_kappa && ctx->diff_kappa != ctx->diff_nu) f[n++] = ctx->diff_kappa;
    return bzi_fill_halos_multi(ctx, f, kinds, n);
}

static bool dif_momentum_on(const bz_ctx *ctx) { return ctx->diff_nu || ctx->diffusivity.nu != 0.0; }
static bool dif_scalars_on(const bz_ctx *ctx) { return ctx->diff_kappa || ctx->diffusivity.kappa != 0.0; }

// closure terms of compute_tendencies! (scale = 1, tendency arrays) or of a fused-RK stage (scale = alpha dt, the arrays its RK update
// just wrote) — the contract of bzi_apply_closure
int bzi_apply_diffusivity(bz_ctx *ctx, const bz_state *s, double *Gu, double *Gv, double *Gw, double *Gth, double *Gq, double scale)
{
    int rc;
    { const int rcs = bzi_refresh_diagnostics(ctx, s, "bz_compute_tendencies"); if (rcs) return rcs; }
    if ((rc = bzi_diffusivity_halos(ctx))) return rc;
    const DevGrid &g = ctx->dg;
    const bool vert = ctx->diffusivity.formulation == 1, impl = ctx->diffusivity.time_discretization == 1;
    if (vert && impl) return BZ_OK;      // the implicit solve covers every flux of the vertical formulation
    ProfileScope ps(ctx, "diffusivity_tendencies");
    const KSource NUs{ctx->diff_nu, ctx->diffusivity.nu}, KAs{ctx->diff_kappa, ctx->diffusivity.kappa};
    const dim3 grid((g.Nx + 255) / 256, g.Ny, g.Nz), block(256);
    if (dif_momentum_on(ctx)) {
#define DIF_MOM(V, I) hipLaunchKernelGGL((k_diffusivity_momentum<V, I, RhoColumn>), grid, block, 0, ctx->stream, g, NUs, RhoColumn(), (const double *)s->u, (const double *)s->v, (const double *)s->w, Gu, Gv, Gw, scale)
        if (vert) DIF_MOM(true, false);
        else if (impl) DIF_MOM(false, true);
        else DIF_MOM(false, false);
#undef DIF_MOM
    }
    if (dif_scalars_on(ctx)) {
        const bool in_place = Gth == s->rho_theta;      // the whole-step seam updates the densities in place (bzi_apply_closure)
        const double *cs[4 + BZ_MAX_TRACERS];
        double *Gs[4 + BZ_MAX_TRACERS];
        int ns = 0;
        cs[ns] = s->theta; Gs[ns++] = Gth;
        cs[ns] = s->q; Gs[ns++] = Gq;
        if (g.microphysics == 2) {
            cs[ns] = (const double *)ctx->kessler.cloud_liquid_mass_fraction; Gs[ns++] = (double *)(in_place ? ctx->kessler.cloud_liquid_density : ctx->kessler.G_cloud_liquid_density);
            cs[ns] = (const double *)ctx->kessler.rain_mass_fraction; Gs[ns++] = (double *)(in_place ? ctx->kessler.rain_density : ctx->kessler.G_rain_density);
        }
        for (int t = 0; t < ctx->n_tracers; ++t) {
            cs[ns] = (const double *)ctx->tracers[t].specific; Gs[ns++] = (double *)(in_place ? ctx->tracers[t].density : ctx->tracers[t].G);
        }
        for (int q = 0; q < ns; ++q) {
#define DIF_SCA(V, I) hipLaunchKernelGGL((k_diffusivity_scalar<V, I, RhoColumn>), grid, block, 0, ctx->stream, g, KAs, RhoColumn(), cs[q], Gs[q], scale)
            if (vert) DIF_SCA(true, false);
            else if (impl) DIF_SCA(false, true);
            else DIF_SCA(false, false);
#undef DIF_SCA
        }
    }
    BZ_LAUNCH_CHECK();
    return BZ_OK;
}

// implicit_step! of every prognostic field with dtau = alpha dt: momentum from (ru, rv, rw), the thermodynamic density and the moisture
// from (rth, rq), the Kessler species and the tracers from the context.  One table launch (constant K) and one solve launch.
int bzi_implicit_step(bz_ctx *ctx, double *ru, double *rv, double *rw, double *rth, double *rq, double dtau)
{
    if (!ctx->has_diffusivity || ctx->diffusivity.time_discretization != 1) return BZ_OK;
    int rc;
    if ((rc = bzi_diffusivity_halos(ctx))) return rc;
    const DevGrid &g = ctx->dg;
    ImplicitList L;
    int nf = 0;
    if (dif_momentum_on(ctx)) {
        L.f[nf] = ru; L.cls[nf++] = DIF_CLASS_U;
        L.f[nf] = rv; L.cls[nf++] = DIF_CLASS_V;
        L.f[nf] = rw; L.cls[nf++] = DIF_CLASS_W;
    }
    if (dif_scalars_on(ctx)) {
        L.f[nf] = rth; L.cls[nf++] = DIF_CLASS_C;
        L.f[nf] = rq; L.cls[nf++] = DIF_CLASS_C;
        if (g.microphysics == 2) {
            L.f[nf] = (double *)ctx->kessler.cloud_liquid_density; L.cls[nf++] = DIF_CLASS_C;
            L.f[nf] = (double *)ctx->kessler.rain_density; L.cls[nf++] = DIF_CLASS_C;
        }
        for (int t = 0; t < ctx->n_tracers; ++t) { L.f[nf] = (double *)ctx->tracers[t].density; L.cls[nf++] = DIF_CLASS_C; }
    }
    if (!nf) return BZ_OK;
    for (int q = 0; q < nf; ++q)
        if (!L.f[q]) return BZ_ERR_INVALID;
    ProfileScope ps(ctx, "implicit_step");
    const KSource NUs{ctx->diff_nu, ctx->diffusivity.nu}, KAs{ctx->diff_kappa, ctx->diffusivity.kappa};
    const dim3 grid((g.Nx + 63) / 64, g.Ny, nf), block(64);
    if (ctx->diff_nu || ctx->diff_kappa) {
        if ((rc = dif_ensure_scratch(ctx, nf))) return rc;
        hipLaunchKernelGGL(k_implicit_step<true>, grid, block, 0, ctx->stream, g, L, NUs, KAs, dtau, (const double *)nullptr, ctx->d_diff_scratch,
                           g.Sxy * (long long)(g.Nz + 2 * g.Hz + 1));
    } else {
        hipLaunchKernelGGL(k_implicit_table, dim3(1), dim3(64), 0, ctx->stream, g, ctx->diffusivity.nu, ctx->diffusivity.kappa, dtau, ctx->d_diff_table);
        hipLaunchKernelGGL(k_implicit_step<false>, grid, block, 0, ctx->stream, g, L, NUs, KAs, dtau, (const double *)ctx->d_diff_table, (double *)nullptr, 0LL);
    }
    BZ_LAUNCH_CHECK();
    return BZ_OK;
}

extern "C" int bz_implicit_step(bz_ctx *ctx, const bz_state *s, double dt)
{
    if (!ctx || !s) return BZ_ERR_INVALID;
    BZ_REJECT_KINEMATIC(ctx, "bz_implicit_step");
    return bzi_implicit_step(ctx, s->rho_u, s->rho_v, s->rho_w, s->rho_theta, s->rho_q, dt);
}

// ---- CompressibleDynamics + SplitExplicitTimeDiscretization: the closure terms are slow terms of the split-explicit step ----
// (src/TimeSteppers/acoustic_substep_helpers.jl:55-93; potential_temperature_tendency.jl:100-105; dynamics_kernel_functions.jl:132-159)
// momentum and rho theta with rho_d at the flux locations, after the advective slow tendencies
int bzi_cmp_diffusivity_slow(bz_ctx *ctx, const bz_compressible_state *s, const bz_compressible_prognostic *G)
{
    int rc;
    if (!dif_momentum_on(ctx) && !dif_scalars_on(ctx)) return BZ_OK;      // nu = kappa = the number 0: nothing is launched
    if ((rc = bzi_diffusivity_halos(ctx))) return rc;
    const DevGrid &g = ctx->dg;
    const bool vert = ctx->diffusivity.formulation == 1;
    ProfileScope ps(ctx, "diffusivity_tendencies");
    const KSource NUs{ctx->diff_nu, ctx->diffusivity.nu}, KAs{ctx->diff_kappa, ctx->diffusivity.kappa};
    const RhoField R{s->rho_d};
    const dim3 grid((g.Nx + 255) / 256, g.Ny, g.Nz), block(256);
    bz_bools([&](auto v) {
        if (dif_momentum_on(ctx))
            hipLaunchKernelGGL((k_diffusivity_momentum<v(), false, RhoField>), grid, block, 0, ctx->stream, g, NUs, R, (const double *)s->u,
                               (const double *)s->v, (const double *)s->w, G->rho_u, G->rho_v, G->rho_w, 1.0);
        if (dif_scalars_on(ctx))
            hipLaunchKernelGGL((k_diffusivity_scalar<v(), false, RhoField>), grid, block, 0, ctx->stream, g, KAs, R, (const double *)s->theta,
                               G->rho_theta, 1.0);
    }, vert);
    BZ_LAUNCH_CHECK();
    return BZ_OK;
}

// the water scalars (rho q; with Kessler rho q^cl, rho q^r) of either closure with the total density at the faces: one launch
int bzi_cmp_water_closure(bz_ctx *ctx, const bz_compressible_state *s, const bz_compressible_prognostic *G, const int *skip_if_dry)
{
    if (!ctx->has_closure && !ctx->has_diffusivity) return BZ_OK;
    if (ctx->has_diffusivity && !dif_scalars_on(ctx)) return BZ_OK;
    int rc;
    if (ctx->has_diffusivity && (rc = bzi_diffusivity_halos(ctx))) return rc;
    const DevGrid &g = ctx->dg;
    ProfileScope ps(ctx, "water_closure_tendencies");
    WaterList L;
    L.c[0] = s->q; L.G[0] = G->rho_q;
    const bool kes = g.microphysics == 2;
    L.c[1] = kes ? (const double *)ctx->kessler.cloud_liquid_mass_fraction : nullptr; L.G[1] = kes ? (double *)ctx->kessler.G_cloud_liquid_density : nullptr;
    L.c[2] = kes ? (const double *)ctx->kessler.rain_mass_fraction : nullptr; L.G[2] = kes ? (double *)ctx->kessler.G_rain_density : nullptr;
    const RhoField R{s->rho};
    const dim3 grid((g.Nx + 255) / 256, g.Ny, g.Nz), block(256);
    const bool vert = ctx->has_diffusivity && ctx->diffusivity.formulation == 1;
    bz_bools([&](auto v, auto k3) {
        constexpr int NS = k3() ? 3 : 1;
        if (ctx->has_closure)      // kappa = nu_e / Pr; nu_e carries its halos (bzi_cmp_closure_fields)
            hipLaunchKernelGGL((k_water_closure<false, NS, KScaled>), grid, block, 0, ctx->stream, g, KScaled{ctx->closure_nu, 1.0 / ctx->closure.prandtl_number},
                               R, L, skip_if_dry);
        else
            hipLaunchKernelGGL((k_water_closure<v(), NS, KSource>), grid, block, 0, ctx->stream, g, KSource{ctx->diff_kappa, ctx->diffusivity.kappa}, R, L,
                               skip_if_dry);
    }, vert, kes);
    BZ_LAUNCH_CHECK();
    return BZ_OK;
}
