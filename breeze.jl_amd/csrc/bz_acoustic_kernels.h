// bz_acoustic_kernels.h — kernels of the acoustic substep loop (launched by bz_acoustic.hip; the kernel structure of a substep is described
// at the top of bz_compressible.hip).
#pragma once
#include "bz_compressible_internal.h"

// ---------------------------------------------------------------------------------------------------------------------
// acoustic stage kernels
// ---------------------------------------------------------------------------------------------------------------------
// _zero_x_wall_face! / _zero_y_wall_face! (acoustic_substepping.jl:1367-1375) as a mask on the four faces a column's predictor reads: the
// reference zeroes the plane after the horizontal step and again after the damping; nothing reads the face between the kernel that writes it and
// the zeroing, so forming the zero where the face value is formed gives the same fields
__device__ __forceinline__ void ac_wall_faces(const DevGrid &g, const AcParams &P, int i, int j, double &up0, double &up1, double &vp0, double &vp1)
{
    if (g.bounded_x) {
        if (i == 0 && P.wall_w) up0 = 0.0;
        if (i == g.Nx - 1) up1 = 0.0;
    }
    if (g.bounded_y) {
        if (j == 0 && P.wall_s) vp0 = 0.0;
        if (j == g.Ny - 1) vp1 = 0.0;
    }
}
__device__ __forceinline__ bool ac_accumulate(const AcParams &P)
{
    return !(P.skip_avg_if_dry && __builtin_amdgcn_readfirstlane(*P.skip_avg_if_dry) == 1);
}

// Block order of the pointwise stage kernels (grid (Nx / 256, Ny, Nz)).  They read the row below (j - 1) and the level below (k - 1) of one to
// three of their 19 - 41 arrays; in launch order row j - 1 belonged to another XCD and level k - 1 had been read a whole plane of all the arrays
// earlier (PMC r05: stage-init 12.2 GB per launch for 10.2 GB of words, stage-end 23.0 / 25.1 for 19.9 / 22.0).  Here XCD c owns the groups of
// eight rows G = c, c + 8, ... and walks a group x fastest, then its eight rows, then z: the level below is eight rows of traffic away (~0.7 MB),
// the row below inside the group too.  Ny a multiple of 64, else launch order.
__device__ __forceinline__ void ac_pencil_block(int &bx, int &j, int &k)
{
    bx = blockIdx.x; j = blockIdx.y; k = blockIdx.z;
    const unsigned gx = gridDim.x, gy = gridDim.y, gz = gridDim.z;
    if ((gy & 63u) == 0) {
        const unsigned w = bx + gx * (j + gy * k), c = w & 7u;
        unsigned r = w >> 3;
        bx = (int)(r % gx); r /= gx;
        const unsigned jj = r & 7u; r >>= 3;
        k = (int)(r % gz); r /= gz;
        j = (int)(((r * 8 + c) * 8) + jj);
    }
    bx = __builtin_amdgcn_readfirstlane(bx); j = __builtin_amdgcn_readfirstlane(j); k = __builtin_amdgcn_readfirstlane(k);
}

// assemble_slow_vertical_momentum_tendency! + initialize_stage_perturbations! (acoustic_substepping.jl:727-752,793-838)
// ZERO: the three time-average accumulators are zeroed here (unfused substeps); with the fused substep kernels the first substep of a
// stage assigns them instead (three words per cell and stage written only to be read back once).
// STORE0: first stage of a whole step — the state IS U0, so the perturbations are exact zeros and store_initial_state! rides along
// (the six copies of bzi_compressible_store_initial_state: 12 words per cell; here 6, and the five state reads are shared).
// PF (round 6): the horizontal gradient of the stage's p^L, which the reference's explicit horizontal step re-evaluates in every substep
// (acoustic_substepping.jl:859-876), is folded into the slow tendencies once per stage: Gp_ru = G_ru - dx p^L, Gp_rv = G_rv - dy p^L.
// NOPERT (round 6): the stage's initial perturbations are not stored — the first forward / backward sweep of the stage forms them from
// U0 - U itself (k_ac_forward2<.., INIT>: 1) or knows them to be exact zeros (first stage of a whole step: 2)
template <bool ZERO, bool STORE0, bool PF, bool NOPERT, class ST>
__global__ __launch_bounds__(256) void k_ac_stage_init(DevGrid g, AcFieldsT<ST> F)
{
    int bx, j, k;
    ac_pencil_block(bx, j, k);
    const int i = bx * 256 + threadIdx.x;
    if (i >= g.Nx) return;
    const long long sz = g.Sxy;
    const long long n = g.idx(i, j, k);
    if (j >= g.Ny) {
        // y-slab: the row above the slab.  The north face of the slab's last row reads its folded tendency; G_rv and p of this row arrived
        // with the halo exchanges, and the rank that owns the row forms the same value from the same numbers
        if (PF) F.Gp_rv[n] = F.G_rv[n] - (F.p[n] - F.p[n - g.Sx]) * g.rdy;
        return;
    }
    if (PF) {
        const WrapIdx W = wrap_of(g, i, j);
        const double p0 = F.p[n];
        F.Gp_ru[n] = F.G_ru[n] - (p0 - F.p[n + W.im]) * g.rdx;
        F.Gp_rv[n] = F.G_rv[n] - (p0 - F.p[n + W.jm]) * g.rdy;
    }
    if (STORE0) {
        // U0 - U with U0 := U: (+0) for every finite value, as the subtraction of the stored copy gives
        ((double *)F.U0_rho_d)[n] = F.rho_d[n];
        ((double *)F.U0_rth)[n] = F.rth[n];
        ((double *)F.U0_ru)[n] = F.ru[n];
        ((double *)F.U0_rv)[n] = F.rv[n];
        ((double *)F.U0_rw)[n] = F.rw[n];
        ((double *)F.U0_rq)[n] = F.rq[n];
        if (!NOPERT) { F.rp[n] = 0.0; F.rthp_out[n] = 0.0; F.rup[n] = 0.0; F.rvp[n] = 0.0; F.rwp[n] = 0.0; }
    } else if (!NOPERT) {
    F.rp[n] = F.U0_rho_d[n] - F.rho_d[n];
    F.rthp_out[n] = F.U0_rth[n] - F.rth[n];     // start buffers of the ping-pong fields (set by the launcher)
    F.rup[n] = F.U0_ru[n] - F.ru[n];
    F.rvp[n] = F.U0_rv[n] - F.rv[n];
    F.rwp[n] = F.U0_rw[n] - F.rw[n];
    }
    if (ZERO) {
    F.au[n] = 0.0;
    F.av[n] = 0.0;
    F.aw[n] = 0.0;
    }
    if (k == 0) {
        F.Gs[n] = 0.0;
    } else {
        const long long m = n - sz;
        const double dp = ((F.p[n] - g.p_r[k]) - (F.p[m] - g.p_r[k - 1])) * g.rdzf[k];
        const double rf = ((F.rho[n] - g.rho[k]) + (F.rho[m] - g.rho[k - 1])) / 2.0;
        F.Gs[n] = F.G_rw[n] - dp - g.g * rf;
    }
    if (k == g.Nz - 1) {
        if (STORE0) { ((double *)F.U0_rw)[n + sz] = F.rw[n + sz]; if (!NOPERT) F.rwp[n + sz] = 0.0; }
        else if (!NOPERT) F.rwp[n + sz] = F.U0_rw[n + sz] - F.rw[n + sz];
        F.Gs[n + sz] = 0.0;
    }
}

// Klemp-Skamarock-Ha damping of the previous substep (acoustic_substepping.jl:1123-1139) followed by the explicit
// horizontal step of this substep (:860-881) and the time-average accumulation (:999-1000).
template <bool DAMP, bool STEP, class ST>
__global__ __launch_bounds__(256) void k_ac_horizontal(DevGrid g, AcFieldsT<ST> F, AcParams P)
{
    const int i = blockIdx.x * 256 + threadIdx.x, j = blockIdx.y, k = blockIdx.z;
    if (i >= g.Nx) return;
    const WrapIdx W = wrap_of(g, i, j);
    const long long n = g.idx(i, j, k), mx = n + W.im, my = n + W.jm;
    double up = F.rup[n], vp = F.rvp[n];
    const double rt = F.rthp[n], rtx = F.rthp[mx], rty = F.rthp[my];
    if (DAMP) {
        const double d0 = rt - F.rth_old[n];
        const double ddx = (d0 - (rtx - F.rth_old[mx])) * g.rdx;
        const double ddy = (d0 - (rty - F.rth_old[my])) * g.rdy;
        const double th = F.thL[n];
        up -= P.kdamp * ddx / ((th + F.thL[mx]) / 2.0);
        vp -= P.kdamp * ddy / ((th + F.thL[my]) / 2.0);
    }
    if (STEP) {
        const double p0 = F.p[n];
        double dpx = (p0 - F.p[mx]) * g.rdx;
        double dpy = (p0 - F.p[my]) * g.rdy;
        if (P.gate != 0.0) {
            const double c0 = F.Clin[n] * rt;
            dpx = dpx + P.gate * ((c0 - F.Clin[mx] * rtx) * g.rdx);
            dpy = dpy + P.gate * ((c0 - F.Clin[my] * rty) * g.rdy);
        }
        up += P.dtau * (F.G_ru[n] - dpx);
        vp += P.dtau * (F.G_rv[n] - dpy);
        if (g.bounded_x && i == 0 && P.wall_w) up = 0.0;
        if (g.bounded_y && j == 0 && P.wall_s) vp = 0.0;
        F.au[n] += up;
        F.av[n] += vp;
    }
    if (g.bounded_x && i == 0 && P.wall_w) up = 0.0;
    if (g.bounded_y && j == 0 && P.wall_s) vp = 0.0;
    F.rup[n] = up;
    F.rvp[n] = vp;
}

// boundary-aware centre->face interpolation of theta^L (acoustic_substepping.jl:539-550) from the two cell values
__device__ __forceinline__ double ibz(double fp, double fm, bool p_per, bool m_per)
{
    fp = p_per ? fm : fp;
    fm = m_per ? fp : fm;
    return (fp + fm) / 2.0;
}

// one face of k_ac_horizontal: cells a (low side) and b (high side) of the face, rd = 1/spacing
template <bool DAMP>
__device__ __forceinline__ double ac_face_update(double up, double G, double rt_b, double rt_a, double rto_b, double rto_a,
                                                 double th_b, double th_a, double C_b, double C_a, double p_b, double p_a,
                                                 double rd, const AcParams &P)
{
    if (DAMP) {
        const double dd = ((rt_b - rto_b) - (rt_a - rto_a)) * rd;
        up -= P.kdamp * dd / ((th_b + th_a) / 2.0);
    }
    double dp = (p_b - p_a) * rd;
    if (P.gate != 0.0) dp = dp + P.gate * ((C_b * rt_b - C_a * rt_a) * rd);
    return up + P.dtau * (G - dp);
}

// block shapes of the column kernels (measured on MI355X, 512x512x256: forward sweep 64x4 99 ms/step vs 256x1 102;
// backward sweep 256x1 32.5 vs 64x4 37.8)
#define ACX 64
#define ACY 4
#define ABX 256
#define ABY 1
#define AC_MINW 1
// _build_predictors! + _build_vertical_rhs! + forward sweep of the BatchedTridiagonalSolver
// (acoustic_substepping.jl:605-659,907-970).  FUSED: the horizontal step (k_ac_horizontal) of the four faces of the
// column is evaluated in place of loading (rho u)', (rho v)': each face is computed by its two adjacent columns with
// identical arithmetic and stored by its owner, which removes one read + one write of (rho u)', (rho v)' and the separate
// pass over (rho theta)', theta^L, C per substep.
template <bool FIRST, bool FUSED, bool DAMP, class ST>
__global__ __launch_bounds__(ACX * ACY, AC_MINW) void k_ac_column_forward(DevGrid g, AcFieldsT<ST> F, AcParams P)
{
    // Workgroups go round-robin to the 8 XCDs in launch order (x fastest), so in launch order XCD c owns the tile COLUMN bx = c (mod 8): the
    // x neighbours of every tile live behind another XCD's L2, and the one value a row's edge lane needs of them (eight arrays) costs a
    // 128-byte line through the fabric each.  With P.xcd XCD c owns the BAND of tile rows [c gy/8, (c+1) gy/8) instead and walks it x fastest:
    // both x neighbours and (but at the band edges) both y neighbours are tiles of the same L2.
    int bx = blockIdx.x, by = blockIdx.y;
    if (P.xcd) {
        const unsigned w = blockIdx.y * gridDim.x + blockIdx.x, c = w & 7u, r = w >> 3;
        bx = (int)(r % gridDim.x);
        by = (int)(c * (gridDim.y >> 3) + r / gridDim.x);
    }
    const int i = bx * ACX + threadIdx.x, j = by * ACY + threadIdx.y;
    if (i >= g.Nx || j >= g.Ny) return;
    const WrapIdx W = wrap_of(g, i, j);
    const long long sz = g.Sxy;
    const int Nz = g.Nz;
    long long n = g.idx(i, j, 0);
    const double dtn2 = P.dtn * P.dtn;

    // rings: theta^L at k, k+1 (own column) and at faces k-1, k; C at k-1, k; old (rho w)' at faces k-1, k, k+1
    double th_0 = F.thL[n], th_p = F.thL[n + sz];
    double C_m = 0.0, C_0 = F.Clin[n];
    // Neighbours of the two linearisation fields (round 4).  The own-column values ride rings that are loaded one (C) or two (theta_L)
    // levels ahead; the neighbours used to be loaded at the level that needs them — the same cache lines, one or two level fronts of
    // the whole grid later (47 KB per block and level x 1024 resident blocks: long evicted), so every line of theta_L and C crossed
    // the fabric twice.  Now the x neighbours come from the neighbouring lanes' ring values (a row of the block is one wavefront; only
    // its two edge lanes load), and the y neighbours are requested together with the own-column value of their level and carried.
    const bool FX = FUSED && (ACX == 64) && sizeof(ST) == 8;      // (Float32 working fields: measured slower — 74 -> 101 ms per step of forward sweeps — and stay on the loads)
    const int lane = threadIdx.x;
    double thy_m0 = 0.0, thy_p0 = 0.0, thy_m1 = 0.0, thy_p1 = 0.0;      // theta_L of rows j-1 / j+1 at levels k and k+1
    double cy_m0 = 0.0, cy_p0 = 0.0;                                    // C of rows j-1 / j+1 at level k
    if (FX) {
        thy_m0 = F.thL[n + W.jm]; thy_p0 = F.thL[n + W.jp];
        thy_m1 = F.thL[n + sz + W.jm]; thy_p1 = F.thL[n + sz + W.jp];
        cy_m0 = F.Clin[n + W.jm]; cy_p0 = F.Clin[n + W.jp];
    }
    double w_m = 0.0, w_0 = F.rwp[n], w_p = F.rwp[n + sz];
    double rs_m = 0.0, rths_m = 0.0, rp_m = 0.0, rthp_m = 0.0;
    double beta = 1.0, phi_m = 0.0, c_m = 0.0;     // row 0: b = 1, c = 0, f = 0
    double thf_0 = th_0, thf_m = th_0;               // theta at faces k (k = 0: one-sided) and k-1

    for (int k = 0; k < Nz; ++k, n += sz) {
        const double rdc = g.rdzc[k];
        const double Ax = g.Ax[k], Ay = g.Ay[k], Vinv = g.Vinv_c[k];
        const double rp = F.rp[n], rthp = F.rthp[n];
        double thxm, thxp, thym, thyp;
        if (FX) {
            // lanes 0 and 63 of the row hold the block's edge columns: their outer neighbours belong to another block (or wrap around)
            const double e_m = (lane == 0) ? F.thL[n + W.im] : 0.0, e_p = (lane == ACX - 1 || i == g.Nx - 1) ? F.thL[n + W.ip] : 0.0;
            thxm = __shfl_up(th_0, 1); thxp = __shfl_down(th_0, 1);
            if (lane == 0) thxm = e_m;
            if (lane == ACX - 1 || i == g.Nx - 1) thxp = e_p;
            thym = thy_m0; thyp = thy_p0;
        } else {
            thxm = F.thL[n + W.im]; thxp = F.thL[n + W.ip]; thym = F.thL[n + W.jm]; thyp = F.thL[n + W.jp];
        }
        double up0, up1, vp0, vp1;
        if (FUSED) {
            const long long nxm = n + W.im, nxp = n + W.ip, nym = n + W.jm, nyp = n + W.jp;
            const double rt_xm = F.rthp[nxm], rt_xp = F.rthp[nxp], rt_ym = F.rthp[nym], rt_yp = F.rthp[nyp];
            double o0 = 0.0, o_xm = 0.0, o_xp = 0.0, o_ym = 0.0, o_yp = 0.0;
            if (DAMP) { o0 = F.rth_old[n]; o_xm = F.rth_old[nxm]; o_xp = F.rth_old[nxp]; o_ym = F.rth_old[nym]; o_yp = F.rth_old[nyp]; }
            double c_xm = 0.0, c_xp = 0.0, c_ym = 0.0, c_yp = 0.0;
            if (FX) {
                const double e_m = (lane == 0) ? F.Clin[nxm] : 0.0, e_p = (lane == ACX - 1 || i == g.Nx - 1) ? F.Clin[nxp] : 0.0;
                c_xm = __shfl_up(C_0, 1); c_xp = __shfl_down(C_0, 1);
                if (lane == 0) c_xm = e_m;
                if (lane == ACX - 1 || i == g.Nx - 1) c_xp = e_p;
                c_ym = cy_m0; c_yp = cy_p0;
            } else if (P.gate != 0.0) { c_xm = F.Clin[nxm]; c_xp = F.Clin[nxp]; c_ym = F.Clin[nym]; c_yp = F.Clin[nyp]; }
            const double p0 = F.p[n], p_xm = F.p[nxm], p_xp = F.p[nxp], p_ym = F.p[nym], p_yp = F.p[nyp];
            up0 = ac_face_update<DAMP>(F.rup_in[n], F.G_ru[n], rthp, rt_xm, o0, o_xm, th_0, thxm, C_0, c_xm, p0, p_xm, g.rdx, P);
            up1 = ac_face_update<DAMP>(F.rup_in[nxp], F.G_ru[nxp], rt_xp, rthp, o_xp, o0, thxp, th_0, c_xp, C_0, p_xp, p0, g.rdx, P);
            vp0 = ac_face_update<DAMP>(F.rvp_in[n], F.G_rv[n], rthp, rt_ym, o0, o_ym, th_0, thym, C_0, c_ym, p0, p_ym, g.rdy, P);
            vp1 = ac_face_update<DAMP>(F.rvp_in[nyp], F.G_rv[nyp], rt_yp, rthp, o_yp, o0, thyp, th_0, c_yp, C_0, p_yp, p0, g.rdy, P);
            ac_wall_faces(g, P, i, j, up0, up1, vp0, vp1);
            F.rup[n] = up0;
            F.rvp[n] = vp0;
            if (FIRST) { F.au[n] = 0.0 + up0; F.av[n] = 0.0 + vp0; }      // first substep of the stage: the accumulators start here (0 + x keeps the bits of the zeroed array)
            else { F.au[n] += up0; F.av[n] += vp0; }
        } else {
            up0 = F.rup[n]; up1 = F.rup[n + W.ip]; vp0 = F.rvp[n]; vp1 = F.rvp[n + W.jp];
            ac_wall_faces(g, P, i, j, up0, up1, vp0, vp1);
            F.rth_old[n] = rthp;
        }
        // theta face k+1 (top face: one-sided)
        const double thf_p = (k + 1 < Nz) ? (th_p + th_0) / 2.0 : th_0;

        const double dxM = Ax * up1 - Ax * up0;
        const double dxT = Ax * ((thxp + th_0) / 2.0) * up1 - Ax * ((th_0 + thxm) / 2.0) * up0;
        const double dyM = Ay * vp1 - Ay * vp0;
        const double dyT = Ay * ((thyp + th_0) / 2.0) * vp1 - Ay * ((th_0 + thym) / 2.0) * vp0;
        const double divM = Vinv * (dxM + dyM);
        const double divT = Vinv * (dxT + dyT);
        const double dzW = (w_p - w_0) * rdc;
        const double dzT = (thf_p * w_p - thf_0 * w_0) * rdc;
        const double rs = rp + P.dtau * (F.G_rho_d[n] - divM) - P.dto * dzW;
        const double rths = rthp + P.dtau * (P.f_theta * F.G_rth[n] - divT) - P.dto * dzT;
        F.rs[n] = rs;
        F.rths[n] = rths;

        double phi = 0.0;
        if (k > 0) {
            const double rdf = g.rdzf[k], rdm = g.rdzc[k - 1];
            // right-hand side at face k
            const double dps = (C_0 * rths - C_m * rths_m) * rdf;
            const double dpo = (C_0 * rthp - C_m * rthp_m) * rdf;
            const double Gp = P.dto * dpo + P.dtn * dps;
            const double Gb = g.g * (P.dto * ((rp + rp_m) / 2.0) + P.dtn * ((rs + rs_m) / 2.0));
            const double d2 = ((w_p - w_0) * rdc - (w_0 - w_m) * rdm) * rdf;
            const double Gd = -P.d_old * d2;
            const double sp = F.sponge[k];                // sponge_rhs / sponge_term_diag (acoustic_substepping.jl:591-602)
            const double f = w_0 + P.dtau * P.f_w * F.Gs[n] - Gp - Gb - Gd - fabs(P.dto) * sp * w_0;
            // coefficients of row k
            const double a = -dtn2 * C_m * thf_m * rdm * rdf + dtn2 * g.g * rdm / 2.0 + (-P.d_new * rdm * rdf);
            const double b = 1.0 + (dtn2 * thf_0 * (C_0 * rdc + C_m * rdm) * rdf + dtn2 * g.g * (rdc - rdm) / 2.0 +
                                    P.d_new * (rdc + rdm) * rdf + fabs(P.dtn) * sp);
            const double t = c_m / beta;
            beta = b - a * t;
            phi = (f - a * phi_m) / beta;
            if (FIRST) F.tfac[n] = t;
            // upper coefficient of this row, used by the next one
            c_m = -dtn2 * C_0 * thf_p * rdc * rdf + (-dtn2 * g.g * rdc / 2.0) + (-P.d_new * rdc * rdf);
        } else if (FIRST) {
            F.tfac[n] = 0.0;
        }
        F.phi[n] = phi;
        phi_m = phi;

        // advance the rings
        rs_m = rs; rths_m = rths; rp_m = rp; rthp_m = rthp;
        C_m = C_0;
        th_0 = th_p; thf_m = thf_0; thf_0 = thf_p;
        w_m = w_0; w_0 = w_p;
        if (k + 1 < Nz) {
            C_0 = F.Clin[n + sz];
            th_p = (k + 2 < Nz) ? F.thL[n + 2 * sz] : th_0;
            w_p = F.rwp[n + 2 * sz];
            if (FX) {      // the y neighbours of the levels just requested, with them
                cy_m0 = F.Clin[n + sz + W.jm]; cy_p0 = F.Clin[n + sz + W.jp];
                thy_m0 = thy_m1; thy_p0 = thy_p1;
                if (k + 2 < Nz) { thy_m1 = F.thL[n + 2 * sz + W.jm]; thy_p1 = F.thL[n + 2 * sz + W.jp]; }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// The fused forward sweep of periodic grids (ac_forward2_ok), written for the memory pipe.  A block is 512 threads (64 x 8, 128 x 4,
// 256 x 2 or 512 x 1 columns; a wavefront is always 64 consecutive cells of one row) with a register budget of two waves per SIMD.  A
// column marches up its levels; per level
//   * every load — the level's own words, the neighbours' and the ring words of the levels above — is issued before the first store, and
//     all stores close the level, so the compiler never has to drain the vector-memory counter between a store and a load it cannot prove
//     independent;
//   * every access is `uniform base + 32-bit per-lane byte offset` (the saddr form of global_load: one offset register per neighbour
//     displacement instead of a 64-bit address per array);
//   * the loads of level k + 1 are issued before level k is worked on (two levels per trip, see the loop), so they fly under the
//     arithmetic, the stores and the barrier of level k;
//   * one s_barrier keeps the rows of a block in step: a row's y neighbours are requested while their lines are near;
//   * neighbours in x of theta_L, C, (rho theta)' and its previous value come from the neighbouring lanes by DPP moves (bz_lane_up /
//     bz_lane_down); the two edge lanes of a row fetch theirs with one predicated load per array.
// What each of these bought over k_ac_column_forward, and the variants that lost, are in DESIGN §7 ("k_ac_forward2").
// The arithmetic is the text of the kernel above, so the results carry its bits; PF folds the stage-constant horizontal gradient of p^L
// into the slow tendencies (Gp_ru, Gp_rv written by k_ac_stage_init: one array and four neighbour loads less per level and substep; the
// only deviation, one rounding of G - dp).
// ---------------------------------------------------------------------------------------------------------------------
template <class T>
__device__ __forceinline__ T ac_ld(const T *base, unsigned e)
{
    return *(const T *)((const char *)base + (size_t)(e * (unsigned)sizeof(T)));
}
// (non-temporal forms for the words no other column reads were tried and did not pay: every access is a plain one)
template <class T, class V>
__device__ __forceinline__ void ac_st(T *base, unsigned e, V v)
{
    *(T *)((char *)base + (size_t)(e * (unsigned)sizeof(T))) = (T)v;
}

template <bool DAMP, bool PF>
__device__ __forceinline__ double ac_face_update2(double up, double G, double rt_b, double rt_a, double rto_b, double rto_a,
                                                  double th_b, double th_a, double C_b, double C_a, double p_b, double p_a,
                                                  double rd, const AcParams &P)
{
    if (DAMP) {
        const double dd = ((rt_b - rto_b) - (rt_a - rto_a)) * rd;
        up -= P.kdamp * dd / ((th_b + th_a) / 2.0);
    }
    if (PF) {      // G already carries -(p_b - p_a) rd
        if (P.gate != 0.0) G = G - P.gate * ((C_b * rt_b - C_a * rt_a) * rd);
        return up + P.dtau * G;
    }
    double dp = (p_b - p_a) * rd;
    if (P.gate != 0.0) dp = dp + P.gate * ((C_b * rt_b - C_a * rt_a) * rd);
    return up + P.dtau * (G - dp);
}

// INIT (first substep of a stage only): 0 the stage's initial perturbations are read from their arrays (k_ac_stage_init stored them);
// 1 they are formed here from U0 - U (rounded through the storage type, as the stored ones are) — the initialisation pass neither writes
// them (5 words per cell) nor does this sweep read them back (5): it reads U0 and U (10) and stores the initial (rho theta)' (1), which
// the next substep's damping and the stage epilogue read; 2 first stage of a whole step: the state IS U0, the perturbations are exact zeros
template <bool FIRST, bool DAMP, bool PF, class ST, int INIT = 0>
__global__ __launch_bounds__(512, 2) void k_ac_forward2(DevGrid g, AcFieldsT<ST> F, AcParams P)
{
    static_assert(FIRST || INIT == 0, "initial perturbations belong to the first substep of a stage");
    int bx = blockIdx.x, by = blockIdx.y;
    if (P.xcd) {      // XCD c owns the band of tile rows [c gy/8, (c+1) gy/8) (see k_ac_column_forward)
        const unsigned w = blockIdx.y * gridDim.x + blockIdx.x, c = w & 7u, r = w >> 3;
        bx = (int)(r % gridDim.x);
        by = (int)(c * (gridDim.y >> 3) + r / gridDim.x);
    }
    // 512 threads as 64 x 8, 128 x 4, 256 x 2 or 512 x 1 columns (BZ_AC_BX): a wavefront is always 64 consecutive cells of one row
    const int i = bx * (int)blockDim.x + threadIdx.x, j = by * (int)blockDim.y + threadIdx.y;
    if (i >= g.Nx || j >= g.Ny) return;
    const WrapIdx W = wrap_of(g, i, j);
    const unsigned sz = (unsigned)g.Sxy;
    const unsigned dxp = (unsigned)(int)W.ip, dym = (unsigned)(int)W.jm, dyp = (unsigned)(int)W.jp;
    const int Nz = g.Nz;
    unsigned e = (unsigned)g.idx(i, j, 0);
    const double dtn2 = P.dtn * P.dtn;
    const int lane = threadIdx.x & 63;
    const bool edge_m = (lane == 0), edge_p = (lane == 63 || i == g.Nx - 1);
    const bool edge = edge_m || edge_p;
    const unsigned dedge = edge_m ? (unsigned)(int)W.im : dxp;
    const ColPtr::cptr sponge = (ColPtr::cptr)F.sponge;
    const double *Gu = PF ? F.Gp_ru : F.G_ru, *Gv = PF ? F.Gp_rv : F.G_rv;
    const bool acc = ac_accumulate(P);      // uniform: the time-average accumulators of this stage are wanted

    // rings (see k_ac_column_forward): theta_L at k, k+1 of the own column and of rows j-1 / j+1, C at k-1, k (rows j-1 / j+1: k),
    // old (rho w)' at faces k-1, k, k+1
    double th_0 = ac_ld(F.thL, e), th_p = ac_ld(F.thL, e + sz);
    double C_m = 0.0, C_0 = ac_ld(F.Clin, e);
    double thy_m0 = ac_ld(F.thL, e + dym), thy_p0 = ac_ld(F.thL, e + dyp);
    double thy_m1 = ac_ld(F.thL, e + sz + dym), thy_p1 = ac_ld(F.thL, e + sz + dyp);
    double cy_m0 = ac_ld(F.Clin, e + dym), cy_p0 = ac_ld(F.Clin, e + dyp);
    // initial perturbation of a prognostic field at element ee, as k_ac_stage_init stores it (the working fields in the storage type)
    auto pert = [&](const double *U0, const double *U, unsigned ee) { return (double)(ST)(ac_ld(U0, ee) - ac_ld(U, ee)); };
    auto pert_w = [&](unsigned ee) { return ac_ld(F.U0_rw, ee) - ac_ld((const double *)F.rw, ee); };      // (rho w)' stays in the grid's type
    double w_m = 0.0, w_0, w_p;
    if (INIT == 2) { w_0 = 0.0; w_p = 0.0; }
    else if (INIT == 1) { w_0 = pert_w(e); w_p = pert_w(e + sz); }
    else { w_0 = ac_ld(F.rwp, e); w_p = ac_ld(F.rwp, e + sz); }
    double rs_m = 0.0, rths_m = 0.0, rp_m = 0.0, rthp_m = 0.0;
    double beta = 1.0, phi_m = 0.0, c_m = 0.0;     // row 0: b = 1, c = 0, f = 0
    double thf_0 = th_0, thf_m = th_0;               // theta at faces k (k = 0: one-sided) and k-1

    // every word a level asks the memory for, as one record: `level(e, k)` issues the loads (own level k, the neighbours', the ring words of the
    // levels above); the record of level k + 1 is requested before level k is worked on (its loads fly under the ~280 VALU
    // instructions, the stores and the barrier of level k: the rows of a block that advance in lock step would otherwise leave the memory
    // pipe idle between a level's stores and the next level's loads)
    struct AcLevel {
        double rp, rthp, rt_ym, rt_yp, o0, o_ym, o_yp, ru0, ru1, rv0, rv1, Gu0, Gu1, Gv0, Gv1, p0, p_xm, p_xp, p_ym, p_yp, au_o, av_o, Grho, Grth, Gs_k;
        double e_th, e_C, e_rt, e_o;      // the row's outer neighbour: lane 0 the left one, the last lane the right one
        double C_n, cy_mn, cy_pn, th_n, thy_mn, thy_pn, w_n;
    };
    auto level = [&](const unsigned e, const int k) {
        AcLevel L;
        const unsigned exp_ = e + dxp, eym = e + dym, eyp = e + dyp;
        if (INIT == 2) { L.rp = 0.0; L.rthp = 0.0; L.rt_ym = 0.0; L.rt_yp = 0.0; }
        else if (INIT == 1) {
            L.rp = pert(F.U0_rho_d, F.rho_d, e); L.rthp = pert(F.U0_rth, F.rth, e);
            L.rt_ym = pert(F.U0_rth, F.rth, eym); L.rt_yp = pert(F.U0_rth, F.rth, eyp);
        } else {
        L.rp = ac_ld(F.rp, e); L.rthp = ac_ld(F.rthp, e);
        L.rt_ym = ac_ld(F.rthp, eym); L.rt_yp = ac_ld(F.rthp, eyp);
        }
        L.o0 = 0.0; L.o_ym = 0.0; L.o_yp = 0.0;
        if (DAMP) { L.o0 = ac_ld(F.rth_old, e); L.o_ym = ac_ld(F.rth_old, eym); L.o_yp = ac_ld(F.rth_old, eyp); }
        if (INIT == 2) { L.ru0 = 0.0; L.ru1 = 0.0; L.rv0 = 0.0; L.rv1 = 0.0; }
        else if (INIT == 1) {
            L.ru0 = pert(F.U0_ru, F.ru, e); L.ru1 = pert(F.U0_ru, F.ru, exp_); L.rv0 = pert(F.U0_rv, F.rv, e); L.rv1 = pert(F.U0_rv, F.rv, eyp);
        } else {
        L.ru0 = ac_ld(F.rup_in, e); L.ru1 = ac_ld(F.rup_in, exp_); L.rv0 = ac_ld(F.rvp_in, e); L.rv1 = ac_ld(F.rvp_in, eyp);
        }
        L.Gu0 = ac_ld(Gu, e); L.Gu1 = ac_ld(Gu, exp_); L.Gv0 = ac_ld(Gv, e); L.Gv1 = ac_ld(Gv, eyp);
        L.p0 = 0.0; L.p_xm = 0.0; L.p_xp = 0.0; L.p_ym = 0.0; L.p_yp = 0.0;
        if (!PF) {
            L.p0 = ac_ld(F.p, e); L.p_xm = ac_ld(F.p, e + (unsigned)(int)W.im); L.p_xp = ac_ld(F.p, exp_);
            L.p_ym = ac_ld(F.p, eym); L.p_yp = ac_ld(F.p, eyp);
        }
        L.au_o = 0.0; L.av_o = 0.0;
        if (!FIRST && acc && P.acc_mode != 1) { L.au_o = ac_ld(F.au, e); L.av_o = ac_ld(F.av, e); }
        L.Grho = ac_ld(F.G_rho_d, e); L.Grth = ac_ld(F.G_rth, e); L.Gs_k = ac_ld(F.Gs, e);
        L.e_th = 0.0; L.e_C = 0.0; L.e_rt = 0.0; L.e_o = 0.0;
        if (edge) {
            const unsigned ee = e + dedge;
            L.e_th = ac_ld(F.thL, ee); L.e_C = ac_ld(F.Clin, ee);
            L.e_rt = INIT == 2 ? 0.0 : INIT == 1 ? pert(F.U0_rth, F.rth, ee) : ac_ld(F.rthp, ee);
            if (DAMP) L.e_o = ac_ld(F.rth_old, ee);
        }
        // ring words of the levels above (the last levels re-read an in-range level; those values are never used)
        const unsigned e1 = (k + 1 < Nz) ? e + sz : e, e2 = (k + 2 < Nz) ? e1 + sz : e1;
        L.C_n = ac_ld(F.Clin, e1); L.cy_mn = ac_ld(F.Clin, e1 + dym); L.cy_pn = ac_ld(F.Clin, e1 + dyp);
        L.th_n = ac_ld(F.thL, e2); L.thy_mn = ac_ld(F.thL, e2 + dym); L.thy_pn = ac_ld(F.thL, e2 + dyp);
        L.w_n = INIT == 2 ? 0.0 : INIT == 1 ? pert_w(e1 + sz) : ac_ld(F.rwp, e1 + sz);
        return L;
    };
    auto work = [&](const AcLevel &L, const int k, const unsigned e) {
        const double rdc = g.rdzc[k];
        const double Ax = g.Ax[k], Ay = g.Ay[k], Vinv = g.Vinv_c[k];
        const double rp = L.rp, rthp = L.rthp, rt_ym = L.rt_ym, rt_yp = L.rt_yp, o0 = L.o0, o_ym = L.o_ym, o_yp = L.o_yp;
        const double ru0 = L.ru0, ru1 = L.ru1, rv0 = L.rv0, rv1 = L.rv1, Gu0 = L.Gu0, Gu1 = L.Gu1, Gv0 = L.Gv0, Gv1 = L.Gv1;
        const double p0 = L.p0, p_xm = L.p_xm, p_xp = L.p_xp, p_ym = L.p_ym, p_yp = L.p_yp, au_o = L.au_o, av_o = L.av_o;
        const double Grho = L.Grho, Grth = L.Grth, Gs_k = L.Gs_k, e_th = L.e_th, e_C = L.e_C, e_rt = L.e_rt, e_o = L.e_o;
        const double C_n = L.C_n, cy_mn = L.cy_mn, cy_pn = L.cy_pn, th_n = L.th_n, thy_mn = L.thy_mn, thy_pn = L.thy_pn, w_n = L.w_n;
        const double sp = sponge[k];                // sponge_rhs / sponge_term_diag (acoustic_substepping.jl:591-602)

        // ---- neighbours in x from the neighbouring lanes ----
        double thxm = bz_lane_up(th_0), thxp = bz_lane_down(th_0);
        double c_xm = bz_lane_up(C_0), c_xp = bz_lane_down(C_0);
        double rt_xm = bz_lane_up(rthp), rt_xp = bz_lane_down(rthp);
        double o_xm = 0.0, o_xp = 0.0;
        if (DAMP) { o_xm = bz_lane_up(o0); o_xp = bz_lane_down(o0); }
        if (edge_m) { thxm = e_th; c_xm = e_C; rt_xm = e_rt; o_xm = e_o; }
        if (edge_p) { thxp = e_th; c_xp = e_C; rt_xp = e_rt; o_xp = e_o; }
        const double thym = thy_m0, thyp = thy_p0, c_ym = cy_m0, c_yp = cy_p0;

        const double up0 = ac_face_update2<DAMP, PF>(ru0, Gu0, rthp, rt_xm, o0, o_xm, th_0, thxm, C_0, c_xm, p0, p_xm, g.rdx, P);
        const double up1 = ac_face_update2<DAMP, PF>(ru1, Gu1, rt_xp, rthp, o_xp, o0, thxp, th_0, c_xp, C_0, p_xp, p0, g.rdx, P);
        const double vp0 = ac_face_update2<DAMP, PF>(rv0, Gv0, rthp, rt_ym, o0, o_ym, th_0, thym, C_0, c_ym, p0, p_ym, g.rdy, P);
        const double vp1 = ac_face_update2<DAMP, PF>(rv1, Gv1, rt_yp, rthp, o_yp, o0, thyp, th_0, c_yp, C_0, p_yp, p0, g.rdy, P);
        const double au_n = FIRST ? 0.0 + up0 : (P.acc_mode == 2) ? au_o + (ru0 + up0) : au_o + up0;
        const double av_n = FIRST ? 0.0 + vp0 : (P.acc_mode == 2) ? av_o + (rv0 + vp0) : av_o + vp0;
        // theta face k+1 (top face: one-sided)
        const double thf_p = (k + 1 < Nz) ? (th_p + th_0) / 2.0 : th_0;

        const double dxM = Ax * up1 - Ax * up0;
        const double dxT = Ax * ((thxp + th_0) / 2.0) * up1 - Ax * ((th_0 + thxm) / 2.0) * up0;
        const double dyM = Ay * vp1 - Ay * vp0;
        const double dyT = Ay * ((thyp + th_0) / 2.0) * vp1 - Ay * ((th_0 + thym) / 2.0) * vp0;
        const double divM = Vinv * (dxM + dyM);
        const double divT = Vinv * (dxT + dyT);
        const double dzW = (w_p - w_0) * rdc;
        const double dzT = (thf_p * w_p - thf_0 * w_0) * rdc;
        const double rs = rp + P.dtau * (Grho - divM) - P.dto * dzW;
        const double rths = rthp + P.dtau * (P.f_theta * Grth - divT) - P.dto * dzT;

        double phi = 0.0, t = 0.0;
        if (k > 0) {
            const double rdf = g.rdzf[k], rdm = g.rdzc[k - 1];
            // right-hand side at face k
            const double dps = (C_0 * rths - C_m * rths_m) * rdf;
            const double dpo = (C_0 * rthp - C_m * rthp_m) * rdf;
            const double Gp = P.dto * dpo + P.dtn * dps;
            const double Gb = g.g * (P.dto * ((rp + rp_m) / 2.0) + P.dtn * ((rs + rs_m) / 2.0));
            const double d2 = ((w_p - w_0) * rdc - (w_0 - w_m) * rdm) * rdf;
            const double Gd = -P.d_old * d2;
            const double f = w_0 + P.dtau * P.f_w * Gs_k - Gp - Gb - Gd - fabs(P.dto) * sp * w_0;
            // coefficients of row k
            const double a = -dtn2 * C_m * thf_m * rdm * rdf + dtn2 * g.g * rdm / 2.0 + (-P.d_new * rdm * rdf);
            const double b = 1.0 + (dtn2 * thf_0 * (C_0 * rdc + C_m * rdm) * rdf + dtn2 * g.g * (rdc - rdm) / 2.0 +
                                    P.d_new * (rdc + rdm) * rdf + fabs(P.dtn) * sp);
            t = c_m / beta;
            beta = b - a * t;
            phi = (f - a * phi_m) / beta;
            // upper coefficient of this row, used by the next one
            c_m = -dtn2 * C_0 * thf_p * rdc * rdf + (-dtn2 * g.g * rdc / 2.0) + (-P.d_new * rdc * rdf);
        }
        // ---- every store of the level ----
        if (INIT) ac_st(F.rthp, e, rthp);      // the initial (rho theta)': the next substep's damping and the stage epilogue read it
        if (INIT && !g.wrap_y) {               // y-slab: and its halo rows (the exchange before this sweep carried a buffer nobody had filled)
            if (j == 0) ac_st(F.rthp, e + dym, rt_ym);
            if (j == g.Ny - 1) ac_st(F.rthp, e + dyp, rt_yp);
        }
        ac_st(F.rup, e, up0);
        ac_st(F.rvp, e, vp0);
        if (acc && (FIRST || P.acc_mode != 1)) {
            ac_st(F.au, e, au_n);
            ac_st(F.av, e, av_n);
        }
        ac_st(F.rs, e, rs);
        ac_st(F.rths, e, rths);
        if (FIRST) ac_st(F.tfac, e, t);
        ac_st(F.phi, e, phi);
        phi_m = phi;
        __builtin_amdgcn_s_barrier();      // the rows of a block advance together: a row's y neighbours are requested while their lines are near

        // advance the rings
        rs_m = rs; rths_m = rths; rp_m = rp; rthp_m = rthp;
        C_m = C_0; C_0 = C_n;
        thf_m = thf_0; thf_0 = thf_p;
        th_0 = th_p; th_p = th_n;
        w_m = w_0; w_0 = w_p; w_p = w_n;
        cy_m0 = cy_mn; cy_p0 = cy_pn;
        thy_m0 = thy_m1; thy_p0 = thy_p1; thy_m1 = thy_mn; thy_p1 = thy_pn;
    };
    // two levels per trip so that the two records live in fixed registers (a rotation `current = next` would have to wait for the
    // next level's loads before it could copy them); the last level re-reads itself
    AcLevel LA = level(e, 0), LB;
#pragma unroll 1
    for (int k = 0; k < Nz; k += 2, e += 2 * sz) {
        const int k1 = (k + 1 < Nz) ? k + 1 : k;
        LB = level(e + (unsigned)(k1 - k) * sz, k1);
        work(LA, k, e);
        if (k + 1 < Nz) {
            const int k2 = (k + 2 < Nz) ? k + 2 : k + 1;
            LA = level(e + (unsigned)(k2 - k) * sz, k2);
            work(LB, k + 1, e + sz);
        }
    }
}

// back substitution + _post_solve_recovery! (acoustic_substepping.jl:993-1002)
// INIT (FIRST only; see k_ac_forward2): 1 / 2 — the initial (rho w)' of the held top face is formed here (U0 - U / zero) and stored
template <bool FIRST, class ST, int INIT = 0>      // FIRST: first substep of a stage with the fused forward sweep: <rho w> starts here
__global__ __launch_bounds__(ABX * ABY) void k_ac_column_backward(DevGrid g, AcFieldsT<ST> F, AcParams P)
{
    const int i = blockIdx.x * ABX + threadIdx.x, j = blockIdx.y * ABY + threadIdx.y;
    if (i >= g.Nx || j >= g.Ny) return;
    const long long sz = g.Sxy;
    const int Nz = g.Nz;
    const bool acc = ac_accumulate(P);
    long long n = g.idx(i, j, Nz - 1);
    double w_hi = F.rwp[n + sz];                 // top face: held at its (zero) rewind value
    if (INIT) {
        w_hi = (INIT == 2) ? 0.0 : F.U0_rw[n + sz] - F.rw[n + sz];
        F.rwp[n + sz] = w_hi;
    }
    double th_0 = F.thL[n];                      // theta at cell k
    double thf_hi = th_0;                        // face Nz: one-sided
    double t_hi = 0.0;                           // t_{k+1}
    for (int k = Nz - 1; k >= 0; --k, n -= sz) {
        const double th_m = (k > 0) ? F.thL[n - sz] : th_0;
        const double thf_lo = (k > 0) ? (th_0 + th_m) / 2.0 : th_0;
        double w_lo = F.phi[n];
        if (k < Nz - 1) w_lo -= t_hi * w_hi;
        const double rdc = g.rdzc[k];
        const double dzW = (w_hi - w_lo) * rdc;
        const double dzT = (thf_hi * w_hi - thf_lo * w_lo) * rdc;
        F.rp[n] = F.rs[n] - P.dtn * dzW;
        F.rthp_out[n] = F.rths[n] - P.dtn * dzT;
        // <w> two substeps at a time (AcParams::acc_mode): the second substep of a pair adds (w'_{n-1} + w'_n) with w'_{n-1} read from the field
        // it is about to overwrite (one word instead of the accumulator's two in the pair's first substep)
        const double w_old = (!FIRST && acc && P.acc_mode == 2) ? F.rwp[n] : 0.0;
        F.rwp[n] = w_lo;
        if (acc) {
            if (FIRST) F.aw[n] = 0.0 + w_lo;
            else if (P.acc_mode == 2) F.aw[n] += (w_old + w_lo);
            else if (P.acc_mode == 0) F.aw[n] += w_lo;
        }
        t_hi = F.tfac[n];
        w_hi = w_lo;
        thf_hi = thf_lo;
        th_0 = th_m;
    }
}

// last substep's damping + _finalize_time_averaged_velocity! (acoustic_substepping.jl:1225-1250); writes the periodic
// halo images and z-halo copies of the averaged velocities (they feed WENO stencils of the moisture tendency).
template <bool DAMP, class ST>
__global__ __launch_bounds__(256) void k_ac_finalize(DevGrid g, AcFieldsT<ST> F, AcParams P)
{
    const int i = blockIdx.x * 256 + threadIdx.x, j = blockIdx.y, k = blockIdx.z;
    if (i >= g.Nx) return;
    const WrapIdx W = wrap_of(g, i, j);
    const long long sz = g.Sxy;
    const long long n = g.idx(i, j, k), mx = n + W.im, my = n + W.jm;
    if (DAMP) {
        const double d0 = F.rthp[n] - F.rth_old[n];
        const double ddx = (d0 - (F.rthp[mx] - F.rth_old[mx])) * g.rdx;
        const double ddy = (d0 - (F.rthp[my] - F.rth_old[my])) * g.rdy;
        const double th = F.thL[n];
        double up = F.rup[n] - P.kdamp * ddx / ((th + F.thL[mx]) / 2.0);
        double vp = F.rvp[n] - P.kdamp * ddy / ((th + F.thL[my]) / 2.0);
        if (g.bounded_x && i == 0 && P.wall_w) up = 0.0;
        if (g.bounded_y && j == 0 && P.wall_s) vp = 0.0;
        F.rup[n] = up;
        F.rvp[n] = vp;
    }
    const double r0 = F.rho_d[n];
    double rx = (r0 + F.rho_d[mx]) / 2.0, ry = (r0 + F.rho_d[my]) / 2.0;
    rx = (rx == 0.0) ? 1.0 : rx;
    ry = (ry == 0.0) ? 1.0 : ry;
    const double ua = (F.ru[n] + F.au[n] * P.inv_N) / rx;
    const double va = (F.rv[n] + F.av[n] * P.inv_N) / ry;
    st_img(F.au, n, ua, W.ox, W.oy);
    st_img(F.av, n, va, W.ox, W.oy);
    double wa = 0.0;
    if (k > 0) {
        double rz = (r0 + F.rho_d[n - sz]) / 2.0;
        rz = (rz == 0.0) ? 1.0 : rz;
        wa = (F.rw[n] + F.aw[n] * P.inv_N) / rz;
    }
    st_img(F.aw, n, wa, W.ox, W.oy);
    if (k == 0 || k == g.Nz - 1) {
        const long long h = (k == 0) ? -sz : sz;
        st_img(F.au, n + h, ua, W.ox, W.oy);
        st_img(F.av, n + h, va, W.ox, W.oy);
        if (k == g.Nz - 1) st_img(F.aw, n + sz, 0.0, W.ox, W.oy);
    }
}

// _recover_full_state! (acoustic_substepping.jl:1274-1292) [+ WS-RK3 update of the moisture density,
// acoustic_runge_kutta_3.jl:189-192, when dt_stage_q != 0 pointer-wise]
template <int MOIST, class ST>      // MOIST 0: acoustic prognostics only; 1: + rho q^v; 2: + rho q^v and the Kessler species
__global__ __launch_bounds__(256) void k_ac_recover(DevGrid g, AcFieldsT<ST> F, double dt_stage)
{
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long long)g.Ny * g.Sx) return;
    const int k = blockIdx.y;
    const long long n = g.Sxy * (k + g.Hz) + (long long)g.Hy * g.Sx + t;
    if (g.bounded_x) {      // the halo columns of a Bounded x hold the caller's boundary values of the model fields, not periodic images
        const int c = (int)(t % g.Sx);
        if (c < g.Hx || c >= g.Hx + g.Nx) return;
    }
    F.rho_d[n] = F.rho_d[n] + F.rp[n];
    F.rth[n] = F.rth[n] + F.rthp[n];
    F.ru[n] = F.ru[n] + F.rup[n];
    F.rv[n] = F.rv[n] + F.rvp[n];
    F.rw[n] = F.rw[n] + F.rwp[n];
    if (MOIST) F.rq[n] = F.U0_rq[n] + dt_stage * F.G_rq[n];
    if (MOIST == 2) {
        F.rqcl[n] = F.U0_rqcl[n] + dt_stage * F.G_rqcl[n];
        F.rqr[n] = F.U0_rqr[n] + dt_stage * F.G_rqr[n];
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Stage epilogue of the whole-step seam in ONE pass (round 4): k_ac_finalize + k_ac_recover<MOIST> +
// k_cmp_diagnose<true, LIN, MP> — three passes that re-read each other's output (17 + 18 + 18 words per cell) as one (38) plus the
// three-word density pass below.  Same expressions in the same order as the three kernels, so the results carry their bits:
//   * the last substep's divergence damping of (rho u)', (rho v)' (the damped values are consumed here and not stored: nothing reads
//     the perturbation fields between the recovery and the next stage's initialisation);
//   * time-averaged velocities from the accumulators and the STAGE-ENTRY densities, with their halo images;
//   * recovery U = U^L + U' of rho theta, momentum (stored in place: pointwise) and of rho_d — which is NOT stored here, because the
//     averages above and the velocities below read rho_d of the x / y / z neighbours: every thread forms the neighbours' new density
//     from the old one and rho' itself, and k_ac_recover_density writes the field afterwards;
//   * WS-RK3 update of the moisture density (and the Kessler species);
//   * update_state!: total density, velocities, theta, q, Newton temperature, pressure, every halo image, and (LIN) the next
//     stage's linearisation — theta_L goes to `thL_out`, a second buffer, because the damping of this pass reads the old theta_L
//     of the neighbours (bz_ctx::d_thL2; the stage driver alternates the two).
// Single-device contexts only (a y-slab has no rho' in its halo rows).
template <bool DAMP, bool LIN, int MP, class ST>
__global__ __launch_bounds__(256) void k_ac_stage_end(DevGrid g, AcFieldsT<ST> F, DiagFields D, AcParams P, double dt_stage, ST *__restrict__ thL_out,
                                                      double abstol, int maxiter, const double *fl)
{
    // 3: the FlatauPolynomial instantiation of 1; 4 | 5: the mixed-phase instantiations of 1 | 3 (k_cmp_diagnose)
    constexpr bool KES = (MP == 2), MIX = (MP == 4 || MP == 5), SA = (MP == 1 || MP == 3 || MIX), FL = (MP == 3 || MP == 5);
    int bx, j, k;
    ac_pencil_block(bx, j, k);
    const int i = bx * 256 + threadIdx.x;
    if (i >= g.Nx) return;
    const WrapIdx W = wrap_of(g, i, j);
    const long long ox = W.ox, oy = W.oy;
    const long long sz = g.Sxy;
    const long long n = g.idx(i, j, k), mx = n + W.im, my = n + W.jm, mz = n - sz;
    const bool bot = (k == 0), top = (k == g.Nz - 1);

    // ---- k_ac_finalize: damping of the last substep ----
    ST up_s = F.rup[n], vp_s = F.rvp[n];
    if (DAMP) {
        const double d0 = F.rthp[n] - F.rth_old[n];
        const double ddx = (d0 - (F.rthp[mx] - F.rth_old[mx])) * g.rdx;
        const double ddy = (d0 - (F.rthp[my] - F.rth_old[my])) * g.rdy;
        const double th = F.thL[n];
        up_s -= P.kdamp * ddx / ((th + F.thL[mx]) / 2.0);
        vp_s -= P.kdamp * ddy / ((th + F.thL[my]) / 2.0);
    }
    // ---- k_ac_finalize: time-averaged velocities (stage-entry densities and momentum) ----
    const double r0 = F.rho_d[n], r_mx = F.rho_d[mx], r_my = F.rho_d[my];
    const double ru0 = F.ru[n], rv0 = F.rv[n];
    double r_mz = 0.0, rw0 = 0.0;
    if (!bot) {
        r_mz = F.rho_d[mz];
        rw0 = F.rw[n];
    }
    if (ac_accumulate(P)) {      // (a dry stage 1 / 2 of a whole step carries no accumulators: AcParams::skip_avg_if_dry)
        double rx = (r0 + r_mx) / 2.0, ry = (r0 + r_my) / 2.0;
        rx = (rx == 0.0) ? 1.0 : rx;
        ry = (ry == 0.0) ? 1.0 : ry;
        const double ua = (ru0 + F.au[n] * P.inv_N) / rx;
        const double va = (rv0 + F.av[n] * P.inv_N) / ry;
        st_img(F.au, n, ua, ox, oy);
        st_img(F.av, n, va, ox, oy);
        double wa = 0.0;
        if (!bot) {
            double rz = (r0 + r_mz) / 2.0;
            rz = (rz == 0.0) ? 1.0 : rz;
            wa = (rw0 + F.aw[n] * P.inv_N) / rz;
        }
        st_img(F.aw, n, wa, ox, oy);
        if (bot || top) {
            const long long h = bot ? -sz : sz;
            st_img(F.au, n + h, ua, ox, oy);
            st_img(F.av, n + h, va, ox, oy);
            if (top) st_img(F.aw, n + sz, 0.0, ox, oy);
        }
    }
    // ---- k_ac_recover ----
    const double rd = r0 + F.rp[n];
    const double rth = F.rth[n] + F.rthp[n];
    const double ru = ru0 + up_s, rv = rv0 + vp_s;
    const bool dryq = (MP == 0) && P.dry_q && __builtin_amdgcn_readfirstlane(*P.dry_q) == 1;
    const double rq = dryq ? 0.0 : F.U0_rq[n] + dt_stage * F.G_rq[n];
    double rqcl = 0.0, rqr = 0.0;
    if (KES) {
        rqcl = F.U0_rqcl[n] + dt_stage * F.G_rqcl[n];
        rqr = F.U0_rqr[n] + dt_stage * F.G_rqr[n];
    }
    // ---- k_cmp_diagnose<true, LIN, MP> on the recovered state ----
    const double rdx = (rd + (r_mx + F.rp[mx])) / 2.0;
    const double rdy = (rd + (r_my + F.rp[my])) / 2.0;
    const double u = ru / rdx, v = rv / rdy;
    if (P.out_of_place) st_img(D.rho_d, n, rd, ox, oy);
    st_img(D.rth, n, rth, ox, oy);
    st_img(D.ru, n, ru, ox, oy);
    st_img(D.rv, n, rv, ox, oy);
    st_img(D.u, n, u, ox, oy);
    st_img(D.v, n, v, ox, oy);
    if (!bot) {
        const double rw = rw0 + F.rwp[n];
        const double rdz = (rd + (r_mz + F.rp[mz])) / 2.0;
        st_img(D.rw, n, rw, ox, oy);
        st_img(D.w, n, rw / rdz, ox, oy);
    } else {
        st_img(D.rw, n, 0.0, ox, oy);      // impenetrable walls
        st_img(D.w, n, 0.0, ox, oy);
    }
    if (top) {
        st_img(D.rw, n + sz, 0.0, ox, oy);
        st_img(D.w, n + sz, 0.0, ox, oy);
    }
    double r, q, th, T, p, qcl_v = 0.0, qr_v = 0.0, sa_qv = 0.0, sa_ql = 0.0, sa_qi = 0.0;
    {
        double ql = 0.0;
        if (KES) r = rd + (rq + (rqcl + (rqr + 0.0)));
        else r = rd + (rq + 0.0);
        th = rth / rd;
        q = rq / r;
        if (KES) {
            qcl_v = rqcl / r;
            qr_v = rqr / r;
            ql = qcl_v + qr_v;
        }
        double qvap = q;
        if constexpr (MIX) {
            T = bz_ds_adjust_mixed<FL>(g, th, q, r, abstol, maxiter, qvap, ql, sa_qi, ColPtr(fl));
            st_img(g.qv_field, n, qvap, ox, oy);
            st_img(g.ql_field, n, ql, ox, oy);
            st_img(g.qi_field, n, sa_qi, ox, oy);
            sa_qv = qvap; sa_ql = ql;
        } else if (SA) {
            T = bz_ds_adjust<FL>(g, th, q, r, abstol, maxiter, qvap, ql, ColPtr(fl));
            st_img(g.qv_field, n, qvap, ox, oy);
            st_img(g.ql_field, n, ql, ox, oy);
            sa_qv = qvap; sa_ql = ql;
        }
        const double qd = MIX ? 1.0 - (qvap + ql + sa_qi) : 1.0 - (qvap + ql);
        const double Rm = qd * g.Rd + qvap * g.Rv;
        const double cpm = MIX ? qd * g.cpd + qvap * g.cpv + ql * g.sa_cl + sa_qi * g.sa_ci
                               : (KES || SA) ? qd * g.cpd + qvap * g.cpv + ql * g.sa_cl : qd * g.cpd + qvap * g.cpv;
        if (!SA) {
            const double kap = Rm / cpm;
            const double gam = cpm / (cpm - Rm);
            const double Lt = KES ? (g.sa_Ll * ql) / cpm : 0.0;
            T = pow(th, gam) * pow(r * Rm / g.pst, gam - 1.0) + Lt;
            double dT = T;
            for (int it = 0; it < maxiter && fabs(dT) > abstol; ++it) {
                const double Phi = pow(r * Rm * T / g.pst, kap) * th;
                dT = -(T - Phi - Lt) / (1.0 - kap * Phi / T);
                T += dT;
            }
        }
        p = r * Rm * T;
        if (KES) {
            st_img(F.rqcl, n, rqcl, ox, oy);
            st_img(F.rqr, n, rqr, ox, oy);
            st_img(g.qcl_field, n, qcl_v, ox, oy);
            st_img(g.qr_field, n, qr_v, ox, oy);
            st_img(g.qv_field, n, q, ox, oy);
        }
        if (!dryq || P.out_of_place) st_img(D.rq, n, rq, ox, oy);
        st_img(D.rho, n, r, ox, oy);
        st_img(D.theta, n, th, ox, oy);
        if (!dryq) st_img(D.q, n, q, ox, oy);
        st_img(D.T, n, T, ox, oy);
        st_img(D.p, n, p, ox, oy);
        if (LIN) {
            const double Pi = pow(p / g.pst, g.Rd / g.cpd);
            const double thl = rth / ((rd == 0.0) ? 1.0 : rd);
            const double gr = cpm * Rm / (cpm - Rm);
            st_store(D.Pi, n, Pi, D.st32);
            thL_out[n] = (ST)thl;
            st_store(D.gR, n, gr, D.st32);
            st_store(D.Clin, n, gr * Pi, D.st32);
        }
    }
    if (bot || top) {     // first z-halo cell of the no-flux centre fields (rho_d: k_ac_recover_density)
        const long long h = bot ? -sz : sz;
        if (P.out_of_place) st_img(D.rho_d, n + h, rd, ox, oy);
        st_img(D.ru, n + h, ru, ox, oy);
        st_img(D.rv, n + h, rv, ox, oy);
        st_img(D.rth, n + h, rth, ox, oy);
        st_img(D.u, n + h, u, ox, oy);
        st_img(D.v, n + h, v, ox, oy);
        if (!dryq || P.out_of_place) st_img(D.rq, n + h, rq, ox, oy);
        st_img(D.rho, n + h, r, ox, oy);
        st_img(D.theta, n + h, th, ox, oy);
        if (!dryq) st_img(D.q, n + h, q, ox, oy);
        st_img(D.T, n + h, T, ox, oy);
        st_img(D.p, n + h, p, ox, oy);
        if (SA) {
            st_img(g.qv_field, n + h, sa_qv, ox, oy);
            st_img(g.ql_field, n + h, sa_ql, ox, oy);
        }
        if constexpr (MIX) st_img(g.qi_field, n + h, sa_qi, ox, oy);
        if (KES) {
            st_img(F.rqcl, n + h, rqcl, ox, oy);
            st_img(F.rqr, n + h, rqr, ox, oy);
            st_img(g.qcl_field, n + h, qcl_v, ox, oy);
            st_img(g.qr_field, n + h, qr_v, ox, oy);
            st_img(g.qv_field, n + h, q, ox, oy);
        }
    }
}

// rho_d = rho_d^L + rho' with its halo images and z-halo copies: the one field of the recovery whose neighbours k_ac_stage_end reads
template <class ST>
__global__ __launch_bounds__(256) void k_ac_recover_density(DevGrid g, double *__restrict__ rho_d, const ST *__restrict__ rp)
{
    const int i = blockIdx.x * 256 + threadIdx.x, j = blockIdx.y, k = blockIdx.z;
    if (i >= g.Nx) return;
    const WrapIdx W = wrap_of(g, i, j);
    const long long n = g.idx(i, j, k);
    const double rd = rho_d[n] + rp[n];
    st_img(rho_d, n, rd, W.ox, W.oy);
    if (k == 0 || k == g.Nz - 1) st_img(rho_d, n + ((k == 0) ? -g.Sxy : g.Sxy), rd, W.ox, W.oy);
}

// apply_divergence_damping!(::DirectDivergenceDamping) (acoustic_substepping.jl:1158-1188): delta = V^-1 (dx(thetaF^x) + dy(thetaF^y))
// into the density predictor (free between recovery and the next predictor build), then the theta_L-scaled gradient of delta onto the
// horizontal momentum perturbations.  Periodic neighbours by wrap indexing: no halo fill of delta, (rho u)', (rho v)' or theta_L.
// y-slabs (wrap_y == 0): the neighbours are halo rows — theta_L is linearised on one halo row each side, (rho u)' and (rho v)' are
// exchanged by the driver between the column solve and this pair (bz_acoustic_direct_damping) — and delta is evaluated from row -1
// (jofs = -1, Ny + 1 rows) so that the gradient at row 0 needs no exchange of its own.
__global__ __launch_bounds__(256) void k_ac_direct_delta(DevGrid g, double *__restrict__ delta, const double *__restrict__ thL,
                                                         const double *__restrict__ up, const double *__restrict__ vp, int jofs)
{
    const int i = blockIdx.x * 256 + threadIdx.x, j = (int)blockIdx.y + jofs, k = blockIdx.z;
    if (i >= g.Nx) return;
    const long long n = g.idx(i, j, k);
    const long long ip = (i + 1 < g.Nx || g.bounded_x) ? 1 : 1 - g.Nx, im = (i > 0 || g.bounded_x) ? -1 : g.Nx - 1;
    const long long jp = (j + 1 < g.Ny || !g.wrap_y) ? (long long)g.Sx : (long long)g.Sx * (1 - g.Ny);
    const long long jm = (j > 0 || !g.wrap_y) ? -(long long)g.Sx : (long long)g.Sx * (g.Ny - 1);
    const double Ax = g.Ax[k], Ay = g.Ay[k];
    // Bounded directions: the east / north wall face is an exact zero (AcParams::wall_w); the west / south one holds the value the substep stored
    const double up1 = (g.bounded_x && i == g.Nx - 1) ? 0.0 : up[n + ip], vp1 = (g.bounded_y && j == g.Ny - 1) ? 0.0 : vp[n + jp];
    const double fx = Ax * ((thL[n + ip] + thL[n]) / 2.0) * up1 - Ax * ((thL[n] + thL[n + im]) / 2.0) * up[n];
    const double fy = Ay * ((thL[n + jp] + thL[n]) / 2.0) * vp1 - Ay * ((thL[n] + thL[n + jm]) / 2.0) * vp[n];
    delta[n] = (fx + fy) * g.Vinv_c[k];
}
__global__ __launch_bounds__(256) void k_ac_direct_apply(DevGrid g, const double *__restrict__ delta, const double *__restrict__ thL,
                                                         double *__restrict__ up, double *__restrict__ vp, double alpha, int wall_w, int wall_s)
{
    const int i = blockIdx.x * 256 + threadIdx.x, j = blockIdx.y, k = blockIdx.z;
    if (i >= g.Nx) return;
    const long long n = g.idx(i, j, k);
    const long long im = (i > 0 || g.bounded_x) ? -1 : g.Nx - 1;
    const long long jm = (j > 0 || !g.wrap_y) ? -(long long)g.Sx : (long long)g.Sx * (g.Ny - 1);
    double u1 = up[n] + alpha * (g.dx * g.dx) * ((delta[n] - delta[n + im]) * g.rdx) / ((thL[n] + thL[n + im]) / 2.0);
    double v1 = vp[n] + alpha * (g.dy * g.dy) * ((delta[n] - delta[n + jm]) * g.rdy) / ((thL[n] + thL[n + jm]) / 2.0);
    if (g.bounded_x && i == 0 && wall_w) u1 = 0.0;      // enforce_wall_impenetrability! after the damping (acoustic_substepping.jl:1547-1550)
    if (g.bounded_y && j == 0 && wall_s) v1 = 0.0;
    up[n] = u1;
    vp[n] = v1;
}

// ---------------------------------------------------------------------------------------------------------------------
// Lateral boundaries of the acoustic loop (round 6): topologies with a Bounded x and / or y.
// The substepper's own fields carry the default boundary conditions of their location (acoustic_substepping.jl:207-231; the test
// test/acoustic_substepping_open_boundaries.jl:70-73 pins that the momentum perturbations do not inherit the model's): a field that is a
// centre along a Bounded direction gets a zero-gradient halo from fill_halo_regions!, the wall faces of a face field are not touched by it.
// k_ac_fill_walls is that fill for the one halo row / column the substep kernels read (the kernels reach neighbours through halo cells on
// Bounded directions: wrap_of); the model's own fields (rho_d, rho theta, p, the slow tendencies) keep the halos the caller's boundary
// conditions gave them.
// ---------------------------------------------------------------------------------------------------------------------
template <class T>
__global__ __launch_bounds__(256) void k_ac_fill_walls(DevGrid g, T *__restrict__ f)
{
    const int t = blockIdx.x * 256 + threadIdx.x, k = blockIdx.y;
    const int ny_rows = g.bounded_y ? 2 * g.Nx : 0, nx_cols = g.bounded_x ? 2 * g.Ny : 0;
    if (t < ny_rows) {
        const int side = t / g.Nx, i = t - side * g.Nx;
        f[g.idx(i, side ? g.Ny : -1, k)] = f[g.idx(i, side ? g.Ny - 1 : 0, k)];
    } else if (t - ny_rows < nx_cols) {
        const int u = t - ny_rows, side = u / g.Ny, j = u - side * g.Ny;
        f[g.idx(side ? g.Nx : -1, j, k)] = f[g.idx(side ? g.Nx - 1 : 0, j, k)];
    }
}

// _relax_open_boundary_x! / _relax_open_boundary_y! (acoustic_substepping.jl:1323-1337): the outermost cell of rho' and (rho theta)' is pulled
// towards the prescribed wall value v; the model's Value boundary condition left rho^L[halo] = 2 v - rho^L[cell], so the target perturbation
// v - rho^L[cell] is (rho^L[halo] - rho^L[cell]) / 2.  One launch per open side: dir 0 = a y-z plane (cell column cb, halo column ch), 1 = an x-z plane.
template <class ST>
__global__ __launch_bounds__(256) void k_ac_relax_open_boundary(DevGrid g, ST *__restrict__ rp, ST *__restrict__ rthp, const double *__restrict__ rho_d,
                                                                const double *__restrict__ rth, int dir, int cb, int ch, double alpha)
{
    const int t = blockIdx.x * 256 + threadIdx.x, k = blockIdx.y;
    if (t >= (dir ? g.Nx : g.Ny)) return;
    const long long nb = dir ? g.idx(t, cb, k) : g.idx(cb, t, k), nh = dir ? g.idx(t, ch, k) : g.idx(ch, t, k);
    const double r = rp[nb], q = rthp[nb];
    rp[nb] = r + alpha * ((rho_d[nh] - rho_d[nb]) / 2.0 - r);
    rthp[nb] = q + alpha * ((rth[nh] - rth[nb]) / 2.0 - q);
}
