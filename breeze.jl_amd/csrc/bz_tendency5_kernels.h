// bz_tendency5_kernels.h — "lean" tendency kernels of the whole-step seam (fifth generation).
//
// What changed against generation 4 (bz_tendency4_kernels.h) and why (PMC of the gen-4 kernels in
// profiles/r02_pmc_gen4_sq.json: 61-68 % of wave cycles parked in s_waitcnt, 13 % VALU-active):
//   * the kernels read the PROGNOSTIC fields only.  In the anelastic model u, v, w, theta, q^v are the prognostic densities
//     divided by a column constant (update_atmosphere_model_state.jl:122-155,256-292), so they are derived on the fly with
//     bz_cdiv (correctly rounded: bit-identical to the stored diagnostics) instead of being written by the projection kernel
//     and read back: no u, v, w, theta, q arrays on the hot path, and the projection kernel of stages 1-2 shrinks to the
//     momentum update.  T enters only through the buoyancy and is rebuilt from rho theta, rho q in the w kernel.
//   * rho theta / rho q advance through a ping-pong pair (stage input -> stage output) because the stencils now read the
//     array the RK update writes; the kernel stores the periodic halo images of what it produces.
//   * XCD-contiguous block order (bz_block5): the y-frame rows a tile stages are its neighbour tiles' interior rows; with
//     round-robin dispatch those neighbours run on other XCDs and every L2 fetches the rows again.
// Same fluxes, same order of floating-point operations as generation 4 (and as the oracle); reference semantics:
// src/Advection.jl:20-35, src/AtmosphereModels/dynamics_kernel_functions.jl:54-159,
// src/AnelasticEquations/anelastic_buoyancy.jl:36-72, src/TimeSteppers/ssp_runge_kutta_3.jl:167-173 (paths under /root/reference).
#pragma once
#include "bz_internal.h"
#include "bz_weno.h"
#include "bz_tendency4_kernels.h"      // Tend3Fields, adv_x / adv_y, hflux, flux_x_at, vflux, buoyancy3

// element index type of the momentum kernels: 64-bit, so that the +-1, +-2, +-3 neighbours of a row fold into the immediate offset
// of one address per array and level (with 32-bit unsigned indices every neighbour costs its own address arithmetic: measured
// +10 % on the x-momentum kernel); the scalar-pair kernel keeps 32-bit indices, which is what lets it fit 128 VGPRs
typedef long long ix_t;
typedef unsigned ix32_t;     // z-momentum kernel: 32-bit (138 -> 121 VGPRs, 3 -> 4 waves per SIMD; measured 3.61 -> 2.94 ms)

// Column constants of one level, packed: the scalar-pair kernel reads eleven column-table entries per level; as separate tables that
// is eleven address computations + s_loads and 22 SGPRs of pointers (the kernel spilled 44 SGPRs to VGPR lanes: ~50 v_readlane per
// level); as one row it is one s_load_dwordx16 (+ two narrow ones for the levels above).  Built on the device from the same tables
// (k_lev_rows, bz_tendency5.hip), so every value carries the bits the separate tables hold.
struct LevRow5 {
    double rho, rrho;        // rho_r[k] and its correctly rounded reciprocal
    double rho_f, rrho_f;    // the same at the lower face of level k
    double Ax, Ay, Vinv_c;
    double pi;               // dry Exner factor (p_r[k]/p_st)^(Rd/cpd)
    double Vinv_f, T_r;      // round 4 (z-momentum kernel): 1 / V at the lower face, reference temperature
    double pad[6];           // rows of 128 bytes
};
// row access through the constant address space, field by field (adjacent fields merge into one wide s_load)
struct Lev5 {
    const LevRow5 *p;
#ifdef __HIPCC__
    __device__ __forceinline__ double at(int k, int f) const { return ((ColPtr::cptr)(const double *)p)[(long long)k * 16 + f]; }
    __device__ __forceinline__ double rho(int k) const { return at(k, 0); }
    __device__ __forceinline__ double rrho(int k) const { return at(k, 1); }
    __device__ __forceinline__ double rho_f(int k) const { return at(k, 2); }
    __device__ __forceinline__ double rrho_f(int k) const { return at(k, 3); }
    __device__ __forceinline__ double Ax(int k) const { return at(k, 4); }
    __device__ __forceinline__ double Ay(int k) const { return at(k, 5); }
    __device__ __forceinline__ double Vinv_c(int k) const { return at(k, 6); }
    __device__ __forceinline__ double pi(int k) const { return at(k, 7); }
    __device__ __forceinline__ double Vinv_f(int k) const { return at(k, 8); }
    __device__ __forceinline__ double T_r(int k) const { return at(k, 9); }
#endif
};
static_assert(sizeof(LevRow5) == 16 * sizeof(double), "LevRow5 is sixteen reals");

// Waves per SIMD the lean kernels are compiled for: 4 in Float64 (two 512-thread workgroups per CU, <= 128 VGPRs), 6 in the Float32
// build (three workgroups, <= 80 VGPRs: a Float32 value is one register, and the Float32 kernels sat at 84-85 — allocated as 88,
// i.e. five waves per SIMD = still two workgroups).  Measured at 512^3 Float32: scalar-pair kernel 2.04 -> 1.88 ms with three spilled
// registers; the z-momentum kernel and the forcing variant of the y-momentum kernel spill eight and lose 7-13 %, so they keep the default.
#define BZ_LEAN_WAVES (sizeof(double) == 8 ? 4 : 6)
// Round-4 additions to the scalar-pair kernel — the zero-field shortcut of the second scalar and ring tops requested one level ahead —
// cost ~8 registers.  The Float32 kernel sat at 80 registers for six waves per SIMD: with the additions it spilled (19 registers,
// 1.78 -> 2.48 ms per launch at 512^3; the shortcut alone 2.25), so the Float32 scalar kernel is compiled for four waves per SIMD
// instead (two workgroups per CU, as Float64) with both additions on: 1.47 ms (four waves without them: 1.85).  The momentum kernels
// keep BZ_LEAN_WAVES.
// (later in round 4 the Float32 objects lost the SLP vectoriser — csrc/Makefile: F32FLAGS — and with it the operand-pair moves: the Float32
// scalar kernel needs 75 - 80 registers with both additions and runs at six waves again: 0.97 -> 0.92 ms per launch in its dry form)
#define BZ5_SCALAR_WAVES (sizeof(double) == 8 ? 4 : 6)
#define BZ6_W_WAVES 4           // the z-momentum kernel, both precisions
constexpr int BZ5_EB = 64;      // levels per batch of the out-of-wave x flux (lane l <-> level k + l): a power of two <= 64
// Decided experiments of the momentum kernels' level loop (HISTORY.md has the figures): the per-level barrier is __syncthreads() — an
// LDS-scoped release / s_barrier / acquire bought nothing —, the top-row duty flux stays with wave 0 (rotated over the waves: +2 %), and the
// loop is not unrolled by two.

struct Lean5 {
    const double *ru, *rv, *rw;      // stage-start momentum (halos valid)
    const double *pa, *pb;           // stage-start rho theta, rho q (halos valid)
    double *out;                     // momentum kernels: predictor momentum (the G slot of the component)
    double *oa, *ob;                 // scalar kernel: updated rho theta, rho q (the other buffer of the ping-pong pair)
    double *T;                       // temperature of the stage-start state (w kernel: read; scalar kernel: writes the updated one)
    ColPtr pi_dry;                   // (p_r[k]/p_st)^(Rd/cpd) indexed by level, or nullptr
    const LevRow5 *lev;              // the column constants of a level packed in one 64-byte row (indexed by level, -Hz .. Nz+Hz-1)
    // momentum terms of a forcing stack folded into the RK epilogue of k6_u / k6_v (bz_step.hip: lean seam with bzi_lean_forcings_ok):
    // f-plane Coriolis f * (4-point average of the other momentum component) and the specific u / v profiles times rho_r (geostrophic
    // forcing).  mforce: 0 none, else bit 0 Coriolis, bit 1 Fu, bit 2 Fv.  Terms and order as k_apply_forcings (bz_forcing.hip).
    int mforce;
    double cor_f;
    ColPtr Fu, Fv;
    ColPtr Su, Sv;                   // mforce bits 3 / 4: subsidence profiles of u / v (per-stage column data: -<w_s dz(avg)>, bz_forcing.hip: k_subsidence_profiles),
                                     // added before the static profile as k_apply_forcings' column() does (fused-RK tier with the stored-velocity kernels)
    // ST instantiations of k6_u / k6_v / k6_w (round 5): the advected velocity is a STORED field (the fused-RK tier of models the lean seam does
    // not cover — saturation adjustment, closures, tracers, forcing stacks —, the per-operator entry points, and the slow tendencies of the
    // compressible model, where rho is a 3-D field and nothing can be derived from a column constant): vel = u | v | w of the component,
    // bT / bq = the buoyancy inputs of the z-momentum kernel (T and q; pressure and total density in the compressible form)
    const double *vel, *bT, *bq;
    const int *qstate;               // moisture scan (bz_moisture.hip: bzi_scan_moisture): *qstate == 1 <=> rho q is identically zero; nullptr: not known
    int xcd;                         // 1: XCD-contiguous block order (grid size divisible by 8)
    int by0, bys;                    // tile row of block row b is by0 + b * bys (sub-launches of the slab driver: interior rows
                                     // while the y-halo exchange is in flight, then the two edge rows)
};

// Hardware deals consecutive workgroup ids round-robin to the 8 XCDs; give XCD c the contiguous range
// [c W/8, (c+1) W/8) of logical tiles (x fastest, then y, then z chunk) so that y-adjacent tiles share an L2.
__device__ __forceinline__ void bz_block5(const Lean5 &L, int &bx, int &by, int &bz)
{
    bx = blockIdx.x; by = blockIdx.y; bz = blockIdx.z;
    if (L.xcd) {
        const unsigned gx = gridDim.x, gy = gridDim.y;
        const unsigned W = gx * gy * gridDim.z;
        unsigned w = bx + gx * (by + gy * bz);
        w = (w & 7u) * (W >> 3) + (w >> 3);
        bx = (int)(w % gx);
        by = (int)((w / gx) % gy);
        bz = (int)(w / (gx * gy));
    }
    by = L.by0 + by * L.bys;
    // the divisions above run on the vector ALU; tell the compiler the results are wave-uniform, otherwise the level index lives in
    // a VGPR and every column-table read (g.rho[k], g.Ax[k], ...) becomes a vector load with its own s_waitcnt instead of an s_load
    bx = __builtin_amdgcn_readfirstlane(bx);
    by = __builtin_amdgcn_readfirstlane(by);
    bz = __builtin_amdgcn_readfirstlane(bz);
}

// store v at n and at its periodic images (ox / oy = element offset of the x / y image, 0 if none)
__device__ __forceinline__ void st_img5(double *__restrict__ f, long long n, double v, long long ox, long long oy)
{
    f[n] = v;
    if (ox) f[n + ox] = v;
    if (oy) {
        f[n + oy] = v;
        if (ox) f[n + ox + oy] = v;
    }
}


// T = Pi^(Rm/cpm) theta of a cell from its prognostic densities: the expressions of k_project_diagnose<0> (bz_fused.hip), so
// the field carries the same bits as the one the full diagnosis writes.  When every lane of the wave is dry the Exner factor of
// the level comes from a table built on the device with the same pow().
// Moist wavefronts: bz_exner_factor (bz_internal.h) — one exp() of a small argument on the level's tabulated dry factor and ln Pi instead
// of the pow() round 4 kept behind a call (its extended-precision log + exp cost the z-momentum kernel 0.8 ms per launch at 512^3).
__device__ __forceinline__ double bz_temperature5(const DevGrid &g, double rth, double rq, int k, const ColPtr pi_dry)
{
    const double rho = g.rho[k], rrho = g.rrho[k];
    const double th = bz_cdiv(rth, rho, rrho), q = bz_cdiv(rq, rho, rrho);
    if (pi_dry.p && __all(q == 0.0)) return pi_dry[k] * th;
    const double qd = 1.0 - q;
    const double cpm = qd * g.cpd + q * g.cpv;
    return bz_exner_factor(g, k, q, cpm) * th;
}

// the same with the level's constants already in registers (LevRow5)
__device__ __forceinline__ double bz_temperature5r(const DevGrid &g, double rth, double rq, int k, double rho, double rrho, double pi)
{
    const double th = bz_cdiv(rth, rho, rrho), q = bz_cdiv(rq, rho, rrho);
    if (__all(q == 0.0)) return pi * th;
    const double qd = 1.0 - q;
    const double cpm = qd * g.cpd + q * g.cpv;
    return bz_exner_factor(g, k, q, cpm) * th;
}

// Walls in y (topology (Periodic, Bounded, Bounded)): WY instantiations of the four kernels reconstruct in y with the buffer that fits
// at the row (wave-uniform: a wavefront is one row of the tile) and interpolate the advecting mass flux with the matching Centered order,
// exactly as the per-operator kernels do (bz_tendency.hip: by_face, by_center, symm_y).  WY = false compiles to the code it replaced.
template <bool WY> __device__ __forceinline__ int by5_face(const DevGrid &g, int j) { return WY ? bz_buffer_face(j, g.Ny) : 3; }
template <bool WY> __device__ __forceinline__ int by5_center(const DevGrid &g, int j) { return WY ? bz_buffer_center(j, g.Ny) : 3; }
template <bool WY>
__device__ __forceinline__ double bz_up5y(double m3, double m2, double m1, double p0, double p1, double p2, bool left, int B)
{
    if constexpr (WY) return bz_upB(m3, m2, m1, p0, p1, p2, left, B);
    else return bz_up5(m3, m2, m1, p0, p1, p2, left);
}
template <bool WY>
__device__ __forceinline__ double bz_symm4y(double qm2, double qm1, double q0, double qp1, int B)
{
    if constexpr (WY) return (B == 3) ? bz_symm4(qm2, qm1, q0, qp1) : bz_symm2(qm1, q0);
    else return bz_symm4(qm2, qm1, q0, qp1);
}

// ---------------------------------------------------------------------------------------------------------------------
// rho theta + rho q: tendencies -div_rhoUc(theta), -div_rhoUc(q) and their SSP-RK3 update, from rho u, rho v, rho w,
// rho theta, rho q alone.  Structure of k_scalar_pair_lds: 64 x TY tile marching in z, (TY+6) x 70 frame of theta and q in LDS
// (double-buffered, frame cells prefetched one level ahead), y-face fluxes shared through LDS, x-face fluxes through a wave
// shuffle + the batched out-of-wave flux, z stencils in register rings.
// ---------------------------------------------------------------------------------------------------------------------
// DRYQ: the second scalar is identically zero in the whole field (Lean5::qstate, set by the scan that opens every step call:
// bz_moisture.hip: bzi_scan_moisture) — rho q of a dry run, which the reference advects all the same
// (update_atmosphere_model_state.jl:333-343).  Every flux of it is an exact zero and its update is 0 -> 0, so the instantiation
// neither loads nor stores anything of q: 4.6 of the kernel's 13 words per cell.  Identical bits: the arrays stay zero.
template <int TY, bool WY, bool DRYQ>
__device__ __forceinline__ void k5_scalar_pair_body(const DevGrid &g, const Lean5 &F, int kchunk, const RKEpilogue &E, double *Tp, double *FYp, int *ZF)
{
    constexpr bool Q = !DRYQ;
    constexpr int TR = TY + 6, TC = 72;                 // tile rows, padded row length (70 used)
    constexpr int NHALO = TR * 70 - TY * 64;            // frame cells per field
    constexpr int NT = 64 * TY;
    constexpr int HPT = (NHALO + NT - 1) / NT;          // frame cells per thread
    double(*T)[2][TR][TC] = (double(*)[2][TR][TC])Tp;                  // T[2][2][TR][TC]
    double(*FY)[2][TY + 1][64] = (double(*)[2][TY + 1][64])FYp;        // FY[2][2][TY + 1][64]
    // General body: the RK update re-reads the cell's own prognostic values.  Carrying them in per-thread LDS slots instead moved 1.6 GB
    // less per launch and was 1.5 % faster on one box, 4 % slower on another, so they are re-read.
    // Zero-field shortcut of the second scalar (rho q of a dry run is identically zero, and the reference advects it all the same:
    // update_atmosphere_model_state.jl:333-343).  ZF[l % 3] != 0: every staged value of q at level l — the tile and its frame — is +-0.
    // Then the x / y reconstructions of that level return exactly 0 (WENO of zeros; every variant of bz_weno5) and the fluxes are
    // exact zeros: the kernel stores 0.0 instead of evaluating them.  The vertical flux takes the same shortcut per wavefront from a
    // per-thread count of consecutive zero ring tops.  Identical bits either way (the sums of +-0 fluxes the RK update sees are +0 with
    // or without the shortcut, and alpha (0 + dt * -0) = +0); costs ~8 instructions per level where q is not zero, saves three
    // reconstructions (~150) where it is.  (ZF: three ints of the caller's LDS; this local form still serves fields that are zero only in part.)
    constexpr bool ZS = Q;

    int bx, by, bz;
    bz_block5(F, bx, by, bz);
    const int tx = threadIdx.x, ty = threadIdx.y, t = ty * 64 + tx;
    const int tyu = __builtin_amdgcn_readfirstlane(ty);      // one tile row per wavefront: wave-uniform, kept in an SGPR for the duty tests below
    const Lev5 LV{F.lev};
    const int i0 = bx * 64, j0 = by * TY;
    const int i = i0 + tx, j = j0 + ty;
    const int ic = min(i, g.Nx + 2), jc = min(j, g.Ny + 2);
    const int nact = min(64, g.Nx - i0);
    const int ie = i0 + nact, le = nact - 1;
    const int kbeg = bz * kchunk, kend = min(kbeg + kchunk, g.Nz);
    if (kbeg >= kend) return;                           // block-uniform
    const int Byj = by5_face<WY>(g, j0 + tyu), Byt = by5_face<WY>(g, j0 + TY);      // y buffers of the own low face and of the face above the tile
    const unsigned sz = (unsigned)g.Sxy;      // 32-bit element indices: the context checks that a parent array holds < 2^32 elements
    const bool store = (i < g.Nx) && (j < g.Ny);
    const double *__restrict__ ru = F.ru, *__restrict__ rv = F.rv, *__restrict__ rw = F.rw;
    const double *__restrict__ pa = F.pa, *__restrict__ pb = F.pb;
    unsigned n = (unsigned)g.idx(ic, jc, kbeg);

    int hr[HPT], hc[HPT];
    unsigned hn[HPT];
    bool hok[HPT];
#pragma unroll
    for (int q = 0; q < HPT; ++q) {
        const int h = t + q * NT;
        hok[q] = h < NHALO;
        int r, c;
        if (h < 6 * 70) {                               // three rows below and three above the tile, full width
            const int rr = h / 70;
            c = h - rr * 70;
            r = (rr < 3) ? rr : TY + rr;
        } else {                                        // side columns of the TY interior rows
            const int hh = h - 6 * 70;
            const int rr = hh / 6, cc = hh - rr * 6;
            r = 3 + rr;
            c = (cc < 3) ? cc : 64 + cc;
        }
        if (!hok[q]) { r = 0; c = 0; }
        hr[q] = r; hc[q] = c;
        const int gi = min(i0 - 3 + c, g.Nx + 2), gj = min(j0 - 3 + r, g.Ny + 2);
        hn[q] = (unsigned)g.idx(gi, gj, kbeg);
    }
    const unsigned ntop0 = (unsigned)g.idx(ic, min(j0 + TY, g.Ny), kbeg);

    // vertical rings of theta, q
    double a[6], b[6];
    // DRYQ: the registers the second scalar would take hold the own column's RAW rho theta of levels k .. k + 2, so that the RK update
    // finds its own cell without the re-read the general path does three levels after the value arrived as ring top (one word per cell
    // out of the Infinity Cache)
    double araw[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int s = 0; s < 6; ++s) {
        const double rh = g.rho[kbeg + s - 3], rr = g.rrho[kbeg + s - 3];
        const double raw = pa[n + s * sz - 3 * sz];
        a[s] = bz_cdiv(raw, rh, rr);
        if (DRYQ && s >= 3) araw[s - 3] = raw;
        if constexpr (Q) {
            const double rawb = pb[n + s * sz - 3 * sz];
            b[s] = bz_cdiv(rawb, rh, rr);
        } else b[s] = 0.0;
    }
    double fza, fzb = 0.0;
    {
        const double wt = bz_cdiv(rw[n], g.rho_f[kbeg], g.rrho_f[kbeg]);
        const bool left = wt > 0.0;
        const int B = bz_buffer_face(kbeg, g.Nz);
        const double cf = g.Az * wt, rf = g.rho_f[kbeg];
        fza = rf * (cf * bz_upB(a[0], a[1], a[2], a[3], a[4], a[5], left, B));
        if constexpr (Q) fzb = rf * (cf * bz_upB(b[0], b[1], b[2], b[3], b[4], b[5], left, B));
    }
    // consecutive zero values of q at the top of the own column's ring (saturates; 6 = the whole ring)
    int zrun = 0;
    if constexpr (ZS) {
#pragma unroll
        for (int s = 0; s < 6; ++s) zrun = (b[s] == 0.0) ? zrun + 1 : 0;
        if (t < 3) ZF[t] = 1;
        __syncthreads();
    }
    T[0][0][ty + 3][tx + 3] = a[3];
    if constexpr (Q) T[0][1][ty + 3][tx + 3] = b[3];
    {
        const double rh = g.rho[kbeg], rr = g.rrho[kbeg];
        bool z0 = (b[3] == 0.0);
#pragma unroll
        for (int q = 0; q < HPT; ++q)
            if (hok[q]) {
                T[0][0][hr[q]][hc[q]] = bz_cdiv(pa[hn[q]], rh, rr);
                if constexpr (Q) {
                    const double hbv = bz_cdiv(pb[hn[q]], rh, rr);
                    T[0][1][hr[q]][hc[q]] = hbv;
                    z0 = z0 && (hbv == 0.0);
                }
            }
        if (ZS && !__all(z0) && tx == 0) ZF[0] = 0;
    }
    __syncthreads();

    double ea = 0.0, eb = 0.0;
    int buf = 0;
    // the level's own momentum elements arrive one level ahead (software pipeline: the advecting fluxes are the first thing a level
    // computes, so loads issued at its top were waited for at once — a full memory latency per level and wave)
    double ru_n = ru[n], rv_n = rv[n], rw_n = rw[n + sz];
    double rvtop_n = (tyu == 0 || (Q && tyu == TY / 2)) ? rv[ntop0] : 0.0;      // top-face duties of the first level: rows 0 and TY / 2
    // ring tops arrive one level ahead as well: they are consumed mid-level (vertical flux), and a load issued at the top of its own
    // level sits behind the previous level's stores in the in-order memory counter
    double ta_nx = pa[n + 3 * sz], tb_nx = 0.0;
    if constexpr (Q) tb_nx = pb[n + 3 * sz];
    for (int k = kbeg; k < kend; ++k, n += sz) {
        // ---- loads, issued in the order their values are needed (s_waitcnt counts vector loads in order, so waiting for a load
        //      waits for everything issued before it): ring tops (vertical flux, mid-level), next level's frame cells (staging, end of
        //      the level), U0 (RK update, very end), and last what only the NEXT level reads — its own momentum elements and the
        //      velocity row of its top-face duty (round 2 loaded those at the top of the level that used them: a full memory
        //      latency per level and wave, because the advecting fluxes are the first thing a level computes) ----
        double ha[HPT], hb[HPT];
        const unsigned lev = (unsigned)(k + 1 - kbeg) * sz;
        const double ta_raw = ta_nx, tb_raw = tb_nx;
        const unsigned up = (k + 4 <= g.Nz + g.Hz - 1) ? 4 * sz : 3 * sz;      // the last level's request stays inside the parent array (unused)
        ta_nx = pa[n + up];
        if constexpr (Q) tb_nx = pb[n + up];
        const int lv3 = ZS ? (k - kbeg) % 3 : 0;
        bool zxy = false;
        if constexpr (ZS) {
            if (t == 0) ZF[(lv3 + 2) % 3] = 1;      // reset the flag of level k + 2 (set while level k + 1 is staged, at the end of the next trip)
            zxy = __builtin_amdgcn_readfirstlane(ZF[lv3]) != 0;      // q is zero on the whole staged level k: exact zero x / y fluxes
        }
#pragma unroll
        for (int q = 0; q < HPT; ++q) {
            ha[q] = hok[q] ? pa[hn[q] + lev] : 0.0;
            hb[q] = (Q && hok[q]) ? pb[hn[q] + lev] : 0.0;
        }
        const double u0a = (E.mode == 2) ? E.u0[n] : 0.0, u0b = (Q && E.mode == 2) ? E.u0b[n] : 0.0;
        const double ru_t = ru_n, rv_t = rv_n, rw_t = rw_n, rvtop = rvtop_n;
        // The y face above the tile belongs to no row of the tile: one wavefront per field evaluates it, and the duty rotates with the
        // level (field a: row (k - kbeg) mod TY, field b: half a turn later).
        const int turn = (k - kbeg) & (TY - 1);
        const bool duty_a = tyu == turn, duty_b = Q && tyu == ((turn + TY / 2) & (TY - 1));
        ru_n = ru[n + sz]; rv_n = rv[n + sz]; rw_n = rw[n + 2 * sz];      // level k + 1 (level kend of the last trip is a halo level: in bounds, unused)
        {
            const int turn_n = (turn + 1) & (TY - 1);
            const bool duty_n = tyu == turn_n || (Q && tyu == ((turn_n + TY / 2) & (TY - 1)));
            rvtop_n = duty_n ? rv[ntop0 + lev] : 0.0;
        }
        const double rho = LV.rho(k), rrho = LV.rrho(k), Ax_k = LV.Ax(k), Ay_k = LV.Ay(k), Vi_k = LV.Vinv_c(k);
        const double rho1 = LV.rho(k + 1), rrho1 = LV.rrho(k + 1), rhof1 = LV.rho_f(k + 1), rrhof1 = LV.rrho_f(k + 1);
        const double rho3 = LV.rho(k + 3), rrho3 = LV.rrho(k + 3);
        if (((k - kbeg) & (BZ5_EB - 1)) == 0) {       // out-of-wave x flux for the next 64 levels (lane l <-> level k + l)
            const int kk = min(k + (tx & (BZ5_EB - 1)), kend - 1);
            const long long ne = g.idx(ie, jc, kk);
            const double rhk = g.rho[kk], rrk = g.rrho[kk];
            const double ue = bz_cdiv(ru[ne], rhk, rrk);
            const bool le_ = ue > 0.0;
            const double cf = g.Ax[kk] * ue;
            ea = rhk * (cf * bz_up5(bz_cdiv(pa[ne - 3], rhk, rrk), bz_cdiv(pa[ne - 2], rhk, rrk), bz_cdiv(pa[ne - 1], rhk, rrk),
                                    bz_cdiv(pa[ne], rhk, rrk), bz_cdiv(pa[ne + 1], rhk, rrk), bz_cdiv(pa[ne + 2], rhk, rrk), le_));
            if constexpr (Q)
            eb = rhk * (cf * bz_up5(bz_cdiv(pb[ne - 3], rhk, rrk), bz_cdiv(pb[ne - 2], rhk, rrk), bz_cdiv(pb[ne - 1], rhk, rrk),
                                    bz_cdiv(pb[ne], rhk, rrk), bz_cdiv(pb[ne + 1], rhk, rrk), bz_cdiv(pb[ne + 2], rhk, rrk), le_));
        }
        const int src = (k - kbeg) & (BZ5_EB - 1);
        // advecting fluxes of the three low/upper faces (shared by both fields)
        const double ut = bz_cdiv(ru_t, rho, rrho), vt = bz_cdiv(rv_t, rho, rrho);
        const double wt = bz_cdiv(rw_t, rhof1, rrhof1);
        const double cfx = Ax_k * ut, cfy = Ay_k * vt, cfz = g.Az * wt, rf = rhof1;
        const bool lx = ut > 0.0, ly = vt > 0.0, lz = wt > 0.0;
        const int Bz = bz_buffer_face(k + 1, g.Nz);
        double cfy2 = 0.0;
        bool ly2 = false;
        if (duty_a || duty_b) {
            const double vtop = bz_cdiv(rvtop, rho, rrho);
            ly2 = vtop > 0.0;
            cfy2 = Ay_k * vtop;
        }
        const int c = tx + 3;
        // one field at a time (keeps the live set of the WENO evaluations small): x low face from the tile row, y low face from
        // the tile column (wave 0 also the face above the tile), upper z face from the ring
        double fxa, fya, fza_hi, fxb, fyb, fzb_hi;
        const double ta = bz_cdiv(ta_raw, rho3, rrho3);
        {
            const double(*Tk)[TC] = T[buf][0];
            const double *rr_ = Tk[ty + 3] + tx;
            fxa = rho * (cfx * bz_up5(rr_[0], rr_[1], rr_[2], a[3], rr_[4], rr_[5], lx));
            fya = rho * (cfy * bz_up5y<WY>(Tk[ty][c], Tk[ty + 1][c], Tk[ty + 2][c], a[3], Tk[ty + 4][c], Tk[ty + 5][c], ly, Byj));
            FY[buf][0][ty][tx] = fya;
            if (duty_a)
                FY[buf][0][TY][tx] = rho * (cfy2 * bz_up5y<WY>(Tk[TY][c], Tk[TY + 1][c], Tk[TY + 2][c], Tk[TY + 3][c], Tk[TY + 4][c], Tk[TY + 5][c], ly2, Byt));
            fza_hi = rf * (cfz * bz_upB(a[1], a[2], a[3], a[4], a[5], ta, lz, Bz));
        }
        double tb = 0.0;
        fxb = 0.0; fyb = 0.0; fzb_hi = 0.0;
        if constexpr (Q) {
        tb = bz_cdiv(tb_raw, rho3, rrho3);
        bool zz = false;
        if constexpr (ZS) {
            zrun = (tb == 0.0) ? min(zrun + 1, 6) : 0;
            zz = __all(zrun >= 6);      // b[1] .. b[5], tb are all zero in every column of the wavefront: exact zero vertical flux
        }
        if (zxy) {
            fxb = 0.0; fyb = 0.0;
            FY[buf][1][ty][tx] = 0.0;
            if (duty_b) FY[buf][1][TY][tx] = 0.0;
        } else {
            const double(*Tk)[TC] = T[buf][1];
            const double *rr_ = Tk[ty + 3] + tx;
            fxb = rho * (cfx * bz_up5(rr_[0], rr_[1], rr_[2], b[3], rr_[4], rr_[5], lx));
            fyb = rho * (cfy * bz_up5y<WY>(Tk[ty][c], Tk[ty + 1][c], Tk[ty + 2][c], b[3], Tk[ty + 4][c], Tk[ty + 5][c], ly, Byj));
            FY[buf][1][ty][tx] = fyb;
            if (duty_b)
                FY[buf][1][TY][tx] = rho * (cfy2 * bz_up5y<WY>(Tk[TY][c], Tk[TY + 1][c], Tk[TY + 2][c], Tk[TY + 3][c], Tk[TY + 4][c], Tk[TY + 5][c], ly2, Byt));
        }
        if (zz) fzb_hi = 0.0;
        else fzb_hi = rf * (cfz * bz_upB(b[1], b[2], b[3], b[4], b[5], tb, lz, Bz));
        }
        // x flux of the upper face = the low-face flux of lane tx + 1 (DPP move, vector ALU) or, in the row's last lane le, lane `src` of the
        // out-of-wave batch (v_readlane: src is wave-uniform).  Formed here, where the fluxes are complete, not behind the level's barrier:
        // neither operand depends on it.  Lane 63 receives 0 from the shift: it is lane le (replaced) or a lane beyond a ragged row (store =
        // false).  Outside the wave-uniform shortcut branches above, so all 64 lanes are active; both fields after the second one's fluxes
        // (the first field's exchange ahead of them cost the general body with y walls two registers of scratch).
        double na = bz_lane_down(fxa);
        const double xa = bz_lane_read(ea, src);
        if (tx == le) na = xa;
        const double dxa = na - fxa;
        double dxb = 0.0;
        if constexpr (Q) {
            double nb = bz_lane_down(fxb);
            const double xb = bz_lane_read(eb, src);
            if (tx == le) nb = xb;
            dxb = nb - fxb;
        }
        // the cell's own prognostic values (read three levels ago as ring tops: an L2 / Infinity-Cache hit), requested before the staging
        // arithmetic so that the RK update after the barrier finds them
        double pa_n, pb_n;
        if constexpr (DRYQ) { pa_n = araw[0]; pb_n = b[3]; araw[0] = araw[1]; araw[1] = araw[2]; araw[2] = ta_raw; }
        else { pa_n = pa[n]; pb_n = pb[n]; }
        // ---- stage level k+1 in the other buffer ----
        T[buf ^ 1][0][ty + 3][tx + 3] = a[4];
        if constexpr (Q) T[buf ^ 1][1][ty + 3][tx + 3] = b[4];
        {
            const double rh = rho1, rr = rrho1;
            bool z1 = (b[4] == 0.0);
#pragma unroll
            for (int q = 0; q < HPT; ++q)
                if (hok[q]) {
                    T[buf ^ 1][0][hr[q]][hc[q]] = bz_cdiv(ha[q], rh, rr);
                    if constexpr (Q) {
                        const double hbv = bz_cdiv(hb[q], rh, rr);
                        T[buf ^ 1][1][hr[q]][hc[q]] = hbv;
                        z1 = z1 && (hbv == 0.0);
                    }
                }
            if (ZS && !__all(z1) && tx == 0) ZF[(lv3 + 1) % 3] = 0;
        }
        __syncthreads();
        // ---- combine, SSP-RK3 update, temperature of the updated cell for the next stage's buoyancy ----
        {
            const double dya = FY[buf][0][ty + 1][tx] - fya;
            const double Vi = Vi_k;
            const double ga = -(Vi * (dxa + dya + (fza_hi - fza)));
            double gb = 0.0;
            if constexpr (Q) {
                const double dyb = FY[buf][1][ty + 1][tx] - fyb;
                gb = -(Vi * (dxb + dyb + (fzb_hi - fzb)));
            }
            if (store) {
                const double rth = bz_rk_apply_pre(E.mode, E.dt, E.alpha, E.oma, u0a, E.u0_out, ga, pa_n, n);
                F.oa[n] = rth;        // interior only: the projection kernel that follows stores the periodic images
                if constexpr (Q) {
                    const double rq = bz_rk_apply_pre(E.mode, E.dt, E.alpha, E.oma, u0b, E.u0b_out, gb, pb_n, n);
                    F.ob[n] = rq;     // (the temperature the buoyancy needs is derived from these two by the z-momentum kernel of the next stage)
                }
            }
        }
        fza = fza_hi; fzb = fzb_hi;
#pragma unroll
        for (int s = 0; s < 5; ++s) { a[s] = a[s + 1]; b[s] = b[s + 1]; }
        a[5] = ta; b[5] = tb;
        buf ^= 1;
    }
}


// DRYQ instantiations: the dry and the general body are separate KERNELS (round 5; round 4 dispatched on the scan's word inside one kernel,
// so rocprofv3 could not tell a dry launch from a moist one: VERDICT r04 item 2).  The host follows the scan's verdict (bz_ctx::q_host,
// bz_step.hip): once it knows the model is moist it launches the general kernel alone (GUARD = false).  While the last verdict is "dry" —
// a dry model is scanned at every call and the verdict of THIS call is not on the host yet — it launches the dry kernel and the general
// one with GUARD = true: each reads the word the scan just wrote and the one it does not apply to returns at once (a few microseconds of
// empty workgroups, under a kernel name of their own).  Contexts without a word launch the general kernel only.
template <bool DRYQ, bool GUARD>
__device__ __forceinline__ bool bz_lean_skip(const Lean5 &F)
{
    if constexpr (!GUARD) return false;
    const bool dry = F.qstate != nullptr && __builtin_amdgcn_readfirstlane(*F.qstate) == 1;      // wave-uniform: one scalar load
    return dry != DRYQ;
}
template <int TY, bool WY = false, bool DRYQ = false, bool GUARD = true>
__global__ __launch_bounds__(64 * TY) __attribute__((amdgpu_waves_per_eu(BZ5_SCALAR_WAVES, BZ5_SCALAR_WAVES))) void k5_scalar_pair(DevGrid g, Lean5 F, int kchunk, RKEpilogue E)
{
    constexpr int TR = TY + 6, TC = 72;
    __shared__ double T[2 * 2 * TR * TC];
    __shared__ double FY[2 * 2 * (TY + 1) * 64];
    __shared__ int ZF[3];
    if (bz_lean_skip<DRYQ, GUARD>(F)) return;
    k5_scalar_pair_body<TY, WY, DRYQ>(g, F, kchunk, E, T, FY, ZF);
}

// out-of-wave x fluxes of the momentum kernels with the advected velocity derived from its momentum component
// (flux_x_at of bz_tendency4_kernels.h with c = m / rho)
// By: walls in y — buffer of the y-face the advecting flux of the v kernel is interpolated to (3: order 4, the periodic case)
template <int KIND>
__device__ __forceinline__ double flux_x_lean(const DevGrid &g, const Tend3Fields &F, const double *__restrict__ m, int i, int j, int k, int By = 3)
{
    const long long n = g.idx(i, j, k);
    const double a = (KIND == T3_V && By != 3) ? bz_symm2(g.Ax[k] * F.ru[n - g.Sx], g.Ax[k] * F.ru[n]) : adv_x<KIND>(g, F, n, k);
    const double rh = (KIND == T3_W) ? g.rho_f[k] : g.rho[k], rr = (KIND == T3_W) ? g.rrho_f[k] : g.rrho[k];
    if constexpr (KIND == T3_U)
        return a * bz_up5(bz_cdiv(m[n - 2], rh, rr), bz_cdiv(m[n - 1], rh, rr), bz_cdiv(m[n], rh, rr), bz_cdiv(m[n + 1], rh, rr),
                          bz_cdiv(m[n + 2], rh, rr), bz_cdiv(m[n + 3], rh, rr), a > 0.0);
    else
        return a * bz_up5(bz_cdiv(m[n - 3], rh, rr), bz_cdiv(m[n - 2], rh, rr), bz_cdiv(m[n - 1], rh, rr), bz_cdiv(m[n], rh, rr),
                          bz_cdiv(m[n + 1], rh, rr), bz_cdiv(m[n + 2], rh, rr), a > 0.0);
}


// ---------------------------------------------------------------------------------------------------------------------
// x-momentum, sixth generation: EVERYTHING a level needs from its neighbours comes from LDS, and every global load of an iteration
// is a prefetch for the NEXT level (register -> LDS at the end of the iteration).  Why: the ISA of k5_u has 28 vector loads and 19
// s_waitcnt per level; with 128 VGPRs the compiler cannot hoist them, so each wave stalls on L1/L2 latency ~19 times per level and
// the SIMDs idle (VALU busy 13 % of wave cycles at 4 waves / SIMD: 40-50 % of issue capacity) while neither HBM nor the ALUs are
// saturated.  Here a level issues <= 6 loads per thread at its top (ring top of the next level, own rho_v / rho_w elements, u0, and
// <= 2 frame cells), consumes them at its end, and reads its stencils with ds_read (tiles: u derived (TY+6) x 70; raw rho_u TY x 67;
// raw rho_v (TY+1) x 67; raw rho_w TY x 67 at the upper face; double-buffered).  Same arithmetic, same bits as k5_u.
// ---------------------------------------------------------------------------------------------------------------------
// ST: the advected velocity is read from the stored field Lean5::vel instead of being derived from the momentum (see Lean5); the
// arithmetic per flux is that of k_u_tend_lds (bz_tendency4_kernels.h), which these instantiations replace.
template <int TY, bool MF = false, bool WY = false, bool ST = false>      // MF: momentum terms of a forcing stack in the RK epilogue (Lean5::mforce); WY: walls in y
__global__ __launch_bounds__(64 * TY, BZ_LEAN_WAVES) void k6_u(DevGrid g, Lean5 L, int kchunk, RKEpilogue E)
{
    static_assert(!(ST && WY), "stored-velocity instantiations: periodic / slab rows");
    constexpr int TR = TY + 6, TC = 72, NT = 64 * TY;
    constexpr int NH1 = TR * 70 - TY * 64;               // frame of the u tile (468 for TY = 8): one cell per thread
    constexpr int NH2 = 3 * (TY + 1) + 64 + 3 * TY;      // rho_v side columns + its top row + rho_w side columns (115)
    static_assert(NH1 <= NT && NH2 <= NT, "one frame cell of each kind per thread");
    __shared__ double U[2][TR][TC];
    __shared__ double RU[2][TY][TC];
    __shared__ double RV[2][TY + 1][TC];
    __shared__ double RW[2][TY][TC];
    __shared__ double FY[2][TY + 1][64];
    int bx, by, bz;
    bz_block5(L, bx, by, bz);
    const int tx = threadIdx.x, ty = threadIdx.y, t = ty * 64 + tx, tc = tx + 3;
    const int i0 = bx * 64, j0 = by * TY;
    const int i = i0 + tx, j = j0 + ty;
    const int ic = min(i, g.Nx + 2), jc = min(j, g.Ny + 2);
    const int ie = i0 - 1, le = 0;
    const int kbeg = bz * kchunk, kend = min(kbeg + kchunk, g.Nz);
    if (kbeg >= kend) return;
    const ix_t sz = (ix_t)g.Sxy;
    const bool store = (i < g.Nx) && (j < g.Ny);
    const double *__restrict__ ru = L.ru, *__restrict__ rv = L.rv, *__restrict__ rw = L.rw;
    const double *__restrict__ vel = ST ? L.vel : L.ru;      // stored u (ST) — else unused
    Tend3Fields F;
    F.ru = L.ru; F.rv = L.rv; F.rw = L.rw; F.u = F.v = F.w = F.T = F.q = nullptr; F.c = ST ? L.vel : nullptr; F.G = L.out;
    ix_t n = (ix_t)g.idx(ic, jc, kbeg);
    // frame cell 1: the u tile's frame (raw rho_u; its side cells next to the interior also feed the raw rho_u tile)
    const bool h1ok = t < NH1;
    int h1r = 0, h1c = 0;
    {
        const int h = h1ok ? t : 0;
        if (h < 6 * 70) { const int rr = h / 70; h1c = h - rr * 70; h1r = (rr < 3) ? rr : TY + rr; }
        else { const int hh = h - 6 * 70, rr = hh / 6, cc = hh - rr * 6; h1r = 3 + rr; h1c = (cc < 3) ? cc : 64 + cc; }
    }
    const ix_t h1n = (ix_t)g.idx(min(i0 - 3 + h1c, g.Nx + 2), min(j0 - 3 + h1r, g.Ny + 2), kbeg);
    const bool h1raw = h1ok && h1r >= 3 && h1r < TY + 3 && (h1c == 2 || h1c == 67 || h1c == 68);
    // frame cell 2: rho_v side columns (cols i0-2, i0-1, i0+64; rows j0 .. j0+TY), rho_v top row, rho_w side columns (upper face)
    const bool h2ok = t < NH2;
    int h2sel = 0, h2r = 0, h2c = 0;             // sel 0: rho_v, 1: rho_w
    {
        const int id = h2ok ? t : 0;
        if (id < 3 * (TY + 1)) { h2r = id / 3; const int cc = id - 3 * h2r; h2c = (cc < 2) ? 1 + cc : 67; }
        else if (id < 3 * (TY + 1) + 64) { h2r = TY; h2c = 3 + (id - 3 * (TY + 1)); }
        else { h2sel = 1; const int m = id - 3 * (TY + 1) - 64; h2r = m / 3; const int cc = m - 3 * h2r; h2c = (cc < 2) ? 1 + cc : 67; }
    }
    const double *__restrict__ h2src = h2sel ? rw : rv;
    const ix_t h2n = (ix_t)g.idx(min(i0 - 3 + h2c, g.Nx + 2), min(j0 + h2r, g.Ny + 2), kbeg) + (h2sel ? sz : (ix_t)0);

    double r[6];
#pragma unroll
    for (int s = 0; s < 6; ++s) r[s] = ST ? vel[n + s * sz - 3 * sz] : bz_cdiv(ru[n + s * sz - 3 * sz], g.rho[kbeg + s - 3], g.rrho[kbeg + s - 3]);
    double fz_lo = vflux<T3_U>(g, F, n, kbeg, r[0], r[1], r[2], r[3], r[4], r[5]);
    double q0 = ru[n], q1 = ru[n + sz], q2 = ru[n + 2 * sz];          // raw rho_u of the own column at levels k, k+1, k+2
    // tiles of level kbeg
    U[0][ty + 3][tc] = r[3];
    RU[0][ty][tc] = q0;
    RV[0][ty][tc] = rv[n];
    RW[0][ty][tc] = rw[n + sz];
    if (h1ok) {
        const double raw = (ST && !h1raw) ? 0.0 : ru[h1n];
        U[0][h1r][h1c] = ST ? vel[h1n] : bz_cdiv(raw, g.rho[kbeg], g.rrho[kbeg]);
        if (h1raw) RU[0][h1r - 3][h1c] = raw;
    }
    if (h2ok) { if (h2sel) RW[0][h2r][h2c] = h2src[h2n]; else RV[0][h2r][h2c] = h2src[h2n]; }
    double tcur_raw = ru[n + 3 * sz];
    double tcur_v = ST ? vel[n + 3 * sz] : 0.0;      // ST: the ring top of the stored velocity travels beside the raw momentum
    double u0cur = (E.mode == 2) ? E.u0[n] : 0.0;
    __syncthreads();

    double edge = 0.0;
    int buf = 0;
    for (int k = kbeg; k < kend; ++k, n += sz) {
        const ix_t lev1 = (ix_t)(k + 1 - kbeg) * sz;
        // ---- prefetch for level k+1 (consumed at the end of this iteration / in the next one) ----
        // ST: the raw momentum of the next level is read where it is staged (one register) instead of riding the three-level delay line
        // behind the ring-top load: the stored-velocity ring top took its registers
        const double p_top = ST ? ru[n + sz] : ru[n + ((k + 4 <= g.Nz + g.Hz - 1) ? 4 * sz : 3 * sz)];
        const double p_topv = ST ? vel[n + ((k + 4 <= g.Nz + g.Hz - 1) ? 4 * sz : 3 * sz)] : 0.0;
        const double p_h1 = h1ok ? (ST ? vel : ru)[h1n + lev1] : 0.0;
        const double p_h1raw = (ST && h1raw) ? ru[h1n + lev1] : 0.0;
        const double p_h2 = h2ok ? h2src[h2n + lev1] : 0.0;
        const double p_rv = rv[n + sz], p_rw = rw[n + 2 * sz];
        const double p_u0 = (E.mode == 2) ? E.u0[n + sz] : 0.0;
        if (((k - kbeg) & (BZ5_EB - 1)) == 0) {
            const int kk = min(k + (tx & (BZ5_EB - 1)), kend - 1);
            edge = ST ? flux_x_at<T3_U>(g, F, ie, jc, kk) : flux_x_lean<T3_U>(g, F, ru, ie, jc, kk);
        }
        const int src = (k - kbeg) & (BZ5_EB - 1);
        const double Ax = g.Ax[k], Ay = g.Ay[k], Az = g.Az;
        const double c0 = r[3];
        const double(*Uk)[TC] = U[buf];
        // ---- x: flux at centre i ----
        const double *rur = RU[buf][ty] + tc, *ur = Uk[ty + 3] + tc;
        const double ax = bz_symm4(Ax * rur[-1], Ax * q0, Ax * rur[1], Ax * rur[2]);
        const double fx = ax * bz_up5(ur[-2], ur[-1], c0, ur[1], ur[2], ur[3], ax > 0.0);
        // flux at centre i - 1: lane tx - 1 (DPP move) or, in lane le = 0, lane `src` of the out-of-wave batch (v_readlane, src wave-uniform); formed
        // here, ahead of the level's barrier, which neither operand depends on.  Lane 0 receives 0 from the shift and is the lane replaced.
        // (The forcing instantiations keep their shuffles behind the barrier: with the exchange moved or replaced the compiler contracts
        // one product of their epilogue differently — one v_fma_f64 less, one v_add_f64 more — and their results move in the last bit.)
        double nb = 0.0;
        if constexpr (!MF) {
            nb = bz_lane_up(fx);
            const double e = bz_lane_read(edge, src);
            if (tx == le) nb = e;
        }
        // ---- y: flux at the own low y-face ----
        const double *rvr = RV[buf][ty] + tc;
        const double ay = bz_symm4(Ay * rvr[-2], Ay * rvr[-1], Ay * rvr[0], Ay * rvr[1]);
        const double fy = ay * bz_up5y<WY>(Uk[ty][tc], Uk[ty + 1][tc], Uk[ty + 2][tc], c0, Uk[ty + 4][tc], Uk[ty + 5][tc], ay > 0.0, by5_face<WY>(g, __builtin_amdgcn_readfirstlane(j)));
        FY[buf][ty][tx] = fy;
        if (ty == 0) {
            const double *rvt = RV[buf][TY] + tc;
            const double at = bz_symm4(Ay * rvt[-2], Ay * rvt[-1], Ay * rvt[0], Ay * rvt[1]);
            FY[buf][TY][tx] = at * bz_up5y<WY>(Uk[TY][tc], Uk[TY + 1][tc], Uk[TY + 2][tc], Uk[TY + 3][tc], Uk[TY + 4][tc], Uk[TY + 5][tc], at > 0.0,
                                               by5_face<WY>(g, j0 + TY));
        }
        // ---- z: upper face k+1 ----
        const double tnew = ST ? tcur_v : bz_cdiv(tcur_raw, g.rho[k + 3], g.rrho[k + 3]);
        const double *rwr = RW[buf][ty] + tc;
        const double wt = bz_symm4(Az * rwr[-2], Az * rwr[-1], Az * rwr[0], Az * rwr[1]);
        const double fz_hi = wt * bz_upB(r[1], r[2], r[3], r[4], r[5], tnew, wt > 0.0, bz_buffer_face(k + 1, g.Nz));
        // ---- stage level k+1 from the prefetch registers ----
        U[buf ^ 1][ty + 3][tc] = r[4];
        RU[buf ^ 1][ty][tc] = ST ? p_top : q1;
        RV[buf ^ 1][ty][tc] = p_rv;
        RW[buf ^ 1][ty][tc] = p_rw;
        if (h1ok) {
            U[buf ^ 1][h1r][h1c] = ST ? p_h1 : bz_cdiv(p_h1, g.rho[k + 1], g.rrho[k + 1]);
            if (h1raw) RU[buf ^ 1][h1r - 3][h1c] = ST ? p_h1raw : p_h1;
        }
        if (h2ok) { if (h2sel) RW[buf ^ 1][h2r][h2c] = p_h2; else RV[buf ^ 1][h2r][h2c] = p_h2; }
        __syncthreads();
        {
            if constexpr (MF) {
                nb = __shfl_up(fx, 1);
                const double e = __shfl(edge, src);
                if (tx == le) nb = e;
            }
            const double dx = fx - nb;
            const double dy = FY[buf][ty + 1][tx] - fy;
            double Gu = -(g.Vinv_c[k] * (dx + dy + (fz_hi - fz_lo)));
            if constexpr (MF) {      // -x_f_cross_U + rho F_u: rho_v at (i-1, j), (i-1, j+1), (i, j), (i, j+1) from the raw rho_v tile
                if (L.mforce & 1) {
                    const double *rv0 = RV[buf][ty] + tc, *rv1 = RV[buf][ty + 1] + tc;
                    const double a = (rv0[-1] + rv1[-1]) / 2, b = (rv0[0] + rv1[0]) / 2;
                    Gu -= -L.cor_f * ((a + b) / 2);
                }
                if (L.mforce & (2 | 8)) {      // rho x (subsidence profile + static profile), summed in that order
                    const double rho = g.rho[k];
                    double tot = (L.mforce & 8) ? rho * L.Su[k] : 0.0;
                    if (L.mforce & 2) tot = (L.mforce & 8) ? tot + rho * L.Fu[k] : rho * L.Fu[k];
                    Gu += tot;
                }
            }
            if (store) L.out[n] = (ST && E.mode == 0) ? Gu : bz_rk_apply_pre(E.mode, E.dt, E.alpha, E.oma, u0cur, E.u0_out, Gu, q0, n);
        }
        fz_lo = fz_hi;
#pragma unroll
        for (int s = 0; s < 5; ++s) r[s] = r[s + 1];
        r[5] = tnew;
        if (ST) q0 = p_top;
        else { q0 = q1; q1 = q2; q2 = tcur_raw; tcur_raw = p_top; }
        u0cur = p_u0;
        if (ST) tcur_v = p_topv;
        buf ^= 1;
    }
}


// ---------------------------------------------------------------------------------------------------------------------
// y-momentum, sixth generation (see k6_u): the v tile carries its x halo, so the x-stencil is five ds_reads instead of five loads +
// five column divisions; ring top and u0 are loaded one level ahead.  Same arithmetic, same bits as k5_v.
// ---------------------------------------------------------------------------------------------------------------------
template <int TY, bool MF = false, bool WY = false, bool ST = false>      // ST: stored v (see k6_u)
__global__ __launch_bounds__(64 * TY, ((MF && WY) ? 4 : BZ_LEAN_WAVES)) void k6_v(DevGrid g, Lean5 L, int kchunk, RKEpilogue E)
{
    static_assert(!(ST && WY), "stored-velocity instantiations: periodic / slab rows");
    constexpr int RV = TY + 6, RM = TY + 4;               // rows of the v tile / of the momentum tiles
    constexpr int TC = 72;                                // v tile with its x halo: columns i0-3 .. i0+65 at offset 3
    __shared__ double Tv[2][RV][TC];
    __shared__ double Tm[2][3][RM][64];                   // 0: Ax*rho_u, 1: Ay*rho_v, 2: Az*rho_w at the upper z-face
    __shared__ double FY[2][TY + 1][64];
    constexpr int NT = 64 * TY, NFR = 16 * 64, HPT = (NFR + NT - 1) / NT;
    int bx, by, bz;
    bz_block5(L, bx, by, bz);
    const int tx = threadIdx.x, ty = threadIdx.y, t = ty * 64 + tx, tc = tx + 3;
    const int i0 = bx * 64, j0 = by * TY;
    const int i = i0 + tx, j = j0 + ty;
    const int ic = min(i, g.Nx + 2), jc = min(j, g.Ny + 2);
    const int nact = min(64, g.Nx - i0);
    const int ie = i0 + nact, le = nact - 1;              // x flux at x-faces: last lane needs face i0+nact
    const int kbeg = bz * kchunk, kend = min(kbeg + kchunk, g.Nz);
    if (kbeg >= kend) return;
    const ix_t sz = (ix_t)g.Sxy;
    const bool store = (i < g.Nx) && (j < g.Ny) && !(WY && j == 0);      // walls in y: the wall face is never updated
    const int ju = __builtin_amdgcn_readfirstlane(j);      // one row per wavefront
    const int Bf = by5_face<WY>(g, ju), Bc = by5_center<WY>(g, ju), Bc0 = by5_center<WY>(g, j0 - 1);
    const double *__restrict__ ru = L.ru, *__restrict__ rv = L.rv, *__restrict__ rw = L.rw;
    const double *__restrict__ vel = ST ? L.vel : L.rv;      // stored v (ST) — else unused
    Tend3Fields F;
    F.ru = L.ru; F.rv = L.rv; F.rw = L.rw; F.u = F.v = F.w = F.T = F.q = nullptr; F.c = ST ? L.vel : nullptr; F.G = L.out;
    const double Az = g.Az;
    ix_t n = (ix_t)g.idx(ic, jc, kbeg);

    // frame rows: id 0..5 v tile rows {0,1,2,TY+3,TY+4,TY+5}; 6..8 rho_u rows {0,1,TY+2}; 9..12 rho_v rows
    // {0,1,TY+2,TY+3}; 13..15 rho_w rows {0,1,TY+2}   (momentum-tile row r' <-> grid row j0-2+r').  A frame row is staged by
    // one wave (id = wave index + TY q), so the source array and the scaling are wave-uniform: kept in scalar registers.
    bool hok[HPT];
    int hsel[HPT], hrow[HPT];
    ix_t hn[HPT];
    const double *hsrc[HPT];
#pragma unroll
    for (int q = 0; q < HPT; ++q) {
        const int h = t + q * NT;
        hok[q] = h < NFR;
        const int id = __builtin_amdgcn_readfirstlane(hok[q] ? (h >> 6) : 0);
        int sel, row, grow;                                // sel: 0 v, 1 rho_u, 2 rho_v, 3 rho_w
        if (id < 6) { sel = 0; row = (id < 3) ? id : TY + id; grow = j0 - 3 + row; }
        else if (id < 9) { sel = 1; const int m = id - 6; row = (m < 2) ? m : TY + 2; grow = j0 - 2 + row; }
        else if (id < 13) { sel = 2; const int m = id - 9; row = (m < 2) ? m : TY + m; grow = j0 - 2 + row; }
        else { sel = 3; const int m = id - 13; row = (m < 2) ? m : TY + 2; grow = j0 - 2 + row; }
        hsel[q] = sel; hrow[q] = row;
        hsrc[q] = (sel == 1) ? ru : (sel == 3) ? rw : (ST && sel == 0) ? vel : rv;
        hn[q] = (ix_t)g.idx(min(i0 + tx, g.Nx + 2), min(grow, g.Ny + 2), kbeg) + (sel == 3 ? sz : (ix_t)0);
    }
    auto frame_load = [&](int q, ix_t lev) -> double { return hsrc[q][hn[q] + lev]; };   // raw value at the level offset
    auto frame_store = [&](int b, int q, double raw, int klev) {          // scale / derive and stage for level klev
        if (hsel[q] == 0) Tv[b][hrow[q]][tc] = ST ? raw : bz_cdiv(raw, g.rho[klev], g.rrho[klev]);
        else Tm[b][hsel[q] - 1][hrow[q]][tx] = ((hsel[q] == 1) ? g.Ax[klev] : (hsel[q] == 2) ? g.Ay[klev] : Az) * raw;
    };

    // side cells of the own rows (x halo of the v tile: columns i0-3 .. i0-1 and i0+64, i0+65): one cell for the first 5 TY threads
    const bool sok = t < 5 * TY;
    const int srow = sok ? t / 5 : 0, scc = sok ? t % 5 : 0, scol = (scc < 3) ? scc : 64 + scc;
    const ix_t sn = (ix_t)g.idx(min(i0 - 3 + scol, g.Nx + 2), min(j0 + srow, g.Ny + 2), kbeg);

    double r[6];
#pragma unroll
    for (int s = 0; s < 6; ++s) r[s] = ST ? vel[n + s * sz - 3 * sz] : bz_cdiv(rv[n + s * sz - 3 * sz], g.rho[kbeg + s - 3], g.rrho[kbeg + s - 3]);
    double fz_lo;
    if (WY && Bf != 3) {      // walls in y: the advecting flux at (y-face j, z-face kbeg) from rows j-1, j only
        const double wt0 = bz_symm2(Az * rw[n - (ix_t)g.Sx], Az * rw[n]);
        fz_lo = wt0 * bz_upB(r[0], r[1], r[2], r[3], r[4], r[5], wt0 > 0.0, bz_buffer_face(kbeg, g.Nz));
    } else fz_lo = vflux<T3_V>(g, F, n, kbeg, r[0], r[1], r[2], r[3], r[4], r[5]);
    // raw rho_v of the own column at levels k .. k+2 (the ring-top load of level k+3 enters at the end of each iteration)
    double q0 = rv[n], q1 = rv[n + sz], q2 = rv[n + 2 * sz];
    Tv[0][ty + 3][tc] = r[3];
    if (sok) Tv[0][srow + 3][scol] = ST ? vel[sn] : bz_cdiv(rv[sn], g.rho[kbeg], g.rrho[kbeg]);
    Tm[0][0][ty + 2][tx] = g.Ax[kbeg] * ru[n];
    Tm[0][1][ty + 2][tx] = g.Ay[kbeg] * q0;
    Tm[0][2][ty + 2][tx] = Az * rw[n + sz];
#pragma unroll
    for (int q = 0; q < HPT; ++q)
        if (hok[q]) frame_store(0, q, frame_load(q, 0), kbeg);
    __syncthreads();

    double tcur_raw = rv[n + 3 * sz];
    double tcur_v = ST ? vel[n + 3 * sz] : 0.0;
    double u0cur = (E.mode == 2) ? E.u0[n] : 0.0;
    double edge = 0.0;
    int buf = 0;
    for (int k = kbeg; k < kend; ++k, n += sz) {
        const ix_t lev = (ix_t)(k + 1 - kbeg) * sz;
        double hnext[HPT];
#pragma unroll
        for (int q = 0; q < HPT; ++q) hnext[q] = hok[q] ? frame_load(q, lev) : 0.0;
        const double p_side = sok ? (ST ? vel : rv)[sn + lev] : 0.0;
        const double p_top = ST ? rv[n + sz] : rv[n + ((k + 4 <= g.Nz + g.Hz - 1) ? 4 * sz : 3 * sz)];      // ST: the next level's raw momentum, read where it is staged (see k6_u)
        const double p_topv = ST ? vel[n + ((k + 4 <= g.Nz + g.Hz - 1) ? 4 * sz : 3 * sz)] : 0.0;
        const double p_u0 = (E.mode == 2) ? E.u0[n + sz] : 0.0;
        const double tnew_raw = tcur_raw, u0v = u0cur;
        const double ru_n = g.Ax[k + 1] * ru[n + sz], rw_n = Az * rw[n + 2 * sz];
        // Coriolis: rho_u at (i, j-1), (i+1, j-1), (i, j), (i+1, j).  The Ax rho_u tile of this level holds the rows j-1 and j (premultiplied
        // by the level's Ax, no x halo): three of the four values come from LDS for every lane, the column i+1 of the last lane from memory;
        // one register crosses the barrier instead of four (round 3 loaded all four from memory: the forcing variant ran at 4 waves per
        // SIMD in Float32 because of them and cost 0.70 ms per launch at 512 x 512 x 256 against 0.52 without forcing)
        // (the last lane's two loads are requested here with the level's other loads and used after the stencil arithmetic)
        double cor_u = 0.0, cg1 = 0.0, cg3 = 0.0;
        if constexpr (MF) { if ((L.mforce & 1) && tx == 63) { const ix_t sy = (ix_t)g.Sx; cg1 = ru[n - sy + 1]; cg3 = ru[n + 1]; } }
        if (((k - kbeg) & (BZ5_EB - 1)) == 0) {
            const int kk = min(k + (tx & (BZ5_EB - 1)), kend - 1);
            edge = ST ? flux_x_at<T3_V>(g, F, ie, jc, kk) : flux_x_lean<T3_V>(g, F, rv, ie, jc, kk, Bf);
        }
        const int src = (k - kbeg) & (BZ5_EB - 1);
        const double rho = g.rho[k];
        const double c0 = r[3];
        const double(*V)[TC] = Tv[buf];
        const double *vrow = V[ty + 3] + tc;
        const double(*MU)[64] = Tm[buf][0];
        const double(*MV)[64] = Tm[buf][1];
        const double(*MW)[64] = Tm[buf][2];
        // ---- x: flux at (x-face i, y-face j): rho_u rows j-2..j+1, v x-stencil derived from the rho_v row ----
        const double ut = bz_symm4y<WY>(MU[ty][tx], MU[ty + 1][tx], MU[ty + 2][tx], MU[ty + 3][tx], Bf);
        const double fx = ut * bz_up5(vrow[-3], vrow[-2], vrow[-1], c0, vrow[1], vrow[2], ut > 0.0);
        // flux at x-face i + 1: lane tx + 1 (DPP move) or, in the row's last lane le, lane `src` of the out-of-wave batch (v_readlane, src
        // wave-uniform); formed here, ahead of the level's barrier, which neither operand depends on.  Lane 63 receives 0 from the shift: it is
        // lane le (replaced) or a lane beyond a ragged row (store = false; the wall-face stores below do not use it).
        // (The forcing instantiations keep their shuffles behind the barrier, as in k6_u: the same bits as before.)
        double nb = 0.0;
        if constexpr (!MF) {
            nb = bz_lane_down(fx);
            const double e = bz_lane_read(edge, src);
            if (tx == le) nb = e;
        }
        // ---- y: flux at centre j: rho_v rows j-1..j+2, v rows j-2..j+3 (walls: order 2 from faces j, j+1 next to a wall) ----
        const double vt = (!WY || Bc == 3) ? bz_symm4(MV[ty + 1][tx], MV[ty + 2][tx], MV[ty + 3][tx], MV[ty + 4][tx]) : bz_symm2(MV[ty + 2][tx], MV[ty + 3][tx]);
        const double fy = vt * bz_up5y<WY>(V[ty + 1][tc], V[ty + 2][tc], c0, V[ty + 4][tc], V[ty + 5][tc], V[ty + 6][tc], vt > 0.0, Bc);
        FY[buf][ty + 1][tx] = fy;
        if (ty == 0) {       // centre j0-1: rho_v rows j0-2..j0+1, v rows j0-3..j0+2
            const double vb = (!WY || Bc0 == 3) ? bz_symm4(MV[0][tx], MV[1][tx], MV[2][tx], MV[3][tx]) : bz_symm2(MV[1][tx], MV[2][tx]);
            FY[buf][0][tx] = vb * bz_up5y<WY>(V[0][tc], V[1][tc], V[2][tc], V[3][tc], V[4][tc], V[5][tc], vb > 0.0, Bc0);
        }
        // ---- z: advecting flux at (y-face j, z-face k+1) from the rho_w tile rows j-2..j+1 ----
        const double tnew = ST ? tcur_v : bz_cdiv(tnew_raw, g.rho[k + 3], g.rrho[k + 3]);
        const double wt = bz_symm4y<WY>(MW[ty][tx], MW[ty + 1][tx], MW[ty + 2][tx], MW[ty + 3][tx], Bf);
        const double fz_hi = wt * bz_upB(r[1], r[2], r[3], r[4], r[5], tnew, wt > 0.0, bz_buffer_face(k + 1, g.Nz));
        if constexpr (MF) {
            if (L.mforce & 1) {      // column tx + 1 of the last lane reads the next row's first element (in bounds) and is replaced
                const double Axk = g.Ax[k];
                const double l1 = MU[ty + 1][tx + 1], l3 = MU[ty + 2][tx + 1];
                const double c1 = (tx == 63) ? Axk * cg1 : l1, c3 = (tx == 63) ? Axk * cg3 : l3;
                cor_u = (((MU[ty + 1][tx] + c1) / 2 + (MU[ty + 2][tx] + c3) / 2) / 2) / Axk;
            }
        }
        // ---- stage level k+1 ----
        Tv[buf ^ 1][ty + 3][tc] = r[4];
        if (sok) Tv[buf ^ 1][srow + 3][scol] = ST ? p_side : bz_cdiv(p_side, g.rho[k + 1], g.rrho[k + 1]);
        Tm[buf ^ 1][0][ty + 2][tx] = ru_n;
        Tm[buf ^ 1][1][ty + 2][tx] = g.Ay[k + 1] * (ST ? p_top : q1);
        Tm[buf ^ 1][2][ty + 2][tx] = rw_n;
#pragma unroll
        for (int q = 0; q < HPT; ++q)
            if (hok[q]) frame_store(buf ^ 1, q, hnext[q], k + 1);
        __syncthreads();
        {
            if constexpr (MF) {
                nb = __shfl_down(fx, 1);
                const double e = __shfl(edge, src);
                if (tx == le) nb = e;
            }
            const double dx = nb - fx;
            const double dy = fy - FY[buf][ty][tx];
            double Gv = -(g.Vinv_c[k] * (dx + dy + (fz_hi - fz_lo)));
            if constexpr (MF) {      // -y_f_cross_U + rho F_v
                if (L.mforce & 1) Gv -= L.cor_f * cor_u;
                if (L.mforce & (4 | 16)) {
                    double tot = (L.mforce & 16) ? rho * L.Sv[k] : 0.0;
                    if (L.mforce & 4) tot = (L.mforce & 16) ? tot + rho * L.Fv[k] : rho * L.Fv[k];
                    Gv += tot;
                }
            }
            if (store) L.out[n] = (ST && E.mode == 0) ? Gv : bz_rk_apply_pre(E.mode, E.dt, E.alpha, E.oma, u0v, E.u0_out, Gv, q0, n);
            if constexpr (WY) {      // the wall faces of the predictor: j = 0 (this row, not updated) and j = Ny (first halo row above the last row)
                if (i < g.Nx && j == 0) L.out[n] = 0.0;
                if (i < g.Nx && j == g.Ny - 1) L.out[n + (ix_t)g.Sx] = 0.0;
            }
        }
        fz_lo = fz_hi;
        if (ST) q0 = p_top;
        else { q0 = q1; q1 = q2; q2 = tnew_raw; tcur_raw = p_top; }
        u0cur = p_u0;
        if (ST) tcur_v = p_topv;
#pragma unroll
        for (int s = 0; s < 5; ++s) r[s] = r[s + 1];
        r[5] = tnew;
        buf ^= 1;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// z-momentum: k_w_tend_lds<TY, 0> with w = rho_w / Iz(rho_r)(k) derived at staging time and the anelastic buoyancy from T and q
// derived from the stage-start rho theta, rho q of the own column (round 4: the scalar kernel used to store T for this kernel —
// one word per cell and stage written only to be read once; the derivation is a Markstein quotient and, in dry wavefronts, one
// multiplication by the level's Exner factor).
// ---------------------------------------------------------------------------------------------------------------------
// buoyancy of a cell from its prognostic densities: T = Pi^(Rm/cpm) theta as bz_temperature5r (the bits of the stored diagnostic),
// q = rho q / rho_r, then the expression of buoyancy3
// DRY (the DRYQ body of k6_w: rho q identically zero): q = 0 folded at compile time — T = pi theta, R_m = R_d.  The same bits as the
// general expression gives for rq = +0: bz_cdiv(+0, rho, rrho) = +0, so every wavefront takes the dry Exner factor, and
// (1 - 0) R_d + 0 R_v = R_d exactly (with or without contraction of the sum into an FMA); about nine instructions per cell and level less.
template <bool DRY = false>
__device__ __forceinline__ double buoyancy5(const DevGrid &g, double rth, double rq, int k, double rho, double rrho, double pi, double T_ref)
{
    if constexpr (DRY) {
        const double T = pi * bz_cdiv(rth, rho, rrho);
        const double rhop = rho * (g.Rd * T_ref / (g.Rd * T) - 1.0);
        return -g.g * rhop;
    }
    const double th = bz_cdiv(rth, rho, rrho), q = bz_cdiv(rq, rho, rrho);
    double T;
    if (__all(q == 0.0)) T = pi * th;
    else {
        const double qd = 1.0 - q;
        const double cpm = qd * g.cpd + q * g.cpv;
        T = bz_exner_factor(g, k, q, cpm) * th;
    }
    // buoyancy3 with the level's rho_r and T_r from the packed row (the same table entries)
    const double Rm = (1.0 - q) * g.Rd + q * g.Rv;
    const double rhop = rho * (g.Rd * T_ref / (Rm * T) - 1.0);
    return -g.g * rhop;
}


// ---------------------------------------------------------------------------------------------------------------------
// z-momentum, sixth generation (see k6_u): the w tile carries its x halo (70 columns), so the x-stencil is five ds_reads instead of
// five loads + five column divisions; the ring top, the own T / rho q values and u0 are loaded one level ahead; the raw rho_w of the
// own column rides a register delay line (advecting-flux ring and RK update).  Same arithmetic, same bits as k5_w.
// ---------------------------------------------------------------------------------------------------------------------
// BM: 4 the lean seam (w and the buoyancy inputs derived from the prognostic fields); 0 .. 3 the STORED-velocity instantiations (see Lean5 / k6_u)
// with the buoyancy modes of k_w_tend_lds (bz_tendency4_kernels.h), which they replace: 0 anelastic buoyancy from the stored T, q;
// 3 the same with the diagnosed q^v, q^l of saturation adjustment / the Kessler species; 5 its mixed-phase instantiation (q^l + q^i); 1 none; 2 the compressible slow vertical
// momentum G^s = G_adv - dz(p - p_r) - g Iz(rho - rho_r) with Lean5::bT = pressure, bq = total density (acoustic_substepping.jl:727-752)
template <int TY, bool WY = false, bool DRYQ = false, bool GUARD = true, int BM = 4>      // DRYQ: rho q identically zero (see k5_scalar_pair): its loads are skipped, every wavefront takes the dry Exner factor
__global__ __launch_bounds__(64 * TY, BZ6_W_WAVES) void k6_w(DevGrid g, Lean5 L, int kchunk, RKEpilogue E)
{
    constexpr bool ST = BM != 4;
    static_assert(!(ST && (WY || DRYQ || GUARD)), "stored-velocity instantiations: periodic / slab rows, no moisture-scan dispatch");
    if (bz_lean_skip<DRYQ, GUARD>(L)) return;
    constexpr int TR = TY + 6, TC = 72, NT = 64 * TY, NH = TR * 70 - TY * 64;
    static_assert(NH <= NT, "one frame cell per thread");
    __shared__ double T[2][TR][TC];
    __shared__ double FY[2][TY + 1][64];
    int bx, by, bz;
    bz_block5(L, bx, by, bz);
    const int tx = threadIdx.x, ty = threadIdx.y, t = ty * 64 + tx, tc = tx + 3;
    const int i0 = bx * 64, j0 = by * TY;
    const int i = i0 + tx, j = j0 + ty;
    const int ic = min(i, g.Nx + 2), jc = min(j, g.Ny + 2);
    const int nact = min(64, g.Nx - i0);
    const int ie = i0 + nact, le = nact - 1;
    const int kbeg = 1 + bz * kchunk, kend = min(kbeg + kchunk, g.Nz);
    if (kbeg >= kend) return;
    const ix32_t sz = (ix32_t)g.Sxy;
    const bool store = (i < g.Nx) && (j < g.Ny);
    const double *__restrict__ ru = L.ru, *__restrict__ rv = L.rv, *__restrict__ rw = L.rw;
    const double *__restrict__ pa = L.pa, *__restrict__ pb = L.pb;       // rho theta, rho q of the stage-start state
    const double *__restrict__ vel = ST ? L.vel : L.rw;                 // stored w (ST) — else unused
    const double *__restrict__ bT = L.bT, *__restrict__ bq = L.bq;       // ST: buoyancy inputs (stored fields)
    const Lev5 LV{L.lev};
    constexpr bool dryq = DRYQ;
    Tend3Fields F;
    F.ru = L.ru; F.rv = L.rv; F.rw = L.rw; F.u = F.v = F.w = F.T = F.q = nullptr; F.c = ST ? L.vel : nullptr; F.G = L.out;
    const double Az = g.Az;
    ix32_t n = (ix32_t)g.idx(ic, jc, kbeg);
    const bool hok = t < NH;
    int hr = 0, hc = 0;
    {
        const int h = hok ? t : 0;
        if (h < 6 * 70) { const int rr = h / 70; hc = h - rr * 70; hr = (rr < 3) ? rr : TY + rr; }
        else { const int hh = h - 6 * 70, rr = hh / 6, cc = hh - rr * 6; hr = 3 + rr; hc = (cc < 3) ? cc : 64 + cc; }
    }
    const ix32_t hn = (ix32_t)g.idx(min(i0 - 3 + hc, g.Nx + 2), min(j0 - 3 + hr, g.Ny + 2), kbeg);
    const ix32_t ntop0 = (ix32_t)g.idx(ic, min(j0 + TY, g.Ny), kbeg);
    const bool top = (ty == 0);

    double wr[6], qu[4], qv[4], qt[4], qw[4];       // qt: rho_v ring of the row above the tile (wave 0 only)
    double raw0 = 0.0, raw1 = 0.0, raw2 = 0.0;      // raw rho_w of the own column at levels k, k+1, k+2
#pragma unroll
    for (int s = 0; s < 6; ++s) {
        const double x = rw[n + s * sz - 3 * sz];
        wr[s] = ST ? vel[n + s * sz - 3 * sz] : bz_cdiv(x, LV.rho_f(kbeg + s - 3), LV.rrho_f(kbeg + s - 3));
        if (s >= 1 && s <= 4) qw[s - 1] = Az * x;   // levels kbeg-2 .. kbeg+1
        if (s == 3) raw0 = x;
        if (s == 4) raw1 = x;
        if (s == 5) raw2 = x;
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int kk = kbeg - 2 + s;
        const double Axk = ST ? g.Ax[kk] : LV.Ax(kk), Ayk = ST ? g.Ay[kk] : LV.Ay(kk);      // (compressible contexts have no packed level rows)
        qu[s] = Axk * ru[n + s * sz - 2 * sz];
        qv[s] = Ayk * rv[n + s * sz - 2 * sz];
        qt[s] = top ? Ayk * rv[ntop0 + s * sz - 2 * sz] : 0.0;
    }
    double fz_lo, b_lo, r_lo = 0.0;
    {
        const int B = bz_buffer_center(kbeg - 1, g.Nz);
        const double wt = (B == 3) ? bz_symm4(qw[0], qw[1], qw[2], qw[3]) : bz_symm2(qw[1], qw[2]);
        fz_lo = wt * bz_upB(wr[0], wr[1], wr[2], wr[3], wr[4], wr[5], wt > 0.0, B);
        if constexpr (BM == 4) b_lo = buoyancy5<dryq>(g, pa[n - sz], dryq ? 0.0 : pb[n - sz], kbeg - 1, LV.rho(kbeg - 1), LV.rrho(kbeg - 1), LV.pi(kbeg - 1), LV.T_r(kbeg - 1));
        else if constexpr (BM == 0) b_lo = buoyancy3(g, bT[n - sz], bq[n - sz], kbeg - 1);
        else if constexpr (BM == 3) b_lo = bz_buoyancy(g, bT, bq, (long long)(n - sz), kbeg - 1);
        else if constexpr (BM == 5) b_lo = bz_buoyancy<true>(g, bT, bq, (long long)(n - sz), kbeg - 1);
        else if constexpr (BM == 2) { b_lo = bT[n - sz] - g.p_r[kbeg - 1]; r_lo = bq[n - sz] - g.rho[kbeg - 1]; }
        else b_lo = 0.0;
    }
    T[0][ty + 3][tc] = wr[3];
    if (hok) T[0][hr][hc] = ST ? vel[hn] : bz_cdiv(rw[hn], LV.rho_f(kbeg), LV.rrho_f(kbeg));
    double tcur_raw = rw[n + 3 * sz];
    double tcur_v = ST ? vel[n + 3 * sz] : 0.0;
    double u0cur = (E.mode == 2) ? E.u0[n] : 0.0;
    __syncthreads();

    double edge = 0.0;
    int buf = 0;
    for (int k = kbeg; k < kend; ++k, n += sz) {
        const ix32_t lev = (ix32_t)(k - kbeg) * sz;
        // ---- prefetch for level k+1 ----
        const double p_h = hok ? (ST ? vel : rw)[hn + lev + sz] : 0.0;
        const double p_top = rw[n + ((k + 4 <= g.Nz + g.Hz) ? 4 * sz : 3 * sz)];
        const double p_topv = ST ? vel[n + ((k + 4 <= g.Nz + g.Hz) ? 4 * sz : 3 * sz)] : 0.0;
        const double Tcur = (BM == 1) ? 0.0 : (ST ? bT : pa)[n], rqcur = (BM == 1) ? 0.0 : ST ? bq[n] : dryq ? 0.0 : pb[n];          // rho theta, rho q (not read where the scan found it zero): consumed mid-level (buoyancy)
        const double p_u0 = (E.mode == 2) ? E.u0[n + sz] : 0.0;
        const double Axn = ST ? g.Ax[k + 2] : LV.Ax(k + 2), Ayn = ST ? g.Ay[k + 2] : LV.Ay(k + 2);
        const double qun = Axn * ru[n + 2 * sz], qvn = Ayn * rv[n + 2 * sz];
        const double qtn = top ? Ayn * rv[ntop0 + lev + 2 * sz] : 0.0;
        if (((k - kbeg) & (BZ5_EB - 1)) == 0) {
            const int kk = min(k + (tx & (BZ5_EB - 1)), kend - 1);
            edge = ST ? flux_x_at<T3_W>(g, F, ie, jc, kk) : flux_x_lean<T3_W>(g, F, rw, ie, jc, kk);
        }
        const int src = (k - kbeg) & (BZ5_EB - 1);
        const int Bf = bz_buffer_face(k, g.Nz);
        const double w0 = wr[3];
        // ST: the raw momentum of the own column is read where it is used (level k + 2 for the advecting flux, level k for the RK update)
        // instead of riding a three-level delay line: the stored-velocity ring top took its registers
        const double qwnew = Az * (ST ? rw[n + 2 * sz] : raw2);
        const double uold = ST ? rw[n] : raw0;
        const double(*Tk)[TC] = T[buf];
        const double *wrow = Tk[ty + 3] + tc;
        const double ut = (Bf == 3) ? bz_symm4(qu[0], qu[1], qu[2], qu[3]) : bz_symm2(qu[1], qu[2]);
        const double fx = ut * bz_up5(wrow[-3], wrow[-2], wrow[-1], w0, wrow[1], wrow[2], ut > 0.0);
        // flux at x-face i + 1: lane tx + 1 (DPP move) or, in the row's last lane le, lane `src` of the out-of-wave batch (v_readlane, src
        // wave-uniform); formed here, ahead of the level's barrier, which neither operand depends on.  Lane 63 receives 0 from the shift: it is
        // lane le (replaced) or a lane beyond a ragged row (store = false).
        double nb = bz_lane_down(fx);
        const double e = bz_lane_read(edge, src);
        if (tx == le) nb = e;
        const double dx = nb - fx;
        const double vt = (Bf == 3) ? bz_symm4(qv[0], qv[1], qv[2], qv[3]) : bz_symm2(qv[1], qv[2]);
        const double fy = vt * bz_up5y<WY>(Tk[ty][tc], Tk[ty + 1][tc], Tk[ty + 2][tc], w0, Tk[ty + 4][tc], Tk[ty + 5][tc], vt > 0.0, by5_face<WY>(g, __builtin_amdgcn_readfirstlane(j)));
        FY[buf][ty][tx] = fy;
        if (top) {
            const double v2 = (Bf == 3) ? bz_symm4(qt[0], qt[1], qt[2], qt[3]) : bz_symm2(qt[1], qt[2]);
            FY[buf][TY][tx] = v2 * bz_up5y<WY>(Tk[TY][tc], Tk[TY + 1][tc], Tk[TY + 2][tc], Tk[TY + 3][tc], Tk[TY + 4][tc], Tk[TY + 5][tc], v2 > 0.0,
                                               by5_face<WY>(g, j0 + TY));
        }
        const double wnew = ST ? tcur_v : bz_cdiv(tcur_raw, LV.rho_f(k + 3), LV.rrho_f(k + 3));
        double fz_hi;
        {
            const int B = bz_buffer_center(k, g.Nz);
            const double wt = (B == 3) ? bz_symm4(qw[1], qw[2], qw[3], qwnew) : bz_symm2(qw[2], qw[3]);
            fz_hi = wt * bz_upB(wr[1], wr[2], wr[3], wr[4], wr[5], wnew, wt > 0.0, B);
        }
        double b_hi = 0.0, r_hi = 0.0;
        if constexpr (BM == 4) b_hi = buoyancy5<dryq>(g, Tcur, rqcur, k, LV.rho(k), LV.rrho(k), LV.pi(k), LV.T_r(k));
        else if constexpr (BM == 0) b_hi = buoyancy3(g, Tcur, rqcur, k);
        else if constexpr (BM == 3) b_hi = bz_buoyancy(g, bT, bq, (long long)n, k);
        else if constexpr (BM == 5) b_hi = bz_buoyancy<true>(g, bT, bq, (long long)n, k);
        else if constexpr (BM == 2) { b_hi = Tcur - g.p_r[k]; r_hi = rqcur - g.rho[k]; }
        T[buf ^ 1][ty + 3][tc] = wr[4];
        if (hok) T[buf ^ 1][hr][hc] = ST ? p_h : bz_cdiv(p_h, LV.rho_f(k + 1), LV.rrho_f(k + 1));
        __syncthreads();
        {
            const double dy = FY[buf][ty + 1][tx] - fy;
            const double adv = -((ST ? g.Vinv_f[k] : LV.Vinv_f(k)) * (dx + dy + (fz_hi - fz_lo)));
            double Gval;
            if constexpr (BM == 2) Gval = adv - (b_hi - b_lo) * g.rdzf[k] - g.g * ((r_hi + r_lo) / 2.0);
            else if constexpr (BM == 1) Gval = adv;
            else Gval = adv + 0.5 * (b_lo + b_hi);
            if (store)
                L.out[n] = (ST && E.mode == 0) ? Gval : bz_rk_apply_pre(E.mode, E.dt, E.alpha, E.oma, u0cur, E.u0_out, Gval, uold, n);
        }
        fz_lo = fz_hi;
        b_lo = b_hi;
        r_lo = r_hi;
#pragma unroll
        for (int s = 0; s < 3; ++s) { qu[s] = qu[s + 1]; qv[s] = qv[s + 1]; qt[s] = qt[s + 1]; qw[s] = qw[s + 1]; }
        qu[3] = qun; qv[3] = qvn; qt[3] = qtn; qw[3] = qwnew;
        raw0 = raw1; raw1 = raw2; raw2 = tcur_raw;
        tcur_raw = p_top; u0cur = p_u0;
        if (ST) tcur_v = p_topv;
#pragma unroll
        for (int s = 0; s < 5; ++s) wr[s] = wr[s + 1];
        wr[5] = wnew;
        buf ^= 1;
    }
}
