// bz_closure_carriers.h — where the closure kernels (bz_closure.hip, bz_diffusivity.hip) take the density of a flux location and the
// Exner factor of theta_v from.  One set of flux expressions serves both models: the kernels are templates on these carriers.
//   anelastic     the reference column: rho_r[k] at centres / corners of a level, rho_r at the z faces; (pst / p_r[k])^(Rd/cpd) from a table
//   compressible  the model's own 3-D fields (dynamics_density = rho_d for momentum and rho theta, the total density for water;
//                 dynamics_pressure in theta_v): the cell value at ccc, two- and four-point means of the field at faces and edges in the
//                 order of the nu averages of bz_closure.hip, read through the field's halos (periodic images in x / y, the zero-gradient
//                 first cell in z)          src/TurbulenceClosures/TurbulenceClosures.jl:65-101 of the reference
// `n` is the index of the cell that shares its index with the location (an x face i and the cell i to its right, ...), `k` its level.
#pragma once
#include "bz_internal.h"

#ifdef __HIPCC__
struct RhoColumn {
    static constexpr bool field = false;
    __device__ __forceinline__ double ccc(const DevGrid &g, long long, int k) const { return g.rho[k]; }
    __device__ __forceinline__ double fcc(const DevGrid &g, long long, int k) const { return g.rho[k]; }
    __device__ __forceinline__ double cfc(const DevGrid &g, long long, int k) const { return g.rho[k]; }
    __device__ __forceinline__ double ffc(const DevGrid &g, long long, int k) const { return g.rho[k]; }
    __device__ __forceinline__ double ccf(const DevGrid &g, long long, int k) const { return g.rho_f[k]; }
    __device__ __forceinline__ double fcf(const DevGrid &g, long long, int k) const { return g.rho_f[k]; }
    __device__ __forceinline__ double cff(const DevGrid &g, long long, int k) const { return g.rho_f[k]; }
};

struct RhoField {
    static constexpr bool field = true;
    const double *__restrict__ r;
    __device__ __forceinline__ double ccc(const DevGrid &, long long n, int) const { return r[n]; }
    __device__ __forceinline__ double fcc(const DevGrid &, long long n, int) const { return (r[n - 1] + r[n]) / 2; }
    __device__ __forceinline__ double cfc(const DevGrid &g, long long n, int) const { return (r[n - g.Sx] + r[n]) / 2; }
    __device__ __forceinline__ double ccf(const DevGrid &g, long long n, int) const { return (r[n - g.Sxy] + r[n]) / 2; }
    __device__ __forceinline__ double ffc(const DevGrid &g, long long n, int) const
    {
        const long long sy = g.Sx;
        return ((r[n - 1 - sy] + r[n - sy]) / 2 + (r[n - 1] + r[n]) / 2) / 2;
    }
    __device__ __forceinline__ double fcf(const DevGrid &g, long long n, int) const
    {
        const long long sz = g.Sxy;
        return ((r[n - 1 - sz] + r[n - sz]) / 2 + (r[n - 1] + r[n]) / 2) / 2;
    }
    __device__ __forceinline__ double cff(const DevGrid &g, long long n, int) const
    {
        const long long sy = g.Sx, sz = g.Sxy;
        return ((r[n - sy - sz] + r[n - sz]) / 2 + (r[n - sy] + r[n]) / 2) / 2;
    }
};

// (pst / p)^(Rd/cpd) of theta_v = R_m / R_d T (pst / p)^(Rd/cpd) at a cell (atmosphere_model_buoyancy.jl:59-68: dynamics_pressure)
struct ExnerColumn {      // ipi[k], k = -1 .. Nz (k_inverse_exner_column)
    static constexpr int kchunk = 1;      // levels a workgroup of k_smagorinsky_viscosity walks (the strain loads bound it, not the logarithms)
    const double *__restrict__ ipi;
    __device__ __forceinline__ double at(const DevGrid &, long long, int k) const { return ipi[k]; }
};
struct ExnerField {       // the model's 3-D pressure (zero-gradient first halo cell in z)
    static constexpr int kchunk = 8;      // ... here a cell's log(theta_v) costs a pow as well: the ring of three evaluates 10 per 8 cells
    const double *__restrict__ p;
    __device__ __forceinline__ double at(const DevGrid &g, long long n, int) const { return pow(g.pst / p[n], g.Rd / g.cpd); }
};
#endif
