"""Independent reference of the forcing, Coriolis, sponge and bottom-flux terms of the anelastic potential-temperature model, numpy in
np.longdouble, ONE ARRAY PER TERM so that each can be compared alone.  Written from the operator definitions, not from oracle/forcings.py
and not from csrc/bz_forcing.hip; it shares no code with oracle/ (the only import is the Geometry / written pair of
tests/advection_reference.py, whose conventions it keeps).  Breeze sources (relative to the reference checkout):

  SubsidenceForcing       src/Forcings/subsidence_forcing.jl:84-100 (w_dz at faces, the zb average with one-sided ends, the minus sign),
                          126-128 (Average(specific field, dims = (1, 2)))
  geostrophic_forcings    src/Forcings/geostrophic_forcings.jl (F_u = -f v_g, F_v = +f u_g: finished specific columns arrive here)
  SpecificForcing         src/Forcings/specific_forcing.jl:61-74 (rho_r at the field's own location times the specific forcing)
  energy forcing          src/PotentialTemperatureFormulations/potential_temperature_tendency.jl:86-104 (F_rho_e / (c_pm Pi))
  Coriolis                src/AtmosphereModels/dynamics_kernel_functions.jl:79,99 (- x_f_cross_U, - y_f_cross_U)
  call order, flux BCs    src/AtmosphereModels/update_atmosphere_model_state.jl:81-86 (compute_forcings!), 418-434 (compute_flux_bc_tendencies!)
  bulk conditions         src/BoundaryConditions/bulk_drag.jl (114-134), bulk_scalar_fluxes.jl (82-89, 123-138, 206-234),
                          BoundaryConditions.jl:67-85 (wind_speed^2 at fcc, cfc, ccc), thermodynamic_variable_bcs.jl (J_theta = Q / c_pm)
  friction-velocity drag  examples/bomex.jl:95-101, with the regulariser of benchmarking/src/convective_boundary_layer.jl:142-146
Oceananigans operators, restated from their published definitions: FPlane (x_f_cross_U = -f xy-average(V) at the u point, y_f_cross_U =
+f xy-average(U) at the v point), Relaxation (F = rate mask (target - field)), a bottom FluxBoundaryCondition J (G[i, j, 1] += J Az / V =
J / dz_c(1); field dependencies interpolated to the location of the condition), and the interpolations: the xy average to an x face (i, j)
takes the y faces (i-1, j), (i, j), (i-1, j+1), (i, j+1); to a y face (i, j) the x faces (i, j-1), (i+1, j-1), (i, j), (i+1, j).

CONVENTIONS (tests/advection_reference.py): inputs are halo-filled, halo-inclusive arrays (z, y, x); index 0 is the first interior entry; u on
x faces, v on y faces, w on z faces; a Flat y has Ny = 1, no halo, and every y interpolation is the identity.  Nothing here fills a halo or
adjusts to saturation: q^v, q^l of a saturation-adjustment model are inputs.  Columns (rho_r, p_r, profiles, rates, targets) have Nz entries
at centres, w_s, the w rate and the w target Nz + 1 at faces.  rho_f(k) = (rho_r(k-1) + rho_r(k)) / 2 on the interior faces.
Volume terms come back over the interior (w: faces 0 .. Nz - 1), bottom fluxes over the first level (Ny, Nx); entries the operator does
not write hold NaN: `written(geometry, field, shape)` — the u face i = 0 between x walls, the v face j = 0 between y walls, both w wall faces.

KEYWORD SWITCHES reproduce plausible kernel mistakes (tests/test_forcing_reference.py proves the cases can see each):
  subsidence_dzf_shift          dz_f of the neighbouring face in w_dz
  subsidence_ends_halved        the end cells average their one face with a zero face
  coriolis_two_point            the j + 1 (u point) / i + 1 (v point) pair of the average is dropped
  coriolis_same_sign            both components take the sign of the u component
  energy_dry_constants          R_d, c_pd instead of the mixture's R_m, c_pm
  drag_unaveraged_speed         the other momentum component at the same index instead of its four-point average
  bulk_square_of_mean           the square of the averaged velocity instead of the average of squares
  relaxation_w_centre_density   rho_r(k) instead of rho_f(k) for the specific-keyed w sponge
  bottom_dz_regular             Lz / Nz instead of dz_c of the first level
"""
from types import SimpleNamespace

import numpy as np

from advection_reference import Geometry, written          # noqa: F401  (re-exported: the conventions of that reference)

LD = np.longdouble

# ThermodynamicConstants defaults (src/Thermodynamics/thermodynamics_constants.jl): published numbers
CONSTANTS = SimpleNamespace(R=8.314462618, Md=0.02897, Mv=0.018015, cpd=1005.0, cpv=1850.0, cl=4181.0, Ll=2500800.0, T_energy=273.15,
                            Ttr=273.16, ptr=611.657)


def _gas(c):
    return LD(c.R) / LD(c.Md), LD(c.R) / LD(c.Mv)


def _sizes(geo, a):
    Hz, Hy, Hx = geo.H
    return geo.Nz, a.shape[1] - 2 * Hy, a.shape[2] - 2 * Hx


def _at(geo, a, dj=0, di=0, level=None):
    """interior of a centre-level array shifted by (dj, di), in long double; level: one level only (-> (Ny, Nx))"""
    Hz, Hy, Hx = geo.H
    Nz, Ny, Nx = _sizes(geo, a)
    if geo.flat_y:
        dj = 0
    ys, xs = slice(Hy + dj, Hy + dj + Ny), slice(Hx + di, Hx + di + Nx)
    if level is None:
        return np.asarray(a[Hz:Hz + Nz, ys, xs], dtype=LD)
    return np.asarray(a[Hz + level, ys, xs], dtype=LD)


def _col(p):
    return np.asarray(p, dtype=LD)[:, None, None]


def _mask(geo, field, out):
    """NaN outside the cells the operator writes; `out` over the interior (3-D) or the first level (2-D)"""
    if out.ndim == 3:
        keep = np.zeros(out.shape, dtype=bool)
        keep[written(geo, field, out.shape)] = True
    else:
        keep = np.zeros(out.shape, dtype=bool)
        _, ys, xs = written(geo, field, (geo.Nz,) + out.shape)
        keep[ys, xs] = True
    out = out.copy()
    out[~keep] = LD("nan")
    return out


def _to_u_point(geo, a, level=None, two_point=False, square=False):
    """four-point xy average of a y-face field to the x face (i, j): (i-1, j), (i, j), (i-1, j+1), (i, j+1)"""
    f = (lambda x: x * x) if square else (lambda x: x)
    at = lambda dj, di: f(_at(geo, a, dj, di, level))
    if two_point:
        return (at(0, -1) + at(0, 0)) / 2
    return ((at(0, -1) + at(1, -1)) / 2 + (at(0, 0) + at(1, 0)) / 2) / 2


def _to_v_point(geo, a, level=None, two_point=False, square=False):
    """four-point xy average of an x-face field to the y face (i, j): (i, j-1), (i+1, j-1), (i, j), (i+1, j)"""
    f = (lambda x: x * x) if square else (lambda x: x)
    at = lambda dj, di: f(_at(geo, a, dj, di, level))
    if two_point:
        return (at(-1, 0) + at(0, 0)) / 2
    return ((at(-1, 0) + at(-1, 1)) / 2 + (at(0, 0) + at(0, 1)) / 2) / 2


# ---- Coriolis -----------------------------------------------------------------------------------------------------------------------------
def coriolis(geo, f, ru, rv, coriolis_two_point=False, coriolis_same_sign=False):
    """(- x_f_cross_U, - y_f_cross_U) = (+f xy-average(rho v) at the u point, -f xy-average(rho u) at the v point)"""
    f = LD(f)
    tu = f * _to_u_point(geo, rv, two_point=coriolis_two_point)
    tv = (f if coriolis_same_sign else -f) * _to_v_point(geo, ru, two_point=coriolis_two_point)
    return _mask(geo, "u", tu), _mask(geo, "v", tv)


# ---- column profiles ----------------------------------------------------------------------------------------------------------------------
def column_term(geo, field, rho, profile, shape):
    """rho_r(k) F(k) over the interior of `field` in "u", "v", "c" (shape: the interior's)"""
    return _mask(geo, field, np.broadcast_to(_col(rho) * _col(profile), shape).astype(LD))


def mixture(c, q=None, qv=None, ql=None):
    """(R_m, c_pm) from q (no microphysics: vapour only) or from q^v, q^l (saturation adjustment)"""
    Rd, Rv = _gas(c)
    if qv is None:
        qv, ql = q, LD(0) * q
    qd = 1 - (qv + ql)
    return qd * Rd + qv * Rv, qd * LD(c.cpd) + qv * LD(c.cpv) + ql * LD(c.cl)


def energy_forcing(geo, rho, p_r, pst, Fe, c, q=None, qv=None, ql=None, energy_dry_constants=False):
    """rho_r F_e / (c_pm Pi), Pi = (p_r / p_st)^(R_m / c_pm)"""
    moist = qv is not None
    Rm, cpm = mixture(c, None if moist else _at(geo, q), _at(geo, qv) if moist else None, _at(geo, ql) if moist else None)
    if energy_dry_constants:
        Rm, cpm = _gas(c)[0] + 0 * Rm, LD(c.cpd) + 0 * cpm
    Pi = (_col(p_r) / LD(pst)) ** (Rm / cpm)
    return (_col(rho) * _col(Fe)) / (cpm * Pi)


# ---- subsidence ---------------------------------------------------------------------------------------------------------------------------
def horizontal_average(geo, a):
    """Average(field, dims = (1, 2)) over the interior -> Nz values"""
    return _at(geo, a).mean(axis=(1, 2), dtype=LD)


def subsidence_profile(geo, ws, avg, subsidence_dzf_shift=False, subsidence_ends_halved=False):
    """F(k) = - zb-average of w_dz, w_dz(k) = w_s[k] (avg[k] - avg[k-1]) / dz_f(k) on faces 1 .. Nz - 1: interior cells take the mean of their
    two faces, the bottom cell the face above only, the top cell the face below only"""
    Nz = geo.Nz
    ws, avg = np.asarray(ws, dtype=LD), np.asarray(avg, dtype=LD)
    wdz = np.zeros(Nz + 1, dtype=LD)
    for k in range(1, Nz):
        kk = k
        if subsidence_dzf_shift:
            kk = k + 1 if k + 1 <= Nz - 1 else k - 1
        wdz[k] = ws[k] * (avg[k] - avg[k - 1]) / geo.dzf_[kk]
    out = np.empty(Nz, dtype=LD)
    for k in range(Nz):
        if k == Nz - 1:
            out[k] = wdz[k] / 2 if subsidence_ends_halved else wdz[k]
        elif k == 0:
            out[k] = wdz[1] / 2 if subsidence_ends_halved else wdz[1]
        else:
            out[k] = (wdz[k + 1] + wdz[k]) / 2
    return -out


# ---- Relaxation and the field forcing -------------------------------------------------------------------------------------------------------
def face_density(rho):
    """rho_f on faces 0 .. Nz - 1 (face 0 is a wall: NaN)"""
    rho = np.asarray(rho, dtype=LD)
    out = np.full(rho.size, LD("nan"))
    out[1:] = (rho[:-1] + rho[1:]) / 2
    return out


def relaxation(geo, field, rate, target, a, rho=None, relaxation_w_centre_density=False):
    """rate(k) (target(k) - a) over the interior of `field` in "u", "v", "w", "c"; rho: the reference column for a specific key (a is then
    the specific field and the term carries rho_r at the field's location), None for a density key.  w: rate and target hold Nz + 1 face
    values, the result faces 0 .. Nz - 1."""
    Nz = geo.Nz
    x = _at(geo, a)          # w: levels 0 .. Nz - 1 of a face array are its faces 0 .. Nz - 1
    r, t = np.asarray(rate, dtype=LD)[:Nz], np.asarray(target, dtype=LD)[:Nz]
    F = _col(r) * (_col(t) - x)
    if rho is not None:
        dens = np.asarray(rho, dtype=LD) if (field != "w" or relaxation_w_centre_density) else face_density(rho)
        F = _col(dens) * F
    return _mask(geo, field, F)


def field_forcing(geo, F, specific, rho):
    """Forcing(F(x, y, z)) on the thermodynamic variable: keyed theta it is specific (rho_r F), keyed rho theta it is F; F over the interior"""
    F = np.asarray(F, dtype=LD)
    return _col(rho) * F if specific else F.copy()


# ---- bottom fluxes: J / dz_c(1) over the first level ------------------------------------------------------------------------------------------
def bottom_dz(geo, Lz=None, bottom_dz_regular=False):
    return LD(Lz) / geo.Nz if bottom_dz_regular else geo.dzc[0]


def constant_flux(geo, J, shape, dz):
    return np.full(shape, LD(J) / dz)


def energy_flux(geo, Q, c, dz, q=None, qv=None, ql=None):
    """an energy flux Q keyed rho e in a potential-temperature model: J_theta = Q / c_pm of the lowest cell"""
    moist = qv is not None
    _, cpm = mixture(c, None if moist else _at(geo, q, level=0), _at(geo, qv, level=0) if moist else None,
                     _at(geo, ql, level=0) if moist else None)
    return (LD(Q) / cpm) / dz


def friction_drag(geo, rho0_ustar2, epsilon, ru, rv, dz, drag_unaveraged_speed=False):
    """J_u = -rho_0 u*^2 rho u / sqrt(rho u^2 + <rho v>^2 + eps) at the u point, J_v likewise at the v point"""
    D, e = LD(rho0_ustar2), LD(epsilon)
    u, v = _at(geo, ru, level=0), _at(geo, rv, level=0)
    v_u = v if drag_unaveraged_speed else _to_u_point(geo, rv, level=0)
    u_v = u if drag_unaveraged_speed else _to_v_point(geo, ru, level=0)
    Ju = -D * u / np.sqrt(u * u + v_u * v_u + e)
    Jv = -D * v / np.sqrt(u_v * u_v + v * v + e)
    return _mask(geo, "u", Ju / dz), _mask(geo, "v", Jv / dz)


def saturation_specific_humidity(T, rho, c):
    """q^v+(T, rho) over a planar liquid surface: Clausius-Clapeyron vapour pressure / (rho R_v T)"""
    _, Rv = _gas(c)
    T, dc = LD(T), LD(c.cpv) - LD(c.cl)
    L0 = LD(c.Ll) - dc * LD(c.T_energy)
    ps = LD(c.ptr) * (T / LD(c.Ttr)) ** (dc / Rv) * np.exp((1 / LD(c.Ttr) - 1 / T) * L0 / Rv)
    return ps / (LD(rho) * Rv * T)


def bulk_fluxes(geo, c, p0, pst, u, v, theta, qv, dz, drag=None, heat=None, vapor=None, bulk_square_of_mean=False):
    """BulkDrag / BulkSensibleHeatFlux / BulkVaporFlux with constant coefficients; each of drag, heat, vapor: None or (coefficient,
    gustiness, surface temperature).  -> {"u", "v", "theta", "q"}: J / dz of the conditions that are present.
      J_u = -rho_0 C U~ u at the x face, U~^2 = u^2 + xy-average(v^2) + gustiness^2;  J_v likewise
      J_theta = -rho_0 C U~ (theta - theta_0), J_q = -rho_0 C U~ (q^v - q^v+(T_0, rho_0)) at centres, U~^2 = x-average(u^2) + y-average(v^2)
      + gustiness^2;  rho_0 = p_0 / (R_d T_0), theta_0 = T_0 / (p_0 / p_st)^(R_d / c_pd), each from the condition's own T_0"""
    Rd, _ = _gas(c)
    out = {}
    u0, v0 = _at(geo, u, level=0), _at(geo, v, level=0)
    sq = lambda x: x * x
    if drag is not None:
        C, gust, T0 = (LD(x) for x in drag)
        rho0 = LD(p0) / (Rd * T0)
        if bulk_square_of_mean:
            v2, u2 = sq(_to_u_point(geo, v, level=0)), sq(_to_v_point(geo, u, level=0))
        else:
            v2, u2 = _to_u_point(geo, v, level=0, square=True), _to_v_point(geo, u, level=0, square=True)
        out["u"] = _mask(geo, "u", (-rho0 * C * np.sqrt(sq(u0) + v2 + sq(gust)) * u0) / dz)
        out["v"] = _mask(geo, "v", (-rho0 * C * np.sqrt(u2 + sq(v0) + sq(gust)) * v0) / dz)
    if heat is not None or vapor is not None:
        ue, vn = _at(geo, u, 0, 1, level=0), _at(geo, v, 1, 0, level=0)
        U2 = sq((u0 + ue) / 2) + sq((v0 + vn) / 2) if bulk_square_of_mean else (sq(u0) + sq(ue)) / 2 + (sq(v0) + sq(vn)) / 2
    if heat is not None:
        C, gust, T0 = (LD(x) for x in heat)
        rho0 = LD(p0) / (Rd * T0)
        theta0 = T0 / (LD(p0) / LD(pst)) ** (Rd / LD(c.cpd))
        out["theta"] = (-rho0 * C * np.sqrt(U2 + sq(gust)) * (_at(geo, theta, level=0) - theta0)) / dz
    if vapor is not None:
        C, gust, T0 = (LD(x) for x in vapor)
        rho0 = LD(p0) / (Rd * T0)
        out["q"] = (-rho0 * C * np.sqrt(U2 + sq(gust)) * (_at(geo, qv, level=0) - saturation_specific_humidity(T0, rho0, c))) / dz
    return out
