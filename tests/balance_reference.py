"""numpy restatement of the discrete hydrostatic balance of the compressible model's initial and base state (csrc/bz_balance.hip), after
the reference's src/Thermodynamics/reference_states.jl:572-672 (moist_reference_constants, newton_hydrostatic_pressure,
_compute_exner_column!, integrate_exner_column!) and src/AtmosphereModels/set_to_mean.jl:53-110,271-310 (the rescaling kernels and
set_hydrostatically_balanced_density!).  Pinned by tests/test_balance_reference.py.

Arrays are (Nz, ...) with z first; every trailing axis is a column index, so one call integrates a profile, a row or a whole (Nz, Ny, Nx)
field.  All arithmetic runs in `dtype` (float64, longdouble or float32): constants and metrics are cast first, so that nothing is promoted."""
import numpy as np


def constants_tuple(c):
    """(g, Rd, Rv, cpd, cpv) of a ThermodynamicConstants as Python floats"""
    from breeze_jl_amd.thermodynamics import dry_air_gas_constant, vapor_gas_constant
    return (c.gravitational_acceleration, dry_air_gas_constant(c), vapor_gas_constant(c), c.dry_air_heat_capacity, c.vapor_heat_capacity)


def z_metrics(zf):
    """Δzᶜ (Nz) and Δzᶠ (Nz + 1; entries 1 .. Nz - 1 are the interior faces) of face heights zf (Nz + 1), as Oceananigans defines them"""
    zf = np.asarray(zf, dtype=np.float64)
    zc = 0.5 * (zf[:-1] + zf[1:])
    dzf = np.empty(len(zf))
    dzf[1:-1] = np.diff(zc)
    dzf[0] = 2 * (zc[0] - zf[0])
    dzf[-1] = 2 * (zf[-1] - zc[-1])
    return np.diff(zf), dzf


def exner_columns(theta, qv, dzc, dzf, p0, pst, constants, dtype=np.float64):
    """_compute_exner_column! for every column of theta, qv (shape (Nz, ...)): (exner, pressure, density) in `dtype`."""
    T = np.dtype(dtype).type
    g, Rd, Rv, cpd, cpv = (T(x) for x in constants)
    p0, pst = T(p0), T(pst)
    one, two = T(1), T(2)
    th = np.asarray(theta, dtype=dtype)
    q = np.zeros_like(th) if qv is None else np.asarray(qv, dtype=dtype)
    dzc = np.asarray(dzc, dtype=dtype)
    dzf = np.asarray(dzf, dtype=dtype)
    Nz = th.shape[0]
    Pi, p, rho = np.zeros_like(th), np.zeros_like(th), np.zeros_like(th)

    def moist(qk):      # moist_reference_constants
        qd = one - qk
        Rm, cpm = qd * Rd + qk * Rv, qd * cpd + qk * cpv
        return Rm, cpm, Rm / cpm

    Rm, cpm, kap = moist(q[0])
    Pi[0] = (p0 / pst) ** kap - g * dzc[0] / (two * cpm * th[0])
    p[0] = pst * Pi[0] ** (one / kap)
    rho[0] = p[0] / (Rm * th[0] * Pi[0])
    for k in range(1, Nz):
        Rm, cpm, kap = moist(q[k])
        th_face = (th[k] + th[k - 1]) / two
        pk = pst * (Pi[k - 1] - g * dzf[k] / (cpm * th_face)) ** (one / kap)
        A = g * pst ** kap / (two * Rm * th[k])
        Cc = p[k - 1] / dzf[k] - g * rho[k - 1] / two
        for _ in range(5):      # FixedIterations(5)
            rp = pk ** (-kap)
            f = pk / dzf[k] + A * pk * rp - Cc
            df = one / dzf[k] + A * (one - kap) * rp
            pk = pk - f / df
        p[k] = pk
        Pi[k] = (pk / pst) ** kap
        rho[k] = pk / (Rm * th[k] * Pi[k])
    return Pi, p, rho


def balance_ratio(p, rho, dzf, g, eps):
    """max over interior faces and columns of |(p[k]-p[k-1])/Δzᶠ[k] + g (ρ[k]+ρ[k-1])/2| / (eps p[k-1]/Δzᶠ[k]), evaluated in longdouble on the
    values as they are stored; 0 for a single level."""
    L = np.longdouble
    p, rho = np.asarray(p).astype(L), np.asarray(rho).astype(L)
    if p.shape[0] < 2:
        return 0.0
    dz = np.asarray(dzf).astype(L)[1:p.shape[0]].reshape((-1,) + (1,) * (p.ndim - 1))
    res = np.abs((p[1:] - p[:-1]) / dz + L(g) * (rho[1:] + rho[:-1]) / 2)
    return float(np.max(res / (L(eps) * p[:-1] / dz)))


def max_rel(a, b):
    """max |a - b| / |b| in longdouble"""
    a, b = np.asarray(a).astype(np.longdouble), np.asarray(b).astype(np.longdouble)
    return float(np.max(np.abs(a - b) / np.abs(b)))


def _face_mean(a, axis):
    return (a + np.roll(a, 1, axis=axis)) / 2      # ℑxᶠᵃᵃ / ℑyᵃᶠᵃ on a periodic axis: cells i - 1 and i


def condensate(state, kessler):
    """total_condensate_density: ρqᵛᵉ + Σ species, in the association of the device's total density"""
    if kessler:
        return state["rq"] + (state["rqcl"] + (state["rqr"] + 0))
    return state["rq"] + 0


def balanced_set(state, theta, dzc, dzf, p0, pst, constants, kessler=False, flat_y=False, dtype=np.float64):
    """set_hydrostatically_balanced_density! on interior arrays (Nz, Ny, Nx) in `dtype`, periodic in x and y (flat_y: the y mean is the
    identity).  state: rho_d, ru, rv, rth, rq (centres in z), rw (Nz + 1 faces) and, with kessler, rqcl, rqr; theta: the specific θˡⁱ the
    preceding update_state! left.  Returns the new state with "rho" (total), "p_column" and "rho_column" (the integration's own)."""
    state = {k: np.asarray(v).astype(dtype) for k, v in state.items()}
    theta = np.asarray(theta).astype(dtype)
    old = state["rho_d"]
    qv = state["rq"] / old                                          # _dry_weighted_specific_moisture!
    _, p_col, rho = exner_columns(theta, qv, dzc, dzf, p0, pst, constants, dtype=dtype)
    out = {k: np.array(v) for k, v in state.items()}
    ratio = rho / old                                               # scale_total_density_weighted_fields!
    out["rq"] = state["rq"] * ratio
    if kessler:
        out["rqcl"], out["rqr"] = state["rqcl"] * ratio, state["rqr"] * ratio
    new = rho - condensate(out, kessler)                            # _set_dry_density_from_total_density!
    out["rho_d"] = new
    out["ru"] = state["ru"] * (_face_mean(new, 2) / _face_mean(old, 2))      # _rescale_momentum!
    out["rv"] = state["rv"] * (new / old if flat_y else _face_mean(new, 1) / _face_mean(old, 1))
    Nz = old.shape[0]
    out["rw"][1:Nz] = state["rw"][1:Nz] * (((new[1:] + new[:-1]) / 2) / ((old[1:] + old[:-1]) / 2))      # wall faces keep their values
    out["rth"] = state["rth"] * (new / old)
    out["rho"] = new + condensate(out, kessler)
    out["p_column"], out["rho_column"] = p_col, rho
    return out
