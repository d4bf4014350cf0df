"""Plain numpy restatement of the output diagnostics behind bz_compute_diagnostics (csrc/bz_diagnostics.hip), one function per kind,
built on oracle/thermo.py (constants, mixture properties, secant_solve).  Formulas as the reference writes them:
  potential temperatures   src/AtmosphereModels/Diagnostics/potential_temperatures.jl:538-616
  static energy            src/AtmosphereModels/Diagnostics/static_energy.jl:94-120
  relative humidity        src/Microphysics/microphysics_diagnostics.jl:139-170
  saturation humidities    src/AtmosphereModels/Diagnostics/saturation_specific_humidity.jl:111-149, src/Thermodynamics/vapor_saturation.jl:216-230
  dewpoint                 src/Thermodynamics/vapor_saturation.jl:313-331
Every function takes arrays of one dtype (T, qv, ql, p of the cells; rho, z, qe where used) and constants from `constants(dtype)`, and
computes in that dtype: Float64 is the reference of the device tests, np.float32 measures the formulas' own Float32 error.  The module
imports neither torch nor the package under test."""
import numpy as np

from oracle import thermo

NAMES = ("POTENTIAL_TEMPERATURE", "LIQUID_ICE_POTENTIAL_TEMPERATURE", "VIRTUAL_POTENTIAL_TEMPERATURE",
         "EQUIVALENT_POTENTIAL_TEMPERATURE", "STABILITY_EQUIVALENT_POTENTIAL_TEMPERATURE", "STATIC_ENERGY",
         "RELATIVE_HUMIDITY", "SATURATION_SPECIFIC_HUMIDITY", "SATURATION_SPECIFIC_HUMIDITY_EQUILIBRIUM",
         "SATURATION_SPECIFIC_HUMIDITY_TOTAL_MOISTURE", "DEWPOINT_TEMPERATURE")
DENSITY_FLAVOURED = NAMES[:6]


class _Typed:
    pass


def constants(dtype=np.float64, pst=1e5, **kw):
    """oracle.thermo.ThermoConstants with every value a scalar of `dtype` (so that nothing is promoted), plus the standard pressure."""
    c0, c = thermo.ThermoConstants(**kw), _Typed()
    real = np.dtype(dtype).type
    for k, v in vars(c0).items():
        setattr(c, k, real(v))
    c.Rd, c.Rv = c.R / c.Md, c.R / c.Mv
    c.pst = real(pst)
    c.real = real
    return c


def mixture(qv, ql, c):
    """(R_m, c_pm) of q = (qv, ql, 0)"""
    zero = c.real(0)
    return thermo.mixture_gas_constant(qv, ql, zero, c), thermo.mixture_heat_capacity(qv, ql, zero, c)


def saturation_vapor_pressure(T, c):
    """Clausius-Clapeyron over a planar liquid surface: oracle.thermo.saturation_vapor_pressure on arrays"""
    dc = c.cpv - c.cl
    L0 = c.Ll - dc * c.T_energy
    return c.ptr * (T / c.Ttr) ** (dc / c.Rv) * np.exp((1 / c.Ttr - 1 / T) * L0 / c.Rv)


def vapor_pressure(T, qv, ql, p, c):
    Rm, _ = mixture(qv, ql, c)
    rho = p / (Rm * T)
    return rho * qv * c.Rv * T


def potential_temperature(T, qv, ql, p, c):
    Rm, cpm = mixture(qv, ql, c)
    return T / (p / c.pst) ** (Rm / cpm)


def liquid_ice_potential_temperature(T, qv, ql, p, c):
    _, cpm = mixture(qv, ql, c)
    return potential_temperature(T, qv, ql, p, c) * (1 - c.Ll * ql / (cpm * T))


def virtual_potential_temperature(T, qv, ql, p, c):
    return T / (p / c.pst) ** (c.Rd / c.cpd) * (1 + (c.Rv / c.Rd - 1) * qv - ql)


def equivalent_potential_temperature(T, qv, ql, p, c):
    _, cpm = mixture(qv, ql, c)
    H = vapor_pressure(T, qv, ql, p, c) / saturation_vapor_pressure(T, c)
    Ll = c.Ll + (c.cpv - c.cl) * (T - c.T_energy)
    with np.errstate(divide="ignore"):
        return T * (c.pst / p) ** (c.Rd / cpm) * np.exp(Ll * qv / (cpm * T)) * H ** (-c.Rv * qv / cpm)


def stability_equivalent_potential_temperature(T, qv, ql, p, c):
    _, cpm = mixture(qv, ql, c)
    return equivalent_potential_temperature(T, qv, ql, p, c) * (T / c.T_energy) ** (c.cl * ql / cpm)


def static_energy(T, qv, ql, z, c):
    _, cpm = mixture(qv, ql, c)
    return cpm * T + c.g * z - c.Ll * ql


def relative_humidity(T, qv, ql, p, c):
    ps = saturation_vapor_pressure(T, c)
    return vapor_pressure(T, qv, ql, p, c) / np.maximum(ps, np.finfo(ps.dtype).eps)


def saturation_specific_humidity(T, qv, ql, p, c):
    Rm, _ = mixture(qv, ql, c)
    rho = p / (Rm * T)
    return saturation_vapor_pressure(T, c) / (rho * c.Rv * T)


def saturation_specific_humidity_equilibrium(T, qe, p, c):
    ps = saturation_vapor_pressure(T, c)
    eps = c.Rd / c.Rv
    q1 = eps * (1 - qe) * ps / (p - ps)
    rho = p / ((c.Rd * (1 - qe) + c.Rv * qe) * T)
    q0 = ps / (rho * c.Rv * T)
    return np.where(qe >= q0, q1, q0)


def saturation_specific_humidity_total_moisture(T, p, c):
    ps = saturation_vapor_pressure(T, c)
    eps = c.Rd / c.Rv
    return eps * ps / (p + (eps - 1) * ps)


def dewpoint_temperature(T, qv, ql, p, c):
    """Float64, cell by cell through oracle.thermo.secant_solve(reltol = 1e-4, abstol = 0, maxiter = 10, scale = p^v)"""
    tc = thermo.ThermoConstants()
    for k, v in vars(tc).items():
        setattr(tc, k, float(getattr(c, k)))
    pv = vapor_pressure(T, qv, ql, p, c)
    out = np.empty(T.shape, np.float64)
    for idx in np.ndindex(T.shape):
        Tk, pvk = float(T[idx]), float(pv[idx])
        ps1 = thermo.saturation_vapor_pressure(Tk, tc, "liquid")
        if ps1 - pvk <= 0:
            out[idx] = Tk
            continue
        T2 = Tk - (1 - pvk / ps1) * 20
        try:
            out[idx] = thermo.secant_solve(lambda x: thermo.saturation_vapor_pressure(x, tc, "liquid") - pvk, Tk, T2, pvk,
                                           reltol=1e-4, abstol=0.0, maxiter=10)
        except (ValueError, OverflowError, ZeroDivisionError, TypeError):      # p^v = 0: the iteration leaves the positive temperatures
            out[idx] = np.nan
    return out


def evaluate(name, T, qv, ql, p, rho, z, qe, c):
    """Kind `name` (optionally prefixed "DENSITY_") on cell arrays; z broadcasts against T."""
    dens = name.startswith("DENSITY_")
    base = name[len("DENSITY_"):] if dens else name
    if base == "STATIC_ENERGY":
        v = static_energy(T, qv, ql, z, c)
    elif base == "SATURATION_SPECIFIC_HUMIDITY_EQUILIBRIUM":
        v = saturation_specific_humidity_equilibrium(T, qe, p, c)
    elif base == "SATURATION_SPECIFIC_HUMIDITY_TOTAL_MOISTURE":
        v = saturation_specific_humidity_total_moisture(T, p, c)
    else:
        v = {"POTENTIAL_TEMPERATURE": potential_temperature, "LIQUID_ICE_POTENTIAL_TEMPERATURE": liquid_ice_potential_temperature,
             "VIRTUAL_POTENTIAL_TEMPERATURE": virtual_potential_temperature,
             "EQUIVALENT_POTENTIAL_TEMPERATURE": equivalent_potential_temperature,
             "STABILITY_EQUIVALENT_POTENTIAL_TEMPERATURE": stability_equivalent_potential_temperature,
             "RELATIVE_HUMIDITY": relative_humidity, "SATURATION_SPECIFIC_HUMIDITY": saturation_specific_humidity,
             "DEWPOINT_TEMPERATURE": dewpoint_temperature}[base](T, qv, ql, p, c)
    return rho * v if dens else v
