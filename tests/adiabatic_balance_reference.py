"""The adiabatic balance (balance_adiabatically!, src/AtmosphereModels/adiabatic_balance.jl:44-86) composed from the oracle models' own
pieces: time_step(+dt) and time_step(-dt), numpy nudges over whole parent arrays and update_state.  It is the reference the device loop
(csrc/bz_adiabatic_balance.hip) is compared with, and the set-ups of the reference's tests (test/balance_adiabatically.jl) on the oracle."""
import numpy as np

T_ISO = 250.0      # the isothermal reference of test/balance_adiabatically.jl:25-28


def iso_theta(constants):
    """theta_r(z) of an isothermal column at T_ISO: T_ISO exp(g z / (cpd T_ISO))."""
    g, cpd = constants.g, constants.cpd
    return lambda z: T_ISO * np.exp(g * z / (cpd * T_ISO))


def initial_names(om):
    """Names of the oracle arrays that are nudged: every prognostic field but rho w (and the Kessler species, which the balance does not
    carry)."""
    return tuple(n for n in om.PROGNOSTIC if n not in ("rw", "rqcl", "rqr"))


def snapshot(om):
    return {n: getattr(om, n).copy() for n in initial_names(om)}


def nudge(om, snap, weight):
    """x <- (x + weight x0) / (1 + weight) over whole arrays, in the arrays' precision."""
    for n, x0 in snap.items():
        x = getattr(om, n)
        w = x.dtype.type(weight)
        x[...] = (x + w * x0) / (1 + w)


def balance(om, dt, cycles=1, weight=2.0):
    """balance_adiabatically!(model; dt, cycles, weight) on an oracle model (anelastic or compressible); the halo fills of the nudged fields
    are those update_state opens with.  The clock is reset."""
    snap = snapshot(om)
    for _ in range(cycles):
        for s in (1.0, -1.0):
            om.time_step(s * dt)
            om.time_step(-s * dt)
            nudge(om, snap, weight)
            om.update_state(compute_tendencies=True)
    om.iteration, om.clock_time = 0, 0.0
    return om


# ---- the reference's test set-ups on the oracle ---------------------------------------------------------------------------------------
REST_SIZE, REST_HALO = (8, 8, 32), (5, 5, 5)
REST_EXTENT = dict(x=(0.0, 100e3), y=(0.0, 100e3), z=(0.0, 10e3))


def compressible_rest_oracle(orc, oc, size=REST_SIZE, halo=REST_HALO, **td):
    """_build_adiabatic_model + _set_discrete_rest! (test/balance_adiabatically.jl:32-62): the isothermal reference at 250 K, p0 = pst = 1e5,
    no sponge; rho_d = rho_ref, rho theta = p_ref / (R_d Pi_ref) over the whole columns, zero velocities, update_state."""
    og = orc.Grid(size, halo=halo, **REST_EXTENT)
    c = orc.Constants()
    om = oc.CompressibleOracleModel(og, constants=c, time_discretization=oc.SplitExplicit(**td), surface_pressure=1e5, standard_pressure=1e5,
                                    reference_potential_temperature=iso_theta(c))
    set_discrete_rest(om)
    return om


def set_discrete_rest(om):
    ref, c = om.ref, om.constants
    om.rho_d[...] = ref.density[:, None, None]
    om.rtheta[...] = (ref.pressure / (c.Rd * np.where(ref.exner_function != 0, ref.exner_function, 1.0)))[:, None, None]
    for f in (om.ru, om.rv, om.rw, om.u, om.v, om.w):
        f[...] = 0.0
    om.update_state(compute_tendencies=True)


def seed_w(om, amplitude=0.01, wavelength=2e3):
    """set!(model; w = 0.01 sin(2 pi z / 2 km)); update_state! (test/balance_adiabatically.jl:115-116)."""
    om.set(w=lambda x, y, z: amplitude * np.sin(2 * np.pi * z / wavelength) + 0 * x + 0 * y)
    om.update_state(compute_tendencies=True)


def anelastic_rest_oracle(orc, size=(8, 8, 16), halo=(3, 3, 3)):
    """The anelastic rest state of test/balance_adiabatically.jl:128-145: theta = theta_r = 300 K, p0 = 1e5, zero velocities."""
    og = orc.Grid(size, x=(0.0, 1e4), y=(0.0, 1e4), z=(0.0, 4e3), halo=halo)
    om = orc.OracleModel(og, surface_pressure=1e5, potential_temperature=300.0)
    om.set(theta=300.0)
    return om


def max_abs(a):
    return float(np.max(np.abs(a)))
