"""Float64 numpy restatement of the wind- and stability-dependent bulk surface fluxes on a filtered surface state — a helper of
tests/test_surface_layer*.py and tests/test_example_prescribed_sst.py, not collected as a test.  Written from the equations of
  src/BoundaryConditions/polynomial_bulk_coefficient.jl   neutral_coefficient_10m :526-532, bulk_richardson_number :556-561,
                                                           Ri_B -> zeta :246-275, Psi^D / Psi^T :288-335, correction factors :341-351,
                                                           surface_virtual_potential_temperature :581-589, the coefficient :625-659,
                                                           bulk_coefficient :687-707
  src/BoundaryConditions/BoundaryConditions.jl             wind speeds at the three locations :64-124, near_surface_velocity :134-137
  src/BoundaryConditions/bulk_drag.jl :114-134, bulk_scalar_fluxes.jl :82-99,123-138,206-234
  src/BoundaryConditions/filtered_surface_state.jl         the exponential filter :183-226
  src/BoundaryConditions/update_boundary_conditions.jl     what is filtered (theta; the specific prognostic moisture) :20-47
  src/AtmosphereModels/Diagnostics/potential_temperatures.jl :574-579 (theta_v), saturation_specific_humidity.jl :111-118 (q^v+_t)
of the reference.  Arrays are (Ny, Nx) first-level fields; neighbours wrap periodically and collapse onto the cell in a Flat direction.
Whole steps drive the existing oracle model (oracle/oracle.py:652-668 restated around its own methods) with oracle.forcings._add_bulk_fluxes
patched at test time."""
import numpy as np

DRAG_POLYNOMIAL = (0.142, 0.076, 2.7)
HEAT_POLYNOMIAL = (0.128, 0.068, 2.43)
VAPOR_POLYNOMIAL = (0.120, 0.070, 2.55)


class Constants:
    """ThermodynamicConstants() of the reference (the defaults of oracle/thermo.py: ThermoConstants)."""
    R, Md, Mv = 8.314462618, 0.02897, 0.018015
    cpd, cpv, cl, Ll = 1005.0, 1850.0, 4181.0, 2500800.0
    T_energy, Ttr, ptr = 273.15, 273.16, 611.657
    Rd, Rv = R / Md, R / Mv


class StabilityParameters:
    gamma_d, gamma_t, a, b, c, d = 19.3, 11.6, 1.0, 2.0 / 3.0, 5.0, 0.35


class Mapping:
    stable_unstable_transition, strongly_stable_transition = 0.0, 0.2
    au11, bu11, bu12, au21, au22, bu31, bu32, bu33 = 0.0450, 0.0030, 0.0059, -0.0828, 0.8845, 0.1739, -0.9213, -0.1057
    aw11, aw12, aw21, aw22, bw11, bw12, bw21, bw22 = 0.5738, -0.4399, -4.901, 52.50, -0.0539, 1.540, -0.6690, -3.282
    as11, as21, bs11, bs21, bs22 = 0.7529, 14.94, 0.1569, -0.3091, -1.303


def neutral_coefficient_10m(polynomial, U10, U_min):
    a0, a1, a2 = polynomial
    Us = np.maximum(U10, U_min)
    return (a0 + a1 * Us + a2 / Us) * 1e-3


def bulk_richardson_number(h, thv, thv0, U, U_min, g=9.81):
    Us = np.maximum(U, U_min)
    return (g / ((thv + thv0) / 2)) * h * (thv - thv0) / Us ** 2


def zeta_from_richardson(Ri, alpha, beta, m=Mapping):
    Ri = np.asarray(Ri, dtype=np.float64)
    zu = (m.au11 * alpha) * Ri ** 2 + ((m.bu11 * beta + m.bu12) * alpha ** 2 + (m.au21 * beta + m.au22) * alpha +
                                       (m.bu31 * beta ** 2 + m.bu32 * beta + m.bu33)) * Ri
    zw = ((m.aw11 * beta + m.aw12) * alpha + (m.aw21 * beta + m.aw22)) * Ri ** 2 + \
         ((m.bw11 * beta + m.bw12) * alpha + (m.bw21 * beta + m.bw22)) * Ri
    zs = (m.as11 * alpha + m.as21) * Ri + m.bs11 * alpha + m.bs21 * beta + m.bs22
    return np.where(Ri < m.stable_unstable_transition, zu, np.where(Ri <= m.strongly_stable_transition, zw, zs))


def psi_momentum(zeta, p=StabilityParameters):
    zeta = np.asarray(zeta, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        x = np.sqrt(np.sqrt(np.maximum(1 - p.gamma_d * zeta, 0.0)))
        unstable = 2 * np.log((1 + x) / 2) + np.log((1 + x ** 2) / 2) - 2 * np.arctan(x) + np.pi / 2
        stable = -(p.a * zeta + p.b * (zeta - p.c / p.d) * np.exp(-p.d * zeta) + p.b * p.c / p.d)
    return np.where(zeta < 0, unstable, stable)


def psi_scalar(zeta, p=StabilityParameters):
    zeta = np.asarray(zeta, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        y = np.sqrt(np.maximum(1 - p.gamma_t * zeta, 0.0))
        unstable = 2 * np.log((1 + y) / 2)
        x = np.maximum(1 + 2 * p.a / 3 * zeta, 0.0)
        stable = -(x * np.sqrt(x) + p.b * (zeta - p.c / p.d) * np.exp(-p.d * zeta) + p.b * p.c / p.d - 1)
    return np.where(zeta < 0, unstable, stable)


def stability_correction_factor(alpha, beta, psi_d, psi_t, kind="momentum"):
    d_d = np.maximum(alpha - psi_d, alpha / 10)
    if kind == "momentum":
        return (alpha / d_d) ** 2
    bh = alpha + beta
    d_t = np.maximum(bh - psi_t, bh / 10)
    return (alpha / d_d) * (bh / d_t)


def fitted_stability_function(Ri, alpha, beta, kind="momentum", mapping=Mapping, params=StabilityParameters):
    """sf(Ri_B, alpha, beta[, Val(:scalar)]) (:223-228)"""
    zeta = zeta_from_richardson(Ri, alpha, beta, mapping)
    return stability_correction_factor(alpha, beta, psi_momentum(zeta, params), psi_scalar(zeta, params), kind)


def saturation_vapor_pressure(T, c=Constants):
    dc = c.cpv - c.cl
    L0 = c.Ll - dc * c.T_energy
    return c.ptr * (T / c.Ttr) ** (dc / c.Rv) * np.exp((1 / c.Ttr - 1 / T) * L0 / c.Rv)


def surface_virtual_potential_temperature(T0, p0, c=Constants):
    ps = saturation_vapor_pressure(T0, c)
    e = c.Rd / c.Rv
    qs = e * ps / (p0 + (e - 1) * ps)
    return T0 * (1 + (c.Rv / c.Rd - 1) * qs)


def virtual_potential_temperature(T, qv, ql, p_r, pst, c=Constants):
    return (T / (p_r / pst) ** (c.Rd / c.cpd)) * (1 + (c.Rv / c.Rd - 1) * qv - ql)


class Polynomial:
    """A PolynomialCoefficient attached to one condition: polynomial filled, kind = "momentum" | "scalar"."""

    def __init__(self, polynomial, kind, roughness_length=1.5e-4, minimum_wind_speed=0.1, stability=True, scalar_roughness_length=None,
                 mapping=Mapping, params=StabilityParameters):
        self.polynomial, self.kind, self.ell, self.U_min, self.stability = tuple(polynomial), kind, roughness_length, minimum_wind_speed, stability
        self.ell_h = roughness_length / 7.3 if scalar_roughness_length is None else scalar_roughness_length
        self.mapping, self.params = mapping, params

    def richardson(self, U, T0, h, thv, p0, c=Constants):
        return bulk_richardson_number(h, thv, surface_virtual_potential_temperature(T0, p0, c), U, self.U_min)

    def __call__(self, U, T0, h, thv, p0, c=Constants):
        C10 = neutral_coefficient_10m(self.polynomial, U, self.U_min)
        alpha = np.log(h / self.ell)
        Ch = C10 * (np.log(10 / self.ell) / alpha) ** 2
        if not self.stability:
            return Ch
        beta = np.log(self.ell / self.ell_h)
        return Ch * fitted_stability_function(self.richardson(U, T0, h, thv, p0, c), alpha, beta, self.kind, self.mapping, self.params)


class SurfaceLayer:
    """drag / heat / vapor: None or (coefficient, gustiness, T0) with coefficient a number or a Polynomial and T0 a number or an
    (Ny, Nx) array; filtered: the fluxes read the filtered fields; tau, stages: the filter of whole steps."""

    def __init__(self, p0, pst=1e5, drag=None, heat=None, vapor=None, filtered=False, tau=np.inf, stages=(1, 3)):
        self.p0, self.pst, self.drag_params, self.heat, self.vapor = float(p0), float(pst), drag, heat, vapor
        self.filtered, self.tau, self.stages = filtered, tau, tuple(stages)
        self.fields = None      # filtered {"u", "v", "thv", "theta", "q"}


def _shift(a, di, dj, flat_x, flat_y):
    """a[j + dj, i + di] with periodic wrap; a Flat direction has no neighbours"""
    if di and not flat_x:
        a = np.roll(a, -di, axis=1)
    if dj and not flat_y:
        a = np.roll(a, -dj, axis=0)
    return a


def fluxes(sl, u, v, theta, q, thv, h, flat_x=False, flat_y=False, c=Constants):
    """-> {"Ju", "Jv", "Jtheta", "Jq", "Ri": {...}} from (Ny, Nx) first-level fields: u at x faces, v at y faces, theta / q / theta_v at
    centres (the filtered fields when filtering is on; q is then the filtered specific prognostic moisture, else q^v)."""
    sq = lambda a, di=0, dj=0: _shift(a, di, dj, flat_x, flat_y) ** 2
    U2c = (sq(u) + sq(u, 1, 0)) / 2 + (sq(v) + sq(v, 0, 1)) / 2
    Uc = np.sqrt(U2c)
    out, Ri = {}, {}

    def coefficient(name, C, T0):
        if isinstance(C, Polynomial):
            if C.stability:
                Ri[name] = C.richardson(Uc, T0, h, thv, sl.p0, c) + 0 * Uc
            return C(Uc, T0, h, thv, sl.p0, c)
        return C

    if sl.drag_params is not None:
        C, gust, T0 = sl.drag_params
        rho0 = sl.p0 / (c.Rd * T0)
        CD = coefficient("drag", C, T0)
        v2_fc = ((sq(v, -1, 0) + sq(v, -1, 1)) / 2 + (sq(v) + sq(v, 0, 1)) / 2) / 2
        u2_cf = ((sq(u, 0, -1) + sq(u, 1, -1)) / 2 + (sq(u) + sq(u, 1, 0)) / 2) / 2
        out["Ju"] = -rho0 * CD * np.sqrt(u ** 2 + v2_fc + gust ** 2) * u
        out["Jv"] = -rho0 * CD * np.sqrt(u2_cf + v ** 2 + gust ** 2) * v
    if sl.heat is not None:
        C, gust, T0 = sl.heat
        rho0 = sl.p0 / (c.Rd * T0)
        theta0 = T0 / (sl.p0 / sl.pst) ** (c.Rd / c.cpd)
        out["Jtheta"] = -rho0 * coefficient("heat", C, T0) * np.sqrt(U2c + gust ** 2) * (theta - theta0)
    if sl.vapor is not None:
        C, gust, T0 = sl.vapor
        rho0 = sl.p0 / (c.Rd * T0)
        q0 = saturation_vapor_pressure(T0, c) / (rho0 * c.Rv * T0)
        out["Jq"] = -rho0 * coefficient("vapor", C, T0) * np.sqrt(U2c + gust ** 2) * (q - q0)
    out["Ri"] = Ri
    return out


def filter_update(f_hat, f, eps):
    return (f_hat + eps * f) / (1 + eps)


# ---- the oracle model as the carrier of whole steps ---------------------------------------------------------------------------------
def first_level(om):
    """(Ny, Nx) first-level fields of an OracleModel: u, v, theta, q (specific prognostic moisture), qv, ql, T, theta_v"""
    g = om.grid
    I = lambda f: g.interior(f)[0].copy()
    sa = om.microphysics == "SaturationAdjustment"
    qv, ql = (I(om.qv), I(om.ql)) if sa else (I(om.q), np.zeros((g.Ny, g.Nx)))
    f = dict(u=I(om.u), v=I(om.v), theta=I(om.theta), q=I(om.q), qv=qv, ql=ql, T=I(om.T))
    f["thv"] = virtual_potential_temperature(f["T"], qv, ql, om.ref.pressure[g.Hz], om.ref.pst)
    return f


def _flat(g):
    return (g.Nx == 1 and g.Hx == 0), (g.Ny == 1 and g.Hy == 0)


def add_surface_layer_fluxes(m, sl, dz):
    """what oracle.forcings._add_bulk_fluxes does for the constant set: G[., ., 1] += J / dz_1"""
    g = m.grid
    f = first_level(m)
    if sl.filtered:
        F = sl.fields
        J = fluxes(sl, F["u"], F["v"], F["theta"], F["q"], F["thv"], g.zc[0], *_flat(g))
    else:
        J = fluxes(sl, f["u"], f["v"], f["theta"], f["qv"], f["thv"], g.zc[0], *_flat(g))
    for key, name in (("Ju", "ru"), ("Jv", "rv"), ("Jtheta", "rtheta"), ("Jq", "rq")):
        if key in J:
            g.interior(m.G[name])[0] += J[key] * 1.0 / dz
    return J


class patched_oracle:
    """with patched_oracle(): oracle.forcings._add_bulk_fluxes serves SurfaceLayer objects (and the constant set as before)"""

    def __enter__(self):
        from oracle import forcings
        self.forcings, self.original = forcings, forcings._add_bulk_fluxes
        original = self.original
        forcings._add_bulk_fluxes = lambda m, B, dz: add_surface_layer_fluxes(m, B, dz) if isinstance(B, SurfaceLayer) else original(m, B, dz)
        return self

    def __exit__(self, *exc):
        self.forcings._add_bulk_fluxes = self.original


def initialize_filter(om, sl):
    f = first_level(om)
    sl.fields = {k: f[k].copy() for k in ("u", "v", "thv", "theta", "q")}


def advance_filter(om, sl, eps):
    f = first_level(om)
    for k in sl.fields:
        sl.fields[k] = filter_update(sl.fields[k], f[k], eps)


def time_step(om, sl, dt):
    """OracleModel.time_step (oracle/oracle.py:652-668) with the filter advanced after update_state of the stages sl.stages names;
    call inside `with patched_oracle()`"""
    from oracle.forcings import add_flux_bc_tendencies
    if om.iteration == 0:
        om.update_state(compute_tendencies=True)
    if sl.filtered and sl.fields is None:
        initialize_filter(om, sl)
    for n in om.PROGNOSTIC:
        om.U0[n][...] = getattr(om, n)
    for stage, alpha in enumerate((1.0, 1.0 / 4.0, 2.0 / 3.0), start=1):
        add_flux_bc_tendencies(om)
        om.rk3_substep(dt, alpha)
        om.compute_pressure_correction(alpha * dt)
        om.make_pressure_correction(alpha * dt)
        om.update_state(compute_tendencies=True)
        if sl.filtered and stage in sl.stages:
            advance_filter(om, sl, dt / sl.tau)
    om.clock_time += dt
    om.iteration += 1
