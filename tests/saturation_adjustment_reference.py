"""Typed restatement of the per-cell thermodynamic inversions and the parcel sweeps that drive them.  TEST INFRASTRUCTURE ONLY.

What is restated (every constant and every intermediate in ONE numpy scalar type: float32, float64 or longdouble):
  pressure form   adjust_thermodynamic_state(::LiquidIcePotentialTemperatureState, ::SaturationAdjustment), warm phase
                  (src/Microphysics/saturation_adjustment.jl:168-235; oracle/thermo.py: adjust_warm_phase)          device: bz_sa_diagnose
  density form    the same on a LiquidIceDensityState, around the Newton temperature (:236-301; oracle/thermo.py:
                  adjust_warm_phase_density, density_state_temperature)                                             device: bz_ds_adjust
  plain diagnoses vapour-only T = (p_r / p_st)^(R_m / c_pm) theta, Kessler's closed form with a given condensate, and the compressible
                  vapour-only / Kessler Newton inversions                                  device: bz_exner_factor, bz_kessler_T, k_cmp_diagnose
Typed subclasses instantaneous_precipitation_reference.TypedFormulas (its constants and mixture formulas); in float64 pow and exp are
libm's through Python floats, the functions oracle/thermo.py calls, so the float64 restatement returns that module's bits (pinned by
tests/test_saturation_adjustment_reference.py, which inherits the reference's known answers of tests/test_golden_reference.py).

Every adjustment returns (T, q^v, q^l, Trace): the branch taken, the secant iteration count, the |r2| sequence, the half step of the second
guess, and whether an intermediate was non-finite.  force_branch = "clear" | "cloudy" evaluates that branch whatever the threshold test says.

The module also owns the sweeps (deterministic, seeded; every parcel carries the name of its population):
  bulk                density form: theta in U[250, 330] K, rho in U[0.2, 1.3], q^t log-uniform in [1e-5, 0.04], one parcel in ten in [-1e-5, 0)
                      pressure form: (level k, T-target in U[220, 310], s log-uniform in [0.05, 4]): theta = T-target / Pi_d,k and
                      q^t = min(s q*(T-target, p_r[k]), 0.04)
  negative_or_zero_q  q^t in {0, -1e-12, -1e-6, -1e-5}
  marginal            q^t = q* (1 + delta), delta in DELTAS; q* is the float64 restatement's own threshold of the parcel, the fixed point of
                      q^t = q^s(T1(q^t)) (60 iterations).  delta in {0, +-2^-52} is the population marginal_edge
  guess_switch        q^t chosen (bisection) so that dT / 2 of the second guess is one of GUESS_HALF_STEPS, around the floor 0.01
  theta_zero          cells with rho theta = 0
  exp_small           (anelastic, microphysics = nothing) q in {0.1, 0.2, 0.4, 0.8} on the top level of a 24 km column, where the argument
                      (q kap_num / (c_pm c_pd)) ln(p_r / p_st) of bz_exp_small needs 0, 1 and 2 halvings in neighbouring lanes
The tested domain is q^t <= 0.04 and p_r >= 20 kPa (the 11 km column): beyond it the reference's own secant leaves the domain of its
saturation pressure (NaN), where the device's fmax (drops a NaN) and the reference's max (keeps it) are not expected to agree.

A seeded permutation places the parcels on the grid; placement 1 shuffles placement 0 inside every level (the pressure-form parcels are
realised on their level).  A case holds the prognostic arrays a device model is given; the restatement starts from those arrays and repeats
the kernels' first lines (theta = rho theta / rho_d, rho = rho_d + rho q, q = rho q / rho; anelastic: divisions by rho_r[k])."""
import functools
import math

import numpy as np

import instantaneous_precipitation_reference as ipr
from oracle import thermo

CLEAR, CLOUDY, THETA_ZERO = 0, 1, 2
DELTAS = (0.0, 2.0 ** -52, -2.0 ** -52, 1e-12, -1e-12, 1e-9, 1e-6, 1e-3)
EDGE_DELTAS = DELTAS[:3]
GUESS_HALF_STEPS = (0.005, 0.01 * (1 - 1e-9), 0.01 * (1 + 1e-9), 0.02)
NEGATIVE_Q = (0.0, -1e-12, -1e-6, -1e-5)
EXP_SMALL_Q = (0.1, 0.2, 0.4, 0.8)
DEFAULT_SOLVER = (1e-4, 20)
SOLVERS = (DEFAULT_SOLVER, (1e-4, 0), (1e-4, 2), (0.0, 50))
NEWTON = (1e-4, 8)
LOOSE_NEWTONS = ((1e-4, 0), (1e-4, 1), (1.0, 8))      # temperature solvers that stop on maxiter = 0 (T is the first guess), on maxiter = 1 and on
                                     # abstol = 1 K, long before convergence: a Newton loop that ignores either bound gives another answer
                                     # (under the default one the last step is below 1e-13 of T)
KNIFE_EDGE = 1e-9                    # K: |r2| this close to a non-zero abstol may stop one iteration apart in two arithmetics
PST = 1e5
Q_CAP = 0.04
COMPRESSIBLE_GRIDS = ((66, 6, 4), (130, 9, 6))
ANELASTIC_GRIDS = ((66, 8, 12), (130, 9, 6))
COLUMN, TALL_COLUMN = 11e3, 24e3     # p_r >= 20 kPa on the first; the top level of the second is below 2 kPa (exp_small)
SURFACE_PRESSURE, THETA_0 = 101325.0, 300.0
POPULATIONS = ("bulk", "negative_or_zero_q", "marginal", "marginal_edge", "guess_switch", "theta_zero", "exp_small")


class Trace:
    __slots__ = ("branch", "iterations", "residuals", "half_step", "nonfinite")

    def __init__(self):
        self.branch, self.iterations, self.residuals, self.half_step, self.nonfinite = CLEAR, 0, [], None, False

    def knife_edge(self, abstol):
        return abstol > 0 and any(abs(r - abstol) <= KNIFE_EDGE for r in self.residuals)


class Typed(ipr.TypedFormulas):
    """TypedFormulas with the pressure form, the plain diagnoses and a trace.  pw / ex: in float64 libm through Python floats."""

    def __init__(self, dtype, c=None):
        super().__init__(dtype, c)
        self.eps = self.Rd / self.Rv
        self.kap_num = self.Rv * self.cpd - self.Rd * self.cpv
        self._f64 = dtype is np.float64

    def pw(self, a, b):
        if not self._f64:
            return a ** b
        try:
            r = float(a) ** float(b)
        except (OverflowError, ZeroDivisionError):
            return np.float64(np.inf)
        return np.float64(r) if isinstance(r, float) else np.float64(np.nan)

    def ex(self, x):
        if not self._f64:
            return np.exp(x)
        try:
            return np.float64(math.exp(x))
        except OverflowError:
            return np.float64(np.inf)

    # ---- shared pieces ------------------------------------------------------------------------------------------------------------------
    def psat(self, T):
        t = self.dtype
        return self.ptr * self.pw(T / self.Ttr, self.dc / self.Rv) * self.ex((t(1) / self.Ttr - t(1) / T) * self.L0 / self.Rv)

    def _secant(self, residual, x1, x2, abstol, maxiter, tr):
        t = self.dtype
        r1, r2, it = residual(x1), residual(x2), 0
        tr.residuals.append(abs(r2))
        while abs(r2) > abstol and it < maxiter:
            denom = r2 - r1
            s = (x2 - x1) / denom if denom != 0 else t(np.inf)
            valid = bool(np.isfinite(s))
            s = s if valid else t(0)
            x1, r1 = x2, r2
            x2 = x2 - r2 * s
            r2 = residual(x2) if valid else t(0)
            it += 1
            tr.residuals.append(abs(r2))
            tr.nonfinite |= not (np.isfinite(x2) and np.isfinite(r2))
        tr.iterations = it
        return x2

    def _second_guess(self, T1, qv1, ql1, tr):
        t = self.dtype
        dT = (self.Ll * ql1) / self._mix(qv1, ql1)[1]
        tr.half_step = dT / t(2)
        return T1 + max(t(0.01), dT / t(2))

    # ---- pressure form (anelastic) ------------------------------------------------------------------------------------------------------
    def T_pressure(self, theta, qv, ql, pr, pst):
        """T of a LiquidIcePotentialTemperatureState: Pi(q) theta + L q^l / c_pm (dynamic_states.jl:46-58); with q^l = 0 the vapour-only
        diagnosis, with a given condensate Kessler's closed form"""
        Rm, cpm = self._mix(qv, ql)
        return self.pw(pr / pst, Rm / cpm) * theta + (self.Ll * ql) / cpm

    def _adjust_p(self, T, qt, pr):
        t = self.dtype
        ps = self.psat(T)
        qs = self.eps * (t(1) - qt) * ps / (pr - ps)
        ql = max(t(0), qt - qs)
        return qt - ql, ql

    def threshold_pressure(self, T1, qt, pr):
        rho1 = pr / (self._mix(qt, self.dtype(0))[0] * T1)
        return self.psat(T1) / (rho1 * self.Rv * T1)

    def adjust_pressure(self, theta, qt, pr, pst, abstol, maxiter, force_branch=None):
        t, tr = self.dtype, Trace()
        if theta == 0:
            tr.branch = THETA_ZERO
            return t(0), qt, t(0), tr
        T1 = self.T_pressure(theta, qt, t(0), pr, pst)
        clear = bool(qt <= self.threshold_pressure(T1, qt, pr)) if force_branch is None else force_branch == "clear"
        tr.nonfinite |= not np.isfinite(T1)
        if clear:
            return T1, qt, t(0), tr
        tr.branch = CLOUDY
        T2 = self._second_guess(T1, *self._adjust_p(T1, qt, pr), tr)
        Ts = self._secant(lambda T: T - self.T_pressure(theta, *self._adjust_p(T, qt, pr), pr, pst), T1, T2, abstol, maxiter, tr)
        qv, ql = self._adjust_p(Ts, qt, pr)
        T = self.T_pressure(theta, qv, ql, pr, pst)
        tr.nonfinite |= not (np.isfinite(T) and np.isfinite(ql))
        return T, qv, ql, tr

    def exp_small_argument(self, q, pr, pst):
        """the argument bz_exner_factor hands to bz_exp_small"""
        cpm = self._mix(q, self.dtype(0))[1]
        return ((q * self.kap_num) / (cpm * self.cpd)) * np.log(pr / pst)

    # ---- density form (compressible) ----------------------------------------------------------------------------------------------------
    def temperature(self, theta, qv, ql, rho, pst, abstol, maxiter):
        """temperature(::LiquidIceDensityState): Newton on T = (rho R_m T / p_st)^kappa theta + L; q^l = 0: the vapour-only inversion"""
        t = self.dtype
        Rm, cpm = self._mix(qv, ql)
        kap, gam = Rm / cpm, cpm / (cpm - Rm)
        L = (self.Ll * ql) / cpm
        T = self.pw(theta, gam) * self.pw(rho * Rm / pst, gam - t(1)) + L
        dT, it = T, 0
        while abs(dT) > abstol and it < maxiter:
            Phi = self.pw(rho * Rm * T / pst, kap) * theta
            dT = -(T - Phi - L) / (t(1) - kap * Phi / T)
            T = T + dT
            it += 1
        return T

    def residual(self, T, theta0, rho, qt, pst):
        t = self.dtype
        qs = self.psat(T) / (rho * self.Rv * T)
        ql = max(t(0), qt - qs)
        qv = qt - ql
        Rm, cpm = self._mix(qv, ql)
        L = (self.Ll * ql) / cpm
        p = rho * Rm * T
        return (T - L) * self.pw(pst / p, Rm / cpm) - theta0, qv, ql

    def adjust_density(self, theta, qt, rho, pst, abstol, maxiter, newton_abstol, newton_maxiter, force_branch=None):
        t, tr = self.dtype, Trace()
        if theta == 0:
            tr.branch = THETA_ZERO
            return t(0), qt, t(0), tr
        T1 = self.temperature(theta, qt, t(0), rho, pst, newton_abstol, newton_maxiter)
        clear = bool(qt <= self.psat(T1) / (rho * self.Rv * T1)) if force_branch is None else force_branch == "clear"
        tr.nonfinite |= not np.isfinite(T1)
        if clear:
            return T1, qt, t(0), tr
        tr.branch = CLOUDY
        _, qv1, ql1 = self.residual(T1, theta, rho, qt, pst)
        T2 = self._second_guess(T1, qv1, ql1, tr)
        Ts = self._secant(lambda T: self.residual(T, theta, rho, qt, pst)[0], T1, T2, abstol, maxiter, tr)
        _, qv, ql = self.residual(Ts, theta, rho, qt, pst)
        T = self.temperature(theta, qv, ql, rho, pst, newton_abstol, newton_maxiter)
        tr.nonfinite |= not (np.isfinite(T) and np.isfinite(ql))
        return T, qv, ql, tr

    def adjust(self, theta, qt, rho, pst, abstol, maxiter, newton_abstol, newton_maxiter):
        return self.adjust_density(theta, qt, rho, pst, abstol, maxiter, newton_abstol, newton_maxiter)[:3]


@functools.lru_cache(maxsize=None)
def typed(dtype):
    return Typed(dtype)


# ---- reference columns of the anelastic model (reference_states.jl:84-123: dry adiabatic, hydrostatic) ------------------------------------
def reference_column(Nz, Lz, p0=SURFACE_PRESSURE, theta0=THETA_0, pst=PST):
    """(p_r, rho_r) at the centres of Nz uniform levels under Lz; the host model evaluates the same expressions"""
    c = thermo.ThermoConstants()
    z = (np.arange(Nz) + 0.5) * (Lz / Nz)
    T0 = theta0 * (p0 / pst) ** (c.Rd / c.cpd)
    p = p0 * (1 - c.g * z / (c.cpd * T0)) ** (c.cpd / c.Rd)
    rho0 = p0 / (c.Rd * ((p0 / pst) ** (c.Rd / c.cpd) * theta0))
    return p, rho0 * (p / p0) ** (1 - c.Rd / c.cpd)


# ---- the sweeps ---------------------------------------------------------------------------------------------------------------------------
def _population_sizes(n):
    m = max(8, n // 130)             # parcels per value of a special population
    special = m * (len(NEGATIVE_Q) + len(DELTAS) + len(GUESS_HALF_STEPS)) + 4
    return m, n - special


def _tags(n, bulk_only=False):
    """population and sub-value (delta, half step, q) of each of n parcels, specials first"""
    if bulk_only:
        return np.array(["bulk"] * n), np.zeros(n)
    m, bulk = _population_sizes(n)
    tag, sub = [], []
    for q in NEGATIVE_Q:
        tag += ["negative_or_zero_q"] * m
        sub += [q] * m
    for d in DELTAS:
        tag += ["marginal_edge" if d in EDGE_DELTAS else "marginal"] * m
        sub += [d] * m
    for h in GUESS_HALF_STEPS:
        tag += ["guess_switch"] * m
        sub += [h] * m
    tag += ["theta_zero"] * 4 + ["bulk"] * bulk
    sub += [0.0] * (4 + bulk)
    return np.array(tag), np.array(sub)


def _bisect(f, lo, hi):
    """root of the increasing f between lo and hi, to the last bit"""
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if mid == lo or mid == hi:
            break
        lo, hi = (mid, hi) if f(mid) < 0 else (lo, mid)
    return hi


def _density_threshold(F, theta, rho):
    q = np.float64(0.01)
    for _ in range(60):
        T1 = F.temperature(theta, q, np.float64(0), rho, np.float64(PST), *_newton(np.float64))
        q = F.psat(T1) / (rho * F.Rv * T1)
    return q


def _pressure_threshold(F, theta, pr):
    q = np.float64(0.005)
    for _ in range(60):
        q = F.threshold_pressure(F.T_pressure(theta, q, np.float64(0), pr, np.float64(PST)), q, pr)
    return q


def _newton(t):
    return t(NEWTON[0]), NEWTON[1]


@functools.lru_cache(maxsize=None)
def density_parcels(n, seed=80, bulk_only=False):
    """(theta, rho, q^t, tag, sub) of n parcels of the density form"""
    F, f = typed(np.float64), np.float64
    rng = np.random.default_rng(seed)
    tag, sub = _tags(n, bulk_only)
    theta, rho = rng.uniform(250.0, 330.0, n), rng.uniform(0.2, 1.3, n)
    qt = 10.0 ** rng.uniform(np.log10(1e-5), np.log10(Q_CAP), n)
    negative = rng.random(n) < 0.1
    qt[negative] = -rng.uniform(0.0, 1e-5, n)[negative]
    with np.errstate(all="ignore"):
        for i in range(n):
            if tag[i] == "negative_or_zero_q":
                qt[i] = sub[i]
            elif tag[i] in ("marginal", "marginal_edge", "guess_switch"):
                while True:          # a parcel whose threshold lies inside the tested domain
                    qstar = _density_threshold(F, f(theta[i]), f(rho[i]))
                    if 1e-5 <= qstar <= 0.03:
                        break
                    theta[i], rho[i] = rng.uniform(250.0, 330.0), rng.uniform(0.2, 1.3)
                if tag[i] == "guess_switch":
                    def miss(q, i=i):
                        tr = F.adjust_density(f(theta[i]), f(q), f(rho[i]), f(PST), f(1e-4), 0, *_newton(f), force_branch="cloudy")[3]
                        return float(tr.half_step) - sub[i]
                    qt[i] = _bisect(miss, float(qstar), float(qstar) + 2e-3)
                else:
                    qt[i] = float(qstar) * (1.0 + sub[i])
    return theta, rho, qt, tag, sub


@functools.lru_cache(maxsize=None)
def pressure_parcels(n, seed=81, bulk_only=False):
    """(T-target, s, tag, sub) of n parcels of the pressure form; theta and q^t follow on the level the placement gives"""
    rng = np.random.default_rng(seed)
    tag, sub = _tags(n, bulk_only)
    return rng.uniform(220.0, 310.0, n), 10.0 ** rng.uniform(np.log10(0.05), np.log10(4.0), n), tag, sub


@functools.lru_cache(maxsize=None)
def placement(shape, which=0, seed=82):
    """(Nz, Ny, Nx) array: the parcel of each cell.  which = 1: placement 0 shuffled inside every level"""
    Nx, Ny, Nz = shape
    rng = np.random.default_rng(seed)
    P = rng.permutation(Nx * Ny * Nz).reshape(Nz, Ny, Nx)
    if which:
        rng = np.random.default_rng(seed + which)
        P = np.stack([lev.ravel()[rng.permutation(Ny * Nx)].reshape(Ny, Nx) for lev in P])
    return P


@functools.lru_cache(maxsize=None)
def _level_of_parcel(shape):
    P = placement(shape, 0)
    k = np.empty(P.size, int)
    for lev in range(P.shape[0]):
        k[P[lev].ravel()] = lev
    return k


class Case(dict):
    """prognostic arrays shaped (Nz, Ny, Nx), `tag`, `sub`, and for the anelastic model p_r, rho_r"""
    __getattr__ = dict.__getitem__


@functools.lru_cache(maxsize=None)
def compressible_case(shape, which=0, bulk_only=False):
    """rho_d, rho theta, rho q^t (and planted Kessler condensate densities rho q^cl, rho q^r, read only by the Kessler model).
    bulk_only: the state a whole step starts from"""
    n = shape[0] * shape[1] * shape[2]
    theta, rho, qt, tag, sub = density_parcels(n, bulk_only=bulk_only)
    rng = np.random.default_rng(83)
    rq = rho * qt
    rho_d = rho - rq
    rtheta = np.where(tag == "theta_zero", 0.0, rho_d * theta)
    cloud = rng.random(n) < 0.5
    rqcl, rqr = np.where(cloud, rho * rng.uniform(0, 2e-3, n), 0.0), np.where(cloud, rho * rng.uniform(0, 1e-3, n), 0.0)
    P = placement(shape, which)
    return Case(rho_d=rho_d[P], rtheta=rtheta[P], rq=rq[P], rqcl=rqcl[P], rqr=rqr[P], tag=tag[P], sub=sub[P], parcel=P)


@functools.lru_cache(maxsize=None)
def anelastic_case(shape, Lz=COLUMN, which=0, exp_small=False, bulk_only=False):
    """rho theta, rho q on the model's own rho_r; planted Kessler condensate (the diagnostic fractions q^cl, q^r the diagnosis reads, and the
    densities it refreshes them from).  exp_small = True (microphysics = nothing): EXP_SMALL_Q scattered over the top level.
    bulk_only: the state a whole step starts from"""
    F, f = typed(np.float64), np.float64
    Nx, Ny, Nz = shape
    n = Nx * Ny * Nz
    p_r, rho_r = reference_column(Nz, Lz)
    Tt, s, tag, sub = pressure_parcels(n, bulk_only=bulk_only)
    tag, sub = tag.copy(), sub.copy()
    k = _level_of_parcel(shape)
    kd = thermo.ThermoConstants()
    theta, qt = np.empty(n), np.empty(n)
    pst = f(PST)
    with np.errstate(all="ignore"):
        for i in range(n):
            pr, T = f(p_r[k[i]]), Tt[i]
            pi_d = (p_r[k[i]] / PST) ** (kd.Rd / kd.cpd)
            if tag[i] in ("marginal", "marginal_edge", "guess_switch"):
                while True:          # lower the target until the parcel's threshold lies inside the tested domain
                    th = f((rho_r[k[i]] * (T / pi_d)) / rho_r[k[i]])
                    qstar = _pressure_threshold(F, th, pr)
                    if np.isfinite(qstar) and 1e-6 <= qstar <= 0.03:
                        break
                    T -= 10.0
                theta[i] = T / pi_d
                if tag[i] == "guess_switch":
                    def miss(q, th=th, pr=pr):
                        return float(F.adjust_pressure(th, f(q), pr, pst, f(1e-4), 0, force_branch="cloudy")[3].half_step) - sub[i]
                    qt[i] = _bisect(miss, float(qstar), float(qstar) + 2e-3)
                else:
                    qt[i] = float(qstar) * (1.0 + sub[i])
                continue
            theta[i] = T / pi_d
            if tag[i] == "negative_or_zero_q":
                qt[i] = sub[i]
            else:
                qstar = F.threshold_pressure(f(T), f(0), pr)      # of dry air at the target temperature
                qt[i] = min(s[i] * float(qstar), Q_CAP) if qstar > 0 else Q_CAP
    theta[tag == "theta_zero"] = 0.0
    rng = np.random.default_rng(84)
    if exp_small:
        top = np.flatnonzero((k == Nz - 1) & (tag == "bulk"))
        m = 3                        # few: most wavefronts of the level hold none, so a lane's neighbours differ between the placements
        chosen = rng.choice(top, 4 * m, replace=False)
        for j, q in enumerate(EXP_SMALL_Q):
            qt[chosen[j * m:(j + 1) * m]] = q
            tag[chosen[j * m:(j + 1) * m]] = "exp_small"
            sub[chosen[j * m:(j + 1) * m]] = q
    cloud = rng.random(n) < 0.5
    qcl, qr = np.where(cloud, rng.uniform(0, 2e-3, n), 0.0), np.where(cloud, rng.uniform(0, 1e-3, n), 0.0)
    qcl2, qr2 = np.where(cloud, rng.uniform(0, 2e-3, n), 0.0), np.where(cloud, rng.uniform(0, 1e-3, n), 0.0)
    P = placement(shape, which)
    col = rho_r[:, None, None]
    return Case(rtheta=col * theta[P], rq=col * qt[P], qcl=qcl[P], qr=qr[P], rqcl=col * qcl2[P], rqr=col * qr2[P], tag=tag[P], sub=sub[P],
                parcel=P, p_r=p_r, rho_r=rho_r)


# ---- the restatement over a case ----------------------------------------------------------------------------------------------------------
class Result(dict):
    __getattr__ = dict.__getitem__


def _empty(shape, dtype, names):
    out = Result({n: np.zeros(shape, dtype) for n in names})
    out.update(branch=np.zeros(shape, int), iterations=np.zeros(shape, int), knife=np.zeros(shape, bool), nonfinite=np.zeros(shape, bool),
               half_step=np.full(shape, np.nan))
    return out


def _record(out, idx, tr, abstol):
    out.branch[idx], out.iterations[idx], out.nonfinite[idx] = tr.branch, tr.iterations, tr.nonfinite
    out.knife[idx] = tr.knife_edge(abstol)
    if tr.half_step is not None:
        out.half_step[idx] = float(tr.half_step)


def diagnose_compressible(arrays, mp, dtype=np.float64, solver=DEFAULT_SOLVER, newton=NEWTON, force_branch=None, pst=PST):
    """k_cmp_diagnose<MP> cell by cell from rho_d, rho theta, rho q (MP = 2: and rho q^cl, rho q^r) -> theta, q, rho, T, p, q^v, q^l (+ trace).
    MP = 0: vapour only; 1: SaturationAdjustment; 2: Kessler (q^v = q, q^l = q^cl + q^r)"""
    F, t = typed(dtype), dtype
    shape = arrays["rho_d"].shape
    out = _empty(shape, dtype, ("theta", "q", "rho", "T", "p", "qv", "ql", "qcl", "qr"))
    pst, abstol, nab = t(pst), t(solver[0]), t(newton[0])
    with np.errstate(all="ignore"):
        for idx in np.ndindex(shape):
            rd, rth, rq = t(arrays["rho_d"][idx]), t(arrays["rtheta"][idx]), t(arrays["rq"][idx])
            ql = t(0)
            if mp == 2:
                rqcl, rqr = t(arrays["rqcl"][idx]), t(arrays["rqr"][idx])
                r = rd + (rq + (rqcl + (rqr + t(0))))
            else:
                r = rd + (rq + t(0))
            th, q = rth / rd, rq / r
            qv = q
            if mp == 2:
                out.qcl[idx], out.qr[idx] = rqcl / r, rqr / r
                ql = out.qcl[idx] + out.qr[idx]
            if mp == 1:
                T, qv, ql, tr = F.adjust_density(th, q, r, pst, abstol, solver[1], nab, newton[1], force_branch)
                _record(out, idx, tr, float(solver[0]))
            else:
                T = F.temperature(th, qv, ql, r, pst, nab, newton[1])
                out.nonfinite[idx] = not np.isfinite(T)
            Rm = F._mix(qv, ql)[0]
            out.theta[idx], out.q[idx], out.rho[idx], out.T[idx], out.p[idx], out.qv[idx], out.ql[idx] = th, q, r, T, r * Rm * T, qv, ql
    return out


def diagnose_anelastic(arrays, mp, p_r, rho_r, dtype=np.float64, solver=DEFAULT_SOLVER, force_branch=None, pst=PST):
    """k_thermo cell by cell from rho theta, rho q (MP = 2: and the diagnostic q^cl, q^r of before the launch) -> theta, q, T, q^v, q^l.
    MP = 0: T = Pi(q) theta; 1: SaturationAdjustment; 2: Kessler's closed form with the lagged condensate"""
    F, t = typed(dtype), dtype
    shape = arrays["rtheta"].shape
    out = _empty(shape, dtype, ("theta", "q", "T", "qv", "ql", "halvings"))
    pst, abstol = t(pst), t(solver[0])
    with np.errstate(all="ignore"):
        for idx in np.ndindex(shape):
            rho, pr = t(rho_r[idx[0]]), t(p_r[idx[0]])
            th, q = t(arrays["rtheta"][idx]) / rho, t(arrays["rq"][idx]) / rho
            qv, ql = q, t(0)
            if mp == 1:
                T, qv, ql, tr = F.adjust_pressure(th, q, pr, pst, abstol, solver[1], force_branch)
                _record(out, idx, tr, float(solver[0]))
            else:
                if mp == 2:
                    ql = t(arrays["qcl"][idx]) + t(arrays["qr"][idx])
                T = F.T_pressure(th, q, ql, pr, pst)
                out.nonfinite[idx] = not np.isfinite(T)
                a, s = abs(float(F.exp_small_argument(q, pr, pst))), 0
                while a > 0.0625 and s < 64:
                    a, s = a * 0.5, s + 1
                out.halvings[idx] = s
            out.theta[idx], out.q[idx], out.T[idx], out.qv[idx], out.ql[idx] = th, q, T, qv, ql
    return out


@functools.lru_cache(maxsize=None)
def restated(form, shape, mp, dtype, solver=DEFAULT_SOLVER, force_branch=None, which=0, Lz=COLUMN, exp_small=False, newton=NEWTON):
    """the restatement of a case of this module, cached: form "density" (compressible_case) or "pressure" (anelastic_case)"""
    if form == "density":
        return diagnose_compressible(compressible_case(shape, which), mp, dtype, solver, newton, force_branch)
    case = anelastic_case(shape, Lz, which, exp_small)
    return diagnose_anelastic(case, mp, case.p_r, case.rho_r, dtype, solver, force_branch)


# ---- distances and the judging rules --------------------------------------------------------------------------------------------------------
def distances(a, b):
    """per cell: |dT| / |T| (0 where both are 0), |dq^v|, |dq^l| in float64 (longdouble differences are formed in longdouble first)"""
    wide = np.longdouble
    Ta, Tb = a["T"].astype(wide), b["T"].astype(wide)
    with np.errstate(all="ignore"):
        dT = np.where(Tb == 0, np.abs(Ta - Tb), np.abs(Ta - Tb) / np.abs(Tb))
    return dict(T=dT.astype(np.float64), qv=np.abs(a["qv"].astype(wide) - b["qv"].astype(wide)).astype(np.float64),
                ql=np.abs(a["ql"].astype(wide) - b["ql"].astype(wide)).astype(np.float64))


def by_population(tag, values, mask=None):
    """max of `values` over the cells of each population present"""
    out = {}
    for name in POPULATIONS:
        sel = (tag == name) if mask is None else (tag == name) & mask
        if sel.any():
            out[name] = float(np.max(values[sel]))
    return out


@functools.lru_cache(maxsize=None)
def d80(form, shape, mp, solver=DEFAULT_SOLVER, Lz=COLUMN, exp_small=False, newton=NEWTON):
    """the restatement's own rounding sensitivity: float64 against longdouble, per population {name: (dT rel, dq^v, dq^l)}; knife-edge
    parcels and (marginal_edge) parcels on different branches are left out, as the judging leaves them out"""
    a = restated(form, shape, mp, np.float64, solver, Lz=Lz, exp_small=exp_small, newton=newton)
    b = restated(form, shape, mp, np.longdouble, solver, Lz=Lz, exp_small=exp_small, newton=newton)
    tag = (compressible_case(shape) if form == "density" else anelastic_case(shape, Lz, 0, exp_small)).tag
    d = distances(a, b)
    keep = ~a.knife & (a.branch == b.branch)
    per = {n: by_population(tag, d[n], keep) for n in ("T", "qv", "ql")}
    return {name: tuple(per[n].get(name, 0.0) for n in ("T", "qv", "ql")) for name in POPULATIONS if (tag == name).any()}


EPS = float(np.finfo(np.float64).eps)
T_FLOOR, Q_FLOOR, MARGIN = 1e-13, 1e-15, 16.0


def bounds64(tag, table):
    """per cell (T relative, q^v absolute, q^l absolute): max(floor, 16 d80 of the cell's population)"""
    bT, bv, bl = np.full(tag.shape, T_FLOOR), np.full(tag.shape, Q_FLOOR), np.full(tag.shape, Q_FLOOR)
    for name, (dT, dv, dl) in table.items():
        sel = tag == name
        bT[sel], bv[sel], bl[sel] = max(T_FLOOR, MARGIN * dT), max(Q_FLOOR, MARGIN * dv), max(Q_FLOOR, MARGIN * dl)
    return bT, bv, bl


def judge64(dev, want, tag, table, clear=None, cloudy=None, adjusted=True):
    """The Float64 rules.  dev / want: T, q^v, q^l (+ q, branch, knife of `want`); clear / cloudy: the forced-branch restatements, needed where
    marginal_edge parcels exist; adjusted = False: a plain diagnosis (no branches, q^v and q^l are inputs).  -> (failures {rule: cell count}, report {population: largest device distance (T, q^v, q^l)}, skipped)"""
    bT, bv, bl = bounds64(tag, table)

    def within(ref):
        d = distances(dev, ref)
        return (d["T"] <= bT) & (d["qv"] <= bv) & (d["ql"] <= bl), d

    ok, d = within(want)
    zero = want["branch"] == THETA_ZERO
    edge = (tag == "marginal_edge") & ~zero & adjusted
    skipped = want["knife"] & ~edge & ~zero
    fails = {}
    finite = np.isfinite(dev["T"]) & np.isfinite(dev["qv"]) & np.isfinite(dev["ql"])
    if not finite.all():
        fails["non-finite"] = int((~finite).sum())
    ordinary = ~zero & ~edge & ~skipped
    if not ok[ordinary].all():
        fails["ordinary parcels beyond max(floor, 16 d80)"] = int((~ok[ordinary]).sum())
    exact = (want["branch"] == CLEAR) & ordinary & adjusted
    bits = (dev["ql"] == 0) & (dev["qv"] == want["q"])
    if not bits[exact].all():
        fails["clear parcels: q^l an exact zero and q^v the bits of q^t"] = int((~bits[exact]).sum())
    if zero.any():
        z = (dev["T"] == 0) & (dev["qv"] == want["q"]) & (dev["ql"] == 0)
        if not z[zero].all():
            fails["theta = 0 guard"] = int((~z[zero]).sum())
    if edge.any():
        either = within(clear)[0] | within(cloudy)[0]
        if not either[edge].all():
            fails["threshold parcels on neither branch"] = int((~either[edge]).sum())
    report = {name: tuple(by_population(tag, d[n], ordinary).get(name, 0.0) for n in ("T", "qv", "ql")) for name in POPULATIONS
              if ((tag == name) & ordinary).any()}
    return fails, report, int(skipped.sum())


def judge32(dev, want32, want64, tag, qt_max, clear64, cloudy64):
    """The Float32 rule of tests/test_diagnostics.py: the device within 4 d32 of the Float64 restatement of the same (Float32) inputs; floors
    4 ulp of T and 4 x 2^-24 max q^t.  d32, per population, is the distance of the float32 restatement from the Float64 restatement ON THE
    BRANCH THE FLOAT32 ONE TOOK (clear64 / cloudy64: the forced Float64 restatements; the plain one where there are no branches).  Parcels
    the float32 restatement itself puts on the other branch, and the marginal ones, pass on either forced branch.
    -> (failures, {population: largest device distance}, {population: d32})"""
    names = ("T", "qv", "ql")
    cloudy32 = want32["branch"] == CLOUDY
    same = {n: np.where(cloudy32, cloudy64[n], clear64[n]) for n in names}
    d32 = distances(want32, same)
    either = (want32["branch"] != want64["branch"]) | (tag == "marginal") | (tag == "marginal_edge")
    zero = want64["branch"] == THETA_ZERO
    with np.errstate(all="ignore"):
        ulpT = np.spacing(np.abs(want64["T"]).astype(np.float32)).astype(np.float64) / np.abs(want64["T"].astype(np.float64))
    qfloor = 4.0 * 2.0 ** -24 * qt_max
    refs = (want64, clear64, cloudy64)
    dd = [distances(dev, r) for r in refs]
    fails, report, table = {}, {}, {}
    for name in POPULATIONS:
        sel = (tag == name) & ~zero
        if not sel.any():
            continue
        table[name] = tuple(float(d32[n][sel].max()) for n in names)
        bT = np.maximum(4.0 * table[name][0], 4.0 * ulpT)
        bq = [max(4.0 * table[name][j], qfloor) for j in (1, 2)]
        inside = [(d["T"] <= bT) & (d["qv"] <= bq[0]) & (d["ql"] <= bq[1]) for d in dd]
        ok = np.where(either, inside[0] | inside[1] | inside[2], inside[0])
        if not ok[sel].all():
            fails[name] = int((~ok[sel]).sum())
        nearest = {n: np.where(either, np.minimum(np.minimum(dd[0][n], dd[1][n]), dd[2][n]), dd[0][n]) for n in names}
        report[name] = tuple(float(nearest[n][sel].max()) for n in names)
    if zero.any():
        z = (dev["T"] == 0) & (dev["ql"] == 0) & (dev["qv"] == want32["q"])
        if not z[zero].all():
            fails["theta = 0 guard"] = int((~z[zero]).sum())
    return fails, report, table


def wavefront_mixing(result, width=64):
    """every aligned run of `width` cells along x (full runs; a ragged tail shorter than `width` cannot hold the property) -> the smallest
    number of branches and of distinct iteration counts found in a run"""
    Nx = result.branch.shape[-1]
    branches, counts = 9, 99
    for lo in range(0, Nx - width + 1, width):
        b, it = result.branch[..., lo:lo + width], result.iterations[..., lo:lo + width]
        for row_b, row_it in zip(b.reshape(-1, width), it.reshape(-1, width)):
            kinds = set(row_b[row_b != THETA_ZERO])
            branches = min(branches, len(kinds))
            counts = min(counts, len(set(row_it)))           # a clear lane iterates 0 times
    return branches, counts
