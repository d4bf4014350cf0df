"""Typed restatement of the mixed-phase saturation adjustment, the parcel sweep that drives it and an oracle model that carries it.
TEST INFRASTRUCTURE ONLY.

What is restated (every constant and every intermediate in ONE numpy scalar type: float32, float64 or longdouble, in the manner of
saturation_adjustment_reference.Typed, which this subclasses; in float64 pow and exp are libm's, the functions oracle/thermo.py calls):
  adjust_thermodynamic_state(::LiquidIcePotentialTemperatureState, ::SaturationAdjustment{MixedPhaseEquilibrium})
      src/Microphysics/saturation_adjustment.jl:92-100 (partition), 165-231 (first guess, threshold, second guess, secant)
      src/Thermodynamics/vapor_saturation.jl:146-185 (lambda(T) = (clamp(T, T^h, T^f) - T^h) / (T^f - T^h), taken at the temperature of
          every saturation evaluation), 250-278 (q^v+ = eps (1 - q^t) p^v+ / (p_r - p^v+)), 14-35 with clausius_clapeyron.jl:59-68 (the
          PlanarMixedPhaseSurface: ONE Clausius-Clapeyron expression with dc = lambda dc_l + (1 - lambda) dc_i, L0 likewise; the
          expression of oracle/thermo.py: _surface(('mixed', lambda)), pinned to the reference's doctest value)
      src/Thermodynamics/dynamic_states.jl:29-58 (T = Pi^(R_m / c_pm) theta + (L_l q^l + L_i q^i) / c_pm, c_pm with c_i q^i)
  device: bz_mp_diagnose (csrc/bz_internal.h).
With T^f and T^h below every parcel lambda = 1 everywhere and the float64 restatement returns the bits of oracle.thermo.adjust_warm_phase
(tests/test_mixed_phase_reference.py).

Every adjustment returns (T, q^v, q^l, q^i, Trace) with the Trace of saturation_adjustment_reference.

The sweep (deterministic, seeded; pressure form on the anelastic grids sar.ANELASTIC_GRIDS over the 24 km sar.TALL_COLUMN, whose upper levels are
far colder than T^h).  A parcel is built backwards from a target adjusted state: a final temperature T*, a condensate q^c and the level's
p_r give lambda(T*), q^v = q^v+(T*), q^t = q^v + q^c and theta = (T* - (L_l q^l + L_i q^i) / c_pm) / Pi^(R_m / c_pm), so the adjustment of
(theta, q^t) ends within the solver tolerance of T*.  Populations (a parcel's population is drawn among those its level can host: a level
hosts T* only where q^v+(T*, p_r) <= 0.03):
  clear               q^t = s q^v+(T*), s in U[0.05, 0.95]
  warm_cloudy         T* >= T^f + 5.5 K           (final T >= T^f + 5 K: lambda = 1, q^i an exact zero)
  all_ice             T* <= T^h - 5.5 K           (final T <= T^h - 5 K: lambda = 0, q^l an exact zero)
  mixed_range         T^h + 0.1 <= T* <= T^f - 0.1
  kink_Th, kink_Tf    T* within 0.05 K of the kink, on both sides (the sign alternates with the parcel index)
  marginal_edge       q^t = q* (1 + delta), delta in {0, +-2^-52}; q* the float64 restatement's own threshold (fixed point, 60 iterations)
  negative_or_zero_q  q^t in sar.NEGATIVE_Q
  theta_zero          cells with rho theta = 0
sar.placement places the parcels; placement 1 shuffles placement 0 inside every level, so that a parcel shares its wavefront with other
neighbours, on both branches.  The solvers are sar.SOLVERS.

MixedPhaseOracleModel(OracleModel): the oracle's warm-phase update_state!, followed by the restated mixed diagnosis of T, q^v, q^l, q^i on
the interior (a vectorised float64 transcription of the typed formulas: numpy's pow and exp instead of libm's, pinned to the typed
restatement by tests/test_mixed_phase_reference.py).  `self.ql` holds q^l + q^i: the oracle's moist w tendency (og_w_tendency_moist) reads
the condensate only as that sum (R_m = (1 - (q^v + q^c)) R_d + q^v R_v), which is all the ice loading does to the buoyancy.  The separate
q^l and q^i sit beside it as `self.ql_liquid` and `self.qi`, halos refilled.  The tendencies follow."""
import functools

import numpy as np

import saturation_adjustment_reference as sar
from oracle import thermo
from oracle.oracle import OracleModel

TF, TH = 273.15, 233.15
CLEAR, CLOUDY, THETA_ZERO = sar.CLEAR, sar.CLOUDY, sar.THETA_ZERO
POPULATIONS = ("clear", "warm_cloudy", "all_ice", "mixed_range", "kink_Th", "kink_Tf", "marginal_edge", "negative_or_zero_q", "theta_zero")
EDGE_DELTAS = sar.EDGE_DELTAS
Q_HOST = 0.03                        # a level hosts T* where q^v+(T*, p_r) is at most this
KINK = 0.05                          # K
NAMES = ("T", "qv", "ql", "qi")


class TypedMixed(sar.Typed):
    """sar.Typed with the ice phase and the mixed-phase equilibrium"""

    def __init__(self, dtype, Tf=TF, Th=TH, c=None):
        super().__init__(dtype, c)
        c = c or thermo.ThermoConstants()
        t = dtype
        self.Li, self.ci = t(c.Li), t(c.ci)
        self.dci = t(c.cpv) - t(c.ci)
        self.L0i = self.Li - self.dci * t(c.T_energy)
        self.Tf, self.Th = t(Tf), t(Th)

    def lam(self, T):
        Tc = self.Tf if T > self.Tf else (self.Th if T < self.Th else T)          # clamp(T, T^h, T^f)
        return (Tc - self.Th) / (self.Tf - self.Th)

    def psat_mixed(self, T, lam):
        t = self.dtype
        dc = lam * self.dc + (t(1) - lam) * self.dci
        L0 = lam * self.L0 + (t(1) - lam) * self.L0i
        return self.ptr * self.pw(T / self.Ttr, dc / self.Rv) * self.ex((t(1) / self.Ttr - t(1) / T) * L0 / self.Rv)

    def _mix3(self, qv, ql, qi):
        qd = self.dtype(1) - (qv + ql + qi)
        return qd * self.Rd + qv * self.Rv, qd * self.cpd + qv * self.cpv + ql * self.cl + qi * self.ci

    def T_mixed(self, theta, qv, ql, qi, pr, pst):
        Rm, cpm = self._mix3(qv, ql, qi)
        return self.pw(pr / pst, Rm / cpm) * theta + (self.Ll * ql + self.Li * qi) / cpm

    def saturated_vapor(self, T, qt, pr):
        """adjustment_saturation_specific_humidity over the surface equilibrated at T"""
        ps = self.psat_mixed(T, self.lam(T))
        return self.eps * (self.dtype(1) - qt) * ps / (pr - ps)

    def _adjust_m(self, T, qt, pr):
        t = self.dtype
        lam = self.lam(T)
        qc = max(t(0), qt - self.saturated_vapor(T, qt, pr))
        return qt - qc, lam * qc, (t(1) - lam) * qc

    def threshold_mixed(self, T1, qt, pr):
        rho1 = pr / (self._mix(qt, self.dtype(0))[0] * T1)
        return self.psat_mixed(T1, self.lam(T1)) / (rho1 * self.Rv * T1)

    def adjust_mixed(self, theta, qt, pr, pst, abstol, maxiter, force_branch=None):
        t, tr = self.dtype, sar.Trace()
        if theta == 0:
            tr.branch = THETA_ZERO
            return t(0), qt, t(0), t(0), tr
        T1 = self.T_mixed(theta, qt, t(0), t(0), pr, pst)
        clear = bool(qt <= self.threshold_mixed(T1, qt, pr)) if force_branch is None else force_branch == "clear"
        tr.nonfinite |= not np.isfinite(T1)
        if clear:
            return T1, qt, t(0), t(0), tr
        tr.branch = CLOUDY
        qv1, ql1, qi1 = self._adjust_m(T1, qt, pr)
        dT = (self.Ll * ql1 + self.Li * qi1) / self._mix3(qv1, ql1, qi1)[1]
        tr.half_step = dT / t(2)
        T2 = T1 + max(t(0.01), dT / t(2))
        Ts = self._secant(lambda T: T - self.T_mixed(theta, *self._adjust_m(T, qt, pr), pr, pst), T1, T2, abstol, maxiter, tr)
        qv, ql, qi = self._adjust_m(Ts, qt, pr)
        T = self.T_mixed(theta, qv, ql, qi, pr, pst)
        tr.nonfinite |= not (np.isfinite(T) and np.isfinite(ql) and np.isfinite(qi))
        return T, qv, ql, qi, tr

    def theta_of(self, T, qv, ql, qi, pr, pst):
        """theta^li of a known (T, q): the inverse of T_mixed"""
        Rm, cpm = self._mix3(qv, ql, qi)
        return (T - (self.Ll * ql + self.Li * qi) / cpm) / self.pw(pr / pst, Rm / cpm)

    def known_answer(self, T, qt, pr, pst):
        """(theta, q^v, q^l, q^i) of the state the reference's known-answer tests build at (T, q^t) (test/saturation_adjustment.jl:150-239):
        q^v+ = equilibrium_saturation_specific_humidity(T, p_r, q^t) (vapor_saturation.jl:216-230: the saturated form where q^t reaches
        the unsaturated one), the condensate q^t - q^v+ split by lambda(T), theta^li from (T, q).  Where q^t <= q^v+ the reference's guard
        skips its assertions (300 K / 0.02 at 1013 hPa is such a state); the known answer is then the unsaturated state itself."""
        t = self.dtype
        ps = self.psat_mixed(T, self.lam(T))
        q0 = ps / ((pr / (self._mix(qt, t(0))[0] * T)) * self.Rv * T)
        qs = self.saturated_vapor(T, qt, pr) if qt >= q0 else q0
        qc = max(t(0), qt - qs)
        lam = self.lam(T)
        qv, ql, qi = qt - qc, lam * qc, (t(1) - lam) * qc
        return self.theta_of(T, qv, ql, qi, pr, pst), qv, ql, qi


@functools.lru_cache(maxsize=None)
def typed(dtype, Tf=TF, Th=TH):
    return TypedMixed(dtype, Tf, Th)


# the reference's known answers (test/saturation_adjustment.jl:150-239): (T, q^t) at the lowest level's p_r of ReferenceState(p0 = 101325,
# theta0 = 288); its tolerances (:24-27): SecantSolver(abstol = solver_tol = 1e-6), atol = test_tol = 10 sqrt(solver_tol)
KNOWN = ((300.0, 0.02), (220.0, 0.01), (253.15, 0.015))
KNOWN_IDS = ("warm-300K", "ice-220K", "mixed-253.15K")
KNOWN_P0, KNOWN_THETA0 = 101325.0, 288.0
SOLVER_TOL, TEST_TOL = 1e-6, 10 * 1e-6 ** 0.5


# ---- the sweep --------------------------------------------------------------------------------------------------------------------------------
def _host_limit(F, pr):
    """largest T* (K, at most 310) the level hosts: dry-air q^v+(T*, p_r) over the equilibrated surface <= Q_HOST"""
    f = np.float64

    def over(T):
        ps = F.psat_mixed(f(T), F.lam(f(T)))
        return not (ps < pr and F.eps * ps / (pr - ps) <= Q_HOST)
    if not over(310.0):
        return 310.0
    lo, hi = 150.0, 310.0
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        lo, hi = (lo, mid) if over(mid) else (mid, hi)
    return lo


def _threshold(F, theta, pr):
    q = np.float64(1e-4)
    for _ in range(60):
        q = F.threshold_mixed(F.T_mixed(theta, q, np.float64(0), np.float64(0), pr, np.float64(sar.PST)), q, pr)
    return q


@functools.lru_cache(maxsize=None)
def mixed_case(shape, which=0, seed=91, Tf=TF, Th=TH):
    """rho theta, rho q on the reference column of the device model over sar.TALL_COLUMN, with tag, sub (the delta or q of a special parcel),
    target (T*) and parcel (the placement)"""
    F, f = typed(np.float64, Tf, Th), np.float64
    Nx, Ny, Nz = shape
    n = Nx * Ny * Nz
    p_r, rho_r = sar.reference_column(Nz, sar.TALL_COLUMN)
    level = sar._level_of_parcel(shape)
    rng = np.random.default_rng(seed)
    limit = [_host_limit(F, f(p)) for p in p_r]
    pst = f(sar.PST)
    tag, sub, target = np.empty(n, dtype="U20"), np.zeros(n), np.zeros(n)
    theta, qt = np.empty(n), np.empty(n)
    weights = dict(clear=0.30, warm_cloudy=0.14, all_ice=0.14, mixed_range=0.16, kink_Th=0.07, kink_Tf=0.07, marginal_edge=0.07,
                   negative_or_zero_q=0.05)
    with np.errstate(all="ignore"):
        for i in range(n):
            k = level[i]
            pr, Tmax = f(p_r[k]), limit[k]
            hosts = {"clear": True, "all_ice": True, "marginal_edge": True, "negative_or_zero_q": True, "kink_Th": Tmax >= Th + 1.0,
                     "mixed_range": Tmax >= Th + 1.0, "kink_Tf": Tmax >= Tf + 1.0, "warm_cloudy": Tmax >= Tf + 6.5}
            names = [m for m in weights if hosts[m]]
            w = np.array([weights[m] for m in names])
            name = names[int(rng.choice(len(names), p=w / w.sum()))]
            u, v, pick = rng.random(), rng.random(), int(rng.integers(0, 1 << 30))
            if name == "warm_cloudy":
                T = Tf + 5.5 + u * (Tmax - (Tf + 5.5))
            elif name == "all_ice":
                T = 190.0 + u * (Th - 5.5 - 190.0)
            elif name == "mixed_range":
                hi = min(Tf - 0.1, Tmax)
                T = Th + 0.1 + u * (hi - (Th + 0.1))
            elif name in ("kink_Th", "kink_Tf"):
                T = (Th if name == "kink_Th" else Tf) + (1.0 if i % 2 else -1.0) * (1e-4 + u * (KINK - 2e-4))
                sub[i] = T - (Th if name == "kink_Th" else Tf)
            else:
                T = 195.0 + u * (Tmax - 195.0)
            T, tag[i], target[i] = f(T), name, T
            qs_dry = F.eps * F.psat_mixed(T, F.lam(T)) / (pr - F.psat_mixed(T, F.lam(T)))
            if name in ("clear", "negative_or_zero_q", "marginal_edge"):
                th = F.theta_of(T, f(0), f(0), f(0), pr, pst)          # of dry air at the target temperature
                if name == "clear":
                    q = f((0.05 + 0.9 * v) * float(qs_dry))
                elif name == "negative_or_zero_q":
                    sub[i] = sar.NEGATIVE_Q[pick % len(sar.NEGATIVE_Q)]
                    q = f(sub[i])
                else:
                    sub[i] = EDGE_DELTAS[pick % len(EDGE_DELTAS)]
                    q = f(float(_threshold(F, th, pr)) * (1.0 + sub[i]))
            else:
                lam = F.lam(T)
                qc = f(min(10.0 ** (-6.0 + v * (np.log10(5e-3) + 6.0)), sar.Q_CAP - float(qs_dry)))
                qv = F.eps * (f(1) - qc) * (qs_dry / F.eps) / (f(1) + qs_dry)      # q^v = eps (1 - q^c - q^v) r, r = p^v+ / (p_r - p^v+)
                q = qv + qc
                th = F.theta_of(T, qv, lam * qc, (f(1) - lam) * qc, pr, pst)
            theta[i], qt[i] = th, q
    zero = rng.choice(n, 4, replace=False)
    tag[zero], theta[zero] = "theta_zero", 0.0
    P = sar.placement(shape, which)
    col = rho_r[:, None, None]
    return sar.Case(rtheta=col * theta[P], rq=col * qt[P], tag=tag[P], sub=sub[P], target=target[P], parcel=P, p_r=p_r, rho_r=rho_r)


# ---- the restatement over a case ------------------------------------------------------------------------------------------------------------
def diagnose_mixed(arrays, p_r, rho_r, dtype=np.float64, solver=sar.DEFAULT_SOLVER, force_branch=None, pst=sar.PST, Tf=TF, Th=TH):
    """k_thermo<true> cell by cell from rho theta, rho q -> theta, q, T, q^v, q^l, q^i (+ trace)"""
    F, t = typed(dtype, Tf, Th), dtype
    shape = arrays["rtheta"].shape
    out = sar._empty(shape, dtype, ("theta", "q", "T", "qv", "ql", "qi"))
    out["last_residual"] = np.zeros(shape)          # |T* - T(T*)| of the iterate T* at which the condensate was split (0 for clear parcels)
    pst, abstol = t(pst), t(solver[0])
    with np.errstate(all="ignore"):
        for idx in np.ndindex(shape):
            rho, pr = t(rho_r[idx[0]]), t(p_r[idx[0]])
            th, q = t(arrays["rtheta"][idx]) / rho, t(arrays["rq"][idx]) / rho
            T, qv, ql, qi, tr = F.adjust_mixed(th, q, pr, pst, abstol, solver[1], force_branch)
            sar._record(out, idx, tr, float(solver[0]))
            out.last_residual[idx] = float(tr.residuals[-1]) if tr.residuals else 0.0
            out.theta[idx], out.q[idx], out.T[idx], out.qv[idx], out.ql[idx], out.qi[idx] = th, q, T, qv, ql, qi
    return out


@functools.lru_cache(maxsize=None)
def restated(shape, dtype, solver=sar.DEFAULT_SOLVER, force_branch=None, which=0):
    case = mixed_case(shape, which)
    return diagnose_mixed(case, case.p_r, case.rho_r, dtype, solver, force_branch)


def distances(a, b):
    """sar.distances with q^i beside q^l"""
    d = sar.distances(a, b)
    wide = np.longdouble
    d["qi"] = np.abs(a["qi"].astype(wide) - b["qi"].astype(wide)).astype(np.float64)
    return d


def own_distance(a, b, tag):
    """{population: (dT rel, dq^v, dq^l, dq^i)} between two restatements of one case; knife-edge parcels and parcels on different branches
    are left out, as the judging leaves them out"""
    d = distances(a, b)
    keep = ~a.knife & (a.branch == b.branch)
    out = {}
    for name in POPULATIONS:
        sel = (tag == name) & keep
        if (tag == name).any():
            out[name] = tuple(float(d[n][sel].max()) if sel.any() else 0.0 for n in NAMES)
    return out


@functools.lru_cache(maxsize=None)
def d80(shape, solver=sar.DEFAULT_SOLVER):
    """the restatement's own rounding sensitivity, float64 against longdouble, per population"""
    return own_distance(restated(shape, np.float64, solver), restated(shape, np.longdouble, solver), mixed_case(shape).tag)


EXACT_MARGIN = 4.0                   # K


def exact_partition_masks(want, tag):
    """(warm, ice): the warm cloudy parcels whose q^i, and the all-ice parcels whose q^l, must be an exact zero.  The condensate is split at
    the last secant iterate T*, which lies within |r| = |T* - T| of the returned T; the rule holds where T* is at least EXACT_MARGIN kelvin
    beyond the kink (T - |r| >= T^f + 4 K; T + |r| <= T^h - 4 K).  Under a converged solver (|r| <= abstol) that is every parcel of the two
    populations (final T >= T^f + 5 K / <= T^h - 5 K; asserted on the CPU); under maxiter = 0 or 2 a parcel that is still kelvins from
    its root may be split inside the mixed range, by the restatement as by the device, and is judged by the bounds alone."""
    cloudy = want["branch"] == CLOUDY
    T, r = want["T"].astype(np.float64), want["last_residual"]
    return (tag == "warm_cloudy") & cloudy & (T - r >= TF + EXACT_MARGIN), (tag == "all_ice") & cloudy & (T + r <= TH - EXACT_MARGIN)


def _as_liquid(r, name):
    """the (T, q^v, q^l) view sar.judge64 / sar.judge32 take, with `name` (ql or qi) in the q^l slot"""
    if r is None:
        return None
    out = sar.Result({k: r[k] for k in ("T", "qv", "q", "branch", "knife") if k in r})
    out["ql"] = r[name]
    return out


def judge64(dev, want, tag, table, clear=None, cloudy=None):
    """sar.judge64, unchanged, twice: on (T, q^v, q^l) and on (T, q^v, q^i), each with its own row of `table` ({population: (dT, dq^v, dq^l,
    dq^i)}).  Clear parcels therefore hold exact zeros in q^l AND q^i and the bits of q^t in q^v.  Then the two exact rules of the mixed
    phase: warm cloudy parcels hold an exact zero in q^i, all-ice parcels an exact zero in q^l.
    -> (failures, {population: largest device distance (T, q^v, q^l, q^i)}, skipped)"""
    fails, skipped = {}, 0
    for name, col in (("ql", 2), ("qi", 3)):
        rows = {p: (r[0], r[1], r[col]) for p, r in table.items()}
        f, _, skipped = sar.judge64(_as_liquid(dev, name), _as_liquid(want, name), tag, rows, _as_liquid(clear, name), _as_liquid(cloudy, name))
        fails.update({f"{name}: {k}": v for k, v in f.items()})
    for pop, name, sel in zip(("warm_cloudy", "all_ice"), ("qi", "ql"), exact_partition_masks(want, tag)):
        if not (dev[name][sel] == 0).all():
            fails[f"{pop}: {name} an exact zero"] = int((dev[name][sel] != 0).sum())
    d = distances(dev, want)
    zero = want["branch"] == THETA_ZERO
    ordinary = ~zero & ~(tag == "marginal_edge") & ~want["knife"]
    report = {p: tuple(float(d[n][(tag == p) & ordinary].max()) for n in NAMES) for p in POPULATIONS if ((tag == p) & ordinary).any()}
    return fails, report, skipped


def judge32(dev, want32, want64, tag, qt_max, clear64, cloudy64):
    """sar.judge32, unchanged, twice (q^l, then q^i in the q^l slot).  sar.judge32 walks sar.POPULATIONS, so the populations of this sweep
    are judged under the names it knows: marginal_edge, negative_or_zero_q and theta_zero keep theirs, every other one is `bulk` — one d32
    for them all, the largest of the float32 restatement over them, within 4 of which the device must stay."""
    known = np.where(np.isin(tag, ("marginal_edge", "negative_or_zero_q", "theta_zero")), tag, "bulk")
    fails, report, table = {}, {}, {}
    for name in ("ql", "qi"):
        f, r, t = sar.judge32(_as_liquid(dev, name), _as_liquid(want32, name), _as_liquid(want64, name), known, qt_max,
                              _as_liquid(clear64, name), _as_liquid(cloudy64, name))
        fails.update({f"{name}: {k}": v for k, v in f.items()})
        report[name], table[name] = r, t
    return fails, report, table


def by_parcel(case, field):
    return field.ravel()[np.argsort(case.parcel.ravel())]


# ---- the oracle model -------------------------------------------------------------------------------------------------------------------------
def adjust_mixed_array(theta, qt, pr, pst=sar.PST, abstol=1e-4, maxiter=20, Tf=TF, Th=TH, c=None):
    """adjust_mixed of TypedMixed(float64) over arrays (theta, q^t, p_r broadcastable): the same expressions in the same order, every cell
    following its own branch and its own iteration count; numpy's pow / exp.  -> T, q^v, q^l, q^i"""
    F = typed(np.float64, Tf, Th) if c is None else TypedMixed(np.float64, Tf, Th, c)
    theta, qt, pr = np.broadcast_arrays(*(np.asarray(a, dtype=np.float64) for a in (theta, qt, pr)))

    def lam(T):
        return (np.clip(T, F.Th, F.Tf) - F.Th) / (F.Tf - F.Th)

    def psat(T, l):
        dc, L0 = l * F.dc + (1.0 - l) * F.dci, l * F.L0 + (1.0 - l) * F.L0i
        return F.ptr * (T / F.Ttr) ** (dc / F.Rv) * np.exp((1.0 / F.Ttr - 1.0 / T) * L0 / F.Rv)

    def mix(qv, ql, qi):
        qd = 1.0 - (qv + ql + qi)
        return qd * F.Rd + qv * F.Rv, qd * F.cpd + qv * F.cpv + ql * F.cl + qi * F.ci

    def temperature(th, qv, ql, qi, p):
        Rm, cpm = mix(qv, ql, qi)
        return (p / pst) ** (Rm / cpm) * th + (F.Ll * ql + F.Li * qi) / cpm

    def adjust(T, q, p):
        l = lam(T)
        ps = psat(T, l)
        qc = np.maximum(0.0, q - F.eps * (1.0 - q) * ps / (p - ps))
        return q - qc, l * qc, (1.0 - l) * qc

    with np.errstate(all="ignore"):
        zero = np.zeros_like(theta)
        T1 = temperature(theta, qt, zero, zero, pr)
        rho1 = pr / (mix(qt, zero, zero)[0] * T1)
        cloudy = ~(qt <= psat(T1, lam(T1)) / (rho1 * F.Rv * T1)) & (theta != 0)
        th, q, p, x1 = theta[cloudy], qt[cloudy], pr[cloudy], T1[cloudy]
        qv1, ql1, qi1 = adjust(x1, q, p)
        dT = (F.Ll * ql1 + F.Li * qi1) / mix(qv1, ql1, qi1)[1]
        x2 = x1 + np.maximum(0.01, dT / 2.0)

        def residual(T):
            return T - temperature(th, *adjust(T, q, p), p)
        r1, r2 = residual(x1), residual(x2)
        for _ in range(maxiter):
            active = np.abs(r2) > abstol
            if not active.any():
                break
            s = (x2 - x1) / (r2 - r1)
            valid = np.isfinite(s)
            s = np.where(valid, s, 0.0)
            nx2 = x2 - r2 * s
            nr2 = np.where(valid, residual(nx2), 0.0)
            x1, r1 = np.where(active, x2, x1), np.where(active, r2, r1)
            x2, r2 = np.where(active, nx2, x2), np.where(active, nr2, r2)
        qv, ql, qi = qt.copy(), zero.copy(), zero.copy()
        T = T1.copy()
        qv[cloudy], ql[cloudy], qi[cloudy] = adjust(x2, q, p)
        T[cloudy] = temperature(th, qv[cloudy], ql[cloudy], qi[cloudy], p)
        T[theta == 0] = 0.0
    return T, qv, ql, qi


class MixedPhaseOracleModel(OracleModel):
    """OracleModel(microphysics = "SaturationAdjustment") whose update_state! ends in the mixed-phase diagnosis (see the module header)."""

    def __init__(self, grid, freezing_temperature=TF, homogeneous_ice_nucleation_temperature=TH, **kw):
        self._Tf, self._Th = float(freezing_temperature), float(homogeneous_ice_nucleation_temperature)
        self._solver = (float(kw.get("sa_abstol", 1e-4)), int(kw.get("sa_maxiter", 20)))
        self.ql_liquid, self.qi = grid.center_field(), grid.center_field()
        kw.setdefault("microphysics", "SaturationAdjustment")
        assert kw["microphysics"] == "SaturationAdjustment"
        super().__init__(grid, **kw)

    def update_state(self, compute_tendencies=True):
        closure, forcings = self.closure, self.forcings
        self.closure = self.forcings = None          # they read T and the moisture fractions: after the mixed diagnosis
        try:
            super().update_state(compute_tendencies=False)
        finally:
            self.closure, self.forcings = closure, forcings
        g, I = self.grid, self.grid.interior
        pr = self.ref.pressure[g.Hz:g.Hz + g.Nz][:, None, None]
        T, qv, ql, qi = adjust_mixed_array(I(self.theta), I(self.q), pr, self.ref.pst, *self._solver, Tf=self._Tf, Th=self._Th)
        I(self.T)[...], I(self.qv)[...], I(self.ql_liquid)[...], I(self.qi)[...] = T, qv, ql, qi
        I(self.ql)[...] = ql + qi                    # what og_w_tendency_moist loads the buoyancy with
        for f in (self.T, self.qv, self.ql, self.ql_liquid, self.qi):
            self._halo_center(f)
        if self.closure is not None:
            from oracle.closure import compute_closure_fields
            compute_closure_fields(self)
        if self.forcings is not None:
            from oracle.forcings import compute_forcings
            compute_forcings(self)
        if compute_tendencies:
            self.compute_tendencies()
