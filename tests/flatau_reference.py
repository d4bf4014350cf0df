"""Typed restatement of the saturation adjustments under ThermodynamicConstants(saturation_vapor_pressure = FlatauPolynomial()), the parcel
sweeps that drive them and the oracle models that carry them.  TEST INFRASTRUCTURE ONLY.

What is restated (src/Thermodynamics/flatau_polynomial.jl:61-122): with x = max(T - T_r, -delta T), T_r = 273.16 K, delta T = 80 K,
    p^v+l = sum_n a^l_n x^n,   p^v+i = sum_n a^i_n x^n   (n = 0 .. 8; evalpoly: Horner from the highest coefficient down),
    mixed surface: lambda p^v+l + (1 - lambda) p^v+i     (two polynomials blended, not blended coefficients).
Everything around p^v+ is what saturation_adjustment_reference.Typed and mixed_phase_reference.TypedMixed restate; the classes here override
the saturation pressure and nothing else:
    TypedFlatau(sar.Typed)              psat                 device: bz_sa_diagnose<true>, bz_ds_adjust<true> (bz_fl_psat_liquid)
    TypedFlatauMixed(mpr.TypedMixed)    psat, psat_mixed     device: bz_mp_diagnose<true> (bz_fl_psat_mixed)
The Horner steps are one multiplication and one addition in the type of the restatement; the device fuses each into one fma.  That
difference is of the size of the restatement's own float64-to-longdouble distance d80, which is what the judging rules scale by.

The sweeps are those of the two helper modules, built again with the polynomial in the place of the Clausius-Clapeyron expression: the
builders and the cell-by-cell diagnoses of sar and mpr look their formulas up through the module-level `typed` factory, and `polynomial()`
puts the factories of this module there for the duration of a call.  Their caches are not touched: a builder is called through __wrapped__,
and the cached functions of this module (anelastic_case, compressible_case, mixed_case, restated, d80, ...) are its own.  Marginal parcels
therefore sit at the POLYNOMIAL's threshold, the mixed populations straddle the kinks of lambda as before, and the all-ice population
(T* from 190 K) and the density-form bulk (down to ~115 K) put parcels on both sides of the clamp at T_r - delta T = 193.16 K.

Array forms (numpy's own arithmetic, every cell on its own branch and iteration count) for the oracle models:
    adjust_pressure_array               warm (equilibrium = None) and mixed ((T^f, T^h)) pressure form
    FlatauOracleModel, FlatauMixedOracleModel     OracleModel whose update_state! ends in that diagnosis, as MixedPhaseOracleModel does
    FlatauCompressibleOracle            CompressibleOracleModel whose _sa_thermo runs TypedFlatau(float64).adjust_density cell by cell"""
import contextlib
import functools

import numpy as np

import mixed_phase_reference as mpr
import saturation_adjustment_reference as sar
from oracle.oracle import OracleModel
from oracle.oracle_compressible import CompressibleOracleModel

# Flatau, Walko and Cotton (1992), relative-error-norm fits (their Tables 3 and 4), hPa -> Pa (flatau_polynomial.jl:64-69)
LIQUID = (611.239921, 44.3987641, 1.42986287, 2.64847430e-2, 3.02950461e-4, 2.06739458e-6, 6.40689451e-9, -9.52447341e-12, -9.76195544e-14)
ICE = (611.147274, 50.3160820, 1.88439774, 4.20895665e-2, 6.15021634e-4, 6.02588177e-6, 3.85852041e-8, 1.46898966e-10, 2.52751365e-13)
T_REF, T_OFFSET = 273.16, 80.0
CLAMP = T_REF - T_OFFSET
TF, TH = mpr.TF, mpr.TH
# (grid, secant solver) of every diagnosis sweep tests/test_flatau.py runs, per form; tests/test_flatau_reference.py asserts the sweep
# conditions for each.  The small grids also run maxiter = 0 and 2 (the maxiter exit) and abstol = 0 (until the `valid` guard fires)
SWEEPS = {"pressure": [(sar.ANELASTIC_GRIDS[0], s) for s in sar.SOLVERS] + [(sar.ANELASTIC_GRIDS[1], sar.DEFAULT_SOLVER)],
          "mixed": [(sar.ANELASTIC_GRIDS[0], s) for s in sar.SOLVERS] + [(sar.ANELASTIC_GRIDS[1], sar.DEFAULT_SOLVER)],
          "density": [(sar.COMPRESSIBLE_GRIDS[0], s) for s in sar.SOLVERS] + [(sar.COMPRESSIBLE_GRIDS[1], sar.DEFAULT_SOLVER)]}


class _Polynomial:
    """the coefficients in the type of the restatement, and the two chains"""

    ps_max = -np.inf                 # the largest p^v+ evaluated since it was last reset (evaluation_margin)

    def _seen(self, ps):
        if ps > self.ps_max:
            self.ps_max = ps
        return ps

    def _set_polynomial(self, liquid=LIQUID, ice=ICE, reference_temperature=T_REF, minimum_temperature_offset=T_OFFSET):
        t = self.dtype
        self.fl_liquid, self.fl_ice = tuple(t(a) for a in liquid), tuple(t(a) for a in ice)
        self.fl_Tr, self.fl_dT = t(reference_temperature), t(minimum_temperature_offset)

    def fl_x(self, T):
        return max(T - self.fl_Tr, -self.fl_dT)

    @staticmethod
    def _chain(a, x):
        p = a[8]
        for n in range(7, -1, -1):
            p = p * x + a[n]
        return p

    def psat_liquid(self, T):
        return self._chain(self.fl_liquid, self.fl_x(T))

    def psat_ice(self, T):
        return self._chain(self.fl_ice, self.fl_x(T))


class TypedFlatau(sar.Typed, _Polynomial):
    def __init__(self, dtype, c=None, **polynomial):
        super().__init__(dtype, c)
        self._set_polynomial(**polynomial)

    def psat(self, T):
        return self._seen(self.psat_liquid(T))


class TypedFlatauMixed(mpr.TypedMixed, _Polynomial):
    def __init__(self, dtype, Tf=TF, Th=TH, c=None, **polynomial):
        super().__init__(dtype, Tf, Th, c)
        self._set_polynomial(**polynomial)

    def psat(self, T):
        return self._seen(self.psat_liquid(T))

    def psat_mixed(self, T, lam):
        return self._seen(lam * self.psat_liquid(T) + (self.dtype(1) - lam) * self.psat_ice(T))


@functools.lru_cache(maxsize=None)
def typed(dtype):
    return TypedFlatau(dtype)


@functools.lru_cache(maxsize=None)
def typed_mixed(dtype, Tf=TF, Th=TH):
    return TypedFlatauMixed(dtype, Tf, Th)


# polynomial() below relies on the helper modules looking `typed` up as a module global at call time; a helper that bound it early (a default
# argument, a closure) would silently keep the Clausius-Clapeyron formulas.  Checked here, once, for every function this module drives
for _f in (sar.anelastic_case.__wrapped__, sar.density_parcels.__wrapped__, sar.diagnose_anelastic, sar.diagnose_compressible,
           mpr.mixed_case.__wrapped__, mpr.diagnose_mixed):
    assert "typed" in _f.__code__.co_names and "typed" in _f.__globals__, f"{_f.__module__}.{_f.__name__} no longer looks `typed` up as a module global"


@contextlib.contextmanager
def polynomial():
    """inside: the builders and diagnoses of sar and mpr evaluate the polynomial (see the module header)"""
    saved = sar.typed, mpr.typed
    sar.typed, mpr.typed = typed, typed_mixed
    try:
        yield
    finally:
        sar.typed, mpr.typed = saved


# ---- the sweeps ---------------------------------------------------------------------------------------------------------------------------
ALL_ITERATES = (0.0, 50)             # abstol = 0: the secant visits every iterate any other solver of sar.SOLVERS stops at
FIXED_POPULATIONS = ("marginal", "marginal_edge", "guess_switch", "negative_or_zero_q", "theta_zero")


def evaluation_margin(form, case, solver=ALL_ITERATES):
    """per cell of a pressure-form case: p_r minus the largest p^v+ the float64 adjustment evaluates on its way (first guess, threshold, every
    secant iterate, the final partition); +inf where theta = 0"""
    F, f = (typed_mixed if form == "mixed" else typed)(np.float64), np.float64
    out = np.full(case.rtheta.shape, np.inf)
    with np.errstate(all="ignore"):
        for idx in np.ndindex(out.shape):
            rho, pr = f(case.rho_r[idx[0]]), f(case.p_r[idx[0]])
            th, q = f(case.rtheta[idx]) / rho, f(case.rq[idx]) / rho
            if th == 0:
                continue
            F.ps_max = -np.inf
            (F.adjust_mixed if form == "mixed" else F.adjust_pressure)(th, q, pr, f(sar.PST), f(solver[0]), solver[1])
            out[idx] = float(pr - F.ps_max)
    return out


def _keep_below_the_reference_pressure(form, case):
    """The sweeps of sar and mpr reach q^t = 0.04 at 20 - 30 kPa (and 0.03 at 2 - 4 kPa on the tall column); there the second secant iterate of a
    few parcels overshoots to a temperature whose p^v+ exceeds p_r, where q^v+ = eps (1 - q^t) p^v+ / (p_r - p^v+) changes sign.  Such a parcel
    is dried (q^t halved, as often as needed) until every evaluation of its adjustment keeps p_r - p^v+ > 0; parcels whose q^t carries their
    population's meaning are never touched (none of them overshoots: asserted)."""
    rq = case.rq.copy()
    for _ in range(12):
        bad = evaluation_margin(form, sar.Case(case, rq=rq)) <= 0
        if not bad.any():
            break
        assert not np.isin(case.tag[bad], FIXED_POPULATIONS).any()
        rq[bad] *= 0.5
    else:
        raise AssertionError("parcels above the reference pressure remain")
    return sar.Case(case, rq=rq, dried=(rq != case.rq))


COLD_SHARE, COLD_RANGE = 0.04, (165.0, 193.0)      # of the bulk parcels; target temperatures below the clamp at T_r - delta T = 193.16 K
SMALL_CLOUD_LEVELS, SMALL_CLOUD_T, SMALL_CLOUD_Q = 3, (TF + 5.5, TF + 12.0), (3e-5, 3e-4)      # the clear parcels of the lowest levels become these


def _draws(case, seed, count):
    """`count` uniform draws per PARCEL (not per cell): both placements of a case change the same parcels in the same way"""
    return np.random.default_rng(seed).random((count, case.parcel.size))


def _with_cold_bulk(case):
    """sar.anelastic_case targets 220 .. 310 K: no parcel of it reaches the clamp x = -delta T of the polynomial.  A share COLD_SHARE of its bulk
    parcels is rebuilt, by the builder's own recipe (theta = T / Pi_d of the level, q^t = s q*(T, p_r) with s log-uniform in [0.05, 4]: clear
    and cloudy), at a target temperature in COLD_RANGE, where p^v+ is the constant the clamp leaves"""
    from oracle import thermo
    F, f, kd = typed(np.float64), np.float64, thermo.ThermoConstants()
    u = _draws(case, 85, 3)
    rtheta, rq, tag = case.rtheta.copy(), case.rq.copy(), case.tag.copy()
    cold = np.zeros(tag.shape, bool)
    for idx in np.ndindex(tag.shape):
        n = case.parcel[idx]
        if tag[idx] != "bulk" or u[0, n] >= COLD_SHARE:
            continue
        pr, rho = case.p_r[idx[0]], case.rho_r[idx[0]]
        T = COLD_RANGE[0] + u[1, n] * (COLD_RANGE[1] - COLD_RANGE[0])
        s = 10.0 ** (np.log10(0.05) + u[2, n] * (np.log10(4.0) - np.log10(0.05)))
        qt = s * float(F.threshold_pressure(f(T), f(0), f(pr)))
        rtheta[idx], rq[idx], cold[idx] = rho * (T / (pr / sar.PST) ** (kd.Rd / kd.cpd)), rho * qt, True
    return sar.Case(case, rtheta=rtheta, rq=rq, cold=cold)


def _with_small_warm_clouds(case):
    """Under SecantSolver(maxiter = 0) the condensate is split at the second GUESS x2 = T1 + max(0.01, dT / 2), T1 the temperature of the parcel
    without condensate.  For a warm parcel adjusted to T* with condensate q^c, T1 = T* - D (D = L q^c / c_pm) and dT = D (1 + g) with
    g = L^2 q^v+ / (c_pm R^v T^2), so x2 = T* + D (g - 1) / 2 and the condensate left at x2 is q^c (1 - g (g - 1) / 2): none once g >= 2
    (above ~285 K, or at low pressure), and none where the 0.01 K floor exceeds D (q^c below ~1e-5).  Most warm cloudy parcels of
    mpr.mixed_case are one or the other, or their guess falls into the mixed range.  The clear parcels of the SMALL_CLOUD_LEVELS lowest levels
    (p_r >= 54 kPa) therefore become warm cloudy parcels with T* in SMALL_CLOUD_T and q^c log-uniform in SMALL_CLOUD_Q, built backwards from
    (T*, q^c) as mpr.mixed_case builds its own: g < 2, D >= 0.07 K, every guess and iterate above T^f + 4 K — liquid only under every solver"""
    F, f = typed_mixed(np.float64), np.float64
    u = _draws(case, 86, 3)
    pst = f(sar.PST)
    limit = [mpr._host_limit(F, f(p)) for p in case.p_r]
    rtheta, rq, tag, target = case.rtheta.copy(), case.rq.copy(), case.tag.copy(), case.target.copy()
    with np.errstate(all="ignore"):
        for idx in np.ndindex(tag.shape):
            n, Tmax = case.parcel[idx], limit[idx[0]]
            if tag[idx] != "clear" or idx[0] >= SMALL_CLOUD_LEVELS:
                continue
            pr, rho = f(case.p_r[idx[0]]), case.rho_r[idx[0]]
            T = f(SMALL_CLOUD_T[0] + u[1, n] * (min(Tmax, SMALL_CLOUD_T[1]) - SMALL_CLOUD_T[0]))
            qc = f(SMALL_CLOUD_Q[0] * (SMALL_CLOUD_Q[1] / SMALL_CLOUD_Q[0]) ** u[2, n])
            ps = F.psat_mixed(T, F.lam(T))
            r = ps / (pr - ps)
            qv = F.eps * (f(1) - qc) * r / (f(1) + F.eps * r)
            rtheta[idx], rq[idx] = rho * float(F.theta_of(T, qv, qc, f(0), pr, pst)), rho * float(qv + qc)
            tag[idx], target[idx] = "warm_cloudy", float(T)
    return sar.Case(case, rtheta=rtheta, rq=rq, tag=tag, target=target)


@functools.lru_cache(maxsize=None)
def anelastic_case(shape, Lz=sar.COLUMN, which=0, bulk_only=False):
    with polynomial():
        case = sar.anelastic_case.__wrapped__(shape, Lz, which, False, bulk_only)
    return _keep_below_the_reference_pressure("pressure", _with_cold_bulk(case))


@functools.lru_cache(maxsize=None)
def _density_parcels(n, bulk_only=False):
    with polynomial():
        return sar.density_parcels.__wrapped__(n, 80, bulk_only)


@functools.lru_cache(maxsize=None)
def compressible_case(shape, which=0, bulk_only=False):
    """sar.compressible_case (without the Kessler condensate) from the density parcels of the polynomial"""
    theta, rho, qt, tag, sub = _density_parcels(shape[0] * shape[1] * shape[2], bulk_only)
    rq = rho * qt
    rho_d = rho - rq
    rtheta = np.where(tag == "theta_zero", 0.0, rho_d * theta)
    P = sar.placement(shape, which)
    return sar.Case(rho_d=rho_d[P], rtheta=rtheta[P], rq=rq[P], tag=tag[P], sub=sub[P], parcel=P)


@functools.lru_cache(maxsize=None)
def mixed_case(shape, which=0):
    with polynomial():
        case = mpr.mixed_case.__wrapped__(shape, which)
    return _keep_below_the_reference_pressure("mixed", _with_small_warm_clouds(case))


def diagnose_anelastic(arrays, p_r, rho_r, dtype=np.float64, solver=sar.DEFAULT_SOLVER, force_branch=None):
    with polynomial():
        return sar.diagnose_anelastic(arrays, 1, p_r, rho_r, dtype, solver, force_branch)


def diagnose_compressible(arrays, dtype=np.float64, solver=sar.DEFAULT_SOLVER, newton=sar.NEWTON, force_branch=None):
    with polynomial():
        return sar.diagnose_compressible(arrays, 1, dtype, solver, newton, force_branch)


def diagnose_mixed(arrays, p_r, rho_r, dtype=np.float64, solver=sar.DEFAULT_SOLVER, force_branch=None):
    with polynomial():
        return mpr.diagnose_mixed(arrays, p_r, rho_r, dtype, solver, force_branch)


@functools.lru_cache(maxsize=None)
def restated(form, shape, dtype, solver=sar.DEFAULT_SOLVER, force_branch=None, which=0):
    """form: "pressure" (anelastic_case), "density" (compressible_case) or "mixed" (mixed_case)"""
    if form == "density":
        return diagnose_compressible(compressible_case(shape, which), dtype, solver, force_branch=force_branch)
    case = mixed_case(shape, which) if form == "mixed" else anelastic_case(shape, which=which)
    return (diagnose_mixed if form == "mixed" else diagnose_anelastic)(case, case.p_r, case.rho_r, dtype, solver, force_branch)


def case_of(form, shape, which=0):
    return {"pressure": anelastic_case, "density": compressible_case, "mixed": mixed_case}[form](shape, which=which)


def own_distance(a, b, tag):
    """{population: (dT rel, dq^v, dq^l)} between two warm restatements; knife-edge parcels and parcels on different branches are left
    out, as the judging leaves them out (sar.d80)"""
    d = sar.distances(a, b)
    keep = ~a.knife & (a.branch == b.branch)
    per = {n: sar.by_population(tag, d[n], keep) for n in ("T", "qv", "ql")}
    return {name: tuple(per[n].get(name, 0.0) for n in ("T", "qv", "ql")) for name in sar.POPULATIONS if (tag == name).any()}


@functools.lru_cache(maxsize=None)
def d80(form, shape, solver=sar.DEFAULT_SOLVER):
    """the restatement's own rounding sensitivity, float64 against longdouble, per population"""
    a, b = restated(form, shape, np.float64, solver), restated(form, shape, np.longdouble, solver)
    tag = case_of(form, shape).tag
    return mpr.own_distance(a, b, tag) if form == "mixed" else own_distance(a, b, tag)


def knife_edge(a, b, tag):
    """parcels whose float64 (a) and longdouble (b) restatements take different branches or iteration counts, or whose |r2| passes within
    sar.KNIFE_EDGE of abstol; threshold parcels aside, which are judged on either branch (the count tests/test_mixed_phase_reference.py caps)"""
    return (a.knife | (a.branch != b.branch) | (a.iterations != b.iterations)) & ~(tag == "marginal_edge")


def float32_knife_edge(want32, want64, abstol):
    """The Float32 analogue of the exclusion the Float64 rule makes, for a solver that stops on abstol > 0.  In Float32 the residual of the secant
    carries ~3e-5 K of rounding, a third of the default abstol = 1e-4 K, so two float32 arithmetics (the device's fma and powf, numpy's) may stop
    at iterates up to abstol apart.  Two kinds of parcel are not decided beyond that and are left out of the judging; the callers print how many:
      - parcels whose float32 and float64 restatements OF THE SAME (Float32) INPUTS take different branches or iteration counts;
      - cloudy-branch parcels whose condensate is smaller than what abstol resolves, q^l <= (dq^v+/dT) abstol with dq^v+/dT = q^v+ L / (R^v T^2)
        (about 1.4e-7 at 300 K): whether such a parcel ends with q^l = 0 or with a few 1e-8 is the position of the last iterate inside the
        tolerance.  Measured: the one threshold parcel of the density sweep that missed 4 d32 = 2.3e-8 holds q^l = 4.3e-8 on the device and an
        exact 0 in both restatements, its temperatures 1.6e-4 K apart.
    sar.judge32 has no such rule.  Nothing is left out under abstol = 0, where every parcel runs until the secant stagnates."""
    if not abstol > 0:
        return np.zeros(want32.branch.shape, bool)
    F = typed(np.float64)
    T, qv, ql = (want64[n].astype(np.float64) for n in ("T", "qv", "ql"))
    with np.errstate(all="ignore"):
        unresolved = (want64.branch == sar.CLOUDY) & (ql <= qv * float(F.Ll) / (float(F.Rv) * T * T) * abstol)
    return (want32.iterations != want64.iterations) | (want32.branch != want64.branch) | unresolved


# ---- array forms and the oracle models --------------------------------------------------------------------------------------------------------
def adjust_pressure_array(theta, qt, pr, pst=sar.PST, abstol=1e-4, maxiter=20, equilibrium=None, F=None):
    """adjust_pressure of TypedFlatau(float64) (equilibrium = None: warm phase) or adjust_mixed of TypedFlatauMixed(float64) (equilibrium =
    (T^f, T^h)) over arrays: the same expressions in the same order, every cell following its own branch and iteration count.
    -> T, q^v, q^l, q^i (q^i exact zeros in the warm phase, where lambda = 1 and every ice term is an exact + 0)"""
    mixed = equilibrium is not None
    F = F or (typed_mixed(np.float64, *equilibrium) if mixed else typed_mixed(np.float64))
    theta, qt, pr = np.broadcast_arrays(*(np.asarray(a, dtype=np.float64) for a in (theta, qt, pr)))

    def lam(T):
        return (np.clip(T, F.Th, F.Tf) - F.Th) / (F.Tf - F.Th) if mixed else np.ones_like(T)

    def chain(a, x):
        p = np.full_like(x, a[8])
        for n in range(7, -1, -1):
            p = p * x + a[n]
        return p

    def psat(T, l):
        x = np.maximum(T - F.fl_Tr, -F.fl_dT)
        return l * chain(F.fl_liquid, x) + (1.0 - l) * chain(F.fl_ice, x) if mixed else chain(F.fl_liquid, x)

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


class FlatauMixedOracleModel(mpr.MixedPhaseOracleModel):
    """MixedPhaseOracleModel whose update_state! ends in the polynomial's mixed diagnosis (the method of the parent class with
    adjust_pressure_array in the place of mpr.adjust_mixed_array)"""

    _equilibrium = True

    def update_state(self, compute_tendencies=True):
        closure, forcings = self.closure, self.forcings
        self.closure = self.forcings = None          # they read T and the moisture fractions: after the diagnosis
        try:
            OracleModel.update_state(self, compute_tendencies=False)
        finally:
            self.closure, self.forcings = closure, forcings
        g, I = self.grid, self.grid.interior
        pr = self.ref.pressure[g.Hz:g.Hz + g.Nz][:, None, None]
        T, qv, ql, qi = adjust_pressure_array(I(self.theta), I(self.q), pr, self.ref.pst, *self._solver,
                                              equilibrium=(self._Tf, self._Th) if self._equilibrium else None)
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


class FlatauOracleModel(FlatauMixedOracleModel):
    """OracleModel(microphysics = "SaturationAdjustment") whose update_state! ends in the polynomial's WARM diagnosis: q^i stays an exact
    zero and `ql` is q^l"""

    _equilibrium = False


class FlatauCompressibleOracle(CompressibleOracleModel):
    """CompressibleOracleModel(microphysics = "SaturationAdjustment") with the polynomial inside the density-based adjustment;
    refresh_linearization is the parent's (it reads the q^v, q^l this leaves)"""

    def _sa_thermo(self):
        F, f = typed(np.float64), np.float64
        I = self.grid.interior
        rd, r = I(self.rho_d), I(self.rho)
        th, qt = I(self.rtheta) / rd, I(self.rq) / r
        I(self.theta)[...], I(self.q)[...] = th, qt
        T, qv, ql, p = I(self.T), I(self.qv), I(self.ql), I(self.p)
        with np.errstate(all="ignore"):
            for idx in np.ndindex(th.shape):
                T[idx], qv[idx], ql[idx] = F.adjust(f(th[idx]), f(qt[idx]), f(r[idx]), f(self.pst), f(self.sa_solver[0]), self.sa_solver[1],
                                                    f(self.newton[0]), self.newton[1])
                p[idx] = r[idx] * F._mix(f(qv[idx]), f(ql[idx]))[0] * T[idx]
