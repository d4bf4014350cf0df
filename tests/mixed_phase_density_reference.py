"""Typed restatement of the DENSITY form of the mixed-phase saturation adjustment, the parcel sweep that drives it and a compressible oracle
model that carries it.  TEST INFRASTRUCTURE ONLY.

What is restated (every constant and every intermediate in ONE numpy scalar type, in the manner of mixed_phase_reference.TypedMixed, which
this subclasses; in float64 pow and exp are libm's, the functions oracle/thermo.py calls):
  adjust_thermodynamic_state(::LiquidIceDensityState, ::SaturationAdjustment{MixedPhaseEquilibrium})
      src/Microphysics/saturation_adjustment.jl:241-253 (saturated_density_residual: q^v+ = p^v+ / (rho R^v T) over the surface equilibrated at
          T, the partition of :92-100, r(T) = (T - L) (p_st / (rho R_m T))^(R_m / c_pm) - theta_0 with L = (L_l q^l + L_i q^i) / c_pm),
      :264-293 (theta = 0, the clear exit, the second guess T_1 + max(0.01, dT / 2), the secant, the final partition)
      src/Thermodynamics/dynamic_states.jl:197-232 (temperature(::LiquidIceDensityState): Newton on T = (rho R_m T / p_st)^kappa theta + L)
      src/Thermodynamics/vapor_saturation.jl:170-185 (lambda(T) and the blended Clausius-Clapeyron surface; flatau_polynomial.jl:93-122 under
          FlatauPolynomial: flatau_reference._Polynomial)
  device: bz_ds_adjust_mixed<FL> (csrc/bz_internal.h) inside k_cmp_diagnose<.., 4 | 5> and k_ac_stage_end<.., 4 | 5, ..>.
With T^f and T^h below every parcel lambda = 1 everywhere and the float64 restatement returns the bits of oracle.thermo.adjust_warm_phase_density
(tests/test_mixed_phase_density_reference.py).

TypedMixedDensity.adjust(theta, q^t, rho, p_st, secant, newton) -> (T, q^v, q^l, q^i, Trace); Trace.final_iterate is the secant iterate T* at
which the condensate was split (the returned T is the Newton temperature of that partition).

The sweep (deterministic, seeded).  Levels carry the densities of sar.reference_column over sar.COLUMN (1.1 to 0.4 kg/m^3: the tested domain
of the density form, p >= 20 kPa, so that theta stays in the 250 - 400 K of sar's density sweep; the 24 km column of the pressure-form sweep
would put theta above 500 K on its top levels, where the Float32 residual's rounding, eps32 theta, reaches a third of abstol and the share
of parcels flr.float32_knife_edge leaves out grows with it), each parcel its level's density times a factor in [0.9, 1.1]; every level hosts
the all-ice population, whose q^v+ is small at any density.  A parcel is built backwards from a target adjusted state: T*, q^c and rho give lambda(T*),
q^v = q^v+(T*, rho), q^t = q^v + q^c and theta = (T* - L) (p_st / p)^kappa with p = rho R_m T*.  The populations are mpr.POPULATIONS, a
parcel's population drawn among those its level hosts (a level hosts T* only where q^v+(T*, 0.9 rho_level) <= mpr.Q_HOST); sar.placement
places the parcels, in both placements.  A case holds rho_d = rho - rho q^t, rho theta = rho_d theta and rho q^t, the arrays a device model
is given; the restatement starts from those arrays and repeats the kernel's first lines.

MixedCompressibleOracle(CompressibleOracleModel): _sa_thermo runs the float64 restatement cell by cell and carries q^i (`self.qi`);
refresh_linearization forms gamma R_m with q^d = 1 - q^v - q^l - q^i and c_pm with c_i q^i (acoustic_substepping.jl:390-410)."""
import functools

import numpy as np

import flatau_reference as flr
import mixed_phase_reference as mpr
import saturation_adjustment_reference as sar
from oracle.oracle_compressible import CompressibleOracleModel

TF, TH = mpr.TF, mpr.TH
CLEAR, CLOUDY, THETA_ZERO = sar.CLEAR, sar.CLOUDY, sar.THETA_ZERO
NAMES = mpr.NAMES
DENSITY_SPREAD = (0.9, 1.1)          # a parcel's density: its level's times a factor drawn from this range


class Trace(sar.Trace):
    __slots__ = ("final_iterate",)

    def __init__(self):
        super().__init__()
        self.final_iterate = None


class TypedMixedDensity(mpr.TypedMixed):
    """mpr.TypedMixed with the density form"""

    def temperature_mixed(self, theta, qv, ql, qi, rho, pst, abstol, maxiter, leave_out_ci=False):
        """temperature(::LiquidIceDensityState) with ice; leave_out_ci: the planted error of tests/test_mixed_phase_density_reference.py"""
        t = self.dtype
        Rm, cpm = self._mix3(qv, ql, qi)
        if leave_out_ci:
            cpm = cpm - qi * self.ci
        kap, gam = Rm / cpm, cpm / (cpm - Rm)
        L = (self.Ll * ql + self.Li * qi) / cpm
        T = self.pw(theta, gam) * self.pw(rho * Rm / pst, gam - t(1)) + L
        dT, it = T, 0
        while abs(dT) > abstol and it < maxiter:
            Phi = self.pw(rho * Rm * T / pst, kap) * theta
            dT = -(T - Phi - L) / (t(1) - kap * Phi / T)
            T = T + dT
            it += 1
        return T

    def saturated_vapor_density(self, T, rho):
        return self.psat_mixed(T, self.lam(T)) / (rho * self.Rv * T)

    def residual_mixed(self, T, theta0, rho, qt, pst):
        t = self.dtype
        lam = self.lam(T)
        qc = max(t(0), qt - self.saturated_vapor_density(T, rho))
        qv, ql, qi = qt - qc, lam * qc, (t(1) - lam) * qc
        Rm, cpm = self._mix3(qv, ql, qi)
        L = (self.Ll * ql + self.Li * qi) / cpm
        p = rho * Rm * T
        return (T - L) * self.pw(pst / p, Rm / cpm) - theta0, qv, ql, qi

    def adjust_density_mixed(self, theta, qt, rho, pst, abstol, maxiter, newton_abstol, newton_maxiter, force_branch=None, leave_out_ci=False):
        t, tr = self.dtype, Trace()
        if theta == 0:
            tr.branch = THETA_ZERO
            return t(0), qt, t(0), t(0), tr
        T1 = self.temperature_mixed(theta, qt, t(0), t(0), rho, pst, newton_abstol, newton_maxiter)
        clear = bool(qt <= self.saturated_vapor_density(T1, rho)) if force_branch is None else force_branch == "clear"
        tr.nonfinite |= not np.isfinite(T1)
        if clear:
            return T1, qt, t(0), t(0), tr
        tr.branch = CLOUDY
        _, qv1, ql1, qi1 = self.residual_mixed(T1, theta, rho, qt, pst)
        dT = (self.Ll * ql1 + self.Li * qi1) / self._mix3(qv1, ql1, qi1)[1]
        tr.half_step = dT / t(2)
        T2 = T1 + max(t(0.01), dT / t(2))
        Ts = self._secant(lambda T: self.residual_mixed(T, theta, rho, qt, pst)[0], T1, T2, abstol, maxiter, tr)
        tr.final_iterate = Ts
        _, qv, ql, qi = self.residual_mixed(Ts, theta, rho, qt, pst)
        T = self.temperature_mixed(theta, qv, ql, qi, rho, pst, newton_abstol, newton_maxiter, leave_out_ci)
        tr.nonfinite |= not (np.isfinite(T) and np.isfinite(ql) and np.isfinite(qi))
        return T, qv, ql, qi, tr

    def adjust(self, theta, qt, rho, pst, secant=sar.DEFAULT_SOLVER, newton=sar.NEWTON):
        t = self.dtype
        return self.adjust_density_mixed(theta, qt, rho, t(pst), t(secant[0]), secant[1], t(newton[0]), newton[1])

    def theta_of_density(self, T, qv, ql, qi, rho, pst):
        """theta^li of a known (T, q, rho): (T - L) (p_st / p)^kappa, p = rho R_m T"""
        Rm, cpm = self._mix3(qv, ql, qi)
        return (T - (self.Ll * ql + self.Li * qi) / cpm) * self.pw(pst / (rho * Rm * T), Rm / cpm)


class TypedFlatauMixedDensity(TypedMixedDensity, flr._Polynomial):
    """the same over flr's polynomial surface (the overrides of flr.TypedFlatauMixed)"""

    def __init__(self, dtype, Tf=TF, Th=TH, c=None, **polynomial):
        super().__init__(dtype, Tf, Th, c)
        self._set_polynomial(**polynomial)

    def psat(self, T):
        return self.psat_liquid(T)

    def psat_mixed(self, T, lam):
        return lam * self.psat_liquid(T) + (self.dtype(1) - lam) * self.psat_ice(T)


@functools.lru_cache(maxsize=None)
def typed(dtype, polynomial=False, Tf=TF, Th=TH):
    return (TypedFlatauMixedDensity if polynomial else TypedMixedDensity)(dtype, Tf, Th)


# ---- the sweep --------------------------------------------------------------------------------------------------------------------------------
def level_densities(Nz):
    return sar.reference_column(Nz, sar.COLUMN)[1]


def _host_limit(F, rho):
    """largest T* (K, at most 310) a level of density rho hosts: q^v+(T*, rho) over the equilibrated surface <= mpr.Q_HOST"""
    f = np.float64

    def over(T):
        return not (F.saturated_vapor_density(f(T), f(rho)) <= mpr.Q_HOST)
    if not over(310.0):
        return 310.0
    lo, hi = 150.0, 310.0
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        lo, hi = (lo, mid) if over(mid) else (mid, hi)
    return lo


def _threshold(F, theta, rho):
    f = np.float64
    q = f(1e-4)
    for _ in range(60):
        q = F.saturated_vapor_density(F.temperature_mixed(theta, q, f(0), f(0), rho, f(sar.PST), f(sar.NEWTON[0]), sar.NEWTON[1]), rho)
    return q


@functools.lru_cache(maxsize=None)
def mixed_density_parcels(shape, polynomial=False, seed=92, bulk_only=False):
    """(theta, rho, q^t, tag, sub, target) of the parcels of a grid, parcel n on level sar._level_of_parcel(shape)[n].
    bulk_only: the state a whole step starts from — no threshold, negative-moisture or theta = 0 parcels"""
    F, f = typed(np.float64, polynomial), np.float64
    Nx, Ny, Nz = shape
    n = Nx * Ny * Nz
    rho_level = level_densities(Nz)
    level = sar._level_of_parcel(shape)
    rng = np.random.default_rng(seed)
    limit = [_host_limit(F, DENSITY_SPREAD[0] * r) for r in rho_level]
    pst = f(sar.PST)
    tag, sub, target = np.empty(n, dtype="U20"), np.zeros(n), np.zeros(n)
    theta, rho, qt = np.empty(n), np.empty(n), np.empty(n)
    weights = dict(clear=0.30, warm_cloudy=0.14, all_ice=0.14, mixed_range=0.16, kink_Th=0.07, kink_Tf=0.07, marginal_edge=0.07,
                   negative_or_zero_q=0.05)
    if bulk_only:
        weights = {k: w for k, w in weights.items() if k not in ("marginal_edge", "negative_or_zero_q")}
    with np.errstate(all="ignore"):
        for i in range(n):
            k = level[i]
            Tmax = limit[k]
            hosts = {"clear": True, "all_ice": True, "marginal_edge": True, "negative_or_zero_q": True, "kink_Th": Tmax >= TH + 1.0,
                     "mixed_range": Tmax >= TH + 1.0, "kink_Tf": Tmax >= TF + 1.0, "warm_cloudy": Tmax >= TF + 6.5}
            names = [m for m in weights if hosts[m]]
            w = np.array([weights[m] for m in names])
            name = names[int(rng.choice(len(names), p=w / w.sum()))]
            u, v, s, pick = rng.random(), rng.random(), rng.random(), int(rng.integers(0, 1 << 30))
            r = f(rho_level[k] * (DENSITY_SPREAD[0] + s * (DENSITY_SPREAD[1] - DENSITY_SPREAD[0])))
            if name == "warm_cloudy":
                T = TF + 5.5 + u * (Tmax - (TF + 5.5))
            elif name == "all_ice":
                T = 190.0 + u * (TH - 5.5 - 190.0)
            elif name == "mixed_range":
                hi = min(TF - 0.1, Tmax)
                T = TH + 0.1 + u * (hi - (TH + 0.1))
            elif name in ("kink_Th", "kink_Tf"):
                T = (TH if name == "kink_Th" else TF) + (1.0 if i % 2 else -1.0) * (1e-4 + u * (mpr.KINK - 2e-4))
                sub[i] = T - (TH if name == "kink_Th" else TF)
            else:
                T = 195.0 + u * (Tmax - 195.0)
            T, tag[i], target[i], rho[i] = f(T), name, T, r
            qs = F.saturated_vapor_density(T, r)
            if name in ("clear", "negative_or_zero_q", "marginal_edge"):
                th = F.theta_of_density(T, f(0), f(0), f(0), r, pst)          # of dry air at the target temperature
                if name == "clear":
                    q = f((0.05 + 0.9 * v) * float(qs))
                elif name == "negative_or_zero_q":
                    sub[i] = sar.NEGATIVE_Q[pick % len(sar.NEGATIVE_Q)]
                    q = f(sub[i])
                else:
                    sub[i] = mpr.EDGE_DELTAS[pick % len(mpr.EDGE_DELTAS)]
                    while True:      # lower the target until the parcel's threshold lies inside the hosted domain (sar.anelastic_case)
                        qstar = _threshold(F, th, r)
                        if np.isfinite(qstar) and qstar <= mpr.Q_HOST:
                            break
                        T = T - f(5.0)
                        th, target[i] = F.theta_of_density(T, f(0), f(0), f(0), r, pst), T
                    q = f(float(qstar) * (1.0 + sub[i]))
            else:
                lam = F.lam(T)
                qc = f(min(10.0 ** (-6.0 + v * (np.log10(5e-3) + 6.0)), sar.Q_CAP - float(qs)))
                q = qs + qc
                th = F.theta_of_density(T, qs, lam * qc, (f(1) - lam) * qc, r, pst)
            theta[i], qt[i] = th, q
    if not bulk_only:
        zero = rng.choice(n, 4, replace=False)
        tag[zero], theta[zero] = "theta_zero", 0.0
    return theta, rho, qt, tag, sub, target


@functools.lru_cache(maxsize=None)
def mixed_density_case(shape, which=0, polynomial=False, bulk_only=False):
    """rho_d, rho theta, rho q^t of a compressible model (sar.compressible_case), with tag, sub, target (T*) and parcel (the placement)"""
    theta, rho, qt, tag, sub, target = mixed_density_parcels(shape, polynomial, bulk_only=bulk_only)
    rq = rho * qt
    rho_d = rho - rq
    rtheta = np.where(tag == "theta_zero", 0.0, rho_d * theta)
    P = sar.placement(shape, which)
    return sar.Case(rho_d=rho_d[P], rtheta=rtheta[P], rq=rq[P], tag=tag[P], sub=sub[P], target=target[P], parcel=P)


# ---- the restatement over a case ------------------------------------------------------------------------------------------------------------
def diagnose_mixed_density(arrays, dtype=np.float64, solver=sar.DEFAULT_SOLVER, newton=sar.NEWTON, force_branch=None, polynomial=False,
                           pst=sar.PST, Tf=TF, Th=TH, leave_out_ci=False):
    """k_cmp_diagnose<true, false, 4 | 5> cell by cell from rho_d, rho theta, rho q -> theta, q, rho, T, p, q^v, q^l, q^i (+ trace).
    last_residual: |T - T*|, the distance of the returned temperature from the iterate T* at which the condensate was split (0 for clear
    parcels): the slot mpr.exact_partition_masks reads, so that its masks select the parcels whose T* is EXACT_MARGIN beyond a kink"""
    F, t = typed(dtype, polynomial, Tf, Th), dtype
    shape = arrays["rho_d"].shape
    out = sar._empty(shape, dtype, ("theta", "q", "rho", "T", "p", "qv", "ql", "qi"))
    out["last_residual"] = np.zeros(shape)
    pst, abstol, nab = t(pst), t(solver[0]), t(newton[0])
    with np.errstate(all="ignore"):
        for idx in np.ndindex(shape):
            rd, rth, rq = t(arrays["rho_d"][idx]), t(arrays["rtheta"][idx]), t(arrays["rq"][idx])
            r = rd + (rq + t(0))
            th, q = rth / rd, rq / r
            T, qv, ql, qi, tr = F.adjust_density_mixed(th, q, r, pst, abstol, solver[1], nab, newton[1], force_branch, leave_out_ci)
            sar._record(out, idx, tr, float(solver[0]))
            if tr.final_iterate is not None:
                out.last_residual[idx] = abs(float(T) - float(tr.final_iterate))
            Rm = F._mix3(qv, ql, qi)[0]
            out.theta[idx], out.q[idx], out.rho[idx], out.T[idx], out.p[idx] = th, q, r, T, r * Rm * T
            out.qv[idx], out.ql[idx], out.qi[idx] = qv, ql, qi
    return out


@functools.lru_cache(maxsize=None)
def restated(shape, dtype, solver=sar.DEFAULT_SOLVER, force_branch=None, which=0, polynomial=False):
    return diagnose_mixed_density(mixed_density_case(shape, which, polynomial), dtype, solver, force_branch=force_branch, polynomial=polynomial)


@functools.lru_cache(maxsize=None)
def d80(shape, solver=sar.DEFAULT_SOLVER, polynomial=False):
    """the restatement's own rounding sensitivity, float64 against longdouble, per population: (dT rel, dq^v, dq^l, dq^i)"""
    return mpr.own_distance(restated(shape, np.float64, solver, polynomial=polynomial), restated(shape, np.longdouble, solver, polynomial=polynomial),
                            mixed_density_case(shape, 0, polynomial).tag)


def knife_edge(a, b, tag):
    """flr.knife_edge: parcels whose float64 (a) and longdouble (b) restatements differ in branch or iteration count, or pass within
    sar.KNIFE_EDGE of abstol; threshold parcels aside"""
    return flr.knife_edge(a, b, tag)


def float32_knife_edge(want32, want64, abstol):
    """flr.float32_knife_edge with the condensate q^l + q^i in the place of q^l (the rule is about the condensate abstol resolves; the slope
    dq^v+/dT = q^v+ L / (R^v T^2) is taken with the liquid latent heat, the smaller of the two, as there)"""
    both = sar.Result(want64)
    both["ql"] = want64["ql"] + want64["qi"]
    return flr.float32_knife_edge(want32, both, abstol)


# ---- the set-up of the whole-step tests ---------------------------------------------------------------------------------------------------------
# A 10 km column under theta = 300 K crosses T^f near 2.7 km and T^h near 6.8 km.  The total moisture is a multiple of the column's own
# q^v+(T_ref(z), rho_ref(z)) over the equilibrated surface: 0.6 of it at the x edges of the domain, 1.3 of it in the middle (plus the bubble),
# so every level holds clear and cloudy cells, and the cloudy ones are liquid below T^f, liquid + ice between the kinks and ice above T^h.
STEP_SHAPES = ((16, 12, 12), (66, 6, 12))
STEP_EXTENT = {(16, 12, 12): dict(x=(0.0, 4e3), y=(0.0, 3e3), z=(0.0, 10e3)), (66, 6, 12): dict(x=(0.0, 6.6e3), y=(0.0, 3e3), z=(0.0, 10e3))}
STEP_DT, STEP_COUNT, STEP_SUBSTEPS, STEP_WIND = 1.0, 3, 6, 2.0
MIN_REGIME_SHARE = 0.05
REGIMES = ("clear", "liquid only", "liquid + ice", "ice only")


def regime_shares(ql, qi):
    """the share of the cells in each of REGIMES"""
    return (float(((ql == 0) & (qi == 0)).mean()), float(((ql > 0) & (qi == 0)).mean()), float(((ql > 0) & (qi > 0)).mean()),
            float(((qi > 0) & (ql == 0)).mean()))


def step_state(om, polynomial=False):
    """(rho column, theta, q^t) of the moist bubble on the grid of the oracle model `om` (arrays shaped (Nz, 1, 1) and (Nz, Ny, Nx))"""
    F, f, g = typed(np.float64, polynomial), np.float64, om.grid
    x, y, z = g.nodes("ccc")
    Lx, Ly = g.Nx * g.dx, g.Ny * g.dy
    rho = om.ref.density[g.Hz:g.Hz + g.Nz]
    Tr = om.ref.pressure[g.Hz:g.Hz + g.Nz] / (rho * om.constants.Rd)
    qs = np.array([float(F.saturated_vapor_density(f(T), f(r))) for T, r in zip(Tr, rho)])[:, None, None]
    bub = np.maximum(0.0, 1.0 - np.sqrt(((x - Lx / 2) / (Lx / 4)) ** 2 + ((y - Ly / 2) / (Ly / 2)) ** 2 + ((z - 4500.0) / 3000.0) ** 2))
    shape = (g.Nz, g.Ny, g.Nx)
    window = 0.5 * (1.0 - np.cos(2 * np.pi * x / Lx))
    qt = np.broadcast_to(np.minimum(0.03, qs * (0.6 + 0.7 * window + 0.2 * bub)), shape).copy()
    theta = np.broadcast_to(300.0 + 0.5 * bub + 0 * z, shape).copy()
    return rho[:, None, None], theta, qt


_STEP_RUNS = {}


def step_wind(om, sheared=False):
    """the uniform wind of the whole-step tests; sheared (the SmagorinskyLilly step): with a shear, so that the eddy viscosity is not zero"""
    if not sheared:
        return STEP_WIND
    g = om.grid
    x, y, z = g.nodes("fcc")
    return np.broadcast_to(STEP_WIND * (1.0 + 0.5 * np.sin(2 * np.pi * x / (g.Nx * g.dx)) * np.cos(np.pi * z / 10e3)) + 0 * y, (g.Nz, g.Ny, g.Nx)).copy()


def oracle_model(oracle, oc, size, smagorinsky=False, **kw):
    og = oracle.Grid(size, **STEP_EXTENT[size])
    cls = MixedCompressibleOracle
    if smagorinsky:
        from compressible_closure_reference import ClosureCompressibleModel
        from oracle.closure import SmagorinskyLilly
        cls = type("MixedClosureOracle", (MixedCompressibleOracle, ClosureCompressibleModel), {})
        kw["closure"] = SmagorinskyLilly()
    return cls(og, time_discretization=oc.SplitExplicit(substeps=STEP_SUBSTEPS), surface_pressure=1e5, reference_potential_temperature=300.0, **kw)


def oracle_fields(om):
    g = om.grid
    out = {n: g.interior(getattr(om, n), n == "rw").copy() for n in ("rho_d", "rho", "rtheta", "rq", "ru", "rv", "rw", "T", "p", "qv", "ql", "qi")}
    return out


def oracle_steps(oracle, oc, size, polynomial=False, leave_out_ci=None, steps=STEP_COUNT, smagorinsky=False):
    """(fields after set!, fields after `steps` steps) of MixedCompressibleOracle from step_state, once per set-up; smagorinsky: with
    closure = SmagorinskyLilly() (compressible_closure_reference.ClosureCompressibleModel) in the sheared wind; the largest eddy viscosity
    of the last update_state! is returned with the fields as "nu_e_max" """
    key = (size, polynomial, leave_out_ci, steps, smagorinsky)
    if key not in _STEP_RUNS:
        om = oracle_model(oracle, oc, size, smagorinsky, polynomial=polynomial, leave_out_ci=leave_out_ci)
        rho, theta, qt = step_state(om, polynomial)
        om.set(rho=rho, theta=theta, u=step_wind(om, smagorinsky), v=0.0, w=0.0, qv=qt)
        start = oracle_fields(om)
        for _ in range(steps):
            om.time_step(STEP_DT)
        end = oracle_fields(om)
        if smagorinsky:
            end["nu_e_max"] = float(np.max(om.nu_e))
        _STEP_RUNS[key] = (start, end)
    return _STEP_RUNS[key]


def scaled_errors(got, want, names):
    """max-abs error relative to the field's max-abs; the momentum components share the vector's scale (tests/test_gpu_compressible.py:
    cmp_interior)"""
    mom = max(np.abs(want[n]).max() for n in ("ru", "rv", "rw"))
    return {n: float(np.abs(got[n] - want[n]).max() / max(mom if n in ("ru", "rv", "rw") else np.abs(want[n]).max(), 1e-300)) for n in names}


# ---- the oracle model -------------------------------------------------------------------------------------------------------------------------
class MixedCompressibleOracle(CompressibleOracleModel):
    """CompressibleOracleModel(microphysics = "SaturationAdjustment") with the mixed-phase equilibrium inside the density-based adjustment;
    `self.ql` is q^l, `self.qi` q^i.  polynomial = True: over flr's polynomial surface.  leave_out_ci: "linearization" | "inversion" plants
    an error (c_i q^i left out of c_pm there) for tests/test_mixed_phase_density_reference.py"""

    def __init__(self, grid, freezing_temperature=TF, homogeneous_ice_nucleation_temperature=TH, polynomial=False, leave_out_ci=None, **kw):
        kw.setdefault("microphysics", "SaturationAdjustment")
        assert kw["microphysics"] == "SaturationAdjustment" and leave_out_ci in (None, "linearization", "inversion")
        self._F = typed(np.float64, polynomial, float(freezing_temperature), float(homogeneous_ice_nucleation_temperature))
        self._leave_out_ci = leave_out_ci
        self.qi = grid.center_field()
        super().__init__(grid, **kw)

    def _sa_thermo(self):
        F, f = self._F, np.float64
        I = self.grid.interior
        rd, r = I(self.rho_d), I(self.rho)
        th, qt = I(self.rtheta) / rd, I(self.rq) / r
        I(self.theta)[...], I(self.q)[...] = th, qt
        T, qv, ql, qi, p = I(self.T), I(self.qv), I(self.ql), I(self.qi), I(self.p)
        args = (f(self.pst), f(self.sa_solver[0]), self.sa_solver[1], f(self.newton[0]), self.newton[1], None, self._leave_out_ci == "inversion")
        with np.errstate(all="ignore"):
            for idx in np.ndindex(th.shape):
                T[idx], qv[idx], ql[idx], qi[idx] = F.adjust_density_mixed(f(th[idx]), f(qt[idx]), f(r[idx]), *args)[:4]
                p[idx] = r[idx] * F._mix3(f(qv[idx]), f(ql[idx]), f(qi[idx]))[0] * T[idx]
        self._halo_center(self.qi)

    def refresh_linearization(self):
        super().refresh_linearization()
        c, F, I = self.constants, self._F, self.grid.interior
        qv, ql, qi = I(self.qv), I(self.ql), I(self.qi)
        qd = 1 - qv - ql - qi
        Rm = qd * c.Rd + qv * c.Rv
        cpm = qd * c.cpd + qv * c.cpv + ql * float(F.cl) + qi * (0.0 if self._leave_out_ci == "linearization" else float(F.ci))
        I(self.gR)[...] = cpm * Rm / (cpm - Rm)
        self._halo_sub(self.gR)
