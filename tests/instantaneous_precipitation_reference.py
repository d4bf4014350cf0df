"""Float64 restatement of microphysics = InstantaneousPrecipitation(equilibrium = WarmPhaseEquilibrium(), solver) on the compressible
split-explicit model: the Reed-Jablonowski large-scale condensation with immediate rain-out.  TEST INFRASTRUCTURE ONLY.

Followed line by line (paths relative to the reference):
  InstantaneousPrecipitation wraps a SaturationAdjustment; prognostic rho q^v, no condensate fields; microphysical fields q^v and a centre
  field precipitation_rate (kg m^-3 s^-1)                                    src/Microphysics/instantaneous_precipitation.jl:39-70
  inside a stage nothing condenses (the state is returned unchanged, the moisture fractions are vapour only): a stage is the stage of
  microphysics = nothing                                                      :73-86
  microphysics_model_update!: once per step, after the update_state! that follows stage 3; skipped for dt NaN, infinite or <= 0; ends in
  update_state!(model)                                                        :115-141, src/TimeSteppers/acoustic_runge_kutta_3.jl:307-316
  the kernel                                                                  :143-185
  adjust_thermodynamic_state(::LiquidIceDensityState, ::SaturationAdjustment) src/Microphysics/saturation_adjustment.jl:236-301
                                                                              (oracle/thermo.py: adjust_warm_phase_density)
  with_temperature(::LiquidIceDensityState, T)                                src/Thermodynamics/dynamic_states.jl:251-264
  precipitation_rate(model, :liquid | :ice), surface_precipitation_flux       :88-102

PARITY STATUS: pinned by tests/test_instantaneous_precipitation_reference.py, which restates the reference's own parity test
(test/instantaneous_precipitation.jl:38-127: the pre-refactor inline formulas) and its integration scenario (:131-217).

`ip_update` is the scalar update in Float64 on oracle/thermo.py.  `in_dtype(dtype)` gives the same formulas written on numpy scalars of
`dtype` (every constant and every intermediate in that type): in numpy.float64 it reproduces `ip_update` (pinned by the CPU test), in
numpy.float32 it is the yardstick of the Float32 library."""
import math

import numpy as np

from oracle import thermo
from oracle.oracle_compressible import CompressibleOracleModel


def ip_update(theta0, qt, rho, pst, c=None, abstol=1e-4, maxiter=20, newton_abstol=1e-4, newton_maxiter=8):
    """One cell of _instantaneous_precipitation_update! -> dict(T, qv, qc, theta_f): temperature and vapour fraction of the adjusted state,
    the condensate that leaves, and the potential temperature of the vapour-only parcel that keeps T."""
    c = c or thermo.ThermoConstants()
    T, qv, ql = thermo.adjust_warm_phase_density(theta0, qt, rho, pst, c, abstol, maxiter, newton_abstol, newton_maxiter)
    Rm = thermo.mixture_gas_constant(qv, 0.0, 0.0, c)
    cpm = thermo.mixture_heat_capacity(qv, 0.0, 0.0, c)
    p = rho * Rm * T
    theta_f = (T - 0.0) * (pst / p) ** (Rm / cpm)
    return dict(T=T, qv=qv, qc=ql, theta_f=theta_f)


class TypedFormulas:
    """The formulas of `ip_update` (and of oracle/thermo.py beneath it) on numpy scalars of one type."""

    def __init__(self, dtype, c=None):
        self.dtype = t = dtype
        c = c or thermo.ThermoConstants()
        self.Rd, self.Rv, self.cpd, self.cpv = t(c.Rd), t(c.Rv), t(c.cpd), t(c.cpv)
        self.Ll, self.cl, self.Ttr, self.ptr = t(c.Ll), t(c.cl), t(c.Ttr), t(c.ptr)
        self.dc = t(c.cpv) - t(c.cl)
        self.L0 = self.Ll - self.dc * t(c.T_energy)

    def _mix(self, qv, ql):
        qd = self.dtype(1) - (qv + ql)
        return qd * self.Rd + qv * self.Rv, qd * self.cpd + qv * self.cpv + ql * self.cl

    def psat(self, T):
        t = self.dtype
        return self.ptr * (T / self.Ttr) ** (self.dc / self.Rv) * np.exp((t(1) / self.Ttr - t(1) / T) * self.L0 / self.Rv)

    def temperature(self, theta, qv, ql, rho, pst, abstol, maxiter):
        t = self.dtype
        Rm, cpm = self._mix(qv, ql)
        kap, gam = Rm / cpm, cpm / (cpm - Rm)
        L = (self.Ll * ql) / cpm
        T = theta ** gam * (rho * Rm / pst) ** (gam - t(1)) + L
        dT, it = T, 0
        while abs(dT) > abstol and it < maxiter:
            Phi = (rho * Rm * T / pst) ** kap * theta
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
        return (T - L) * (pst / p) ** (Rm / cpm) - theta0, qv, ql

    def adjust(self, theta, qt, rho, pst, abstol, maxiter, newton_abstol, newton_maxiter):
        t = self.dtype
        T1 = self.temperature(theta, qt, t(0), rho, pst, newton_abstol, newton_maxiter)
        if qt <= self.psat(T1) / (rho * self.Rv * T1):
            return T1, qt, t(0)
        _, qv1, ql1 = self.residual(T1, theta, rho, qt, pst)
        dT = (self.Ll * ql1) / self._mix(qv1, ql1)[1]
        x1, x2 = T1, T1 + max(t(0.01), dT / t(2))
        r1, r2, it = self.residual(x1, theta, rho, qt, pst)[0], self.residual(x2, theta, rho, qt, pst)[0], 0
        while abs(r2) > abstol and it < maxiter:
            denom = r2 - r1
            s = (x2 - x1) / denom if denom != 0 else t(np.inf)
            valid = bool(np.isfinite(s))
            s = s if valid else t(0)
            x1, r1 = x2, r2
            x2 = x2 - r2 * s
            r2 = self.residual(x2, theta, rho, qt, pst)[0] if valid else t(0)
            it += 1
        _, qv, ql = self.residual(x2, theta, rho, qt, pst)
        return self.temperature(theta, qv, ql, rho, pst, newton_abstol, newton_maxiter), qv, ql

    def ip_update(self, theta0, qt, rho, pst, abstol=1e-4, maxiter=20, newton_abstol=1e-4, newton_maxiter=8):
        t = self.dtype
        theta0, qt, rho, pst = t(theta0), t(qt), t(rho), t(pst)
        with np.errstate(all="ignore"):
            T, qv, ql = self.adjust(theta0, qt, rho, pst, t(abstol), maxiter, t(newton_abstol), newton_maxiter)
            Rm, cpm = self._mix(qv, t(0))
            theta_f = T * (pst / (rho * Rm * T)) ** (Rm / cpm)
        return dict(T=T, qv=qv, qc=ql, theta_f=theta_f)


def in_dtype(dtype, c=None):
    return TypedFormulas(dtype, c)


class InstantaneousPrecipitationModel(CompressibleOracleModel):
    """CompressibleOracleModel(microphysics = None) — every stage is the vapour-only stage — with the once-per-step update behind it.
    solver = (abstol, maxiter) of the wrapped SaturationAdjustment's SecantSolver."""

    def __init__(self, grid, solver=(1e-4, 20), **kw):
        assert kw.pop("microphysics", None) is None
        super().__init__(grid, microphysics=None, **kw)
        self.thermo = thermo.ThermoConstants()
        self.sa_solver = (float(solver[0]), int(solver[1]))
        self.precipitation_rate = grid.center_field()
        self.last_dt = math.inf                      # clock.last_dt before the first step
        self.condensed = np.zeros((grid.Nz, grid.Ny, grid.Nx), dtype=bool)      # cells the LAST executed update condensed in

    def microphysics_model_update(self, dt=None):
        dt = self.last_dt if dt is None else float(dt)
        if math.isnan(dt) or math.isinf(dt) or dt <= 0:
            return
        g, tc = self.grid, self.thermo
        I = g.interior
        r, rd, rq, rth, P = I(self.rho), I(self.rho_d), I(self.rq), I(self.rtheta), I(self.precipitation_rate)
        self.condensed[...] = False
        for idx in np.ndindex(r.shape):
            rho, rho_d = float(r[idx]), float(rd[idx])
            qt = float(rq[idx]) / rho
            th0 = float(rth[idx]) / rho_d
            u = ip_update(th0, qt, rho, self.pst, tc, self.sa_solver[0], self.sa_solver[1], self.newton[0], self.newton[1])
            c = rho * max(0, qt - u["qv"])
            rq[idx] = rho * u["qv"]
            rth[idx] = rho_d * u["theta_f"]
            I(self.q)[idx] = u["qv"]
            if c > 0:
                P[idx] = c / dt
                self.condensed[idx] = True
        self.update_state(compute_tendencies=True)

    def time_step(self, dt):
        super().time_step(dt)
        self.last_dt = float(dt)
        self.microphysics_model_update(self.last_dt)

    def surface_precipitation_flux(self):
        """Field(Integral(precipitation_rate, dims = 3)): (Ny, Nx), summed upward from k = 0"""
        g = self.grid
        P = g.interior(self.precipitation_rate)
        dz = g.dzc[g.Hz:g.Hz + g.Nz]
        out = np.zeros((g.Ny, g.Nx))
        for k in range(g.Nz):
            out += P[k] * dz[k]
        return out


# ---- the mixed bubble of tests/test_gpu_compressible.py::test_compressible_saturation_adjustment_matches_oracle, scaled to a grid ----------
def theta_ref(z):
    return 300.0 * np.exp(9.80616 * z / (1005 * 300.0))


def bubble_state(Lx, Ly, Lz):
    """(theta, q^t) as functions of (x, y, z) on a domain [0, Lx] x [0, Ly] x [0, Lz]: the bubble of that test (centre (Lx / 2, Ly / 2, 0.4 Lz),
    radius 900 m on a 4 km x 3 km x 3 km domain) with its radius in the same proportion of each extent"""
    def bub(x, y, z):
        return np.maximum(0.0, 1.0 - np.sqrt(((x - 0.5 * Lx) / (0.225 * Lx)) ** 2 + ((y - 0.5 * Ly) / (0.3 * Ly)) ** 2 + ((z - 0.4 * Lz) / (0.3 * Lz)) ** 2))

    def theta(x, y, z):
        return 300.0 + 0.5 * bub(x, y, z) + 0 * z

    def qt(x, y, z):
        return 0.012 + 0.014 * bub(x, y, z) + 0.004 * (z / Lz)

    return theta, qt


def z_faces(Nz, Lz, stretched):
    if not stretched:
        return (0.0, float(Lz))
    s = np.linspace(0.0, 1.0, Nz + 1)
    return np.round(Lz * (0.5 * s + 0.5 * s ** 2))      # whole-number faces


def extents(shape, stretched=False):
    """The reference's 1 km cube for its own (8, 8, 8) grid; 100 m cells in x and y under a 3 km column (cold, saturated upper levels and a warm,
    clear surface layer around the bubble) for every other shape"""
    Nx, Ny, Nz = shape
    if shape == (8, 8, 8):
        return dict(x=(0.0, 1e3), y=(0.0, 1e3), z=z_faces(Nz, 1e3, stretched)), (1e3, 1e3, 1e3)
    return dict(x=(0.0, 100.0 * Nx), y=(0.0, 100.0 * Ny), z=z_faces(Nz, 3e3, stretched)), (100.0 * Nx, 100.0 * Ny, 3e3)


def make_restatement(oracle, oc, shape, halo, stretched=False, solver=(1e-4, 20), scheme=True, substeps=6):
    """The restatement (or, scheme = False, the plain CompressibleOracleModel with microphysics = None) on the test grids; surface pressure =
    standard pressure = 1e5 and theta_ref as in the reference's integration scenario"""
    ext, L = extents(shape, stretched)
    og = oracle.Grid(shape, halo=halo, **ext)
    kw = dict(time_discretization=oc.SplitExplicit(substeps=substeps), surface_pressure=1e5, standard_pressure=1e5,
              reference_potential_temperature=theta_ref)
    om = InstantaneousPrecipitationModel(og, solver=solver, **kw) if scheme else oc.CompressibleOracleModel(og, **kw)
    return om, ext, L
