"""Float64 restatement of the turbulence closures on the compressible split-explicit model: closure = SmagorinskyLilly(),
ScalarDiffusivity(nu, kappa) or VerticalScalarDiffusivity(nu, kappa) with the explicit time discretisation.  TEST INFRASTRUCTURE ONLY.
PARITY STATUS: **parity unpinned** on the Oceananigans side (the reading include/breeze_hip.h states, shared with oracle/closure.py and
tests/scalar_diffusivity_reference.py); the Breeze side is followed line by line:
  slow momentum tendencies take model.closure / closure_fields      src/TimeSteppers/acoustic_substep_helpers.jl:55-93
  dynamic stresses = density at the flux location x kinematic flux  src/TurbulenceClosures/TurbulenceClosures.jl:65-101
      density = dynamics_density = rho_d, the 3-D field: the cell value at ccc, the two-point means at the faces, the four-point means at
      ffc / fcf / cff (in the order the nu averages take), through the field's halos: periodic in x / y, zero gradient in z
  rho theta: - div J^c with rho_d at the faces, c = theta           src/PotentialTemperatureFormulations/potential_temperature_tendency.jl:100-105
  water scalars: - div J^c with the TOTAL density at the faces      src/AtmosphereModels/dynamics_kernel_functions.jl:132-159
  compute_closure_fields! closes compute_auxiliary_variables!       src/AtmosphereModels/update_atmosphere_model_state.jl:218
  N^2 = g dz log theta_v, theta_v from the 3-D pressure at each cell, q^v = specific_humidity(model)
                                                                    src/AtmosphereModels/atmosphere_model_buoyancy.jl:46-68
  order of the terms: advection, Coriolis, closure, forcing         src/AtmosphereModels/dynamics_kernel_functions.jl:77-81
tests/test_compressible_closure_reference.py pins it (the anelastic restatements with rho_d = rho_r(z) and p = p_r(z), closed forms,
conservation, the reference's own known answers) before tests/test_compressible_closure.py compares the device with it."""
import copy
import types

import numpy as np

from oracle.closure import _pad_center, _pad_x, _pad_y, strain
from oracle.oracle_compressible import CompressibleOracleModel
from scalar_diffusivity_reference import Diffusivity, _locations


def _columns(g):
    Hz, Nz = g.Hz, g.Nz
    return g.dzc[Hz:Hz + Nz], g.dzf[Hz:Hz + Nz + 1]      # centres 0..Nz-1; faces 0..Nz


def _strain(m):
    """oracle.closure.strain reads the grid and the velocities only; its column helper also touches m.ref"""
    g = m.grid
    col = np.zeros(g.Szc)
    return strain(types.SimpleNamespace(grid=g, ref=types.SimpleNamespace(density=col, pressure=col), u=m.u, v=m.v, w=m.w))


def _pad_interior(g, a):
    """(Nz, Ny, Nx) -> (Nz+2, Ny+2, Nx+2): periodic in x and y, zero gradient in z"""
    ap = _pad_x(g, _pad_y(g, a))
    return np.concatenate([ap[:1], ap, ap[-1:]], axis=0)


def specific_humidity(m):
    """specific_humidity(model): the prognostic moisture fraction without microphysics, the vapour fraction with saturation adjustment or
    Kessler (whose q slot is q^v)"""
    return m.qv if m.microphysics == "SaturationAdjustment" else m.q


def strain_rate_squared(m):
    S11, S22, S33, S12, S13, S23 = _strain(m)
    sq12, sq13, sq23 = S12 ** 2, S13 ** 2, S23 ** 2
    a12 = ((sq12[:, :-1, :-1] + sq12[:, :-1, 1:]) / 2 + (sq12[:, 1:, :-1] + sq12[:, 1:, 1:]) / 2) / 2
    a13 = ((sq13[:-1, :, :-1] + sq13[:-1, :, 1:]) / 2 + (sq13[1:, :, :-1] + sq13[1:, :, 1:]) / 2) / 2
    a23 = ((sq23[:-1, :-1, :] + sq23[:-1, 1:, :]) / 2 + (sq23[1:, :-1, :] + sq23[1:, 1:, :]) / 2) / 2
    return (S11 ** 2 + S22 ** 2 + S33 ** 2) + 2 * a12 + 2 * a13 + 2 * a23


def buoyancy_frequency(m):
    """N^2 at centres: the mean of g dz(log theta_v) on the two faces; T, p, q^v carry zero-gradient z halos, so the wall faces hold exact zeros"""
    g, c = m.grid, m.constants
    _, dzf = _columns(g)
    T = _pad_center(g, m.T)[:, 1:-1, 1:-1]
    p = _pad_center(g, m.p)[:, 1:-1, 1:-1]
    qv = _pad_center(g, specific_humidity(m))[:, 1:-1, 1:-1]
    Rm = (1.0 - (qv + 0.0 + 0.0)) * c.Rd + qv * c.Rv
    lg = np.log(Rm / c.Rd * T * (m.pst / p) ** (c.Rd / c.cpd))
    dzb = c.g * ((lg[1:] - lg[:-1]) / dzf[:, None, None])       # faces 0..Nz
    return (dzb[:-1] + dzb[1:]) / 2


def stability_argument(m):
    """(Sigma^2, C_b N^2+ / Sigma^2 where Sigma^2 > 0 else nan): the classes of the stability factor the device test asks for"""
    Sig2 = strain_rate_squared(m)
    N2p = np.maximum(0.0, buoyancy_frequency(m))
    with np.errstate(divide="ignore", invalid="ignore"):
        return Sig2, np.where(Sig2 == 0, np.nan, m.closure.Cb * N2p / Sig2)


def eddy_viscosity(m):
    """nu_e = varsigma (C Delta)^2 sqrt(2 Sigma^2) on the interior (Nz, Ny, Nx)"""
    g, cl = m.grid, m.closure
    dzc, _ = _columns(g)
    Sig2 = strain_rate_squared(m)
    N2p = np.maximum(0.0, buoyancy_frequency(m))
    with np.errstate(divide="ignore", invalid="ignore"):
        sig2 = 1.0 - np.minimum(1.0, cl.Cb * N2p / Sig2)
        stab = np.where(Sig2 == 0, 0.0, np.sqrt(sig2))
    delta = np.cbrt(g.dx * g.dy * dzc)[:, None, None]
    return (stab * cl.C ** 2) * delta ** 2 * np.sqrt(2 * Sig2)


def density_locations(g, rho):
    """rho: a centre field (parent array).  Returns the density at ccc (Nz, Ny, Nx), at the x / y / z faces (fcc (Nz, Ny, Nx+1),
    cfc (Nz, Ny+1, Nx), ccf (Nz+1, Ny, Nx)) and at ffc (Nz, Ny+1, Nx+1), fcf (Nz+1, Ny, Nx+1), cff (Nz+1, Ny+1, Nx)"""
    Nz, Ny, Nx = g.Nz, g.Ny, g.Nx
    rp = _pad_center(g, rho)
    fcc = (rp[1:-1, 1:-1, 0:Nx + 1] + rp[1:-1, 1:-1, 1:Nx + 2]) / 2
    cfc = (rp[1:-1, 0:Ny + 1, 1:-1] + rp[1:-1, 1:Ny + 2, 1:-1]) / 2
    ccf = (rp[0:Nz + 1, 1:-1, 1:-1] + rp[1:Nz + 2, 1:-1, 1:-1]) / 2
    ffc, fcf, cff = _locations(g, rp)
    return rp[1:-1, 1:-1, 1:-1], fcc, cfc, ccf, ffc, fcf, cff


def momentum_closure_terms(m, nu, vertical=False):
    """(d_j T_1j, d_j T_2j, d_j T_3j): what the slow G_rho_u, G_rho_v (Nz, Ny, Nx) and G_rho_w (interior faces 1..Nz-1) lose.  nu: (Nz, Ny, Nx).
    vertical: the VerticalScalarDiffusivity formulation (tau_uz = -nu_fcf dz u, tau_vz = -nu_cff dz v, tau_wz = -nu dz w, nothing else)."""
    g = m.grid
    dzc, dzf = _columns(g)
    Nz, Ny, Nx = g.Nz, g.Ny, g.Nx
    dx, dy = g.dx, g.dy
    dz3 = dzc[:, None, None]
    r, _, _, _, r_ffc, r_fcf, r_cff = density_locations(g, m.rho_d)
    nu_ffc, nu_fcf, nu_cff = _locations(g, _pad_interior(g, nu))
    S11, S22, S33, S12, S13, S23 = _strain(m)
    if vertical:
        u, v = _pad_center(g, m.u), _pad_center(g, m.v)
        dzf3 = dzf[:, None, None]
        uz = (u[1:2 + Nz, 1:1 + Ny, 1:2 + Nx] - u[0:1 + Nz, 1:1 + Ny, 1:2 + Nx]) / dzf3
        vz = (v[1:2 + Nz, 1:2 + Ny, 1:1 + Nx] - v[0:1 + Nz, 1:2 + Ny, 1:1 + Nx]) / dzf3
        T11 = T22 = np.zeros((Nz, Ny, Nx), dtype=nu.dtype)
        T12 = np.zeros((Nz, Ny + 1, Nx + 1), dtype=nu.dtype)
        Twx, Twy = np.zeros((Nz + 1, Ny, Nx + 1), dtype=nu.dtype), np.zeros((Nz + 1, Ny + 1, Nx), dtype=nu.dtype)
        Tuz, Tvz, Twz = r_fcf * (-nu_fcf * uz), r_cff * (-nu_cff * vz), r * (-nu * S33)
    else:
        T11, T22, T12 = r * (-2 * nu * S11), r * (-2 * nu * S22), r_ffc * (-2 * nu_ffc * S12)
        Twx, Twy = r_fcf * (-2 * nu_fcf * S13), r_cff * (-2 * nu_cff * S23)
        Tuz, Tvz, Twz = Twx, Twy, r * (-2 * nu * S33)
    Ax, Ay, Az = dy * dz3, dx * dz3, dx * dy
    Vc = dx * dy * dz3
    T11m = np.roll(T11, 1, axis=2)
    div_u = (Ax * T11 - Ax * T11m) + (Ay * T12[:, 1:, :-1] - Ay * T12[:, :-1, :-1]) + (Az * Tuz[1:, :, :-1] - Az * Tuz[:-1, :, :-1])
    T22m = np.roll(T22, 1, axis=1)
    div_v = (Ax * T12[:, :-1, 1:] - Ax * T12[:, :-1, :-1]) + (Ay * T22 - Ay * T22m) + (Az * Tvz[1:, :-1, :] - Az * Tvz[:-1, :-1, :])
    dzfi = dzf[1:Nz, None, None]
    Axf, Ayf, Vf = dy * dzfi, dx * dzfi, dx * dy * dzfi
    div_w = (Axf * Twx[1:Nz, :, 1:] - Axf * Twx[1:Nz, :, :-1]) + (Ayf * Twy[1:Nz, 1:, :] - Ayf * Twy[1:Nz, :-1, :]) + (Az * Twz[1:] - Az * Twz[:-1])
    return div_u / Vc, div_v / Vc, div_w / Vf


def scalar_closure_term(m, c, kappa, rho, vertical=False):
    """div J^c / V with J = density at the face x (-kappa_face grad c).  c, rho: centre fields (parent arrays); kappa: (Nz, Ny, Nx)."""
    g = m.grid
    dzc, dzf = _columns(g)
    Nz, Ny, Nx = g.Nz, g.Ny, g.Nx
    dx, dy = g.dx, g.dy
    dz3 = dzc[:, None, None]
    _, r_fcc, r_cfc, r_ccf, _, _, _ = density_locations(g, rho)
    kap = _pad_interior(g, kappa)
    cp = _pad_center(g, c)
    kz = (kap[0:Nz + 1, 1:-1, 1:-1] + kap[1:Nz + 2, 1:-1, 1:-1]) / 2
    Jz = r_ccf * (-kz * ((cp[1:Nz + 2, 1:-1, 1:-1] - cp[0:Nz + 1, 1:-1, 1:-1]) / dzf[:, None, None]))      # zero on the walls (no-flux pad)
    Ax, Ay, Az = dy * dz3, dx * dz3, dx * dy
    div = Az * Jz[1:] - Az * Jz[:-1]
    if not vertical:
        kx = (kap[1:-1, 1:-1, 0:Nx + 1] + kap[1:-1, 1:-1, 1:Nx + 2]) / 2
        ky = (kap[1:-1, 0:Ny + 1, 1:-1] + kap[1:-1, 1:Ny + 2, 1:-1]) / 2
        Jx = r_fcc * (-kx * ((cp[1:-1, 1:-1, 1:Nx + 2] - cp[1:-1, 1:-1, 0:Nx + 1]) / dx))
        Jy = r_cfc * (-ky * ((cp[1:-1, 1:Ny + 2, 1:-1] - cp[1:-1, 0:Ny + 1, 1:-1]) / dy))
        div = (Ax * Jx[:, :, 1:] - Ax * Jx[:, :, :-1]) + (Ay * Jy[:, 1:, :] - Ay * Jy[:, :-1, :]) + div
    return div / (dx * dy * dz3)


def in_dtype(m, dtype):
    """A view of the model whose fields, grid metrics and closure coefficients are rounded to `dtype`: eddy_viscosity, slow_closure_terms and
    water_closure_terms of the view evaluate every formula of this file in that type (numpy keeps the array type against Python numbers).
    The Float32 bound of the device test is the error of the view in numpy.float32 on the device's own inputs."""
    v = copy.copy(m)
    g = copy.copy(m.grid)
    g.dx, g.dy = dtype(m.grid.dx), dtype(m.grid.dy)
    g.dzc, g.dzf = m.grid.dzc.astype(dtype), m.grid.dzf.astype(dtype)
    v.grid = g
    for n in ("rho_d", "rho", "u", "v", "w", "theta", "q", "T", "p", "qv", "qcl", "qr"):
        if hasattr(m, n):
            setattr(v, n, getattr(m, n).astype(dtype))
    if m.nu_e is not None:
        v.nu_e = m.nu_e.astype(dtype)
    return v


class ClosureCompressibleModel(CompressibleOracleModel):
    """CompressibleOracleModel with closure = SmagorinskyLilly (`closure`: an oracle.closure.SmagorinskyLilly) or ScalarDiffusivity /
    VerticalScalarDiffusivity (`diffusivity`: a tests.scalar_diffusivity_reference.Diffusivity, explicit; nu / kappa numbers or
    (Nz, Ny, Nx) arrays, which the caller may rewrite between steps)."""

    def __init__(self, grid, closure=None, diffusivity=None, **kw):
        assert closure is None or diffusivity is None, "one closure"
        assert diffusivity is None or (isinstance(diffusivity, Diffusivity) and not diffusivity.implicit)
        self.closure, self.diffusivity = closure, diffusivity
        self.nu_e = None
        super().__init__(grid, **kw)

    # -- what the closure hands the flux formulas ----------------------------------------------------------------------------------
    def _nu(self):
        if self.closure is not None:
            return self.nu_e, False
        d = self.diffusivity
        return (np.ascontiguousarray(d.array("nu", self.grid)).astype(self.theta.dtype) if d.on("nu") else None), d.formulation == 1

    def _kappa(self):
        if self.closure is not None:
            return self.nu_e / self.closure.Pr, False
        d = self.diffusivity
        return (np.ascontiguousarray(d.array("kappa", self.grid)).astype(self.theta.dtype) if d.on("kappa") else None), d.formulation == 1

    def slow_closure_terms(self):
        """{"ru", "rv", "rw" (faces 1..Nz-1), "rtheta"}: what the closure subtracts from the slow tendencies (absent: nothing)"""
        out = {}
        if self.closure is None and self.diffusivity is None:
            return out
        nu, vert = self._nu()
        if nu is not None:
            out["ru"], out["rv"], out["rw"] = momentum_closure_terms(self, nu, vert)
        kappa, vert = self._kappa()
        if kappa is not None:
            out["rtheta"] = scalar_closure_term(self, self.theta, kappa, self.rho_d, vert)
        return out

    def water_closure_terms(self):
        """{"rq" [, "rqcl", "rqr"]}: what the closure subtracts from the water tendencies, the total density at the faces"""
        out = {}
        if self.closure is None and self.diffusivity is None:
            return out
        kappa, vert = self._kappa()
        if kappa is None:
            return out
        scalars = [("rq", self.q)] + ([("rqcl", self.qcl), ("rqr", self.qr)] if self.microphysics == "Kessler" else [])
        for name, c in scalars:
            out[name] = scalar_closure_term(self, c, kappa, self.rho, vert)
        return out

    # -- the two overrides ---------------------------------------------------------------------------------------------------------
    def compute_closure_fields(self):
        if self.closure is not None:
            self.nu_e = eddy_viscosity(self)

    def update_state(self, compute_tendencies=True):
        # (the advective water tendencies do not read the closure fields: forming them before compute_closure_fields! changes nothing)
        super().update_state(compute_tendencies)
        self.compute_closure_fields()
        if compute_tendencies:
            I = self.grid.interior
            for name, term in self.water_closure_terms().items():
                I(self.G[name])[...] -= term

    def compute_slow_tendencies(self):
        g, G, I = self.grid, self.G, self.grid.interior
        f, relax, ff = self.coriolis_f, self.relaxation, getattr(self, "field_forcing", None)
        self.coriolis_f, self.relaxation, self.field_forcing = 0.0, None, None
        try:
            super().compute_slow_tendencies()      # advection
        finally:
            self.coriolis_f, self.relaxation, self.field_forcing = f, relax, ff
        if f != 0.0:
            from oracle.forcings import _xy_to_cf, _xy_to_fc
            I(G["ru"])[...] -= -f * _xy_to_fc(self, self.rv)
            I(G["rv"])[...] -= f * _xy_to_cf(self, self.ru)
        terms = self.slow_closure_terms()
        for name in ("ru", "rv", "rtheta"):
            if name in terms:
                I(G[name])[...] -= terms[name]
        if "rw" in terms:
            I(G["rw"], True)[1:g.Nz] -= terms["rw"]
        if relax:
            from oracle.forcings import add_relaxation_tendencies
            add_relaxation_tendencies(self)
        if ff is not None:
            from oracle.forcings import add_field_forcing
            add_field_forcing(self)
