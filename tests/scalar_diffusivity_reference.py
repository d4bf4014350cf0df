"""Float64 restatement of closure = ScalarDiffusivity(...) / VerticalScalarDiffusivity(...), explicit or vertically implicit, on the
anelastic model.  TEST INFRASTRUCTURE ONLY.  PARITY STATUS: **parity unpinned** (Oceananigans is not vendored).
  Breeze side, followed line by line:
    dynamic fluxes = rho_r at the flux location x kinematic flux, disc = time_discretization(closure) passed into every flux
                                                              src/TurbulenceClosures/TurbulenceClosures.jl:48-101
    implicit_step!(field, solver, closure, ..., alpha dt) after the RK update of every prognostic field
                                                              src/TimeSteppers/ssp_runge_kutta_3.jl:124-161
    order inside a stage                                      src/TimeSteppers/ssp_runge_kutta_3.jl:229-236
    z-Face rows                                               src/AtmosphereModels/implicit_vertical_advection.jl:202-214,270-292
  Oceananigans side — the reading (include/breeze_hip.h states it in full):
    isotropic: -2 nu Sigma_ij with nu averaged to ccc / ffc / fcf / cff, -kappa grad c with kappa averaged to the face;
    vertical: tau_uz = -nu_fcf dz u, tau_vz = -nu_cff dz v, tau_wz = -nu_ccc dz w, J_z = -kappa_ccf dz c, nothing else;
    vertically implicit: the explicit tendency keeps tau_uz = -nu_fcf dx w, tau_vz = -nu_cff dy w (isotropic only) and drops
    tau_wz, J_z; the solve is (I - dtau dz K dz) phi = phi* on the density-weighted field, no density in the operator.
It owns an OracleModel (grid, reference state, advection, pressure solve, thermodynamics) and reuses oracle.closure's strain and
padding code; tests/test_scalar_diffusivity_reference.py pins it (closed forms, numpy.linalg.solve, the reference's own numbers from
test/vertical_diffusion.jl and test/turbulence_closures.jl) before tests/test_scalar_diffusivity.py compares the device with it."""
import numpy as np

from oracle import oracle as orc
from oracle.closure import _columns, _pad_center, _pad_w, _pad_x, _pad_y, strain


class Diffusivity:
    """formulation 0 isotropic (ScalarDiffusivity), 1 vertical (VerticalScalarDiffusivity); nu, kappa: numbers or (Nz, Ny, Nx) arrays."""

    def __init__(self, formulation=0, implicit=False, nu=0.0, kappa=0.0):
        self.formulation, self.implicit, self.nu, self.kappa = int(formulation), bool(implicit), nu, kappa

    def on(self, which):
        K = getattr(self, which)
        return isinstance(K, np.ndarray) or K != 0.0

    def array(self, which, g):
        return np.broadcast_to(np.asarray(getattr(self, which), dtype=np.float64), (g.Nz, g.Ny, g.Nx))


# ---- rows and the Thomas solve (dtype-generic: the Float32 bound of the device test evaluates them in numpy float32) -------------------
def centre_rows(dzc, dzf, Kf, dtau):
    """Rows of a z-centre field.  dzc (Nz,), dzf (Nz+1,) spacings at faces 0..Nz, Kf (Nz+1, ...) K at the z faces of the column (the
    wall entries are not used).  Returns (lower, diag, upper), each (Nz, ...); lower[0] = upper[-1] = 0."""
    Nz = dzc.shape[0]
    sh = (Nz,) + (1,) * (Kf.ndim - 1)
    one = Kf.dtype.type(1)
    upper = -dtau * Kf[1:] / (dzc.reshape(sh) * dzf[1:].reshape(sh))
    lower = -dtau * Kf[:-1] / (dzc.reshape(sh) * dzf[:-1].reshape(sh))
    upper[-1] = 0
    lower[0] = 0
    return lower, (one - upper) - lower, upper


def face_rows(dzc, dzf, nu, dtau):
    """Rows of rho w at the interior faces 1..Nz-1 (0-based).  nu (Nz, ...) at centres.  The wall value w = 0 enters the first and the
    last row through the diagonal only: the returned lower[0] and upper[-1] are 0, diag keeps both terms."""
    Nz = dzc.shape[0]
    sh = (Nz - 1,) + (1,) * (nu.ndim - 1)
    one = nu.dtype.type(1)
    dzf_i = dzf[1:Nz].reshape(sh)
    upper = -dtau * nu[1:] / (dzf_i * dzc[1:].reshape(sh))
    lower = -dtau * nu[:-1] / (dzf_i * dzc[:-1].reshape(sh))
    diag = (one - upper) - lower
    upper, lower = upper.copy(), lower.copy()
    if Nz > 1:
        upper[-1] = 0
        lower[0] = 0
    return lower, diag, upper


def thomas(lower, diag, upper, d):
    """Unpivoted elimination along axis 0, in the order of operations of k_implicit_step."""
    nr = d.shape[0]
    x = np.empty_like(d)
    if nr == 0:
        return x
    cp = np.empty_like(d)
    cprev = np.zeros_like(d[0])
    dprev = np.zeros_like(d[0])
    for r in range(nr):
        m = d.dtype.type(1) / (diag[r] - lower[r] * cprev)
        cprev = upper[r] * m
        dprev = (d[r] - lower[r] * dprev) * m
        cp[r] = cprev
        x[r] = dprev
    for r in range(nr - 2, -1, -1):
        x[r] = x[r] - cp[r] * x[r + 1]
    return x


def dense_rows(lower, diag, upper):
    """The (nr, nr) matrix of one column's rows."""
    nr = diag.shape[0]
    A = np.diag(diag)
    for r in range(1, nr):
        A[r, r - 1] = lower[r]
        A[r - 1, r] = upper[r - 1]
    return A


# ---- K at the flux locations ----------------------------------------------------------------------------------------------------------
def _pad_K(g, K):
    """(Nz+2, Ny+2, Nx+2): periodic in x and y, zero gradient in z (as oracle/closure.py pads nu_e)."""
    Kp = _pad_x(g, _pad_y(g, K))
    return np.concatenate([Kp[:1], Kp, Kp[-1:]], axis=0)


def _locations(g, nup):
    Nz, Ny, Nx = g.Nz, g.Ny, g.Nx
    nu_ffc = ((nup[1:-1, 0:Ny + 1, 0:Nx + 1] + nup[1:-1, 0:Ny + 1, 1:Nx + 2]) / 2 +
              (nup[1:-1, 1:Ny + 2, 0:Nx + 1] + nup[1:-1, 1:Ny + 2, 1:Nx + 2]) / 2) / 2          # (Nz, Ny+1, Nx+1)
    nu_fcf = ((nup[0:Nz + 1, 1:-1, 0:Nx + 1] + nup[0:Nz + 1, 1:-1, 1:Nx + 2]) / 2 +
              (nup[1:Nz + 2, 1:-1, 0:Nx + 1] + nup[1:Nz + 2, 1:-1, 1:Nx + 2]) / 2) / 2          # (Nz+1, Ny, Nx+1)
    nu_cff = ((nup[0:Nz + 1, 0:Ny + 1, 1:-1] + nup[0:Nz + 1, 1:Ny + 2, 1:-1]) / 2 +
              (nup[1:Nz + 2, 0:Ny + 1, 1:-1] + nup[1:Nz + 2, 1:Ny + 2, 1:-1]) / 2) / 2          # (Nz+1, Ny+1, Nx)
    return nu_ffc, nu_fcf, nu_cff


def _scalars(m):
    """(prognostic density name, specific field) of every scalar of the model"""
    out = [("rtheta", m.theta), ("rq", m.q)]
    if m.microphysics == "Kessler":
        out += [("rqcl", m.qcl), ("rqr", m.qr)]
    return out + [(f"rc{t}", getattr(m, f"c{t}")) for t in range(m.n_tracers)]


def add_diffusivity_tendencies(m):
    """G -= div(rho_r x kinematic flux) for what the closure's time discretisation leaves explicit."""
    d, g = m.diffusivity, m.grid
    vert, impl = d.formulation == 1, d.implicit
    if vert and impl:
        return
    dzc, dzf, rho, rho_f, _ = _columns(m)
    Nz, Ny, Nx = g.Nz, g.Ny, g.Nx
    dx, dy = g.dx, g.dy
    r3, rf3, dz3 = rho[:, None, None], rho_f[:, None, None], dzc[:, None, None]
    Ax, Ay, Az = dy * dz3, dx * dz3, dx * dy
    Vc = dx * dy * dz3
    I = g.interior
    if d.on("nu"):
        nu = d.array("nu", g)
        nu_ffc, nu_fcf, nu_cff = _locations(g, _pad_K(g, nu))
        S11, S22, S33, S12, S13, S23 = strain(m)
        u, v, w = _pad_center(g, m.u, xface=True), _pad_center(g, m.v, yface=True), _pad_w(g, m.w)
        dzf3 = dzf[:, None, None]
        uz = (u[1:2 + Nz, 1:1 + Ny, 1:2 + Nx] - u[0:1 + Nz, 1:1 + Ny, 1:2 + Nx]) / dzf3        # (Nz+1, Ny, Nx+1); zero on the walls (no-flux pad)
        wx = (w[:, 1:1 + Ny, 1:2 + Nx] - w[:, 1:1 + Ny, 0:1 + Nx]) / dx                        # zero on the walls (w = 0)
        vz = (v[1:2 + Nz, 1:2 + Ny, 1:1 + Nx] - v[0:1 + Nz, 1:2 + Ny, 1:1 + Nx]) / dzf3
        wy = (w[:, 1:2 + Ny, 1:1 + Nx] - w[:, 0:1 + Ny, 1:1 + Nx]) / dy
        zero = 0.0
        if vert:
            T11 = T22 = np.zeros((Nz, Ny, Nx))
            T12 = np.zeros((Nz, Ny + 1, Nx + 1))
            Twx, Twy = np.zeros((Nz + 1, Ny, Nx + 1)), np.zeros((Nz + 1, Ny + 1, Nx))
            Tuz, Tvz, Twz = rf3 * (-nu_fcf * uz), rf3 * (-nu_cff * vz), r3 * (-nu * S33)
        else:
            T11, T22, T12 = r3 * (-2 * nu * S11), r3 * (-2 * nu * S22), r3 * (-2 * nu_ffc * S12)
            Twx, Twy = rf3 * (-2 * nu_fcf * S13), rf3 * (-2 * nu_cff * S23)
            if impl:
                Tuz, Tvz, Twz = rf3 * (-nu_fcf * wx), rf3 * (-nu_cff * wy), np.zeros((Nz, Ny, Nx)) + zero
            else:
                Tuz, Tvz, Twz = Twx, Twy, r3 * (-2 * nu * S33)
        T11m = np.roll(T11, 1, axis=2)
        div_u = (Ax * T11 - Ax * T11m) + (Ay * T12[:, 1:, :-1] - Ay * T12[:, :-1, :-1]) + (Az * Tuz[1:, :, :-1] - Az * Tuz[:-1, :, :-1])
        I(m.G["ru"])[...] -= div_u / Vc
        T22m = np.roll(T22, 1, axis=1)
        div_v = (Ax * T12[:, :-1, 1:] - Ax * T12[:, :-1, :-1]) + (Ay * T22 - Ay * T22m) + (Az * Tvz[1:, :-1, :] - Az * Tvz[:-1, :-1, :])
        I(m.G["rv"])[...] -= div_v / Vc
        if Nz > 1:
            dzfi = dzf[1:Nz, None, None]
            Axf, Ayf, Vf = dy * dzfi, dx * dzfi, dx * dy * dzfi
            div_w = (Axf * Twx[1:Nz, :, 1:] - Axf * Twx[1:Nz, :, :-1]) + (Ayf * Twy[1:Nz, 1:, :] - Ayf * Twy[1:Nz, :-1, :]) + \
                    (Az * Twz[1:] - Az * Twz[:-1])
            I(m.G["rw"], zface=True)[1:Nz] -= div_w / Vf
    if d.on("kappa"):
        kap = _pad_K(g, d.array("kappa", g))
        kx = (kap[1:-1, 1:-1, 0:Nx + 1] + kap[1:-1, 1:-1, 1:Nx + 2]) / 2
        ky = (kap[1:-1, 0:Ny + 1, 1:-1] + kap[1:-1, 1:Ny + 2, 1:-1]) / 2
        kz = (kap[0:Nz + 1, 1:-1, 1:-1] + kap[1:Nz + 2, 1:-1, 1:-1]) / 2
        for name, field in _scalars(m):
            c = _pad_center(g, field)
            div = 0.0
            if not impl:
                Jz = rf3 * (-kz * ((c[1:Nz + 2, 1:-1, 1:-1] - c[0:Nz + 1, 1:-1, 1:-1]) / dzf[:, None, None]))      # zero on the walls (no-flux pad)
                div = Az * Jz[1:] - Az * Jz[:-1]
            if not vert:
                Jx = r3 * (-kx * ((c[1:-1, 1:-1, 1:Nx + 2] - c[1:-1, 1:-1, 0:Nx + 1]) / dx))
                Jy = r3 * (-ky * ((c[1:-1, 1:Ny + 2, 1:-1] - c[1:-1, 0:Ny + 1, 1:-1]) / dy))
                div = (Ax * Jx[:, :, 1:] - Ax * Jx[:, :, :-1]) + (Ay * Jy[:, 1:, :] - Ay * Jy[:, :-1, :]) + div
            I(m.G[name])[...] -= div / Vc


def implicit_coefficients(m):
    """{class: K array the rows of that class take}: "u" nu_fcf (Nz+1, Ny, Nx), "v" nu_cff, "w" nu_ccc (Nz, Ny, Nx), "c" kappa_ccf."""
    d, g = m.diffusivity, m.grid
    Nz = g.Nz
    out = {}
    if d.on("nu"):
        nu = np.ascontiguousarray(d.array("nu", g))
        _, nu_fcf, nu_cff = _locations(g, _pad_K(g, nu))
        out["u"], out["v"], out["w"] = nu_fcf[:, :, :-1], nu_cff[:, :-1, :], nu
    if d.on("kappa"):
        kap = _pad_K(g, d.array("kappa", g))
        out["c"] = (kap[0:Nz + 1, 1:-1, 1:-1] + kap[1:Nz + 2, 1:-1, 1:-1]) / 2
    return out


def implicit_step(m, dtau, dtype=np.float64):
    """implicit_step! of every prognostic field (interior cells; the wall faces of rho w are not touched).  dtype = float32 evaluates
    rows and solve in Float32 (inputs rounded first) and returns {name: solution} WITHOUT writing the model: the device test's bound."""
    d, g = m.diffusivity, m.grid
    if not d.implicit:
        return {}
    Nz, Hz = g.Nz, g.Hz
    f64 = dtype == np.float64
    dzc, dzf = g.dzc[Hz:Hz + Nz].astype(dtype), g.dzf[Hz:Hz + Nz + 1].astype(dtype)
    K = {k: v.astype(dtype) for k, v in implicit_coefficients(m).items()}
    dtau = dtype(dtau)
    out = {}
    fields = []
    if "u" in K:
        fields += [("ru", "u"), ("rv", "v"), ("rw", "w")]
    if "c" in K:
        fields += [(name, "c") for name, _ in _scalars(m)]
    for name, cls in fields:
        if cls == "w":
            if Nz < 2:
                continue
            view = g.interior(getattr(m, name), zface=True)[1:Nz]
            rows = face_rows(dzc, dzf, K["w"], dtau)
        else:
            view = g.interior(getattr(m, name))
            rows = centre_rows(dzc, dzf, K[cls], dtau)
        x = thomas(*rows, view.astype(dtype))
        out[name] = x
        if f64:
            view[...] = x
    return out


class DiffusivityModel(orc.OracleModel):
    """OracleModel with closure = ScalarDiffusivity / VerticalScalarDiffusivity (`diffusivity`: a Diffusivity)."""

    def __init__(self, grid, diffusivity, **kw):
        self.diffusivity = diffusivity          # before the constructor's first update_state
        super().__init__(grid, **kw)

    def _compute_tendencies(self):
        super()._compute_tendencies()
        add_diffusivity_tendencies(self)

    def implicit_step(self, dtau):
        implicit_step(self, dtau)

    def time_step(self, dt):
        """time_step! with implicit_step!(alpha dt) between the RK update and the pressure correction of every stage"""
        if self.iteration == 0:
            self.update_state(compute_tendencies=True)
        for n in self.PROGNOSTIC:
            self.U0[n][...] = getattr(self, n)
        for alpha in (1.0, 1.0 / 4.0, 2.0 / 3.0):
            self.rk3_substep(dt, alpha)
            self.implicit_step(alpha * dt)
            self.compute_pressure_correction(alpha * dt)
            self.make_pressure_correction(alpha * dt)
            self.update_state(compute_tendencies=True)
        if self.microphysics == "Kessler":
            self.microphysics_model_update(dt)
        self.clock_time += dt
        self.iteration += 1
