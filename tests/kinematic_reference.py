"""Float64 restatement of the reference's kinematic driver, AtmosphereModel(grid; dynamics = PrescribedDynamics(reference_state)):
    src/KinematicDriver/prescribed_dynamics.jl:27-84                 density and pressure are the reference state's
    src/KinematicDriver/kinematic_driver_time_stepping.jl:16-49      compute_velocities!, the pressure correction: no-ops
    src/KinematicDriver/kinematic_driver_time_stepping.jl:55-73      div_rhoU and the correction c div_rhoU
    src/AtmosphereModels/dynamics_kernel_functions.jl:155-156        G = -div_rhoUc + c div_rhoU
    src/TimeSteppers/ssp_runge_kutta_3.jl:209-278                    time_step!
It owns an OracleModel for the grid, the reference state, the halo fills and the thermodynamics, and advances the scalars itself through
the oracle library's C functions: og_scalar_tendency with the prescribed u, v, w per scalar, og_rk3_substep, og_compute_thermo(_sa) —
update_state! minus og_compute_velocities — and a numpy div_rhoU.  It never calls the pressure solve.  tests/test_kinematic_reference.py
pins it (the reference's own Gaussian advection test among others) before tests/test_kinematic.py compares the device with it."""
import ctypes as C

import numpy as np


def velocity_field(Lx, Ly, Lz):
    """The smooth, sign-changing, divergent field of the kinematic tests: each direction meets both upwind biases."""
    u = lambda x, y, z: 3.0 + 4.0 * np.sin(2 * np.pi * x / Lx) * np.cos(2 * np.pi * y / Ly) + 0 * z
    v = lambda x, y, z: -2.0 + 3.0 * np.cos(2 * np.pi * x / Lx) * np.sin(2 * np.pi * y / Ly) + 0 * z
    w = lambda x, y, z: 2.0 * np.sin(np.pi * z / Lz) * (1.0 + 0.5 * np.cos(2 * np.pi * x / Lx)) + 0 * y
    return u, v, w


class KinematicReference:
    """Scalars: "rtheta", "rq", "rc0", "rc1", ... (densities, parent arrays of the oracle model `self.m`); their specific fields are
    "theta", "q", "c0", ..."""

    def __init__(self, orc, size, x, y, z, topology=("Periodic", "Periodic", "Bounded"), halo=3, potential_temperature=300.0,
                 microphysics=None, tracers=0, divergence_correction=False):
        self.orc = orc
        self.grid = g = orc.Grid(size, x=x, y=y, z=z, topology=topology, halo=halo)
        # initialize=False: OracleModel.set would project the momentum
        self.m = orc.OracleModel(g, potential_temperature=potential_temperature, microphysics=microphysics, tracers=tracers, initialize=False)
        self.correction = bool(divergence_correction)
        self.scalars = ["rtheta", "rq"] + [f"rc{t}" for t in range(tracers)]
        self.specific = {"rtheta": "theta", "rq": "q", **{f"rc{t}": f"c{t}" for t in range(tracers)}}
        self.iteration, self.time = 0, 0.0

    # -- set! -----------------------------------------------------------------------------------------------------------------------
    def set(self, **kw):
        m, g = self.m, self.grid
        rho = m.ref.density[g.Hz:g.Hz + g.Nz][:, None, None]
        for name, value in kw.items():
            if name in ("u", "v"):
                g.interior(getattr(m, name))[...] = m._eval(value, "fcc" if name == "u" else "cfc")
            elif name == "w":
                wi = g.interior(m.w, True)
                wi[...] = m._eval(value, "ccf")
                wi[0] = 0.0          # default boundary conditions: impenetrable faces k = 1 and k = Nz + 1
                wi[-1] = 0.0
            elif name == "theta":
                g.interior(m.rtheta)[...] = rho * m._eval(value, "ccc")
            elif name in ("qt", "qv"):
                g.interior(m.rq)[...] = rho * m._eval(value, "ccc")
            elif name in self.scalars:          # a density: rtheta, rq, rc0, ... (set!(model, c = ...) sets the tracer's density field)
                g.interior(getattr(m, name))[...] = m._eval(value, "ccc")
            else:
                raise ValueError(name)
        m._halo_velocity(m.u, xface=True)
        m._halo_velocity(m.v, yface=True)
        m._halo_w(m.w, wall=True)
        self.update_state()

    # -- update_state! without compute_velocities! ------------------------------------------------------------------------------------
    def update_state(self):
        m, g = self.m, self.grid
        cg = C.byref(m.cg)
        p = self.orc._p
        m._halo_center(m.rtheta)
        m._halo_center(m.rq)
        if m.microphysics == "SaturationAdjustment":
            m.lib.og_compute_thermo_sa(cg, C.byref(m._sa), p(m.theta), p(m.q), p(m.qv), p(m.ql), p(m.T), p(m.rtheta), p(m.rq))
            m._halo_center(m.qv)
            m._halo_center(m.ql)
        else:
            m.lib.og_compute_thermo(cg, p(m.theta), p(m.q), p(m.T), p(m.rtheta), p(m.rq))
        for f in (m.T, m.q, m.theta):
            m._halo_center(f)
        rho = m.ref.density[g.Hz:g.Hz + g.Nz][:, None, None]
        for t in range(m.n_tracers):          # tracer_density_to_specific! + halo fill
            c = getattr(m, f"c{t}")
            g.interior(c)[...] = g.interior(getattr(m, f"rc{t}")) / rho
            m._halo_center(c)

    # -- div_rhoU = 1/V [dx(Ax Ix(rho) u) + dy(Ay Iy(rho) v) + dz(Az Iz(rho) w)] -------------------------------------------------------------
    def metrics(self):
        g = self.grid
        dzc = g.dzc[g.Hz:g.Hz + g.Nz][:, None, None]
        return g.dy * dzc, g.dx * dzc, g.dx * g.dy, 1.0 / (g.dx * g.dy * dzc)      # Ax, Ay, Az, 1 / V

    def face_densities(self):
        """Ix(rho) = Iy(rho) = rho_r[k] (a column); Iz(rho) at the faces k = 0 .. Nz."""
        m, g = self.m, self.grid
        rho = m.ref.density
        return rho[g.Hz:g.Hz + g.Nz][:, None, None], (0.5 * (rho[g.Hz - 1:g.Hz + g.Nz] + rho[g.Hz:g.Hz + g.Nz + 1]))[:, None, None]

    def div_rhoU(self):
        """In the reference's order: interpolate rho, times the velocity, times the area, difference, times 1 / V."""
        m, g = self.m, self.grid
        Hx, Hy, Hz, Nx, Ny, Nz = g.Hx, g.Hy, g.Hz, g.Nx, g.Ny, g.Nz
        Ax, Ay, Az, Vinv = self.metrics()
        rho, rho_f = self.face_densities()
        K, J, I = slice(Hz, Hz + Nz), slice(Hy, Hy + Ny), slice(Hx, Hx + Nx)
        dx = Ax * (rho * m.u[K, J, Hx + 1:Hx + Nx + 1]) - Ax * (rho * m.u[K, J, I])
        if g.topo[1] == self.orc.FLAT:
            dy = 0.0
        else:
            dy = Ay * (rho * m.v[K, Hy + 1:Hy + Ny + 1, I]) - Ay * (rho * m.v[K, J, I])
        dz = Az * (rho_f[1:] * m.w[Hz + 1:Hz + Nz + 1, J, I]) - Az * (rho_f[:-1] * m.w[K, J, I])
        return Vinv * (dx + dy + dz)

    def max_mass_flux(self):
        g, m = self.grid, self.m
        rho, rho_f = self.face_densities()
        return max(np.abs(rho * g.interior(m.u)).max(), np.abs(rho * g.interior(m.v)).max(), np.abs(rho_f * g.interior(m.w, True)).max())

    def min_spacing(self):
        g = self.grid
        d = [g.dx, g.dzc[g.Hz:g.Hz + g.Nz].min()]
        if g.topo[1] != self.orc.FLAT:
            d.append(g.dy)
        return min(d)

    # -- tendencies and the step ----------------------------------------------------------------------------------------------------------
    def compute_tendencies(self):
        """G = -div_rhoUc(c) [+ c div_rhoU] of every scalar into self.m.G (interiors)."""
        m, g = self.m, self.grid
        cg = C.byref(m.cg)
        p = self.orc._p
        D = self.div_rhoU() if self.correction else None
        for name in self.scalars:
            c = getattr(m, self.specific[name])
            m.lib.og_scalar_tendency(cg, p(m.G[name]), p(m.u), p(m.v), p(m.w), p(c))
            if D is not None:
                Gi = g.interior(m.G[name])
                Gi[...] = Gi + g.interior(c) * D
        return {name: g.interior(m.G[name]) for name in self.scalars}

    def time_step(self, dt):
        m, g = self.m, self.grid
        if self.iteration == 0:
            self.update_state()
        for name in self.scalars:          # store_initial_state!
            m.U0[name][...] = getattr(m, name)
        for alpha in (1.0, 1.0 / 4.0, 2.0 / 3.0):
            self.compute_tendencies()      # what the previous update_state! ends with: nothing has moved since
            for name in self.scalars:
                m.lib.og_rk3_substep(C.byref(m.cg), self.orc._p(getattr(m, name)), self.orc._p(m.U0[name]), self.orc._p(m.G[name]),
                                     C.c_double(dt), C.c_double(alpha), C.c_int(0), C.c_int(g.Nz))
            self.update_state()
        self.iteration += 1
        self.time += dt

    # -- views ------------------------------------------------------------------------------------------------------------------------------
    def interior(self, name):
        return self.grid.interior(getattr(self.m, name), zface=(name == "w"))

    def cell_volumes(self):
        g = self.grid
        return g.dx * g.dy * g.dzc[g.Hz:g.Hz + g.Nz][:, None, None] * np.ones((g.Nz, g.Ny, g.Nx))
