"""Shared helpers for the parity tests: matched oracle / HIP models on the same seeded inputs."""
import numpy as np


def bubble_theta(theta0, g, N2=1e-6, dtheta=10.0, r0=2e3, zc=3000.0):
    def f(x, y, z):
        r = np.sqrt(x ** 2 + y ** 2 + (z - zc) ** 2)
        return theta0 * np.exp(N2 * z / g) + dtheta * np.maximum(0.0, 1.0 - r / r0)
    return f


def make_pair(orc, bz, size, halo=(3, 3, 3), extent=((-10e3, 10e3), (-10e3, 10e3), (0.0, 10e3)), theta0=300.0,
              z_faces=None, formulation="LiquidIcePotentialTemperature"):
    """Return (oracle model, HIP model) on identical grids / reference states."""
    z = z_faces if z_faces is not None else extent[2]
    og = orc.Grid(size, x=extent[0], y=extent[1], z=z, halo=halo)
    om = orc.OracleModel(og, potential_temperature=theta0, formulation=formulation)
    grid = bz.RectilinearGrid(size, x=extent[0], y=extent[1], z=z, halo=halo)
    ref = bz.ReferenceState(grid, potential_temperature=theta0)
    hm = bz.AtmosphereModel(grid, dynamics=bz.AnelasticDynamics(ref), advection=bz.WENO(order=5), formulation=formulation)
    return om, hm


ORACLE_TO_HIP = {
    "ru": lambda m: m.momentum["ρu"], "rv": lambda m: m.momentum["ρv"], "rw": lambda m: m.momentum["ρw"],
    "rtheta": lambda m: m.potential_temperature_density, "rq": lambda m: m.moisture_density,
    "u": lambda m: m.velocities["u"], "v": lambda m: m.velocities["v"], "w": lambda m: m.velocities["w"],
    "theta": lambda m: m.potential_temperature, "q": lambda m: m.specific_moisture, "T": lambda m: m.temperature,
    "phi": lambda m: m.dynamics.pressure_anomaly,
}
PROG = {"ru": "ρu", "rv": "ρv", "rw": "ρw", "rtheta": "ρθ", "rq": "ρq"}


def push_state(om, hm, names=None):
    """Copy oracle parent arrays (halos included) into the HIP model's fields, bit for bit."""
    import torch
    for n in (names or ORACLE_TO_HIP):
        ORACLE_TO_HIP[n](hm).parent.copy_(torch.from_numpy(getattr(om, n)))
    for n, k in PROG.items():
        hm.G[k].parent.copy_(torch.from_numpy(om.G[n]))
        hm.U0[k].parent.copy_(torch.from_numpy(om.U0[n]))


def randomize(om, seed, amp_u=5.0, amp_theta=2.0, amp_q=5e-3):
    """Seeded smooth + rough perturbation of every prognostic field of the oracle model (interior),
    followed by update_state so that halos / diagnostics are consistent."""
    g = om.grid
    rng = np.random.default_rng(seed)
    x, y, z = g.nodes("ccc")
    Lx, Ly, Lz = g.Nx * g.dx, g.Ny * g.dy, g.zf[-1] - g.zf[0]

    def field(shape, amp):
        smooth = np.sin(2 * np.pi * x / Lx + 0.3) * np.cos(2 * np.pi * y / Ly - 0.2) * np.sin(np.pi * (z - g.zf[0]) / Lz)
        return amp * (np.broadcast_to(smooth, shape) * 0.7 + 0.3 * rng.standard_normal(shape))

    Hz, Nz = g.Hz, g.Nz
    rho_c = om.ref.density[Hz:Hz + Nz][:, None, None]
    sh = (g.Nz, g.Ny, g.Nx)
    g.interior(om.ru)[...] = rho_c * field(sh, amp_u)
    g.interior(om.rv)[...] = rho_c * field(sh, amp_u)
    wi = np.zeros((g.Nz + 1, g.Ny, g.Nx))
    wi[1:-1] = 0.5 * (field(sh, amp_u)[1:] + field(sh, amp_u)[:-1])
    g.interior(om.rw, True)[...] = wi
    g.interior(om.rtheta)[...] = rho_c * (om.ref.theta0 + field(sh, amp_theta))
    g.interior(om.rq)[...] = rho_c * np.abs(field(sh, amp_q))
    om.update_state(compute_tendencies=False)


def relerr(a, b):
    scale = np.max(np.abs(b))
    return np.max(np.abs(a - b)) / (scale if scale > 0 else 1.0)


# ---- Float32 steps: errors measured against what the step did, not against the field's background ----------------------------------------
def increment_error(got, want, start, floor=1e-7):
    """max|got - want| / max|want - start|: the error of a stepped field relative to the largest change the reference made to it.
    `start` is the state both models were given (interior, Float64) before the first step.  A field the reference did not move
    (max|want - start| <= floor * max|want|, or zero) cannot be judged this way, and is an error rather than a vacuous pass."""
    got, want, start = (np.asarray(a, dtype=np.float64) for a in (got, want, start))
    inc = float(np.max(np.abs(want - start)))
    if not inc > floor * float(np.max(np.abs(want))) or inc == 0.0:
        raise ValueError(f"increment_error: the reference moved the field by {inc:.3e} only (max |want| {np.max(np.abs(want)):.3e})")
    return float(np.max(np.abs(got - want))) / inc


# Tolerances of increment_error for Float32 models against the Float64 oracle (or, where stated, against a Float32 run of a second
# kernel sequence), per field, one table for each dynamical core and one for Float32 substep storage in a Float64 compressible model.
# Each value is at most 4x the worst error measured on the MI355X over every case that uses it (tests/test_float32.py,
# tests/test_float32_increments.py, tests/test_gpu_compressible.py), and at most a third of the smallest error the CPU test
# tests/test_float32_tolerances.py measures between the oracle and the oracle with a known defect (dt x 1.01, WENO7 for WENO5,
# 5 acoustic substeps for 6).  Worst measured on the MI355X (lean and BZ_NO_LEAN=1 runs agree to the digits shown):
#   anelastic     ru 7.6e-5 (mixed orders), rv 6.8e-5 (mixed orders), rw 3.2e-5 (BOMEX), rho theta 1.3e-3 (sweep, walls in y, first step),
#                 rho q 4.6e-4 (mixed orders), T 2.0e-3 (sweep, walls in y, first step), tracer 2.6e-4, rho q^r 5.9e-6 (Kessler)
#   compressible  rho_d 2.8e-4, rho theta 2.4e-4, rho q 4.8e-4, T 6.2e-4, p 3.2e-4, rho u 5.2e-4, rho w 3.3e-4
#   substep storage (Float32 acoustic working fields in a Float64 model): rho_d 6.8e-8, rho theta 2.1e-8, rho q 6.2e-8, T 1.8e-7,
#                 p 2.1e-8, rho u 1.8e-7, rho v 2.4e-7, rho w 4.7e-8
# The smallest defect distances (dt x 1.01) are 6.5e-3 .. 1e-2 of the increment for every field but two of the anelastic Kessler case
# (see tests/test_float32_tolerances.py: DT_EXEMPT).
F32_INCREMENT_TOL = {
    "anelastic": {"ru": 2e-4, "rv": 2e-4, "rw": 1.2e-4, "rtheta": 2e-3, "rq": 1e-3, "T": 2.9e-3, "rc0": 1e-3, "rqr": 2.3e-5},
    "compressible": {"rho_d": 1e-3, "rtheta": 9e-4, "rq": 1.5e-3, "T": 2e-3, "p": 1.2e-3, "ru": 1.5e-3, "rw": 1.2e-3},
    "substep_storage": {"rho_d": 2.5e-7, "rtheta": 8e-8, "rq": 2.4e-7, "T": 7e-7, "p": 8e-8, "ru": 7e-7, "rv": 9e-7, "rw": 1.8e-7},
}


def assert_increments(label, got, want, start, table, report=None):
    """increment_error of every field of `got` (name -> array) against F32_INCREMENT_TOL[table]; all fields are measured and printed
    before the assertion so that one run shows the whole picture."""
    tol = F32_INCREMENT_TOL[table]
    errs = {n: increment_error(got[n], want[n], start[n]) for n in got}
    print(f"F32INC {label} [{table}]:", " ".join(f"{n}={e:.2e}" for n, e in errs.items()))
    if report is not None:
        report.update(errs)
    bad = {n: (e, tol[n]) for n, e in errs.items() if not e < tol[n]}
    assert not bad, f"{label}: increment errors beyond the Float32 tolerance {bad} (all: {errs})"
    return errs
