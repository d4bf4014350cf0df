"""Inputs, oracle runs and the comparison measure for the Kessler column tests (tests/test_oracle_kessler.py on the CPU,
tests/test_kessler_columns.py on the device).  Everything here is deterministic: both sides see the same numbers.

The column case is the smallest that drives `k_kessler_column` through every branch: 72 x 3 columns (one full 64-lane block and
one with 8 live lanes, on three rows), 24 stretched levels, dt = 60 s, rain on the lowest level (surface precipitation), rain
on the top level (the dz_half branch), columns without any rain (W = 0, max_dt = inf, one pass) next to columns that need up to
7 sedimentation subcycles, and a few slightly negative inputs for the clamps.

Measure.  The update leaves small values behind large cancellations (rcl + dC, rv - dC + dE), so an elementwise relative error
is ill-conditioned: the oracle itself moves by 2e-11 elementwise when its inputs move by one unit in the last place.  Errors are
therefore scaled by the largest magnitude of the same field in the same column.
"""
import math

import numpy as np

NX, NY, NZ = 72, 3, 24
X_EXTENT, Y_EXTENT = (0.0, 7200.0), (0.0, 300.0)
Z_FACES = 4000.0 * np.linspace(0.0, 1.0, NZ + 1) ** 1.3
DT = 60.0
P0 = 1e5
VARIANTS = ("arrays", "reference columns")
FIELDS = ("theta", "rtheta", "rqv", "rqcl", "rqr", "qv", "qcl", "qr", "W")

# constants of the reference test's profile (tests/test_gpu_parity.py::test_kessler_column_update_matches_oracle)
R_GAS, CPD, RD = 8.314462618, 1003.0, 287.0
MD = R_GAS / RD
LATENT, TETENS_OFFSET = 2500000.0, 36.0

# c1: the oracle's own conditioning on this case, the largest column-scaled change of any output field (or relative change of the
# precipitation rate) when theta, q^v, q^cl and q^r are each multiplied by 1 +- 2^-52 with random signs; worst of three draws and
# both variants.  Measured 2026-10-19 (x86-64, glibc libm): 1.33e-13, in q^cl of a column whose cloud shrinks to a fifth.  tests/test_oracle_kessler.py measures it again and
# fails when it exceeds twice this constant.
C1_MEASURED = 1.33e-13
# The device differs from the oracle by few-ulp pow / exp differences and FMA contraction, repeated through up to 7 subcycles and
# 24 levels: 100 x c1, and never below the project's tolerance for this kernel.
TOL = max(1e-11, 100.0 * C1_MEASURED)

# columns that carry slightly negative inputs: (i, j) -> species -> levels
NEGATIVE_CELLS = {
    (3, 0): {"rqcl": (1, 2), "rqr": (16, 17), "rqv": (NZ - 1,)},
    (37, 1): {"rqcl": (3,), "rqr": (15,), "rqv": (NZ - 2, NZ - 1)},
    (66, 2): {"rqcl": (0, 22), "rqr": (17, 18), "rqv": (NZ - 1,)},
    (20, 2): {"rqcl": (5,), "rqr": (14,), "rqv": (NZ - 3,)},
}
NEGATIVE_SIZE = {"rqcl": -1e-7, "rqr": -1e-8, "rqv": -1e-6}      # times the cell's density

_RAIN_LEVELS = (0.02, 1.5, 0.3, 6.0, 0.08, 3.0, 0.7)


def z_centers():
    return 0.5 * (Z_FACES[:-1] + Z_FACES[1:])


def constants(ks):
    """(TetensConstants, KesslerParameters) of the oracle for this case."""
    c = ks.TetensConstants(molar_gas_constant=R_GAS, dry_air_molar_mass=MD, vapor_molar_mass=MD, dry_air_heat_capacity=CPD,
                           vapor_heat_capacity=CPD, liquid_latent_heat=LATENT, liquid_heat_capacity=CPD,
                           liquid_temperature_offset=TETENS_OFFSET)
    return c, ks.KesslerParameters()


def reference_columns():
    """Density and pressure of ReferenceState(surface_pressure = 1e5, potential_temperature = 300) on the stretched grid."""
    from oracle import oracle as orc
    g = orc.Grid((NX, NY, NZ), x=X_EXTENT, y=Y_EXTENT, z=Z_FACES)
    c = orc.Constants(molar_gas_constant=R_GAS, dry_air_molar_mass=MD, vapor_molar_mass=MD, dry_air_heat_capacity=CPD,
                      vapor_heat_capacity=CPD)
    ref = orc.ReferenceState(g, c, surface_pressure=P0, potential_temperature=300.0)
    return ref.density[g.Hz:g.Hz + NZ].copy(), ref.pressure[g.Hz:g.Hz + NZ].copy()


def rain_amplitude():
    """a_r(i, j), shape (1, NY, NX): exactly 0 in every ninth column, elsewhere steps of up to 300x between neighbouring lanes."""
    i, j = np.arange(NX)[None, :], np.arange(NY)[:, None]
    a = np.asarray(_RAIN_LEVELS)[(3 * i + 2 * j) % len(_RAIN_LEVELS)] * (1.0 + 0.07 * np.sin(0.9 * i + 1.9 * j))
    a = np.where(dry_columns(), np.maximum(a, 0.3), a)
    return np.where((i + 4 * j) % 9 == 0, 0.0, a)[None]


def dry_columns():
    """(NY, NX) mask of the columns whose vapour stays below saturation everywhere: their cloud evaporates completely."""
    i, j = np.arange(NX)[None, :], np.arange(NY)[:, None]
    return (i + j) % 4 == 0


def moisture_amplitude():
    """Per-column amplitude of vapour and cloud, shape (1, NY, NX), from two bands: 0.15 .. 0.25 in the dry columns, 1.15 .. 2 elsewhere.
    Amplitudes in between leave a cloud remnant of a few percent of the input behind a cancellation, and 0.02-amplitude rain in
    a dry column evaporates to a remnant whose terminal velocity W ~ rr^0.1364 is still large: either makes the column-scaled
    measure ill-conditioned (c1 above 2e-13), which is a property of such inputs and not of an implementation."""
    i, j = np.arange(NX)[None, :], np.arange(NY)[:, None]
    s = 0.5 + 0.5 * np.sin(1.7 * i + 2.3 * j + 0.4)
    return np.where(dry_columns(), 0.15 + 0.1 * s, 1.15 + 0.85 * s)[None]


def column_case(variant, reference=None):
    """Inputs of one variant as (NZ, NY, NX) arrays: rho, p, theta, qv, qcl, qr (mass fractions; the densities handed to the kernel
    are rho * q, with the negative cells of NEGATIVE_CELLS written into rqv / rqcl / rqr).  `reference`: (density, pressure)
    columns for the "reference columns" variant, by default those of reference_columns()."""
    assert variant in VARIANTS
    zc = z_centers()
    i, j, z = np.arange(NX)[None, None, :], np.arange(NY)[None, :, None], zc[:, None, None]
    shape = (NZ, NY, NX)
    if variant == "arrays":
        T1 = 288.0 - 0.0065 * zc
        p1 = 101325.0 * (T1 / 288.0) ** (9.81 / (RD * 0.0065))
        rho1 = p1 / (RD * T1)
        rho = rho1[:, None, None] * (1.0 + 0.02 * np.sin(0.7 * i + 1.3 * j + z / 900.0))
        p = p1[:, None, None] * (1.0 + 0.015 * np.cos(0.5 * i - 0.9 * j + z / 1300.0))
    else:
        rho1, p1 = reference_columns() if reference is None else reference
        rho, p = np.broadcast_to(rho1[:, None, None], shape).copy(), np.broadcast_to(p1[:, None, None], shape).copy()
    T = p / (RD * rho)
    amp = moisture_amplitude()
    a_r = rain_amplitude()
    rv = 0.015 * np.exp(-((z - 1000.0) / 1000.0) ** 2) * amp
    rcl = np.where((z > 1500.0) & (z < 2500.0), 0.002, 0.0) * amp
    rr = (np.where(z < 2000.0, 0.0005, 0.0) + np.where(z > 3500.0, 0.0003, 0.0)) * a_r
    rt = rv + rcl + rr
    qv, qcl, qr = rv / (1 + rt), rcl / (1 + rt), rr / (1 + rt)
    ql = qcl + qr
    Rd, cpd = R_GAS / MD, CPD                                                   # R_v = R_d, c_pv = c_l = c_pd here
    cpm = (1 - (qv + ql)) * cpd + qv * cpd + ql * cpd
    Rm = (1 - (qv + ql)) * Rd + qv * Rd
    theta = (T - LATENT * ql / cpm) / (p / P0) ** (Rm / cpm)
    case = {"rho": rho, "p": p, "theta": theta, "qv": qv, "qcl": qcl, "qr": qr}
    return densities(case)


def densities(case):
    """Add rtheta, rqv, rqcl, rqr = rho * (theta, qv, qcl, qr) to a case, with the negative cells written in."""
    rho = case["rho"]
    out = dict(case)
    out["rtheta"] = rho * case["theta"]
    for n, q in (("rqv", "qv"), ("rqcl", "qcl"), ("rqr", "qr")):
        out[n] = rho * case[q]
    for (i, j), cells in NEGATIVE_CELLS.items():
        for n, levels in cells.items():
            for k in levels:
                out[n][k, j, i] = NEGATIVE_SIZE[n] * rho[k, j, i]
    return out


def negative_columns():
    mask = np.zeros((NY, NX), dtype=bool)
    for (i, j) in NEGATIVE_CELLS:
        mask[j, i] = True
    return mask


def subcycle_ratio(ks, dt, rho, zc, rqv, rqcl, rqr, mp):
    """dt / max_dt of one column, from the oracle's own functions in the kernel's operation order: Ns = max(1, ceil(ratio))."""
    max_dt = dt
    for k in range(len(rho) - 1):
        r = rho[k]
        qv, qcl, qr = max(0, rqv[k] / r), max(0, rqcl[k] / r), max(0, rqr[k] / r)
        inv_qd = 1.0 / (1 - (qv + (qcl + qr) + 0.0))
        rt = qv * inv_qd + (qcl + qr) * inv_qd + 0.0 * inv_qd
        W = ks.terminal_velocity(qr * (1 + rt), r, rho[0], mp)
        if W > 0:
            max_dt = min(max_dt, mp.substep_cfl * (zc[k + 1] - zc[k]) / W)
    return dt / max_dt


def subcycle_ratios(ks, dt, rho, zc, rqv, rqcl, rqr, mp):
    """subcycle_ratio of every column of (Nz, Ny, Nx) arrays; rho may be a 1-D column."""
    Ny, Nx = rqv.shape[1:]
    rho3 = np.broadcast_to(rho[:, None, None], rqv.shape) if rho.ndim == 1 else rho
    out = np.zeros((Ny, Nx))
    for j in range(Ny):
        for i in range(Nx):
            out[j, i] = subcycle_ratio(ks, dt, rho3[:, j, i], zc, rqv[:, j, i], rqcl[:, j, i], rqr[:, j, i], mp)
    return out


def integer_distance(ratios):
    """Distance of dt / max_dt from the nearest integer over the columns that subcycle (ratio > 1); inf if none does."""
    r = np.asarray(ratios)
    r = r[r > 1.0]
    return float(np.abs(r - np.round(r)).min()) if r.size else math.inf


def run_oracle(ks, case, dt=DT):
    """oracle.kessler.kessler_column_update on every column of a case: the nine output fields as (NZ, NY, NX) arrays,
    "precip" and "Ns" as (NY, NX)."""
    c, mp = constants(ks)
    zc = z_centers()
    out = {n: np.zeros((NZ, NY, NX)) for n in FIELDS}
    out["precip"], out["Ns"] = np.zeros((NY, NX)), np.zeros((NY, NX), dtype=int)
    for j in range(NY):
        for i in range(NX):
            cols = [np.ascontiguousarray(case[n][:, j, i]) for n in ("rho", "p", "theta", "rtheta", "rqv", "rqcl", "rqr")]
            rho, p, th, rth, a, b, d = cols
            qv, qcl, qr, W, P, Ns = ks.kessler_column_update(dt, rho, p, P0, zc, th, rth, a, b, d, mp, c)
            for n, col in zip(FIELDS, (th, rth, a, b, d, qv, qcl, qr, W)):
                out[n][:, j, i] = col
            out["precip"][j, i], out["Ns"][j, i] = P, Ns
    return out


_CACHE = {}


def oracle_case(ks, variant):
    """(inputs, oracle outputs, dt / max_dt) of a variant on the default reference columns, computed once and read-only."""
    if variant not in _CACHE:
        case = column_case(variant)
        want = run_oracle(ks, case)
        _, mp = constants(ks)
        ratios = subcycle_ratios(ks, DT, case["rho"], z_centers(), case["rqv"], case["rqcl"], case["rqr"], mp)
        for d in (case, want):
            for a in d.values():
                a.setflags(write=False)
        ratios.setflags(write=False)
        _CACHE[variant] = (case, want, ratios)
    return _CACHE[variant]


def column_errors(got, want, fields=FIELDS):
    """Per field, the worst column-scaled error max_k |got - want| / max_k |want| over the columns, with the (i, j) of the worst
    column.  A column that the reference leaves identically zero must be identically zero: its error is 0 if it is, inf if not."""
    worst = {}
    for n in fields:
        g, w = np.asarray(got[n], dtype=np.float64), np.asarray(want[n], dtype=np.float64)
        assert g.shape == w.shape, (n, g.shape, w.shape)
        scale = np.abs(w).max(axis=0)
        with np.errstate(invalid="ignore"):
            diff = np.abs(g - w).max(axis=0)
        diff = np.where(np.isfinite(g).all(axis=0), diff, np.inf)
        err = np.where(scale > 0, diff / np.where(scale > 0, scale, 1.0), np.where(diff == 0, 0.0, np.inf))
        j, i = np.unravel_index(np.argmax(err), err.shape)
        worst[n] = (float(err[j, i]), (int(i), int(j)))
    return worst


def precipitation_error(got, want):
    """Worst relative error of the precipitation rate over the columns where the reference is non-zero; inf where the
    reference is exactly zero and the device is not."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape
    nz = want != 0
    err = np.where(nz, np.abs(got - want) / np.where(nz, np.abs(want), 1.0), np.where(got == 0, 0.0, np.inf))
    err = np.where(np.isfinite(got), err, np.inf)
    j, i = np.unravel_index(np.argmax(err), err.shape)
    return float(err[j, i]), (int(i), int(j))


def assert_columns_match(label, got, want, tol=TOL):
    """Every column of every field within tol of the column's own scale, precipitation within tol relative; prints the worst
    errors before asserting and returns them."""
    worst = column_errors(got, want)
    worst["precip"] = precipitation_error(got["precip"], want["precip"])
    print(f"kessler columns [{label}] tol {tol:.1e}:", " ".join(f"{n}={e:.1e}@{ij}" for n, (e, ij) in worst.items()))
    bad = {n: v for n, v in worst.items() if not v[0] <= tol}
    assert not bad, f"{label}: column-scaled errors beyond {tol:.1e} (field: (error, (i, j))): {bad}"
    return worst


# ---- whole model steps whose columns subcycle -------------------------------------------------------------------------------------------
# The moist bubble of the Kessler model tests, low enough for its rain to reach the ground.  dt is the smallest whole number of
# seconds at which columns reach Ns = 3 with every dt / max_dt at least 1e-3 from an integer (rain falls at up to 5.6 m/s:
# max_dt = 0.8 dz / W is 7.1 s on 50 m levels, 1.4 s on 10 m levels).  Larger steps make the step itself ill-conditioned: the bubble's
# cloud evaporates in the first column update, the cooled air sinks at 4 to 5 m/s, and at dt = 22 s on 50 m levels (vertical
# advective Courant number 2) the oracle's own W moves by 1.3e-8 of its scale when its initial state moves by one unit in the last
# place, more than the 1e-8 the device is held to.  tests/test_oracle_kessler.py asserts that the oracle's own one-ulp response
# stays below STEPS_CONDITIONING.
ANELASTIC_STEPS = dict(size=(16, 12, 40), z=(0.0, 2000.0), bubble_height=600.0, dt=16.0, steps=2)
# The compressible case starts at rest.  On its 10 m levels a 2 m/s wind drags WENO tails of rain of 1e-17 into clear cells, where the
# column update evaporates them to exactly zero and leaves W ~ rr^0.1364 = 0.08 m/s computed from the tail: the oracle's own W then
# moves by 4.4e-8 of its scale under a one-ulp change of the initial state (1.1e-10 at rest).  The bubble's own circulation keeps the
# density three-dimensional.
COMPRESSIBLE_STEPS = dict(size=(16, 12, 40), z=(0.0, 400.0), bubble_height=200.0, dt=4.0, steps=2, substeps=12, u=0.0)
STEPS_X, STEPS_Y = (0.0, 4e3), (0.0, 3e3)
STEPS_TOL = 1e-8                    # of the field scale: the tolerance of the model tests these cases are built from
STEPS_CONDITIONING = STEPS_TOL / 4  # the most the oracle may move under a one-ulp change of its initial state


def bubble(height):
    return lambda x, y, z: np.maximum(0.0, 1.0 - np.sqrt((x - 2e3) ** 2 + (y - 1.5e3) ** 2 + (z - height) ** 2) / 1200.0)


def anelastic_initial_conditions(bubble_height=1500.0):
    bub = bubble(bubble_height)
    return dict(qt=lambda x, y, z: 0.016 * np.exp(-z / 3000.0) + 0.004 * bub(x, y, z),
                theta=lambda x, y, z: 300.0 + 0.004 * z + 1.0 * bub(x, y, z),
                qcl=lambda x, y, z: 0.003 * bub(x, y, z), qr=lambda x, y, z: 0.001 * bub(x, y, z), u=2.0)


def compressible_initial_conditions(bubble_height=1500.0, u=2.0):
    bub = bubble(bubble_height)
    return dict(theta=lambda x, y, z: 300.0 + 0.004 * z + 1.0 * bub(x, y, z),
                qv=lambda x, y, z: 0.014 * np.exp(-z / 3000.0) + 0.004 * bub(x, y, z),
                qcl=lambda x, y, z: 0.003 * bub(x, y, z), qr=lambda x, y, z: 0.001 * bub(x, y, z), u=u, v=0.0, w=0.0)


def anelastic_oracle(oracle, size, z, **_):
    og = oracle.Grid(size, x=STEPS_X, y=STEPS_Y, z=z)
    return oracle.OracleModel(og, surface_pressure=1e5, potential_temperature=300.0, microphysics="Kessler")


def compressible_oracle(oracle, oc, size, z, substeps, **_):
    og = oracle.Grid(size, x=STEPS_X, y=STEPS_Y, z=z)
    return oc.CompressibleOracleModel(og, time_discretization=oc.SplitExplicit(substeps=substeps), surface_pressure=1e5,
                                      reference_potential_temperature=300.0, microphysics="Kessler")


def set_compressible_oracle(om, bubble_height, u=2.0, **_):
    g = om.grid
    rho = om.ref.density[g.Hz:g.Hz + g.Nz][:, None, None]
    om.set(rho=rho, **compressible_initial_conditions(bubble_height, u))
    return rho


def record_subcycling(ks, om, dt, density):
    """Records dt / max_dt of every column of an oracle model: record["measure"]() takes it now ("before" a step), and every later
    call of the model's column update takes it from the state the columns really see, after the dynamics of the step ("at call")."""
    g = om.grid
    I = g.interior
    ratios = lambda: subcycle_ratios(ks, dt, density(), g.zc, I(om.rq), I(om.rqcl), I(om.rqr), om.kessler)
    record = {"before": [], "at call": []}
    update = om.microphysics_model_update

    def recording_update(d):
        record["at call"].append(ratios())
        return update(d)
    om.microphysics_model_update = recording_update
    record["measure"] = lambda: record["before"].append(ratios())
    return record


def assert_subcycling(label, record, steps):
    """Before every step and at every column update: columns at Ns = 1 and at Ns >= 3, and no ratio within 1e-3 of an integer."""
    assert len(record["before"]) == len(record["at call"]) == steps
    for when in ("before", "at call"):
        for s, r in enumerate(record[when]):
            Ns = np.maximum(1, np.ceil(r)).astype(int)
            d = integer_distance(r)
            print(f"{label} step {s} ({when}): Ns {sorted(set(Ns.ravel().tolist()))}, {(Ns >= 3).sum()} columns at Ns >= 3, integer distance {d:.2e}")
            assert Ns.max() >= 3 and Ns.min() == 1 and len(set(Ns.ravel().tolist())) >= 3, (label, when, s)
            assert d >= 1e-3, (label, when, s, d)


def move_by_one_ulp(om, names, seed):
    """Multiply the interior of the named prognostic fields of an oracle model by 1 +- 2^-52, random signs."""
    rng = np.random.default_rng(seed)
    for n in names:
        a = om.grid.interior(getattr(om, n))
        a *= 1.0 + rng.choice([-1.0, 1.0], size=a.shape) * 2.0 ** -52
    om.update_state(compute_tendencies=False)


def field_scale_errors(om_a, om_b, names):
    """max |a - b| over the interior relative to the field's scale (the momentum components share one scale)."""
    g = om_a.grid
    I = lambda m, n: g.interior(getattr(m, n), n == "rw")
    mom = max(np.abs(I(om_a, n)).max() for n in ("ru", "rv", "rw"))
    return {n: float(np.abs(I(om_a, n) - I(om_b, n)).max() / (mom if n in ("ru", "rv", "rw") else max(np.abs(I(om_a, n)).max(), 1e-9)))
            for n in names}
