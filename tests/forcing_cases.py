"""Grids, forcing stacks and states shared by tests/test_forcing_reference.py (CPU: oracle/forcings.py against the long-double reference of
tests/forcing_reference.py) and tests/test_forcing_device.py (device kernels of csrc/bz_forcing.hip against that reference).

GRIDS: those of tests/advection_cases.py (order 5, halos of 3; stretched z = Lz linspace(0, 1, Nz + 1)^1.3) and two more:
  waves   (320, 8, 6) stretched, periodic: rows of five wavefronts in k_level_wave_sums, the second 256-thread block with one live wave
  short   (16, 8, 3) stretched, periodic: the bottom and the top cell of the subsidence profile with ONE cell taking the two-face mean between
          them.  The issue asked for Nz = 2; a context refuses Nz < Hz (csrc/bz_context.hip: bzi_create returns BZ_ERR_UNSUPPORTED) and
          order 5 needs Hz = 3, so Nz = 3 is the smallest column a device model is created on.

PROFILES: w_s, the geostrophic wind, the drying and cooling columns, the sponge rates and their targets are piecewise linear in s = z / Lz
with one kink and one sign change each and are non-zero at the first and the last level (the theta targets change sign relative to the 300 K
background: 300 + a sign-changing profile).  Amplitudes are set so that each term is visible beside the advective tendency of the state it
is added to (the ratio is printed by both tests and asserted on the CPU: within two orders of magnitude on at least one grid per term).

STACKS (reference arguments, oracle/forcings.py arguments and the bz constructor's keywords come from the same record):
  bomex, bomex_eps0   FPlane, geostrophic F_u, F_v, subsidence on u, v, theta, q, drying F_q, cooling F_e, constant J_theta, J_q and the
                      friction-velocity drag with epsilon = 1e-10 / 0 (the two differ in the bottom fluxes only)
  momentum_only       FPlane, geostrophic profiles, J_theta and the drag with epsilon = 1e-10: the CBL list, k_apply_forcings<false>
  sub_u, sub_v, sub_theta, sub_q   subsidence on that one field (the mask bits and the field order of the partial sums)
  sponge_density      Relaxation keyed rho u, rho v, rho w, rho theta, rho q and a 3-D Forcing keyed rho theta
  sponge_specific     Relaxation keyed u, v, w and a 3-D Forcing keyed theta.  (One Relaxation per field is what the host takes — breeze.jl_amd
                      /forcings.py: materialize_relaxation — so the two keyed forms are two stacks.)
  bulk                BulkDrag, BulkSensibleHeatFlux, BulkVaporFlux with constant coefficients, three surface temperatures, three gustinesses
  energy_flux         a bottom flux keyed rho e, and J_q
bomex, bomex_eps0, bulk and energy_flux also run with SaturationAdjustment(WarmPhaseEquilibrium) on the moist state.  No grid and stack
pair of these tables is refused by the host or the library.

STATES: dry — the planted state of advection_cases.oracle_case (built the same way on "waves"; "short" keeps the seeded state of
helpers.randomize alone, its three levels hold no planted line); moist — a seeded state on a
stratified theta with q scattered about saturation, so that cloudy and clear cells sit side by side at the first level and aloft
(test_forcing_reference asserts it).  Both carry cell-scale noise in every field: the points of every horizontal average differ."""
import functools

import numpy as np

import advection_cases as adv
import forcing_reference as ref

LD = ref.LD
GRIDS = dict(adv.GRIDS)
GRIDS["waves"] = ((320, 8, 6), True, adv.PPB)
GRIDS["short"] = ((16, 8, 3), True, adv.PPB)
ORDER, LZ = 5, adv.EXT[2][1]
P0, PST, THETA0 = 101325.0, 1e5, 300.0
FIELDS = ("ru", "rv", "rw", "rtheta", "rq")
KIND = {"ru": "u", "rv": "v", "rw": "w", "rtheta": "c", "rq": "c"}
MOIST_STACKS = ("bomex", "bomex_eps0", "bulk", "energy_flux")


def z_faces(name):
    size, stretched, _ = GRIDS[name]
    a, b = adv.EXT[2]
    return a + (b - a) * np.linspace(0.0, 1.0, size[-1] + 1) ** 1.3 if stretched else adv.EXT[2]


def grid_arguments(name):
    """(size, keyword arguments) of oracle.Grid; RectilinearGrid takes the same with its own topology objects"""
    size, _, topo = GRIDS[name]
    kw = dict(x=adv.EXT[0], z=z_faces(name), topology=topo, halo=(3,) * len(size))
    if len(size) == 3:
        kw["y"] = adv.EXT[1]
    return size, kw


# ---- profiles: piecewise linear in s = z / Lz, (value at 0, slope below the kink, kink, slope above) ---------------------------------------
def _pl(a, b, sk, c):
    def f(z):
        s = z / LZ
        return a + b * s if s < sk else a + b * sk + c * (s - sk)
    return f


F0 = 2.0e-3
w_subsidence = _pl(2.7, -8.4, 0.5, -1.8)                # m/s: 2.7 -> -1.5 at the kink -> -2.4
u_geostrophic = _pl(-8.0, 26.0, 0.4, -3.0)
v_geostrophic = _pl(3.0, -10.0, 0.5, 1.0)
drying = _pl(-2.0e-7, 5.0e-7, 0.5, -0.8e-7)
cooling = _pl(-30.0, 90.0, 0.5, -18.0)                  # F_e = c_pd dT/dt, W/kg
J_THETA, J_Q, RHO0, USTAR, Q_ENERGY = 0.35, 6.0e-5, 1.15, 0.4, 120.0
RATES = {"u": _pl(-2e-3, 1.5e-2, 0.6, 4e-3), "v": _pl(-2.5e-3, 1.4e-2, 0.55, 5e-3), "w": _pl(-1.5e-3, 1.6e-2, 0.5, 3e-3),
         "theta": _pl(-3e-3, 3.6e-2, 0.65, 1.8e-2), "q": _pl(-3e-3, 1.3e-2, 0.45, 2e-3)}
TARGETS = {"u": _pl(4.0, -14.0, 0.5, 2.0), "v": _pl(-3.0, 11.0, 0.4, -2.5), "w": _pl(0.8, -3.0, 0.45, 0.6),
           "theta": _pl(1.5, -6.0, 0.5, 1.0), "q": _pl(4e-3, -1.4e-2, 0.5, 2e-3)}
# (the heat condition's T_0 keeps theta - theta_0 at several kelvin: the difference of two numbers near 300 K is then conditioned well enough
# for a bound of 1e-13 in Float64)
BULK = dict(drag=(1.2e-3, 0.2, 299.8), heat=(1.1e-3, 0.35, 312.0), vapor=(1.3e-3, 0.1, 302.4))


def heating(x, y, z):
    """a rainband-like patch (K/s) that changes sign across the domain"""
    return 4e-2 * np.sin(2 * np.pi * x / 20e3 + 0.4) * np.cos(2 * np.pi * y / 20e3 - 0.3) * (0.3 + np.sin(np.pi * z / LZ) ** 2)


def _stack(**kw):
    base = dict(f=0.0, geostrophic=False, subsidence=(), drying=False, cooling=False, J_theta=0.0, J_q=0.0, drag=None, Q=0.0, bulk=None,
                relax=(), field_forcing=None)
    base.update(kw)
    return base


STACKS = {
    "bomex": _stack(f=F0, geostrophic=True, subsidence=("u", "v", "theta", "q"), drying=True, cooling=True, J_theta=RHO0 * 8e-3, J_q=RHO0 * 5.2e-5,
                    drag=(RHO0 * USTAR ** 2, 1e-10)),
    "bomex_eps0": _stack(f=F0, geostrophic=True, subsidence=("u", "v", "theta", "q"), drying=True, cooling=True, J_theta=RHO0 * 8e-3,
                         J_q=RHO0 * 5.2e-5, drag=(RHO0 * USTAR ** 2, 0.0)),
    "momentum_only": _stack(f=F0, geostrophic=True, J_theta=RHO0 * J_THETA, drag=(RHO0 * USTAR ** 2, 1e-10)),
    "sub_u": _stack(subsidence=("u",)), "sub_v": _stack(subsidence=("v",)), "sub_theta": _stack(subsidence=("theta",)),
    "sub_q": _stack(subsidence=("q",)),
    "sponge_density": _stack(relax=("ru", "rv", "rw", "rtheta", "rq"), field_forcing="rtheta"),
    "sponge_specific": _stack(relax=("u", "v", "w"), field_forcing="theta"),
    "bulk": _stack(bulk=BULK),
    "energy_flux": _stack(Q=Q_ENERGY, J_q=J_Q),
}
SUBSIDENCE_ONE = ("sub_u", "sub_v", "sub_theta", "sub_q")


# ---- states -------------------------------------------------------------------------------------------------------------------------------
def _oracle_grid(name):
    from oracle import oracle
    oracle.build()
    size, kw = grid_arguments(name)
    return oracle, oracle.Grid(size, **kw)


@functools.lru_cache(maxsize=None)
def dry_state(name):
    """the oracle model holding the planted dry state (computed once, shared with the advection tests, never changed)"""
    if name in adv.GRIDS:
        return adv.oracle_case(name, ORDER)
    from helpers import randomize
    oracle, og = _oracle_grid(name)
    om = oracle.OracleModel(og, potential_temperature=THETA0)
    randomize(om, seed=adv.SEED)
    om.planted = adv.plant(om) if og.Nz >= 6 else None          # "short": three levels hold no planted line; the seeded state as it is
    return om


@functools.lru_cache(maxsize=None)
def moist_state(name):
    """a saturation-adjustment oracle model: theta = 300 + 3 K / km z + 0.3 K of smooth-plus-rough perturbation, q = the saturation humidity
    of the reference column times (1 + 0.25 x perturbation), winds of 0.7 m/s; update_state diagnoses q^v, q^l, T and fills the halos"""
    oracle, og = _oracle_grid(name)
    om = oracle.OracleModel(og, potential_temperature=THETA0, microphysics="SaturationAdjustment")
    g = og
    rng = np.random.default_rng(adv.SEED + 1)
    x, y, z = g.nodes("ccc")
    Lx, Ly = g.Nx * g.dx, g.Ny * g.dy
    sh = (g.Nz, g.Ny, g.Nx)

    def field():
        smooth = np.sin(2 * np.pi * x / Lx + 0.3) * np.cos(2 * np.pi * y / Ly - 0.2) * (0.4 + np.sin(np.pi * z / LZ))
        return np.broadcast_to(smooth, sh) * 0.6 + 0.4 * rng.uniform(-1.0, 1.0, sh)

    rho = om.ref.density[g.Hz:g.Hz + g.Nz][:, None, None]
    # saturation humidity of the level's mean state: T = Pi_r theta_mean, q+ = eps p+ / (p_r - p+) with the Clausius-Clapeyron p+ of the reference
    c = ref.CONSTANTS
    T_m = om.ref.temperature[g.Hz:g.Hz + g.Nz] * (THETA0 + 3e-3 * g.zc) / THETA0
    p_r = om.ref.pressure[g.Hz:g.Hz + g.Nz]
    ps = np.array([float(ref.saturation_specific_humidity(T_m[k], 1.0, c)) * (c.R / c.Mv) * T_m[k] for k in range(g.Nz)])
    qs = ((c.Mv / c.Md) * ps / (p_r - ps))[:, None, None]
    g.interior(om.ru)[...] = rho * 0.7 * field()
    g.interior(om.rv)[...] = rho * 0.7 * field()
    wi = np.zeros((g.Nz + 1,) + sh[1:])
    f1, f2 = field(), field()
    wi[1:-1] = 0.15 * (f1[1:] + f2[:-1])
    g.interior(om.rw, True)[...] = wi
    g.interior(om.rtheta)[...] = rho * (THETA0 + 3e-3 * z + 0.3 * field())
    g.interior(om.rq)[...] = rho * qs * (1.0 + 0.25 * field())
    om.update_state(compute_tendencies=False)
    return om


def state(name, moist):
    return moist_state(name) if moist else dry_state(name)


def geometry(om):
    return adv.geometry(om)


STATE_ARRAYS = ("ru", "rv", "rw", "rtheta", "rq", "u", "v", "w", "theta", "q", "T", "qv", "ql")


def state_fields(om):
    return {n: getattr(om, n) for n in STATE_ARRAYS}


# ---- columns of a stack on a grid (Float64: what the host hands to the library, and what the reference takes as data) ----------------------
def columns(name, stack_id):
    om = dry_state(name)
    g, S = om.grid, STACKS[stack_id]
    zc, zf = g.zc, g.zf
    col = lambda fn, z: np.array([float(fn(v)) for v in z])
    rho = om.ref.density[g.Hz:g.Hz + g.Nz].copy()
    out = dict(rho=rho, p_r=om.ref.pressure[g.Hz:g.Hz + g.Nz].copy(), Fu=None, Fv=None, Fq=None, Fe=None, ws=None, relax={}, F3=None)
    if S["geostrophic"]:
        out["Fu"], out["Fv"] = -S["f"] * col(v_geostrophic, zc), S["f"] * col(u_geostrophic, zc)
    if S["drying"]:
        out["Fq"] = col(drying, zc)
    if S["cooling"]:
        out["Fe"] = col(cooling, zc)
    if S["subsidence"]:
        out["ws"] = col(w_subsidence, zf)
    for key in S["relax"]:
        spec = key.lstrip("r")
        z = zf if spec == "w" else zc
        target = col(TARGETS[spec], z)
        if spec == "theta":
            target = THETA0 + target
        if key.startswith("r") and spec != "w":
            target = rho * target          # a density target: the same Float64 column goes to the host, the oracle and the reference
        out["relax"][key] = (col(RATES[spec], z), target)
    if S["field_forcing"]:
        x, y, z = g.nodes("ccc")
        out["F3"] = np.ascontiguousarray(np.broadcast_to(heating(x, y, z), (g.Nz, g.Ny, g.Nx)))
    return out


# ---- the reference, term by term -------------------------------------------------------------------------------------------------------------
SWITCHES = ("subsidence_dzf_shift", "subsidence_ends_halved", "coriolis_two_point", "coriolis_same_sign", "energy_dry_constants",
            "drag_unaveraged_speed", "bulk_square_of_mean", "relaxation_w_centre_density", "bottom_dz_regular")


def reference_terms(name, stack_id, moist, fields=None, **switch):
    """{"coriolis", "column", "energy", "relaxation", "field", "flux"}: {field: long-double array} of the terms the stack holds ("flux":
    (Ny, Nx) arrays of the first level), "avg" / "sub": the horizontal averages and subsidence profiles (Nz values per name).  fields: the
    halo-inclusive state arrays (default: the shared oracle state)."""
    assert set(switch) <= set(SWITCHES), switch
    on = lambda k: bool(switch.get(k, False))
    om = state(name, moist)
    geo, S, C, c = geometry(om), STACKS[stack_id], columns(name, stack_id), ref.CONSTANTS
    A = fields or state_fields(om)
    g = om.grid
    shape = (g.Nz, g.Ny, g.Nx)
    rho = C["rho"]
    wet = dict(qv=A["qv"], ql=A["ql"]) if moist else dict(q=A["q"])
    T = {k: {} for k in ("coriolis", "column", "energy", "relaxation", "field", "flux", "avg", "sub")}
    if S["f"]:
        T["coriolis"]["ru"], T["coriolis"]["rv"] = ref.coriolis(geo, S["f"], A["ru"], A["rv"], coriolis_two_point=on("coriolis_two_point"),
                                                                coriolis_same_sign=on("coriolis_same_sign"))
    for spec, key, static in (("u", "ru", C["Fu"]), ("v", "rv", C["Fv"]), ("theta", "rtheta", None), ("q", "rq", C["Fq"])):
        total = None
        if spec in S["subsidence"]:
            T["avg"][spec] = ref.horizontal_average(geo, A[spec])
            T["sub"][spec] = ref.subsidence_profile(geo, C["ws"], T["avg"][spec], subsidence_dzf_shift=on("subsidence_dzf_shift"),
                                                    subsidence_ends_halved=on("subsidence_ends_halved"))
            total = T["sub"][spec]
        if static is not None:
            total = np.asarray(static, dtype=LD) if total is None else total + np.asarray(static, dtype=LD)
        if total is not None:
            T["column"][key] = ref.column_term(geo, KIND[key], rho, total, shape)
    if C["Fe"] is not None:
        T["energy"]["rtheta"] = ref.energy_forcing(geo, rho, C["p_r"], PST, C["Fe"], c, energy_dry_constants=on("energy_dry_constants"), **wet)
    for key, (rate, target) in C["relax"].items():
        specific = not key.startswith("r")
        T["relaxation"]["r" + key if specific else key] = ref.relaxation(
            geo, KIND["r" + key if specific else key], rate, target, A[key], rho=rho if specific else None,
            relaxation_w_centre_density=on("relaxation_w_centre_density"))
    if C["F3"] is not None:
        T["field"]["rtheta"] = ref.field_forcing(geo, C["F3"], S["field_forcing"] == "theta", rho)
    dz = ref.bottom_dz(geo, LZ, bottom_dz_regular=on("bottom_dz_regular"))
    flat = shape[1:]
    if S["J_theta"]:
        T["flux"]["rtheta"] = ref.constant_flux(geo, S["J_theta"], flat, dz)
    if S["J_q"]:
        T["flux"]["rq"] = ref.constant_flux(geo, S["J_q"], flat, dz)
    if S["Q"]:
        T["flux"]["rtheta"] = ref.energy_flux(geo, S["Q"], c, dz, **wet)
    if S["drag"]:
        T["flux"]["ru"], T["flux"]["rv"] = ref.friction_drag(geo, S["drag"][0], S["drag"][1], A["ru"], A["rv"], dz,
                                                             drag_unaveraged_speed=on("drag_unaveraged_speed"))
    if S["bulk"]:
        B = ref.bulk_fluxes(geo, c, P0, PST, A["u"], A["v"], A["theta"], A["qv"] if moist else A["q"], dz,
                            bulk_square_of_mean=on("bulk_square_of_mean"), **S["bulk"])
        T["flux"].update({"r" + k: v for k, v in B.items()})
    return T


VOLUME_TERMS = ("coriolis", "column", "energy", "relaxation", "field")


def tendency_sum(T, field):
    """(sum of the volume terms the stack adds to G(field), m = the number of separate additions), or (None, 0)"""
    parts = [T[t][field] for t in VOLUME_TERMS if field in T[t]]
    if not parts:
        return None, 0
    total = parts[0]
    for p in parts[1:]:
        total = total + p
    return total, len(parts)


# ---- derived bounds of the device comparison (tests/test_forcing_device.py, section (b)) -----------------------------------------------------
FSLICES = 8


def sum_chain(name, path):
    """the longest chain of additions behind one horizontal sum of csrc/bz_forcing.hip.  "slices" (k_level_sums): a thread adds
    ceil(cells of its slice / 256) values, 8 tree levels, FSLICES slice sums in k_subsidence_profiles.  "waves" (k_level_wave_sums): 6 shuffle
    steps, then k_level_reduce over P = Ny ceil(Nx / 256) 4 slots: ceil(P / 256) strided adds and 8 tree levels, and the single partial sum
    of k_subsidence_profiles.  "numpy": the oracle's np.mean over (y, x) of the interior view — pairwise over a row (eight accumulators of at
    most 16 terms for blocks of 128, 3 levels to combine them, one level per doubling of the blocks), then row after row."""
    om = dry_state(name)
    Nx, Ny = om.grid.Nx, om.grid.Ny
    if path == "slices":
        rows = max((Ny * (s + 1)) // FSLICES - (Ny * s) // FSLICES for s in range(FSLICES))
        return -(-(rows * Nx) // 256) + 8 + FSLICES
    if path == "waves":
        P = Ny * (-(-Nx // 256)) * 4
        return 6 + -(-P // 256) + 8 + 1
    assert path == "numpy"
    return 16 + 3 + max(0, int(np.ceil(np.log2(max(Nx / 128.0, 1.0))))) + Ny


def device_sum_path(name, no_fuse_level_sums=False):
    return "waves" if dry_state(name).grid.Nx % 64 == 0 and not no_fuse_level_sums else "slices"


def subsidence_bound(name, stack_id, moist, spec, path, fields=None):
    """bound of the error that the rounding of the horizontal sums leaves in rho_r x (subsidence profile of `spec`): a mean is off by at most
    c 2^-53 mean|field|, a face value w_s (avg[k] - avg[k-1]) / dz_f by |w_s| / dz_f times twice that, a cell takes the mean of its two
    faces or its single face"""
    om = state(name, moist)
    geo, C = geometry(om), columns(name, stack_id)
    A = fields or state_fields(om)
    err_mean = sum_chain(name, path) * LD(2) ** -53 * np.abs(ref._at(geo, A[spec])).mean(dtype=LD)
    Nz, ws = geo.Nz, np.abs(np.asarray(C["ws"], dtype=LD))
    face = np.zeros(Nz + 1, dtype=LD)
    face[1:Nz] = ws[1:Nz] / geo.dzf_[1:Nz] * 2 * err_mean
    cell = np.array([face[k] if k == Nz - 1 else face[1] if k == 0 else (face[k] + face[k + 1]) / 2 for k in range(Nz)], dtype=LD)
    return float(np.max(np.asarray(C["rho"], dtype=LD) * cell))


def tendency_bound(name, stack_id, moist, field, T, G_max, path, fields=None):
    """|D - t| <= m 2^-53 max|G_forced| + 1e-13 max|t| (+ the subsidence part): (bound, its three parts)"""
    t, m = tendency_sum(T, field)
    spec = {"ru": "u", "rv": "v", "rtheta": "theta", "rq": "q"}.get(field)
    parts = (m * 2.0 ** -53 * G_max, 1e-13 * float(np.nanmax(np.abs(t))),
             subsidence_bound(name, stack_id, moist, spec, path, fields) if spec in STACKS[stack_id]["subsidence"] else 0.0)
    return sum(parts), parts


# ---- the same stack for oracle/forcings.py ----------------------------------------------------------------------------------------------------
def oracle_model(name, stack_id, moist, only=None):
    """an oracle model on the shared state carrying the stack; only: "coriolis" | "column" | "energy" | "flux" keeps that part of the column stack"""
    from oracle.forcings import BulkFluxes, ColumnForcings
    oracle, og = _oracle_grid(name)
    S, C, src = STACKS[stack_id], columns(name, stack_id), state(name, moist)
    keep = lambda part: only is None or only == part
    kw = {}
    if keep("coriolis"):
        kw["coriolis_f"] = S["f"]
    if keep("column"):
        kw.update(Fu=C["Fu"], Fv=C["Fv"], Fq=C["Fq"], w_subsidence=C["ws"], subsidence_on=S["subsidence"])
    if keep("energy"):
        kw["Fe"] = C["Fe"]
    if keep("flux"):
        kw.update(flux_theta=S["J_theta"], flux_q=S["J_q"], flux_energy=S["Q"])
        if S["drag"]:
            kw.update(drag_rho0_ustar2=S["drag"][0], drag_epsilon=S["drag"][1])
        if S["bulk"]:
            kw["bulk"] = BulkFluxes(P0, PST, **S["bulk"])
    m = oracle.OracleModel(og, potential_temperature=THETA0, microphysics="SaturationAdjustment" if moist else None, forcings=ColumnForcings(**kw))
    for n in STATE_ARRAYS:
        getattr(m, n)[...] = getattr(src, n)
    m.relaxation = dict(C["relax"]) or None
    m.field_forcing = (C["F3"], S["field_forcing"] == "theta") if C["F3"] is not None else None
    return m


# ---- the same stack for the device model -------------------------------------------------------------------------------------------------------
def device_grid(bz, name):
    size, kw = grid_arguments(name)
    kw["topology"] = tuple(getattr(bz, t) for t in kw["topology"])
    return bz.RectilinearGrid(size, **kw)


def device_model(bz, name, stack_id=None, moist=False):
    """AtmosphereModel on the grid with the stack attached (None: the unforced model of the same grid and microphysics)"""
    grid = device_grid(bz, name)
    dynamics = bz.AnelasticDynamics(bz.ReferenceState(grid, surface_pressure=P0, potential_temperature=THETA0))
    kw = dict(microphysics=bz.SaturationAdjustment(equilibrium=bz.WarmPhaseEquilibrium())) if moist else {}
    if stack_id is not None:
        kw.update(device_keywords(bz, name, stack_id))
    return bz.AtmosphereModel(grid, dynamics=dynamics, advection=bz.WENO(order=ORDER), **kw)


def device_keywords(bz, name, stack_id):
    S, C = STACKS[stack_id], columns(name, stack_id)
    forcing, bcs, kw = {}, {}, {}
    bottom = lambda cond: bz.FieldBoundaryConditions(bottom=cond)
    if S["f"]:
        kw["coriolis"] = bz.FPlane(f=S["f"])
    sub = bz.SubsidenceForcing(w_subsidence)
    geo = bz.geostrophic_forcings(u_geostrophic, v_geostrophic) if S["geostrophic"] else None
    for spec, key in (("u", "u"), ("v", "v"), ("theta", "θ"), ("q", "qᵉ")):
        items = []
        if spec in S["subsidence"]:
            items.append(sub)
        if geo is not None and spec in ("u", "v"):
            items.append(getattr(geo, spec))
        if spec == "q" and S["drying"]:
            items.append(bz.Forcing(drying))
        if items:
            forcing[key] = tuple(items)
    if S["cooling"]:
        forcing["e"] = bz.Forcing(cooling)
    host = {"ru": "ρu", "rv": "ρv", "rw": "ρw", "rtheta": "ρθ", "rq": "ρqᵛ", "u": "u", "v": "v", "w": "w"}
    for key, (_, target) in C["relax"].items():
        spec = key.lstrip("r")
        forcing[host[key]] = (bz.Relaxation(rate=1.0, mask=RATES[spec], target=target),)
    if C["F3"] is not None:
        k = "θ" if S["field_forcing"] == "theta" else "ρθ"
        forcing[k] = tuple(forcing.get(k, ())) + (bz.Forcing(C["F3"]),)
    if S["J_theta"]:
        bcs["ρθ"] = bottom(bz.FluxBoundaryCondition(S["J_theta"]))
    if S["J_q"]:
        bcs["ρqᵉ"] = bottom(bz.FluxBoundaryCondition(S["J_q"]))
    if S["Q"]:
        bcs["ρe"] = bottom(bz.FluxBoundaryCondition(S["Q"]))
    if S["drag"]:
        rho0_ustar2, eps = S["drag"]
        drag = bottom(bz.FluxBoundaryCondition(bz.FrictionVelocityDrag(RHO0, USTAR, epsilon=eps)))
        assert RHO0 * USTAR ** 2 == rho0_ustar2
        bcs["ρu"], bcs["ρv"] = drag, drag
    if S["bulk"]:
        B = S["bulk"]
        for k in ("ρu", "ρv"):
            bcs[k] = bottom(bz.BulkDrag(coefficient=B["drag"][0], gustiness=B["drag"][1], surface_temperature=B["drag"][2]))
        bcs["ρθ"] = bottom(bz.BulkSensibleHeatFlux(coefficient=B["heat"][0], gustiness=B["heat"][1], surface_temperature=B["heat"][2]))
        bcs["ρqᵉ"] = bottom(bz.BulkVaporFlux(coefficient=B["vapor"][0], gustiness=B["vapor"][1], surface_temperature=B["vapor"][2]))
    if forcing:
        kw["forcing"] = forcing
    if bcs:
        kw["boundary_conditions"] = bcs
    return kw
