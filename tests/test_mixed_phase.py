"""SaturationAdjustment(equilibrium = MixedPhaseEquilibrium()) on the device: the mixed-phase inversion (bz_mp_diagnose in k_thermo<true> and
k_project_diagnose<3>) over the parcel sweep of tests/mixed_phase_reference.py, the reference's known answers, tendencies and whole steps
against MixedPhaseOracleModel on every tier, and the switch back to the warm phase.

Judging of the sweep (mixed_phase_reference.judge64 / judge32, which call sar.judge64 / sar.judge32 unchanged; nothing of a bound comes
from the device): Float64 T within max(1e-13, 16 d80) relative, each of q^v, q^l, q^i within max(1e-15, 16 d80) absolute, d80 the restatement's
own float64-to-longdouble distance of the parcel's population and solver; clear parcels: q^l and q^i exact zeros and q^v the bits of q^t;
warm cloudy parcels: q^i an exact zero; all-ice parcels: q^l an exact zero; threshold parcels on either forced branch; theta = 0 exact;
knife-edge parcels skipped (at most 0.5 % of the cloudy ones, asserted on the CPU).  Float32 within 4 d32.
Tendencies after one update_state!: 1e-12 of each tendency's scale.  Three steps: 1e-9 of each field's scale (the project's tolerances for
anelastic whole steps), and 1e-12 between the tier the model picks and each other tier."""
import ctypes as C

import numpy as np
import pytest

import mixed_phase_reference as mpr
import saturation_adjustment_reference as sar
from helpers import PROG, assert_increments

pytestmark = pytest.mark.gpu
F64, F32 = np.float64, np.float32
A_SMALL, A_LARGE = sar.ANELASTIC_GRIDS
NAN = float("nan")
BZ_ERR_UNSUPPORTED = 2


def _microphysics(bz, solver=sar.DEFAULT_SOLVER):
    return bz.SaturationAdjustment(equilibrium=bz.MixedPhaseEquilibrium(freezing_temperature=mpr.TF, homogeneous_ice_nucleation_temperature=mpr.TH),
                                   solver=bz.SecantSolver(abstol=solver[0], maxiter=solver[1]))


def _sweep_model(bz, shape, solver=sar.DEFAULT_SOLVER, float_type=F64):
    Lz = sar.TALL_COLUMN
    grid = bz.RectilinearGrid(shape, halo=3, float_type=float_type, x=(0.0, 100.0 * shape[0]), y=(0.0, 100.0 * shape[1]), z=(0.0, float(Lz)))
    ref = bz.ReferenceState(grid, surface_pressure=sar.SURFACE_PRESSURE, potential_temperature=sar.THETA_0, standard_pressure=sar.PST)
    hm = bz.AtmosphereModel(grid, dynamics=bz.AnelasticDynamics(ref), advection=bz.WENO(order=5), microphysics=_microphysics(bz, solver))
    assert list(hm.microphysical_fields) == ["qᵛ", "qˡ", "qⁱ", "qᵉ"]
    p_r, rho_r = _columns(hm)
    if float_type is F64:            # the columns the sweep was realised on: the device's, bit for bit
        want_p, want_rho = sar.reference_column(shape[2], Lz)
        assert np.array_equal(p_r, want_p) and np.array_equal(rho_r, want_rho)
    return hm


def _columns(hm):
    rho, p = hm._ref_arrays[0], hm._ref_arrays[1]
    Hz, Nz = hm.grid.Hz, hm.grid.Nz
    return p[Hz:Hz + Nz].copy(), rho[Hz:Hz + Nz].copy()


def _plant(hm, case):
    """the case's arrays into the prognostic fields, every diagnostic the launch must write poisoned.  -> the arrays the device holds"""
    mu = hm.microphysical_fields
    fields = dict(rtheta=hm.potential_temperature_density, rq=hm.moisture_density)
    for n, f in fields.items():
        f.set_interior(case[n])
    for f in (hm.temperature, hm.specific_moisture, hm.potential_temperature, mu["qᵛ"], mu["qˡ"], mu["qⁱ"]):
        f.parent.fill_(NAN)
    return {n: f.interior.cpu().numpy() for n, f in fields.items()}


def _read(hm):
    hm.synchronize()
    mu = hm.microphysical_fields
    get = lambda f: f.interior.cpu().numpy()
    return dict(T=get(hm.temperature), q=get(hm.specific_moisture), theta=get(hm.potential_temperature), qv=get(mu["qᵛ"]), ql=get(mu["qˡ"]),
                qi=get(mu["qⁱ"]))


def _show(label, report, table, skipped=0):
    for name, row in report.items():
        d = table.get(name, (0.0,) * 4)
        print(f"MIXEDPARCELS {label} {name}: device T={row[0]:.1e} qv={row[1]:.1e} ql={row[2]:.1e} qi={row[3]:.1e} | restatement's own T={d[0]:.1e} "
              f"qv={d[1]:.1e} ql={d[2]:.1e} qi={d[3]:.1e}" + (f" | knife-edge skipped: {skipped}" if skipped else ""))


def _diagnose_sweep(bz, shape, solver=sar.DEFAULT_SOLVER, which=0):
    hm = _sweep_model(bz, shape, solver)
    case = mpr.mixed_case(shape, which)
    held = _plant(hm, case)
    for n, a in held.items():
        assert np.array_equal(a, case[n]), n
    bz.update_state_(hm, compute_tendencies=False)
    return hm, case, _read(hm)


SWEEPS = [(A_SMALL, s) for s in sar.SOLVERS] + [(A_LARGE, sar.DEFAULT_SOLVER)]


@pytest.mark.parametrize("shape,solver", SWEEPS, ids=[f"{s[0]}x{s[1]}x{s[2]}-secant{so[0]:g},{so[1]}" for s, so in SWEEPS])
def test_mixed_phase_diagnosis_over_the_sweep(bz, shape, solver):
    """update_state!(compute_tendencies = false): k_thermo<true>.  (66, 8, 12): a partly filled wavefront behind a full one in every row;
    (130, 9, 6): a 9-row ragged tile.  The small grid also runs the other solvers of sar.SOLVERS (maxiter = 0 and 2: the maxiter exit;
    abstol = 0: until the `valid` guard fires, every parcel judged whatever its iteration count)."""
    hm, case, dev = _diagnose_sweep(bz, shape, solver)
    want = mpr.restated(shape, F64, solver)
    table = mpr.d80(shape, solver)
    fails, report, skipped = mpr.judge64(dev, want, case.tag, table, mpr.restated(shape, F64, solver, "clear"), mpr.restated(shape, F64, solver, "cloudy"))
    _show(f"{shape} secant={solver}", report, table, skipped)
    assert not fails, fails
    assert np.array_equal(dev["q"], want["q"]) and np.array_equal(dev["theta"], want["theta"])
    mu = hm.microphysical_fields
    for f in (mu["qᵛ"], mu["qˡ"], mu["qⁱ"], hm.temperature):          # halos: the periodic images and the no-flux z cells of the interior values
        a, g = f.parent.cpu().numpy(), hm.grid
        assert np.array_equal(a[g.Hz:-g.Hz, g.Hy:-g.Hy, :g.Hx], a[g.Hz:-g.Hz, g.Hy:-g.Hy, g.Nx:g.Nx + g.Hx])
        assert np.array_equal(a[g.Hz:-g.Hz, :g.Hy, :], a[g.Hz:-g.Hz, g.Ny:g.Ny + g.Hy, :])
        assert np.array_equal(a[g.Hz - 1], a[g.Hz]) and np.array_equal(a[g.Hz + g.Nz], a[g.Hz + g.Nz - 1])


@pytest.mark.parametrize("shape", sar.ANELASTIC_GRIDS, ids=str)
def test_a_parcels_result_does_not_depend_on_its_wavefront(bz, shape):
    """the same parcels under two placements (the second shuffles every level): the same bits per parcel"""
    outs = []
    for which in (0, 1):
        _, case, dev = _diagnose_sweep(bz, shape, which=which)
        outs.append({n: mpr.by_parcel(case, dev[n]) for n in mpr.NAMES} | {"tag": mpr.by_parcel(case, case.tag)})
    assert np.array_equal(outs[0]["tag"], outs[1]["tag"])
    for n in mpr.NAMES:
        assert np.array_equal(outs[0][n], outs[1][n]), (n, int((outs[0][n] != outs[1][n]).sum()))


def test_float32_diagnosis_over_the_sweep(bz):
    import torch
    shape = A_LARGE
    hm = _sweep_model(bz, shape, float_type=F32)
    assert hm.temperature.parent.dtype == torch.float32 and hm.microphysical_fields["qⁱ"].parent.dtype == torch.float32
    case = mpr.mixed_case(shape)
    held = _plant(hm, case)
    bz.update_state_(hm, compute_tendencies=False)
    dev = _read(hm)
    p32, rho32 = _columns(hm)

    def diagnose(dtype, branch=None):
        return mpr.diagnose_mixed({n: a.astype(dtype) for n, a in held.items()}, p32.astype(dtype), rho32.astype(dtype), dtype, force_branch=branch)

    want32, want64 = diagnose(F32), diagnose(F64)
    fails, report, table = mpr.judge32(dev, want32, want64, case.tag, float(np.abs(want64["q"]).max()), diagnose(F64, "clear"), diagnose(F64, "cloudy"))
    print("MIXEDPARCELS f32", report, table)
    assert not fails, fails
    assert np.array_equal(dev["q"], want32["q"]) and np.array_equal(dev["theta"], want32["theta"])


@pytest.mark.parametrize("T,qt", mpr.KNOWN, ids=mpr.KNOWN_IDS)
def test_reference_known_answers(bz, T, qt):
    """the reference's known answers (test/saturation_adjustment.jl:150-239) on the smallest grid the constructor accepts, every cell holding
    the parcel: theta^li of the known (T, q) at the cell's own p_r; T, q^v, q^l, q^i come back within the reference's atol under its solver
    (SecantSolver(abstol = 1e-6)).  The lowest level is the reference's: 0.5 m above a 101325 Pa surface under theta_0 = 288 K."""
    shape = (3, 3, 3)
    grid = bz.RectilinearGrid(shape, halo=3, x=(0.0, 3.0), y=(0.0, 3.0), z=(0.0, 3.0))
    ref = bz.ReferenceState(grid, surface_pressure=mpr.KNOWN_P0, potential_temperature=mpr.KNOWN_THETA0)
    hm = bz.AtmosphereModel(grid, dynamics=bz.AnelasticDynamics(ref), advection=bz.WENO(order=5), microphysics=_microphysics(bz, (mpr.SOLVER_TOL, 20)))
    p_r, rho_r = _columns(hm)
    assert p_r[0] == sar.reference_column(1, 1.0, p0=mpr.KNOWN_P0, theta0=mpr.KNOWN_THETA0)[0][0]
    F = mpr.typed(F64)
    known = [F.known_answer(F64(T), F64(qt), F64(p), F64(ref.standard_pressure)) for p in p_r]
    theta = np.array([float(k[0]) for k in known])[:, None, None] * np.ones((3, 3, 3))
    _plant(hm, dict(rtheta=rho_r[:, None, None] * theta, rq=rho_r[:, None, None] * qt * np.ones((3, 3, 3))))
    bz.update_state_(hm, compute_tendencies=False)
    dev = _read(hm)
    for k in range(3):
        for name, want in zip(mpr.NAMES, (T,) + tuple(float(x) for x in known[k][1:])):
            assert np.abs(dev[name][k] - want).max() <= mpr.TEST_TOL, (k, name, dev[name][k].ravel()[0], want)
    if T == 300.0:
        assert np.all(dev["ql"] == 0) and np.all(dev["qi"] == 0)
    if T == 220.0:
        assert np.all(dev["ql"] == 0) and np.all(dev["qi"] > 0.009)
    if T == 253.15:
        assert np.all(dev["ql"] > 0.006) and np.all(dev["qi"] > 0.006)


# ---- tendencies and steps against MixedPhaseOracleModel ------------------------------------------------------------------------------------------
PBP, FLAT, PBB = ("Periodic", "Periodic", "Bounded"), ("Periodic", "Flat", "Bounded"), ("Periodic", "Bounded", "Bounded")


def _pair(oracle, bz, size, topology=PBP, halo=3, advection=5, tracers=0, float_type=F64, device=True, wide=False):
    """(MixedPhaseOracleModel, device model or None) on a 10 km deep domain under theta_0 = 300 K: the reference column crosses T^f near
    2.7 km and T^h near 6.8 km.  wide: the 20 km x 20 km extent of helpers.make_pair"""
    flat = topology == FLAT
    ext = dict(x=(-4e3, 4e3), z=(0.0, 10e3)) if flat else dict(x=(-4e3, 4e3), y=(-3e3, 3e3), z=(0.0, 10e3))
    if wide:
        ext = dict(x=(-10e3, 10e3), y=(-10e3, 10e3), z=(0.0, 10e3))
    og = oracle.Grid(size, topology=topology, halo=(halo, halo) if flat else (halo,) * 3, **ext)
    om = mpr.MixedPhaseOracleModel(og, potential_temperature=300.0, advection=f"WENO{advection}", tracers=tracers)
    if not device:
        return om, None
    grid = bz.RectilinearGrid(size, topology=tuple(getattr(bz, t) for t in topology), halo=(halo, halo) if flat else (halo,) * 3, float_type=float_type,
                              **ext)
    ref = bz.ReferenceState(grid, potential_temperature=300.0)
    hm = bz.AtmosphereModel(grid, dynamics=bz.AnelasticDynamics(ref), advection=bz.WENO(order=advection), microphysics=_microphysics(bz),
                            tracers=("a",) if tracers else ())
    return om, hm


def _bubble(og, amplitude=(1.5, 1.0)):
    """a smooth moist bubble in a column that is subsaturated near the ground, liquid below T^f, mixed between and all ice above T^h.
    amplitude: (of the theta bubble in kelvin, factor on the wind)"""
    amplitude, wind = amplitude
    x, y, z = og.nodes("ccc")
    Lx = 8e3
    r2 = (x / 2500.0) ** 2 + ((y / 2500.0) ** 2 if og.Ny > 1 else 0.0) + ((z - 4500.0) / 2500.0) ** 2
    shape = (og.Nz, og.Ny, og.Nx)
    qt = np.broadcast_to(0.019 * np.exp(-z / 2600.0) * (1.0 + 0.15 * np.exp(-r2) + 0.05 * np.sin(2 * np.pi * x / Lx)), shape).copy()
    th = np.broadcast_to(300.0 + 1.0e-4 * z + amplitude * np.exp(-r2), shape).copy()
    u = np.broadcast_to(wind * (3.0 + 1.0 * np.sin(2 * np.pi * x / Lx) * np.cos(np.pi * z / 10e3)), shape).copy()
    return dict(theta=th, qt=qt, u=u)


def _tracer(om, ic):
    g = om.grid
    return om.ref.density[g.Hz:g.Hz + g.Nz][:, None, None] * (1.0 + 0.5 * np.tanh(ic["theta"] - 300.5))


def _set_oracle(om, tracer=False, amplitude=(1.5, 1.0)):
    ic = _bubble(om.grid, amplitude)
    om.set(qt=ic["qt"], theta=ic["theta"], u=ic["u"], **({"rc0": _tracer(om, ic)} if tracer else {}))


def _set_device(om, hm, tracer=False, amplitude=(1.5, 1.0)):
    """the same state on the device model (the oracle model lends its grid nodes and reference density)"""
    ic = _bubble(om.grid, amplitude)
    if tracer:
        hm.tracers["a"].set_interior(_tracer(om, ic))
    hm.set(qᵗ=ic["qt"], θ=ic["theta"], u=ic["u"])


def _regimes(ql, qi):
    return bool(((ql > 0) & (qi == 0)).any()), bool(((ql > 0) & (qi > 0)).any()), bool(((qi > 0) & (ql == 0)).any()), bool(((ql == 0) & (qi == 0)).any())


@pytest.mark.parametrize("size", [(16, 8, 8), (66, 8, 12)], ids=str)
def test_tendencies_after_one_update_state_match_the_oracle(oracle, bz, size):
    """update_state! on the oracle's prognostic state, halos included: T, q^v, q^l, q^i (halo images too) and every tendency; G_rho_w is
    where the buoyancy sees the ice loading.  The state is helpers.randomize's (seeded smooth + rough perturbations of every prognostic
    field on the grid of helpers.make_pair, what tests/test_gpu_parity.py holds the dry tendencies to 1e-12 with): up to 12 g/kg of moisture
    at every height of a 10 km column is clear near the ground, liquid, mixed and all ice above."""
    from helpers import push_state, randomize, relerr
    om, hm = _pair(oracle, bz, size, wide=True)
    randomize(om, seed=11, amp_q=1.2e-2)
    om.compute_tendencies()
    push_state(om, hm, names=("ru", "rv", "rw", "rtheta", "rq"))
    for k in hm.G.values():
        k.parent.fill_(NAN)
    bz.update_state_(hm, compute_tendencies=True)
    hm.synchronize()
    g, mu = om.grid, hm.microphysical_fields
    assert all(_regimes(g.interior(om.ql_liquid), g.interior(om.qi)))
    assert relerr(hm.temperature.cpu(), om.T) < 1e-13
    for name, want in (("qᵛ", om.qv), ("qˡ", om.ql_liquid), ("qⁱ", om.qi)):
        assert np.abs(mu[name].cpu() - want).max() < 1e-15, name          # parents: halos included
    for n, k in PROG.items():
        zf = n == "rw"
        want, got = g.interior(om.G[n], zface=zf), hm.G[k].interior_cpu()
        if zf:
            want, got = want[1:-1], got[1:-1]
        err = relerr(got, want)
        print(f"MIXEDTENDENCY {size} {n}: {err:.2e}")
        assert err < 1e-12, (n, err)


def _fields(hm, tracer=False):
    mu = hm.microphysical_fields
    out = {n: hm.prognostic_fields()[k].interior_cpu().astype(np.float64) for n, k in PROG.items()}
    out.update(T=hm.temperature.interior_cpu().astype(np.float64), qv=mu["qᵛ"].interior_cpu().astype(np.float64),
               ql=mu["qˡ"].interior_cpu().astype(np.float64), qi=mu["qⁱ"].interior_cpu().astype(np.float64))
    if tracer:
        out["rc0"] = hm.tracers["a"].interior_cpu().astype(np.float64)
    return out


def _oracle_fields(om, tracer=False):
    g = om.grid
    out = {n: np.array(g.interior(getattr(om, n), n == "rw")) for n in PROG}
    out.update(T=np.array(g.interior(om.T)), qv=np.array(g.interior(om.qv)), ql=np.array(g.interior(om.ql_liquid)), qi=np.array(g.interior(om.qi)))
    if tracer:
        out["rc0"] = np.array(g.interior(om.rc0))
    return out


def _scaled_errors(got, want):
    mom = max(np.abs(want[n]).max() for n in ("ru", "rv", "rw"))
    scale = lambda n: mom if n in ("ru", "rv", "rw") else max(np.abs(want[n]).max(), 1e-3 if n in ("rq", "rtheta", "T", "rc0") else 1e-6)
    return {n: float(np.abs(got[n] - want[n]).max() / scale(n)) for n in want}


TIERS = {"picked": {}, "BZ_NO_FUSE_RK": {"BZ_NO_FUSE_RK": "1"}, "BZ_NO_FUSED": {"BZ_NO_FUSED": "1"}}
DT, STEPS = 2.0, 3
_ORACLE_RUNS = {}


def _oracle_run(oracle, key, size, **kw):
    """three steps of the oracle, once per set-up"""
    if key not in _ORACLE_RUNS:
        amplitude = kw.pop("amplitude", (1.5, 1.0))
        om, _ = _pair(oracle, None, size, device=False, **kw)
        _set_oracle(om, bool(kw.get("tracers")), amplitude)
        start = _oracle_fields(om, bool(kw.get("tracers")))
        for _ in range(STEPS):
            om.time_step(DT)
        _ORACLE_RUNS[key] = (start, _oracle_fields(om, bool(kw.get("tracers"))))
    return _ORACLE_RUNS[key]


def _device_run(oracle, bz, monkeypatch, size, env, graph=False, **kw):
    for name in ("BZ_NO_FUSE_RK", "BZ_NO_FUSED"):          # set before the context is created
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    amplitude = kw.pop("amplitude", (1.5, 1.0))
    om, hm = _pair(oracle, bz, size, **kw)
    _set_device(om, hm, bool(kw.get("tracers")), amplitude)
    if graph:
        hm.graph_enable(True)
    else:                            # (a profiled step is not recorded: the kernel table's events sit between its launches)
        hm.profile_enable(True)
        hm.profile_reset()
    for _ in range(STEPS + (3 if graph else 0)):
        hm.time_step(DT)
    hm.synchronize()
    return hm, _fields(hm, bool(kw.get("tracers")))


def _assert_steps(label, got, want, tol):
    errs = _scaled_errors(got, want)
    print(f"MIXEDSTEPS {label}:", " ".join(f"{n}={e:.1e}" for n, e in errs.items()))
    assert all(e < tol for e in errs.values()), (label, {k: f"{v:.1e}" for k, v in errs.items()})


@pytest.mark.parametrize("size", [(64, 16, 12), (66, 9, 9)], ids=["whole-tiles", "ragged"])
def test_three_steps_match_the_oracle_on_every_tier(oracle, bz, monkeypatch, size):
    """three steps of the moist bubble: the tier the model picks within 1e-9 of MixedPhaseOracleModel, each other tier (BZ_NO_FUSE_RK,
    BZ_NO_FUSED) within 1e-12 of the picked one; liquid-only, mixed, ice-only and clear cells are all present at the end"""
    start, want = _oracle_run(oracle, ("pbp", size), size)
    runs = {}
    for tier, env in TIERS.items():
        hm, runs[tier] = _device_run(oracle, bz, monkeypatch, size, env)
        print(f"MIXEDSTEPS {size} {tier} slots:", {k: v[1] for k, v in hm.profile().items()})
    assert all(_regimes(runs["picked"]["ql"], runs["picked"]["qi"])), _regimes(runs["picked"]["ql"], runs["picked"]["qi"])
    assert not np.array_equal(want["rw"], start["rw"])
    _assert_steps(f"{size} picked vs oracle", runs["picked"], want, 1e-9)
    for tier in ("BZ_NO_FUSE_RK", "BZ_NO_FUSED"):
        _assert_steps(f"{size} {tier} vs picked", runs[tier], runs["picked"], 1e-12)


@pytest.mark.parametrize("size,topology", [((64, 12), FLAT), ((16, 8, 8), PBB)], ids=["flat-y", "walls-in-y"])
def test_three_steps_on_the_operators_tier_topologies(oracle, bz, monkeypatch, size, topology):
    """(Periodic, Flat, Bounded) and (Periodic, Bounded, Bounded): k_thermo<true>, the halo fill with q^i and the per-operator z-momentum kernels"""
    start, want = _oracle_run(oracle, (topology, size), size, topology=topology)
    hm, got = _device_run(oracle, bz, monkeypatch, size, {}, topology=topology)
    slots = {k: v[1] for k, v in hm.profile().items()}
    print(f"MIXEDSTEPS {size} {topology} slots:", slots)
    assert slots.get("project_and_diagnose", 0) == 0 and slots.get("compute_auxiliary_thermodynamic_variables", 0) > 0
    assert all(_regimes(got["ql"], got["qi"]))
    _assert_steps(f"{size} {topology[1]} vs oracle", got, want, 1e-9)


def test_three_steps_with_a_tracer(oracle, bz, monkeypatch):
    size = (64, 16, 12)
    start, want = _oracle_run(oracle, ("tracer", size), size, tracers=1)
    hm, got = _device_run(oracle, bz, monkeypatch, size, {}, tracers=1)
    assert not np.array_equal(want["rc0"], start["rc0"]) and all(_regimes(got["ql"], got["qi"]))
    _assert_steps("tracer vs oracle", got, want, 1e-9)


def test_three_steps_with_weno9(oracle, bz, monkeypatch):
    size = (32, 16, 12)
    start, want = _oracle_run(oracle, ("weno9", size), size, advection=9, halo=5)
    hm, got = _device_run(oracle, bz, monkeypatch, size, {}, advection=9, halo=5)
    assert all(_regimes(got["ql"], got["qi"]))
    _assert_steps("WENO9 halo 5 vs oracle", got, want, 1e-9)


def test_graph_replay_is_bit_identical(oracle, bz, monkeypatch):
    size = (64, 16, 12)
    a, fa = _device_run(oracle, bz, monkeypatch, size, {}, graph=True)
    info = a.graph_info()
    assert info[0] and info[1] == 1 and info[2] >= 1, info
    b, fb = _device_run(oracle, bz, monkeypatch, size, {}, graph=False)
    for _ in range(3):
        b.time_step(DT)
    b.synchronize()
    fb = _fields(b)
    for n in fa:
        assert np.isfinite(fa[n]).all() and np.array_equal(fa[n], fb[n]), n
    assert all(_regimes(fa["ql"], fa["qi"]))


def test_float32_three_steps_judged_by_their_increments(oracle, bz, monkeypatch):
    """Float32 against the Float64 oracle by increment_error and F32_INCREMENT_TOL["anelastic"], as the other Float32 step tests.  The bubble
    is a 10 K one, as in those tests (tests/f32_cases.py: bubble(dtheta = 10)), in twice the wind: the measure divides by what three steps move a field, and
    storing rho theta ~ 350 in Float32 costs 1.5e-5 a time whatever the state: under the 1.5 K bubble of the Float64 tests three steps move
    rho theta by 0.01 only, and the rounding of the stores alone is 1e-2 of that (measured: 9.8e-3), which says nothing about the scheme."""
    size = (64, 16, 12)
    start, want = _oracle_run(oracle, ("pbp-10K", size), size, amplitude=(10.0, 2.0))
    hm, got = _device_run(oracle, bz, monkeypatch, size, {}, float_type=F32, amplitude=(10.0, 2.0))
    names = ("ru", "rv", "rw", "rtheta", "rq", "T")
    assert_increments("mixed-phase bubble", {n: got[n] for n in names}, {n: want[n] for n in names}, {n: start[n] for n in names}, "anelastic")
    assert all(_regimes(got["ql"], got["qi"]))


# ---- switching and the C entry point's refusals -----------------------------------------------------------------------------------------------------
def test_back_to_the_warm_phase_steps_like_a_fresh_warm_model(oracle, bz, monkeypatch):
    """bz_set_mixed_phase_equilibrium(NULL) on a context that had the mixed phase attached: three steps bit-identical to a model built
    with WarmPhaseEquilibrium()"""
    size = (64, 16, 12)
    for name in ("BZ_NO_FUSE_RK", "BZ_NO_FUSED"):
        monkeypatch.delenv(name, raising=False)
    om, hm = _pair(oracle, bz, size)
    hm._check(hm._lib.bz_set_mixed_phase_equilibrium(hm._ctx, None, None), "bz_set_mixed_phase_equilibrium")
    grid = hm.grid
    warm = bz.AtmosphereModel(grid, dynamics=bz.AnelasticDynamics(bz.ReferenceState(grid, potential_temperature=300.0)), advection=bz.WENO(order=5),
                              microphysics=bz.SaturationAdjustment(equilibrium=bz.WarmPhaseEquilibrium()))
    hm.microphysical_fields["qⁱ"].parent.fill_(NAN)          # nothing reads or writes it any more
    outs = []
    for m in (hm, warm):
        _set_device(om, m)
        for _ in range(STEPS):
            m.time_step(DT)
        m.synchronize()
        outs.append({k: f.interior_cpu() for k, f in m.prognostic_fields().items()} |
                    {"T": m.temperature.interior_cpu(), "ql": m.microphysical_fields["qˡ"].interior_cpu(), "qv": m.microphysical_fields["qᵛ"].interior_cpu()})
    for k in outs[0]:
        assert np.array_equal(outs[0][k], outs[1][k]), k
    assert (outs[0]["ql"] > 0).any() and np.isnan(hm.microphysical_fields["qⁱ"].parent.cpu().numpy()).all()


def test_the_entry_point_refuses_what_it_does_not_run(bz):
    grid = bz.RectilinearGrid((16, 8, 8), x=(0, 1600.0), y=(0, 800.0), z=(0, 8e3))
    warm = bz.SaturationAdjustment(equilibrium=bz.WarmPhaseEquilibrium())
    dyn = bz.CompressibleDynamics(bz.SplitExplicitTimeDiscretization(substeps=6))
    cm = bz.CompressibleAtmosphereModel(grid, dyn, advection=bz.WENO(order=5), microphysics=warm)
    dry = bz.AtmosphereModel(grid, advection=bz.WENO(order=5))
    P = cm._T.bz_mixed_phase_equilibrium(mpr.TF, mpr.TH, 2834000.0, 2108.0)
    for m, word in ((cm, "CompressibleDynamics"), (dry, "SaturationAdjustment")):
        buf = m.temperature          # any device array of the grid's size stands in for q^i: the call must refuse before it keeps it
        rc = m._lib.bz_set_mixed_phase_equilibrium(m._ctx, C.byref(P), C.c_void_p(buf.ptr()))
        assert rc == BZ_ERR_UNSUPPORTED, rc
        text = m._lib.bz_last_error(m._ctx).decode()
        assert "bz_set_mixed_phase_equilibrium" in text and word in text, text
