"""BulkMicrophysics(negative_moisture_correction = VerticalBorrowing() | SpeciesBorrowing(...)) on the device.

The kernel alone (fix_negative_moisture_, k_fix_negative_moisture of csrc/bz_negative_moisture.hip) against the typed restatement of
tests/negative_moisture_reference.py, BIT FOR BIT, in Float64 and on Float32 grids: the operations are correctly rounded and uncontracted,
so a bit mismatch is a defect, not a tolerance.  Its placement in a step against the corrected oracle models (nmr.corrected): the tier the
model picks within 1e-9 of each field's scale, the other tiers within 1e-12 of the picked one (the standing tolerances of
tests/test_mixed_phase.py), the launch count of the profile slot, hipGraph replay and many_time_steps_ bit-identical to single steps,
Float32 by increments.  Equivalences that must hold to the bit, and the C entry point's refusals."""
import ctypes as C

import numpy as np
import pytest

import negative_moisture_reference as nmr
from helpers import PROG, assert_increments

pytestmark = pytest.mark.gpu
F64, F32 = np.float64, np.float32
NAN = float("nan")
BZ_ERR_INVALID, BZ_ERR_UNSUPPORTED = 1, 2
DT, STEPS = nmr.DT, nmr.STEPS
SLOT = "fix_negative_moisture"


# ---- the kernel alone ------------------------------------------------------------------------------------------------------------------------------
def _kernel_model(bz, Nx, Ny, Nz, dtype, correction="vertical"):
    """a warm-phase model on a stretched z (Ny = 1: Flat y) whose context runs the kernel; -> (model, rho_r, dz in the grid's precision)"""
    zf = nmr.stretched_faces(Nz)
    if Ny == 1:
        grid = bz.RectilinearGrid((Nx, Nz), topology=(bz.Periodic, bz.Flat, bz.Bounded), halo=(3, 3), float_type=dtype, x=(0.0, 100.0 * Nx), z=zf)
    else:
        grid = bz.RectilinearGrid((Nx, Ny, Nz), halo=3, float_type=dtype, x=(0.0, 100.0 * Nx), y=(0.0, 100.0 * Ny), z=zf)
    nmc = {"vertical": bz.VerticalBorrowing(), "species": bz.SpeciesBorrowing(), "both": bz.SpeciesBorrowing(vertical_borrowing=bz.VerticalBorrowing())}[correction]
    hm = bz.AtmosphereModel(grid, dynamics=bz.AnelasticDynamics(bz.ReferenceState(grid, potential_temperature=300.0)), advection=bz.WENO(order=5),
                            microphysics=bz.BulkMicrophysics(cloud_formation=bz.SaturationAdjustment(equilibrium=bz.WarmPhaseEquilibrium()),
                                                             negative_moisture_correction=nmc))
    assert isinstance(hm.microphysics, bz.BulkMicrophysics) and list(hm.microphysical_fields) == ["qᵛ", "qˡ", "qᵉ"]
    rho, dz = nmr.device_columns(hm)
    assert dz.dtype == dtype and np.array_equal(dz.astype(F64), np.diff(zf))          # dyadic spacings: exact in both precisions
    return hm, rho, dz


def _plant(field, interior):
    """the interior into a field whose halo cells are NaN"""
    field.parent.fill_(NAN)
    field.set_interior(interior)
    got = field.interior.cpu().numpy()
    assert nmr.same_bits(got, interior)
    return got


def _halo_is_nan(field):
    a = field.parent.cpu().numpy().copy()
    a[field.grid.interior_slices(False)] = NAN
    return bool(np.isnan(a).all())


NX_NY = [(nx, ny) for nx in (5, 64, 65, 130) for ny in (1, 3)]
NZS = (3, 4, 9, 10, 12, 18)          # NMC_U = 8 levels per batch above the two bottom ones: no batch, one exactly, one and a remainder, two exactly


@pytest.mark.parametrize("dtype", [F64, F32], ids=["Float64", "Float32"])
@pytest.mark.parametrize("Nx,Ny", NX_NY, ids=[f"{a}x{b}" for a, b in NX_NY])
def test_vertical_borrowing_is_the_restatement_bit_for_bit(bz, Nx, Ny, dtype):
    """every population of nmr.POPULATIONS in one field, at every column length; halos poisoned: nothing of them reaches the interior, and
    the kernel writes none of them"""
    for Nz in NZS:
        hm, rho, dz = _kernel_model(bz, Nx, Ny, Nz, dtype)
        field, tag = nmr.populations((Nz, Ny, Nx), rho, dtype, seed=Nz)
        held = _plant(hm.moisture_density, field)
        hm.profile_enable(True)
        hm.profile_reset()
        bz.fix_negative_moisture_(hm)
        hm.synchronize()
        got = hm.moisture_density.interior.cpu().numpy()
        want = nmr.fix_negative_moisture(held.copy(), rho, dz, vertical=True)
        bad = ~((got == want) | (np.isnan(got) & np.isnan(want)))
        assert nmr.same_bits(got, want), (Nz, int(bad.sum()), [nmr.POPULATIONS[t] for t in np.unique(tag[bad.any(axis=0)])])
        assert _halo_is_nan(hm.moisture_density)
        assert hm.profile()[SLOT][1] == 1
        positive = tag == nmr.POPULATIONS.index("positive")
        assert nmr.same_bits(got[:, positive], held[:, positive])
        ok = ~np.isnan(held).any(axis=0)
        m0, m1 = nmr.column_mass(held, dz)[0], nmr.column_mass(got, dz)[0]
        assert np.all(np.abs(m1 - m0)[ok] <= nmr.conservation_bound(held, dz)[ok])
        if Nx >= 12:
            assert not nmr.same_bits(got, held)


def _species_fields(bz, hm, n):
    from breeze_jl_amd.model import Field
    return [Field(hm.grid, hm.moisture_density.loc, hm.device) for _ in range(n)]


def _attach(hm, species, vertical, mass=(), pairs=(), clamp=()):
    d = hm._T.bz_negative_moisture_correction()
    d.species_borrowing, d.vertical_borrowing = int(species), int(vertical)
    d.n_mass, d.n_pairs, d.n_clamp = len(mass), len(pairs), len(clamp)
    for a, f in enumerate(mass):
        d.mass[a] = f.ptr()
    for a, (n, m) in enumerate(pairs):
        d.number[a], d.pair_mass[a] = n.ptr(), m.ptr()
    for a, f in enumerate(clamp):
        d.clamp[a] = f.ptr()
    return hm._lib.bz_set_negative_moisture_correction(hm._ctx, C.byref(d))


@pytest.mark.parametrize("dtype", [F64, F32], ids=["Float64", "Float32"])
@pytest.mark.parametrize("vertical", [False, True], ids=["species-only", "species+vertical"])
@pytest.mark.parametrize("Nx,Ny,Nz", [(65, 3, 9), (130, 1, 12)], ids=str)
def test_species_chains_with_pairs_and_a_clamp_list(bz, Nx, Ny, Nz, vertical, dtype):
    """chains of length 0, 1 and 2 (rain <- cloud <- moisture), the (number, mass) pairs of both species, both numbers clamped, a number
    paired with an array outside the chain; the restatement's bits in every array, NaN halos untouched"""
    hm, rho, dz = _kernel_model(bz, Nx, Ny, Nz, dtype, "both" if vertical else "species")
    rng = np.random.default_rng(Nx + Nz)
    shape = (Nz, Ny, Nx)
    rain, cloud, n_rain, n_cloud, other, n_other = _species_fields(bz, hm, 6)
    for length in (0, 1, 2):
        rq0, _ = nmr.populations(shape, rho, dtype, seed=7 + length)
        make = lambda lo: ((rng.random(shape) - lo) * 4e-3 * rho[:, None, None]).astype(dtype)
        start = dict(rain=make(0.5), cloud=make(0.3), n_rain=make(0.2) * dtype(1e9), n_cloud=make(0.5) * dtype(1e9), other=make(0.5), n_other=make(0.1))
        start["cloud"][Nz // 2, :, ::7] = NAN          # a NaN species cell
        start["rain"][0, :, ::5] = -0.0
        fields = dict(rain=rain, cloud=cloud, n_rain=n_rain, n_cloud=n_cloud, other=other, n_other=n_other)
        held = {k: _plant(fields[k], v) for k, v in start.items()}
        held["rq"] = _plant(hm.moisture_density, rq0)
        mass = {0: (), 1: ("cloud",), 2: ("rain", "cloud")}[length]
        pairs = {0: (("n_other", "other"),), 1: (("n_cloud", "cloud"), ("n_other", "other")), 2: (("n_rain", "rain"), ("n_cloud", "cloud"))}[length]
        clamp = {0: ("n_other",), 1: ("n_cloud",), 2: ("n_rain", "n_cloud", "n_other")}[length]
        rc = _attach(hm, True, vertical, [fields[m] for m in mass], [(fields[n], fields[m]) for n, m in pairs], [fields[c] for c in clamp])
        assert rc == 0, hm._lib.bz_last_error(hm._ctx).decode()
        bz.fix_negative_moisture_(hm)
        hm.synchronize()
        want = {k: v.copy() for k, v in held.items()}
        nmr.fix_negative_moisture(want["rq"], rho, dz, species=True, vertical=vertical, mass=[want[m] for m in mass],
                                  pairs=[(want[n], want[m]) for n, m in pairs], numbers=[want[c] for c in clamp])
        fields["rq"] = hm.moisture_density
        for k, f in fields.items():
            got = f.interior.cpu().numpy()
            assert nmr.same_bits(got, want[k]), (length, k, int((~((got == want[k]) | (np.isnan(got) & np.isnan(want[k])))).sum()))
            assert _halo_is_nan(f), (length, k)
        changed = [k for k in want if not nmr.same_bits(want[k], held[k])]
        assert set(changed) >= set(mass) | {n for n, _ in pairs}, (length, changed)
        if length:          # what a species takes leaves the next one at the same level: the level sum of the chain stays
            s_mass = [held[m].copy() for m in mass]
            s_rq = nmr.fix_negative_moisture(held["rq"].copy(), rho, dz, species=True, mass=s_mass)
            before = held["rq"].astype(F64) + sum(held[m].astype(F64) for m in mass)
            after = s_rq.astype(F64) + sum(x.astype(F64) for x in s_mass)
            finite = np.isfinite(before) & np.isfinite(after)
            assert np.all(np.abs(after - before)[finite] <= 8 * np.finfo(dtype).eps * np.abs(before[finite]).max())
        fields.pop("rq")


# ---- placement in a step ------------------------------------------------------------------------------------------------------------------------------
def _saturation_adjustment(bz, phase):
    return bz.SaturationAdjustment(equilibrium=bz.MixedPhaseEquilibrium() if phase == "mixed" else bz.WarmPhaseEquilibrium())


def _device_model(bz, size, phase, correction="vertical", topology=nmr.PBP, tracers=0, float_type=F64):
    flat = topology == nmr.FLAT
    grid = bz.RectilinearGrid(size, topology=tuple(getattr(bz, t) for t in topology), halo=(3, 3) if flat else (3, 3, 3), float_type=float_type,
                              **nmr.extent(topology))
    sa = _saturation_adjustment(bz, phase)
    micro = {"bare": lambda: sa, "none": lambda: bz.BulkMicrophysics(cloud_formation=sa),
             "species": lambda: bz.BulkMicrophysics(cloud_formation=sa, negative_moisture_correction=bz.SpeciesBorrowing()),
             "vertical": lambda: bz.BulkMicrophysics(cloud_formation=sa, negative_moisture_correction=bz.VerticalBorrowing()),
             "both": lambda: bz.BulkMicrophysics(cloud_formation=sa, negative_moisture_correction=bz.SpeciesBorrowing(bz.VerticalBorrowing()))}[correction]()
    return bz.AtmosphereModel(grid, dynamics=bz.AnelasticDynamics(bz.ReferenceState(grid, potential_temperature=300.0)), advection=bz.WENO(order=5),
                              microphysics=micro, tracers=("a",) if tracers else ())


def _set_device(hm, om, ic):
    if hm.tracers:
        hm.tracers["a"].set_interior(nmr.tracer_density(om, ic))
    hm.set(qᵗ=ic["qt"], θ=ic["theta"], u=ic["u"])


def _fields(hm):
    mu = hm.microphysical_fields
    out = {n: hm.prognostic_fields()[k].interior_cpu().astype(F64) for n, k in PROG.items()}
    out.update(T=hm.temperature.interior_cpu().astype(F64), qv=mu["qᵛ"].interior_cpu().astype(F64), ql=mu["qˡ"].interior_cpu().astype(F64))
    if "qⁱ" in mu:
        out["qi"] = mu["qⁱ"].interior_cpu().astype(F64)
    if hm.tracers:
        out["rc0"] = hm.tracers["a"].interior_cpu().astype(F64)
    return out


def _raw(hm):
    """every field the steps write, in the grid's precision, parents (halos included)"""
    out = {k: f.cpu() for k, f in hm.prognostic_fields().items()}
    out.update({k: f.cpu() for k, f in hm.microphysical_fields.items()}, T=hm.temperature.cpu())
    return out


def _oracle_fields(om, phase):
    g = om.grid
    out = {n: np.array(g.interior(getattr(om, n), n == "rw")) for n in PROG}
    out.update(T=np.array(g.interior(om.T)), qv=np.array(g.interior(om.qv)))
    if phase == "mixed":
        out.update(ql=np.array(g.interior(om.ql_liquid)), qi=np.array(g.interior(om.qi)))
    else:
        out.update(ql=np.array(g.interior(om.ql)))
    if om.n_tracers:
        out["rc0"] = np.array(g.interior(om.rc0))
    return out


def _scaled_errors(got, want):
    mom = max(np.abs(want[n]).max() for n in ("ru", "rv", "rw"))
    scale = lambda n: mom if n in ("ru", "rv", "rw") else max(np.abs(want[n]).max(), 1e-3 if n in ("rq", "rtheta", "T", "rc0") else 1e-6)
    return {n: float(np.abs(got[n] - want[n]).max() / scale(n)) for n in want}


def _assert_steps(label, got, want, tol):
    errs = _scaled_errors(got, want)
    print(f"NMCSTEPS {label}:", " ".join(f"{n}={e:.1e}" for n, e in errs.items()))
    assert all(e < tol for e in errs.values()), (label, {k: f"{v:.1e}" for k, v in errs.items()})


_ORACLE_RUNS = {}


def _oracle_run(oracle, size, phase, topology=nmr.PBP, tracers=0, **bubble):
    """(the oracle model, the initial condition, start fields, fields after STEPS steps) of the corrected oracle, once per set-up"""
    key = (size, phase, topology, tracers, tuple(sorted(bubble.items())))
    if key not in _ORACLE_RUNS:
        om = nmr.oracle_model(oracle, size, phase, topology=topology, tracers=tracers)
        built = len(om.negative_cells)
        ic = nmr.set_oracle(om, bool(tracers), **bubble)
        start = _oracle_fields(om, phase)
        for _ in range(STEPS):
            om.time_step(DT)
        assert min(om.negative_cells[built:]) >= 1
        _ORACLE_RUNS[key] = (om, ic, start, _oracle_fields(om, phase))
    return _ORACLE_RUNS[key]


TIERS = {"picked": {}, "BZ_NO_FUSE_RK": {"BZ_NO_FUSE_RK": "1"}, "BZ_NO_FUSED": {"BZ_NO_FUSED": "1"}}


def _device_run(bz, monkeypatch, om, ic, size, phase, env=None, steps=STEPS, graph=False, **kw):
    for name in ("BZ_NO_FUSE_RK", "BZ_NO_FUSED"):          # read when the context is created
        monkeypatch.delenv(name, raising=False)
    for name, value in (env or {}).items():
        monkeypatch.setenv(name, value)
    hm = _device_model(bz, size, phase, **kw)
    hm.profile_enable(True)
    hm.profile_reset()
    _set_device(hm, om, ic)
    hm.synchronize()
    set_launches = hm.profile().get(SLOT, (0.0, 0))[1]
    if graph:
        hm.profile_enable(False)          # (a profiled step is not recorded: the kernel table's events sit between its launches)
        hm.graph_enable(True)
    else:
        hm.profile_reset()
    for _ in range(steps):
        hm.time_step(DT)
    hm.synchronize()
    return hm, set_launches


@pytest.mark.parametrize("phase", ["warm", "mixed"])
@pytest.mark.parametrize("size", [(64, 16, 12), (66, 9, 9)], ids=["whole-tiles", "ragged"])
def test_three_steps_match_the_corrected_oracle_on_every_tier(oracle, bz, monkeypatch, size, phase):
    """the tier the model picks within 1e-9 of the corrected oracle, each other tier within 1e-12 of the picked one; the slot counts one
    launch per update_state! of the reference: two in set! (before and after the mass-conserving projection), one in the first step's
    maybe_prepare_first_time_step, three per step"""
    om, ic, start, want = _oracle_run(oracle, size, phase)
    runs = {}
    for tier, env in TIERS.items():
        hm, set_launches = _device_run(bz, monkeypatch, om, ic, size, phase, env)
        slots = {k: v[1] for k, v in hm.profile().items()}
        print(f"NMCSTEPS {size} {phase} {tier} slots:", slots)
        assert set_launches == 2 and slots[SLOT] == 1 + 3 * STEPS, (tier, set_launches, slots)
        if tier == "picked":
            assert slots.get("project_and_diagnose", 0) > 0 and slots.get("compute_auxiliary_thermodynamic_variables", 0) <= 1, slots
        runs[tier] = _fields(hm)
    assert not np.array_equal(want["rq"], start["rq"]) and (runs["picked"]["ql"] > 0).any()
    _assert_steps(f"{size} {phase} picked vs oracle", runs["picked"], want, nmr.STEP_TOL)
    for tier in ("BZ_NO_FUSE_RK", "BZ_NO_FUSED"):
        _assert_steps(f"{size} {phase} {tier} vs picked", runs[tier], runs["picked"], nmr.TIER_TOL)


@pytest.mark.parametrize("size,topology,phase", [((64, 12), nmr.FLAT, "warm"), ((16, 8, 8), nmr.PBB, "mixed")], ids=["flat-y", "walls-in-y"])
def test_three_steps_on_the_operators_tier_topologies(oracle, bz, monkeypatch, size, topology, phase):
    om, ic, start, want = _oracle_run(oracle, size, phase, topology=topology)
    hm, set_launches = _device_run(bz, monkeypatch, om, ic, size, phase, topology=topology)
    slots = {k: v[1] for k, v in hm.profile().items()}
    print(f"NMCSTEPS {size} {topology} slots:", slots)
    assert slots.get("project_and_diagnose", 0) == 0 and set_launches == 2 and slots[SLOT] == 1 + 3 * STEPS, slots
    _assert_steps(f"{size} {topology[1]} vs oracle", _fields(hm), want, nmr.STEP_TOL)


def test_three_steps_with_a_tracer(oracle, bz, monkeypatch):
    size = (64, 16, 12)
    om, ic, start, want = _oracle_run(oracle, size, "warm", tracers=1)
    hm, _ = _device_run(bz, monkeypatch, om, ic, size, "warm", tracers=1)
    assert hm.profile()[SLOT][1] == 1 + 3 * STEPS and not np.array_equal(want["rc0"], start["rc0"])
    _assert_steps("tracer vs oracle", _fields(hm), want, nmr.STEP_TOL)


def test_graph_replay_is_bit_identical(oracle, bz, monkeypatch):
    size = (64, 16, 12)
    om, ic, _, _ = _oracle_run(oracle, size, "warm")
    a, _ = _device_run(bz, monkeypatch, om, ic, size, "warm", steps=STEPS + 3, graph=True)
    info = a.graph_info()
    assert info[0] and info[1] == 1 and info[2] >= 1, info
    b, _ = _device_run(bz, monkeypatch, om, ic, size, "warm", steps=STEPS + 3)
    assert b.profile()[SLOT][1] == 1 + 3 * (STEPS + 3)
    fa, fb = _raw(a), _raw(b)
    for n in fa:
        assert np.isfinite(a.prognostic_fields()["ρq"].interior_cpu()).all() and np.array_equal(fa[n], fb[n], equal_nan=True), n


def test_many_time_steps_equal_single_steps(oracle, bz, monkeypatch):
    size = (66, 9, 9)
    om, ic, _, _ = _oracle_run(oracle, size, "mixed")
    a, _ = _device_run(bz, monkeypatch, om, ic, size, "mixed", steps=4)
    b, _ = _device_run(bz, monkeypatch, om, ic, size, "mixed", steps=0)
    bz.many_time_steps_(b, DT, 4)
    b.synchronize()
    assert b.profile()[SLOT][1] == 1 + 3 * 4
    fa, fb = _raw(a), _raw(b)
    for n in fa:
        assert np.array_equal(fa[n], fb[n], equal_nan=True), n


def test_float32_three_steps_judged_by_their_increments(oracle, bz, monkeypatch):
    """Float32 against the Float64 corrected oracle by helpers.assert_increments, under the 10 K bubble in twice the wind of the other Float32
    step tests (the measure divides by what three steps move a field)"""
    size = (64, 16, 12)
    om, ic, start, want = _oracle_run(oracle, size, "warm", amplitude=10.0, wind=2.0)
    hm, set_launches = _device_run(bz, monkeypatch, om, ic, size, "warm", float_type=F32)
    assert set_launches == 2 and hm.profile()[SLOT][1] == 1 + 3 * STEPS
    got = _fields(hm)
    names = ("ru", "rv", "rw", "rtheta", "rq", "T")
    assert_increments("negative moisture correction", {n: got[n] for n in names}, {n: want[n] for n in names}, {n: start[n] for n in names}, "anelastic")


# ---- equivalences, to the bit ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("phase", ["warm", "mixed"])
def test_schemes_with_nothing_to_do_step_like_the_bare_adjustment(oracle, bz, monkeypatch, phase):
    """BulkMicrophysics(negative_moisture_correction = nothing) and SpeciesBorrowing() (an empty chain, no vertical borrowing): the bits of
    the model built with the SaturationAdjustment itself, and no launch in the slot"""
    size = (64, 16, 12)
    om, ic, _, _ = _oracle_run(oracle, size, phase)
    runs = {}
    for correction in ("bare", "none", "species"):
        hm, set_launches = _device_run(bz, monkeypatch, om, ic, size, phase, correction=correction)
        assert set_launches == 0 and hm.profile().get(SLOT, (0.0, 0))[1] == 0, correction
        runs[correction] = _raw(hm)
    assert (runs["bare"]["ρq"] < 0).any()          # nothing repaired the planted cells
    for correction in ("none", "species"):
        for n, a in runs["bare"].items():
            assert np.array_equal(a, runs[correction][n], equal_nan=True), (correction, n)


def test_a_state_without_negative_cells_steps_like_the_uncorrected_model(oracle, bz, monkeypatch):
    size = (64, 16, 12)
    om = nmr.oracle_model(oracle, size, "warm", corrected_run=False)
    ic = nmr.planted_bubble(om.grid)
    ic["qt"] = np.abs(ic["qt"])
    runs = {}
    for correction in ("bare", "vertical", "both"):
        hm, _ = _device_run(bz, monkeypatch, om, ic, size, "warm", correction=correction)
        assert hm.profile().get(SLOT, (0.0, 0))[1] == (0 if correction == "bare" else 1 + 3 * STEPS)
        runs[correction] = _raw(hm)
    assert (runs["bare"]["ρq"][hm.grid.interior_slices(False)] > 0).all()
    for correction in ("vertical", "both"):
        for n, a in runs["bare"].items():
            assert np.array_equal(a, runs[correction][n], equal_nan=True), (correction, n)


def test_detaching_returns_to_the_uncorrected_bits(oracle, bz, monkeypatch):
    size = (64, 16, 12)
    om, ic, _, _ = _oracle_run(oracle, size, "warm")
    bare, _ = _device_run(bz, monkeypatch, om, ic, size, "warm", correction="bare")
    hm = _device_model(bz, size, "warm")
    hm._check(hm._lib.bz_set_negative_moisture_correction(hm._ctx, None), "bz_set_negative_moisture_correction")
    rc = hm._lib.bz_fix_negative_moisture(hm._ctx, C.byref(hm._state))
    assert rc == BZ_ERR_INVALID and "bz_fix_negative_moisture" in hm._lib.bz_last_error(hm._ctx).decode()
    hm.profile_enable(True)
    hm.profile_reset()
    _set_device(hm, om, ic)
    for _ in range(STEPS):
        hm.time_step(DT)
    hm.synchronize()
    assert hm.profile().get(SLOT, (0.0, 0))[1] == 0
    fa, fb = _raw(bare), _raw(hm)
    for n in fa:
        assert np.array_equal(fa[n], fb[n], equal_nan=True), n
    corrected, _ = _device_run(bz, monkeypatch, om, ic, size, "warm")
    assert not np.array_equal(_raw(corrected)["ρq"], fa["ρq"])


# ---- the C entry point's refusals -----------------------------------------------------------------------------------------------------------------------
def test_the_entry_point_refuses_what_it_does_not_run(bz):
    grid = bz.RectilinearGrid((16, 8, 8), x=(0, 1600.0), y=(0, 800.0), z=(0, 8e3))
    warm = bz.SaturationAdjustment(equilibrium=bz.WarmPhaseEquilibrium())
    dyn = bz.CompressibleDynamics(bz.SplitExplicitTimeDiscretization(substeps=6))
    cm = bz.CompressibleAtmosphereModel(grid, dyn, advection=bz.WENO(order=5), microphysics=warm)
    dry = bz.AtmosphereModel(grid, advection=bz.WENO(order=5))
    for m, word in ((cm, "CompressibleDynamics"), (dry, "SaturationAdjustment")):
        rc = _attach(m, False, True)
        text = m._lib.bz_last_error(m._ctx).decode()
        assert rc == BZ_ERR_UNSUPPORTED and "bz_set_negative_moisture_correction" in text and word in text, (rc, text)
    hm = bz.AtmosphereModel(grid, advection=bz.WENO(order=5), microphysics=warm)
    a, b = _species_fields(bz, hm, 2)

    def refused(word, *args, **kw):
        rc = _attach(hm, *args, **kw)
        text = hm._lib.bz_last_error(hm._ctx).decode()
        assert rc == BZ_ERR_INVALID and "bz_set_negative_moisture_correction" in text and word in text, (rc, text)

    refused("twice", True, False, mass=(a, a))
    refused("number and in mass", True, False, mass=(a,), pairs=((a, b),))
    refused("neither", False, False, mass=(a,))
    for name in ("n_mass", "n_pairs", "n_clamp"):
        d = hm._T.bz_negative_moisture_correction()
        d.species_borrowing = 1
        setattr(d, name, 5)
        rc = hm._lib.bz_set_negative_moisture_correction(hm._ctx, C.byref(d))
        assert rc == BZ_ERR_INVALID and name in hm._lib.bz_last_error(hm._ctx).decode()
        setattr(d, name, -1)
        assert hm._lib.bz_set_negative_moisture_correction(hm._ctx, C.byref(d)) == BZ_ERR_INVALID
    d = hm._T.bz_negative_moisture_correction()
    d.species_borrowing, d.n_mass = 1, 1          # mass[0] stays NULL
    rc = hm._lib.bz_set_negative_moisture_correction(hm._ctx, C.byref(d))
    assert rc == BZ_ERR_INVALID and "null" in hm._lib.bz_last_error(hm._ctx).decode()
    # nothing of the refused descriptors was kept: nothing is attached
    assert hm._lib.bz_fix_negative_moisture(hm._ctx, C.byref(hm._state)) == BZ_ERR_INVALID
    # the moisture prognostic itself in the chain: refused by the run, which is where it is known
    assert _attach(hm, True, True, mass=(hm.moisture_density,)) == 0
    rc = hm._lib.bz_fix_negative_moisture(hm._ctx, C.byref(hm._state))
    assert rc == BZ_ERR_INVALID and "moisture prognostic" in hm._lib.bz_last_error(hm._ctx).decode()
