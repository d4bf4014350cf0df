"""ThermodynamicConstants(saturation_vapor_pressure = FlatauPolynomial()) on the device: the polynomial instantiations of k_thermo,
k_project_diagnose<1 | 3>, k_cmp_diagnose<.., 3>, k_ac_stage_end<.., 3> and k_instantaneous_precipitation (bz_fl_psat_* of csrc/bz_internal.h)
over the parcel sweeps of tests/flatau_reference.py, whole steps against the oracle models of that module, graph replay, the switch back
to Clausius-Clapeyron and the entry point's refusals.

Judging of the sweeps (sar.judge64 / judge32 and mpr.judge64 / judge32, unchanged; nothing of a bound comes from the device): Float64 T
within max(1e-13, 16 d80) relative, each fraction within max(1e-15, 16 d80) absolute, d80 the restatement's own float64-to-longdouble
distance of the parcel's population and solver; clear parcels: exact zeros and the bits of q^t; threshold parcels on either forced branch;
theta = 0 exact; knife-edge parcels skipped (at most 0.5 % of the cloudy ones, asserted on the CPU).  Float32 within 4 d32.
Steps: the bounds of the Clausius-Clapeyron tests they mirror — tests/test_mixed_phase.py (picked tier within 1e-9 of the oracle, the other
tiers within 1e-12 of the picked one) and tests/test_gpu_compressible.py::test_compressible_saturation_adjustment_matches_oracle (1e-12 /
1e-13 after set!, 1e-8 / 1e-9 after the steps)."""
import ctypes as C

import numpy as np
import pytest

import flatau_reference as flr
import instantaneous_precipitation_reference as ipr
import mixed_phase_reference as mpr
import saturation_adjustment_reference as sar
from helpers import PROG

pytestmark = pytest.mark.gpu
F64, F32, LD = np.float64, np.float32, np.longdouble
A_SMALL, A_LARGE = sar.ANELASTIC_GRIDS
SMALL, LARGE = sar.COMPRESSIBLE_GRIDS
NAN = float("nan")
EPS = float(np.finfo(F64).eps)
BZ_ERR_UNSUPPORTED = 2
PBP, FLAT, PBB = ("Periodic", "Periodic", "Bounded"), ("Periodic", "Flat", "Bounded"), ("Periodic", "Bounded", "Bounded")


def test_the_class_is_exported(bz):
    assert "FlatauPolynomial" in repr(bz.FlatauPolynomial()) and "bz_set_saturation_vapor_pressure_polynomial" in bz.SYMBOLS


def _constants(bz):
    return bz.ThermodynamicConstants(saturation_vapor_pressure=bz.FlatauPolynomial())


def _adjustment(bz, mixed, solver=sar.DEFAULT_SOLVER):
    eq = bz.MixedPhaseEquilibrium(freezing_temperature=flr.TF, homogeneous_ice_nucleation_temperature=flr.TH) if mixed else bz.WarmPhaseEquilibrium()
    return bz.SaturationAdjustment(equilibrium=eq, solver=bz.SecantSolver(abstol=solver[0], maxiter=solver[1]))


def _columns(hm):
    rho, p = hm._ref_arrays[0], hm._ref_arrays[1]
    Hz, Nz = hm.grid.Hz, hm.grid.Nz
    return p[Hz:Hz + Nz].copy(), rho[Hz:Hz + Nz].copy()


# ---- anelastic sweeps: k_thermo and k_project_diagnose ------------------------------------------------------------------------------------------
def _anelastic(bz, shape, mixed, solver=sar.DEFAULT_SOLVER, float_type=F64):
    Lz = sar.TALL_COLUMN if mixed else sar.COLUMN
    grid = bz.RectilinearGrid(shape, halo=3, float_type=float_type, x=(0.0, 100.0 * shape[0]), y=(0.0, 100.0 * shape[1]), z=(0.0, float(Lz)))
    ref = bz.ReferenceState(grid, surface_pressure=sar.SURFACE_PRESSURE, potential_temperature=sar.THETA_0, standard_pressure=sar.PST)
    hm = bz.AtmosphereModel(grid, dynamics=bz.AnelasticDynamics(ref), advection=bz.WENO(order=5), microphysics=_adjustment(bz, mixed, solver),
                            thermodynamic_constants=_constants(bz))
    if float_type is F64:            # the columns the sweeps were realised on: the device's, bit for bit
        p_r, rho_r = _columns(hm)
        want_p, want_rho = sar.reference_column(shape[2], Lz)
        assert np.array_equal(p_r, want_p) and np.array_equal(rho_r, want_rho)
    return hm


def _plant(hm, case):
    mu = hm.microphysical_fields
    fields = dict(rtheta=hm.potential_temperature_density, rq=hm.moisture_density)
    for n, f in fields.items():
        f.set_interior(case[n])
    for f in [hm.temperature, hm.specific_moisture, hm.potential_temperature] + [mu[k] for k in ("qᵛ", "qˡ", "qⁱ") if k in mu]:
        f.parent.fill_(NAN)
    return {n: f.interior.cpu().numpy() for n, f in fields.items()}


def _read(hm):
    hm.synchronize()
    mu = hm.microphysical_fields
    get = lambda f: f.interior.cpu().numpy()
    out = dict(T=get(hm.temperature), q=get(hm.specific_moisture), theta=get(hm.potential_temperature), qv=get(mu["qᵛ"]), ql=get(mu["qˡ"]))
    if "qⁱ" in mu:
        out["qi"] = get(mu["qⁱ"])
    return out


def _show(label, report, table, skipped=0):
    for name, row in report.items():
        d = table.get(name, (0.0,) * len(row))
        print(f"FLATAUPARCELS {label} {name}: device", " ".join(f"{v:.1e}" for v in row), "| restatement's own", " ".join(f"{v:.1e}" for v in d),
              f"| knife-edge skipped: {skipped}" if skipped else "")


def _judge(label, mixed, dev, want, tag, table, clear, cloudy):
    fails, report, skipped = (mpr.judge64 if mixed else sar.judge64)(dev, want, tag, table, clear, cloudy)
    _show(label, report, table, skipped)
    assert not fails, (label, fails)
    assert np.array_equal(dev["q"], want["q"]) and np.array_equal(dev["theta"], want["theta"])


ANELASTIC_SWEEPS = [(mixed, shape, solver) for mixed in (False, True) for shape, solver in flr.SWEEPS["mixed" if mixed else "pressure"]]


@pytest.mark.parametrize("mixed,shape,solver", ANELASTIC_SWEEPS,
                         ids=[f"{'mixed' if m else 'warm'}-{s[0]}x{s[1]}x{s[2]}-secant{so[0]:g},{so[1]}" for m, s, so in ANELASTIC_SWEEPS])
def test_anelastic_diagnosis_over_the_sweep(bz, mixed, shape, solver):
    """update_state!(compute_tendencies = false): k_thermo<false | true, true>"""
    form = "mixed" if mixed else "pressure"
    hm = _anelastic(bz, shape, mixed, solver)
    case = flr.case_of(form, shape)
    held = _plant(hm, case)
    for n, a in held.items():
        assert np.array_equal(a, case[n]), n
    bz.update_state_(hm, compute_tendencies=False)
    dev = _read(hm)
    _judge(f"k_thermo {form} {shape} secant={solver}", mixed, dev, flr.restated(form, shape, F64, solver), case.tag, flr.d80(form, shape, solver),
           flr.restated(form, shape, F64, solver, "clear"), flr.restated(form, shape, F64, solver, "cloudy"))
    # another formulation than Clausius-Clapeyron ran: the sweep's own Clausius-Clapeyron restatement is kelvins of rounding away
    cc = (mpr.diagnose_mixed(held, case.p_r, case.rho_r, F64, solver) if mixed else sar.diagnose_anelastic(held, 1, case.p_r, case.rho_r, F64, solver))
    assert np.abs(dev["T"] - cc["T"]).max() > 1e-6


@pytest.mark.parametrize("mixed", (False, True), ids=("warm", "mixed"))
def test_fused_step_leaves_the_restatement_of_its_fields(bz, mixed):
    """time_step! (whole step, dt = 1e-3) from the sweep with small smooth winds: what is read was written by the projection-and-diagnosis
    kernel of stage 3 (k_project_diagnose<1 | 3, true>; profile slot project_and_diagnose, three launches), not by k_thermo"""
    from test_saturation_adjustment_parcels import _winds
    form, shape = ("mixed" if mixed else "pressure"), A_SMALL
    hm = _anelastic(bz, shape, mixed)
    if mixed:                        # the sweep itself, its four theta = 0 cells at 300 K (a cell without temperature has no buoyancy to step with)
        case = flr.mixed_case(shape)
        case = sar.Case(case, rtheta=np.where(case.tag == "theta_zero", 300.0 * case.rho_r[:, None, None], case.rtheta))
    else:
        case = flr.anelastic_case(shape, bulk_only=True)
    _plant(hm, case)
    _winds(hm.grid, hm.momentum, case.rho_r[:, None, None])
    hm.profile_enable(True)
    hm.profile_reset()
    bz.time_step_(hm, 1e-3, whole_step=True)
    hm.synchronize()
    stale, profile = bz.diagnostics_stale(hm), hm.profile()
    held = {"rtheta": hm.potential_temperature_density.interior.cpu().numpy(), "rq": hm.moisture_density.interior.cpu().numpy()}
    dev = _read(hm)
    print(f"FLATAUPARCELS step {form} slots:", {k: v[1] for k, v in profile.items()})
    assert not stale and not np.array_equal(held["rtheta"], case.rtheta)
    assert profile.get("project_and_diagnose", (0, 0))[1] == 3 and profile.get("compute_auxiliary_thermodynamic_variables", (0, 0))[1] == 1
    p_r, rho_r = _columns(hm)
    diagnose = flr.diagnose_mixed if mixed else flr.diagnose_anelastic
    want, wide = diagnose(held, p_r, rho_r, F64), diagnose(held, p_r, rho_r, LD)
    assert not want.nonfinite.any() and 0.2 <= np.mean(want.branch == sar.CLOUDY) <= 0.8
    table = mpr.own_distance(want, wide, case.tag) if mixed else flr.own_distance(want, wide, case.tag)
    _judge(f"k_project_diagnose {form}", mixed, dev, want, case.tag, table, diagnose(held, p_r, rho_r, F64, force_branch="clear"),
           diagnose(held, p_r, rho_r, F64, force_branch="cloudy"))


@pytest.mark.parametrize("form", ("pressure", "mixed", "density"))
def test_a_parcels_result_does_not_depend_on_its_wavefront(bz, form):
    """the same parcels under two placements (the second shuffles every level): the same bits per parcel"""
    outs, names = [], ("T", "qv", "ql") + (("qi",) if form == "mixed" else ())
    for which in (0, 1):
        if form == "density":
            hm = _compressible(bz, LARGE)
            case = flr.compressible_case(LARGE, which)
            _plant_compressible(hm, case)
            bz.compressible.update_state_(hm, compute_tendencies=False)
            dev = _read_compressible(hm)
        else:
            hm = _anelastic(bz, A_LARGE, form == "mixed")
            case = flr.case_of(form, A_LARGE, which)
            _plant(hm, case)
            bz.update_state_(hm, compute_tendencies=False)
            dev = _read(hm)
        outs.append({n: mpr.by_parcel(case, dev[n]) for n in names} | {"tag": mpr.by_parcel(case, case.tag)})
    assert np.array_equal(outs[0]["tag"], outs[1]["tag"])
    for n in names:
        assert np.array_equal(outs[0][n], outs[1][n]), (n, int((outs[0][n] != outs[1][n]).sum()))


@pytest.mark.parametrize("mixed", (False, True), ids=("warm", "mixed"))
def test_float32_anelastic_diagnosis_over_the_sweep(bz, mixed):
    import torch
    form, shape = ("mixed" if mixed else "pressure"), A_LARGE
    hm = _anelastic(bz, shape, mixed, float_type=F32)
    assert hm.temperature.parent.dtype == torch.float32
    case = flr.case_of(form, shape)
    held = _plant(hm, case)
    bz.update_state_(hm, compute_tendencies=False)
    dev = _read(hm)
    p32, rho32 = _columns(hm)

    def diagnose(dtype, branch=None):
        return (flr.diagnose_mixed if mixed else flr.diagnose_anelastic)({n: a.astype(dtype) for n, a in held.items()}, p32.astype(dtype),
                                                                         rho32.astype(dtype), dtype, force_branch=branch)

    want32, want64 = diagnose(F32), diagnose(F64)
    fails, report, table = (mpr.judge32 if mixed else sar.judge32)(dev, want32, want64, case.tag, float(np.abs(want64["q"]).max()),
                                                                   diagnose(F64, "clear"), diagnose(F64, "cloudy"))
    print(f"FLATAUPARCELS f32 {form}", report, table)
    assert not fails, fails
    assert np.array_equal(dev["q"], want32["q"]) and np.array_equal(dev["theta"], want32["theta"])


# ---- compressible sweeps: k_cmp_diagnose and k_ac_stage_end -----------------------------------------------------------------------------------------
def _compressible(bz, shape, solver=sar.DEFAULT_SOLVER, float_type=F64, **kw):
    grid = bz.RectilinearGrid(shape, halo=3, float_type=float_type, x=(0.0, 100.0 * shape[0]), y=(0.0, 100.0 * shape[1]), z=(0.0, 3e3))
    dyn = bz.CompressibleDynamics(bz.SplitExplicitTimeDiscretization(substeps=6), surface_pressure=1e5, standard_pressure=sar.PST,
                                  reference_potential_temperature=ipr.theta_ref)
    return bz.CompressibleAtmosphereModel(grid, dyn, advection=bz.WENO(order=5), microphysics=_adjustment(bz, False, solver),
                                          thermodynamic_constants=_constants(bz), temperature_solver=bz.NewtonSolver(abstol=sar.NEWTON[0], maxiter=sar.NEWTON[1]),
                                          **kw)


def _plant_compressible(hm, case):
    mu = hm.microphysical_fields
    fields = dict(rho_d=hm.dynamics.dry_density, rtheta=hm.potential_temperature_density, rq=hm.moisture_density)
    for n, f in fields.items():
        f.set_interior(case[n])
    for f in (hm.temperature, hm.dynamics.pressure, hm.dynamics.total_density, hm.specific_moisture, hm.potential_temperature, mu["qᵛ"], mu["qˡ"]):
        f.parent.fill_(NAN)
    return {n: f.interior.cpu().numpy() for n, f in fields.items()}


def _read_compressible(hm):
    hm.synchronize()
    mu = hm.microphysical_fields
    get = lambda f: f.interior.cpu().numpy()
    return dict(T=get(hm.temperature), p=get(hm.dynamics.pressure), q=get(hm.specific_moisture), rho=get(hm.dynamics.total_density),
                theta=get(hm.potential_temperature), qv=get(mu["qᵛ"]), ql=get(mu["qˡ"]))


def _judge_compressible(label, dev, want, tag, table, clear, cloudy):
    """sar.judge64 on (T, q^v, q^l); rho, theta and the stored q are single IEEE operations on the inputs: the restatement's bits; p = rho R_m T
    within T's bound + 4 eps (tests/test_saturation_adjustment_parcels.py: _compressible_extras)"""
    fails, report, skipped = sar.judge64(dev, want, tag, table, clear, cloudy)
    _show(label, report, table, skipped)
    assert not fails, (label, fails)
    for n in ("rho", "q", "theta"):
        assert np.array_equal(dev[n], want[n]), (label, n)
    bT = sar.bounds64(tag, table)[0]
    ordinary = ~(want["knife"] | (tag == "marginal_edge")) & (want["T"] != 0)
    with np.errstate(all="ignore"):
        ep = np.abs(dev["p"] - want["p"]) / np.abs(want["p"])
    assert np.all(ep[ordinary] <= bT[ordinary] + 4 * EPS), (label, float(ep[ordinary].max()))
    assert np.all(dev["p"][want["branch"] == sar.THETA_ZERO] == 0) and np.isfinite(dev["p"]).all() and np.isfinite(dev["T"]).all()


@pytest.mark.parametrize("shape,solver", flr.SWEEPS["density"], ids=[f"{s[0]}x{s[1]}x{s[2]}-secant{so[0]:g},{so[1]}" for s, so in flr.SWEEPS["density"]])
def test_compressible_diagnosis_over_the_sweep(bz, shape, solver):
    """update_state!(compute_tendencies = false) of the compressible model: k_cmp_diagnose<true, false, 3> (bz_ds_adjust<true>)"""
    hm = _compressible(bz, shape, solver)
    case = flr.compressible_case(shape)
    held = _plant_compressible(hm, case)
    for n, a in held.items():
        assert np.array_equal(a, case[n]), n
    bz.compressible.update_state_(hm, compute_tendencies=False)
    dev = _read_compressible(hm)
    _judge_compressible(f"k_cmp_diagnose {shape} secant={solver}", dev, flr.restated("density", shape, F64, solver), case.tag, flr.d80("density", shape, solver),
                        flr.restated("density", shape, F64, solver, "clear"), flr.restated("density", shape, F64, solver, "cloudy"))
    cc = sar.diagnose_compressible(held, 1, F64, solver)
    assert np.abs(dev["T"] - cc["T"]).max() > 1e-6


@pytest.mark.parametrize("solver", [sar.DEFAULT_SOLVER, (0.0, 20)], ids=["secant1e-4,20", "secant0,20"])
def test_float32_compressible_diagnosis_over_the_sweep(bz, solver):
    """k_cmp_diagnose_f32<.., 3> under the default solver and under SecantSolver(abstol = 0, maxiter = 20), the Float32 solvers of
    tests/test_saturation_adjustment_parcels.py, at 4 d32.  Under abstol = 0 every parcel is judged.  Under the default solver the parcels of
    flr.float32_knife_edge are left out, as the Float64 rule leaves its knife-edge parcels out: those whose float32 and float64 restatements
    stop on different branches or iteration counts, and cloudy parcels whose condensate is below what abstol resolves.  Measured without
    the exclusion: 1 of 162 threshold parcels at 4.2e-8 in q^v against a 4 d32 of 2.3e-8 — the device holds q^l = 4.3e-8 where both
    restatements hold an exact 0, 1.6e-4 K apart in T; with it (440 of 3659 cloudy parcels left out) every population is inside its bound."""
    hm = _compressible(bz, LARGE, solver, float_type=F32)
    case = flr.compressible_case(LARGE)
    held = _plant_compressible(hm, case)
    assert all(a.dtype == F32 for a in held.values())
    bz.compressible.update_state_(hm, compute_tendencies=False)
    dev = _read_compressible(hm)
    diagnose = lambda dtype, branch=None: flr.diagnose_compressible({n: a.astype(dtype) for n, a in held.items()}, dtype, solver, force_branch=branch)
    want32, want64 = diagnose(F32), diagnose(F64)
    out = flr.float32_knife_edge(want32, want64, solver[0])
    assert np.isfinite(dev["T"]).all() and np.isfinite(dev["qv"]).all() and np.isfinite(dev["ql"]).all()
    judged = dict(dev, **{n: np.where(out, want32[n], dev[n]) for n in ("T", "qv", "ql")})
    fails, report, table = sar.judge32(judged, want32, want64, case.tag, float(np.abs(want64["q"]).max()), diagnose(F64, "clear"), diagnose(F64, "cloudy"))
    print(f"FLATAUPARCELS f32 density secant={solver}: left out {int(out.sum())} of {int((want64.branch == sar.CLOUDY).sum())} cloudy parcels", report, table)
    assert not fails, fails
    assert np.array_equal(dev["q"], want32["q"]) and np.array_equal(dev["theta"], want32["theta"])


@pytest.mark.parametrize("substep_floattype", (None, F32), ids=("substeps-f64", "substeps-f32"))
def test_compressible_fused_step_leaves_the_restatement_of_its_fields(bz, substep_floattype):
    """time_step! (whole step, dt = 1e-3, 6 substeps) from the bulk sweep: the T, p, q^v, q^l read were written by the stage-end kernel of stage 3
    (k_ac_stage_end<.., 3, double | float>; profile slots acoustic_stage_end+update_state[+linearization], three launches between them);
    k_cmp_diagnose ran once, in the update_state! that prepares the first step (tests/test_saturation_adjustment_parcels.py)"""
    from test_saturation_adjustment_parcels import _winds
    shape = SMALL
    hm = _compressible(bz, shape, **({"substep_floattype": substep_floattype} if substep_floattype else {}))
    case = flr.compressible_case(shape, bulk_only=True)
    _plant_compressible(hm, case)
    _winds(hm.grid, hm.momentum, case.rho_d)
    hm.profile_enable(True)
    hm.profile_reset()
    hm.time_step(1e-3)
    hm.synchronize()
    profile = hm.profile()
    print("FLATAUPARCELS step compressible slots:", {k: v[1] for k, v in profile.items()})
    held = dict(rho_d=hm.dynamics.dry_density.interior.cpu().numpy(), rtheta=hm.potential_temperature_density.interior.cpu().numpy(),
                rq=hm.moisture_density.interior.cpu().numpy())
    dev = _read_compressible(hm)
    slot = lambda name: profile.get(name, (0.0, 0))[1]
    assert not np.array_equal(held["rtheta"], case.rtheta)
    assert slot("acoustic_stage_end+update_state") + slot("acoustic_stage_end+update_state+linearization") == 3
    assert slot("update_state") + slot("update_state+linearization") == 1 and not bz.diagnostics_stale(hm)
    want, wide = flr.diagnose_compressible(held, F64), flr.diagnose_compressible(held, LD)
    assert not want.nonfinite.any() and 0.2 <= np.mean(want.branch == sar.CLOUDY) <= 0.8
    _judge_compressible("k_ac_stage_end", dev, want, case.tag, flr.own_distance(want, wide, case.tag), None, None)


def test_instantaneous_precipitation_update_on_the_reference_grid(oracle, oc, bz):
    """microphysics_model_update! on the reference's (8, 8, 8) halo-5 grid (test/instantaneous_precipitation.jl:133) in the bubble of
    tests/instantaneous_precipitation_reference.py: rho q^v = rho q^v+ and rho theta = rho_d theta_f of TypedFlatau.ip_update cell by cell, from
    the device's own rho, rho_d, rho theta, rho q; precipitation_rate an exact zero wherever the restatement does not condense"""
    shape, halo = (8, 8, 8), 5
    ext, L = ipr.extents(shape)
    grid = bz.RectilinearGrid(shape, halo=halo, **ext)
    dyn = bz.CompressibleDynamics(bz.SplitExplicitTimeDiscretization(substeps=6), surface_pressure=1e5, standard_pressure=1e5,
                                  reference_potential_temperature=ipr.theta_ref)
    hm = bz.CompressibleAtmosphereModel(grid, dyn, advection=bz.WENO(order=5), thermodynamic_constants=_constants(bz),
                                        microphysics=bz.InstantaneousPrecipitation(equilibrium=bz.WarmPhaseEquilibrium()))
    om, _, _ = ipr.make_restatement(oracle, oc, shape, halo)          # lends the reference density of the grid
    th, qt = ipr.bubble_state(*L)
    g = om.grid
    hm.set(ρ=om.ref.density[g.Hz:g.Hz + g.Nz][:, None, None], θ=th, u=2.0, v=0.0, w=0.0, qᵗ=qt)
    bz.compressible.update_state_(hm)
    get = lambda f: f.interior_cpu().copy()
    r, rd, rth, rq = get(hm.dynamics.total_density), get(hm.dynamics.dry_density), get(hm.potential_temperature_density), get(hm.moisture_density)
    bz.microphysics_model_update_(hm.microphysics, hm, Δt=1.0)
    hm.synchronize()
    rth1, rq1, P = get(hm.potential_temperature_density), get(hm.moisture_density), get(hm.microphysical_fields["precipitation_rate"])
    want = {t: dict(rq=np.zeros(r.shape, t), rth=np.zeros(r.shape, t), c=np.zeros(r.shape, t)) for t in (F64, LD)}
    for t, out in want.items():
        F = flr.TypedFlatau(t)
        for idx in np.ndindex(r.shape):
            rho, rho_d = t(r[idx]), t(rd[idx])
            q0 = t(rq[idx]) / rho
            u = F.ip_update(t(rth[idx]) / rho_d, q0, rho, t(1e5))
            out["rq"][idx], out["rth"][idx], out["c"][idx] = rho * u["qv"], rho_d * u["theta_f"], rho * max(t(0), q0 - u["qv"])
    w, wide = want[F64], want[LD]
    condensed = w["c"] > 0
    assert 0.02 < condensed.mean() < 0.98 and np.array_equal(condensed, wide["c"] > 0)
    d80 = {n: float(np.max(np.abs(w[n].astype(LD) - wide[n]) / np.abs(wide[n]))) for n in ("rq", "rth")}
    err = {n: float(np.max(np.abs(got - w[n]) / np.abs(w[n]))) for n, got in (("rq", rq1), ("rth", rth1))}
    print("FLATAUPARCELS instantaneous precipitation: device", err, "| restatement's own", d80, f"| condensing {condensed.mean():.2f}")
    assert err["rth"] <= max(1e-13, 16 * d80["rth"]) and err["rq"] <= max(1e-13, 16 * d80["rq"])
    assert np.all(P[~condensed] == 0.0) and np.all(P[condensed] > 0.0)
    assert np.all(np.abs(P[condensed] - w["c"][condensed]) <= max(1e-13, 16 * d80["rq"]) * rq[condensed])
    cc = ipr.in_dtype(F64)
    first = tuple(np.argwhere(condensed)[0])
    assert abs(float(cc.ip_update(rth[first] / rd[first], rq[first] / r[first], r[first], 1e5)["qv"]) * r[first] - rq1[first]) > 1e-9 * rq1[first]


# ---- three steps against the oracle models ------------------------------------------------------------------------------------------------------------
DT, STEPS = 2.0, 3
TIERS = {"picked": {}, "BZ_NO_FUSE_RK": {"BZ_NO_FUSE_RK": "1"}, "BZ_NO_FUSED": {"BZ_NO_FUSED": "1"}}
_ORACLE_RUNS = {}


def _pair(oracle, bz, size, mixed, topology=PBP, device=True, set_state=True):
    """the set-up of tests/test_mixed_phase.py (_pair, _bubble): a 10 km column under theta_0 = 300 K crosses T^f near 2.7 km and T^h near 6.8 km"""
    from test_mixed_phase import _bubble
    flat = topology == FLAT
    ext = dict(x=(-4e3, 4e3), z=(0.0, 10e3)) if flat else dict(x=(-4e3, 4e3), y=(-3e3, 3e3), z=(0.0, 10e3))
    og = oracle.Grid(size, topology=topology, halo=(3, 3) if flat else (3,) * 3, **ext)
    om = (flr.FlatauMixedOracleModel if mixed else flr.FlatauOracleModel)(og, potential_temperature=300.0, advection="WENO5")
    ic = _bubble(og)
    if not device:
        om.set(qt=ic["qt"], theta=ic["theta"], u=ic["u"])
        return om, None
    grid = bz.RectilinearGrid(size, topology=tuple(getattr(bz, t) for t in topology), halo=(3, 3) if flat else (3,) * 3, **ext)
    hm = bz.AtmosphereModel(grid, dynamics=bz.AnelasticDynamics(bz.ReferenceState(grid, potential_temperature=300.0)), advection=bz.WENO(order=5),
                            microphysics=_adjustment(bz, mixed), thermodynamic_constants=_constants(bz))
    if set_state:
        hm.set(qᵗ=ic["qt"], θ=ic["theta"], u=ic["u"])
    return om, hm


def _fields(hm):
    mu = hm.microphysical_fields
    out = {n: hm.prognostic_fields()[k].interior_cpu().astype(F64) for n, k in PROG.items()}
    out.update(T=hm.temperature.interior_cpu().astype(F64), qv=mu["qᵛ"].interior_cpu().astype(F64), ql=mu["qˡ"].interior_cpu().astype(F64))
    out["qi"] = mu["qⁱ"].interior_cpu().astype(F64) if "qⁱ" in mu else np.zeros_like(out["ql"])
    return out


def _oracle_run(oracle, size, mixed, topology=PBP):
    key = (size, mixed, topology)
    if key not in _ORACLE_RUNS:
        from test_mixed_phase import _oracle_fields
        om, _ = _pair(oracle, None, size, mixed, topology, device=False)
        start = _oracle_fields(om)
        for _ in range(STEPS):
            om.time_step(DT)
        _ORACLE_RUNS[key] = (start, _oracle_fields(om))
    return _ORACLE_RUNS[key]


def _device_run(oracle, bz, monkeypatch, size, mixed, env, topology=PBP, graph=False, steps=STEPS):
    for name in ("BZ_NO_FUSE_RK", "BZ_NO_FUSED"):          # set before the context is created
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    _, hm = _pair(oracle, bz, size, mixed, topology)
    if graph:
        hm.graph_enable(True)
    else:
        hm.profile_enable(True)
        hm.profile_reset()
    for _ in range(steps):
        hm.time_step(DT)
    hm.synchronize()
    return hm, _fields(hm)


def _assert_steps(label, got, want, tol):
    from test_mixed_phase import _scaled_errors
    errs = _scaled_errors(got, want)
    print(f"FLATAUSTEPS {label}:", " ".join(f"{n}={e:.1e}" for n, e in errs.items()))
    assert all(e < tol for e in errs.values()), (label, {k: f"{v:.1e}" for k, v in errs.items()})


def _clouds(got, mixed):
    from test_mixed_phase import _regimes
    return all(_regimes(got["ql"], got["qi"])) if mixed else bool((got["ql"] > 0).any() and (got["ql"] == 0).any() and not got["qi"].any())


@pytest.mark.parametrize("size", [(64, 16, 12), (66, 9, 9)], ids=["whole-tiles", "ragged"])
@pytest.mark.parametrize("mixed", (False, True), ids=("warm", "mixed"))
def test_three_steps_match_the_oracle_on_every_tier(oracle, bz, monkeypatch, mixed, size):
    """the tier the model picks within 1e-9 of the oracle model with the polynomial, each other tier within 1e-12 of the picked one"""
    start, want = _oracle_run(oracle, size, mixed)
    runs = {}
    for tier, env in TIERS.items():
        hm, runs[tier] = _device_run(oracle, bz, monkeypatch, size, mixed, env)
        print(f"FLATAUSTEPS {size} {tier} slots:", {k: v[1] for k, v in hm.profile().items()})
    assert _clouds(runs["picked"], mixed) and not np.array_equal(want["rw"], start["rw"])
    _assert_steps(f"{'mixed' if mixed else 'warm'} {size} picked vs oracle", runs["picked"], want, 1e-9)
    for tier in ("BZ_NO_FUSE_RK", "BZ_NO_FUSED"):
        _assert_steps(f"{'mixed' if mixed else 'warm'} {size} {tier} vs picked", runs[tier], runs["picked"], 1e-12)


@pytest.mark.parametrize("size,topology", [((64, 12), FLAT), ((16, 8, 8), PBB)], ids=["flat-y", "walls-in-y"])
def test_three_steps_on_the_operators_tier_topologies(oracle, bz, monkeypatch, size, topology):
    start, want = _oracle_run(oracle, size, True, topology)
    hm, got = _device_run(oracle, bz, monkeypatch, size, True, {}, topology)
    slots = {k: v[1] for k, v in hm.profile().items()}
    assert slots.get("project_and_diagnose", 0) == 0 and slots.get("compute_auxiliary_thermodynamic_variables", 0) > 0
    assert _clouds(got, True)
    _assert_steps(f"mixed {size} {topology[1]} vs oracle", got, want, 1e-9)


def test_graph_replay_is_bit_identical(oracle, bz, monkeypatch):
    size = (64, 16, 12)
    a, fa = _device_run(oracle, bz, monkeypatch, size, True, {}, graph=True, steps=2 * STEPS)
    info = a.graph_info()
    assert info[0] and info[1] == 1 and info[2] >= 1, info
    b, fb = _device_run(oracle, bz, monkeypatch, size, True, {}, steps=2 * STEPS)
    for n in fa:
        assert np.isfinite(fa[n]).all() and np.array_equal(fa[n], fb[n]), n
    assert _clouds(fa, True)


def test_null_returns_the_context_to_clausius_clapeyron(oracle, bz, monkeypatch):
    """bz_set_saturation_vapor_pressure_polynomial(NULL): three steps bit-identical to a model built on the default constants in the same
    process, and different from the polynomial's"""
    size = (64, 16, 12)
    for name in ("BZ_NO_FUSE_RK", "BZ_NO_FUSED"):
        monkeypatch.delenv(name, raising=False)
    from test_mixed_phase import _bubble
    # (every model is set once: set! ends in a projection that also corrects the momentum components it was not given, so a second set! of
    # the same keywords does not start from the state of a first one)
    _, hm = _pair(oracle, bz, size, True, set_state=False)
    _, poly = _pair(oracle, bz, size, True, set_state=False)
    hm._check(hm._lib.bz_set_saturation_vapor_pressure_polynomial(hm._ctx, None), "bz_set_saturation_vapor_pressure_polynomial")
    plain = bz.AtmosphereModel(hm.grid, dynamics=bz.AnelasticDynamics(bz.ReferenceState(hm.grid, potential_temperature=300.0)),
                               advection=bz.WENO(order=5), microphysics=_adjustment(bz, True))
    og = oracle.Grid(size, topology=PBP, halo=(3,) * 3, x=(-4e3, 4e3), y=(-3e3, 3e3), z=(0.0, 10e3))
    ic = _bubble(og)
    outs = []
    for m in (hm, plain, poly):
        m.set(qᵗ=ic["qt"], θ=ic["theta"], u=ic["u"])
        for _ in range(STEPS):
            m.time_step(DT)
        m.synchronize()
        outs.append(_fields(m))
    for k in outs[0]:
        assert np.array_equal(outs[0][k], outs[1][k]), k
    assert not np.array_equal(outs[0]["T"], outs[2]["T"]) and _clouds(outs[0], True)


# ---- compressible steps --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,extent", [((16, 12, 12), dict(x=(0.0, 4e3), y=(0.0, 3e3), z=(0.0, 3e3))),
                                         ((66, 6, 6), dict(x=(0.0, 6.6e3), y=(0.0, 3e3), z=(0.0, 3e3)))], ids=["16x12x12", "66-cell-rows"])
@pytest.mark.parametrize("unfused", (False, True), ids=("fused-stage-end", "unfused-stage-end"))
def test_compressible_three_steps_match_the_oracle(oracle, oc, bz, monkeypatch, unfused, size, extent):
    """tests/test_gpu_compressible.py::test_compressible_saturation_adjustment_matches_oracle with the polynomial on both sides, on the fused
    stage epilogue (k_ac_stage_end<.., 3>) and with BZ_NO_AC_END_FUSE=1 (k_cmp_diagnose<.., 3> after every stage)"""
    from test_gpu_compressible import cmp_interior
    monkeypatch.delenv("BZ_NO_AC_END_FUSE", raising=False)
    if unfused:
        monkeypatch.setenv("BZ_NO_AC_END_FUSE", "1")
    thref = lambda z: 300.0 * np.exp(9.80616 * z / (1005 * 300.0))
    og = oracle.Grid(size, **extent)
    om = flr.FlatauCompressibleOracle(og, time_discretization=oc.SplitExplicit(substeps=6), surface_pressure=1e5, reference_potential_temperature=thref,
                                      microphysics="SaturationAdjustment")
    grid = bz.RectilinearGrid(size, **extent)
    dyn = bz.CompressibleDynamics(bz.SplitExplicitTimeDiscretization(substeps=6), surface_pressure=1e5, reference_potential_temperature=thref)
    hm = bz.CompressibleAtmosphereModel(grid, dyn, advection=bz.WENO(order=5), microphysics=_adjustment(bz, False), thermodynamic_constants=_constants(bz))
    Lx, Ly = extent["x"][1], extent["y"][1]
    bub = lambda x, y, z: np.maximum(0.0, 1.0 - np.sqrt(((x - Lx / 2) / (Lx / 4)) ** 2 + ((y - Ly / 2) / (Ly / 2)) ** 2 + ((z - 1200.0) / 900.0) ** 2))
    th = lambda x, y, z: 300.0 + 0.5 * bub(x, y, z) + 0 * z
    qt = lambda x, y, z: 0.012 + 0.014 * bub(x, y, z) + 0.004 * (z / 3e3)
    rho = om.ref.density[og.Hz:og.Hz + og.Nz][:, None, None]
    om.set(rho=rho, theta=th, u=2.0, v=0.0, w=0.0, qv=qt)
    hm.set(ρ=rho, θ=th, u=2.0, v=0.0, w=0.0, qᵗ=qt)
    mu, g = hm.microphysical_fields, om.grid
    ql = g.interior(om.ql)
    assert 0.02 < (ql > 0).mean() < 0.98
    worst = cmp_interior(om, hm, ("rho_d", "rho", "rtheta", "rq", "T", "p"), 1e-12)
    dq = max(np.abs(mu["qˡ"].interior_cpu() - ql).max(), np.abs(mu["qᵛ"].interior_cpu() - g.interior(om.qv)).max())
    print(f"FLATAUSTEPS compressible {size} unfused={unfused} after set:", worst, f"q={dq:.1e}")
    assert dq < 1e-13
    hm.profile_enable(True)
    hm.profile_reset()
    for _ in range(STEPS):
        om.time_step(1.0)
        hm.time_step(1.0)
    slots = {k: v[1] for k, v in hm.profile().items()}
    fused = slots.get("acoustic_stage_end+update_state", 0) + slots.get("acoustic_stage_end+update_state+linearization", 0)
    assert (fused == 0) if unfused else (fused == 3 * STEPS), slots
    worst = cmp_interior(om, hm, ("rho_d", "rtheta", "rq", "ru", "rw", "T", "p"), 1e-8)
    dq = np.abs(mu["qˡ"].interior_cpu() - g.interior(om.ql)).max()
    print(f"FLATAUSTEPS compressible {size} unfused={unfused} after {STEPS} steps:", worst, f"ql={dq:.1e}")
    assert dq < 1e-9


# ---- the entry point ------------------------------------------------------------------------------------------------------------------------------------
class _NoExchange:
    """the decomposition of a one-rank slab model that is never stepped"""
    rows = 0

    def exchange_y_halos(self, tensors):
        pass


def test_the_entry_point_refuses_what_it_does_not_run(bz):
    grid = bz.RectilinearGrid((16, 8, 8), x=(0, 1600.0), y=(0, 800.0), z=(0, 8e3))
    ref = bz.ReferenceState(grid, potential_temperature=300.0)
    warm = _adjustment(bz, False)
    vapor = bz.BulkVaporFlux(coefficient=1e-3, surface_temperature=300.0)
    layer = bz.BulkSensibleHeatFlux(coefficient=bz.PolynomialCoefficient(), surface_temperature=300.0)
    dyn = bz.CompressibleDynamics(bz.SplitExplicitTimeDiscretization(substeps=6))
    models = {
        "kinematic": bz.AtmosphereModel(grid, dynamics=bz.PrescribedDynamics(ref), advection=bz.WENO(order=5), microphysics=warm),
        "bulk vapour flux": bz.AtmosphereModel(grid, dynamics=bz.AnelasticDynamics(ref), advection=bz.WENO(order=5), microphysics=warm,
                                               boundary_conditions={"ρqᵛ": bz.FieldBoundaryConditions(bottom=vapor)}),
        "surface layer": bz.AtmosphereModel(grid, dynamics=bz.AnelasticDynamics(ref), advection=bz.WENO(order=5), microphysics=warm,
                                            boundary_conditions={"ρθ": bz.FieldBoundaryConditions(bottom=layer)}),
        "bulk vapour flux (compressible)": bz.CompressibleAtmosphereModel(grid, dyn, advection=bz.WENO(order=5), microphysics=warm,
                                                                          boundary_conditions={"ρqᵛ": vapor}),
        "y-slab": bz.compressible.SlabCompressibleModel(grid, 0, 1, bz.CompressibleDynamics(bz.SplitExplicitTimeDiscretization(substeps=6),
                                                                                             reference_potential_temperature=300.0),
                                                        advection=bz.WENO(order=5), device="cuda:0", decomp=_NoExchange()),
    }
    fp = bz.FlatauPolynomial()
    for name, m in models.items():
        P = m._T.bz_flatau_polynomial()
        for n in range(9):
            P.liquid_coefficients[n], P.ice_coefficients[n] = fp.liquid_coefficients[n], fp.ice_coefficients[n]
        P.reference_temperature, P.minimum_temperature_offset = fp.reference_temperature, fp.minimum_temperature_offset
        rc = m._lib.bz_set_saturation_vapor_pressure_polynomial(m._ctx, C.byref(P))
        assert rc == BZ_ERR_UNSUPPORTED, (name, rc)
        text = m._lib.bz_last_error(m._ctx).decode()
        assert "bz_set_saturation_vapor_pressure_polynomial" in text, (name, text)
        assert m._lib.bz_set_saturation_vapor_pressure_polynomial(m._ctx, None) == 0      # NULL is always accepted
    # the other order: a surface layer or a vapour flux handed to a context whose adjustment runs on the polynomial
    from breeze_jl_amd import _lib
    tc = _constants(bz)
    am = bz.AtmosphereModel(grid, dynamics=bz.AnelasticDynamics(ref), advection=bz.WENO(order=5), microphysics=warm, thermodynamic_constants=tc)
    cm = bz.CompressibleAtmosphereModel(grid, bz.CompressibleDynamics(bz.SplitExplicitTimeDiscretization(substeps=6)), advection=bz.WENO(order=5),
                                        microphysics=warm, thermodynamic_constants=tc)
    B = am._T.bz_bulk_surface_fluxes()
    B.vapor_coefficient, B.vapor_surface_temperature, B.surface_pressure, B.standard_pressure = 1e-3, 300.0, 101325.0, 1e5
    S = cm._T.bz_compressible_surface_fluxes()
    S.vapor.enabled, S.vapor.coefficient, S.vapor.surface_temperature, S.surface_pressure, S.standard_pressure = 1, 1e-3, 300.0, 1e5, 1e5
    for m, call, arg in ((am, "bz_set_bulk_surface_fluxes", B), (am, "bz_set_surface_layer", am._T.bz_surface_layer()),
                         (cm, "bz_set_compressible_surface_fluxes", S)):
        rc = getattr(m._lib, call)(m._ctx, C.byref(arg))
        text = m._lib.bz_last_error(m._ctx).decode()
        assert rc == BZ_ERR_UNSUPPORTED and call in text and "FlatauPolynomial" in text, (call, rc, text)
    B.vapor_coefficient, B.heat_coefficient, B.heat_surface_temperature = 0.0, 1e-3, 300.0          # drag and heat read no p^v+: accepted
    assert am._lib.bz_set_bulk_surface_fluxes(am._ctx, C.byref(B)) == 0 and am._lib.bz_set_bulk_surface_fluxes(am._ctx, None) == 0
    ok = bz.AtmosphereModel(grid, dynamics=bz.AnelasticDynamics(ref), advection=bz.WENO(order=5), microphysics=warm)
    P = ok._T.bz_flatau_polynomial()
    P.reference_temperature = float("nan")
    assert ok._lib.bz_set_saturation_vapor_pressure_polynomial(ok._ctx, C.byref(P)) == 1          # BZ_ERR_INVALID
