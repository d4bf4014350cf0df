"""SaturationAdjustment(equilibrium = MixedPhaseEquilibrium()) on CompressibleDynamics, on the device: the mixed instantiations of
k_cmp_diagnose<.., 4 | 5> and k_ac_stage_end<.., 4 | 5, double | float> (bz_ds_adjust_mixed of csrc/bz_internal.h) over the parcel sweep
of tests/mixed_phase_density_reference.py, whole steps against MixedCompressibleOracle, the switch back to the warm phase and the entry
point's refusals.

Judging of the sweeps (mpr.judge64 / judge32, unchanged; nothing of a bound comes from the device): Float64 T within max(1e-13, 16 d80)
relative, each fraction within max(1e-15, 16 d80) absolute, d80 the restatement's own float64-to-longdouble distance of the parcel's
population and solver; clear parcels: exact zeros in q^l and q^i and the bits of q^t in q^v; q^i (q^l) an exact zero where the iterate the
condensate was split at lies 4 K above T^f (below T^h); threshold parcels on either forced branch; theta = 0 exact; knife-edge parcels
skipped; rho, theta and q the restatement's bits; p within T's bound + 4 eps.  Float32 within 4 d32.
Steps: the bounds of tests/test_gpu_compressible.py::test_compressible_saturation_adjustment_matches_oracle and of the polynomial's
compressible step test — 1e-12 / 1e-13 after set!, 1e-8 / 1e-9 after the steps.

Measured on the MI355X (the maxima the tests print; fused and unfused stage ends gave the same figures):
    after set!                        state fields <= 1.1e-15 (rho_d, rho, rho theta, rho q: 0), q^v and q^l <= 1.1e-16, q^i <= 6.0e-18
    three steps, (16, 12, 12)         rho_d 1.6e-15 rtheta 1.7e-15 rq 2.1e-15 ru 2.7e-14 rw 1.9e-14 T 1.1e-15 p 1.8e-15; q^l 8.0e-17 q^i 9.1e-18
    three steps, (66, 6, 12)          rho_d 1.6e-15 rtheta 1.9e-15 rq 6.1e-15 ru 5.5e-14 rw 2.8e-14 T 1.3e-15 p 2.3e-15; q^l 1.3e-16 q^i 9.8e-18
    one step, SmagorinskyLilly        rho_d 8.0e-16 rtheta 5.1e-16 rq 1.5e-15 ru 1.6e-14 rw 2.1e-14 T 1.1e-15 p 1.2e-15; q^l 1.2e-16 q^i 7.6e-18
    one step, Float32 substep storage increments: rho_d 5.9e-8 rtheta 6.8e-8 rq 3.7e-8 ru 5.3e-8 rw 7.3e-9 T 2.5e-7 p 4.0e-8
    sweeps, Float64                   T within 1.0e-14 relative and the fractions within 9.4e-16 of the restatement (both under maxiter = 2,
                                      where the restatement's own d80 is 1.1e-14 / 9.3e-16; under the default solver 1.6e-15 / 1.4e-16)
    sweep, Float32                    498 parcels left out, 437 of 4314 cloudy ones (10.1 %; the warm density test: 440 of 3659, 12.0 %)"""
import ctypes as C

import numpy as np
import pytest

import instantaneous_precipitation_reference as ipr
import mixed_phase_density_reference as mdr
import mixed_phase_reference as mpr
import saturation_adjustment_reference as sar
from helpers import assert_increments

pytestmark = pytest.mark.gpu
F64, F32, LD = np.float64, np.float32, np.longdouble
SMALL, LARGE = sar.COMPRESSIBLE_GRIDS
NAN = float("nan")
EPS = float(np.finfo(F64).eps)
BZ_ERR_UNSUPPORTED = 2
ENTRY = "bz_set_compressible_mixed_phase_equilibrium"
WARM_F32_LEFT_OUT = 440 / 3659       # the share of cloudy parcels the warm Float32 density test leaves out (tests/test_flatau.py)


def _adjustment(bz, solver=sar.DEFAULT_SOLVER, mixed=True):
    eq = bz.MixedPhaseEquilibrium(freezing_temperature=mdr.TF, homogeneous_ice_nucleation_temperature=mdr.TH) if mixed else bz.WarmPhaseEquilibrium()
    return bz.SaturationAdjustment(equilibrium=eq, solver=bz.SecantSolver(abstol=solver[0], maxiter=solver[1]))


def _attach(bz, hm):
    """the mixed-phase form on a model built with the warm-phase adjustment (the constructor attaches the warm one: compressible.py)"""
    solver = hm.microphysics.solver
    bz.compressible.set_mixed_phase_equilibrium_(hm, bz.MixedPhaseEquilibrium(freezing_temperature=mdr.TF, homogeneous_ice_nucleation_temperature=mdr.TH))
    assert hm.microphysics.mixed_phase and hm.microphysics.solver is solver
    return hm


def _constants(bz, polynomial):
    return dict(thermodynamic_constants=bz.ThermodynamicConstants(saturation_vapor_pressure=bz.FlatauPolynomial())) if polynomial else {}


# ---- the sweeps: k_cmp_diagnose and k_ac_stage_end ------------------------------------------------------------------------------------------
def _model(bz, shape, solver=sar.DEFAULT_SOLVER, float_type=F64, polynomial=False, **kw):
    flat = shape[1] == 1
    ext = dict(x=(0.0, 100.0 * shape[0]), z=(0.0, 3e3)) if flat else dict(x=(0.0, 100.0 * shape[0]), y=(0.0, 100.0 * shape[1]), z=(0.0, 3e3))
    size, topo = ((shape[0], shape[2]), dict(topology=(bz.Periodic, bz.Flat, bz.Bounded), halo=(3, 3))) if flat else (shape, dict(halo=3))
    grid = bz.RectilinearGrid(size, float_type=float_type, **topo, **ext)
    dyn = bz.CompressibleDynamics(bz.SplitExplicitTimeDiscretization(substeps=6), surface_pressure=1e5, standard_pressure=sar.PST,
                                  reference_potential_temperature=ipr.theta_ref)
    hm = bz.CompressibleAtmosphereModel(grid, dyn, advection=bz.WENO(order=5), microphysics=_adjustment(bz, solver, mixed=False),
                                        temperature_solver=bz.NewtonSolver(abstol=sar.NEWTON[0], maxiter=sar.NEWTON[1]),
                                        **_constants(bz, polynomial), **kw)
    return _attach(bz, hm)


def _plant(hm, case):
    mu = hm.microphysical_fields
    assert list(mu) == ["qᵛ", "qˡ", "qⁱ", "qᵉ"] and mu["qᵉ"] is hm.specific_moisture
    fields = dict(rho_d=hm.dynamics.dry_density, rtheta=hm.potential_temperature_density, rq=hm.moisture_density)
    for n, f in fields.items():
        f.set_interior(case[n])
    for f in (hm.temperature, hm.dynamics.pressure, hm.dynamics.total_density, hm.specific_moisture, hm.potential_temperature, mu["qᵛ"], mu["qˡ"], mu["qⁱ"]):
        f.parent.fill_(NAN)
    return {n: f.interior.cpu().numpy() for n, f in fields.items()}


def _read(hm):
    hm.synchronize()
    mu = hm.microphysical_fields
    get = lambda f: f.interior.cpu().numpy()
    return dict(T=get(hm.temperature), p=get(hm.dynamics.pressure), q=get(hm.specific_moisture), rho=get(hm.dynamics.total_density),
                theta=get(hm.potential_temperature), qv=get(mu["qᵛ"]), ql=get(mu["qˡ"]), qi=get(mu["qⁱ"]))


def _halos_hold_the_images(hm):
    """q^i is stored as q^v and q^l are: periodic images in x and y, the z-halo copies of the bottom and top levels"""
    g, mu = hm.grid, hm.microphysical_fields
    for name in ("qᵛ", "qˡ", "qⁱ"):
        P = mu[name].parent.cpu().numpy()
        Hx, Hy, Hz, Nx, Ny, Nz = g.Hx, g.Hy, g.Hz, g.Nx, g.Ny, g.Nz
        I = P[Hz:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx]
        assert np.array_equal(P[Hz:Hz + Nz, Hy:Hy + Ny, Hx - 1], I[:, :, -1]) and np.array_equal(P[Hz:Hz + Nz, Hy:Hy + Ny, Hx + Nx], I[:, :, 0]), name
        if Hy:
            assert np.array_equal(P[Hz:Hz + Nz, Hy - 1, Hx:Hx + Nx], I[:, -1, :]) and np.array_equal(P[Hz:Hz + Nz, Hy + Ny, Hx:Hx + Nx], I[:, 0, :]), name
        assert np.array_equal(P[Hz - 1, Hy:Hy + Ny, Hx:Hx + Nx], I[0]) and np.array_equal(P[Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx], I[-1]), name


def _show(label, report, table, skipped=0):
    for name, row in report.items():
        d = table.get(name, (0.0,) * len(row))
        print(f"MIXEDDENSITY {label} {name}: device", " ".join(f"{v:.1e}" for v in row), "| restatement's own", " ".join(f"{v:.1e}" for v in d),
              f"| knife-edge skipped: {skipped}" if skipped else "")


def _judge(label, dev, want, tag, table, clear, cloudy):
    fails, report, skipped = mpr.judge64(dev, want, tag, table, clear, cloudy)
    _show(label, report, table, skipped)
    assert not fails, (label, fails)
    for n in ("rho", "q", "theta"):          # single IEEE operations on the inputs
        assert np.array_equal(dev[n], want[n]), (label, n)
    bT = sar.bounds64(tag, {k: v[:3] for k, v in table.items()})[0]
    ordinary = ~(want["knife"] | (tag == "marginal_edge")) & (want["T"] != 0)
    with np.errstate(all="ignore"):
        ep = np.abs(dev["p"] - want["p"]) / np.abs(want["p"])
    assert np.all(ep[ordinary] <= bT[ordinary] + 4 * EPS), (label, float(ep[ordinary].max()))
    assert np.all(dev["p"][want["branch"] == sar.THETA_ZERO] == 0) and np.isfinite(dev["p"]).all() and np.isfinite(dev["T"]).all()


SWEEPS = [(SMALL, s, False) for s in sar.SOLVERS] + [(LARGE, sar.DEFAULT_SOLVER, False), (SMALL, sar.DEFAULT_SOLVER, True), ((66, 1, 4), sar.DEFAULT_SOLVER, False)]


@pytest.mark.parametrize("shape,solver,polynomial", SWEEPS,
                         ids=[f"{s[0]}x{s[1]}x{s[2]}-secant{so[0]:g},{so[1]}" + ("-polynomial" if p else "") for s, so, p in SWEEPS])
def test_diagnosis_over_the_sweep(bz, shape, solver, polynomial):
    """update_state!(compute_tendencies = false): k_cmp_diagnose<true, false, 4> (polynomial: 5).  (66, 6, 4) holds a partly filled wavefront
    behind a full one and runs under every solver of sar.SOLVERS; (66, 1, 4) is the (Periodic, Flat, Bounded) model"""
    hm = _model(bz, shape, solver, polynomial=polynomial)
    case = mdr.mixed_density_case(shape, 0, polynomial)
    held = _plant(hm, case)
    for n, a in held.items():
        assert np.array_equal(a, case[n]), n
    bz.compressible.update_state_(hm, compute_tendencies=False)
    dev = _read(hm)
    _halos_hold_the_images(hm)
    R = lambda dtype, branch=None: mdr.restated(shape, dtype, solver, branch, 0, polynomial)
    _judge(f"k_cmp_diagnose {shape} secant={solver} polynomial={polynomial}", dev, R(F64), case.tag, mdr.d80(shape, solver, polynomial),
           R(F64, "clear"), R(F64, "cloudy"))
    warm = sar.diagnose_compressible(held, 1, F64, solver)
    assert np.nanmax(np.abs(dev["T"] - warm["T"])) > 1e-6


@pytest.mark.parametrize("substep_floattype", (None, F32), ids=("substeps-f64", "substeps-f32"))
def test_fused_step_leaves_the_restatement_of_its_fields(bz, substep_floattype):
    """time_step! (whole step, dt = 1e-3, 6 substeps) from the bulk sweep: the T, p, q^v, q^l, q^i read were written by the stage-end kernel of
    stage 3 (k_ac_stage_end<.., 4, double | float>; three launches of the slots acoustic_stage_end+update_state[+linearization]); k_cmp_diagnose
    ran once, in the update_state! that prepares the first step"""
    from test_saturation_adjustment_parcels import _winds
    shape = SMALL
    hm = _model(bz, shape, **({"substep_floattype": substep_floattype} if substep_floattype else {}))
    case = mdr.mixed_density_case(shape, bulk_only=True)
    _plant(hm, case)
    _winds(hm.grid, hm.momentum, case.rho_d)
    hm.profile_enable(True)
    hm.profile_reset()
    hm.time_step(1e-3)
    hm.synchronize()
    profile = hm.profile()
    print("MIXEDDENSITY step slots:", {k: v[1] for k, v in profile.items()})
    held = dict(rho_d=hm.dynamics.dry_density.interior.cpu().numpy(), rtheta=hm.potential_temperature_density.interior.cpu().numpy(),
                rq=hm.moisture_density.interior.cpu().numpy())
    dev = _read(hm)
    _halos_hold_the_images(hm)
    slot = lambda name: profile.get(name, (0.0, 0))[1]
    assert not np.array_equal(held["rtheta"], case.rtheta)
    assert slot("acoustic_stage_end+update_state") + slot("acoustic_stage_end+update_state+linearization") == 3
    assert slot("update_state") + slot("update_state+linearization") == 1 and not bz.diagnostics_stale(hm)
    want, wide = mdr.diagnose_mixed_density(held, F64), mdr.diagnose_mixed_density(held, LD)
    assert not want.nonfinite.any() and 0.2 <= np.mean(want.branch == sar.CLOUDY) <= 0.8          # (the condition is on the restatement)
    assert ((want["ql"] > 0) & (want["qi"] > 0)).any() and ((want["qi"] > 0) & (want["ql"] == 0)).any()
    _judge("k_ac_stage_end", dev, want, case.tag, mpr.own_distance(want, wide, case.tag), None, None)


def test_a_parcels_result_does_not_depend_on_its_wavefront(bz):
    """the same parcels under two placements (the second shuffles every level): the same bits per parcel"""
    outs = []
    for which in (0, 1):
        hm = _model(bz, LARGE)
        case = mdr.mixed_density_case(LARGE, which)
        _plant(hm, case)
        bz.compressible.update_state_(hm, compute_tendencies=False)
        dev = _read(hm)
        outs.append({n: mpr.by_parcel(case, dev[n]) for n in mpr.NAMES} | {"tag": mpr.by_parcel(case, case.tag)})
    assert np.array_equal(outs[0]["tag"], outs[1]["tag"])
    for n in mpr.NAMES:
        assert np.array_equal(outs[0][n], outs[1][n], equal_nan=True), (n, int((outs[0][n] != outs[1][n]).sum()))
    assert (outs[0]["qi"] > 0).any()


def test_float32_diagnosis_over_the_sweep(bz):
    """k_cmp_diagnose_f32<.., 4> on the Float32 grid at 4 d32 (mpr.judge32), with the knife-edge rule of flr.float32_knife_edge (condensate
    q^l + q^i): parcels whose float32 and float64 restatements of the same Float32 inputs stop on different branches or iteration counts,
    and cloudy parcels whose condensate is below what abstol resolves, are left out; their share of the cloudy parcels may not exceed the
    share the warm Float32 density test leaves out (440 of 3659)"""
    import torch
    solver = sar.DEFAULT_SOLVER
    hm = _model(bz, LARGE, float_type=F32)
    assert hm.temperature.parent.dtype == torch.float32
    case = mdr.mixed_density_case(LARGE)
    held = _plant(hm, case)
    assert all(a.dtype == F32 for a in held.values())
    bz.compressible.update_state_(hm, compute_tendencies=False)
    dev = _read(hm)
    diagnose = lambda dtype, branch=None: mdr.diagnose_mixed_density({n: a.astype(dtype) for n, a in held.items()}, dtype, solver, force_branch=branch)
    want32, want64 = diagnose(F32), diagnose(F64)
    out = mdr.float32_knife_edge(want32, want64, solver[0])
    cloudy = want64.branch == sar.CLOUDY
    assert all(np.isfinite(dev[n]).all() for n in mpr.NAMES)
    judged = dict(dev, **{n: np.where(out, want32[n], dev[n]) for n in mpr.NAMES})
    fails, report, table = mpr.judge32(judged, want32, want64, case.tag, float(np.abs(want64["q"]).max()), diagnose(F64, "clear"), diagnose(F64, "cloudy"))
    print(f"MIXEDDENSITY f32: left out {int(out.sum())} parcels, {int((out & cloudy).sum())} of {int(cloudy.sum())} cloudy ones", report, table)
    assert (out & cloudy).sum() <= WARM_F32_LEFT_OUT * cloudy.sum()
    assert not fails, fails
    assert np.array_equal(dev["q"], want32["q"]) and np.array_equal(dev["theta"], want32["theta"])


# ---- whole steps against MixedCompressibleOracle ---------------------------------------------------------------------------------------------------
STATE, STEPPED = ("rho_d", "rho", "rtheta", "rq", "T", "p"), ("rho_d", "rtheta", "rq", "ru", "rw", "T", "p")
FRACTIONS = {"qv": "qᵛ", "ql": "qˡ", "qi": "qⁱ"}


def _device_model(bz, size, mixed=True, **kw):
    grid = bz.RectilinearGrid(size, **mdr.STEP_EXTENT[size])
    dyn = bz.CompressibleDynamics(bz.SplitExplicitTimeDiscretization(substeps=mdr.STEP_SUBSTEPS), surface_pressure=1e5, reference_potential_temperature=300.0)
    hm = bz.CompressibleAtmosphereModel(grid, dyn, advection=bz.WENO(order=5), microphysics=_adjustment(bz, mixed=False), **kw)
    return _attach(bz, hm) if mixed else hm


def _set(oracle, oc, hm, size, sheared=False):
    om = mdr.oracle_model(oracle, oc, size)          # (for its grid and reference columns: nothing is stepped)
    rho, theta, qt = mdr.step_state(om)
    hm.set(ρ=rho, θ=theta, u=mdr.step_wind(om, sheared), v=0.0, w=0.0, qᵗ=qt)


def _device_fields(hm):
    from test_gpu_compressible import O2H
    hm.synchronize()
    out = {n: O2H[n](hm).interior_cpu().astype(F64) for n in ("rho_d", "rho", "rtheta", "rq", "ru", "rv", "rw", "T", "p")}
    out.update({n: hm.microphysical_fields[k].interior_cpu().astype(F64) for n, k in FRACTIONS.items()})
    return out


def _compare(label, got, want, names, tol, qnames, qtol):
    errs = mdr.scaled_errors(got, want, names)
    dq = {n: float(np.abs(got[n] - want[n]).max()) for n in qnames}
    print(f"MIXEDDENSITYSTEPS {label}:", " ".join(f"{n}={e:.1e}" for n, e in errs.items()), "|", " ".join(f"{n}={e:.1e}" for n, e in dq.items()))
    assert all(e <= tol for e in errs.values()) and all(e < qtol for e in dq.values()), (label, errs, dq)


def _every_regime(label, f):
    shares = mdr.regime_shares(f["ql"], f["qi"])
    assert min(shares) >= mdr.MIN_REGIME_SHARE, (label, dict(zip(mdr.REGIMES, shares)))


@pytest.mark.parametrize("size", mdr.STEP_SHAPES, ids=str)
@pytest.mark.parametrize("unfused", (False, True), ids=("fused-stage-end", "unfused-stage-end"))
def test_three_steps_match_the_oracle(oracle, oc, bz, monkeypatch, unfused, size):
    """the moist bubble in a 10 km column that crosses T^f and T^h, 6 substeps, dt = 1: on the fused stage epilogue (k_ac_stage_end<.., 4, ..>)
    and with BZ_NO_AC_END_FUSE=1 (k_cmp_diagnose<.., 4> after every stage)"""
    monkeypatch.delenv("BZ_NO_AC_END_FUSE", raising=False)
    if unfused:
        monkeypatch.setenv("BZ_NO_AC_END_FUSE", "1")
    start, want = mdr.oracle_steps(oracle, oc, size)
    _every_regime("start", start)
    _every_regime("end", want)
    hm = _device_model(bz, size)
    _set(oracle, oc, hm, size)
    _compare(f"{size} unfused={unfused} after set", _device_fields(hm), start, STATE, 1e-12, FRACTIONS, 1e-13)
    hm.profile_enable(True)
    hm.profile_reset()
    for _ in range(mdr.STEP_COUNT):
        hm.time_step(mdr.STEP_DT)
    slots = {k: v[1] for k, v in hm.profile().items()}
    fused = slots.get("acoustic_stage_end+update_state", 0) + slots.get("acoustic_stage_end+update_state+linearization", 0)
    assert (fused == 0) if unfused else (fused == 3 * mdr.STEP_COUNT), slots
    got = _device_fields(hm)
    _compare(f"{size} unfused={unfused} after {mdr.STEP_COUNT} steps", got, want, STEPPED, 1e-8, ("ql", "qi"), 1e-9)
    _every_regime("device", got)


def test_one_step_with_smagorinsky_lilly(oracle, oc, bz):
    """closure = SmagorinskyLilly() in a sheared wind against the oracle with the closure (compressible_closure_reference), the bounds of the
    three-step test"""
    size = mdr.STEP_SHAPES[0]
    start, want = mdr.oracle_steps(oracle, oc, size, steps=1, smagorinsky=True)
    assert want["nu_e_max"] > 0.1
    hm = _device_model(bz, size, closure=bz.SmagorinskyLilly())
    _set(oracle, oc, hm, size, sheared=True)
    _compare("smagorinsky after set", _device_fields(hm), start, STATE, 1e-12, FRACTIONS, 1e-13)
    hm.time_step(mdr.STEP_DT)
    got = _device_fields(hm)
    _compare("smagorinsky after one step", got, want, STEPPED, 1e-8, ("ql", "qi"), 1e-9)
    assert float(hm.closure_fields["νₑ"].interior.max().item()) > 0.1 and min(mdr.regime_shares(got["ql"], got["qi"])) > 0


def test_one_step_with_float32_substep_storage(oracle, oc, bz):
    """substep_floattype = Float32 inside the Float64 model (k_ac_stage_end<.., 4, float>): no oracle stores its working fields in Float32, so
    the step is judged by its increments against the Float64 oracle (helpers.F32_INCREMENT_TOL["substep_storage"])"""
    size = mdr.STEP_SHAPES[0]
    start, want = mdr.oracle_steps(oracle, oc, size, steps=1)
    hm = _device_model(bz, size, substep_floattype=F32)
    _set(oracle, oc, hm, size)
    _compare("f32 substeps after set", _device_fields(hm), start, STATE, 1e-12, FRACTIONS, 1e-13)
    hm.time_step(mdr.STEP_DT)
    got = _device_fields(hm)
    assert_increments("mixed-phase bubble, Float32 substep storage", {n: got[n] for n in STEPPED}, want, start, "substep_storage")
    assert np.abs(got["qi"] - want["qi"]).max() < 1e-7 and min(mdr.regime_shares(got["ql"], got["qi"])) > 0


# ---- the entry point ------------------------------------------------------------------------------------------------------------------------------------
def test_null_returns_the_context_to_the_warm_phase(oracle, oc, bz, monkeypatch):
    """bz_set_compressible_mixed_phase_equilibrium(NULL) on a context that had the mixed phase attached: three steps bit-identical to a model
    built with WarmPhaseEquilibrium(), q^i filled with NaN and never touched"""
    monkeypatch.delenv("BZ_NO_AC_END_FUSE", raising=False)
    size = mdr.STEP_SHAPES[0]
    hm, warm, mixed = _device_model(bz, size), _device_model(bz, size, mixed=False), _device_model(bz, size)
    hm._check(getattr(hm._lib, ENTRY)(hm._ctx, None, None), ENTRY)
    hm.microphysical_fields["qⁱ"].parent.fill_(NAN)
    outs = []
    for m in (hm, warm, mixed):
        _set(oracle, oc, m, size)
        for _ in range(mdr.STEP_COUNT):
            m.time_step(mdr.STEP_DT)
        from test_gpu_compressible import O2H
        m.synchronize()
        outs.append({n: O2H[n](m).interior_cpu() for n in ("rho_d", "rho", "rtheta", "rq", "ru", "rv", "rw", "T", "p")} |
                    {n: m.microphysical_fields[k].interior_cpu() for n, k in (("qv", "qᵛ"), ("ql", "qˡ"))})
    for k in outs[0]:
        assert np.isfinite(outs[0][k]).all() and np.array_equal(outs[0][k], outs[1][k]), k
    assert (outs[0]["ql"] > 0).any() and not np.array_equal(outs[0]["T"], outs[2]["T"])
    assert np.isnan(hm.microphysical_fields["qⁱ"].parent.cpu().numpy()).all()


class _NoExchange:
    """the decomposition of a one-rank slab model that is never stepped"""
    rows = 0

    def exchange_y_halos(self, tensors):
        pass


def test_the_entry_point_refuses_what_it_does_not_run(bz):
    grid = bz.RectilinearGrid((16, 8, 8), x=(0, 1600.0), y=(0, 800.0), z=(0, 8e3))
    walled = bz.RectilinearGrid((16, 8, 8), x=(0, 1600.0), y=(0, 800.0), z=(0, 8e3), topology=(bz.Periodic, bz.Bounded, bz.Bounded))
    ref = bz.ReferenceState(grid, potential_temperature=300.0)
    warm = bz.SaturationAdjustment(equilibrium=bz.WarmPhaseEquilibrium())
    dyn = lambda **kw: bz.CompressibleDynamics(bz.SplitExplicitTimeDiscretization(substeps=6), **kw)
    cm = lambda g=grid, **kw: bz.CompressibleAtmosphereModel(g, dyn(), advection=bz.WENO(order=5), **kw)
    heat = bz.BulkSensibleHeatFlux(coefficient=1e-3, surface_temperature=300.0)
    tetens = bz.ThermodynamicConstants(saturation_vapor_pressure=bz.TetensFormula())
    models = {
        "anelastic": (bz.AtmosphereModel(grid, dynamics=bz.AnelasticDynamics(ref), advection=bz.WENO(order=5), microphysics=warm), "bz_create_compressible"),
        "kinematic": (bz.AtmosphereModel(grid, dynamics=bz.PrescribedDynamics(ref), advection=bz.WENO(order=5), microphysics=warm), "kinematic"),
        "y-slab": (bz.compressible.SlabCompressibleModel(grid, 0, 1, dyn(reference_potential_temperature=300.0), advection=bz.WENO(order=5),
                                                         device="cuda:0", decomp=_NoExchange()), "y-slab"),
        "walls": (cm(walled), "Bounded"),
        "Kessler": (cm(microphysics=bz.DCMIP2016KesslerMicrophysics(), thermodynamic_constants=tetens), "Kessler"),
        "InstantaneousPrecipitation": (cm(microphysics=bz.InstantaneousPrecipitation()), "InstantaneousPrecipitation"),
        "bulk surface fluxes": (cm(microphysics=warm, boundary_conditions={"ρθ": heat}), "surface fluxes"),
        "no adjustment": (cm(), "SaturationAdjustment"),
    }
    for name, (m, word) in models.items():
        P = m._T.bz_mixed_phase_equilibrium(mpr.TF, mpr.TH, 2834000.0, 2108.0)
        buf = m.temperature          # any device array of the grid's size stands in for q^i: the call must refuse before it keeps it
        rc = getattr(m._lib, ENTRY)(m._ctx, C.byref(P), C.c_void_p(buf.ptr()))
        text = m._lib.bz_last_error(m._ctx).decode()
        assert rc == BZ_ERR_UNSUPPORTED and ENTRY in text and word in text, (name, rc, text)
        assert getattr(m._lib, ENTRY)(m._ctx, None, None) == 0      # NULL is always accepted
    # the other order: bulk surface fluxes handed to a context whose adjustment is mixed-phase
    mixed = _attach(bz, cm(microphysics=warm))
    S = mixed._T.bz_compressible_surface_fluxes()
    S.heat.enabled, S.heat.coefficient, S.heat.surface_temperature, S.surface_pressure, S.standard_pressure = 1, 1e-3, 300.0, 1e5, 1e5
    rc = mixed._lib.bz_set_compressible_surface_fluxes(mixed._ctx, C.byref(S))
    text = mixed._lib.bz_last_error(mixed._ctx).decode()
    assert rc == BZ_ERR_UNSUPPORTED and "bz_set_compressible_surface_fluxes" in text and "MixedPhaseEquilibrium" in text, (rc, text)
    assert mixed._lib.bz_set_compressible_surface_fluxes(mixed._ctx, None) == 0
    # the host function refuses what the entry point refuses, by name and before the context is touched; an invalid pair of kinks is an argument error
    assert "qⁱ" in mixed.microphysical_fields
    eq = bz.MixedPhaseEquilibrium()
    for name in ("walls", "Kessler", "InstantaneousPrecipitation", "bulk surface fluxes", "no adjustment", "y-slab"):
        with pytest.raises(NotImplementedError, match="MixedPhaseEquilibrium"):
            bz.compressible.set_mixed_phase_equilibrium_(models[name][0], eq)
    with pytest.raises(TypeError):
        bz.compressible.set_mixed_phase_equilibrium_(models["anelastic"][0], eq)
    # ... and returns a model to the warm phase
    bz.compressible.set_mixed_phase_equilibrium_(mixed, bz.WarmPhaseEquilibrium())
    assert "qⁱ" not in mixed.microphysical_fields and not mixed.microphysics.mixed_phase
    _attach(bz, mixed)
    P = mixed._T.bz_mixed_phase_equilibrium(mpr.TH, mpr.TF, 2834000.0, 2108.0)
    assert getattr(mixed._lib, ENTRY)(mixed._ctx, C.byref(P), C.c_void_p(mixed.microphysical_fields["qⁱ"].ptr())) == 1
