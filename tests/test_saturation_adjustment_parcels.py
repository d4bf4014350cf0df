"""The per-cell thermodynamic inversions of the device (bz_sa_diagnose, bz_ds_adjust, bz_ds_temperature, the Newton loops written out in
k_cmp_diagnose and in the stage-end kernel, bz_exner_factor / bz_exp_small) over the parcel sweeps of tests/saturation_adjustment_reference.py,
against that module's typed restatement (pinned to oracle/thermo.py bit for bit by tests/test_saturation_adjustment_reference.py).

Inputs are the prognostic arrays written into the model's fields (not set!); the restatement starts from the arrays read back from the
device and repeats the kernels' first lines, so both sides start from the same bits.  p_r, rho_r and p_st are the device model's.

Judging (saturation_adjustment_reference.judge64 / judge32; nothing of a bound comes from the device):
  Float64   ordinary parcels: T within max(1e-13, 16 d80) relative, q^v and q^l within max(1e-15, 16 d80) absolute, d80 the restatement's own
            float64-against-longdouble distance of the parcel's population, solver and form; clear parcels and negative q^t: q^l an exact
            zero and q^v the bits of q^t; threshold parcels (delta in {0, +-2^-52}): on either forced branch; knife-edge parcels skipped (at
            most 0.5 % of the cloudy ones, asserted on the CPU); theta = 0: exact.  Compressible: p within the bound of T plus 4 eps, the
            stored q and rho the restatement's bits.
  Float32   within 4 d32 per population, floors 4 ulp of T and 4 x 2^-24 max q^t; a parcel the float32 restatement itself puts on the other
            branch, or a marginal one, passes on either forced branch."""
import numpy as np
import pytest

import instantaneous_precipitation_reference as ipr
import saturation_adjustment_reference as sar

pytestmark = pytest.mark.gpu
F64, F32 = np.float64, np.float32
EPS = float(np.finfo(F64).eps)
SMALL, LARGE = sar.COMPRESSIBLE_GRIDS
A_SMALL, A_LARGE = sar.ANELASTIC_GRIDS
NAN = float("nan")


def _ext(shape, Lz):
    return dict(x=(0.0, 100.0 * shape[0]), y=(0.0, 100.0 * shape[1]), z=(0.0, float(Lz)))


def _microphysics(bz, mp, solver):
    if mp == 1:
        return bz.SaturationAdjustment(equilibrium=bz.WarmPhaseEquilibrium(), solver=bz.SecantSolver(abstol=solver[0], maxiter=solver[1])), None
    if mp == 2:
        return bz.DCMIP2016KesslerMicrophysics(), bz.ThermodynamicConstants(saturation_vapor_pressure=bz.TetensFormula())
    return None, None


def _compressible(bz, shape, mp, solver=sar.DEFAULT_SOLVER, newton=sar.NEWTON, float_type=F64):
    grid = bz.RectilinearGrid(shape, halo=3, float_type=float_type, **_ext(shape, 3e3))
    dyn = bz.CompressibleDynamics(bz.SplitExplicitTimeDiscretization(substeps=6), surface_pressure=1e5, standard_pressure=sar.PST,
                                  reference_potential_temperature=ipr.theta_ref)
    micro, tc = _microphysics(bz, mp, solver)
    return bz.CompressibleAtmosphereModel(grid, dyn, advection=bz.WENO(order=5), microphysics=micro, thermodynamic_constants=tc,
                                          temperature_solver=bz.NewtonSolver(abstol=newton[0], maxiter=newton[1]))


def _anelastic(bz, shape, mp, Lz=sar.COLUMN, solver=sar.DEFAULT_SOLVER, float_type=F64):
    grid = bz.RectilinearGrid(shape, halo=3, float_type=float_type, **_ext(shape, Lz))
    ref = bz.ReferenceState(grid, surface_pressure=sar.SURFACE_PRESSURE, potential_temperature=sar.THETA_0, standard_pressure=sar.PST)
    micro, tc = _microphysics(bz, mp, solver)
    hm = bz.AtmosphereModel(grid, dynamics=bz.AnelasticDynamics(ref), advection=bz.WENO(order=5), microphysics=micro, thermodynamic_constants=tc)
    p_r, rho_r = _columns(hm)
    assert p_r.dtype == float_type and ref.standard_pressure == sar.PST
    if float_type is F64:            # the columns the sweeps were realised on (and the cached restatements evaluated on): the device's, bit for bit
        want_p, want_rho = sar.reference_column(shape[2], Lz)
        assert np.array_equal(p_r, want_p) and np.array_equal(rho_r, want_rho)
    return hm


def _columns(hm):
    """p_r and rho_r of the model's reference state as the model handed them to the device, in its own element type"""
    rho, p = hm._ref_arrays[0], hm._ref_arrays[1]
    Hz, Nz = hm.grid.Hz, hm.grid.Nz
    return p[Hz:Hz + Nz].copy(), rho[Hz:Hz + Nz].copy()


def _plant_compressible(hm, case, mp):
    """the case's arrays into the prognostic fields; every diagnostic the launch must write is poisoned.  -> the arrays the device holds"""
    mu = hm.microphysical_fields
    fields = dict(rho_d=hm.dynamics.dry_density, rtheta=hm.potential_temperature_density, rq=hm.moisture_density)
    if mp == 2:
        fields.update(rqcl=mu["ρqᶜˡ"], rqr=mu["ρqʳ"])
    for n, f in fields.items():
        f.set_interior(case[n])
    for f in (hm.temperature, hm.dynamics.pressure, hm.dynamics.total_density, hm.specific_moisture, hm.potential_temperature):
        f.parent.fill_(NAN)
    if mp == 1:
        mu["qᵛ"].parent.fill_(NAN)
        mu["qˡ"].parent.fill_(NAN)
    return {n: f.interior.cpu().numpy() for n, f in fields.items()}


def _read_compressible(hm, mp):
    hm.synchronize()
    mu = hm.microphysical_fields
    out = dict(T=hm.temperature.interior.cpu().numpy(), p=hm.dynamics.pressure.interior.cpu().numpy(), q=hm.specific_moisture.interior.cpu().numpy(),
               rho=hm.dynamics.total_density.interior.cpu().numpy(), theta=hm.potential_temperature.interior.cpu().numpy())
    if mp == 1:
        out.update(qv=mu["qᵛ"].interior.cpu().numpy(), ql=mu["qˡ"].interior.cpu().numpy())
    elif mp == 2:
        out.update(qv=mu["qᵛ"].interior.cpu().numpy(), ql=None, qcl=mu["qᶜˡ"].interior.cpu().numpy(), qr=mu["qʳ"].interior.cpu().numpy())
    else:
        out.update(qv=out["q"], ql=np.zeros_like(out["q"]))
    return out


def _plant_anelastic(hm, case, mp):
    mu = hm.microphysical_fields
    fields = dict(rtheta=hm.potential_temperature_density, rq=hm.moisture_density)
    if mp == 2:
        fields.update(qcl=mu["qᶜˡ"], qr=mu["qʳ"], rqcl=mu["ρqᶜˡ"], rqr=mu["ρqʳ"])
    for n, f in fields.items():
        f.set_interior(case[n])
    for f in (hm.temperature, hm.specific_moisture, hm.potential_temperature):
        f.parent.fill_(NAN)
    if mp == 1:
        mu["qᵛ"].parent.fill_(NAN)
        mu["qˡ"].parent.fill_(NAN)
    return {n: f.interior.cpu().numpy() for n, f in fields.items()}


def _read_anelastic(hm, mp):
    hm.synchronize()
    mu = hm.microphysical_fields
    out = dict(T=hm.temperature.interior.cpu().numpy(), q=hm.specific_moisture.interior.cpu().numpy(), theta=hm.potential_temperature.interior.cpu().numpy())
    if mp == 1:
        out.update(qv=mu["qᵛ"].interior.cpu().numpy(), ql=mu["qˡ"].interior.cpu().numpy())
    elif mp == 2:
        out.update(qv=mu["qᵛ"].interior.cpu().numpy(), ql=None, qcl=mu["qᶜˡ"].interior.cpu().numpy(), qr=mu["qʳ"].interior.cpu().numpy())
    else:
        out.update(qv=out["q"], ql=np.zeros_like(out["q"]))
    return out


def _show(label, report, table, skipped=0):
    for name, row in report.items():
        d = table.get(name, (0.0, 0.0, 0.0))
        print(f"SAPARCELS {label} {name}: device T={row[0]:.1e} qv={row[1]:.1e} ql={row[2]:.1e} | restatement's own T={d[0]:.1e} qv={d[1]:.1e} "
              f"ql={d[2]:.1e}" + (f" | knife-edge skipped: {skipped}" if skipped else ""))


def _judge64(label, dev, want, tag, table, forced=None, adjusted=True):
    """the Float64 rules on (T, q^v, q^l); `forced`: callable branch -> restatement, evaluated only where threshold parcels exist"""
    if dev["ql"] is None:            # Kessler: the condensate is an input; T alone is diagnosed
        dev = dict(dev, ql=want["ql"])
    clear = cloudy = None
    if adjusted and forced is not None and (tag == "marginal_edge").any():
        clear, cloudy = forced("clear"), forced("cloudy")
    fails, report, skipped = sar.judge64(dev, want, tag, table, clear, cloudy, adjusted)
    _show(label, report, table, skipped)
    assert not fails, (label, fails)
    return report


def _compressible_extras(label, dev, want, tag, table, mp):
    """rho, theta and the stored q are single IEEE operations on the inputs: the restatement's bits; p = rho R_m T within T's bound + 4 eps"""
    for n in ("rho", "q") + (("qcl", "qr") if mp == 2 else ()):
        assert np.array_equal(dev[n], want[n]), (label, n)
    live = want["branch"] != sar.THETA_ZERO
    assert np.array_equal(dev["theta"], want["theta"])
    bT = sar.bounds64(tag, table)[0]
    ordinary = ~(want["knife"] | (tag == "marginal_edge")) & (want["T"] != 0)
    with np.errstate(all="ignore"):
        ep = np.abs(dev["p"] - want["p"]) / np.abs(want["p"])
    assert np.all(ep[ordinary] <= bT[ordinary] + 4 * EPS), (label, float(ep[ordinary].max()))
    if mp != 2:                      # theta = 0 (with Kessler's condensate T is the latent term, not 0)
        assert np.all(dev["p"][~live] == 0)
    assert np.isfinite(dev["p"]).all() and np.isfinite(dev["T"]).all()


# ---- A2: k_cmp_diagnose ----------------------------------------------------------------------------------------------------------------------
A2 = ([(SMALL, 0, sar.DEFAULT_SOLVER, sar.NEWTON), (LARGE, 0, sar.DEFAULT_SOLVER, sar.NEWTON), (SMALL, 2, sar.DEFAULT_SOLVER, sar.NEWTON),
       (LARGE, 2, sar.DEFAULT_SOLVER, sar.NEWTON)]
      + [(shape, 1, solver, sar.NEWTON) for shape in (SMALL, LARGE) for solver in sar.SOLVERS] + [(SMALL, 1, (1e-4, 1), sar.NEWTON)]
      + [(SMALL, mp, sar.DEFAULT_SOLVER, newton) for mp in (1, 0, 2) for newton in sar.LOOSE_NEWTONS])


@pytest.mark.parametrize("shape,mp,solver,newton", A2, ids=[f"{s[0]}x{s[1]}x{s[2]}-MP{m}-secant{so[0]:g},{so[1]}-newton{n[0]:g},{n[1]}" for s, m, so, n in A2])
def test_compressible_diagnosis_over_the_sweep(bz, shape, mp, solver, newton):
    """update_state!(compute_tendencies = false) of the compressible model: k_cmp_diagnose<MP> (MP = 1: bz_ds_adjust around bz_ds_temperature;
    MP = 0, 2: the Newton loop written out in the kernel).  Secant solvers: the default, maxiter = 0, 1, 2 (the maxiter exit) and abstol = 0
    (run until the `valid` guard fires); temperature solvers: (1e-4, 8), and on the small grid under the default secant (1e-4, 0) (no
    iteration: T is the first guess), (1e-4, 1) and (1, 8), which leave on maxiter or on abstol = 1 K long before convergence, where a Newton
    loop that ignores either bound, or always takes a step, gives another answer."""
    hm = _compressible(bz, shape, mp, solver, newton)
    case = sar.compressible_case(shape)
    held = _plant_compressible(hm, case, mp)
    for n, a in held.items():
        assert np.array_equal(a, case[n]), n
    bz.compressible.update_state_(hm, compute_tendencies=False)
    dev = _read_compressible(hm, mp)
    want = sar.restated("density", shape, mp, F64, solver, newton=newton)
    table = sar.d80("density", shape, mp, solver, newton=newton)
    label = f"cmp {shape} MP={mp} secant={solver} newton={newton}"
    _judge64(label, dev, want, case.tag, table, lambda b: sar.restated("density", shape, mp, F64, solver, b, newton=newton), mp == 1)
    _compressible_extras(label, dev, want, case.tag, table, mp)


# ---- A1: k_thermo ----------------------------------------------------------------------------------------------------------------------------
A1 = [(A_SMALL, 0, sar.TALL_COLUMN), (A_LARGE, 0, sar.TALL_COLUMN), (A_SMALL, 1, sar.COLUMN), (A_LARGE, 1, sar.COLUMN), (A_SMALL, 2, sar.COLUMN),
      (A_LARGE, 2, sar.COLUMN)]


@pytest.mark.parametrize("shape,mp,Lz", A1, ids=[f"{s[0]}x{s[1]}x{s[2]}-MP{m}" for s, m, _ in A1])
def test_anelastic_diagnosis_over_the_sweep(bz, shape, mp, Lz):
    """update_state!(compute_tendencies = false) of the anelastic model: k_thermo.  microphysics = nothing takes bz_exner_factor on the 24 km
    column with the exp_small population (0, 1 and 2 halvings of bz_exp_small among ordinary lanes of the top level); SaturationAdjustment is
    bz_sa_diagnose, Kessler bz_kessler_T with the planted, lagged condensate (the diagnostic q^cl, q^r of before the launch), after which the
    launch refreshes them from the planted densities."""
    exp_small = mp == 0
    hm = _anelastic(bz, shape, mp, Lz)
    case = sar.anelastic_case(shape, Lz, 0, exp_small)
    held = _plant_anelastic(hm, case, mp)
    for n, a in held.items():
        assert np.array_equal(a, case[n]), n
    bz.update_state_(hm, compute_tendencies=False)
    dev = _read_anelastic(hm, mp)
    want = sar.restated("pressure", shape, mp, F64, Lz=Lz, exp_small=exp_small)
    table = sar.d80("pressure", shape, mp, Lz=Lz, exp_small=exp_small)
    label = f"anelastic {shape} MP={mp}"
    _judge64(label, dev, want, case.tag, table, lambda b: sar.restated("pressure", shape, mp, F64, sar.DEFAULT_SOLVER, b, Lz=Lz, exp_small=exp_small),
             mp == 1)
    assert np.array_equal(dev["q"], want["q"]) and np.array_equal(dev["theta"], want["theta"])
    if mp == 2:
        col = case.rho_r[:, None, None]
        assert np.array_equal(dev["qcl"], case.rqcl / col) and np.array_equal(dev["qr"], case.rqr / col)
    if exp_small:
        sel = case.tag == "exp_small"
        assert set(want.halvings[sel]) == {0, 1, 2}


@pytest.mark.parametrize("solver", [(0.0, 50), (1e-4, 2), (1e-4, 0)], ids=["abstol0", "maxiter2", "maxiter0"])
def test_anelastic_saturation_adjustment_under_other_solvers(bz, solver):
    """bz_sa_diagnose under SecantSolver(abstol = 0, maxiter = 50) (run until the `valid` guard fires: every parcel is judged, whatever its
    iteration count) and under maxiter = 2 and 0 (the maxiter exit)"""
    shape = A_SMALL
    hm = _anelastic(bz, shape, 1, solver=solver)
    case = sar.anelastic_case(shape)
    _plant_anelastic(hm, case, 1)
    bz.update_state_(hm, compute_tendencies=False)
    dev = _read_anelastic(hm, 1)
    want = sar.restated("pressure", shape, 1, F64, solver)
    _judge64(f"anelastic {shape} MP=1 secant={solver}", dev, want, case.tag, sar.d80("pressure", shape, 1, solver),
             lambda b: sar.restated("pressure", shape, 1, F64, solver, b))


# ---- A3: the Float32 twins ---------------------------------------------------------------------------------------------------------------------
def _judge32(label, dev, tag, diagnose):
    """diagnose(dtype, force_branch) -> restatement of the device's own (Float32) inputs"""
    want32, want64 = diagnose(F32, None), diagnose(F64, None)
    clear = cloudy = want64          # without an adjustment there are no branches
    if (want64.branch == sar.CLOUDY).any():
        clear, cloudy = diagnose(F64, "clear"), diagnose(F64, "cloudy")
    if dev["ql"] is None:            # Kessler: the condensate is an input
        dev = dict(dev, ql=want32["ql"])
    assert dev["T"].dtype == F32
    fails, report, table = sar.judge32(dev, want32, want64, tag, float(np.abs(want64["q"]).max()), clear, cloudy)
    _show(label, report, table)
    assert not fails, (label, fails)
    assert np.array_equal(dev["q"], want32["q"]) and np.array_equal(dev["theta"], want32["theta"])


@pytest.mark.parametrize("mp,abstol", [(0, 1e-4), (2, 1e-4), (1, 1e-4), (1, 1e-6), (1, 0.0)], ids=["MP0", "MP2", "MP1-1e-4", "MP1-1e-6", "MP1-0"])
def test_float32_compressible_diagnosis_over_the_sweep(bz, mp, abstol):
    import torch
    solver = (abstol, 20)
    hm = _compressible(bz, LARGE, mp, solver, float_type=F32)
    assert hm.temperature.parent.dtype == torch.float32
    case = sar.compressible_case(LARGE)
    held = _plant_compressible(hm, case, mp)
    assert all(a.dtype == F32 for a in held.values())
    bz.compressible.update_state_(hm, compute_tendencies=False)
    dev = _read_compressible(hm, mp)

    def diagnose(dtype, branch):
        return sar.diagnose_compressible({n: a.astype(dtype) for n, a in held.items()}, mp, dtype, solver, force_branch=branch)

    _judge32(f"f32 cmp MP={mp} abstol={abstol:g}", dev, case.tag, diagnose)


@pytest.mark.parametrize("mp,abstol", [(0, 1e-4), (2, 1e-4), (1, 1e-4), (1, 1e-6), (1, 0.0)], ids=["MP0", "MP2", "MP1-1e-4", "MP1-1e-6", "MP1-0"])
def test_float32_anelastic_diagnosis_over_the_sweep(bz, mp, abstol):
    import torch
    solver, Lz = (abstol, 20), (sar.TALL_COLUMN if mp == 0 else sar.COLUMN)
    hm = _anelastic(bz, A_LARGE, mp, Lz, solver, float_type=F32)
    assert hm.temperature.parent.dtype == torch.float32
    case = sar.anelastic_case(A_LARGE, Lz, 0, mp == 0)
    held = _plant_anelastic(hm, case, mp)
    bz.update_state_(hm, compute_tendencies=False)
    dev = _read_anelastic(hm, mp)
    p32, rho32 = _columns(hm)

    def diagnose(dtype, branch):
        return sar.diagnose_anelastic({n: a.astype(dtype) for n, a in held.items()}, mp, p32.astype(dtype), rho32.astype(dtype), dtype, solver, branch)

    _judge32(f"f32 anelastic MP={mp} abstol={abstol:g}", dev, case.tag, diagnose)


# ---- lane independence ---------------------------------------------------------------------------------------------------------------------------
def _by_parcel(case, field):
    return field.ravel()[np.argsort(case.parcel.ravel())]


@pytest.mark.parametrize("model,mp", [("anelastic", 0), ("anelastic", 1), ("compressible", 1)], ids=["anelastic-nothing", "anelastic-SA", "compressible-SA"])
def test_a_parcels_result_does_not_depend_on_its_wavefront(bz, model, mp):
    """The same parcels under two placements (the second shuffles every level) on (130, 9, 6): the same bits per parcel.  The anelastic
    model without microphysics runs the tall column with the exp_small lanes, whose halving count must stay a lane's own."""
    outs = []
    for which in (0, 1):
        if model == "anelastic":
            Lz = sar.TALL_COLUMN if mp == 0 else sar.COLUMN
            hm = _anelastic(bz, A_LARGE, mp, Lz)
            case = sar.anelastic_case(A_LARGE, Lz, which, mp == 0)
            _plant_anelastic(hm, case, mp)
            bz.update_state_(hm, compute_tendencies=False)
            dev = _read_anelastic(hm, mp)
        else:
            hm = _compressible(bz, LARGE, mp)
            case = sar.compressible_case(LARGE, which)
            _plant_compressible(hm, case, mp)
            bz.compressible.update_state_(hm, compute_tendencies=False)
            dev = _read_compressible(hm, mp)
        outs.append({n: _by_parcel(case, dev[n]) for n in ("T", "qv", "ql")} | {"tag": _by_parcel(case, case.tag)})
    assert np.array_equal(outs[0]["tag"], outs[1]["tag"])
    for n in ("T", "qv", "ql"):
        assert np.array_equal(outs[0][n], outs[1][n]), (n, int((outs[0][n] != outs[1][n]).sum()))


# ---- B: what a step leaves -------------------------------------------------------------------------------------------------------------------------
DT = 1e-3


def _winds(grid, hm_fields, rho):
    x = (np.arange(grid.Nx) + 0.5) * 100.0
    y = (np.arange(grid.Ny) + 0.5) * 100.0
    u = 2.0 + np.sin(2 * np.pi * x / (100.0 * grid.Nx))[None, None, :] * np.ones((grid.Nz, grid.Ny, 1))
    v = 1.0 + np.cos(2 * np.pi * y / (100.0 * grid.Ny))[None, :, None] * np.ones((grid.Nz, 1, grid.Nx))
    hm_fields["ρu"].set_interior(rho * u)
    hm_fields["ρv"].set_interior(rho * v)


def _slot(profile, name):
    return profile.get(name, (0.0, 0))[1]


def _step_anelastic(bz, shape, whole):
    hm = _anelastic(bz, shape, 1)
    case = sar.anelastic_case(shape, bulk_only=True)
    _plant_anelastic(hm, case, 1)
    _winds(hm.grid, hm.momentum, case.rho_r[:, None, None])
    hm.profile_enable(True)
    hm.profile_reset()
    bz.time_step_(hm, DT, whole_step=whole)
    hm.synchronize()
    stale, profile = bz.diagnostics_stale(hm), hm.profile()
    held = {"rtheta": hm.potential_temperature_density.interior.cpu().numpy(), "rq": hm.moisture_density.interior.cpu().numpy()}
    dev = _read_anelastic(hm, 1)     # raw reads: nothing is rebuilt
    assert not np.array_equal(held["rtheta"], case.rtheta)      # the step acted
    p_r, rho_r = _columns(hm)
    want = sar.diagnose_anelastic(held, 1, p_r, rho_r, F64)
    wide = sar.diagnose_anelastic(held, 1, p_r, rho_r, np.longdouble)
    d = sar.distances(want, wide)
    keep = ~want.knife & (want.branch == wide.branch)
    table = {"bulk": tuple(float(d[n][keep].max()) for n in ("T", "qv", "ql"))}
    assert 0.2 <= np.mean(want.branch == sar.CLOUDY) <= 0.8 and not want.nonfinite.any()
    return hm, dev, want, table, stale, profile, case


def test_anelastic_fused_step_leaves_the_restatement_of_its_fields(bz):
    """time_step! (whole step, dt = 1e-3) of the anelastic SaturationAdjustment model from the bulk sweep with small smooth winds.  The
    fused-RK tier: the T, q^v, q^l read here were written by the projection-and-diagnosis kernel of stage 3 (k_project_diagnose<1>,
    bz_fused.hip; profile slot project_and_diagnose, three launches), not by k_thermo, whose single launch is the update_state! that
    prepares the first step; the diagnostics are not stale, so the read rebuilds nothing."""
    hm, dev, want, table, stale, profile, case = _step_anelastic(bz, A_SMALL, True)
    print("SAPARCELS step anelastic fused slots:", {k: v[1] for k, v in profile.items()})
    assert not stale
    assert _slot(profile, "project_and_diagnose") == 3 and _slot(profile, "compute_auxiliary_thermodynamic_variables") == 1
    _judge64("step anelastic fused-RK", dev, want, case.tag, table)


def test_anelastic_operator_step_leaves_the_restatement_of_its_fields(bz):
    """The same step through the per-operator entry points (time_step_(whole_step = False)): every stage ends in update_state!, so the fields
    read were written by k_thermo (slot compute_auxiliary_thermodynamic_variables: the preparing launch and one per stage); no
    project_and_diagnose launch."""
    hm, dev, want, table, stale, profile, case = _step_anelastic(bz, A_SMALL, False)
    print("SAPARCELS step anelastic operators slots:", {k: v[1] for k, v in profile.items()})
    assert not stale
    assert _slot(profile, "project_and_diagnose") == 0 and _slot(profile, "compute_auxiliary_thermodynamic_variables") == 4
    _judge64("step anelastic operators", dev, want, case.tag, table)


@pytest.mark.parametrize("mp", [1, 0], ids=["SaturationAdjustment", "vapour-only"])
def test_compressible_fused_step_leaves_the_restatement_of_its_fields(bz, mp):
    """time_step! (whole step, dt = 1e-3, 6 substeps) of the compressible model from the bulk sweep, with SaturationAdjustment and without
    microphysics: the T, p (q^v, q^l) read were written by the stage-end kernel of stage 3 (k_ac_stage_end<.., MP>, bz_acoustic_kernels.h:
    bz_ds_adjust, or the Newton loop written out in its epilogue; profile slots acoustic_stage_end+update_state[+linearization], three
    launches between them); k_cmp_diagnose ran once, in the update_state! that prepares the first step."""
    shape = SMALL
    hm = _compressible(bz, shape, mp)
    case = sar.compressible_case(shape, bulk_only=True)
    _plant_compressible(hm, case, mp)
    _winds(hm.grid, hm.momentum, case.rho_d)
    hm.profile_enable(True)
    hm.profile_reset()
    hm.time_step(DT)
    hm.synchronize()
    profile = hm.profile()
    label = f"step compressible stage-end MP={mp}"
    print(f"SAPARCELS {label} slots:", {k: v[1] for k, v in profile.items()})
    held = dict(rho_d=hm.dynamics.dry_density.interior.cpu().numpy(), rtheta=hm.potential_temperature_density.interior.cpu().numpy(),
                rq=hm.moisture_density.interior.cpu().numpy())
    dev = _read_compressible(hm, mp)
    assert not np.array_equal(held["rtheta"], case.rtheta)
    fused = _slot(profile, "acoustic_stage_end+update_state") + _slot(profile, "acoustic_stage_end+update_state+linearization")
    plain = _slot(profile, "update_state") + _slot(profile, "update_state+linearization")
    assert fused == 3 and plain == 1, profile
    assert not bz.diagnostics_stale(hm)          # and the reads above are raw: nothing was rebuilt
    want = sar.diagnose_compressible(held, mp, F64)
    wide = sar.diagnose_compressible(held, mp, np.longdouble)
    d = sar.distances(want, wide)
    keep = ~want.knife & (want.branch == wide.branch)
    table = {"bulk": tuple(float(d[n][keep].max()) for n in ("T", "qv", "ql"))}
    assert not want.nonfinite.any()
    if mp == 1:
        assert 0.2 <= np.mean(want.branch == sar.CLOUDY) <= 0.8
    _judge64(label, dev, want, case.tag, table, adjusted=mp == 1)
    _compressible_extras(label, dev, want, case.tag, table, mp)
