"""CPU pins of tests/mixed_phase_density_reference.py and of the host side of SaturationAdjustment(equilibrium = MixedPhaseEquilibrium()) on
CompressibleDynamics: the warm-phase limit against oracle.thermo, the reference's own known answers, the properties of an adjusted parcel,
the conditions the sweeps and the whole-step set-up are built to meet, the oracle model against the warm one, two planted errors and the
host refusals.  No test here needs a GPU."""
import ctypes
import os

import numpy as np
import pytest

import mixed_phase_density_reference as mdr
import mixed_phase_reference as mpr
import saturation_adjustment_reference as sar
from oracle import thermo

F64, LD = np.float64, np.longdouble
SMALL, LARGE = sar.COMPRESSIBLE_GRIDS
PST = F64(sar.PST)


# ---- the restatement ----------------------------------------------------------------------------------------------------------------------------
def test_below_both_kinks_the_restatement_is_the_warm_density_adjustment_bit_for_bit():
    """T^f = 100 K, T^h = 50 K: lambda = 1 at every evaluation, q^i an exact + 0, and every ice term adds an exact zero"""
    F = mdr.typed(F64, False, 100.0, 50.0)
    theta, rho, qt, tag, _ = sar.density_parcels(600)
    tc = thermo.ThermoConstants()
    cloudy = 0
    with np.errstate(all="ignore"):
        for th, r, q, name in zip(theta, rho, qt, tag):
            th = 0.0 if name == "theta_zero" else th
            for solver in (sar.DEFAULT_SOLVER, (1e-4, 2), (0.0, 50)):
                want = thermo.adjust_warm_phase_density(float(th), float(q), float(r), sar.PST, tc, solver[0], solver[1], *sar.NEWTON)
                T, qv, ql, qi, tr = F.adjust(F64(th), F64(q), F64(r), PST, solver, sar.NEWTON)
                if not np.isfinite(want[0]):
                    continue
                assert (float(T), float(qv), float(ql)) == want and qi == 0 and not np.signbit(qi), (th, r, q, solver)
            cloudy += tr.branch == sar.CLOUDY
    assert 100 < cloudy < 500


MOISTURES = ((0.020, 0.0, 0.0), (0.018, 0.005, 0.0), (0.015, 0.003, 0.002))


@pytest.mark.parametrize("q", MOISTURES, ids=("vapour", "liquid", "mixed"))
def test_the_references_known_answers_of_the_density_state(q):
    """test/compressible_saturation_adjustment.jl:33-51 of the reference: at theta = 300 K, rho = 1 kg/m^3 the inverted temperature is the
    fixed point T = (rho R_m T / p_st)^kappa theta + L to 1e-9, and theta round-trips"""
    F = mdr.typed(F64)
    th, rho = F64(300.0), F64(1.0)
    qv, ql, qi = (F64(v) for v in q)
    T = F.temperature_mixed(th, qv, ql, qi, rho, PST, F64(sar.NEWTON[0]), sar.NEWTON[1])
    Rm, cpm = F._mix3(qv, ql, qi)
    L = (F.Ll * ql + F.Li * qi) / cpm
    assert abs(T - ((rho * Rm * T / PST) ** (Rm / cpm) * th + L)) <= 1e-9 * T
    assert abs(F.theta_of_density(T, qv, ql, qi, rho, PST) - th) <= 1e-9 * th
    if qi > 0:          # the ice terms are in: without them the fixed point is kelvins away
        assert abs(T - F.temperature_mixed(th, qv, ql + qi, F64(0), rho, PST, F64(1e-4), 8)) > 0.1


@pytest.mark.parametrize("polynomial", (False, True), ids=("clausius-clapeyron", "polynomial"))
def test_an_adjusted_cloudy_parcel_sits_on_the_surface_at_its_own_density(polynomial):
    """q^v = q^v+(T*, rho) over the mixed surface at the final iterate, q^l / q^c = lambda(T*) exactly, theta conserved to the solver's
    tolerance; under abstol = 0 the final iterate and the returned temperature agree to rounding"""
    F = mdr.typed(F64, polynomial)
    case = mdr.mixed_density_case(SMALL, 0, polynomial)
    want = mdr.restated(SMALL, F64, (0.0, 50), polynomial=polynomial)
    seen = 0
    for idx in np.ndindex(case.tag.shape):
        if want.branch[idx] != sar.CLOUDY or want.nonfinite[idx] or case.tag[idx] == "marginal_edge":
            continue
        T, qv, ql, qi, rho, th, q = (F64(want[n][idx]) for n in ("T", "qv", "ql", "qi", "rho", "theta", "q"))
        qc = ql + qi
        if not qc > 1e-9:
            continue
        seen += 1
        assert abs(qv - F.saturated_vapor_density(T, rho)) <= 1e-10, idx
        lam = F.lam(T)
        assert abs(ql - lam * qc) <= 1e-9 * qc + 1e-18 and abs(qv + ql + qi - q) <= 4e-16, idx
        assert abs(F.theta_of_density(T, qv, ql, qi, rho, PST) - th) <= 1e-9 * th, idx
        # and the partition itself is exact at the iterate it was split at
        r, v, l, i = F.residual_mixed(T, th, rho, q, PST)
        assert l == F.lam(T) * max(F64(0), q - F.saturated_vapor_density(T, rho))
    assert seen > 300


# ---- the sweeps -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("polynomial", (False, True), ids=("clausius-clapeyron", "polynomial"))
def test_the_sweep_holds_what_it_is_built_to_hold(polynomial):
    """every population present; both placements hold the same parcels; warm cloudy parcels end at least 5 K above T^f and all-ice ones 5 K
    below T^h under the default solver (so the exact-zero rule applies to each of them); the mixed range and both sides of both kinks are
    reached; wavefronts mix branches and iteration counts; few knife-edge parcels; no non-finite intermediate; the hosting rule holds"""
    case = mdr.mixed_density_case(SMALL, 0, polynomial)
    other = mdr.mixed_density_case(SMALL, 1, polynomial)
    assert set(mpr.POPULATIONS) == set(np.unique(case.tag))
    for n in ("rho_d", "rtheta", "rq", "tag"):
        assert np.array_equal(mpr.by_parcel(case, case[n]), mpr.by_parcel(other, other[n])) and not np.array_equal(case[n], other[n]), n
    want, wide = mdr.restated(SMALL, F64, polynomial=polynomial), mdr.restated(SMALL, LD, polynomial=polynomial)
    assert not want.nonfinite.any() and np.isfinite(want["T"]).all()
    cloudy = want.branch == sar.CLOUDY
    assert 0.2 <= cloudy.mean() <= 0.8
    warm, ice = mpr.exact_partition_masks(want, case.tag)
    assert np.array_equal(warm, (case.tag == "warm_cloudy") & cloudy) and warm.sum() > 20 and (want["qi"][warm] == 0).all()
    assert np.array_equal(ice, (case.tag == "all_ice") & cloudy) and ice.sum() > 20 and (want["ql"][ice] == 0).all()
    both = cloudy & (want["ql"] > 0) & (want["qi"] > 0)
    assert both.sum() > 100 and set(np.unique(case.tag[both])) >= {"mixed_range", "kink_Th", "kink_Tf"}
    for name, kink in (("kink_Th", mdr.TH), ("kink_Tf", mdr.TF)):
        T = want["T"][(case.tag == name) & cloudy].astype(F64)
        assert (T > kink).any() and (T < kink).any() and np.abs(T - kink).max() < 2 * mpr.KINK
    assert sar.wavefront_mixing(want) >= (2, 2)
    knife = mdr.knife_edge(want, wide, case.tag)
    assert knife.sum() <= 0.005 * cloudy.sum() + 2, int(knife.sum())
    F = mdr.typed(F64, polynomial)
    hosted = np.isin(case.tag, ("warm_cloudy", "all_ice", "mixed_range", "kink_Th", "kink_Tf"))
    qs = np.array([float(F.saturated_vapor_density(F64(T), F64(r))) for T, r in zip(case.target[hosted], want["rho"][hosted].astype(F64))])
    assert qs.max() <= mpr.Q_HOST * 1.0001 and np.abs(want["q"]).max() <= sar.Q_CAP * 1.0001
    # the mixed diagnosis is not the warm one
    held = {n: case[n] for n in ("rho_d", "rtheta", "rq")}
    assert np.nanmax(np.abs(want["T"].astype(F64) - sar.diagnose_compressible(held, 1, F64)["T"])) > 1e-6


def test_the_restatements_own_sensitivity_is_small():
    for polynomial in (False, True):
        table = mdr.d80(SMALL, polynomial=polynomial)
        assert set(table) == set(mpr.POPULATIONS) - {"theta_zero"} | ({"theta_zero"} & set(table))
        for name, row in table.items():
            assert row[0] <= 1e-12 and max(row[1:]) <= 1e-14, (polynomial, name, row)


def test_a_planted_error_in_the_inversion_fails_the_sweep():
    """c_i q^i left out of c_pm in the closing temperature inversion: the judging rules of tests/test_compressible_mixed_phase.py reject it"""
    case = mdr.mixed_density_case(SMALL)
    held = {n: case[n] for n in ("rho_d", "rtheta", "rq")}
    wrong = mdr.diagnose_mixed_density(held, F64, leave_out_ci=True)
    want = mdr.restated(SMALL, F64)
    fails, _, _ = mpr.judge64(wrong, want, case.tag, mdr.d80(SMALL), mdr.restated(SMALL, F64, force_branch="clear"),
                              mdr.restated(SMALL, F64, force_branch="cloudy"))
    assert any("ordinary parcels" in k for k in fails), fails
    right, _, _ = mpr.judge64(want, want, case.tag, mdr.d80(SMALL), mdr.restated(SMALL, F64, force_branch="clear"),
                              mdr.restated(SMALL, F64, force_branch="cloudy"))
    assert not right, right


# ---- the oracle model ---------------------------------------------------------------------------------------------------------------------------
def _small_pair(oracle, oc, **kw):
    size, ext = (8, 6, 6), dict(x=(0.0, 2e3), y=(0.0, 1.5e3), z=(0.0, 3e3))
    thref = lambda z: 300.0 * np.exp(9.80616 * z / (1005 * 300.0))
    args = dict(time_discretization=oc.SplitExplicit(substeps=6), surface_pressure=1e5, reference_potential_temperature=thref,
                microphysics="SaturationAdjustment")
    warm = oc.CompressibleOracleModel(oracle.Grid(size, **ext), **args)
    mixed = mdr.MixedCompressibleOracle(oracle.Grid(size, **ext), **args, **kw)
    bub = lambda x, y, z: np.maximum(0.0, 1.0 - np.sqrt(((x - 1e3) / 500.0) ** 2 + ((y - 750.0) / 750.0) ** 2 + ((z - 1200.0) / 900.0) ** 2))
    th = lambda x, y, z: 300.0 + 0.5 * bub(x, y, z) + 0 * z
    qt = lambda x, y, z: 0.012 + 0.014 * bub(x, y, z) + 0.004 * (z / 3e3)
    for om in (warm, mixed):
        om.set(rho=om.ref.density[om.grid.Hz:om.grid.Hz + om.grid.Nz][:, None, None], theta=th, u=2.0, v=0.0, w=0.0, qv=qt)
    return warm, mixed


def test_without_ice_the_oracle_model_steps_like_the_warm_one_bit_for_bit(oracle, oc):
    """T^f and T^h far below the column: q^i stays an exact zero and two steps leave the bits of CompressibleOracleModel(microphysics =
    "SaturationAdjustment")"""
    warm, mixed = _small_pair(oracle, oc, freezing_temperature=100.0, homogeneous_ice_nucleation_temperature=50.0)
    for _ in range(2):
        warm.time_step(1.0)
        mixed.time_step(1.0)
    assert (warm.grid.interior(warm.ql) > 0).any()
    for n in ("rho_d", "rho", "rtheta", "rq", "ru", "rv", "rw", "T", "p", "qv", "ql", "Pi", "thL", "gR"):
        assert np.array_equal(getattr(warm, n), getattr(mixed, n)), n
    assert not mixed.qi.any()


def test_with_ice_the_oracle_model_differs_from_the_warm_one(oracle, oc):
    """the same column with the kinks at 295 K and 285 K, so that its clouds are mixed and ice: T and gamma R_m move"""
    warm, mixed = _small_pair(oracle, oc, freezing_temperature=295.0, homogeneous_ice_nucleation_temperature=285.0)
    g = mixed.grid
    assert (g.interior(mixed.qi) > 0).any() and np.abs(g.interior(mixed.T) - g.interior(warm.T)).max() > 1e-3
    warm.refresh_linearization()
    mixed.refresh_linearization()
    assert np.abs(g.interior(mixed.gR) - g.interior(warm.gR)).max() > 1e-6


@pytest.mark.parametrize("size", mdr.STEP_SHAPES, ids=str)
def test_the_whole_step_set_up_holds_every_regime(oracle, oc, size):
    """the condition tests/test_compressible_mixed_phase.py asserts again on the GPU machine, decided here: at the start and after the three
    steps each of clear, liquid only, liquid + ice and ice only holds at least 5 % of the cells of the oracle's fields"""
    start, end = mdr.oracle_steps(oracle, oc, size)
    for label, f in (("start", start), ("end", end)):
        shares = mdr.regime_shares(f["ql"], f["qi"])
        print(f"MIXEDDENSITY regimes {size} {label}:", dict(zip(mdr.REGIMES, (round(s, 3) for s in shares))))
        assert min(shares) >= mdr.MIN_REGIME_SHARE, (label, shares)
        assert all(np.isfinite(v).all() for v in f.values())
    assert not np.array_equal(start["rw"], end["rw"]) and np.abs(end["T"] - start["T"]).max() > 1e-3


def test_a_planted_error_in_the_linearisation_fails_the_step_bounds(oracle, oc):
    """c_i q^i left out of c_pm in refresh_linearization: three steps leave the 1e-8 bound of the whole-step test"""
    size = mdr.STEP_SHAPES[0]
    _, want = mdr.oracle_steps(oracle, oc, size)
    _, wrong = mdr.oracle_steps(oracle, oc, size, leave_out_ci="linearization")
    errs = mdr.scaled_errors(wrong, want, ("rho_d", "rtheta", "rq", "ru", "rw", "T", "p"))
    print("MIXEDDENSITY planted linearisation error:", {k: f"{v:.1e}" for k, v in errs.items()})
    assert max(errs.values()) > 1e-8, errs


# ---- the host side --------------------------------------------------------------------------------------------------------------------------------
def _grid(bz, **kw):
    return bz.RectilinearGrid((16, 8, 8), x=(0, 1600.0), y=(0, 800.0), z=(0, 8e3), **kw)


def _stand_in(bz, **kw):
    """a CompressibleAtmosphereModel that has no device and no context: what the host checks read, nothing else"""
    m = object.__new__(kw.pop("cls", bz.CompressibleAtmosphereModel))
    m.microphysics = bz.SaturationAdjustment(equilibrium=bz.WarmPhaseEquilibrium())
    m.lateral_walls, m.grid, m.dynamics, m._sa, m._surface_fluxes, m.thermodynamic_constants = False, _grid(bz), None, True, {}, bz.ThermodynamicConstants()
    for k, v in kw.items():
        setattr(m, k, v)
    return m


def test_every_host_refusal_names_the_equilibrium_before_asking_for_a_gpu(bz):
    """the constructor keeps attaching the warm-phase adjustment and says where the mixed-phase form is attached; that function,
    compressible.set_mixed_phase_equilibrium_, refuses by name and with a reason before it touches the context (the stand-ins have none)"""
    attach = bz.compressible.set_mixed_phase_equilibrium_
    dyn = bz.CompressibleDynamics(bz.SplitExplicitTimeDiscretization(substeps=6))
    with pytest.raises(NotImplementedError, match="set_mixed_phase_equilibrium_") as e:
        bz.CompressibleAtmosphereModel(_grid(bz), dyn, advection=bz.WENO(order=5), microphysics=bz.SaturationAdjustment())
    assert "MixedPhaseEquilibrium" in str(e.value)
    eq = bz.MixedPhaseEquilibrium()
    cases = {
        "slab": _stand_in(bz, cls=bz.compressible.SlabCompressibleModel),
        "walls": _stand_in(bz, lateral_walls=True),
        "bulk surface fluxes": _stand_in(bz, _surface_fluxes={"heat": object()}),
        "tetens": _stand_in(bz, thermodynamic_constants=bz.ThermodynamicConstants(saturation_vapor_pressure=bz.TetensFormula())),
        "kessler": _stand_in(bz, _sa=False, microphysics=bz.DCMIP2016KesslerMicrophysics()),
        "instantaneous precipitation": _stand_in(bz, _sa=False, microphysics=bz.InstantaneousPrecipitation()),
        "no microphysics": _stand_in(bz, _sa=False, microphysics=None),
    }
    for name, m in cases.items():
        with pytest.raises(NotImplementedError, match="MixedPhaseEquilibrium") as e:
            attach(m, eq)
        assert len(str(e.value)) > 60, (name, str(e.value))          # ... and a reason
    with pytest.raises(TypeError):
        attach(_stand_in(bz), object())
    with pytest.raises(TypeError):
        attach(object(), eq)
    for build in (lambda: bz.InstantaneousPrecipitation(equilibrium=eq),):
        with pytest.raises(NotImplementedError, match="MixedPhaseEquilibrium"):
            build()


def test_operations_on_a_mixed_phase_compressible_model_refuse_by_name(bz):
    """set!(T | H), the diagnostics, the hydrostatic balances and the moisture-carrying adiabatic balance check the model's microphysics
    before they touch its context: a stand-in that has no context shows it"""
    from breeze_jl_amd import balance, compressible, diagnostics as D

    m = _stand_in(bz, microphysics=bz.SaturationAdjustment())          # what set_mixed_phase_equilibrium_ leaves in `microphysics`
    calls = {
        "set!(T)": lambda: compressible.set_(m, T=280.0),
        "set!(H)": lambda: compressible.set_(m, relative_humidity=0.5),
        "HydrostaticallyBalancedDensity": lambda: compressible.set_(m, ρ=bz.compressible.HydrostaticallyBalancedDensity()),
        "compute_reference_state": lambda: compressible.set_(m, compute_reference_state=True, θ=300.0),
        "diagnostics": lambda: D.RelativeHumidity(m),
        "balance": lambda: balance.balance_adiabatically_(m, balance.AdiabaticBalancer(Δt=1.0, time_stepping=None)),
    }
    for name, call in calls.items():
        with pytest.raises(NotImplementedError, match="MixedPhaseEquilibrium"):
            call()
    m.microphysics = bz.SaturationAdjustment(equilibrium=bz.WarmPhaseEquilibrium())
    with pytest.raises(ValueError, match="Cannot set! T"):          # a warm model keeps the message of an unknown keyword
        compressible.set_(m, T=280.0)


def test_symbol_and_headers(bz):
    from breeze_jl_amd import _lib
    res, args = bz.SYMBOLS["bz_set_compressible_mixed_phase_equilibrium"]
    assert res is ctypes.c_int and len(args) == 3 and args[1]._type_ is _lib.bz_mixed_phase_equilibrium
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for header, real in (("breeze_hip.h", "double"), ("breeze_hip_f32.h", "float")):
        text = open(os.path.join(root, "include", header), encoding="utf-8").read()
        assert f"int bz_set_compressible_mixed_phase_equilibrium(bz_ctx *ctx, const bz_mixed_phase_equilibrium *params, {real} *q_ice);" in text, header
