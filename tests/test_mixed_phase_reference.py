"""CPU pins of tests/mixed_phase_reference.py and of the host side of SaturationAdjustment(equilibrium = MixedPhaseEquilibrium()):
the restatement meets the reference's three known answers (test/saturation_adjustment.jl:150-239, restated for theta), conserves the total
moisture, returns the bits of oracle.thermo.adjust_warm_phase once T^f and T^h lie below every parcel, the sweep meets the conditions the
device tests rely on (among them the knife-edge cap), the vectorised transcription the oracle model uses agrees with the typed one, and
the host classes construct, refuse and bind as the model documentation says.  Nothing here needs a GPU."""
import numpy as np
import pytest

import mixed_phase_reference as mpr
import saturation_adjustment_reference as sar
from oracle import thermo

F64, LD, F32 = np.float64, np.longdouble, np.float32
EPS = float(np.finfo(F64).eps)


def lowest_level_pressure():
    """p_r of the single level of the reference's (1, 1, 1) grid over z = (0, 1) under ReferenceState(p0 = 101325, theta0 = 288)"""
    return float(sar.reference_column(1, 1.0, p0=mpr.KNOWN_P0, theta0=mpr.KNOWN_THETA0)[0][0])


@pytest.mark.parametrize("T,qt", mpr.KNOWN, ids=mpr.KNOWN_IDS)
def test_reference_known_answers(T, qt):
    """theta^li built from the known (T, q); the adjustment returns T, q^v, q^l, q^i within the reference's atol under its solver.  220 K and
    253.15 K are saturated (all ice; half liquid, half ice).  300 K / 0.02 is NOT saturated at 1013 hPa (q^v+ = 0.0220): the reference's own
    guard skips its assertions there; here the unsaturated state is the known answer, and q^l = q^i = 0 exactly."""
    F, pr, pst = mpr.typed(F64), F64(lowest_level_pressure()), F64(sar.PST)
    theta, qv, ql, qi = F.known_answer(F64(T), F64(qt), pr, pst)
    got = F.adjust_mixed(theta, F64(qt), pr, pst, F64(mpr.SOLVER_TOL), 20)
    for name, g, w in zip(mpr.NAMES, got[:4], (T, qv, ql, qi)):
        assert abs(float(g) - float(w)) <= mpr.TEST_TOL, (name, g, w)
    if T == 300.0:
        assert got[4].branch == mpr.CLEAR and got[1] == qt and got[2] == 0 and got[3] == 0
    if T == 220.0:
        assert got[4].branch == mpr.CLOUDY and got[2] == 0 and got[3] > 0.009
    if T == 253.15:
        assert got[4].branch == mpr.CLOUDY and got[2] > 0.006 and abs(float(got[2]) - float(got[3])) <= mpr.TEST_TOL


def test_liquid_fraction_at_the_reference_temperatures():
    F = mpr.typed(F64)
    assert F.lam(F64(300.0)) == 1 and F.lam(F64(200.0)) == 0
    assert abs(float(F.lam(F64(253.15))) - 0.5) <= 2 * EPS
    assert F.lam(F64(mpr.TF)) == 1 and F.lam(F64(mpr.TH)) == 0


def test_mixed_surface_is_the_oracles():
    """one Clausius-Clapeyron expression with blended constants: oracle/thermo.py's ('mixed', lambda) surface, bit for bit"""
    F, c = mpr.typed(F64), thermo.ThermoConstants()
    for T in (215.0, 233.15, 240.0, 253.15, 268.3, 273.15, 290.0):
        lam = F.lam(F64(T))
        assert float(F.psat_mixed(F64(T), lam)) == thermo.saturation_vapor_pressure(T, c, ("mixed", float(lam)))


@pytest.mark.parametrize("shape", sar.ANELASTIC_GRIDS, ids=str)
def test_total_moisture_is_conserved(shape):
    r = mpr.restated(shape, F64)
    total = (r.qv + r.ql) + r.qi
    assert np.all(np.abs(total - r.q) <= 2 * EPS * np.maximum(np.abs(r.q), 1.0))
    assert np.all(np.abs(total - r.q) <= 2 * EPS)


@pytest.mark.parametrize("shape", sar.ANELASTIC_GRIDS, ids=str)
def test_below_both_temperatures_it_is_the_warm_phase_bit_for_bit(shape):
    """T^f and T^h moved below every parcel of the warm sweep (sar.anelastic_case, T >= ~200 K): lambda = 1 at every evaluation, and the
    float64 restatement returns the bits of oracle.thermo.adjust_warm_phase under every solver of the sweep"""
    c, case = thermo.ThermoConstants(), sar.anelastic_case(shape)
    solvers = sar.SOLVERS if shape == sar.ANELASTIC_GRIDS[0] else (sar.DEFAULT_SOLVER,)
    for solver in solvers:
        r = mpr.diagnose_mixed(case, case.p_r, case.rho_r, F64, solver, Tf=60.0, Th=50.0)
        assert (r.branch == mpr.CLOUDY).mean() > 0.2
        for idx in np.ndindex(r.T.shape):
            want = thermo.adjust_warm_phase(float(r.theta[idx]), float(r.q[idx]), float(case.p_r[idx[0]]), sar.PST, c, solver[0], solver[1])
            got = (float(r.T[idx]), float(r.qv[idx]), float(r.ql[idx]))
            assert got == tuple(float(w) for w in want) and r.qi[idx] == 0, (solver, idx, got, want)


def solvers_of(shape):
    return sar.SOLVERS if shape == sar.ANELASTIC_GRIDS[0] else (sar.DEFAULT_SOLVER,)


@pytest.mark.parametrize("shape", sar.ANELASTIC_GRIDS, ids=str)
def test_sweep_conditions_and_the_knife_edge_cap(shape):
    """The cap: knife-edge parcels — those where the float64 and the longdouble restatement take different branches or different iteration
    counts (or whose |r2| comes within 1e-9 K of abstol, the flag the judging skips by) — are at most 0.5 % of the cloudy parcels, threshold
    parcels aside (they are judged on either branch).  It is asserted for every solver whose abstol is not zero: there one iteration more or
    less moves the answer by up to abstol.  Under SecantSolver(abstol = 0) the iteration runs until the secant stagnates (the `valid` guard);
    how many steps that takes depends on the last bits, the answer does not: there the branches must agree, no parcel is flagged or skipped
    (every one is judged on the device), and the float64-to-longdouble distance must stay a rounding figure."""
    case = mpr.mixed_case(shape)
    tag = case.tag
    for name in mpr.POPULATIONS:
        assert (tag == name).any(), name
    assert case.p_r[-1] < 2e3                    # the column's top is far colder than T^h
    for solver in solvers_of(shape):
        r, wide = mpr.restated(shape, F64, solver), mpr.restated(shape, LD, solver)
        assert not r.nonfinite.any(), (solver, int(r.nonfinite.sum()))
        cloudy = r.branch == mpr.CLOUDY
        free = tag == "marginal_edge"            # threshold parcels are judged on either branch, never as knife-edge ones
        knife = (r.knife | (r.branch != wide.branch) | (r.iterations != wide.iterations)) & ~free
        print(f"MIXEDSWEEP {shape} solver={solver}: clear={np.mean(r.branch == mpr.CLEAR):.2f} cloudy={cloudy.mean():.2f} "
              f"iterations={sorted(set(int(i) for i in r.iterations[cloudy]))} knife-edge={int(knife.sum())}/{int(cloudy.sum())}")
        if solver[0] > 0:
            assert int(knife.sum()) <= 0.005 * cloudy.sum()      # the cap the device tests rely on
        else:
            assert not r.knife.any() and np.array_equal(r.branch[~free], wide.branch[~free])
            for name, row in mpr.own_distance(r, wide, tag).items():
                assert row[0] <= 1e-13 and max(row[1:]) <= 1e-14, (name, row)
        assert np.mean(r.branch == mpr.CLEAR) >= 0.2 and cloudy.mean() >= 0.2
        live = r.branch != mpr.THETA_ZERO
        assert r.q[live].max() <= sar.Q_CAP * (1 + 1e-12) and r.q[live].min() >= -1e-5 * (1 + 1e-12)
        for name, row in mpr.own_distance(r, wide, tag).items():
            print(f"MIXEDD80 {shape} solver={solver} {name}: T={row[0]:.1e} qv={row[1]:.1e} ql={row[2]:.1e} qi={row[3]:.1e}")
    r = mpr.restated(shape, F64)
    sel = lambda name: (tag == name) & (r.branch == mpr.CLOUDY)
    warm, ice = mpr.exact_partition_masks(r, tag)          # under the converged solver the exact rules cover both populations entirely
    assert np.array_equal(warm, tag == "warm_cloudy") and np.array_equal(ice, tag == "all_ice")
    for solver in solvers_of(shape):
        rs = mpr.restated(shape, F64, solver)
        w, i = mpr.exact_partition_masks(rs, tag)
        assert w.any() and i.any() and np.all(rs.qi[w] == 0) and np.all(rs.ql[i] == 0), solver
    # the populations are what their names say, on the adjusted state
    assert sel("warm_cloudy").sum() == (tag == "warm_cloudy").sum() and np.all(r.T[sel("warm_cloudy")] >= mpr.TF + 5.0)
    assert np.all(r.qi[sel("warm_cloudy")] == 0) and np.all(r.ql[sel("warm_cloudy")] > 0)
    assert sel("all_ice").sum() == (tag == "all_ice").sum() and np.all(r.T[sel("all_ice")] <= mpr.TH - 5.0)
    assert np.all(r.ql[sel("all_ice")] == 0) and np.all(r.qi[sel("all_ice")] > 0)
    m = sel("mixed_range")
    assert m.sum() == (tag == "mixed_range").sum() and np.all((r.ql[m] > 0) & (r.qi[m] > 0))
    for name, kink in (("kink_Th", mpr.TH), ("kink_Tf", mpr.TF)):
        d = r.T[sel(name)] - kink
        assert np.all(np.abs(d) <= mpr.KINK) and (d > 0).any() and (d < 0).any(), name
    assert set(case.sub[tag == "marginal_edge"]) == set(mpr.EDGE_DELTAS)
    edge = r.branch[tag == "marginal_edge"]
    assert (edge == mpr.CLEAR).any() and (edge == mpr.CLOUDY).any()
    assert set(case.sub[tag == "negative_or_zero_q"]) == set(sar.NEGATIVE_Q) and np.all(r.branch[tag == "negative_or_zero_q"] == mpr.CLEAR)
    assert np.all(r.branch[tag == "theta_zero"] == mpr.THETA_ZERO) and (tag == "theta_zero").sum() == 4


@pytest.mark.parametrize("shape", sar.ANELASTIC_GRIDS, ids=str)
def test_two_placements_mix_the_branches_in_a_wavefront(shape):
    a, b = mpr.mixed_case(shape, 0), mpr.mixed_case(shape, 1)
    assert not np.array_equal(a.parcel, b.parcel)
    for n in ("rtheta", "rq", "tag"):            # the same parcels, level by level
        assert np.array_equal(mpr.by_parcel(a, a[n]), mpr.by_parcel(b, b[n])), n
    for which in (0, 1):
        branches, counts = sar.wavefront_mixing(mpr.restated(shape, F64, which=which))
        assert branches >= 2 and counts >= 3, (which, branches, counts)


def test_float32_restatement_stays_a_rounding_distance_away():
    shape = sar.ANELASTIC_GRIDS[0]
    case = mpr.mixed_case(shape)
    arrays = {n: case[n].astype(F32) for n in ("rtheta", "rq")}
    r32 = mpr.diagnose_mixed(arrays, case.p_r.astype(F32), case.rho_r.astype(F32), F32)
    r64 = mpr.diagnose_mixed({n: a.astype(F64) for n, a in arrays.items()}, case.p_r.astype(F32).astype(F64), case.rho_r.astype(F32).astype(F64), F64)
    same = (r32.branch == r64.branch) & (r64.branch == mpr.CLOUDY) & ~np.isin(case.tag, ("kink_Th", "kink_Tf", "marginal_edge"))
    d = mpr.distances(r32, r64)
    print("MIXEDD32", {n: float(d[n][same].max()) for n in mpr.NAMES})
    assert d["T"][same].max() <= 1e-4 and max(d[n][same].max() for n in ("qv", "ql", "qi")) <= 1e-4


def test_vectorised_transcription_agrees_with_the_typed_restatement():
    """adjust_mixed_array (what MixedPhaseOracleModel runs) against TypedMixed(float64) over the sweep: the same branch for every parcel
    off the threshold, T within 1e-13 relative and the fractions within 1e-15 (numpy's pow / exp against libm's)"""
    shape = sar.ANELASTIC_GRIDS[0]
    case, r = mpr.mixed_case(shape), mpr.restated(shape, F64)
    T, qv, ql, qi = mpr.adjust_mixed_array(r.theta, r.q, case.p_r[:, None, None])
    keep = (case.tag != "marginal_edge") & ~r.knife
    assert np.array_equal((ql + qi > 0)[keep], (r.ql + r.qi > 0)[keep])
    assert np.all(np.abs(T - r.T)[keep] <= 1e-13 * np.maximum(np.abs(r.T[keep]), 1.0))
    for got, name in ((qv, "qv"), (ql, "ql"), (qi, "qi")):
        assert np.abs(got - r[name])[keep].max() <= 1e-15, name
    zero = r.branch == mpr.THETA_ZERO
    assert np.all(T[zero] == 0) and np.all(ql[zero] == 0) and np.all(qi[zero] == 0)


def test_oracle_model_carries_the_mixed_diagnosis(oracle):
    """MixedPhaseOracleModel: T, q^v, q^l, q^i of the interior are the restatement's, self.ql is q^l + q^i (what the moist w tendency
    reads), halos are refilled, and the ice loading reaches G_rho_w"""
    g = oracle.Grid((8, 4, 12), x=(0, 8e3), y=(0, 4e3), z=(0, 12e3))
    om = mpr.MixedPhaseOracleModel(g, potential_temperature=300.0)
    qt = lambda x, y, z: 0.02 * np.exp(-z / 2500.0) * (1 + 0.1 * np.sin(2 * np.pi * x / 8e3)) + 0 * y
    om.set(qt=qt, theta=lambda x, y, z: 300.0 + 0.0 * x)
    om.compute_tendencies()
    I = g.interior
    pr = om.ref.pressure[g.Hz:g.Hz + g.Nz][:, None, None]
    T, qv, ql, qi = mpr.adjust_mixed_array(I(om.theta), I(om.q), pr, om.ref.pst)
    assert np.array_equal(I(om.T), T) and np.array_equal(I(om.qv), qv) and np.array_equal(I(om.ql_liquid), ql) and np.array_equal(I(om.qi), qi)
    assert np.array_equal(I(om.ql), ql + qi)
    assert ((ql > 0) & (qi == 0)).any() and ((qi > 0) & (ql == 0)).any() and ((ql > 0) & (qi > 0)).any()
    for f in (om.qi, om.ql_liquid, om.ql, om.T):
        assert np.array_equal(f[g.Hz:g.Hz + g.Nz, g.Hy:g.Hy + g.Ny, 0], f[g.Hz:g.Hz + g.Nz, g.Hy:g.Hy + g.Ny, g.Nx])      # periodic image in x
    warm = oracle.OracleModel(g, potential_temperature=300.0, microphysics="SaturationAdjustment")
    warm.set(qt=qt, theta=lambda x, y, z: 300.0 + 0.0 * x)
    warm.compute_tendencies()
    assert not np.array_equal(om.G["rw"], warm.G["rw"])          # the freezing warms the upper cells and loads them with ice
    assert np.array_equal(om.G["rq"], warm.G["rq"])


# ---- the host side ---------------------------------------------------------------------------------------------------------------------------
def _grid(bz, **kw):
    return bz.RectilinearGrid((16, 8, 8), x=(0, 1600.0), y=(0, 800.0), z=(0, 8e3), **kw)


def test_constructor_defaults_and_errors(bz):
    from breeze_jl_amd.microphysics import MixedPhaseEquilibrium
    assert bz.MixedPhaseEquilibrium is MixedPhaseEquilibrium
    eq = bz.MixedPhaseEquilibrium()
    assert (eq.freezing_temperature, eq.homogeneous_ice_nucleation_temperature) == (273.15, 233.15)
    eq = bz.MixedPhaseEquilibrium(freezing_temperature=270.0, homogeneous_ice_nucleation_temperature=240.0)
    assert (eq.freezing_temperature, eq.homogeneous_ice_nucleation_temperature) == (270.0, 240.0)
    with pytest.raises(ValueError) as e:
        bz.MixedPhaseEquilibrium(freezing_temperature=230.0)
    assert str(e.value) == "`freezing_temperature` must be greater than `homogeneous_ice_nucleation_temperature`"
    with pytest.raises(ValueError, match="0 / 0"):
        bz.MixedPhaseEquilibrium(freezing_temperature=250.0, homogeneous_ice_nucleation_temperature=250.0)
    sa = bz.SaturationAdjustment()               # the reference's default equilibrium
    assert isinstance(sa.equilibrium, bz.MixedPhaseEquilibrium) and (sa.solver.abstol, sa.solver.maxiter) == (1e-4, 20)
    assert isinstance(bz.SaturationAdjustment(equilibrium=bz.WarmPhaseEquilibrium()).equilibrium, bz.WarmPhaseEquilibrium)
    with pytest.raises(NotImplementedError):
        bz.SaturationAdjustment(equilibrium=object())


def test_instantaneous_precipitation_still_refuses_the_mixed_phase(bz):
    with pytest.raises(NotImplementedError, match="MixedPhaseEquilibrium"):
        bz.InstantaneousPrecipitation(equilibrium=bz.MixedPhaseEquilibrium())
    assert isinstance(bz.InstantaneousPrecipitation().saturation_adjustment.equilibrium, bz.WarmPhaseEquilibrium)


def test_every_refusal_names_the_equilibrium_before_asking_for_a_gpu(bz):
    """each model or attachment the mixed-phase adjustment does not run on raises NotImplementedError naming MixedPhaseEquilibrium where the
    microphysics type is checked: on a machine without a GPU none of these reaches the RuntimeError of the device check"""
    from breeze_jl_amd import distributed
    grid = _grid(bz)
    ref = bz.ReferenceState(grid, potential_temperature=300.0)
    mixed = bz.SaturationAdjustment()
    dyn = lambda: bz.CompressibleDynamics(bz.SplitExplicitTimeDiscretization(substeps=6))
    anelastic = dict(dynamics=bz.AnelasticDynamics(ref), advection=bz.WENO(order=5), microphysics=mixed)
    heat = bz.BulkSensibleHeatFlux(coefficient=1e-3, surface_temperature=300.0)
    cases = {
        "compressible": lambda: bz.CompressibleAtmosphereModel(grid, dyn(), advection=bz.WENO(order=5), microphysics=mixed),
        "compressible slab": lambda: bz.compressible.SlabCompressibleModel(grid, 0, 1, dyn(), advection=bz.WENO(order=5), microphysics=mixed,
                                                                           device="cuda:0"),      # (the device is named: nothing asks torch for one)
        "kinematic": lambda: bz.AtmosphereModel(grid, dynamics=bz.PrescribedDynamics(ref), advection=bz.WENO(order=5), microphysics=mixed),
        "library slab": lambda: distributed.LibrarySlabAtmosphereModel(grid, 0, 1, advection=bz.WENO(order=5), microphysics=mixed, device="cuda:0"),
        "tetens": lambda: bz.AtmosphereModel(grid, thermodynamic_constants=bz.ThermodynamicConstants(saturation_vapor_pressure=bz.TetensFormula()),
                                             **anelastic),
        "energy forcing": lambda: bz.AtmosphereModel(grid, forcing={"e": bz.Forcing(lambda z: 0.0 * z)}, **anelastic),
        "bottom energy flux": lambda: bz.AtmosphereModel(grid, boundary_conditions={"ρe": bz.FieldBoundaryConditions(bottom=bz.FluxBoundaryCondition(10.0))},
                                                         **anelastic),
        "bulk flux": lambda: bz.AtmosphereModel(grid, boundary_conditions={"ρθ": bz.FieldBoundaryConditions(bottom=heat)}, **anelastic),
    }
    for name, make in cases.items():
        with pytest.raises(NotImplementedError, match="MixedPhaseEquilibrium"):
            make()
    # the StaticEnergy formulation keeps its pinned message
    with pytest.raises(NotImplementedError) as e:
        bz.AtmosphereModel(grid, formulation="StaticEnergy", **anelastic)
    assert str(e.value) == "microphysics is implemented for the potential-temperature formulation"


def test_diagnostics_refuse_a_mixed_phase_model(bz):
    """the operations of diagnostics.py check the model's microphysics when they are built: no device is touched"""
    class Model:
        microphysics = bz.SaturationAdjustment()
    from breeze_jl_amd import diagnostics as D
    for op in (D.PotentialTemperature, D.VirtualPotentialTemperature, D.LiquidIcePotentialTemperature, D.EquivalentPotentialTemperature,
               D.StabilityEquivalentPotentialTemperature, D.RelativeHumidity, D.DewpointTemperature, D.StaticEnergy, D.SaturationSpecificHumidity):
        with pytest.raises(NotImplementedError, match="MixedPhaseEquilibrium"):
            op(Model())
    with pytest.raises(NotImplementedError, match="MixedPhaseEquilibrium"):
        D.Average(D.RelativeHumidity(Model()), dims=(1, 2))

    class Warm:
        microphysics = bz.SaturationAdjustment(equilibrium=bz.WarmPhaseEquilibrium())
    assert D.RelativeHumidity(Warm()).model is not None


def test_symbol_struct_and_header(bz):
    import ctypes
    import os
    from breeze_jl_amd import _lib
    assert "bz_set_mixed_phase_equilibrium" in bz.SYMBOLS
    res, args = bz.SYMBOLS["bz_set_mixed_phase_equilibrium"]
    assert res is ctypes.c_int and len(args) == 3
    assert [n for n, _ in _lib.bz_mixed_phase_equilibrium._fields_] == ["freezing_temperature", "homogeneous_ice_nucleation_temperature",
                                                                        "ice_latent_heat", "ice_heat_capacity"]
    assert ctypes.sizeof(_lib.bz_mixed_phase_equilibrium) == 32 and ctypes.sizeof(_lib.types(4).bz_mixed_phase_equilibrium) == 16
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for header in ("breeze_hip.h", "breeze_hip_f32.h"):
        text = open(os.path.join(root, "include", header), encoding="utf-8").read()
        assert "int bz_set_mixed_phase_equilibrium(bz_ctx *ctx, const bz_mixed_phase_equilibrium *params," in text, header
