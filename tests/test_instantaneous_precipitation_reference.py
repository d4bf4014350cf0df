"""tests/instantaneous_precipitation_reference.py against the reference's own tests of InstantaneousPrecipitation
(test/instantaneous_precipitation.jl): the parity of the delegated update with the pre-refactor inline formulas (:38-127), the integration
scenario of the once-per-step kernel (:131-217), the persistence of the rate in a cell that stops condensing, the skipped update, and the
host side (constructors that refuse, the pinned refusal messages, the symbol table).  CPU only."""
import math

import numpy as np
import pytest

import instantaneous_precipitation_reference as ipr
from oracle import thermo


# ---- the reference's parity test ---------------------------------------------------------------------------------------------------------
def reference_ip_update(theta0, qt, rho, pst, c):
    """reference_ip_update (test/instantaneous_precipitation.jl:38-84): the pre-refactor scalar math, restated here and nowhere else — a
    constant-density secant on theta^li run for 40 iterations plus the closed-form vapour-only rain-out"""
    def residual(T):
        qs = thermo.saturation_specific_humidity(T, rho, c, "liquid")
        ql = max(0, qt - qs)                        # equilibrated_moisture_mass_fractions, warm phase
        qv = qt - ql
        Rm, cpm = thermo.mixture_gas_constant(qv, ql, 0.0, c), thermo.mixture_heat_capacity(qv, ql, 0.0, c)
        L = (c.Ll * ql + c.Li * 0.0) / cpm
        p = rho * Rm * T
        return (T - L) * (pst / p) ** (Rm / cpm) - theta0, (qv, ql)

    Rt, cpt = thermo.mixture_gas_constant(qt, 0.0, 0.0, c), thermo.mixture_heat_capacity(qt, 0.0, 0.0, c)
    gt = cpt / (cpt - Rt)
    T1 = theta0 ** gt * (rho * Rt / pst) ** (gt - 1)
    r1, q1 = residual(T1)
    cp1 = thermo.mixture_heat_capacity(q1[0], q1[1], 0.0, c)
    L1 = (c.Ll * q1[1]) / cp1
    T2 = T1 + max(0.01, gt * L1)
    r2, _ = residual(T2)
    T = T2
    for _ in range(40):
        d = (T2 - T1) / (r2 - r1) if r2 != r1 else math.inf
        d = d if math.isfinite(d) else 0.0
        T1, r1 = T2, r2
        T2 = T2 - r2 * d
        r2, _ = residual(T2)
        T = T2
    _, (qv, ql) = residual(T)
    Rf, cpf = thermo.mixture_gas_constant(qv, 0.0, 0.0, c), thermo.mixture_heat_capacity(qv, 0.0, 0.0, c)
    gf = cpf / (cpf - Rf)
    theta_f = T ** (1 / gf) * (rho * Rf / pst) ** ((1 - gf) / gf)
    return dict(T=T, qv=qv, qc=ql, theta_f=theta_f)


def approx(a, b, rtol):
    return abs(a - b) <= rtol * max(abs(a), abs(b))


@pytest.mark.parametrize("theta0,qt", [(300.0, 0.030), (295.0, 0.022), (305.0, 0.045)])
def test_supersaturated_parcels_match_the_pre_refactor_formulas(theta0, qt):
    c = thermo.ThermoConstants()
    new = ipr.ip_update(theta0, qt, 1.0, 1e5, c, abstol=1e-12, maxiter=100)
    ref = reference_ip_update(theta0, qt, 1.0, 1e5, c)
    assert new["qc"] > 0
    for n in ("T", "qv", "qc", "theta_f"):
        assert approx(new[n], ref[n], 1e-9), (n, new[n], ref[n])
    assert new["theta_f"] > theta0


def test_subsaturated_parcel_round_trips():
    new = ipr.ip_update(300.0, 0.001, 1.0, 1e5, abstol=1e-12, maxiter=100)
    assert new["qc"] == 0
    assert approx(new["qv"], 0.001, 1e-9) and approx(new["theta_f"], 300.0, 1e-9)


@pytest.mark.parametrize("theta0,qt,rho", [(300.0, 0.030, 1.0), (295.0, 0.022, 1.0), (305.0, 0.045, 1.0), (300.0, 0.001, 1.0),
                                           (300.3, 0.0187, 1.0931), (288.0, 0.0161, 0.8642)])
def test_typed_formulas_in_float64_are_the_scalar_update(theta0, qt, rho):
    """in_dtype(numpy.float64) restates oracle/thermo.py on numpy scalars: the same numbers (one rounding of libm's pow apart at the most),
    the same branch; in numpy.float32 the result is a float32 within the reference's Float32 figures of the Float64 one (abstol = 1e-6,
    rtol = 1e-4, test/instantaneous_precipitation.jl:104-106)"""
    a = ipr.ip_update(theta0, qt, rho, 1e5)
    b = ipr.in_dtype(np.float64).ip_update(theta0, qt, rho, 1e5)
    assert (a["qc"] > 0) == (b["qc"] > 0)
    for n in ("T", "qv", "qc", "theta_f"):
        assert abs(a[n] - b[n]) <= 1e-13 * max(abs(a[n]), 1e-3), (n, a[n], b[n])
    a = ipr.ip_update(theta0, qt, rho, 1e5, abstol=1e-6)
    s = ipr.in_dtype(np.float32).ip_update(theta0, qt, rho, 1e5, abstol=1e-6)
    for n in ("T", "qv", "theta_f"):
        assert type(s[n]) is np.float32, n
        assert approx(float(s[n]), a[n], 1e-4), (n, s[n], a[n])


# ---- the reference's integration scenario ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scenario(oracle, oc):
    def build(qt):
        om, _, _ = ipr.make_restatement(oracle, oc, (8, 8, 8), 5)
        g = om.grid
        om.set(rho=om.ref.density[g.Hz:g.Hz + g.Nz][:, None, None], theta=300.0, qv=qt)
        om.update_state()
        return om
    return build


def test_supersaturated_scenario_condenses_rains_out_and_keeps_the_warming(scenario):
    om = scenario(0.030)
    g, tc = om.grid, thermo.ThermoConstants()
    I = g.interior
    rt, rd, rth0, rq0 = (I(f).copy() for f in (om.rho, om.rho_d, om.rtheta, om.rq))
    assert np.all(I(om.precipitation_rate) == 0)
    om.microphysics_model_update(1.0)
    rth1, rq1, P = I(om.rtheta).copy(), I(om.rq).copy(), I(om.precipitation_rate).copy()
    assert np.all(np.isfinite(rth1)) and np.all(np.isfinite(rq1))
    assert np.all(rq1 < rq0) and np.all(rth1 > rth0) and np.all(P > 0) and om.condensed.all()
    flux = om.surface_precipitation_flux()
    assert np.all(flux > 0)
    dz = g.dzc[g.Hz:g.Hz + g.Nz]
    assert np.allclose(flux, np.einsum("kji,k->ji", P, dz), rtol=1e-14, atol=0)
    assert np.all(np.abs(P - (rq0 - rq1) / 1.0) <= 1e-6 * np.abs(P))          # water budget
    for idx in np.ndindex(rt.shape):      # the vapour-only post-state sits on the saturation curve at the cell's own (pre-update) total density
        qv, thf = rq1[idx] / rt[idx], rth1[idx] / rd[idx]
        T = thermo.density_state_temperature(thf, qv, 0.0, rt[idx], om.pst, tc)
        assert abs(qv - thermo.saturation_specific_humidity(T, rt[idx], tc, "liquid")) < 1e-4
    assert np.allclose(I(om.rho), rd + rq1, rtol=1e-15)      # the trailing update_state!: the total density dropped by the rain
    om.update_state()                                        # a following update_state! preserves the diagnostic
    assert np.array_equal(I(om.precipitation_rate), P)


def test_subsaturated_scenario_is_a_no_op(scenario):
    om = scenario(0.001)
    I = om.grid.interior
    rth0, rq0 = I(om.rtheta).copy(), I(om.rq).copy()
    om.microphysics_model_update(1.0)
    assert np.all(np.abs(I(om.rtheta) - rth0) <= 1e-8 * np.abs(rth0))
    assert np.all(np.abs(I(om.rq) - rq0) <= 1e-8 * np.abs(rq0))
    assert np.all(I(om.precipitation_rate) == 0) and not om.condensed.any()


def test_a_cell_that_stops_condensing_keeps_its_rate(scenario):
    """the reference's ifelse keeps the old value where nothing condenses (instantaneous_precipitation.jl:181-183)"""
    om = scenario(0.030)
    I = om.grid.interior
    om.microphysics_model_update(1.0)
    P1 = I(om.precipitation_rate).copy()
    assert np.all(P1 > 0)
    dry = (slice(0, 4), slice(None), slice(None))
    I(om.rq)[dry] *= 0.5                    # the lower half loses half its vapour: no condensation there in the second update
    om.update_state()
    om.microphysics_model_update(2.0)
    P2 = I(om.precipitation_rate)
    assert not om.condensed[dry].any() and np.array_equal(P2[dry], P1[dry])
    assert om.condensed[4:].all() and np.all(P2[4:] != P1[4:])


@pytest.mark.parametrize("dt", [math.nan, math.inf, -math.inf, 0.0, -1.0])
def test_update_is_skipped_for_an_invalid_time_step(scenario, dt):
    om = scenario(0.030)
    before = {n: getattr(om, n).copy() for n in ("rho", "rho_d", "rtheta", "rq", "T", "p", "q", "precipitation_rate")}
    before["G"] = om.G["rq"].copy()
    om.microphysics_model_update(dt)
    om.microphysics_model_update()           # clock.last_dt before the first step is infinite
    for n, a in before.items():
        assert np.array_equal(a, om.G["rq"] if n == "G" else getattr(om, n)), n


def test_mixed_bubble_has_cloudy_and_clear_cells_on_every_test_grid(oracle, oc):
    """the precondition of tests/test_instantaneous_precipitation.py, on the restatement alone: between 2 % and 98 % of the cells condense"""
    for shape, halo in (((8, 8, 8), 5), ((40, 6, 5), 3), ((40, 10, 5), 5), ((66, 6, 4), 3), ((130, 9, 6), 3), ((258, 6, 3), 3)):
        for stretched in (False, True):
            om, ext, L = ipr.make_restatement(oracle, oc, shape, halo, stretched)
            g = om.grid
            th, qt = ipr.bubble_state(*L)
            x, y, z = g.nodes("ccc")
            rho = om.ref.density[g.Hz:g.Hz + g.Nz][:, None, None] * np.ones((g.Nz, g.Ny, g.Nx))
            thv, qv = np.broadcast_to(th(x, y, z), rho.shape), np.broadcast_to(qt(x, y, z), rho.shape)
            wet = np.array([ipr.ip_update(float(t), float(q), float(r), 1e5)["qc"] > 0 for t, q, r in zip(thv.ravel(), qv.ravel(), rho.ravel())])
            assert 0.02 < wet.mean() < 0.98, (shape, stretched, wet.mean())


# ---- host ----------------------------------------------------------------------------------------------------------------------------------
class Unknown:
    pass


def _grid(bz, topology=None):
    kw = {} if topology is None else dict(topology=topology)
    return bz.RectilinearGrid((16, 16, 8), x=(0, 1e3), y=(0, 1e3), z=(0, 1e3), **kw)


def _dynamics(bz):
    return bz.CompressibleDynamics(bz.SplitExplicitTimeDiscretization(substeps=6))


def test_class_wraps_a_saturation_adjustment(bz):
    from breeze_jl_amd.microphysics import MixedPhaseEquilibrium
    ip = bz.InstantaneousPrecipitation()
    assert isinstance(ip.saturation_adjustment, bz.SaturationAdjustment)
    assert isinstance(ip.saturation_adjustment.equilibrium, bz.WarmPhaseEquilibrium)
    assert (ip.saturation_adjustment.solver.abstol, ip.saturation_adjustment.solver.maxiter) == (1e-4, 20)
    ip = bz.InstantaneousPrecipitation(equilibrium=bz.WarmPhaseEquilibrium(), solver=bz.SecantSolver(abstol=1e-6, maxiter=50))
    assert (ip.saturation_adjustment.solver.abstol, ip.saturation_adjustment.solver.maxiter) == (1e-6, 50)
    with pytest.raises(NotImplementedError, match="MixedPhaseEquilibrium"):
        bz.InstantaneousPrecipitation(equilibrium=MixedPhaseEquilibrium())
    with pytest.raises(NotImplementedError):
        bz.InstantaneousPrecipitation(equilibrium=Unknown())


def test_constructors_that_refuse_name_the_scheme(bz):
    """the anelastic model, the kinematic driver, the slab models and the walled compressible model: new messages for the new class, raised
    where the microphysics type is checked (before anything needs a GPU)"""
    ip = bz.InstantaneousPrecipitation()
    grid = _grid(bz)
    ref = bz.ReferenceState(grid, potential_temperature=300.0)
    cases = {
        "anelastic": lambda: bz.AtmosphereModel(grid, dynamics=bz.AnelasticDynamics(ref), advection=bz.WENO(order=5), microphysics=ip),
        "kinematic": lambda: bz.AtmosphereModel(grid, dynamics=bz.PrescribedDynamics(ref), advection=bz.WENO(order=5), microphysics=ip),
        "walls": lambda: bz.CompressibleAtmosphereModel(_grid(bz, (bz.Periodic, bz.Bounded, bz.Bounded)), _dynamics(bz), advection=bz.WENO(order=5),
                                                        microphysics=ip),
        "flat y": lambda: bz.CompressibleAtmosphereModel(bz.RectilinearGrid((16, 8), x=(0, 1e3), z=(0, 1e3), topology=(bz.Periodic, bz.Flat, bz.Bounded)),
                                                         _dynamics(bz), advection=bz.WENO(order=5), microphysics=ip),
        # (the device is named, so that no constructor asks torch for the current one before it validates)
        "compressible slab": lambda: bz.compressible.SlabCompressibleModel(grid, 0, 1, _dynamics(bz), advection=bz.WENO(order=5), microphysics=ip,
                                                                           device="cuda:0"),
        # (SlabAtmosphereModel takes no microphysics at all)
        "anelastic library slab": lambda: distributed.LibrarySlabAtmosphereModel(grid, 0, 1, advection=bz.WENO(order=5), microphysics=ip,
                                                                                 device="cuda:0"),
    }
    from breeze_jl_amd import distributed
    for name, make in cases.items():
        with pytest.raises(NotImplementedError, match="InstantaneousPrecipitation"):
            make()


def test_unknown_microphysics_keeps_the_pinned_messages(bz):
    """literals copied from tests/test_model_validation.py"""
    grid = _grid(bz)
    ref = bz.ReferenceState(grid, potential_temperature=300.0)
    with pytest.raises(NotImplementedError) as e:
        bz.CompressibleAtmosphereModel(grid, _dynamics(bz), advection=bz.WENO(order=5), microphysics=Unknown())
    assert str(e.value) == ("compressible microphysics: DCMIP2016KesslerMicrophysics() and SaturationAdjustment(equilibrium = "
                            "WarmPhaseEquilibrium()) are implemented")
    with pytest.raises(NotImplementedError) as e:
        bz.AtmosphereModel(grid, dynamics=bz.AnelasticDynamics(ref), advection=bz.WENO(order=5), microphysics=Unknown())
    assert str(e.value) == ("microphysics: SaturationAdjustment(equilibrium = WarmPhaseEquilibrium()) and "
                            "DCMIP2016KesslerMicrophysics() are implemented")


def test_symbol_table_and_exports(bz):
    for name in ("bz_set_instantaneous_precipitation", "bz_instantaneous_precipitation_update", "bz_column_integral"):
        assert name in bz.SYMBOLS, name
    for name in ("InstantaneousPrecipitation", "precipitation_rate", "surface_precipitation_flux"):
        assert hasattr(bz, name), name
