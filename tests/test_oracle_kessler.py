"""Pins for the Kessler column microphysics oracle: the reference's own "Julia vs Fortran" fidelity test
(test/dcmip2016_kessler.jl:262-401) and helper checks (:212-258), restated.  No GPU needed."""
import numpy as np
import pytest


@pytest.fixture(scope="module")
def ks(oracle):
    from oracle import kessler
    return kessler


def reference_test_profile(ks):
    """Inputs of test/dcmip2016_kessler.jl:262-330."""
    Nz = 40
    zc = (np.arange(Nz) + 0.5) * (4000.0 / Nz)
    T_surface, p_surface, g, Rd, cpd, lapse = 288.0, 101325.0, 9.81, 287.0, 1003.0, 0.0065
    T = T_surface - lapse * zc
    p = p_surface * (T / T_surface) ** (g / (Rd * lapse))
    rho = p / (Rd * T)
    rv = 0.015 * np.exp(-((zc - 1000) / 1000) ** 2)
    rcl = np.where((zc > 1500) & (zc < 2500), 0.002, 0.0)
    rr = np.where((zc > 1000) & (zc < 2000), 0.0005, 0.0)
    R = 8.314462618
    Md = R / 287.0
    c = ks.TetensConstants(molar_gas_constant=R, dry_air_molar_mass=Md, vapor_molar_mass=Md, dry_air_heat_capacity=cpd,
                           vapor_heat_capacity=cpd, liquid_latent_heat=2500000.0, liquid_heat_capacity=cpd,
                           liquid_temperature_offset=36.0)
    rt = rv + rcl + rr
    return zc, T, p, rho, rv / (1 + rt), rcl / (1 + rt), rr / (1 + rt), c


def test_kernel_restatement_matches_fortran_translation(ks):
    """Physical fidelity: the kernel restatement and the independent DCMIP2016 translation agree to rtol 1e-12."""
    zc, T, p, rho, qv, qcl, qr, c = reference_test_profile(ks)
    mp = ks.KesslerParameters()
    dt, p0 = 10.0, 100000.0
    T_ref, qv_ref, qcl_ref, qr_ref = T.copy(), qv.copy(), qcl.copy(), qr.copy()
    ks.dcmip2016_fortran_reference(T_ref, qv_ref, qcl_ref, qr_ref, rho, p, dt, zc, c, mp, p0)
    theta = np.zeros_like(T)
    for k in range(len(T)):
        ql = qcl[k] + qr[k]
        cpm, Rm = ks.mixture_heat_capacity(qv[k], ql, c), ks.mixture_gas_constant(qv[k], ql, c)
        theta[k] = (T[k] - c.Ll * ql / cpm) / (p[k] / p0) ** (Rm / cpm)
    rtheta, rqv, rqcl, rqr = rho * theta, rho * qv, rho * qcl, rho * qr
    qv_k, qcl_k, qr_k, W, precip, Ns = ks.kessler_column_update(dt, rho, p, p0, zc, theta, rtheta, rqv, rqcl, rqr, mp, c)
    T_k = np.zeros_like(T)
    for k in range(len(T)):
        qv_b, qcl_b, qr_b = rqv[k] / rho[k], rqcl[k] / rho[k], rqr[k] / rho[k]
        th = rtheta[k] / rho[k]
        cpm, Rm = ks.mixture_heat_capacity(qv_b, qcl_b + qr_b, c), ks.mixture_gas_constant(qv_b, qcl_b + qr_b, c)
        T_k[k] = (p[k] / p0) ** (Rm / cpm) * th + c.Ll * (qcl_b + qr_b) / cpm
    np.testing.assert_allclose(T_k, T_ref, rtol=1e-12)
    np.testing.assert_allclose(rqv / rho, qv_ref, rtol=1e-12, atol=1e-300)
    np.testing.assert_allclose(rqcl / rho, qcl_ref, rtol=1e-12, atol=1e-300)
    np.testing.assert_allclose(rqr / rho, qr_ref, rtol=1e-12, atol=1e-300)
    assert precip >= 0 and Ns >= 1
    assert np.abs(T_ref - T).max() > 1e-3            # the step did something


def test_kessler_helpers(ks):
    """test/dcmip2016_kessler.jl:212-258: terminal velocity range / monotonicity, conversion round trip."""
    mp = ks.KesslerParameters()
    W = ks.terminal_velocity(0.001, 1.0, 1.2, mp)
    assert 0 < W < 20
    assert ks.terminal_velocity(0.0, 1.0, 1.2, mp) == 0.0
    assert ks.terminal_velocity(0.005, 1.0, 1.2, mp) > W
    qv, ql = 0.01, 0.002
    qt = qv + ql
    rv, rl = qv / (1 - qt), ql / (1 - qt)
    qv_b, ql_b = ks._fractions_of_ratios(rv, rl)
    assert qv_b == pytest.approx(qv, rel=1e-10) and ql_b == pytest.approx(ql, rel=1e-10)
    # water is conserved by one step of the column physics apart from surface precipitation
    c = ks.TetensConstants()
    assert ks.saturation_vapor_pressure_tetens(273.15, c) == 610.0


def test_oracle_model_with_kessler_runs_and_makes_rain(oracle):
    """AtmosphereModel(...; microphysics = DCMIP2016KesslerMicrophysics()) on the oracle: supersaturated moist bubble ->
    cloud -> rain; the species stay non-negative and the temperature diagnosis carries the liquid water."""
    g = oracle.Grid((8, 8, 20), x=(0, 4e3), y=(0, 4e3), z=(0, 5e3))
    m = oracle.OracleModel(g, surface_pressure=1e5, potential_temperature=300.0, microphysics="Kessler")
    bubble = lambda x, y, z: np.maximum(0.0, 1.0 - np.sqrt((x - 2e3) ** 2 + (y - 2e3) ** 2 + (z - 1500.0) ** 2) / 1200.0)
    m.set(qt=lambda x, y, z: 0.016 * np.exp(-z / 3000.0) + 0.004 * bubble(x, y, z),
          theta=lambda x, y, z: 300.0 + 0.004 * z + 1.0 * bubble(x, y, z),
          qcl=lambda x, y, z: 0.003 * bubble(x, y, z), qr=lambda x, y, z: 0.001 * bubble(x, y, z))
    I = g.interior
    assert I(m.qcl).max() > 2e-3 and np.allclose(I(m.ql), I(m.qcl) + I(m.qr))
    T0 = I(m.T).copy()
    for _ in range(3):
        m.time_step(5.0)
    for f in (m.rq, m.rqcl, m.rqr):
        assert np.isfinite(I(f)).all() and I(f).min() >= 0.0
    assert I(m.W).max() > 0.5 and np.abs(I(m.T) - T0).max() > 1e-2
    assert set(m.PROGNOSTIC) == {"ru", "rv", "rw", "rtheta", "rq", "rqcl", "rqr"}


def test_compressible_oracle_model_with_kessler(oracle):
    """CompressibleDynamics + DCMIP2016KesslerMicrophysics on the oracle: total density includes the condensates, the EOS
    temperature carries the latent term, a few steps run and total water changes only through surface precipitation."""
    from oracle import oracle_compressible as oc
    g = oracle.Grid((8, 8, 16), x=(0, 4e3), y=(0, 4e3), z=(0, 4e3))
    m = oc.CompressibleOracleModel(g, time_discretization=oc.SplitExplicit(substeps=6), surface_pressure=1e5,
                                   reference_potential_temperature=300.0, microphysics="Kessler")
    bub = lambda x, y, z: np.maximum(0.0, 1.0 - np.sqrt((x - 2e3) ** 2 + (y - 2e3) ** 2 + (z - 1500.0) ** 2) / 1200.0)
    rho = m.ref.density[g.Hz:g.Hz + g.Nz][:, None, None]
    m.set(rho=rho, theta=lambda x, y, z: 300.0 + 0.004 * z + 1.0 * bub(x, y, z), u=0.0, v=0.0, w=0.0,
          qv=lambda x, y, z: 0.014 * np.exp(-z / 3000.0) + 0.004 * bub(x, y, z),
          qcl=lambda x, y, z: 0.003 * bub(x, y, z), qr=lambda x, y, z: 0.001 * bub(x, y, z))
    I = g.interior
    np.testing.assert_allclose(I(m.rho), I(m.rho_d) + I(m.rq) + I(m.rqcl) + I(m.rqr), rtol=1e-15)
    # EOS consistency: theta = T (pst/p)^kappa - latent shift
    c, t = m.constants, m.tetens
    qv, ql = I(m.q), I(m.qcl) + I(m.qr)
    cpm = (1 - qv - ql) * c.cpd + qv * c.cpv + ql * t.cl
    Rm = (1 - qv - ql) * c.Rd + qv * c.Rv
    th_back = (I(m.T) - t.Ll * ql / cpm) * (m.pst / I(m.p)) ** (Rm / cpm)
    np.testing.assert_allclose(th_back, I(m.theta), rtol=1e-6)      # Newton abstol 1e-4 K
    for _ in range(2):
        m.time_step(2.0)
    for f in (m.rq, m.rqcl, m.rqr, m.rho_d):
        assert np.isfinite(I(f)).all()
    assert I(m.rqcl).min() >= 0 and I(m.rqr).min() >= 0 and I(m.W).max() > 0.5


# ---- the column case of tests/kessler_cases.py: what the device test relies on, asserted on the oracle ---------------------------------
import kessler_cases as kc          # noqa: E402


@pytest.mark.parametrize("variant", kc.VARIANTS)
def test_column_case_subcycle_spread(ks, variant):
    """The lanes of one wavefront need different numbers of sedimentation subcycles, the partly filled block subcycles too, and
    no dt / max_dt lies within 1e-3 of an integer, so a few-ulp pow on the device cannot change a column's count."""
    case, want, ratios = kc.oracle_case(ks, variant)
    Ns = want["Ns"]
    assert np.array_equal(np.maximum(1, np.ceil(ratios)).astype(int), Ns)       # subcycle_ratio restates the oracle's decision
    for j in range(kc.NY):
        full, tail = set(Ns[j, :64].tolist()), set(Ns[j, 64:].tolist())
        assert 1 in full and len(full) >= 4 and max(full) >= 6, (j, sorted(full))
        assert max(tail) > 1, (j, sorted(tail))
    assert (ratios[Ns > 1] > 1.0).all()
    assert kc.integer_distance(ratios) >= 1e-3
    print(f"kessler case [{variant}]: Ns {sorted(set(Ns.ravel().tolist()))}, integer distance {kc.integer_distance(ratios):.3f}")


@pytest.mark.parametrize("variant", kc.VARIANTS)
def test_column_case_reaches_every_branch(ks, variant):
    """Surface precipitation, rain on the top level, the three clamps, finite outputs."""
    case, want, _ = kc.oracle_case(ks, variant)
    P = want["precip"]
    assert (P > 0).sum() >= P.size // 2 and (P == 0).any() and (P >= 0).all()
    assert ((case["rqr"][-1] > 0) & (want["rqr"][-1] > 0)).any()               # top level: rain before and after
    for n in ("rqv", "rqcl", "rqr"):
        assert (case[n] < 0).any(), n
        assert (case[n] < 0).any(axis=0)[kc.negative_columns()].all() and not (case[n] < 0).any(axis=0)[~kc.negative_columns()].any()
        assert (want[n] >= 0).all(), n                                          # ... and clamped
    for n in kc.FIELDS + ("precip",):
        assert np.isfinite(want[n]).all(), n
    z = kc.z_centers()
    assert 60.0 < z[1] - z[0] < 90.0 and not np.allclose(np.diff(z), np.diff(z)[0])       # stretched: every dz lookup differs
    if variant == "arrays":                                                     # density and pressure genuinely 3-D
        for n in ("rho", "p"):
            assert np.ptp(case[n], axis=2).min() > 0 and np.ptp(case[n], axis=1).min() > 0, n
    print(f"kessler case [{variant}]: precipitation {P.min():.3g} .. {P.max():.3g}, {(P == 0).sum()} dry columns")


def test_column_case_conditioning(ks):
    """c1: how far the oracle's own outputs move, column-scaled, when every input moves by one unit in the last place.  The device
    tolerance is max(1e-11, 100 c1) with the recorded c1; the case must stay this well conditioned and the record must stay true."""
    c1 = 0.0
    for variant in kc.VARIANTS:
        case, want, _ = kc.oracle_case(ks, variant)
        for seed in (1, 2, 3):
            rng = np.random.default_rng(seed)
            moved = dict(case)
            for n in ("theta", "qv", "qcl", "qr"):
                moved[n] = case[n] * (1.0 + rng.choice([-1.0, 1.0], size=case[n].shape) * 2.0 ** -52)
            got = kc.run_oracle(ks, kc.densities(moved))
            assert np.array_equal(got["Ns"], want["Ns"])
            errs = kc.column_errors(got, want)
            c1 = max([c1, kc.precipitation_error(got["precip"], want["precip"])[0]] + [e for e, _ in errs.values()])
    print(f"kessler case: c1 = {c1:.2e} (recorded {kc.C1_MEASURED:.2e}), device tolerance {kc.TOL:.2e}")
    assert 100.0 * c1 <= 1e-11 * 2
    assert c1 <= 2.0 * kc.C1_MEASURED
    assert kc.TOL == max(1e-11, 100.0 * kc.C1_MEASURED)


@pytest.mark.parametrize("variant", kc.VARIANTS)
def test_kernel_restatement_matches_fortran_translation_with_subcycles(ks, variant):
    """The two independently written implementations at Ns >= 3, where the velocity refresh, dt / Ns and the order of the level
    updates matter: 1e-12 of each column's scale on T, q^v, q^cl, q^r (25x the 4.0e-14 measured on this case).  The Fortran translation
    does not clamp, so the columns with negative inputs are left out of this comparison."""
    case, want, _ = kc.oracle_case(ks, variant)
    c, mp = kc.constants(ks)
    zc = kc.z_centers()
    use = (want["Ns"] >= 3) & ~kc.negative_columns()
    assert use.sum() >= 100 and want["Ns"][use].max() >= 7
    worst = dict.fromkeys(("T", "qv", "qcl", "qr"), 0.0)
    for j, i in zip(*np.nonzero(use)):
        rho, p = case["rho"][:, j, i].copy(), case["p"][:, j, i].copy()
        qv, qcl, qr = (case[n][:, j, i] / rho for n in ("rqv", "rqcl", "rqr"))
        ql = qcl + qr
        cpm, Rm = ks.mixture_heat_capacity(qv, ql, c), ks.mixture_gas_constant(qv, ql, c)
        T = (p / kc.P0) ** (Rm / cpm) * case["theta"][:, j, i] + c.Ll * ql / cpm
        ks.dcmip2016_fortran_reference(T, qv, qcl, qr, rho, p, kc.DT, zc, c, mp, kc.P0)
        kqv, kqcl, kqr = (want[n][:, j, i] / rho for n in ("rqv", "rqcl", "rqr"))
        kql = kqcl + kqr
        cpm, Rm = ks.mixture_heat_capacity(kqv, kql, c), ks.mixture_gas_constant(kqv, kql, c)
        kT = (p / kc.P0) ** (Rm / cpm) * want["theta"][:, j, i] + c.Ll * kql / cpm
        for n, a, b in (("T", kT, T), ("qv", kqv, qv), ("qcl", kqcl, qcl), ("qr", kqr, qr)):
            scale = np.abs(b).max()
            err = np.abs(a - b).max() / scale if scale > 0 else (0.0 if not np.abs(a).max() else np.inf)
            worst[n] = max(worst[n], float(err))
    print(f"kessler restatement vs Fortran translation [{variant}], {use.sum()} columns:", {n: f"{e:.1e}" for n, e in worst.items()})
    assert all(e <= 1e-12 for e in worst.values()), worst


# ---- the whole-step cases of tests/kessler_cases.py ---------------------------------------------------------------------------------------
def _stepped(ks, om, dt, steps, density, seed=None, names=()):
    if seed is not None:
        kc.move_by_one_ulp(om, names, seed)
    record = kc.record_subcycling(ks, om, dt, density)
    for _ in range(steps):
        record["measure"]()
        om.time_step(dt)
    return record


def _assert_steps_conditioning(label, a, b, names):
    errs = kc.field_scale_errors(a, b, names)
    print(f"{label}: the oracle under a one-ulp change of its initial state:", {n: f"{e:.1e}" for n, e in errs.items()})
    assert all(e <= kc.STEPS_CONDITIONING for e in errs.values()), errs


def test_anelastic_steps_case_subcycles_and_is_well_conditioned(oracle, ks):
    """kc.ANELASTIC_STEPS: columns at Ns = 1 and Ns >= 3 before every step and at every column update, no dt / max_dt within 1e-3
    of an integer, rain on the ground, and an oracle that moves by less than a quarter of the device tolerance when its initial
    state moves by one unit in the last place."""
    case = kc.ANELASTIC_STEPS
    runs = []
    for seed in (None, 1):
        om = kc.anelastic_oracle(oracle, **case)
        om.set(**kc.anelastic_initial_conditions(case["bubble_height"]))
        g = om.grid
        rho = np.ascontiguousarray(om.ref.density[g.Hz:g.Hz + g.Nz])
        record = _stepped(ks, om, case["dt"], case["steps"], lambda: rho, seed, ("ru", "rtheta", "rq", "rqcl", "rqr"))
        runs.append(om)
        if seed is None:
            kc.assert_subcycling("anelastic", record, case["steps"])
            assert om.precipitation_rate.max() > 1e-3
    _assert_steps_conditioning("anelastic", runs[0], runs[1], ("ru", "rw", "rtheta", "rq", "rqcl", "rqr", "T", "W"))


def test_compressible_steps_case_subcycles_and_is_well_conditioned(oracle, ks):
    """kc.COMPRESSIBLE_STEPS, as above, with a density that varies along x."""
    from oracle import oracle_compressible as oc
    case = kc.COMPRESSIBLE_STEPS
    runs = []
    for seed in (None, 1):
        om = kc.compressible_oracle(oracle, oc, **case)
        kc.set_compressible_oracle(om, **case)
        g = om.grid
        record = _stepped(ks, om, case["dt"], case["steps"], lambda: g.interior(om.rho_d), seed, ("ru", "rtheta", "rq", "rqcl", "rqr", "rho_d"))
        runs.append(om)
        if seed is None:
            kc.assert_subcycling("compressible", record, case["steps"])
            assert om.precipitation_rate.max() > 1e-3 and np.ptp(g.interior(om.rho_d), axis=2).max() > 1e-3
    _assert_steps_conditioning("compressible", runs[0], runs[1], ("rho_d", "ru", "rw", "rtheta", "rq", "rqcl", "rqr", "T", "p", "W"))
