"""tests/diagnostics_reference.py (the numpy restatement the device diagnostics are held to) against reference-generated numbers —
the `model_diagnostics` doctest outputs of tests/golden/reference_doctests.json — and against closed forms; and the new entry points'
presence in the header, the ctypes binding and the generated Float32 header.  No GPU needed."""
import json
import os
import re

import numpy as np
import pytest

import diagnostics_reference as dr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "reference_doctests.json"), encoding="utf-8") as f:
        return json.load(f)["model_diagnostics"]


def _sig(x, digits=6):
    """Tolerance of a value printed with `digits` significant digits (Julia's Field summary prints 6): the rule of
    tests/test_golden_reference.py."""
    return 0.6 * 10.0 ** (np.floor(np.log10(abs(x))) - (digits - 1))


# golden entry -> (restatement kind, saturation adjustment?); the doctests set θ = 300 and the entry's qᵗ on the default model
ENTRIES = {
    "static_energy": ("STATIC_ENERGY", False),
    "virtual_potential_temperature": ("VIRTUAL_POTENTIAL_TEMPERATURE", False),
    "potential_temperature": ("POTENTIAL_TEMPERATURE", False),
    "liquid_ice_potential_temperature": ("LIQUID_ICE_POTENTIAL_TEMPERATURE", False),
    "equivalent_potential_temperature": ("EQUIVALENT_POTENTIAL_TEMPERATURE", False),
    "stability_equivalent_potential_temperature": ("STABILITY_EQUIVALENT_POTENTIAL_TEMPERATURE", False),
    "dewpoint_temperature": ("DEWPOINT_TEMPERATURE", True),
    "relative_humidity": ("RELATIVE_HUMIDITY", True),
}


def _column(oracle, gd, adjustment, z=(-1000.0, 0.0)):
    """T, qv, ql, p_r, rho_r, z of the doctest's column from the CPU oracle; extent = (., ., 1e3) puts z in (-1000, 0)."""
    Nz = gd["inputs"]["size"][2]
    g = oracle.Grid((4, 4, Nz), x=(0, 1.0), y=(0, 1.0), z=z)
    m = oracle.OracleModel(g, microphysics="SaturationAdjustment" if adjustment else None)
    m.set(theta=float(gd["inputs"]["set"]["theta"]), qt=float(gd["inputs"]["set"].get("qt", 0.0)))
    col = lambda f: np.ascontiguousarray(g.interior(f)[:, 0, 0])
    T = col(m.T)
    qv, ql = (col(m.qv), col(m.ql)) if adjustment else (col(m.q), np.zeros_like(T))
    sl = slice(g.Hz, g.Hz + g.Nz)
    return T, qv, ql, m.ref.pressure[sl].copy(), m.ref.density[sl].copy(), np.asarray(g.zc, dtype=np.float64), qv + ql


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_restatement_reproduces_reference_doctests(oracle, golden, entry):
    kind, adjustment = ENTRIES[entry]
    gd = golden[entry]
    T, qv, ql, p, rho, z, qe = _column(oracle, gd, adjustment)
    v = dr.evaluate(kind, T, qv, ql, p, rho, z, qe, dr.constants())
    digits = 5 if entry == "virtual_potential_temperature" else 6      # printed 301.82 / 301.8 / 301.81
    for key, x in (("max", v.max()), ("min", v.min()), ("mean", v.mean())):
        assert abs(x - gd[key]) <= _sig(gd[key], digits), (entry, key, x, gd[key])


def test_static_energy_doctest_needs_the_negative_z_range(oracle, golden):
    """with z = (0, 1e3) the static energy comes out ~409 J/kg lower than the doctest prints: the comparison above pins the z range"""
    gd = golden["static_energy"]
    T, qv, ql, p, rho, z, qe = _column(oracle, gd, False, z=(0.0, 1000.0))
    e = dr.evaluate("STATIC_ENERGY", T, qv, ql, p, rho, z, qe, dr.constants())
    assert 350.0 < gd["max"] - e.max() < 470.0 and 350.0 < gd["min"] - e.min() < 470.0


def test_array_saturation_pressure_is_the_oracles():
    from oracle import thermo
    tc, c = thermo.ThermoConstants(), dr.constants()
    T = np.linspace(200.0, 320.0, 49)
    want = np.array([thermo.saturation_vapor_pressure(t, tc, "liquid") for t in T])
    np.testing.assert_allclose(dr.saturation_vapor_pressure(T, c), want, rtol=4e-16)


def _random_state(seed=3, n=400):
    rng = np.random.default_rng(seed)
    return rng.uniform(230.0, 310.0, n), rng.uniform(4e4, 1.02e5, n)


def test_dry_air_collapses_every_potential_temperature():
    """q = 0: θᵛ = θˡⁱ = θ exactly; θᵉ = θᵇ = T (pˢᵗ/p)^κ · exp(0) · 0^(-0) agree with θ = T / (p/pˢᵗ)^κ to 1 ulp"""
    T, p = _random_state()
    c, z = dr.constants(), np.zeros_like(T)
    th = dr.potential_temperature(T, z, z, p, c)
    assert np.array_equal(dr.virtual_potential_temperature(T, z, z, p, c), th)
    assert np.array_equal(dr.liquid_ice_potential_temperature(T, z, z, p, c), th)
    for f in (dr.equivalent_potential_temperature, dr.stability_equivalent_potential_temperature):
        got = f(T, z, z, p, c)
        ulps = np.abs(got - th) / np.spacing(th)
        print(f.__name__, "max ulps", ulps.max())
        assert ulps.max() <= 1.0


def test_saturated_cell_has_unit_humidity_and_its_own_dewpoint():
    T, p = _random_state(seed=5)
    c, zero = dr.constants(), np.zeros_like(T)
    # qᵛ = qᵛ⁺(:prognostic) is a fixed point of q -> p^v+ / (rho*(q) R_v T); iterate to it
    qv = np.full_like(T, 1e-2)
    for _ in range(60):
        qv = dr.saturation_specific_humidity(T, qv, zero, p, c)
    H = dr.relative_humidity(T, qv, zero, p, c)
    np.testing.assert_allclose(H, 1.0, rtol=0, atol=8 * np.finfo(float).eps)
    # where rounding leaves p^v+ - p^v <= 0 the dewpoint IS T; elsewhere it sits within the solver's criterion of it
    Td = dr.dewpoint_temperature(T, qv, zero, p, c)
    pv = dr.vapor_pressure(T, qv, zero, p, c)
    assert np.all(np.abs(dr.saturation_vapor_pressure(Td, c) - pv) <= 1e-4 * pv)
    np.testing.assert_allclose(Td, T, rtol=0, atol=1e-9)
    sat = dr.saturation_vapor_pressure(T, c) - pv <= 0
    assert sat.any() and np.array_equal(Td[sat], T[sat])


def test_every_dewpoint_meets_the_solvers_criterion():
    """every dewpoint the secant iteration returns satisfies |p^v+(T+) - p^v| <= 1e-4 p^v; a cell with p^v+(T) - p^v <= 0 never enters
    the iteration and gets T itself (vapor_saturation.jl:320), whatever its residual"""
    rng = np.random.default_rng(11)
    T, p = _random_state(seed=7)
    qv, ql = rng.uniform(1e-3, 0.02, T.size), rng.uniform(0.0, 2e-3, T.size)
    c = dr.constants()
    Td = dr.dewpoint_temperature(T, qv, ql, p, c)
    pv = dr.vapor_pressure(T, qv, ql, p, c)
    sup = dr.saturation_vapor_pressure(T, c) - pv <= 0
    assert sup.sum() > 20 and (~sup).sum() > 20
    assert np.array_equal(Td[sup], T[sup])
    assert np.all(np.abs(dr.saturation_vapor_pressure(Td, c) - pv)[~sup] <= 1e-4 * pv[~sup])
    assert np.all(Td <= T)


def test_float32_restatement_stays_float32():
    c = dr.constants(np.float32)
    T, p = (a.astype(np.float32) for a in _random_state())
    qv, ql = np.full_like(T, 8e-3), np.full_like(T, 1e-3)
    for name in dr.NAMES[:-1]:
        v = dr.evaluate(name, T, qv, ql, p, p / (287 * T), T, qv + ql, c)
        assert v.dtype == np.float32, name


# ---- interface ----------------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("bz_compute_diagnostics", "bz_horizontal_average")


def _code(path):
    with open(os.path.join(ROOT, path), encoding="utf-8") as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


@pytest.mark.parametrize("header", ["include/breeze_hip.h", "include/breeze_hip_f32.h"])
def test_entry_points_are_declared(header):
    code = _code(header)
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), (header, name)
    assert "bz_diagnostic_inputs" in code and "BZ_DIAG_DEWPOINT_TEMPERATURE" in code
    if header.endswith("_f32.h"):
        assert not re.search(r"\bdouble\b", code)


def test_entry_points_are_prototyped_and_kinds_match_the_header(bz):
    from breeze_jl_amd import _lib
    for name in NEW_SYMBOLS:
        assert name in _lib.SYMBOLS
    code = _code("include/breeze_hip.h")
    for name, value in _lib.BZ_DIAG.items():
        assert re.search(r"\bBZ_DIAG_%s\s*=\s*%d\b" % (name, value), code), name
    assert tuple(_lib.DIAGNOSTIC_KINDS) == dr.NAMES
    assert re.search(r"#define\s+BZ_MAX_DIAGNOSTICS\s+%d\b" % _lib.BZ_MAX_DIAGNOSTICS, code)
    assert re.search(r"#define\s+BZ_DIAG_DENSITY_WEIGHTED\s+0x%x\b" % _lib.BZ_DIAG_DENSITY_WEIGHTED, code)


def test_unknown_flavour_raises_value_error(bz):
    class Stub:
        pass
    for op in (bz.PotentialTemperature, bz.StaticEnergy, bz.SaturationSpecificHumidity, bz.EquivalentPotentialTemperature):
        with pytest.raises(ValueError):
            op(Stub(), flavor="nonsense")
    with pytest.raises(ValueError):
        bz.SaturationSpecificHumidity(Stub(), "density")
    assert bz.SaturationSpecificHumidity(Stub(), "total_moisture").kind == "SATURATION_SPECIFIC_HUMIDITY_TOTAL_MOISTURE"
    with pytest.raises(NotImplementedError):
        bz.Average(bz.RelativeHumidity(Stub()), dims=(1,))
