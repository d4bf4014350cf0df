"""CPU pins of tests/saturation_adjustment_reference.py: the float64 restatement returns the bits of oracle/thermo.py (whose known answers
are the reference's, tests/test_golden_reference.py), the sweeps meet the conditions the device tests rely on, and the restatement's own
rounding sensitivity (float64 against longdouble: d80; float32 against float64: d32) is measured per population.  The d80 table printed
here is the one tests/test_saturation_adjustment_parcels.py takes its bounds from (sar.d80) and DESIGN.md quotes."""
import numpy as np
import pytest

import saturation_adjustment_reference as sar
from oracle import thermo

F64, LD, F32 = np.float64, np.longdouble, np.float32
DENSITY = [("density", s, sar.COLUMN) for s in sar.COMPRESSIBLE_GRIDS]
PRESSURE = [("pressure", s, sar.COLUMN) for s in sar.ANELASTIC_GRIDS]
CASES = DENSITY + PRESSURE
IDS = [f"{f}-{s[0]}x{s[1]}x{s[2]}" for f, s, _ in CASES]


def solvers_of(form, shape):
    if form == "pressure":
        return (sar.DEFAULT_SOLVER, (0.0, 50)) + (((1e-4, 2), (1e-4, 0)) if shape == (66, 8, 12) else ())
    return sar.SOLVERS + (((1e-4, 1),) if shape == (66, 6, 4) else ())


def tags(form, shape):
    return (sar.compressible_case(shape) if form == "density" else sar.anelastic_case(shape)).tag


@pytest.mark.parametrize("form,shape,Lz", CASES, ids=IDS)
def test_float64_restatement_returns_the_oracles_bits(form, shape, Lz):
    c = thermo.ThermoConstants()
    for solver in solvers_of(form, shape):
        r = sar.restated(form, shape, 1, F64, solver)
        case = sar.anelastic_case(shape) if form == "pressure" else None
        for idx in np.ndindex(r.T.shape):
            th, q = float(r.theta[idx]), float(r.q[idx])
            if form == "density":
                want = thermo.adjust_warm_phase_density(th, q, float(r.rho[idx]), sar.PST, c, solver[0], solver[1], *sar.NEWTON)
            else:
                want = thermo.adjust_warm_phase(th, q, float(case.p_r[idx[0]]), sar.PST, c, solver[0], solver[1])
            got = (float(r.T[idx]), float(r.qv[idx]), float(r.ql[idx]))
            assert got == tuple(float(w) for w in want), (solver, idx, got, want)


def newtons_of(shape):
    return (sar.NEWTON,) + (sar.LOOSE_NEWTONS if shape == (66, 6, 4) else ())


@pytest.mark.parametrize("shape", sar.COMPRESSIBLE_GRIDS, ids=str)
@pytest.mark.parametrize("mp", [0, 2])
def test_float64_newton_inversions_return_the_oracles_bits(shape, mp):
    c = thermo.ThermoConstants()
    for newton in newtons_of(shape):
        r = sar.restated("density", shape, mp, F64, newton=newton)
        assert not r.nonfinite.any(), newton
        for idx in np.ndindex(r.T.shape):
            want = thermo.density_state_temperature(float(r.theta[idx]), float(r.qv[idx]), float(r.ql[idx]), float(r.rho[idx]), sar.PST, c, *newton)
            assert float(r.T[idx]) == want, (newton, idx, r.T[idx], want)


@pytest.mark.parametrize("newton", sar.LOOSE_NEWTONS, ids=str)
def test_float64_restatement_under_other_temperature_solvers_returns_the_oracles_bits(newton):
    """The density form on (66, 6, 4) under the default secant with the temperature solvers that leave on maxiter = 0, maxiter = 1 and
    abstol = 1 K: the bits of oracle/thermo.py, no non-finite intermediate, no knife-edge parcel; d80 stays a rounding figure"""
    c, shape = thermo.ThermoConstants(), (66, 6, 4)
    r = sar.restated("density", shape, 1, F64, newton=newton)
    assert not r.nonfinite.any() and not r.knife.any()
    for idx in np.ndindex(r.T.shape):
        want = thermo.adjust_warm_phase_density(float(r.theta[idx]), float(r.q[idx]), float(r.rho[idx]), sar.PST, c, *sar.DEFAULT_SOLVER, *newton)
        got = (float(r.T[idx]), float(r.qv[idx]), float(r.ql[idx]))
        assert got == tuple(float(w) for w in want), (newton, idx, got, want)
    wide = sar.restated("density", shape, 1, LD, newton=newton)
    free = (tags("density", shape) == "marginal_edge")
    assert np.array_equal(r.branch[~free], wide.branch[~free]) and np.array_equal(r.iterations[~free], wide.iterations[~free])
    for name, (dT, dv, dl) in sar.d80("density", shape, 1, newton=newton).items():
        print(f"D80 density {shape} newton={newton} {name}: T={dT:.1e} qv={dv:.1e} ql={dl:.1e}")
        assert dT <= 1e-11 and dv <= 1e-12 and dl <= 1e-12, (newton, name)
    for mp in (0, 2):
        for name, row in sar.d80("density", shape, mp, newton=newton).items():
            assert row[0] <= 1e-14, (newton, mp, name, row)


@pytest.mark.parametrize("shape", sar.ANELASTIC_GRIDS, ids=str)
@pytest.mark.parametrize("mp", [0, 2])
def test_float64_closed_forms_return_the_oracles_bits(shape, mp):
    c = thermo.ThermoConstants()
    case = sar.anelastic_case(shape)
    r = sar.restated("pressure", shape, mp, F64)
    for idx in np.ndindex(r.T.shape):
        want = thermo.theta_state_temperature(float(r.theta[idx]), float(r.qv[idx]), float(r.ql[idx]), float(case.p_r[idx[0]]), sar.PST, c)
        assert float(r.T[idx]) == want, (idx, r.T[idx], want)
    assert not r.nonfinite.any()
    if mp == 2:
        assert (r.ql > 0).mean() > 0.3      # the planted condensate is there


def test_reference_columns_stay_inside_the_tested_domain():
    for shape in sar.ANELASTIC_GRIDS:
        p, rho = sar.reference_column(shape[2], sar.COLUMN)
        assert p.min() >= 20e3 and np.all(np.diff(p) < 0) and np.all(rho > 0)
        assert sar.reference_column(shape[2], sar.TALL_COLUMN)[0][-1] < 2e3


@pytest.mark.parametrize("form,shape,Lz", CASES, ids=IDS)
def test_sweep_conditions(form, shape, Lz):
    tag = tags(form, shape)
    for name in ("bulk", "negative_or_zero_q", "marginal", "marginal_edge", "guess_switch", "theta_zero"):
        assert (tag == name).any(), name
    for solver in solvers_of(form, shape):
        r = sar.restated(form, shape, 1, F64, solver)
        assert not r.nonfinite.any(), (solver, int(r.nonfinite.sum()))
        cloudy = r.branch == sar.CLOUDY
        knife = int((r.knife & cloudy).sum())
        print(f"SWEEP {form} {shape} solver={solver}: clear={np.mean(r.branch == sar.CLEAR):.2f} cloudy={cloudy.mean():.2f} "
              f"iterations={sorted(set(r.iterations[cloudy]))} knife-edge={knife}/{int(cloudy.sum())}")
        assert np.mean(r.branch == sar.CLEAR) >= 0.2 and cloudy.mean() >= 0.2
        assert knife <= 0.005 * cloudy.sum()
        qt = r.q[r.branch != sar.THETA_ZERO]
        assert qt.max() <= sar.Q_CAP * (1 + 1e-12) and qt.min() >= -1e-5 * (1 + 1e-12)
    for which in (0, 1):
        r = sar.restated(form, shape, 1, F64, sar.DEFAULT_SOLVER, which=which)
        assert set(range(7)) <= set(r.iterations.ravel())      # 0: the clear parcels (and the theta = 0 guard)
        branches, counts = sar.wavefront_mixing(r)
        assert branches == 2 and counts >= 3, (which, branches, counts)
    # the second placement holds the same parcels on the same levels
    a, b = (sar.compressible_case(shape, w) if form == "density" else sar.anelastic_case(shape, Lz, w) for w in (0, 1))
    assert not np.array_equal(a.parcel, b.parcel)
    for k in range(shape[2]):
        assert np.array_equal(np.sort(a.parcel[k].ravel()), np.sort(b.parcel[k].ravel()))
        oa, ob = np.argsort(a.parcel[k].ravel()), np.argsort(b.parcel[k].ravel())
        for n in ("rtheta", "rq"):
            assert np.array_equal(a[n][k].ravel()[oa], b[n][k].ravel()[ob])


@pytest.mark.parametrize("form,shape,Lz", CASES, ids=IDS)
def test_guess_switch_parcels_straddle_the_floor(form, shape, Lz):
    """dT / 2 of the second guess sits at the four targets to 1e-10 relative, a tenth of their distance 1e-9 from the floor: below the floor 0.01 for the first two, above it for the others"""
    r = sar.restated(form, shape, 1, F64)
    case = sar.compressible_case(shape) if form == "density" else sar.anelastic_case(shape)
    sel = case.tag == "guess_switch"
    assert np.all(r.branch[sel] == sar.CLOUDY)
    assert np.all(np.abs(r.half_step[sel] / case.sub[sel] - 1) <= 1e-10)       # the rounding of rho q / rho moves it by up to 1e-11
    assert set(np.unique(case.sub[sel])) == set(sar.GUESS_HALF_STEPS)
    assert {bool(h > 0.01) for h in r.half_step[sel]} == {True, False}


def test_exp_small_population_takes_zero_one_and_two_halvings():
    for shape in sar.ANELASTIC_GRIDS:
        case = sar.anelastic_case(shape, sar.TALL_COLUMN, 0, True)
        r = sar.restated("pressure", shape, 0, F64, Lz=sar.TALL_COLUMN, exp_small=True)
        sel = case.tag == "exp_small"
        assert sel.sum() == 12 and not sel[:-1].any() and not r.nonfinite.any()
        assert set(r.halvings[sel]) == {0, 1, 2}, set(r.halvings[sel])
        assert set(r.halvings[~sel]) == {0}
        rows = sel[-1].any(axis=1)           # every such row of lanes mixes the counts with ordinary lanes
        assert rows.any() and not sel[-1][rows].all()


@pytest.mark.parametrize("form,shape,Lz", CASES, ids=IDS)
def test_float64_against_longdouble(form, shape, Lz):
    """Same branch outside the threshold and knife-edge parcels, the same iteration count where abstol > 0; d80 per population"""
    tag = tags(form, shape)
    for solver in solvers_of(form, shape):
        a, b = sar.restated(form, shape, 1, F64, solver), sar.restated(form, shape, 1, LD, solver)
        free = (tag == "marginal_edge") | a.knife
        assert np.array_equal(a.branch[~free], b.branch[~free]), solver
        if solver[0] > 0:
            assert np.array_equal(a.iterations[~free], b.iterations[~free]), solver
        table = sar.d80(form, shape, 1, solver)
        for name, (dT, dv, dl) in table.items():
            print(f"D80 {form} {shape} solver={solver} {name}: T={dT:.1e} qv={dv:.1e} ql={dl:.1e}")
            assert dT <= 1e-11 and dv <= 1e-12 and dl <= 1e-12, (solver, name, dT, dv, dl)      # a restatement this sensitive would bound nothing
    for mp in (0, 2):
        for name, row in sar.d80(form, shape, mp).items():
            print(f"D80 {form} {shape} MP={mp} {name}: T={row[0]:.1e}")
            assert row[0] <= 1e-14, (mp, name, row)


@pytest.mark.parametrize("form,shape,Lz", [CASES[1], CASES[3]], ids=[IDS[1], IDS[3]])
@pytest.mark.parametrize("abstol", [1e-4, 1e-6, 0.0])
def test_float32_against_float64(form, shape, Lz, abstol):
    """d32 on the Float32-rounded inputs, per population, as the device test forms it; within the reference's own Float32 figure (rtol 1e-4)"""
    solver = (abstol, 20)
    if form == "density":
        case = sar.compressible_case(shape)
        arrays = {n: case[n].astype(F32) for n in ("rho_d", "rtheta", "rq")}
        a = sar.diagnose_compressible(arrays, 1, F32, solver)
        b = sar.diagnose_compressible({n: v.astype(F64) for n, v in arrays.items()}, 1, F64, solver)
    else:
        case = sar.anelastic_case(shape)
        arrays = {n: case[n].astype(F32) for n in ("rtheta", "rq")}
        p, rho = case.p_r.astype(F32), case.rho_r.astype(F32)
        a = sar.diagnose_anelastic(arrays, 1, p, rho, F32, solver)
        b = sar.diagnose_anelastic({n: v.astype(F64) for n, v in arrays.items()}, 1, p.astype(F64), rho.astype(F64), F64, solver)
    assert a.T.dtype == F32 and not a.nonfinite.any()
    same = a.branch == b.branch
    d = sar.distances(a, b)
    for name in sar.POPULATIONS:
        sel = (case.tag == name) & same
        if sel.any():
            print(f"D32 {form} abstol={abstol:g} {name}: T={d['T'][sel].max():.1e} qv={d['qv'][sel].max():.1e} ql={d['ql'][sel].max():.1e} "
                  f"other branch: {int(((case.tag == name) & ~same).sum())}")
    bulk = case.tag == "bulk"
    assert (bulk & ~same).sum() <= 0.002 * bulk.sum()
    assert d["T"][bulk & same].max() <= 1e-4 and d["qv"][bulk & same].max() <= 1e-4 * sar.Q_CAP


# ---- the judging rules have teeth: restatements with one planted error, judged as a device result would be --------------------------------
class _NoLiquidHeat(sar.Typed):
    def _mix(self, qv, ql):
        qd = self.dtype(1) - (qv + ql)
        return qd * self.Rd + qv * self.Rv, qd * self.cpd + qv * self.cpv


class _WiderFloor(sar.Typed):
    def _second_guess(self, T1, qv1, ql1, tr):
        return T1 + max(self.dtype(0.02), (self.Ll * ql1) / self._mix(qv1, ql1)[1] / self.dtype(2))


class _OneIterationMore(sar.Typed):
    def _secant(self, residual, x1, x2, abstol, maxiter, tr):
        return super()._secant(residual, x1, x2, abstol, maxiter + 1, tr)


class _NewtonIgnoresAbstol(sar.Typed):
    def temperature(self, theta, qv, ql, rho, pst, abstol, maxiter):
        return super().temperature(theta, qv, ql, rho, pst, self.dtype(0), maxiter)


class _AnotherLibm(sar.Typed):
    """float64 with numpy's own pow and exp, not libm's through Python floats: the stand-in for a device that computes correctly"""

    def __init__(self, dtype):
        super().__init__(dtype)
        self._f64 = False


def _judge_planted(monkeypatch, cls, form, solver, newton=sar.NEWTON):
    shape = (66, 6, 4) if form == "density" else (66, 8, 12)
    tag = tags(form, shape)
    want = sar.restated(form, shape, 1, F64, solver, newton=newton)
    clear, cloudy = (sar.restated(form, shape, 1, F64, solver, b, newton=newton) for b in ("clear", "cloudy"))
    table = sar.d80(form, shape, 1, solver, newton=newton)
    monkeypatch.setattr(sar, "typed", lambda dtype: cls(dtype))
    case = sar.compressible_case(shape) if form == "density" else sar.anelastic_case(shape)
    dev = (sar.diagnose_compressible(case, 1, F64, solver, newton) if form == "density" else
           sar.diagnose_anelastic(case, 1, case.p_r, case.rho_r, F64, solver))
    return sar.judge64(dev, want, tag, table, clear, cloudy)


@pytest.mark.parametrize("form", ["density", "pressure"])
def test_judging_passes_a_restatement_on_another_libm(monkeypatch, form):
    for solver in (sar.DEFAULT_SOLVER, (0.0, 50)):
        fails, report, skipped = _judge_planted(monkeypatch, _AnotherLibm, form, solver)
        print(f"ANOTHER LIBM {form} {solver}: {report}")
        assert not fails, (solver, fails)


@pytest.mark.parametrize("form,cls,solver", [("density", _NoLiquidHeat, sar.DEFAULT_SOLVER), ("pressure", _NoLiquidHeat, sar.DEFAULT_SOLVER),
                                             ("density", _WiderFloor, sar.DEFAULT_SOLVER), ("pressure", _WiderFloor, sar.DEFAULT_SOLVER),
                                             ("density", _OneIterationMore, (1e-4, 2)), ("density", _OneIterationMore, (1e-4, 0)),
                                             ("density", _NewtonIgnoresAbstol, sar.DEFAULT_SOLVER)],
                         ids=lambda v: getattr(v, "__name__", str(v)))
def test_judging_refuses_a_planted_error(monkeypatch, form, cls, solver):
    fails, report, skipped = _judge_planted(monkeypatch, cls, form, solver, (1.0, 8) if cls is _NewtonIgnoresAbstol else sar.NEWTON)
    print(f"PLANTED {cls.__name__} {form} {solver}: {fails}")
    assert fails


def _float32_case(cls, monkeypatch):
    case = sar.compressible_case((66, 6, 4))
    arrays = {n: case[n].astype(F32) for n in ("rho_d", "rtheta", "rq")}
    wide = {n: a.astype(F64) for n, a in arrays.items()}
    want32 = sar.diagnose_compressible(arrays, 1, F32)
    want64, clear, cloudy = (sar.diagnose_compressible(wide, 1, F64, force_branch=b) for b in (None, "clear", "cloudy"))
    dev = want32
    if cls is not None:
        monkeypatch.setattr(sar, "typed", lambda dtype: cls(dtype))
        dev = sar.diagnose_compressible(arrays, 1, F32)
    return sar.judge32(dev, want32, want64, case.tag, float(np.abs(want64.q).max()), clear, cloudy)


def test_float32_judging_passes_the_float32_restatement_and_refuses_planted_errors(monkeypatch):
    fails, report, table = _float32_case(None, monkeypatch)
    assert not fails and set(table) >= {"bulk", "marginal", "marginal_edge", "guess_switch"}
    assert all(row[0] > 0 for name, row in table.items())      # every population has a d32 of its own
    for cls in (_NoLiquidHeat, _WiderFloor):
        fails, report, table = _float32_case(cls, monkeypatch)
        print(f"PLANTED float32 {cls.__name__}: {fails}")
        assert fails
