"""CPU: the Float32 increment tolerances (tests/helpers.py: F32_INCREMENT_TOL) stay tight enough to see a wrong kernel.  For every set-up
the Float32 GPU tests run (tests/f32_cases.py), the Float64 oracle runs twice — as it is, and with a known defect — and the defect's
increment error must be at least three times the tolerance of every field it governs.  Defects: every step 1 % too long; the
neighbouring WENO order (WENO7 for WENO5); five acoustic substeps for six.  A tolerance loosened past what sees these defects fails here."""
import numpy as np
import pytest

import f32_cases as fc
from helpers import F32_INCREMENT_TOL, increment_error

DEFECTS = {"dt": {"dt": 1.01}, "weno": {"weno": True}, "substeps": {"substeps": 5}}
MARGIN = 3.0
# (case, field) pairs whose increment is dominated by something a 1 % longer step does not change, so that another defect governs them:
# the anelastic Kessler case's rho q^v moves mostly by the first step's evaporation of the cloud water (WENO7 for WENO5 separates it)
DT_EXEMPT = {("kessler", "rq")}


def _unique(cases):
    seen, out = set(), []
    for c in cases:
        if c.key not in seen:
            seen.add(c.key)
            out.append(c)
    return out


CASES = _unique(list(fc.STEP_CASES.values()) + list(fc.SWEEP_CASES.values()) + list(fc.SUBSTEP_CASES.values()))


def _checkpoints(case):
    # the sweep compares after the first step as well
    return (1, case.steps) if case.name in fc.SWEEP_CASES or case.key in {c.key for c in fc.SWEEP_CASES.values()} else (case.steps,)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_float32_tolerances_see_a_known_defect(oracle, oc, case):
    at = _checkpoints(case)
    start, ref = fc.run_oracle(case, oracle, oc, at=at)
    tol = F32_INCREMENT_TOL[case.kind]
    report = {}
    for dname in case.defects:
        _, bad = fc.run_oracle(case, oracle, oc, DEFECTS[dname], at=at)
        for s in at:
            for n in case.fields:
                e = increment_error(bad[s][n], ref[s][n], start[n])
                report[(dname, s, n)] = e / tol[n]
    print(f"{case.name}: defect / tolerance", {f"{d}@{s}:{n}": f"{r:.1f}" for (d, s, n), r in report.items()})
    # every field the case compares is governed by at least one defect with a margin of three
    for n in case.fields:
        best = max(r for (d, s, m), r in report.items() if m == n)
        assert best >= MARGIN, (case.name, n, {k: v for k, v in report.items() if k[2] == n})
    # and the step-length defect by itself is seen in every field at every checkpoint
    for s in at:
        for n in case.fields:
            if (case.name, n) in DT_EXEMPT:
                continue
            assert report[("dt", s, n)] >= MARGIN, (case.name, "dt", s, n, report[("dt", s, n)])


def test_increment_error_refuses_a_field_the_reference_did_not_move():
    a = np.full((2, 3), 300.0)
    with pytest.raises(ValueError):
        increment_error(a, a, a)
    with pytest.raises(ValueError):
        increment_error(a, a + 1e-12, a)
    assert increment_error(a + 1.001, a + 1.0, a) == pytest.approx(1e-3)


def test_tolerance_tables_cover_every_compared_field():
    for c in list(fc.STEP_CASES.values()) + list(fc.SWEEP_CASES.values()) + list(fc.SUBSTEP_CASES.values()):
        for n in c.fields:
            assert n in F32_INCREMENT_TOL[c.kind], (c.name, n)


def test_sweep_reaches_the_lean_launch_branches():
    """The sweep's shapes take each branch of lean_launch / pick_chunk5 in the Float32 twin (TY = 8, coarse chunk rule)."""
    shapes = {c.name: c for c in fc.SWEEP_CASES.values()}
    sizes = {"nx32_ny20": (32, 20, 16), "nx72_ny12_moist": (72, 12, 12), "nx130_ny16": (130, 16, 12), "nx64_ny24_moist": (64, 24, 16),
             "nx64_ny16_kxchunk": (64, 16, 32)}
    assert set(sizes) <= set(shapes)
    nx = [s[0] for s in sizes.values()]
    assert any(n < 64 for n in nx) and any(n % 64 for n in nx if n > 64) and any(n % 64 == 0 for n in nx)
    assert any(s[1] % 8 for s in sizes.values()) and any((s[1] + 7) // 8 < 3 for s in sizes.values())
    xcd = {fc.lean_xcd(s[0], s[1], s[2]) for s in sizes.values()}
    assert xcd == {True, False}
    assert all(fc.lean_chunks(s[0], s[1], s[2])[1] > 1 for s in sizes.values())
    assert not fc.lean_xcd(130, 16, 12) and "BZ_NO_XCD" in shapes["nx130_ny16_noxcd"].env
    assert "BZ_POISSON_KX_CHUNK_KB" in shapes["nx64_ny16_kxchunk"].env
