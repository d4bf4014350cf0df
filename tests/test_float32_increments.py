"""Float32 lean seam at the shapes where its launches branch (csrc/bz_tendency5.hip: lean_launch, pick_chunk5 on the Float32 twin's coarse
rule, TY = 8): partial x tiles, a partial last tile row, fewer than three tile rows, XCD block order on / off / switched off, several z
chunks, a stretched z grid, walls in y (the WY instantiations), the lean forcing epilogues, and each Poisson path (hand-written x
transforms, kx-major chunked, rocFFT).  One step and three steps against the Float64 oracle, judged by the increment of each field
(tests/helpers.py: increment_error, F32_INCREMENT_TOL), lean and BZ_NO_LEAN=1 alike; the set-ups are tests/f32_cases.py's."""
import numpy as np
import pytest

import f32_cases as fc
from helpers import assert_increments

SWEEP = list(fc.SWEEP_CASES.values())


@pytest.mark.gpu
@pytest.mark.parametrize("lean", [True, False], ids=["lean", "nolean"])
@pytest.mark.parametrize("case", SWEEP, ids=[c.name for c in SWEEP])
def test_float32_lean_sweep_matches_the_float64_oracle_by_increments(oracle, oc, bz, case, lean, monkeypatch):
    import torch
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    if not lean:
        monkeypatch.setenv("BZ_NO_LEAN", "1")
    om, hm = case.build(oracle, oc, bz)
    assert hm.momentum["ρu"].parent.dtype == torch.float32
    start = fc.oracle_fields(om, case.fields)
    hm.profile_enable(True)
    for s in range(1, case.steps + 1):
        om.time_step(case.dt)
        hm.time_step(case.dt)
        if s in (1, case.steps):
            hm.synchronize()
            assert_increments(f"sweep {case.name} {'lean' if lean else 'nolean'} step {s}", fc.device_fields(hm, case.fields),
                              fc.oracle_fields(om, case.fields), start, case.kind)
    names = set(hm.profile())
    assert ("scalar_tendencies+rk3+thermo" in names) == lean, names          # the lean kernels ran / did not run
