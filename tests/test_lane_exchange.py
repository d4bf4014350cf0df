"""The x-face exchange of the tile tendency kernels (csrc/bz_internal.h: bz_lane_up / bz_lane_down / bz_lane_read — DPP moves and
v_readlane where __shfl_up / __shfl_down / __shfl were) at the row shapes where it can go wrong: a row of exactly one wavefront whose edge
flux wraps into the own tile, two tiles, and a ragged second tile whose last active lane is 31 or 7 (the lanes above it receive values
nobody may store, lane 63 a zero).  Mean wind in both directions, so that both upwind sides of the edge flux and of the lane next to it
occur; dry and with vapour (the general scalar-pair body exchanges two fields); Float64 and the Float32 twin (one DPP move per value).

A lean-tier model and a BZ_NO_LEAN=1 model (stored-velocity instantiations of the same kernels inside the fused-RK tier, other
projection and diagnosis kernels) step three times from the same pushed oracle state.  Float64: the five prognostic fields agree to
1e-13 of the field scale, the tolerance of tests/test_gpu_parity.py::test_lean_seam_matches_the_diagnostic_seam in the default build.
Float32: by increments (tests/helpers.py: F32_INCREMENT_TOL["anelastic"]), the second run being the reference; the moisture density of a
dry model is an exact zero in both.  Every case asserts from the profile that the four lean kernel groups ran in the first model and
not in the second.

Both device runs exchange their x fluxes the same way, so the lean run is also held against the CPU oracle stepped from the same state
(computed once per initial state): 1e-7 of the field scale in Float64 (reasoned where it is asserted: above the FMA-contraction
noise of WENO fluxes, below what one wrong x flux does), and the same increments rule in Float32 (the bound tests/test_float32.py holds
Float32 steps to).  The initial state carries waves along x in theta, q, u and v, so that neighbouring lanes hold different fluxes
everywhere — also at the tile edges and the periodic seam, which the bubble does not reach."""
import numpy as np
import pytest

import f32_cases as fc
from helpers import PROG, assert_increments, bubble_theta, push_state, relerr

EXT = ((-10e3, 10e3), (-10e3, 10e3), (0.0, 10e3))
LEAN_GROUPS = ("x_momentum_tendency+rk3+velocity", "y_momentum_tendency+rk3+velocity", "z_momentum_tendency+rk3+velocity",
               "scalar_tendencies+rk3+thermo")
# Nx: 64 one wavefront per row; 128 two tiles; 96 ragged second tile, last active lane 31; 72 the same with lane 7
SHAPES = [(64, 16, 16), (128, 16, 16), (96, 16, 16), (72, 16, 16)]
WINDS = [(3.0, -2.0), (-3.0, 2.0)]
STEPS, DT = 3, 1.5

_ORACLE_STATE = {}      # (size, wind, moist) -> (oracle model holding the initial state: set once, never stepped; the oracle's fields after STEPS steps)


LX, LY = EXT[0][1] - EXT[0][0], EXT[1][1] - EXT[1][0]
KX, KY = 2 * np.pi * 2 / LX, 2 * np.pi / LY


def _oracle_model(oracle, size, wind, moist):
    """The bubble under a mean wind, plus waves along x in every advected quantity (theta 1 K, q 20 %, a non-divergent 0.5 m/s wave in
    u, v): under a uniform wind alone every lane away from the bubble holds the same x flux, and a value taken from the wrong lane — at
    the periodic seam, at a tile edge, in the last lane of a ragged row — would be the right value."""
    og = oracle.Grid(size, x=EXT[0], y=EXT[1], z=EXT[2])
    om = oracle.OracleModel(og, potential_temperature=300.0)
    bub = bubble_theta(300.0, 9.81)
    ic = dict(theta=lambda x, y, z: bub(x, y, z) + 1.0 * np.sin(1.5 * KX * x + 0.4) * np.cos(KY * y) + 0 * z,
              u=lambda x, y, z: wind[0] + 0.5 * np.sin(KX * x + 0.7) * np.cos(KY * y) + 0 * z,
              v=lambda x, y, z: wind[1] - 0.5 * (KX / KY) * np.cos(KX * x + 0.7) * np.sin(KY * y) + 0 * z)
    if moist:
        ic["qt"] = lambda x, y, z: fc.moist_q(x, y, z) * (1.0 + 0.2 * np.sin(KX * x + 1.0))
    om.set(**ic)
    return om


def _initial_state(oracle, size, wind, moist):
    key = (size, wind, moist)
    if key not in _ORACLE_STATE:
        stepped = _oracle_model(oracle, size, wind, moist)
        for _ in range(STEPS):
            stepped.time_step(DT)
        _ORACLE_STATE[key] = (_oracle_model(oracle, size, wind, moist), fc.oracle_fields(stepped, tuple(PROG)))
    return _ORACLE_STATE[key]


def _device_model(bz, size, float_type):
    grid = bz.RectilinearGrid(size, x=EXT[0], y=EXT[1], z=EXT[2], float_type=float_type)
    return bz.AtmosphereModel(grid, dynamics=bz.AnelasticDynamics(bz.ReferenceState(grid, potential_temperature=300.0)),
                              advection=bz.WENO(order=5))


@pytest.mark.gpu
@pytest.mark.parametrize("float_type", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("moist", [False, True], ids=["dry", "moist"])
@pytest.mark.parametrize("wind", WINDS, ids=["u+3v-2", "u-3v+2"])
@pytest.mark.parametrize("size", SHAPES, ids=["%dx%dx%d" % s for s in SHAPES])
def test_lean_and_stored_velocity_steps_agree_across_the_x_face_exchange(oracle, bz, size, wind, moist, float_type, monkeypatch):
    import torch
    om, oracle_end = _initial_state(oracle, size, wind, moist)
    names = tuple(PROG)
    start = fc.oracle_fields(om, names)
    runs = []
    for lean in (True, False):
        if lean:
            monkeypatch.delenv("BZ_NO_LEAN", raising=False)
        else:
            monkeypatch.setenv("BZ_NO_LEAN", "1")      # read when the context is created
        hm = _device_model(bz, size, float_type)
        assert hm.momentum["ρu"].parent.dtype == (torch.float64 if float_type is np.float64 else torch.float32)
        push_state(om, hm)
        hm.profile_enable(True)
        for _ in range(STEPS):
            hm.time_step(DT)
        hm.synchronize()
        groups = set(hm.profile())
        if lean:
            assert all(g in groups for g in LEAN_GROUPS), groups          # the lean tier ran: every one of its four kernel groups
        else:
            assert not any(g in groups for g in LEAN_GROUPS), groups
        runs.append(fc.device_fields(hm, names))
    a, b = runs
    label = "lane exchange %dx%dx%d u=%+g %s %s" % (size + (wind[0], "moist" if moist else "dry", np.dtype(float_type).name))
    for n in names:      # both runs moved every field they are compared on (a step that does nothing agrees with itself)
        if n != "rq" or moist:
            assert np.max(np.abs(b[n] - start[n])) > 0.0, n
    if float_type is np.float64:
        errs = {n: relerr(a[n], b[n]) for n in names}
        print(label, " ".join("%s=%.2e" % kv for kv in errs.items()))
        assert all(e < 1e-13 for e in errs.values()), errs
        # The two device runs share the exchange, the CPU oracle does not.  Bound 1e-7 of the field scale, between two things: the
        # contraction of products into FMAs moves a WENO flux of structured data by ~1e-9 against the oracle's uncontracted arithmetic
        # (nine tendency evaluations in three steps: <= 1e-8), and an x flux taken from the neighbouring lane's
        # neighbour or lost is dt u (change of the field per cell) / dx per stage: with the waves of the initial state >= 1e-5 of
        # rho theta (0.3 K per cell at most, 1.5 s, 3 m/s, 312 m against 300 K) and more of the momenta.
        oerrs = {n: np.max(np.abs(a[n] - oracle_end[n])) / max(np.max(np.abs(oracle_end[n])), 1e-3) for n in names}
        print(label, "against the oracle", " ".join("%s=%.2e" % kv for kv in oerrs.items()))
        assert all(e < 1e-7 for e in oerrs.values()), oerrs
    else:
        judged = [n for n in names if n != "rq" or moist]
        assert_increments(label, {n: a[n] for n in judged}, {n: b[n] for n in judged}, start, "anelastic")
        assert_increments(label + " against the oracle", {n: a[n] for n in judged}, {n: oracle_end[n] for n in judged}, start, "anelastic")
        if not moist:
            assert not a["rq"].any() and not b["rq"].any()
