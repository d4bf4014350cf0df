"""The generation-4 LDS tiles (csrc/bz_tendency4_kernels.h: k_u_tend_lds, k_v_tend_lds, k_w_tend_lds, k_scalar_pair_lds) on a periodic grid.
They are the only fallback of the stored-velocity kernels and by default run between x walls only (tests/test_bounded_x.py);
BZ_NO_K6_STORED=1 selects them everywhere.  72 x 12 x 10 with halo 3: a partial x tile (64 + 8 columns), a partial row of 8-row tiles
(8 + 4 rows) and one z chunk."""
import numpy as np
import pytest

from helpers import PROG, bubble_theta, push_state, randomize, relerr

pytestmark = pytest.mark.gpu

SIZE = (72, 12, 10)
EXTENT = ((-10e3, 10e3), (-10e3, 10e3), (0.0, 10e3))


def _pair(oracle, bz, moist):
    og = oracle.Grid(SIZE, x=EXTENT[0], y=EXTENT[1], z=EXTENT[2], halo=(3, 3, 3))
    om = oracle.OracleModel(og, potential_temperature=300.0, **(dict(microphysics="SaturationAdjustment") if moist else {}))
    grid = bz.RectilinearGrid(SIZE, x=EXTENT[0], y=EXTENT[1], z=EXTENT[2], halo=(3, 3, 3))
    kw = dict(microphysics=bz.SaturationAdjustment(equilibrium=bz.WarmPhaseEquilibrium())) if moist else {}
    hm = bz.AtmosphereModel(grid, dynamics=bz.AnelasticDynamics(bz.ReferenceState(grid, potential_temperature=300.0)),
                            advection=bz.WENO(order=5), **kw)
    return om, hm


@pytest.mark.parametrize("moist", [False, True], ids=["dry", "saturation_adjustment"])
def test_tile_tendencies_match_oracle(oracle, bz, moist, monkeypatch):
    """bz_compute_tendencies through the tiles, field by field, at the tolerance of tests/test_gpu_parity.py's tendency test (1e-12 of
    the tendency scale): dry (k_w_tend_lds<8, 0>) and with saturation adjustment (k_w_tend_lds<8, 3>: buoyancy from q^v, q^l)."""
    monkeypatch.setenv("BZ_NO_K6_STORED", "1")
    om, hm = _pair(oracle, bz, moist)
    randomize(om, seed=11)
    om.compute_tendencies()
    push_state(om, hm, names=("ru", "rv", "rw", "rtheta", "rq"))
    for k in hm.G.values():
        k.parent.zero_()
    bz.update_state_(hm, compute_tendencies=True)
    hm.synchronize()
    g = om.grid
    errs = {}
    for n, k in PROG.items():
        zf = n == "rw"
        want, got = g.interior(om.G[n], zface=zf), hm.G[k].interior_cpu()
        if zf:      # wall faces are never updated
            want, got = want[1:-1], got[1:-1]
        errs[n] = relerr(got, want)
    print("GEN4 tendencies", "moist" if moist else "dry", " ".join(f"{n}={e:.2e}" for n, e in errs.items()))
    assert all(e < 1e-12 for e in errs.values()), errs


def test_tiles_under_the_fused_rk_epilogue(oracle, bz, monkeypatch):
    """BZ_NO_LEAN=1 BZ_NO_K6_STORED=1: the fused-RK tier with the RK update in the tiles' store.  Three steps against the oracle (1e-9, as
    the three-step test of tests/test_gpu_parity.py) and bit for bit against one bz_time_steps_anelastic(n = 3) call (as
    tests/test_multi_step.py requires of the default tier; whole parent arrays)."""
    monkeypatch.setenv("BZ_NO_LEAN", "1")
    monkeypatch.setenv("BZ_NO_K6_STORED", "1")
    th = bubble_theta(300.0, 9.81)
    om, a = _pair(oracle, bz, False)
    _, b = _pair(oracle, bz, False)
    om.set(theta=th, u=3.0, v=-2.0)
    a.profile_enable()
    for m in (a, b):
        m.set(θ=th, u=3.0, v=-2.0)
    for _ in range(3):
        om.time_step(2.0)
        a.time_step(2.0)
    b.time_steps(2.0, 3, diagnose_last=True)
    a.synchronize(); b.synchronize()
    assert "x_momentum_tendency+rk3" in a.profile() and "scalar_tendencies+rk3" in a.profile()      # the fused-RK tier, not the lean seam
    g = om.grid
    errs = {}
    for n, k in PROG.items():
        got, want = a.prognostic_fields()[k].interior_cpu(), g.interior(getattr(om, n), zface=(n == "rw"))
        errs[n] = np.max(np.abs(got - want)) / max(np.max(np.abs(want)), 1e-3)
    errs["T"] = relerr(a.temperature.interior_cpu(), g.interior(om.T))
    print("GEN4 fused-RK steps", " ".join(f"{n}={e:.2e}" for n, e in errs.items()))
    assert all(e < 1e-9 for e in errs.values()), errs
    fields = lambda m: dict(m.prognostic_fields(), u=m.velocities["u"], v=m.velocities["v"], w=m.velocities["w"], θ=m.potential_temperature,
                            q=m.specific_moisture, T=m.temperature, ϕ=m.dynamics.pressure_anomaly)
    fa, fb = fields(a), fields(b)
    for k in fa:
        assert np.array_equal(fa[k].cpu(), fb[k].cpu()), k
