"""The acoustic substep kernels on ragged rows and thin columns, against the CPU oracle.

The compressible oracle tests above this file (test_gpu_compressible.py, test_gpu_large_columns.py, test_weno_orders.py, test_float32.py,
test_compressible_closure.py, test_graph_replay.py) stop at Nx <= 128 on whole tiles (32, 64, 128) or single-wave rows (24, 40) and at
Nz >= 5: no row there ends in a partly filled wavefront behind a full one, none crosses a 256-thread block, none sits on either side of
the launcher's Nx % 64 == 1 fallback, and no column is short enough for the ring clamps and the tail of the two-level pipeline of
k_ac_forward2 (csrc/bz_acoustic_kernels.h) to be most of the march.  A wrong neighbour at a wave seam is a one-column error, which the
whole-tile shapes cannot show.  The shapes here (halo 3 everywhere) and the seam each of them meets:

  (6, 6, 3)      the smallest grid the compressible context accepts (Nx >= 2 Hx, Ny >= 2 Hy); a march of three levels: level 0, one
                 interior level and the top — the ring clamps k + 1 < Nz, k + 2 < Nz act on every level, the two-level pipeline's trip ends odd
  (66, 6, 4)     one full wave plus 2 lanes: lane 63 of the first wave and lane 1 of the second are both right edges of k_ac_forward2 (the
                 edge lanes load the outer neighbour, the others take it by DPP wave shift); Ny < 8: ragged block rows
  (65, 7, 4)     Nx % 64 == 1 — a row's first lane would be its last: ac_forward2_ok (csrc/bz_acoustic.hip) sends the grid to
                 k_ac_column_forward; a ragged row of that kernel, odd Ny
  (130, 9, 6)    two full waves plus 2 lanes; Ny = 9 leaves one row in the second block row of a 128 x 4 block (and of the 64 x 4 / 64 x 8 ones)
  (129, 6, 5)    the fallback again, two full waves in front of the single cell
  (190, 12, 9)   the last wave nearly full (62 lanes); odd Nz: the pipeline's last trip works one level
  (258, 6, 4)    the row crosses a 256-thread block by 2 cells (k_ac_stage_init, k_ac_stage_end, k_ac_column_backward, k_ac_finalize); Nx + 2 Hx = 264
                 for k_cmp_diagnose, which tiles over the halo columns as well
  (320, 8, 5)    whole tiles, but more than one 256-thread block and five tile columns

Nz = 3 is accepted by the host model and by the oracle, so (6, 6, 3) runs as listed.

The GPU tests are Float64 unless they say otherwise; tolerances are those of the tests whose bodies they repeat.  Step lengths are theirs
too wherever the acoustic substeps are stable on these finer cells (down to 25 m where those tests have 125 - 333 m); where they are not,
the step shrinks with the cell and the tolerance stays: loop_dt, WHOLE_STEPS and the Float32 twin test say where and why.  A failure names the
(k, j, i) of the worst cell and i % 64, so that a seam error reads as one.  The CPU test at the end shows that a seam error would be
seen: one column's (rho theta) off by 1e-6 moves the column across the periodic seam, and the one across the wave seam, by far more than
100 x the tolerance of the loop test."""
import numpy as np
import pytest

SHAPES = [(6, 6, 3), (66, 6, 4), (65, 7, 4), (130, 9, 6), (129, 6, 5), (190, 12, 9), (258, 6, 4), (320, 8, 5)]
FALLBACK_SHAPES = [(65, 7, 4), (129, 6, 5)]
MOIST_SHAPES = [(66, 6, 4), (130, 9, 6)]
LOOP_TD = [dict(substeps=6),                                                            # first-substep and plain instantiations, folded p^L in the last stage
           dict(substeps=4, damping_coefficient=0.05, damp_vertical=True),              # damped, implicit vertical damping
           dict(substeps=6, damping_coefficient=None, sponge=(0.2, 3000.0, "cubic"))]   # undamped with the sponge rows
LOOP_TOL, STATE_TOL, STEP_TOL = 2e-11, 1e-12, 5e-9
STEP_FIELDS = ("rho_d", "rtheta", "ru", "rv", "rw", "u", "v", "w", "theta", "T", "p")
AVERAGES = (("au", "time_averaged_u"), ("av", "time_averaged_v"), ("aw", "time_averaged_w"))


def _tg():
    import test_gpu_compressible as tg
    return tg


def _id(v):
    if isinstance(v, tuple):
        return "x".join(str(n) for n in v)
    if isinstance(v, dict):
        return "-".join(f"{k}={'+'.join(map(str, x)) if isinstance(x, tuple) else x}" for k, x in v.items())
    return None


def where(a, b):
    """the worst cell of a - b, as the failure messages print it"""
    d = np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64))
    k, j, i = (int(n) for n in np.unravel_index(int(np.argmax(d)), d.shape))
    return f"worst cell (k, j, i) = ({k}, {j}, {i}), i % 64 = {i % 64}, |diff| = {d[k, j, i]:.3e}"


def cmp_located(om, hm, names, tol, zface_names=("rw", "w")):
    """cmp_interior of test_gpu_compressible.py; a failure also names the worst cell of every field beyond the tolerance"""
    tg = _tg()
    try:
        return tg.cmp_interior(om, hm, names, tol, zface_names)
    except AssertionError as err:
        g, lines = om.grid, []
        for n in names:
            a, b = tg.O2H[n](hm).interior_cpu(), g.interior(getattr(om, n), n in zface_names)
            if np.abs(a - b).max() > 0:
                lines.append(f"  {n}: {where(a, b)}")
        raise AssertionError(f"{err}\n" + "\n".join(lines)) from None


def loop_state(om, perturb_column=None):
    """the state test_acoustic_substep_loop_matches_oracle hands to the loop: seeded rough fields, U0 stored, the stage state moved off U0
    the way an earlier stage would, diagnostics, linearisation and slow tendencies of that state.  perturb_column: after all that, the
    interior rho theta of this one column times 1 + 1e-6 (what a kernel that read a wrong neighbour there would have seen)."""
    tg = _tg()
    tg.seeded_state(om, 4)
    for n in om.PROGNOSTIC:
        om.U0[n][...] = getattr(om, n)
    g = om.grid
    rng = np.random.default_rng(5)
    for n in ("rho_d", "rtheta", "ru", "rv"):
        g.interior(getattr(om, n))[...] *= 1 + 1e-3 * rng.standard_normal((g.Nz, g.Ny, g.Nx))
    g.interior(om.rw, True)[1:-1] *= 1 + 1e-3 * rng.standard_normal((g.Nz - 1, g.Ny, g.Nx))
    om.update_state(compute_tendencies=True)
    om.refresh_linearization()
    om.compute_slow_tendencies()
    if perturb_column is not None:
        g.interior(om.rtheta)[:, :, perturb_column] *= 1 + 1e-6


def loop_dt(size):
    """The loop test's dt = 2 s belongs to its 333 m cells: a stage of six substeps advances by 115 m of sound per substep, a third of a
    cell.  On the 61 m cells of the 130-cell row that is 1.9 cells (5 on the 320-cell row), the explicit horizontal step amplifies the seeded
    state by up to 1e10 in one loop, the recovered dry density changes sign and u = rho u / rho at a face is no longer a function two
    roundings-apart runs agree on (measured on the MI355X with dt = 2: every recovered prognostic field within 1e-15 of the oracle, every
    substepper field within its 2e-11, u up to 3e-10 of its maximum off).  So dt shrinks with the finest horizontal spacing, at the acoustic Courant number of the loop test,
    and stays 2 s on the cells that are as coarse as that test's or coarser ((6, 6, 3))."""
    ext = _tg().EXTENT
    d = min((ext["x"][1] - ext["x"][0]) / size[0], (ext["y"][1] - ext["y"][0]) / size[1])
    return min(2.0, 2.0 * d / ((ext["x"][1] - ext["x"][0]) / 24))


def loop_scale(om, n):
    """the scale the loop test divides the error of substepper field `n` by, from the oracle's fields after the loop"""
    g = om.grid
    if n == "rp":
        return np.abs(g.interior(om.rho_d)).max() * 1e-3
    if n == "rthp":
        return np.abs(g.interior(om.rtheta)).max() * 1e-3
    return max(np.abs(g.interior(getattr(om, n), n in ("rwp", "aw", "Gs"))).max(), 1e-300)


def bubble(x, y, z):
    r = np.sqrt(x ** 2 + (y - 300.0) ** 2 + (z - 3000.0) ** 2)
    return 300.0 + 2.0 * np.maximum(0.0, 1.0 - r / 2000.0)


def _blob(x, y, z):
    return np.maximum(0.0, 1.0 - np.sqrt(x ** 2 + (y - 300.0) ** 2 + (z - 3000.0) ** 2) / 2000.0)


def moist_qv(x, y, z):
    return 0.014 * np.exp(-z / 3000.0) + 0.004 * _blob(x, y, z)


U3 = lambda x, y, z: 3.0 + 0 * x + 0 * y + 0 * z        # noqa: E731
V2 = lambda x, y, z: -2.0 + 0 * x + 0 * y + 0 * z       # noqa: E731


def set_bubble(om, hm, qv=None, species=False, oracle_too=True):
    """the bubble, u = 3, v = -2 of test_forward_sweep_round6_kernel [+ vapour [+ cloud water and rain inside the bubble]]"""
    g = om.grid
    rho = om.ref.density[g.Hz:g.Hz + g.Nz][:, None, None]
    okw, hkw = {}, {}
    if qv is not None:
        okw["qv"], hkw["qᵗ"] = qv, qv
    if species:
        qcl = lambda x, y, z: 0.003 * _blob(x, y, z)      # noqa: E731
        qr = lambda x, y, z: 0.001 * _blob(x, y, z)       # noqa: E731
        okw.update(qcl=qcl, qr=qr)
        hkw.update(qcl=qcl, qr=qr)
    if oracle_too:
        om.set(rho=rho, theta=bubble, u=U3, v=V2, w=0.0, **okw)
    hm.set(ρ=rho, θ=bubble, u=U3, v=V2, w=0.0, **hkw)


# Whole steps: (shape, dt, tolerance).  dt = 0.5 s and 5e-9 are those of test_forward_sweep_round6_kernel.  Every stage of a six-substep step
# advances by dt / 12 per substep, and the forward-backward horizontal step is stable for an acoustic Courant number c_s dt / (12 dx) below
# one (c_s = 347 m/s), less what the divergence damping takes:
#   * up to the 190-cell row (42 m cells, 0.69) the oracle's 2 dx mode of rho u does not grow: dt = 0.5 s, 5e-9;
#   * on the 320-cell row (25 m, 1.16) the CPU oracle itself is non-finite in its second step of 0.5 s — there is nothing to compare with:
#     dt = 0.25 s (0.58), 5e-9;
#   * on the 258-cell row (31 m, 0.93) the oracle's 2 dx mode grows 25 x per step of 0.5 s, and so does every rounding difference: measured
#     against the oracle on the MI355X, rho u and u 3.3e-8 of max-abs with the default library and 1.4e-8 with the -ffp-contract=off one
#     (lib/libbreeze_hip_refdiv.so) — two roundings of the same arithmetic, the same order off, every other field below 1e-9 — so the step of
#     0.5 s is kept with the bound 1.3e-7 (4 x the larger figure, the convention of tests/helpers.py), and the stable step of 0.25 s
#     (measured 2.8e-10 / 7.5e-11) runs at 5e-9 beside it.
WHOLE_STEPS = [(s, 0.5, STEP_TOL) for s in SHAPES if s[0] <= 190] + [((258, 6, 4), 0.5, 1.3e-7), ((258, 6, 4), 0.25, STEP_TOL),
                                                                      ((320, 8, 5), 0.25, STEP_TOL)]


def kessler_pair(oracle, oc, bz, size):
    """the pair of test_compressible_kessler_model_matches_oracle on this file's domain"""
    ext = _tg().EXTENT
    og = oracle.Grid(size, **ext)
    om = oc.CompressibleOracleModel(og, time_discretization=oc.SplitExplicit(substeps=6), surface_pressure=1e5,
                                    reference_potential_temperature=300.0, microphysics="Kessler")
    grid = bz.RectilinearGrid(size, **ext)
    tc = bz.ThermodynamicConstants(saturation_vapor_pressure=bz.TetensFormula())
    dyn = bz.CompressibleDynamics(bz.SplitExplicitTimeDiscretization(substeps=6), surface_pressure=1e5, reference_potential_temperature=300.0)
    hm = bz.CompressibleAtmosphereModel(grid, dyn, advection=bz.WENO(order=5), thermodynamic_constants=tc,
                                        microphysics=bz.DCMIP2016KesslerMicrophysics())
    return om, hm


def check_steps(om, hm, names, tol=STEP_TOL):
    worst = cmp_located(om, hm, names, tol)
    g, sub = om.grid, hm.timestepper.substepper
    scale = max(np.abs(g.interior(getattr(om, n), n == "aw")).max() for n, _ in AVERAGES)
    for n, k in AVERAGES:
        a, b = getattr(sub, k).interior_cpu(), g.interior(getattr(om, n), n == "aw")
        worst[n] = np.abs(a - b).max() / scale
        assert worst[n] <= tol, (n, worst[n], where(a, b))
    return worst


# ---- 1. the acoustic loop at every shape ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("beta", [1.0 / 3.0, 1.0], ids=["beta=1/3", "beta=1"])
@pytest.mark.parametrize("td", LOOP_TD, ids=_id)
@pytest.mark.parametrize("size", SHAPES, ids=_id)
def test_acoustic_loop_on_ragged_rows_matches_oracle(oracle, oc, bz, size, td, beta):
    """The body of test_acoustic_substep_loop_matches_oracle at every shape: perturbations, time-averaged velocities (2e-11), recovered state
    and velocities (1e-12) after acoustic_rk3_substep_loop! from a stage state off U0, dt at that test's acoustic Courant number (loop_dt).  beta = 1/3 runs stages of two substeps (one pair,
    the first-substep instantiation and one more, p^L in the substep), beta = 1 of six / four (the folded p^L, pairs with and without an
    odd substep out); the three time discretisations are the plain, the damped and the undamped-with-sponge instantiations."""
    tg = _tg()
    om, hm = tg.make_pair(oracle, oc, bz, size=size, **td)
    loop_state(om)
    tg.push(om, hm)
    bz.compressible.refresh_linearization_(hm)     # fills the context's gamma R Pi scratch
    dt = loop_dt(size)
    om.acoustic_substep_loop(dt, beta)
    bz.compressible.acoustic_rk3_substep_loop_(hm, dt, beta)
    n_tau, _ = hm.stage_substeps(dt, beta)
    assert n_tau == om.last_substeps[-1]
    g, sub = om.grid, hm.timestepper.substepper
    errs, bad = {}, []
    for n, k in tg.SUB.items():
        if n in ("Pi", "thL", "gR"):
            continue
        a, b = getattr(sub, k).interior_cpu(), g.interior(getattr(om, n), n in ("rwp", "aw", "Gs"))
        errs[n] = np.abs(a - b).max() / loop_scale(om, n)
        if not errs[n] <= LOOP_TOL:
            bad.append(f"  {n}: {errs[n]:.3e}, {where(a, b)}")
    print("LOOP", size, td, f"beta={beta:.3f}", " ".join(f"{n}={e:.1e}" for n, e in errs.items()))
    assert not bad, f"substepper fields beyond {LOOP_TOL} after {n_tau} substeps:\n" + "\n".join(bad)
    worst = cmp_located(om, hm, ("rho_d", "rtheta", "ru", "rv", "rw", "u", "v", "w"), STATE_TOL)
    print("LOOP state", size, " ".join(f"{n}={e:.1e}" for n, e in worst.items()))


# ---- 2. three whole steps at every shape ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("size,dt,tol", WHOLE_STEPS, ids=["%dx%dx%d-dt=%g" % (s + (dt,)) for s, dt, _ in WHOLE_STEPS])
def test_three_steps_on_ragged_rows_match_oracle(oracle, oc, bz, size, dt, tol):
    """Three WS-RK3 steps (six substeps; dt and tolerance: WHOLE_STEPS) of the bubble of test_forward_sweep_round6_kernel in the shipped
    configuration: stage init, first / plain / folded forward sweeps, backward sweeps, the stage epilogue with update_state! and the next
    linearisation, buffer rotation — 5e-9 of max-abs on the state, the diagnostics and the three time-averaged velocities."""
    om, hm = _tg().make_pair(oracle, oc, bz, size=size, substeps=6)
    set_bubble(om, hm)
    for _ in range(3):
        om.time_step(dt)
        hm.time_step(dt)
    hm.synchronize()
    worst = check_steps(om, hm, STEP_FIELDS, tol)
    print("STEPS", size, dt, " ".join(f"{n}={e:.1e}" for n, e in worst.items()))
    assert np.abs(om.grid.interior(om.rw, True)).max() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("kessler", [False, True], ids=["vapour", "kessler"])
@pytest.mark.parametrize("size", MOIST_SHAPES, ids=_id)
def test_three_moist_steps_on_ragged_rows_match_oracle(oracle, oc, bz, size, kessler):
    """The moist bodies of the stage epilogue on the two-lane tails: vapour as a transported density (the moisture tendency reads the
    time-averaged velocities of every stage, nothing is skipped as dry), and DCMIP2016KesslerMicrophysics (condensate-loaded density,
    the species in the epilogue, the column update closing the step).  Same bubble, steps and 5e-9; the Kessler species at the 1e-8 of
    test_compressible_kessler_model_matches_oracle."""
    if kessler:
        om, hm = kessler_pair(oracle, oc, bz, size)
    else:
        om, hm = _tg().make_pair(oracle, oc, bz, size=size, substeps=6)
    set_bubble(om, hm, qv=moist_qv, species=kessler)
    for _ in range(3):
        om.time_step(0.5)
        hm.time_step(0.5)
    hm.synchronize()
    worst = check_steps(om, hm, STEP_FIELDS + ("rq", "q"))
    print("MOIST STEPS", size, "kessler" if kessler else "vapour", " ".join(f"{n}={e:.1e}" for n, e in worst.items()))
    g = om.grid
    assert np.abs(g.interior(om.rq)).max() > 0
    if kessler:
        mu = hm.microphysical_fields
        for n, k in (("rqcl", "ρqᶜˡ"), ("rqr", "ρqʳ")):
            want, got = g.interior(getattr(om, n)), mu[k].interior_cpu()
            assert np.abs(want).max() > 0, n
            assert np.abs(got - want).max() <= 1e-8 * max(np.abs(want).max(), 1e-9), (n, where(got, want))


# ---- 3. the new sweep against the old one -----------------------------------------------------------------------------------------------------
def _sweep_run(oracle, oc, bz, monkeypatch, size, fwd2, pfold=0, bx=128):
    monkeypatch.setenv("BZ_AC_FWD2", str(fwd2))
    if pfold is None:
        monkeypatch.delenv("BZ_AC_PFOLD", raising=False)
    else:
        monkeypatch.setenv("BZ_AC_PFOLD", str(pfold))
    monkeypatch.setenv("BZ_AC_BX", str(bx))
    om, hm = _tg().make_pair(oracle, oc, bz, size=size, substeps=6)
    set_bubble(om, hm, oracle_too=False)
    dt = min(d for s, d, _ in WHOLE_STEPS if s == size)      # the stable step of the shape
    for _ in range(3):
        hm.time_step(dt)
    hm.synchronize()
    out = {k: f.interior_cpu().copy() for k, f in hm.prognostic_fields().items()}
    assert all(np.isfinite(v).all() for v in out.values()) and np.abs(out["ρw"]).max() > 0
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(66, 6, 4), (130, 9, 6), (190, 12, 9), (258, 6, 4)], ids=_id)
def test_forward2_on_ragged_rows_matches_the_column_kernel(oracle, oc, bz, size, monkeypatch):
    """k_ac_forward2 without the p^L fold carries the arithmetic text of k_ac_column_forward: three steps (the shape's stable dt) agree to 1e-13 on every prognostic
    field (BZ_AC_FWD2 = 1 / 0, BZ_AC_PFOLD = 0), and the four row widths a block can have — 128 x 4, 512 x 1, 64 x 8, 256 x 2 (BZ_AC_BX =
    128, 512, 64, 256) — give the same bits: where a row's waves fall in a block, and which of them are ragged, changes nothing."""
    tg = _tg()
    old = _sweep_run(oracle, oc, bz, monkeypatch, size, 0)
    ref = _sweep_run(oracle, oc, bz, monkeypatch, size, 1, 0, 128)
    for k in ref:
        assert tg.rel(ref[k], old[k]) <= 1e-13, (k, tg.rel(ref[k], old[k]), where(ref[k], old[k]))
    for bx in (512, 64, 256):
        b = _sweep_run(oracle, oc, bz, monkeypatch, size, 1, 0, bx)
        for k in ref:
            assert np.array_equal(b[k], ref[k]), (k, bx, where(b[k], ref[k]))


@pytest.mark.gpu
@pytest.mark.parametrize("size", FALLBACK_SHAPES, ids=_id)
def test_rows_of_64n_plus_1_cells_take_the_column_kernel(oracle, oc, bz, size, monkeypatch):
    """Nx % 64 == 1: the launcher's predicate (ac_forward2_ok) must have sent the grid to k_ac_column_forward — with it go the p^L fold, the
    folded initial perturbations and the dry shortcut, which all hang on the new sweep — so asking for the new sweep (the default) and
    switching it off give the same bits."""
    a = _sweep_run(oracle, oc, bz, monkeypatch, size, 1, None)
    b = _sweep_run(oracle, oc, bz, monkeypatch, size, 0, None)
    for k in a:
        assert np.array_equal(a[k], b[k]), (k, where(a[k], b[k]))


# ---- 4. Float32 storage ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("size", [(130, 9, 6), (66, 6, 4)], ids=_id)
def test_float32_substep_storage_on_ragged_rows(oracle, oc, bz, size):
    """substep_floattype = Float32 in the Float64 model (the kernels' ST = float instantiations; DPP shifts of values widened from float),
    judged as test_float32_substep_storage_in_a_float64_model judges it: the increments of three steps against the Float64 oracle with
    the "substep_storage" table of tests/helpers.py.  That test's bubble and vapour; dt = 0.5 s for the 61 m / 121 m cells."""
    import torch
    import f32_cases as fc
    from helpers import assert_increments
    tg = _tg()
    om, hm = tg.make_pair(oracle, oc, bz, size=size, substep_floattype=np.float32, substeps=6)
    _, h64 = tg.make_pair(oracle, oc, bz, size=size, substeps=6)
    sub = hm.timestepper.substepper
    for name, _ in sub.FIELDS:
        assert getattr(sub, name).parent.dtype == (torch.float32 if name in sub.WORKING else torch.float64), name
    fields = fc.SUBSTEP_CASES["substep_storage_0"].fields
    g = om.grid
    rho = om.ref.density[g.Hz:g.Hz + g.Nz][:, None, None]
    om.set(rho=rho, theta=fc.substep_storage_theta, u=U3, v=0.0, w=0.0, qv=fc.substep_storage_qv)
    start = fc.oracle_fields(om, fields)
    for m in (hm, h64):
        m.set(ρ=rho, θ=fc.substep_storage_theta, u=U3, v=0.0, w=0.0, qᵗ=fc.substep_storage_qv)
    for _ in range(3):
        om.time_step(0.5)
        hm.time_step(0.5)
        h64.time_step(0.5)
    got, want = fc.device_fields(hm, fields, compressible=True), fc.oracle_fields(om, fields)
    try:
        assert_increments("ragged_%dx%dx%d" % size, got, want, start, "substep_storage")
    except AssertionError as err:
        raise AssertionError(f"{err}\n" + "\n".join(f"  {n}: {where(got[n], want[n])}" for n in fields)) from None
    cmp_located(om, h64, ("rho_d", "rtheta", "rq", "ru", "rv", "rw", "T", "p"), STEP_TOL)
    a, b = hm.momentum["ρw"].interior_cpu(), h64.momentum["ρw"].interior_cpu()
    assert np.abs(a - b).max() > 1e-12 * np.abs(b).max()      # the Float32 path ran


@pytest.mark.gpu
def test_float32_twin_on_ragged_rows_matches_the_float64_oracle(oracle, oc, bz, monkeypatch):
    """The Float32 twin library on 130 x 9 x 6: the dry case of test_float32_compressible_steps_match_the_float64_oracle (f32_cases.
    compressible_bubble: its domain, reference state and balanced bubble) with the row length changed, judged with the "compressible"
    table.  The case's 4 s are run as four steps of 1 s: its two steps of 2 s have an acoustic Courant number of 0.94 on the 123 m cells
    (0.17 on the case's own), where rounding differences grow as on the 258-cell row above — measured 4e-2 to 6e-2 of the increment in
    every field, no column standing out.  Measured with 1 s steps on the MI355X: rho_d 4.9e-4, rho theta 3.8e-4, rho q 1.0e-3, T 9.0e-4,
    p 4.8e-4, rho u 7.7e-4, rho w 1.3e-4 (eight steps of 0.5 s: the same within 1.4 x)."""
    import torch
    import f32_cases as fc
    from helpers import assert_increments
    case = fc.STEP_CASES["compressible_dry"]
    monkeypatch.setattr(fc, "CS_SIZE", (130, 9, 6))      # the builder reads the size when it runs
    om, hm = fc.compressible_bubble(False)(oracle, oc, bz, {})
    assert (om.grid.Nx, om.grid.Ny, om.grid.Nz) == (130, 9, 6) and hm.momentum["ρu"].parent.dtype == torch.float32
    start = fc.oracle_fields(om, case.fields)
    for _ in range(2 * case.steps):
        om.time_step(case.dt / 2)
        hm.time_step(case.dt / 2)
    hm.synchronize()
    got, want = fc.device_fields(hm, case.fields, compressible=True), fc.oracle_fields(om, case.fields)
    try:
        assert_increments("ragged_twin_130x9x6", got, want, start, case.kind)
    except AssertionError as err:
        raise AssertionError(f"{err}\n" + "\n".join(f"  {n}: {where(got[n], want[n])}" for n in case.fields)) from None


# ---- CPU: the tests above can see a seam error ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def seam_runs(oracle, oc):
    """per shape: the oracle's fields after the loop (substeps = 6, beta = 1) from the loop test's state, unperturbed and with one column off"""
    cache = {}

    def run(size, column):
        key = (size, column)
        if key not in cache:
            tg = _tg()
            og = oracle.Grid(size, x=tg.EXTENT["x"], y=tg.EXTENT["y"], z=tg.EXTENT["z"])
            om = oc.CompressibleOracleModel(og, time_discretization=oc.SplitExplicit(substeps=6), reference_potential_temperature=300.0,
                                            reference_state=True)
            loop_state(om, perturb_column=column)
            om.acoustic_substep_loop(loop_dt(size), 1.0)
            assert om.last_substeps[-1] == 6
            cache[key] = om
        return cache[key]
    return run


@pytest.mark.parametrize("perturbed,observed", [(0, -1), (64, 63)], ids=["periodic-seam", "wave-seam"])
@pytest.mark.parametrize("size", MOIST_SHAPES, ids=_id)
def test_a_wrong_neighbour_at_a_seam_is_far_above_the_loop_tolerance(seam_runs, size, perturbed, observed):
    """rho theta of one column off by 1e-6 before the loop (what its neighbour's edge lane would see of a wrong load): the column on the
    other side of the seam — the row's last cell for column 0, lane 63 of the first wave for column 64 — ends the loop with (rho u)' and
    (rho theta)' more than 100 x 2e-11 away, on the scales the loop test divides by."""
    base, off = seam_runs(size, None), seam_runs(size, perturbed)
    g = base.grid
    i = observed % g.Nx
    for n in ("rup", "rthp"):
        a, b = g.interior(getattr(off, n))[:, :, i], g.interior(getattr(base, n))[:, :, i]
        d = np.abs(a - b).max() / loop_scale(base, n)
        print(f"SEAM {size} column {perturbed} -> {i}: {n} {d:.2e}")
        assert d > 100 * LOOP_TOL, (n, d)
