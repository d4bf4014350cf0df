"""microphysics = InstantaneousPrecipitation(...) on the compressible split-explicit model (csrc/bz_instant_precip.hip through the C ABI)
against the CPU restatement tests/instantaneous_precipitation_reference.py (pinned by tests/test_instantaneous_precipitation_reference.py).

Kernels and shapes.  k_instantaneous_precipitation is one thread per interior cell, 256 threads along x, grid (ceil(Nx / 256), Ny, Nz); a
ragged Nx is a predicate on the lane.  k_column_integral is one lane per column, lanes along x.
    (8, 8, 8) halo 5     the reference's own grid (test/instantaneous_precipitation.jl:133)
    (40, 6, 5) halo 3    a ragged row below a wavefront; (40, 10, 5) halo 5: the same rows under the wider halo (the model needs Ny >= 2 Hy)
    (66, 6, 4), (130, 9, 6)   a partly filled wavefront behind one and two full ones
    (258, 6, 3)          two lanes into a second 256-thread block
each on a uniform and on a stretched z.  State: the mixed bubble of tests/test_gpu_compressible.py::
test_compressible_saturation_adjustment_matches_oracle scaled to the grid (tests/instantaneous_precipitation_reference.py: bubble_state),
on which between 2 % and 98 % of the cells condense: saturated and clear lanes share wavefronts."""
import ctypes as C

import numpy as np
import pytest

import instantaneous_precipitation_reference as ipr

pytestmark = pytest.mark.gpu

SHAPES = [((8, 8, 8), 5), ((40, 6, 5), 3), ((40, 10, 5), 5), ((66, 6, 4), 3), ((130, 9, 6), 3), ((258, 6, 3), 3)]
PROG = {"rho_d": "ρᵈ", "ru": "ρu", "rv": "ρv", "rw": "ρw", "rtheta": "ρθ", "rq": "ρq"}
EPS = np.finfo(np.float64).eps


def _device(bz, shape, halo, ext, scheme=True, solver=(1e-4, 20), float_type=np.float64):
    grid = bz.RectilinearGrid(shape, halo=halo, float_type=float_type, **ext)
    dyn = bz.CompressibleDynamics(bz.SplitExplicitTimeDiscretization(substeps=6), surface_pressure=1e5, standard_pressure=1e5,
                                  reference_potential_temperature=ipr.theta_ref)
    mp = bz.InstantaneousPrecipitation(equilibrium=bz.WarmPhaseEquilibrium(), solver=bz.SecantSolver(abstol=solver[0], maxiter=solver[1])) if scheme else None
    return bz.CompressibleAtmosphereModel(grid, dyn, advection=bz.WENO(order=5), microphysics=mp)


def _pair(oracle, oc, bz, shape, halo, stretched=False, scheme=True, solver=(1e-4, 20), float_type=np.float64):
    om, ext, L = ipr.make_restatement(oracle, oc, shape, halo, stretched, solver=solver, scheme=scheme)
    return om, _device(bz, shape, halo, ext, scheme, solver, float_type), L


def _bubble(om, L, qt=None, u=2.0):
    """keyword values of set! for both models"""
    g = om.grid
    th, q = ipr.bubble_state(*L)
    rho = om.ref.density[g.Hz:g.Hz + g.Nz][:, None, None]
    return dict(rho=rho, theta=th, u=u, v=0.0, w=0.0, qv=q if qt is None else qt)


def _set_device(hm, ic):
    hm.set(ρ=ic["rho"], θ=ic["theta"], u=ic["u"], v=ic["v"], w=ic["w"], qᵗ=ic["qv"])


def _fields(hm):
    out = {n: hm.prognostic_fields()[k].interior_cpu().copy() for n, k in PROG.items()}
    out["T"], out["p"] = hm.temperature.interior_cpu().copy(), hm.dynamics.pressure.interior_cpu().copy()
    out["rho"] = hm.dynamics.total_density.interior_cpu().copy()
    out["P"] = hm.microphysical_fields["precipitation_rate"].interior_cpu().copy() if hm.microphysics is not None else None
    return out


def _worst(got, om, names):
    g = om.grid
    mom = max(np.abs(g.interior(getattr(om, n), n == "rw")).max() for n in ("ru", "rv", "rw"))
    worst = {}
    for n in names:
        want = g.interior(getattr(om, n), n == "rw")
        scale = mom if n in ("ru", "rv", "rw") else np.abs(want).max()
        worst[n] = np.abs(got[n] - want).max() / max(scale, 1e-300)
    return worst


def _periodic_images_hold(field, grid):
    P = field.parent.cpu().numpy()
    Hx, Hy, Hz, Nz = grid.Hx, grid.Hy, grid.Hz, grid.Nz
    want = np.pad(field.interior_cpu(), ((0, 0), (Hy, Hy), (Hx, Hx)), mode="wrap")
    return np.array_equal(P[Hz:Hz + Nz], want)


# ---- the once-per-step update ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stretched", [False, True], ids=["uniform", "stretched"])
@pytest.mark.parametrize("shape,halo", SHAPES, ids=[f"{s[0]}x{s[1]}x{s[2]}-h{h}" for s, h in SHAPES])
def test_update_matches_the_restatement(oracle, oc, bz, shape, halo, stretched):
    """microphysics_model_update! from the same bits (the restatement's state is copied into the device fields, halos included): rho theta,
    rho q^v, rho_d, rho, T, p within 1e-12 of the field's maximum (the bound of the density-based adjustment in tests/test_gpu_compressible.py),
    precipitation_rate within 1e-12 of its maximum and exactly 0 wherever the restatement does not condense, halos refreshed."""
    from test_gpu_compressible import cmp_interior, push
    om, hm, L = _pair(oracle, oc, bz, shape, halo, stretched)
    om.set(**_bubble(om, L))
    om.seed_time_averaged_velocities()
    om.update_state(compute_tendencies=True)
    push(om, hm)
    g = om.grid
    rq0 = g.interior(om.rq).copy()
    om.microphysics_model_update(1.0)
    frac = om.condensed.mean()
    assert 0.02 < frac < 0.98, frac                  # on the restatement alone: cloudy and clear cells
    bz.microphysics_model_update_(hm.microphysics, hm, Δt=1.0)
    hm.synchronize()
    worst = cmp_interior(om, hm, ("rtheta", "rq", "rho_d", "rho", "T", "p"), 1e-12)
    P, Pw = hm.microphysical_fields["precipitation_rate"].interior_cpu(), g.interior(om.precipitation_rate)
    errP = np.abs(P - Pw).max() / Pw.max()
    print(f"IPUPDATE {shape} stretched={stretched} condensing={frac:.2f}:", " ".join(f"{n}={e:.1e}" for n, e in worst.items()), f"P={errP:.1e}")
    assert errP <= 1e-12
    assert np.all(P[~om.condensed] == 0.0) and np.all(P[om.condensed] > 0.0)
    assert np.abs(g.interior(om.rq) - rq0).max() > 1e-6 * rq0.max()      # the update acted
    assert _periodic_images_hold(hm.potential_temperature_density, hm.grid)
    assert _periodic_images_hold(hm.moisture_density, hm.grid)
    # q^v of the microphysical fields is the specific moisture the closing update_state! diagnosed
    assert hm.microphysical_fields["qᵛ"] is hm.specific_moisture
    assert np.abs(hm.specific_moisture.interior_cpu() - g.interior(om.q)).max() <= 1e-12 * g.interior(om.q).max()


@pytest.mark.parametrize("dt", [float("nan"), float("inf"), 0.0, -1.0])
def test_update_is_skipped_for_an_invalid_time_step(oracle, oc, bz, dt):
    om, hm, L = _pair(oracle, oc, bz, (40, 6, 5), 3)
    _set_device(hm, _bubble(om, L))
    before = _fields(hm)
    G0 = hm.G["ρq"].parent.clone()
    hm.G["ρq"].parent.fill_(7.0)                     # the trailing update_state! would rewrite the moisture tendency
    bz.microphysics_model_update_(hm.microphysics, hm, Δt=dt)
    bz.microphysics_model_update_(hm.microphysics, hm)      # clock.last_Δt of a model that has not stepped is infinite
    hm.synchronize()
    after = _fields(hm)
    for n in before:
        assert np.array_equal(before[n], after[n]), n
    assert bool((hm.G["ρq"].parent == 7.0).all())
    hm.G["ρq"].parent.copy_(G0)


# ---- the reference's integration assertions on the device (test/instantaneous_precipitation.jl:131-217) -------------------------------------
def _scenario(oracle, oc, bz, qt):
    om, hm, _ = _pair(oracle, oc, bz, (8, 8, 8), 5)
    g = om.grid
    hm.set(ρ=om.ref.density[g.Hz:g.Hz + g.Nz][:, None, None], θ=300.0, qᵗ=qt)
    bz.compressible.update_state_(hm)
    return om, hm


def test_supersaturated_scenario_on_the_device(oracle, oc, bz):
    from oracle import thermo
    om, hm = _scenario(oracle, oc, bz, 0.030)
    tc = thermo.ThermoConstants()
    before = _fields(hm)
    assert not before["P"].any()
    hm.clock.last_Δt = 1.0
    bz.microphysics_model_update_(hm.microphysics, hm)
    hm.synchronize()
    after = _fields(hm)
    rt, rd, rth1, rq1, P = before["rho"], before["rho_d"], after["rtheta"], after["rq"], after["P"]
    assert np.all(np.isfinite(rth1)) and np.all(np.isfinite(rq1))
    assert np.all(rq1 < before["rq"]) and np.all(rth1 > before["rtheta"]) and np.all(P > 0)
    assert np.all(np.abs(P - (before["rq"] - rq1) / 1.0) <= 1e-6 * np.abs(P))
    for idx in np.ndindex(rt.shape):
        qv, thf = rq1[idx] / rt[idx], rth1[idx] / rd[idx]
        T = thermo.density_state_temperature(thf, qv, 0.0, rt[idx], 1e5, tc)
        assert abs(qv - thermo.saturation_specific_humidity(T, rt[idx], tc, "liquid")) < 1e-4
    assert bz.precipitation_rate(hm, "ice") is None
    assert bz.precipitation_rate(hm, "liquid").compute() is hm.microphysical_fields["precipitation_rate"]
    flux = bz.surface_precipitation_flux(hm).compute().cpu().numpy()
    dz = om.grid.dzc[om.grid.Hz:om.grid.Hz + om.grid.Nz]
    want = np.einsum("kji,k->ji", P, dz)
    assert np.all(flux > 0)
    assert np.all(np.abs(flux - want) <= (om.grid.Nz + 2) * EPS * want)
    bz.compressible.update_state_(hm)                # a following update_state! preserves the diagnostic
    assert np.array_equal(hm.microphysical_fields["precipitation_rate"].interior_cpu(), P)


def test_subsaturated_scenario_on_the_device(oracle, oc, bz):
    om, hm = _scenario(oracle, oc, bz, 0.001)
    before = _fields(hm)
    hm.clock.last_Δt = 1.0
    bz.microphysics_model_update_(hm.microphysics, hm)
    hm.synchronize()
    after = _fields(hm)
    for n in ("rtheta", "rq"):
        assert np.all(np.abs(after[n] - before[n]) <= 1e-8 * np.abs(before[n])), n
    assert not after["P"].any()
    assert not bz.surface_precipitation_flux(hm).compute().cpu().numpy().any()


def test_existing_diagnostics_treat_the_model_as_vapour_only(oracle, oc, bz):
    """RelativeHumidity, SaturationSpecificHumidity and the virtual potential temperature of a model with the scheme are those of a model
    without microphysics in the same state, bit for bit; specific_humidity(model) is the q^v of the microphysical fields"""
    om, a, L = _pair(oracle, oc, bz, (40, 6, 5), 3)
    _, b, _ = _pair(oracle, oc, bz, (40, 6, 5), 3, scheme=False)
    ic = _bubble(om, L)
    for m in (a, b):
        _set_device(m, ic)
    assert bz.compressible.specific_humidity(a) is a.specific_moisture
    for op in (bz.RelativeHumidity, bz.SaturationSpecificHumidity, bz.VirtualPotentialTemperature):
        x, y = op(a).compute().interior_cpu(), op(b).compute().interior_cpu()
        assert np.isfinite(x).all() and np.array_equal(x, y), op.__name__
    with pytest.raises(NotImplementedError, match="InstantaneousPrecipitation"):
        bz.surface_precipitation_flux(b)


# ---- bz_column_integral ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,stretched", [((130, 9, 6), True), ((258, 6, 3), False)], ids=["130x9x6-stretched", "258x6x3"])
def test_column_integral(oracle, oc, bz, shape, stretched):
    """sum_k f[k] dz_c[k] against numpy within (Nz + 2) eps sum |f| dz (Nz products, Nz - 1 additions, fused or not); only interior positions of
    the 2-D array are written; two launches give the same bits"""
    import torch
    om, hm, _ = _pair(oracle, oc, bz, shape, 3, stretched)
    g = om.grid
    rng = np.random.default_rng(3)
    f = bz.Field(hm.grid, (bz.Center, bz.Center, bz.Center), "cuda:0")
    f.parent.fill_(float("nan"))                     # nothing beyond the interior is read
    values = rng.standard_normal((g.Nz, g.Ny, g.Nx)) * 10.0 ** rng.integers(-3, 3, (g.Nz, g.Ny, g.Nx))
    f.set_interior(values)
    dz = g.dzc[g.Hz:g.Hz + g.Nz]
    want, bound = np.einsum("kji,k->ji", values, dz), (g.Nz + 2) * EPS * np.einsum("kji,k->ji", np.abs(values), dz)
    outs = []
    for _ in range(2):
        out = torch.full((g.Ny + 2 * g.Hy, g.Nx + 2 * g.Hx), -7.0, dtype=torch.float64, device="cuda:0")
        hm._check(hm._lib.bz_column_integral(hm._ctx, C.c_void_p(f.ptr()), C.c_void_p(out.data_ptr())), "bz_column_integral")
        hm.synchronize()
        outs.append(out.cpu().numpy())
    assert np.array_equal(outs[0], outs[1])
    inner = outs[0][g.Hy:g.Hy + g.Ny, g.Hx:g.Hx + g.Nx]
    assert np.all(np.abs(inner - want) <= bound), np.abs(inner - want).max()
    halo = outs[0].copy()
    halo[g.Hy:g.Hy + g.Ny, g.Hx:g.Hx + g.Nx] = -7.0
    assert np.all(halo == -7.0)
    lazy = bz.ColumnIntegral(hm, f)
    assert np.array_equal(lazy.compute().cpu().numpy(), inner)


# ---- whole steps ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(40, 6, 5), (66, 6, 4)], ids=["40x6x5", "66x6x4"])
def test_three_steps_match_the_restatement(oracle, oc, bz, shape):
    """time_step!, dt = 1 s, substeps = 6: prognostic fields, T and p within 1e-8 (the bound of the saturation-adjustment steps of
    tests/test_gpu_compressible.py), precipitation_rate within 1e-8 of its maximum"""
    om, hm, L = _pair(oracle, oc, bz, shape, 3)
    ic = _bubble(om, L)
    om.set(**ic)
    _set_device(hm, ic)
    for _ in range(3):
        om.time_step(1.0)
        hm.time_step(1.0)
    hm.synchronize()
    got = _fields(hm)
    worst = _worst(got, om, ("rho_d", "rtheta", "rq", "ru", "rv", "rw", "T", "p"))
    Pw = om.grid.interior(om.precipitation_rate)
    worst["P"] = np.abs(got["P"] - Pw).max() / Pw.max()
    print(f"IPSTEPS {shape}:", " ".join(f"{n}={e:.1e}" for n, e in worst.items()), f"condensing={om.condensed.mean():.2f}")
    assert 0.02 < om.condensed.mean() < 0.98
    assert all(e <= 1e-8 for e in worst.values()), worst
    assert hm.clock.last_Δt == 1.0 and hm.clock.iteration == 3


@pytest.mark.parametrize("shape", [(40, 6, 5), (66, 6, 4)], ids=["40x6x5", "66x6x4"])
def test_a_model_that_never_saturates_steps_like_one_without_the_scheme(oracle, oc, bz, shape):
    """q^t = 0.001 everywhere: the two device models differ by the rho (rho q / rho) and theta round trips of the reference only: 1e-13 of the
    field's maximum after three steps, and no precipitation"""
    om, a, L = _pair(oracle, oc, bz, shape, 3)
    _, b, _ = _pair(oracle, oc, bz, shape, 3, scheme=False)
    ic = _bubble(om, L, qt=0.001)
    for m in (a, b):
        _set_device(m, ic)
        for _ in range(3):
            m.time_step(1.0)
        m.synchronize()
    fa, fb = _fields(a), _fields(b)
    mom = max(np.abs(fb[n]).max() for n in ("ru", "rv", "rw"))
    worst = {n: np.abs(fa[n] - fb[n]).max() / (mom if n in ("ru", "rv", "rw") else np.abs(fb[n]).max()) for n in fb if fb[n] is not None}
    print(f"IPDRYPAIR {shape}:", " ".join(f"{n}={e:.1e}" for n, e in worst.items()))
    assert all(e <= 1e-13 for e in worst.values()), worst
    assert not fa["P"].any()


def test_dcmip2016_keyword_list_steps_match_the_restatement(oracle, oc, bz):
    """validation/DCMIP2016_TC/dcmip2016_tc.jl:277-292 on a Cartesian (Periodic, Periodic, Bounded) grid: CompressibleDynamics(
    SplitExplicitTimeDiscretization()), InstantaneousPrecipitation(equilibrium = WarmPhaseEquilibrium()), VerticalScalarDiffusivity(nu = field,
    kappa = field), FPlane — the update_state! that closes the rain-out also forms the closure's water tendency.  (The bulk drag / heat / vapour
    boundary conditions of that script are refused by the compressible constructor: DESIGN section 15.)  Three steps within 1e-8."""
    import compressible_closure_reference as ccr
    import scalar_diffusivity_reference as sdr

    class Restatement(ipr.InstantaneousPrecipitationModel, ccr.ClosureCompressibleModel):
        pass

    shape, halo = (40, 6, 5), 3
    ext, L = ipr.extents(shape)
    og = oracle.Grid(shape, halo=halo, **ext)
    x, y, z = og.nodes("ccc")
    K = [np.ascontiguousarray(np.broadcast_to(a * (1.0 + 0.5 * np.sin(2 * np.pi * x / L[0]) * np.cos(2 * np.pi * y / L[1])) * np.exp(-z / 2e3),
                                              (og.Nz, og.Ny, og.Nx))) for a in (20.0, 30.0)]
    om = Restatement(og, diffusivity=sdr.Diffusivity(1, False, nu=K[0], kappa=K[1]), time_discretization=oc.SplitExplicit(substeps=6),
                     surface_pressure=1e5, standard_pressure=1e5, reference_potential_temperature=ipr.theta_ref, coriolis_f=1e-4)
    grid = bz.RectilinearGrid(shape, halo=halo, **ext)
    Kf = []
    for a in K:
        f = bz.Field(grid, (bz.Center, bz.Center, bz.Center), "cuda:0")
        f.set_interior(a)
        Kf.append(f)
    dyn = bz.CompressibleDynamics(bz.SplitExplicitTimeDiscretization(substeps=6), surface_pressure=1e5, standard_pressure=1e5,
                                  reference_potential_temperature=ipr.theta_ref)
    hm = bz.CompressibleAtmosphereModel(grid, dyn, advection=bz.WENO(order=5), closure=bz.VerticalScalarDiffusivity(ν=Kf[0], κ=Kf[1]),
                                        coriolis=bz.FPlane(f=1e-4), microphysics=bz.InstantaneousPrecipitation(equilibrium=bz.WarmPhaseEquilibrium()))
    ic = _bubble(om, L)
    om.set(**ic)
    _set_device(hm, ic)
    for _ in range(3):
        om.time_step(1.0)
        hm.time_step(1.0)
    hm.synchronize()
    got = _fields(hm)
    worst = _worst(got, om, ("rho_d", "rtheta", "rq", "ru", "rv", "rw", "T", "p"))
    Pw = og.interior(om.precipitation_rate)
    worst["P"] = np.abs(got["P"] - Pw).max() / Pw.max()
    print("IPDCMIP:", " ".join(f"{n}={e:.1e}" for n, e in worst.items()))
    assert all(e <= 1e-8 for e in worst.values()), worst


def test_operator_sequence_matches_the_whole_step(oracle, oc, bz):
    om, a, L = _pair(oracle, oc, bz, (40, 6, 5), 3)
    _, b, _ = _pair(oracle, oc, bz, (40, 6, 5), 3)
    ic = _bubble(om, L)
    for m, whole in ((a, True), (b, False)):
        _set_device(m, ic)
        for _ in range(2):
            bz.compressible.time_step_(m, 1.0, whole_step=whole)
        m.synchronize()
    fa, fb = _fields(a), _fields(b)
    mom = max(np.abs(fb[n]).max() for n in ("ru", "rv", "rw"))
    worst = {n: np.abs(fa[n] - fb[n]).max() / (mom if n in ("ru", "rv", "rw") else np.abs(fb[n]).max()) for n in fb}
    print("IPSEAM:", " ".join(f"{n}={e:.1e}" for n, e in worst.items()))
    assert fb["P"].max() > 0
    assert all(e <= 1e-13 for e in worst.values()), worst


def test_recorded_step_replays_the_same_bits(oracle, oc, bz):
    """hipGraph replay: a recorded step contains the update like any other launch"""
    out = []
    for graph in (True, False):
        om, hm, L = _pair(oracle, oc, bz, (40, 6, 5), 3)
        _set_device(hm, _bubble(om, L))
        if graph:
            hm.graph_enable(True)
        for _ in range(4):
            hm.time_step(1.0)
        hm.synchronize()
        if graph:
            en, cap, rep = hm.graph_info()
            assert en and cap >= 1 and rep >= 1, (en, cap, rep)
        out.append(_fields(hm))
    assert out[0]["P"].max() > 0
    for n in out[0]:
        assert np.array_equal(out[0][n], out[1][n]), n


# ---- Float32 twin ------------------------------------------------------------------------------------------------------------------------------
def test_float32_update_within_the_references_float32_figures(oracle, oc, bz):
    """eltype(grid) = Float32 at (66, 6, 4), SecantSolver(abstol = 1e-6) (test/instantaneous_precipitation.jl:104-106): the update on the
    device's own inputs.  q^v+ = rho q^v / rho and theta_f = rho theta / rho_d of the device's post-state (rho, rho_d of before the update)
    within rtol = 1e-4 of the Float64 scalar update of each cell; T of the trailing update_state! within rtol = 1e-4 of the Float64
    restatement run from the same inputs.  The same formulas in numpy float32 are evaluated and printed beside the device's errors."""
    import torch
    shape = (66, 6, 4)
    om, hm, L = _pair(oracle, oc, bz, shape, 3, solver=(1e-6, 20), float_type=np.float32)
    assert hm.moisture_density.parent.dtype == torch.float32
    _set_device(hm, _bubble(om, L))
    g = om.grid
    pre = {n: f.parent.cpu().numpy().astype(np.float64) for n, f in (("rho_d", hm.dynamics.dry_density), ("rho", hm.dynamics.total_density),
                                                                      ("rtheta", hm.potential_temperature_density), ("rq", hm.moisture_density),
                                                                      ("ru", hm.momentum["ρu"]), ("rv", hm.momentum["ρv"]), ("rw", hm.momentum["ρw"]))}
    for n, a in pre.items():
        getattr(om, n)[...] = a
    om.update_state(compute_tendencies=False)
    I = g.interior
    r0, rd0, th0, q0 = I(pre["rho"]), I(pre["rho_d"]), I(pre["rtheta"]) / I(pre["rho_d"]), I(pre["rq"]) / I(pre["rho"])
    bz.microphysics_model_update_(hm.microphysics, hm, Δt=1.0)
    hm.synchronize()
    om.microphysics_model_update(1.0)
    assert 0.02 < om.condensed.mean() < 0.98
    qv_dev = hm.moisture_density.interior_cpu().astype(np.float64) / r0
    thf_dev = hm.potential_temperature_density.interior_cpu().astype(np.float64) / rd0
    f32 = ipr.in_dtype(np.float32)
    err = dict(qv=0.0, theta_f=0.0)
    yard = dict(qv=0.0, theta_f=0.0)
    for idx in np.ndindex(r0.shape):
        want = ipr.ip_update(float(th0[idx]), float(q0[idx]), float(r0[idx]), 1e5, abstol=1e-6)
        y = f32.ip_update(th0[idx], q0[idx], r0[idx], 1e5, abstol=1e-6)
        for n, dev in (("qv", qv_dev[idx]), ("theta_f", thf_dev[idx])):
            err[n] = max(err[n], abs(dev - want[n]) / abs(want[n]))
            yard[n] = max(yard[n], abs(float(y[n]) - want[n]) / abs(want[n]))
    Tw = I(om.T)
    err["T"] = float(np.max(np.abs(hm.temperature.interior_cpu().astype(np.float64) - Tw) / Tw))
    print("IPF32 device:", " ".join(f"{n}={e:.2e}" for n, e in err.items()), "| numpy float32:", " ".join(f"{n}={e:.2e}" for n, e in yard.items()))
    assert all(e <= 1e-4 for e in err.values()), err
    P = hm.microphysical_fields["precipitation_rate"].interior_cpu()
    assert P.dtype == np.float32 and P.max() > 0 and np.all(P >= 0)


def test_float32_steps_by_increments(oracle, oc, bz):
    """eltype(grid) = Float32: three steps against the Float64 restatement, judged per field by helpers.increment_error as
    tests/test_compressible_closure.py::test_float32_steps_by_increments judges the closures: the bound is the larger of
    F32_INCREMENT_TOL["compressible"] and 4 x the increment error of the same case without the scheme (Float32 device with microphysics = None
    against the Float64 oracle with microphysics = None), measured in the same test; the ratio is printed."""
    import torch
    from helpers import F32_INCREMENT_TOL, increment_error
    shape = (66, 6, 4)
    names = ("rho_d", "rtheta", "rq", "ru", "rw")
    errs = {}
    for scheme in (False, True):
        om, hm, L = _pair(oracle, oc, bz, shape, 3, scheme=scheme, float_type=np.float32)
        assert hm.momentum["ρu"].parent.dtype == torch.float32
        ic = _bubble(om, L)
        om.set(**ic)
        _set_device(hm, ic)
        g = om.grid
        start = {n: g.interior(getattr(om, n), n == "rw").copy() for n in names}
        for _ in range(3):
            om.time_step(1.0)
            hm.time_step(1.0)
        hm.synchronize()
        got = _fields(hm)
        errs[scheme] = {n: increment_error(got[n], g.interior(getattr(om, n), n == "rw"), start[n]) for n in names}
        print(f"F32INC scheme={scheme}:", " ".join(f"{n}={e:.2e}" for n, e in errs[scheme].items()))
    print("F32INC ratio:", " ".join(f"{n}={errs[True][n] / errs[False][n]:.2f}" for n in names))
    tol = F32_INCREMENT_TOL["compressible"]
    bad = {n: (e, max(tol[n], 4 * errs[False][n])) for n, e in errs[True].items() if not e <= max(tol[n], 4 * errs[False][n])}
    assert not bad, bad


# ---- ABI refusals ------------------------------------------------------------------------------------------------------------------------------
def _refused(model, bz):
    c = model.thermodynamic_constants
    sa = model._T.bz_saturation_adjustment(c.liquid_reference_latent_heat, c.liquid_heat_capacity, c.energy_reference_temperature,
                                           c.triple_point_temperature, c.triple_point_pressure, 1e-4, 20, 0)
    P = bz.Field(model.grid, (bz.Center, bz.Center, bz.Center), "cuda:0")
    rc = model._lib.bz_set_instantaneous_precipitation(model._ctx, C.byref(sa), C.c_void_p(P.ptr()))
    return rc, model._lib.bz_last_error(model._ctx).decode()


def test_abi_refusals_name_the_function(bz):
    ext = dict(x=(0.0, 1.6e3), y=(0.0, 1.6e3), z=(0.0, 1e3))
    grid = bz.RectilinearGrid((16, 16, 8), **ext)
    anelastic = bz.AtmosphereModel(grid, dynamics=bz.AnelasticDynamics(bz.ReferenceState(grid, potential_temperature=300.0)), advection=bz.WENO(order=5))
    dyn = lambda: bz.CompressibleDynamics(bz.SplitExplicitTimeDiscretization(substeps=6), reference_potential_temperature=300.0)
    kessler = bz.CompressibleAtmosphereModel(grid, dyn(), advection=bz.WENO(order=5), microphysics=bz.DCMIP2016KesslerMicrophysics(),
                                             thermodynamic_constants=bz.ThermodynamicConstants(saturation_vapor_pressure=bz.TetensFormula()))
    walls = bz.CompressibleAtmosphereModel(bz.RectilinearGrid((16, 16, 8), topology=(bz.Periodic, bz.Bounded, bz.Bounded), **ext), dyn(),
                                           advection=bz.WENO(order=5))
    for name, model in (("anelastic", anelastic), ("Kessler", kessler), ("walls in y", walls)):
        rc, message = _refused(model, bz)
        assert rc == 2 and "bz_set_instantaneous_precipitation" in message, (name, rc, message)
    plain = bz.CompressibleAtmosphereModel(grid, dyn(), advection=bz.WENO(order=5))
    rc, message = _refused(plain, bz)
    assert rc == 0, (rc, message)
    assert plain._lib.bz_set_instantaneous_precipitation(plain._ctx, None, None) == 0      # NULL detaches
