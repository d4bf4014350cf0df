"""GPU tests of the wind- and stability-dependent bulk surface fluxes on a filtered surface state (bz_set_surface_layer): the device
through the C ABI against the Float64 restatement tests/surface_layer_reference.py."""
import ctypes as C

import numpy as np
import pytest

import helpers
import surface_layer_reference as slr

pytestmark = pytest.mark.gpu

P0, TH0 = 101500.0, 299.1
GRIDS = {"3d": dict(size=(16, 12, 8), ext=dict(x=(0.0, 3200.0), y=(0.0, 2400.0), z=(0.0, 600.0)), topo=("Periodic", "Periodic", "Bounded")),
         "flat": dict(size=(64, 24), ext=dict(x=(-10e3, 10e3), z=(0.0, 3000.0)), topo=("Periodic", "Flat", "Bounded"))}


def _T0(kind):
    """a non-uniform sea-surface temperature: warmer and colder than the air, (Ny, Nx)"""
    if kind == "3d":
        return lambda x, y: 296.0 + 3.0 * np.sin(2 * np.pi * x / 3200.0 + 0.4) * np.cos(2 * np.pi * y / 2400.0 - 0.3)
    return lambda x: 296.0 + 3.0 * np.sin(2 * np.pi * x / 20e3 + 0.4)


def _T0_array(kind, og):
    f = _T0(kind)
    if kind == "3d":
        return np.array([[f(x, y) for x in og.xc] for y in og.yc])
    return np.array([[f(x) for x in og.xc]])


def _pair(oracle, bz, kind, stability=True, filtered=False, tau=np.inf, gust=(0.2, 0.2, 0.1), float_type=np.float64, T0=None, poly=True, graph=False,
          advection=None):
    """(oracle model, SurfaceLayer spec, HIP model) with all three conditions on identical grids"""
    G = GRIDS[kind]
    og = oracle.Grid(G["size"], topology=G["topo"], **G["ext"])
    T0a = _T0_array(kind, og) if T0 is None else T0
    mk = lambda p, k: slr.Polynomial(p, k, stability=stability) if poly else 1.2e-3
    sl = slr.SurfaceLayer(P0, 1e5, drag=(mk(slr.DRAG_POLYNOMIAL, "momentum"), gust[0], T0a), heat=(mk(slr.HEAT_POLYNOMIAL, "scalar"), gust[1], T0a),
                          vapor=(mk(slr.VAPOR_POLYNOMIAL, "scalar"), gust[2], T0a), filtered=filtered, tau=tau)
    from oracle.forcings import ColumnForcings
    om = oracle.OracleModel(og, surface_pressure=P0, potential_temperature=TH0, microphysics="SaturationAdjustment", forcings=ColumnForcings(bulk=sl))
    topo = tuple(getattr(bz, t) for t in G["topo"])
    grid = bz.RectilinearGrid(G["size"], topology=topo, float_type=float_type, **G["ext"])
    ref = bz.ReferenceState(grid, surface_pressure=P0, potential_temperature=TH0)
    coef = (bz.PolynomialCoefficient() if stability else bz.PolynomialCoefficient(stability_function=None)) if poly else 1.2e-3
    fv = bz.FilteredSurfaceVelocities(grid, filter_timescale=tau) if filtered else None
    T0h = T0a if T0 is not None else _T0(kind)
    d = bz.BulkDrag(coefficient=coef, gustiness=gust[0], surface_temperature=T0h, filtered_velocities=fv)
    bcs = {"ρu": bz.FieldBoundaryConditions(bottom=d), "ρv": bz.FieldBoundaryConditions(bottom=d),
           "ρe": bz.FieldBoundaryConditions(bottom=bz.BulkSensibleHeatFlux(coefficient=coef, gustiness=gust[1], surface_temperature=T0h, filtered_velocities=fv)),
           "ρqᵉ": bz.FieldBoundaryConditions(bottom=bz.BulkVaporFlux(coefficient=coef, gustiness=gust[2], surface_temperature=T0h, filtered_velocities=fv))}
    hm = bz.AtmosphereModel(grid, dynamics=bz.AnelasticDynamics(ref), advection=advection or bz.WENO(order=5), boundary_conditions=bcs,
                            microphysics=bz.SaturationAdjustment(equilibrium=bz.WarmPhaseEquilibrium()))
    if graph:
        hm.graph_enable(True)
    return om, sl, hm


def _seed(om, hm, bz, seed, calm=True, amp_q=5e-3):
    """a seeded state on both models; a patch of nearly calm first-level cells so that U < U_min occurs"""
    helpers.randomize(om, seed, amp_q=amp_q)
    if calm:
        g = om.grid
        for f in (om.ru, om.rv):
            g.interior(f)[0, :min(4, g.Ny), 2:7] *= 1e-3
        om.update_state(compute_tendencies=False)
    helpers.push_state(om, hm)
    bz.update_state_(hm, compute_tendencies=False)      # the device's own diagnostics (q^v, q^l of the saturation adjustment included)


def _device_first_level(hm):
    I = lambda f: f.interior_cpu()[0].astype(np.float64)
    μ = hm.microphysical_fields
    g = hm.grid
    ref = hm.dynamics.reference_state
    f = dict(u=I(hm.velocities["u"]), v=I(hm.velocities["v"]), theta=I(hm.potential_temperature), q=I(hm.specific_moisture),
             qv=I(μ["qᵛ"]), ql=I(μ["qˡ"]), T=I(hm.temperature))
    f["thv"] = slr.virtual_potential_temperature(f["T"], f["qv"], f["ql"], ref.pressure[g.Hz], ref.standard_pressure)
    return f


def _flux_tendencies(hm, bz):
    for f in hm.G.values():
        f.parent.zero_()
    bz.compute_flux_bc_tendencies_(hm)
    hm.synchronize()
    return {n: hm.G[k].interior_cpu()[0].astype(np.float64) for n, k in (("Ju", "ρu"), ("Jv", "ρv"), ("Jtheta", "ρθ"), ("Jq", "ρq"))}


def _far_fields(f, rng):
    """filtered fields far from the live ones (the reference's own trick, test/polynomial_bulk_coefficients.jl:808-863), with a calm patch"""
    sh = f["u"].shape
    F = dict(u=-2.0 * f["u"] + 1.5 + rng.standard_normal(sh), v=0.5 * f["v"] - 2.0 + rng.standard_normal(sh), thv=f["thv"] + 1.5 * rng.standard_normal(sh),
             theta=f["theta"] - 0.7 + 0.5 * rng.standard_normal(sh), q=0.5 * f["q"] + 1e-3)
    F["u"][:min(4, sh[0]), 8:13] *= 1e-3
    F["v"][:min(4, sh[0]), 8:13] *= 1e-3
    return F


def _set_filtered(hm, F):
    for name, key in (("u", "u"), ("v", "v"), ("θᵥ", "thv"), ("θ", "theta"), ("q", "q")):
        hm.set_filtered_surface_field(name, F[key])


@pytest.mark.parametrize("filtered", [False, True])
@pytest.mark.parametrize("stability", [True, False])
@pytest.mark.parametrize("kind", ["3d", "flat"])
def test_flux_tendencies_match_restatement(oracle, bz, kind, stability, filtered):
    """one bz_compute_flux_bc_tendencies call against the restatement fed with the device's own first-level fields, 1e-12 of each
    field's tendency scale; the inputs reach every regime of the Ri_B -> zeta mapping and both sides of U_min, away from Ri_B = 0.2"""
    om, sl, hm = _pair(oracle, bz, kind, stability=stability, filtered=filtered)
    _seed(om, hm, bz, 21)
    f = _device_first_level(hm)
    g = om.grid
    flat = (False, g.Ny == 1 and g.Hy == 0)
    if filtered:
        F = _far_fields(f, np.random.default_rng(3))
        _set_filtered(hm, F)
        J = slr.fluxes(sl, F["u"], F["v"], F["theta"], F["q"], F["thv"], g.zc[0], *flat)
        wind = F
    else:
        J = slr.fluxes(sl, f["u"], f["v"], f["theta"], f["qv"], f["thv"], g.zc[0], *flat)
        wind = f
    if stability:
        Ri = J["Ri"]["drag"]
        sq = lambda a, di=0, dj=0: slr._shift(a, di, dj, *flat) ** 2
        Uc = np.sqrt((sq(wind["u"]) + sq(wind["u"], 1, 0)) / 2 + (sq(wind["v"]) + sq(wind["v"], 0, 1)) / 2)
        print(f"SL inputs {kind} filtered={filtered}: Ri_B in [{Ri.min():.3g}, {Ri.max():.3g}], unstable {np.sum(Ri < 0)}, weakly {np.sum((Ri >= 0) & (Ri <= 0.2))}, "
              f"strongly {np.sum(Ri > 0.2)}, U<U_min {np.sum(Uc < 0.1)}, min|Ri-0.2| {np.abs(Ri - 0.2).min():.3g}")
        assert np.any(Ri < 0) and np.any((Ri >= 0) & (Ri <= 0.2)) and np.any(Ri > 0.2)
        assert np.any(Uc < 0.1) and np.any(Uc > 0.1)
        assert np.abs(Ri - 0.2).min() > 1e-6
    got = _flux_tendencies(hm, bz)
    dz = g.dzc[g.Hz]
    for n in ("Ju", "Jv", "Jtheta", "Jq"):
        want = J[n] / dz
        scale = np.abs(want).max()
        err = np.abs(got[n] - want).max() / scale
        print(f"SL flux {kind} stability={stability} filtered={filtered} {n}: {err:.3e}")
        assert scale > 0 and err < 1e-12, (n, err)


@pytest.mark.parametrize("kind", ["3d", "flat"])
def test_filter_initialize_update_and_round_trip(oracle, bz, kind):
    om, sl, hm = _pair(oracle, bz, kind, filtered=True, tau=50.0)
    _seed(om, hm, bz, 4)
    hm.initialize_()
    f0 = _device_first_level(hm)
    names = (("u", "u"), ("v", "v"), ("θᵥ", "thv"), ("θ", "theta"), ("q", "q"))
    for name, key in names:
        got = hm.filtered_surface_field(name)
        assert np.abs(got - f0[key]).max() < 1e-10, name
        if key != "thv":
            assert np.array_equal(got, f0[key]), name
    _seed(om, hm, bz, 5)      # the live fields move; the filter lags
    f1 = _device_first_level(hm)
    eps = 0.1
    hm.update_filtered_surface_state_(eps * 50.0)
    hm.update_filtered_surface_state_(eps * 50.0)
    for name, key in names:
        one = (f0[key] + eps * f1[key]) / (1 + eps)
        two = (one + eps * f1[key]) / (1 + eps)
        err = np.abs(hm.filtered_surface_field(name) - two).max()
        print(f"SL filter {kind} {name}: {err:.3e}")
        assert err < 1e-10, (name, err)
    rng = np.random.default_rng(9)
    for name, _ in names:
        a = rng.standard_normal((hm.grid.Ny, hm.grid.Nx))
        hm.set_filtered_surface_field(name, a)
        assert np.array_equal(hm.filtered_surface_field(name), a), name


def _ic(om, hm, kind):
    th = lambda x, y, z: TH0 + 0.004 * z + 0.5 * np.sin(2 * np.pi * x / (om.grid.Nx * om.grid.dx)) * np.exp(-z / 300.0) + 0 * y
    qt = lambda x, y, z: 0.016 * np.exp(-z / 2200.0) + 0 * x + 0 * y
    u = lambda x, y, z: -4.0 + 2.5 * np.sin(2 * np.pi * x / (om.grid.Nx * om.grid.dx) + 1.0) + 2e-3 * z + 0 * y
    v = lambda x, y, z: 1.5 * np.cos(2 * np.pi * x / (om.grid.Nx * om.grid.dx)) + 0 * y + 0 * z
    om.set(theta=th, qt=qt, u=u, v=v)
    if kind == "flat":
        hm.set(θ=lambda x, z: th(x, 0.0, z), qᵗ=lambda x, z: qt(x, 0.0, z), u=lambda x, z: u(x, 0.0, z), v=lambda x, z: v(x, 0.0, z))
    else:
        hm.set(θ=th, qᵗ=qt, u=u, v=v)


FIELDS = (("ru", lambda m: m.momentum["ρu"]), ("rv", lambda m: m.momentum["ρv"]), ("rw", lambda m: m.momentum["ρw"]),
          ("rtheta", lambda m: m.potential_temperature_density), ("rq", lambda m: m.moisture_density), ("T", lambda m: m.temperature))


def _compare(hm, om, tol, label):
    og = om.grid
    mom = max(np.abs(og.interior(getattr(om, n), n == "rw")).max() for n in ("ru", "rv", "rw"))
    for n, get in FIELDS:
        want, got = og.interior(getattr(om, n), n == "rw"), get(hm).interior_cpu()
        scale = mom if n in ("ru", "rv", "rw") else max(np.abs(want).max(), 1e-6)
        err = np.abs(got - want).max() / scale
        print(f"SL steps {label} {n}: {err:.3e}")
        assert err < tol, (label, n, err)


@pytest.mark.parametrize("kind", ["flat", "3d"])
def test_three_steps_match_oracle_driven_restatement(oracle, bz, kind):
    """three steps, filter on with tau = 3 dt: the whole step against the oracle-driven restatement (2e-9 of each field's scale, the
    tolerance of the constant-coefficient test on the same grid); the per-operator sequence against the whole step (1e-13);
    bz_time_steps_anelastic(n = 3) against three single steps (bitwise)"""
    dt = 3.0
    om, sl, hm = _pair(oracle, bz, kind, filtered=True, tau=3 * dt, gust=(1e-2, 1e-2, 1e-2))
    _, _, hp = _pair(oracle, bz, kind, filtered=True, tau=3 * dt, gust=(1e-2, 1e-2, 1e-2))
    _, _, hn = _pair(oracle, bz, kind, filtered=True, tau=3 * dt, gust=(1e-2, 1e-2, 1e-2))
    _ic(om, hm, kind)
    _ic(om, hp, kind)
    _ic(om, hn, kind)
    with slr.patched_oracle():
        for _ in range(3):
            slr.time_step(om, sl, dt)
    u_start = None
    for _ in range(3):
        hm.time_step(dt)
        bz.time_step_(hp, dt, whole_step=False)
        if u_start is None:
            u_start = hm.filtered_surface_field("u").copy()
    hn.time_steps(dt, 3)
    for m in (hm, hp, hn):
        m.synchronize()
    _compare(hm, om, 2e-9, f"{kind} whole-step vs oracle")
    # the filter visibly moved, and follows the restatement's
    for name, key in (("u", "u"), ("v", "v"), ("θᵥ", "thv"), ("θ", "theta"), ("q", "q")):
        got, want = hm.filtered_surface_field(name), sl.fields[key]
        assert np.abs(got - want).max() < 2e-9 * max(np.abs(want).max(), 1e-6), name
    assert np.abs(hm.filtered_surface_field("u") - u_start).max() > 1e-6
    # the components of a vector share its scale (tests/test_gpu_parity.py): the projection spreads a rounding difference of ρu, ρv
    # into ρw, which in these nearly horizontal flows is a thousand times smaller than they are
    mom = max(np.abs(get(hm).interior_cpu()).max() for n, get in FIELDS if n in ("ru", "rv", "rw"))
    for n, get in FIELDS:
        a, b, c = get(hm).interior_cpu(), get(hp).interior_cpu(), get(hn).interior_cpu()
        scale = mom if n in ("ru", "rv", "rw") else max(np.abs(a).max(), 1e-6)
        err = np.abs(a - b).max() / scale
        print(f"SL steps {kind} per-operator vs whole {n}: {err:.3e}")
        assert err < 1e-13, (n, err)
        assert np.array_equal(a, c), f"{n}: n = 3 call differs from three single steps"
    for name in ("u", "v", "θᵥ", "θ", "q"):
        assert np.array_equal(hm.filtered_surface_field(name), hn.filtered_surface_field(name)), name


def test_polynomial_without_wind_dependence_reproduces_constant_entry_point(oracle, bz):
    """stability off and a1 = a2 = 0: C = a0 1e-3 (ln(10/l) / ln(h/l))^2, the constant-coefficient entry point's flux to 1e-14"""
    G = GRIDS["3d"]
    og = oracle.Grid(G["size"], topology=G["topo"], **G["ext"])
    om = oracle.OracleModel(og, surface_pressure=P0, potential_temperature=TH0, microphysics="SaturationAdjustment")
    grid = bz.RectilinearGrid(G["size"], **G["ext"])
    ref = bz.ReferenceState(grid, surface_pressure=P0, potential_temperature=TH0)
    ell, a0 = 1.5e-4, (1.3, 1.1, 1.2)
    h = grid.zᶜ[0]
    Cn = [a * 1e-3 * (np.log(10 / ell) / np.log(h / ell)) ** 2 for a in a0]
    out = []
    for poly in (True, False):
        c = [bz.PolynomialCoefficient(polynomial=(a, 0.0, 0.0), roughness_length=ell, stability_function=None) for a in a0] if poly else Cn
        d = bz.BulkDrag(coefficient=c[0], gustiness=0.2, surface_temperature=299.8)
        bcs = {"ρu": bz.FieldBoundaryConditions(bottom=d), "ρv": bz.FieldBoundaryConditions(bottom=d),
               "ρθ": bz.FieldBoundaryConditions(bottom=bz.BulkSensibleHeatFlux(coefficient=c[1], gustiness=0.2, surface_temperature=300.4)),
               "ρqᵉ": bz.FieldBoundaryConditions(bottom=bz.BulkVaporFlux(coefficient=c[2], gustiness=0.1, surface_temperature=300.4))}
        hm = bz.AtmosphereModel(grid, dynamics=bz.AnelasticDynamics(ref), advection=bz.WENO(order=5), boundary_conditions=bcs,
                                microphysics=bz.SaturationAdjustment(equilibrium=bz.WarmPhaseEquilibrium()))
        assert (hm.filtered_velocities is None) and (hm._surface_layer_keepalive is not None) == poly
        _seed(om, hm, bz, 8, calm=False)
        out.append(_flux_tendencies(hm, bz))
    for n in out[0]:
        scale = np.abs(out[1][n]).max()
        err = np.abs(out[0][n] - out[1][n]).max() / scale
        print(f"SL neutrality constant {n}: {err:.3e}")
        assert scale > 0 and err < 1e-14, (n, err)


def test_filter_with_huge_epsilon_reproduces_unfiltered_flux(oracle, bz):
    """eps so large that f^ = f to rounding: the filtered flux is the unfiltered one (on a condensate-free first level: the filtered
    vapour flux reads the specific prognostic moisture, the unfiltered one q^v)"""
    om, sl, hu = _pair(oracle, bz, "3d", filtered=False)
    _, _, hf = _pair(oracle, bz, "3d", filtered=True, tau=1.0)
    _seed(om, hu, bz, 12, amp_q=1e-3)
    _seed(om, hf, bz, 12, amp_q=1e-3)
    assert np.all(_device_first_level(hu)["ql"] == 0.0)
    hf.initialize_()
    for name in ("u", "v", "θᵥ", "θ", "q"):
        hf.set_filtered_surface_field(name, 7.0)
    hf.update_filtered_surface_state_(1e30)
    a, b = _flux_tendencies(hu, bz), _flux_tendencies(hf, bz)
    for n in a:
        scale = np.abs(a[n]).max()
        err = np.abs(a[n] - b[n]).max() / scale
        print(f"SL neutrality filter {n}: {err:.3e}")
        assert scale > 0 and err < 1e-12, (n, err)


def _reattach(hm, bz, kind, T0a, tau):
    """bz_set_surface_layer with another surface temperature, the filtered fields carried over"""
    from breeze_jl_amd import forcings as F
    keep = {n: hm.filtered_surface_field(n) for n in ("u", "v", "θᵥ", "θ", "q")}
    fv = bz.FilteredSurfaceVelocities(hm.grid, filter_timescale=tau)
    coef = bz.PolynomialCoefficient()
    d = bz.BulkDrag(coefficient=coef, gustiness=1e-2, surface_temperature=T0a, filtered_velocities=fv)
    bcs = {"ρu": d, "ρv": d, "ρe": bz.BulkSensibleHeatFlux(coefficient=coef, gustiness=1e-2, surface_temperature=T0a, filtered_velocities=fv),
           "ρqᵉ": bz.BulkVaporFlux(coefficient=coef, gustiness=1e-2, surface_temperature=T0a, filtered_velocities=fv)}
    L, arrays, _ = F.materialize_surface_layer(hm.grid, bcs, hm.dynamics.reference_state, hm.thermodynamic_constants)
    hm._check(hm._lib.bz_set_surface_layer(hm._ctx, C.byref(L)), "bz_set_surface_layer")
    for n, a in keep.items():
        hm.set_filtered_surface_field(n, a)


def test_graph_replay_is_bitwise_and_follows_a_new_surface_temperature(oracle, bz):
    dt = 3.0
    kw = dict(filtered=True, tau=3 * dt, gust=(1e-2, 1e-2, 1e-2))
    om, _, hg = _pair(oracle, bz, "3d", graph=True, **kw)
    _, _, hl = _pair(oracle, bz, "3d", **kw)
    _, _, hold = _pair(oracle, bz, "3d", graph=True, **kw)
    for m in (hg, hl, hold):
        _ic(om, m, "3d")
        for _ in range(4):
            m.time_step(dt)
        m.synchronize()
    assert hg.graph_info()[2] >= 1, "no step was replayed from a captured graph"
    for n, get in FIELDS:
        assert np.array_equal(get(hg).interior_cpu(), get(hl).interior_cpu()), n
    T1 = _T0_array("3d", om.grid)[::-1, ::-1].copy() + 1.0
    _reattach(hg, bz, "3d", T1, 3 * dt)
    _reattach(hl, bz, "3d", T1, 3 * dt)
    for m in (hg, hl, hold):
        for _ in range(3):
            m.time_step(dt)
        m.synchronize()
    for n, get in FIELDS:
        assert np.array_equal(get(hg).interior_cpu(), get(hl).interior_cpu()), n
    assert not np.array_equal(hg.potential_temperature_density.interior_cpu(), hold.potential_temperature_density.interior_cpu())


def test_float32_twin_example_shaped_case(oracle, bz):
    """the example-shaped 2-D case in Float32, judged by what the steps did to each field (helpers.assert_increments)"""
    dt = 3.0
    om, sl, hm = _pair(oracle, bz, "flat", filtered=True, tau=3 * dt, gust=(1e-2, 1e-2, 1e-2), float_type=np.float32)
    # a 10 K bubble and a moisture blob over the sheared wind (as tests/f32_cases.py: _two_d_anelastic): three steps then move ρθ by
    # 0.36 of its 350 background, 6e3 Float32 ulps, so the 2e-3 tolerance of the increment is 34 ulps wide; the smooth state of _ic
    # moves it by a few ulps only and cannot be judged in Float32
    bub = lambda x, z: np.cos(np.pi / 2 * np.minimum(1.0, np.hypot(x, z - 1200.0) / 1000.0)) ** 2
    Lx = om.grid.Nx * om.grid.dx
    th = lambda x, z: TH0 + 0.004 * z + 10.0 * bub(x, z)
    qt = lambda x, z: 0.012 * np.exp(-z / 2500.0) + 0.004 * bub(x, z)
    u = lambda x, z: -4.0 + 2.5 * np.sin(2 * np.pi * x / Lx + 1.0) + 2e-3 * z
    v = lambda x, z: 1.5 * np.cos(2 * np.pi * x / Lx) + 0 * z
    om.set(theta=lambda x, y, z: th(x, z) + 0 * y, qt=lambda x, y, z: qt(x, z) + 0 * y, u=lambda x, y, z: u(x, z) + 0 * y, v=lambda x, y, z: v(x, z) + 0 * y)
    hm.set(θ=th, qᵗ=qt, u=u, v=v)
    og = om.grid
    start = {n: og.interior(getattr(om, n), n == "rw").copy() for n, _ in FIELDS}
    with slr.patched_oracle():
        for _ in range(3):
            slr.time_step(om, sl, dt)
    for _ in range(3):
        hm.time_step(dt)
    hm.synchronize()
    got = {n: get(hm).interior_cpu() for n, get in FIELDS}
    want = {n: og.interior(getattr(om, n), n == "rw") for n, _ in FIELDS}
    helpers.assert_increments("surface layer flat f32", got, want, start, "anelastic")


def _layer(bz, grid, ref, fv=None):
    from breeze_jl_amd import forcings as F
    coef = bz.PolynomialCoefficient()
    bcs = {"ρu": bz.BulkDrag(coefficient=coef, surface_temperature=300.0, filtered_velocities=fv),
           "ρθ": bz.BulkSensibleHeatFlux(coefficient=coef, surface_temperature=300.0, filtered_velocities=fv)}
    return F.materialize_surface_layer(grid, bcs, ref, bz.ThermodynamicConstants())[0]


def _expect_unsupported(lib, ctx, L, word):
    rc = lib.bz_set_surface_layer(ctx, C.byref(L))
    msg = lib.bz_last_error(ctx).decode()
    assert rc == 2 and "bz_set_surface_layer" in msg and word in msg, (rc, msg)


def test_unsupported_contexts_say_why(bz):
    from breeze_jl_amd import _lib
    grid = bz.RectilinearGrid((16, 16, 8), x=(0, 1600.0), y=(0, 1600.0), z=(0, 800.0))
    ref = bz.ReferenceState(grid, potential_temperature=300.0)
    L = _layer(bz, grid, ref)
    m = bz.AtmosphereModel(grid, dynamics=bz.AnelasticDynamics(ref), advection=bz.WENO(order=5), formulation="StaticEnergy")
    _expect_unsupported(m._lib, m._ctx, L, "StaticEnergy")
    tc = bz.ThermodynamicConstants(saturation_vapor_pressure=bz.TetensFormula())
    m = bz.AtmosphereModel(grid, dynamics=bz.AnelasticDynamics(bz.ReferenceState(grid, tc, potential_temperature=300.0)), advection=bz.WENO(order=5),
                           thermodynamic_constants=tc, microphysics=bz.DCMIP2016KesslerMicrophysics())
    _expect_unsupported(m._lib, m._ctx, L, "Kessler")
    dyn = bz.CompressibleDynamics(bz.SplitExplicitTimeDiscretization(substeps=6), reference_potential_temperature=300.0)
    m = bz.CompressibleAtmosphereModel(grid, dyn, advection=bz.WENO())
    _expect_unsupported(m._lib, m._ctx, L, "Compressible")
    # a filter reference height other than the first cell
    m = bz.AtmosphereModel(grid, dynamics=bz.AnelasticDynamics(ref), advection=bz.WENO(order=5))
    _expect_unsupported(m._lib, m._ctx, _layer(bz, grid, ref, bz.FilteredSurfaceVelocities(grid, height=10.0, filter_timescale=60.0)), "height")
    assert m._lib.bz_set_surface_layer(m._ctx, C.byref(L)) == 0 and m._lib.bz_set_surface_layer(m._ctx, None) == 0      # attach, detach
    # a y-slab context (one rank)
    lib = m._lib
    zf = np.ascontiguousarray(grid.zᶠ, dtype=np.float64)
    bg = _lib.bz_grid()
    bg.Nx, bg.Ny, bg.Nz, bg.Hx, bg.Hy, bg.Hz = grid.Nx, grid.Ny, grid.Nz, grid.Hx, grid.Hy, grid.Hz
    for d, t in enumerate(grid.topology_codes()):
        bg.topo[d] = t
    bg.ftype, bg.dx, bg.dy, bg.regular_z = 8, grid.Δx, grid.Δy, 1
    bg.zf = zf.ctypes.data_as(C.POINTER(C.c_double))
    c = bz.ThermodynamicConstants()
    from breeze_jl_amd.thermodynamics import dry_air_gas_constant, vapor_gas_constant
    bc = _lib.bz_constants(c.gravitational_acceleration, dry_air_gas_constant(c), vapor_gas_constant(c), c.dry_air_heat_capacity, c.vapor_heat_capacity)
    arrays = [np.ascontiguousarray(a, dtype=np.float64) for a in (ref.density, ref.pressure, ref.temperature)]
    br = _lib.bz_reference_state(ref.surface_pressure, ref.potential_temperature, ref.standard_pressure,
                                 *[a.ctypes.data_as(C.POINTER(C.c_double)) for a in arrays])
    ctx = C.c_void_p()
    assert lib.bz_create_slab(C.byref(ctx), C.byref(bg), C.byref(bc), C.byref(br), 5, 1, 0) == 0
    try:
        _expect_unsupported(lib, ctx, L, "slab")
    finally:
        lib.bz_destroy(ctx)
