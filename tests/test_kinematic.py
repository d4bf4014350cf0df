"""AtmosphereModel(dynamics = PrescribedDynamics(...)) on the device (csrc/bz_kinematic.hip) against the CPU restatement of
tests/kinematic_reference.py (pinned by tests/test_kinematic_reference.py).

Grids: k_kin_scalar_stage owns 64 x 4 tiles of columns and marches level chunks of at least 8 levels, so the 3-D grid is 72 x 42 x 24
(Ny = 42, not 40: off the multiple of the tile's 4 rows): two tiles in x and eleven in y, the last of each partial, three level
chunks.  The Flat-y grid is 48 x 1 x 16 with a stretched z (two chunks).  Halo 3.  Tolerances are the project's (README): tendencies 1e-12,
three steps 1e-9, relative to the field's scale."""
import numpy as np
import pytest

from kinematic_reference import KinematicReference, velocity_field

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
DT = 5.0
LZ = 4000.0
GRIDS = {
    "3d": dict(size=(72, 42, 24), x=(0.0, 7200.0), y=(0.0, 4200.0), z=(0.0, LZ), topology=("Periodic", "Periodic", "Bounded"), halo=(3, 3, 3)),
    "flat": dict(size=(48, 16), x=(0.0, 4800.0), y=None, z=LZ * (np.arange(17) / 16.0) ** 1.2, topology=("Periodic", "Flat", "Bounded"),
                 halo=(3, 3)),
}
# microphysics, vapour, tracers, divergence correction
CASES = {
    "dry": (None, False, 0, False),
    "vapour": (None, True, 0, False),
    "sa": ("SaturationAdjustment", True, 0, False),
    "sa_tracers_correction": ("SaturationAdjustment", True, 2, True),
}
TRACER_NAMES = ("a", "b", "c", "d")


def extents(gname):
    G = GRIDS[gname]
    return G["x"][1], (G["y"][1] if G["y"] else 1.0), LZ


def initial_fields(gname):
    """theta, total moisture and tracer profiles.  With saturation adjustment the moisture crosses saturation inside the domain: about half of
    the cells are cloudy after three steps (asserted on the CPU result before anything is compared)."""
    Lx, Ly, Lz = extents(gname)
    # a stratified column with a smooth 8 K wave.  Its gradient sets the scale of the CORRECTED theta tendency, -div_rhoUc + theta div_rhoU =
    # -rho U . grad(theta): a difference of two terms of size theta |div_rhoU| ~ 3.5 whose rounding — about eps max|rho U theta| / min
    # spacing per flux difference, in the restatement as on the device — does not shrink with the result.  test_tendencies_match_restatement
    # asserts that four such roundings of the restatement itself stay below 1e-12 of the tendency's scale.  Measured: with a 0.5 K wave
    # max|G| = 0.0106 and device - restatement = 1.6e-12 of it (5e-15 of the terms, the figure of every uncorrected tendency); a 10 K bubble
    # with a kink at its rim moved theta's WENO weights by more than that (1.8e-12 of the uncorrected tendency), so the wave is smooth.
    theta = lambda x, y, z: 296.0 + 3e-3 * z + 8.0 * np.sin(2 * np.pi * x / Lx) * (1.0 + 0.3 * np.cos(2 * np.pi * y / Ly))
    qt = lambda x, y, z: 0.021 * np.exp(-z / 2500.0) * (1.0 + 0.3 * np.sin(2 * np.pi * x / Lx + 1.0)) + 0 * y
    tracers = (lambda x, y, z: 1.0 + 0.5 * np.sin(2 * np.pi * x / Lx) * np.cos(2 * np.pi * y / Ly) * np.exp(-z / 2e3),
               lambda x, y, z: np.exp(-((x - 0.4 * Lx) / (0.15 * Lx)) ** 2 - ((z - 0.5 * Lz) / (0.2 * Lz)) ** 2) + 0 * y,
               lambda x, y, z: 2.0 + np.cos(2 * np.pi * x / Lx) * np.sin(np.pi * z / Lz) + 0 * y,
               lambda x, y, z: 1.0 + 0 * x + 0 * y + 0 * z)
    return theta, qt, tracers


def make_reference(oracle, gname, microphysics, vapour, tracers, correction, unit_tracer=False):
    G = GRIDS[gname]
    k = KinematicReference(oracle, G["size"], x=G["x"], y=G["y"], z=G["z"], topology=G["topology"], halo=G["halo"],
                           microphysics=microphysics, tracers=tracers, divergence_correction=correction)
    u, v, w = velocity_field(*extents(gname))
    theta, qt, tr = initial_fields(gname)
    k.set(theta=theta, qt=qt if vapour else 0.0, u=u, v=v, w=w)
    rho = k.m.ref.density[k.grid.Hz:k.grid.Hz + k.grid.Nz][:, None, None]
    x, y, z = k.grid.nodes("ccc")
    # tracer densities rho c; unit_tracer: the last tracer is c = 1 exactly (rho c = rho)
    k.set(**{f"rc{t}": rho * (np.ones((k.grid.Nz, k.grid.Ny, k.grid.Nx)) if unit_tracer and t == tracers - 1 else tr[t](x, y, z))
             for t in range(tracers)})
    return k


def make_device(bz, k, gname, microphysics, tracers, correction):
    """The device model with the reference's initial arrays, bit for bit."""
    G = GRIDS[gname]
    grid = bz.RectilinearGrid(G["size"], x=G["x"], y=G["y"], z=G["z"], topology=G["topology"], halo=G["halo"])
    ref = bz.ReferenceState(grid, potential_temperature=300.0)
    mp = bz.SaturationAdjustment(equilibrium=bz.WarmPhaseEquilibrium()) if microphysics else None
    m = bz.AtmosphereModel(grid, dynamics=bz.PrescribedDynamics(ref, divergence_correction=correction), advection=bz.WENO(order=5),
                           microphysics=mp, tracers=TRACER_NAMES[:tracers])
    m.set(ρθ=k.interior("rtheta").copy(), ρqᵗ=k.interior("rq").copy(), u=k.interior("u").copy(), v=k.interior("v").copy(),
          w=k.interior("w").copy(), **{TRACER_NAMES[t]: k.interior(f"rc{t}").copy() for t in range(tracers)})
    return m


def device_fields(m, tracers):
    out = {"rtheta": m.potential_temperature_density, "rq": m.moisture_density, "theta": m.potential_temperature, "q": m.specific_moisture,
           "T": m.temperature}
    if m.microphysics is not None:
        out["qv"], out["ql"] = m.microphysical_fields["qᵛ"], m.microphysical_fields["qˡ"]
    for t in range(tracers):
        out[f"rc{t}"], out[f"c{t}"] = m.tracers[TRACER_NAMES[t]], m.specific_tracers[TRACER_NAMES[t]]
    return out


def rel_err(got, want):
    return np.abs(got - want).max() / max(np.abs(want).max(), 1e-300)


_stepped = {}


def stepped_reference(oracle, gname, case):
    """Three steps of the restatement, computed once per (grid, case) and left unchanged."""
    if (gname, case) not in _stepped:
        microphysics, vapour, tracers, correction = CASES[case]
        k = make_reference(oracle, gname, microphysics, vapour, tracers, correction)
        initial = {n: k.interior(n).copy() for n in ["rtheta", "rq", "u", "v", "w"] + [f"rc{t}" for t in range(tracers)]}
        for _ in range(3):
            k.time_step(DT)
        names = ["rtheta", "rq", "theta", "q", "T"] + (["qv", "ql"] if microphysics else []) + \
            [f"{p}c{t}" for t in range(tracers) for p in ("r", "")]
        final = {n: k.interior(n).copy() for n in names}
        for a in (*initial.values(), *final.values()):
            a.setflags(write=False)
        _stepped[(gname, case)] = (initial, final)
    return _stepped[(gname, case)]


class _Initial:
    """The interface make_device reads, over stored initial arrays."""

    def __init__(self, arrays):
        self.arrays = arrays

    def interior(self, name):
        return self.arrays[name]


def device_tendencies(bz, m, tracers):
    bz.compute_kinematic_tendencies_(m)
    m.synchronize()
    G = {"rtheta": m.G["ρθ"].interior_cpu(), "rq": m.G["ρq"].interior_cpu()}
    for t in range(tracers):
        G[f"rc{t}"] = m.G[TRACER_NAMES[t]].interior_cpu()
    return G


@pytest.mark.parametrize("gname", ["3d", "flat"])
def test_mass_divergence_matches_numpy(oracle, bz, gname):
    """D of k_kin_mass_divergence, read back as the difference of the tendencies of c = 1 with and without the correction."""
    G = {}
    for correction in (False, True):
        k = make_reference(oracle, gname, None, False, 1, correction, unit_tracer=True)
        m = make_device(bz, k, gname, None, 1, correction)
        assert np.all(m.specific_tracers["a"].interior_cpu() == 1.0)
        G[correction] = device_tendencies(bz, m, 1)["rc0"]
    D = k.div_rhoU()
    err = rel_err(G[True] - G[False], D)
    print(gname, "div_rhoU: max|D|", np.abs(D).max(), "relative error", err)
    assert np.abs(D).max() > 1e-3
    assert err < 1e-12
    assert rel_err(-G[False], D) < 1e-12          # without the correction c = 1 has G = -D


@pytest.mark.parametrize("correction", [False, True])
@pytest.mark.parametrize("gname,tracers", [("3d", 2), ("flat", 2), ("3d", 3)])          # 3 tracers: five scalars, a second scalar group
def test_tendencies_match_restatement(oracle, bz, gname, tracers, correction):
    k = make_reference(oracle, gname, None, True, tracers, correction)
    m = make_device(bz, k, gname, None, tracers, correction)
    want = {n: a.copy() for n, a in k.compute_tendencies().items()}
    got = device_tendencies(bz, m, tracers)
    for n in want:
        # the restatement resolves the tolerance: four roundings of a flux difference stay below 1e-12 of the tendency's scale (initial_fields)
        floor = EPS * k.max_mass_flux() * np.abs(k.interior(k.specific[n])).max() / k.min_spacing()
        assert 4 * floor < 1e-12 * np.abs(want[n]).max(), (n, floor, np.abs(want[n]).max())
        err = rel_err(got[n], want[n])
        print(gname, tracers, correction, n, "scale", np.abs(want[n]).max(), "relative error", err)
        assert np.abs(want[n]).max() > 0
        assert err < 1e-12, n


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("gname", ["3d", "flat"])
def test_three_steps_match_restatement(oracle, bz, gname, case):
    microphysics, vapour, tracers, correction = CASES[case]
    initial, want = stepped_reference(oracle, gname, case)
    if microphysics:
        cloudy = (want["ql"] > 0).mean()
        print(gname, case, "cloudy share of the restatement", cloudy)
        assert 0.1 < cloudy < 0.9
    m = make_device(bz, _Initial(initial), gname, microphysics, tracers, correction)
    for _ in range(3):
        m.time_step(DT)
    m.synchronize()
    assert m.clock.iteration == 3 and m.clock.time == 3 * DT
    got = device_fields(m, tracers)
    for n, w in want.items():
        if not np.abs(w).max() > 0:          # dry: rho q = q = 0 exactly
            assert np.all(got[n].interior_cpu() == 0.0), n
            continue
        err = rel_err(got[n].interior_cpu(), w)
        print(gname, case, n, "relative error", err)
        assert err < 1e-9, n


def test_time_steps_is_three_time_steps_and_velocities_stay(oracle, bz):
    case = "sa_tracers_correction"
    microphysics, vapour, tracers, correction = CASES[case]
    initial, _ = stepped_reference(oracle, "3d", case)
    a = make_device(bz, _Initial(initial), "3d", microphysics, tracers, correction)
    b = make_device(bz, _Initial(initial), "3d", microphysics, tracers, correction)
    velocities = {n: f.cpu().copy() for n, f in a.velocities.items()}
    for _ in range(3):
        a.time_step(DT)
    b.time_steps(DT, 3)
    a.synchronize()
    b.synchronize()
    fa, fb = device_fields(a, tracers), device_fields(b, tracers)
    for n in fa:
        assert np.array_equal(fa[n].cpu(), fb[n].cpu()), n
    for n, before in velocities.items():          # a step never writes u, v or w (parents: halos and wall faces included)
        assert np.array_equal(a.velocities[n].cpu(), before), n
        assert np.array_equal(b.velocities[n].cpu(), before), n
    # the trailing diagnosis may be left out and is caught up on the next read
    b.time_steps(DT, 1, diagnose_last=False)
    assert bz.diagnostics_stale(b)
    a.time_step(DT)
    assert np.array_equal(a.temperature.interior_cpu(), b.temperature.interior_cpu()) and not bz.diagnostics_stale(b)


def small_model(bz, correction=False, tracers=("c",), **kw):
    grid = bz.RectilinearGrid((24, 12, 10), x=(0, 2400.0), y=(0, 1200.0), z=(0, 3000.0))
    ref = bz.ReferenceState(grid, potential_temperature=300.0)
    return bz.AtmosphereModel(grid, dynamics=bz.PrescribedDynamics(ref, divergence_correction=correction), advection=bz.WENO(order=5),
                              tracers=tracers, **kw)


def test_set_w_leaves_zeros_on_the_wall_faces(bz):
    m = small_model(bz)
    m.set(θ=300.0, w=10.0)
    w = m.velocities["w"].interior_cpu()
    assert w.shape[0] == 11
    assert np.all(w[0] == 0.0) and np.all(w[-1] == 0.0) and np.all(w[1:-1] == 10.0)
    m.set(w=lambda x, y, z: 1.0 + 0 * x + 0 * y + 0 * z)
    w = m.velocities["w"].interior_cpu()
    assert np.all(w[0] == 0.0) and np.all(w[-1] == 0.0) and np.all(w[1:-1] == 1.0)


def test_gaussian_advection_on_the_device(bz):
    """The reference's analytic test (test/kinematic_driver.jl:89-115), threshold 0.1."""
    Lz, Nz, w0, z0, sigma = 4000.0, 64, 10.0, 1000.0, 100.0
    exact = lambda t: (lambda x, y, z: np.exp(-(z - z0 - w0 * t) ** 2 / (2 * sigma ** 2)) + 0 * x + 0 * y)
    grid = bz.RectilinearGrid((4, 4, Nz), x=(0, 100), y=(0, 100), z=(0, Lz))
    m = bz.AtmosphereModel(grid, dynamics=bz.PrescribedDynamics(bz.ReferenceState(grid)), tracers="c", advection=bz.WENO())
    assert m.pressure_solver is None and list(m.prognostic_fields()) == ["ρθ", "ρq", "c"]
    m.set(θ=300.0, qᵗ=0.0, w=w0, c=exact(0.0))
    m.time_steps(1.0, 50)
    m.synchronize()
    x, y, z = grid.nodes((bz.Center, bz.Center, bz.Center))
    err = np.abs(m.tracers["c"].interior_cpu() - exact(50.0)(x, y, z)).max()
    print("gaussian advection on the device: max error", err)
    assert err < 0.1


def test_uniform_tracer_stays_uniform_with_the_correction(bz):
    m = small_model(bz, correction=True)
    u, v, w = velocity_field(2400.0, 1200.0, 3000.0)
    m.set(θ=300.0, u=u, v=v, w=w)
    rho = m.dynamics.reference_state.density[3:13][:, None, None]
    m.set(c=rho * np.ones((10, 12, 24)))
    assert np.all(m.specific_tracers["c"].interior_cpu() == 1.0)
    m.time_steps(DT, 50)
    m.synchronize()
    dev = np.abs(m.specific_tracers["c"].interior_cpu() - 1.0).max()
    print("c = 1 after 50 steps with the correction: max|c - 1|", dev, "bound", 50 * 64 * EPS)
    assert dev <= 50 * 64 * EPS


def test_host_contract(bz):
    m = small_model(bz)
    with pytest.raises(ValueError, match="momentum"):
        m.set(ρu=1.0)
    with pytest.raises(ValueError, match="momentum"):
        m.set(rho_w=1.0)
    with pytest.raises(NotImplementedError, match="hipGraph"):
        m.graph_enable()
    # the anelastic step entry refuses a kinematic context; _check turns the code into an exception that carries last_error
    import ctypes as C
    rc = m._lib.bz_time_step_anelastic(m._ctx, C.byref(m._state), C.byref(m._U0), C.byref(m._G), 1.0)
    assert rc == 2          # BZ_ERR_UNSUPPORTED
    with pytest.raises(bz.BreezeHIPError, match="PrescribedDynamics"):
        m._check(rc, "bz_time_step_anelastic")
    assert m._lib.bz_time_steps_anelastic(m._ctx, C.byref(m._state), C.byref(m._U0), C.byref(m._G), 1.0, 2, 1) == 2

    from breeze_jl_amd import distributed
    grid = m.grid
    ref = m.dynamics.reference_state
    dyn = lambda: bz.PrescribedDynamics(ref)
    W = bz.WENO(order=5)
    big = bz.RectilinearGrid((24, 12, 10), x=(0, 2400.0), y=(0, 1200.0), z=(0, 3000.0), halo=(5, 5, 5))
    f32 = bz.RectilinearGrid((24, 12, 10), x=(0, 2400.0), y=(0, 1200.0), z=(0, 3000.0), float_type=np.float32)
    walls = bz.RectilinearGrid((24, 12, 10), x=(0, 2400.0), y=(0, 1200.0), z=(0, 3000.0), topology=("Periodic", "Bounded", "Bounded"))
    tetens = bz.ThermodynamicConstants(saturation_vapor_pressure=bz.TetensFormula())
    out_of_scope = {
        "Float32": lambda: bz.AtmosphereModel(f32, dynamics=bz.PrescribedDynamics(bz.ReferenceState(f32)), advection=W),
        "order = 7": lambda: bz.AtmosphereModel(big, dynamics=bz.PrescribedDynamics(bz.ReferenceState(big)), advection=bz.WENO(order=7)),
        "order = 9": lambda: bz.AtmosphereModel(big, dynamics=bz.PrescribedDynamics(bz.ReferenceState(big)), advection=bz.WENO(order=9)),
        "Centered": lambda: bz.AtmosphereModel(grid, dynamics=dyn(), advection=bz.Centered()),
        "Centered advection": lambda: bz.AtmosphereModel(grid, dynamics=dyn()),          # the constructor's default scheme
        "bounds-preserving": lambda: bz.AtmosphereModel(grid, dynamics=dyn(), advection={"momentum": W, "ρθ": W, "ρqᵉ": bz.WENO(bounds=(0, 1))}),
        "StaticEnergy": lambda: bz.AtmosphereModel(grid, dynamics=dyn(), advection=W, formulation="StaticEnergy"),
        "Kessler": lambda: bz.AtmosphereModel(grid, dynamics=dyn(), advection=W, microphysics=bz.DCMIP2016KesslerMicrophysics(),
                                              thermodynamic_constants=tetens),
        "closure": lambda: bz.AtmosphereModel(grid, dynamics=dyn(), advection=W, closure=bz.SmagorinskyLilly()),
        "forcing": lambda: bz.AtmosphereModel(grid, dynamics=dyn(), advection=W, forcing={"ρθ": bz.Forcing(lambda z: 0 * z)}),
        "sponges": lambda: bz.AtmosphereModel(grid, dynamics=dyn(), advection=W, forcing={"ρw": bz.Relaxation(0.1)}),
        "flux and value boundary conditions": lambda: bz.AtmosphereModel(
            grid, dynamics=dyn(), advection=W, boundary_conditions={"ρθ": bz.FieldBoundaryConditions(bottom=bz.FluxBoundaryCondition(0.1))}),
        "NormalFlowBoundaryCondition": lambda: bz.AtmosphereModel(
            grid, dynamics=dyn(), advection=W, boundary_conditions={"w": bz.FieldBoundaryConditions(bottom=bz.NormalFlowBoundaryCondition(0.5))}),
        "PrescribedVelocityFields": lambda: bz.AtmosphereModel(
            grid, dynamics=dyn(), advection=W, velocities=bz.PrescribedVelocityFields(w=lambda x, y, z, t: np.sin(np.pi * z / 2000))),
        "prognostic density": lambda: bz.AtmosphereModel(grid, dynamics=bz.PrescribedDynamics(np.ones(10)), advection=W),
        "slab": lambda: distributed.LibrarySlabAtmosphereModel(grid, 0, 1, transport="local:kinematic", dynamics=dyn(), advection=W),
        "topology": lambda: bz.AtmosphereModel(walls, dynamics=bz.PrescribedDynamics(bz.ReferenceState(walls)), advection=W),
    }
    for option, construct in out_of_scope.items():
        with pytest.raises(NotImplementedError, match=option):
            construct()
    # and the kinematic entry points refuse an anelastic context; a default anelastic model still constructs and steps
    d = bz.AtmosphereModel(grid, advection=W)
    assert d.pressure_solver is not None
    assert list(d.prognostic_fields())[:3] == ["ρu", "ρv", "ρw"]
    assert d._lib.bz_time_steps_kinematic(d._ctx, C.byref(d._state), C.byref(d._U0), C.byref(d._G), 1.0, 1, 1) == 2
    with pytest.raises(bz.BreezeHIPError, match="PrescribedDynamics"):
        d._check(2, "bz_time_steps_kinematic")
    with pytest.raises(ValueError):
        bz.AtmosphereModel(grid, advection=W, velocities=bz.PrescribedVelocityFields(w=lambda x, y, z, t: 0 * z))
    d.set(θ=lambda x, y, z: 300.0 + 1e-3 * z + 0 * x + 0 * y, u=2.0)
    d.time_step(1.0)
    d.synchronize()
    assert np.isfinite(d.potential_temperature_density.interior_cpu()).all()
