"""closure = ScalarDiffusivity(...) / VerticalScalarDiffusivity(...), explicit and vertically implicit, on the device
(csrc/bz_diffusivity.hip) through the C ABI, against the CPU restatement tests/scalar_diffusivity_reference.py (pinned by
tests/test_scalar_diffusivity_reference.py).

Shapes: (40, 6, 5) — ragged in x (one partial wave), Nz smaller than a halo of 5; (64, 8, 33) — one whole wave per row, an odd number
of levels; (24, 1, 16) — Flat y.  Each on a uniform and on a stretched z, with halo 3 and halo 5 (halo 5 takes Ny = 6, 8 below 2 Hy: the
per-operator tier).  k_implicit_step has one path per K kind (level table / per-column factors), both covered at every shape.
Tolerances: the implicit step by the forward-error bound of the solve, 32 eps (1 + 4 r) max|phi|, r = max dtau K / min(dz)^2 <= 1e3;
closure tendencies 1e-12 of the closure tendency's scale; three steps 1e-9, tiers among themselves 1e-12 (the project's)."""
import numpy as np
import pytest

import scalar_diffusivity_reference as sdr

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
SHAPES = [(40, 6, 5), (64, 8, 33), (24, 1, 16)]
TRACERS = ("a", "b")


def _z_faces(Nz, stretched):
    """dz = 128 on the uniform grid; the stretched faces are whole numbers (every spacing is exact in Float32 too)"""
    if not stretched:
        return (0.0, 128.0 * Nz)
    s = np.linspace(0.0, 1.0, Nz + 1)
    return np.round(128.0 * Nz * (0.35 * s + 0.65 * s ** 2))


def _grids(oracle, bz, shape, stretched, halo, float_type=np.float64):
    Nx, Ny, Nz = shape
    z = _z_faces(Nz, stretched)
    x, y = (0.0, 100.0 * Nx), (0.0, 100.0 * Ny)
    if Ny == 1:
        og = oracle.Grid((Nx, Nz), x=x, y=None, z=z, topology=("Periodic", "Flat", "Bounded"), halo=(halo, halo))
        grid = bz.RectilinearGrid((Nx, Nz), x=x, z=z, topology=(bz.Periodic, bz.Flat, bz.Bounded), halo=(halo, halo), float_type=float_type)
    else:
        og = oracle.Grid(shape, x=x, y=y, z=z, halo=(halo,) * 3)
        grid = bz.RectilinearGrid(shape, x=x, y=y, z=z, halo=(halo,) * 3, float_type=float_type)
    return og, grid


def _dzmin(og):
    Hz, Nz = og.Hz, og.Nz
    return min(og.dzc[Hz:Hz + Nz].min(), og.dzf[Hz + 1:Hz + Nz].min() if Nz > 1 else np.inf)


def _hip_closure(bz, grid, diff, plant_nan=False):
    """bz closure for a sdr.Diffusivity; array-valued coefficients become centre Fields (optionally NaN everywhere outside the interior)"""
    kw, fields = {}, {}
    for name, key in (("nu", "ν"), ("kappa", "κ")):
        K = getattr(diff, name)
        if isinstance(K, np.ndarray):
            f = bz.Field(grid, (bz.Center, bz.Center, bz.Center), "cuda:0")
            if plant_nan:
                f.parent.fill_(float("nan"))
            f.set_interior(K)
            kw[key] = fields[name] = f
        else:
            kw[key] = K
    cls = bz.VerticalScalarDiffusivity if diff.formulation == 1 else bz.ScalarDiffusivity
    disc = bz.VerticallyImplicitTimeDiscretization() if diff.implicit else bz.ExplicitTimeDiscretization()
    return cls(disc, **kw), fields


def _pair(oracle, bz, shape, stretched, halo, diff, formulation="LiquidIcePotentialTemperature", microphysics=None, tracers=2,
          initialize=True, plant_nan=False, float_type=np.float64, closure=True):
    og, grid = _grids(oracle, bz, shape, stretched, halo, float_type)
    kessler = microphysics == "Kessler"
    om = sdr.DiffusivityModel(og, diff, surface_pressure=1e5, potential_temperature=300.0, formulation=formulation,
                              microphysics=microphysics, tracers=tracers, initialize=initialize)
    tc = bz.ThermodynamicConstants(saturation_vapor_pressure=bz.TetensFormula()) if kessler else bz.ThermodynamicConstants()
    ref = bz.ReferenceState(grid, tc, surface_pressure=1e5, potential_temperature=300.0)
    mp = {None: None, "SaturationAdjustment": bz.SaturationAdjustment(equilibrium=bz.WarmPhaseEquilibrium()),
          "Kessler": bz.DCMIP2016KesslerMicrophysics()}[microphysics]
    cl, kfields = _hip_closure(bz, grid, diff, plant_nan) if closure else (None, {})
    hm = bz.AtmosphereModel(grid, dynamics=bz.AnelasticDynamics(ref), advection=bz.WENO(order=5), thermodynamic_constants=tc,
                            formulation=formulation, microphysics=mp, tracers=TRACERS[:tracers], closure=cl)
    hm._k = kfields
    return om, hm


def _field_map(om, hm):
    """oracle prognostic name -> device Field"""
    out = {"ru": hm.momentum["ρu"], "rv": hm.momentum["ρv"], "rw": hm.momentum["ρw"], "rtheta": hm.potential_temperature_density,
           "rq": hm.moisture_density}
    if om.microphysics == "Kessler":
        out["rqcl"], out["rqr"] = hm.microphysical_fields["ρqᶜˡ"], hm.microphysical_fields["ρqʳ"]
    for t, n in enumerate(hm.tracers):
        out[f"rc{t}"] = hm.tracers[n]
    return out


def _push(om, hm, nan_halos=False):
    """oracle parents -> device parents, bit for bit (Float32 grids: rounded); nan_halos: NaN in every cell outside the interior"""
    import torch
    g = om.grid
    pairs = [(getattr(om, n), f) for n, f in _field_map(om, hm).items()]
    if om.microphysics == "Kessler":      # the temperature reads the diagnostic condensate of the previous update_state! (oracle.py: ql_lag)
        pairs += [(om.qcl, hm.microphysical_fields["qᶜˡ"]), (om.qr, hm.microphysical_fields["qʳ"])]
    for a, f in pairs:
        if nan_halos:
            b = np.full_like(a, np.nan)
            g.interior(b, f.zface)[...] = g.interior(a, f.zface)
            a = b
        f.parent.copy_(torch.from_numpy(np.ascontiguousarray(a)))


def _interiors(om, hm):
    g = om.grid
    return {n: (g.interior(getattr(om, n), f.zface), f.interior_cpu().astype(np.float64)) for n, f in _field_map(om, hm).items()}


def _random_prognostic(om, seed):
    """every prognostic array random on the interior (the wall faces of rho w too: the solve must not touch them)"""
    g, rng = om.grid, np.random.default_rng(seed)
    for n in om.PROGNOSTIC:
        a = getattr(om, n)
        a[...] = 0.0
        I = g.interior(a, n == "rw")
        I[...] = (300.0 if n == "rtheta" else 1.0) + rng.standard_normal(I.shape)


def _random_K(og, rng, Kmax, zeros=True):
    K = Kmax * rng.random((og.Nz, og.Ny, og.Nx))
    if zeros:
        K[rng.random(K.shape) < 0.2] = 0.0
    K.flat[rng.integers(K.size)] = Kmax
    return K


def _implicit_cases(og, rng, dtau):
    """name -> (Diffusivity, r): constant K, field K with zero cells and r up to 1e3, nu-only, kappa-only, K = 0"""
    big = 1e3 * _dzmin(og) ** 2 / dtau
    small = 0.4 * _dzmin(og) ** 2 / dtau
    return {
        "constant": (sdr.Diffusivity(1, True, nu=small, kappa=2 * small), 0.8),
        "constant_stiff": (sdr.Diffusivity(0, True, nu=big, kappa=big / 3), 1e3),
        "field": (sdr.Diffusivity(0, True, nu=_random_K(og, rng, big), kappa=_random_K(og, rng, big)), 1e3),
        "field_and_number": (sdr.Diffusivity(1, True, nu=_random_K(og, rng, small), kappa=small), 0.4),
        "nu_only": (sdr.Diffusivity(1, True, nu=small), 0.4),
        "kappa_only": (sdr.Diffusivity(1, True, kappa=_random_K(og, rng, small)), 0.4),
        "zero_field": (sdr.Diffusivity(0, True, nu=np.zeros((og.Nz, og.Ny, og.Nx)), kappa=np.zeros((og.Nz, og.Ny, og.Nx))), 0.0),
    }


def _round32(diff):
    """the same closure with Float32-representable coefficients (the Float32 twin's inputs)"""
    r = lambda K: K.astype(np.float32).astype(np.float64) if isinstance(K, np.ndarray) else float(np.float32(K))
    return sdr.Diffusivity(diff.formulation, diff.implicit, nu=r(diff.nu), kappa=r(diff.kappa))


def _check_implicit_step(oracle, bz, shape, stretched, halo, name, diff, r, microphysics=None, dtau=2.0, seed=0, float_type=np.float64):
    """One case of issue test 1.  NaN sits in every cell of the prognostic fields outside the interior while the solve runs: it never reads
    them.  The K fields are created NaN outside the interior too, but the library fills all of their halo layers before any kernel reads
    them, so for K the planting shows only that the fill runs, not that cells beyond the first halo cell are unread.
    Float32 grids (issue test 6): the same case with Float32-rounded inputs against the Float64 restatement; the bound of a solved field is
    four times the error of the restatement evaluated in numpy float32 on those inputs.  Returns the largest error / bound ratio."""
    f32 = float_type is np.float32
    if f32:
        diff = _round32(diff)
    om, hm = _pair(oracle, bz, shape, stretched, halo, diff, microphysics=microphysics, initialize=False, plant_nan=True, float_type=float_type)
    _random_prognostic(om, seed)
    if f32:
        for n in om.PROGNOSTIC:
            getattr(om, n)[...] = getattr(om, n).astype(np.float32)
    _push(om, hm, nan_halos=True)
    start = {n: a.copy() for n, (a, _) in _interiors(om, hm).items()}
    bz.compute_closure_fields_(hm)          # the K halo fill as a per-operator entry point
    bz.implicit_step_(hm, dtau)
    hm.synchronize()
    x32 = sdr.implicit_step(om, dtau, dtype=np.float32) if f32 else {}
    om.implicit_step(dtau)
    solved = (["ru", "rv", "rw"] if diff.on("nu") else []) + ([n for n in start if n not in ("ru", "rv", "rw")] if diff.on("kappa") else [])
    worst = 0.0
    for n, (want, got) in _interiors(om, hm).items():
        assert np.isfinite(got).all(), (name, n)
        err = np.abs(got - want).max()
        if f32 and n in x32:
            bound = 4 * np.abs(x32[n].astype(np.float64) - (want[1:-1] if n == "rw" else want)).max()
        else:
            bound = 32 * EPS * (1 + 4 * r) * np.abs(start[n]).max()
        print(f"IMPLICIT {'f32' if f32 else 'f64'} {shape} stretched={stretched} halo={halo} {name} {n}: err {err:.2e} bound {bound:.2e}")
        if n not in solved or name == "zero_field":
            assert np.array_equal(got, start[n]), (name, n)        # skipped fields and K = 0: bit-identical
        else:
            assert err <= bound, (name, n, err, bound)
            assert np.abs(want - start[n]).max() > 0, (name, n)
            worst = max(worst, err / bound)
        if n == "rw":
            assert np.array_equal(got[0], start[n][0]) and np.array_equal(got[-1], start[n][-1]), name      # wall faces never written
    return worst


@pytest.mark.parametrize("halo", [3, 5])
@pytest.mark.parametrize("stretched", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_implicit_step_matches_restatement(oracle, bz, shape, stretched, halo):
    og, _ = _grids(oracle, bz, shape, stretched, halo)
    for name, (diff, r) in _implicit_cases(og, np.random.default_rng(7), 2.0).items():
        _check_implicit_step(oracle, bz, shape, stretched, halo, name, diff, r)


def test_implicit_step_covers_the_kessler_species(oracle, bz):
    og, _ = _grids(oracle, bz, SHAPES[0], True, 3)
    cases = _implicit_cases(og, np.random.default_rng(8), 2.0)
    for name in ("constant", "field"):
        _check_implicit_step(oracle, bz, SHAPES[0], True, 3, name, *cases[name], microphysics="Kessler")


def test_closed_forms_on_the_device(oracle, bz):
    """The cosine eigenmode decays by 1 / (1 + K lambda dtau) per solve (1e-13); ten steps of VerticalScalarDiffusivity(vitd; nu) from
    the rest state rho u = cos(pi z / Lz) are a3^10 (1e-12), the scalars bit-identical."""
    Nz, nu, dt = 16, 10.0, 1.0
    g = bz.RectilinearGrid((8, 6, Nz), x=(0, 100.0), y=(0, 100.0), z=(0, 100.0))
    mode = np.cos(np.pi * (np.arange(Nz) + 0.5) / Nz)[:, None, None] + np.zeros((Nz, 6, 8))
    lam = (2 - 2 * np.cos(np.pi / Nz)) / (100.0 / Nz) ** 2

    def model():
        return bz.AtmosphereModel(g, advection=bz.WENO(order=5), closure=bz.VerticalScalarDiffusivity(bz.VerticallyImplicitTimeDiscretization(), ν=nu))
    m = model()
    m.momentum["ρu"].set_interior(mode)
    bz.implicit_step_(m, 3.0)
    got = m.momentum["ρu"].interior_cpu()
    want = mode / (1 + nu * lam * 3.0)
    assert np.abs(got - want).max() <= 1e-13 * np.abs(want).max()
    m = model()
    m.set(ρu=mode)
    rth0 = m.potential_temperature_density.interior_cpu().copy()
    for _ in range(10):
        m.time_step(dt)
    z = nu * lam * dt
    a1 = 1 / (1 + z)
    a2 = (0.75 + 0.25 * a1) / (1 + z / 4)
    a3 = (1 / 3 + 2 / 3 * a2) / (1 + 2 / 3 * z)
    assert np.abs(m.momentum["ρu"].interior_cpu() - a3 ** 10 * mode).max() <= 1e-12
    assert np.array_equal(m.potential_temperature_density.interior_cpu(), rth0)
    assert np.abs(m.moisture_density.interior_cpu()).max() == 0


def _turbulent_ic(om, seed, moist):
    g, rng = om.grid, np.random.default_rng(seed)
    sh = (g.Nz, g.Ny, g.Nx)
    x, y, z = g.nodes("ccc")
    Lz = g.zf[-1]
    ic = dict(theta=300.0 + 0.003 * z + 0.2 * rng.standard_normal(sh), u=-4.0 + 3.0 * z / Lz + 0.6 * rng.standard_normal(sh),
              v=0.6 * rng.standard_normal(sh))
    if g.Ny == 1:
        ic["v"] = 0.5 + 2.0 * z / Lz + 0.3 * np.sin(2 * np.pi * x / (g.Nx * g.dx)) + 0 * y
    if moist:
        ic["qt"] = 0.012 * np.exp(-z / 2200.0) * (1 + 0.02 * rng.standard_normal(sh))
    for t in range(om.n_tracers):
        ic[f"rc{t}"] = 1.0 + 0.5 * rng.random(sh)
    return ic


KINDS = {"isotropic_explicit": (0, False), "isotropic_implicit": (0, True), "vertical_explicit": (1, False), "vertical_implicit": (1, True)}


@pytest.mark.parametrize("moist", [False, True])
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("halo", [3, 5])
@pytest.mark.parametrize("stretched", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_closure_tendencies_match_restatement(oracle, bz, shape, stretched, halo, kind, moist):
    """The closure's part of bz_compute_tendencies — G with the closure minus G of the same model without (the advective bits cancel
    exactly on both sides) — to 1e-12 of its own scale, for field-valued nu and kappa, dry and with saturation adjustment."""
    og, _ = _grids(oracle, bz, shape, stretched, halo)
    rng = np.random.default_rng(11)
    diff = sdr.Diffusivity(*KINDS[kind], nu=_random_K(og, rng, 40.0), kappa=_random_K(og, rng, 60.0))
    mp = "SaturationAdjustment" if moist else None
    om, hm = _pair(oracle, bz, shape, stretched, halo, diff, microphysics=mp)
    om0, hm0 = _pair(oracle, bz, shape, stretched, halo, sdr.Diffusivity(), microphysics=mp, closure=False)
    om.set(**_turbulent_ic(om, 12, moist))
    for n in om.PROGNOSTIC:
        getattr(om0, n)[...] = getattr(om, n)
    om0.update_state()
    om.update_state()
    for o, h in ((om, hm), (om0, hm0)):
        _push(o, h)
        bz.update_state_(h, compute_tendencies=True)
        h.synchronize()
    g = om.grid
    names = {"ru": "ρu", "rv": "ρv", "rw": "ρw", "rtheta": "ρθ", "rq": "ρq", "rc0": "a", "rc1": "b"}
    for n, k in names.items():
        zf = n == "rw"
        want = g.interior(om.G[n], zface=zf) - g.interior(om0.G[n], zface=zf)
        got = hm.G[k].interior_cpu() - hm0.G[k].interior_cpu()
        scale = np.abs(want).max()
        print(f"TENDENCY {shape} {kind} moist={moist} {n}: scale {scale:.3e} err {np.abs(got - want).max():.3e}")
        if kind == "vertical_implicit" or (n == "rq" and not moist):
            assert scale == 0 and np.abs(got).max() == 0, n          # nothing explicit is left / no moisture to diffuse
        else:
            assert scale > 0, n
            assert np.abs(got - want).max() <= 1e-12 * scale, (n, np.abs(got - want).max() / scale)


def _three_steps(oracle, bz, monkeypatch, shape, stretched, halo, diff_of, dt=2.0, operators=False, rewrite=False, **kw):
    """(oracle model, device model) after three steps from the same state; rewrite: the host rewrites the K fields between steps"""
    if operators:
        monkeypatch.setenv("BZ_NO_FUSED", "1")
    else:
        monkeypatch.delenv("BZ_NO_FUSED", raising=False)
    og, _ = _grids(oracle, bz, shape, stretched, halo)
    diff = diff_of(og, np.random.default_rng(21))
    om, hm = _pair(oracle, bz, shape, stretched, halo, diff, **kw)
    ic = _turbulent_ic(om, 22, kw.get("microphysics") is not None)
    if kw.get("microphysics") == "Kessler":
        ic["qcl"], ic["qr"] = 1e-3 * np.ones((og.Nz, og.Ny, og.Nx)), 5e-4 * np.ones((og.Nz, og.Ny, og.Nx))
    om.set(**ic)
    _push(om, hm)
    bz.update_state_(hm, compute_tendencies=True)
    hm.profile_enable(True)
    rng = np.random.default_rng(23)
    for step in range(3):
        if rewrite and step:
            for name in ("nu", "kappa"):
                if name in hm._k:
                    K = _random_K(og, rng, 50.0)
                    setattr(diff, name, K)
                    hm._k[name].set_interior(K)
            om.update_state()                      # as after set!: the tendencies of the next stage see the new K
            bz.update_state_(hm, compute_tendencies=True)
        om.time_step(dt)
        hm.time_step(dt)
    hm.synchronize()
    return om, hm


def _assert_steps(label, om, hm, tol):
    pairs = _interiors(om, hm)
    mom = max(np.abs(pairs[n][0]).max() for n in ("ru", "rv", "rw"))
    for n, (want, got) in pairs.items():
        scale = mom if n in ("ru", "rv", "rw") else max(np.abs(want).max(), 1e-12)
        err = np.abs(got - want).max() / scale
        print(f"STEPS {label} {n}: {err:.2e}")
        assert err <= tol, (label, n, err)


STEP_CASES = {
    # formulation, microphysics, tracers, closure
    "theta_sa_tracer_isotropic_implicit_fields": (dict(microphysics="SaturationAdjustment", tracers=1),
                                                  lambda og, rng: sdr.Diffusivity(0, True, nu=_random_K(og, rng, 40.0), kappa=_random_K(og, rng, 60.0))),
    "theta_dry_vertical_implicit_numbers": (dict(tracers=0), lambda og, rng: sdr.Diffusivity(1, True, nu=30.0, kappa=45.0)),
    "theta_sa_isotropic_explicit_numbers": (dict(microphysics="SaturationAdjustment", tracers=1), lambda og, rng: sdr.Diffusivity(0, False, nu=20.0, kappa=30.0)),
    "energy_vertical_implicit_field_nu": (dict(formulation="StaticEnergy", tracers=1),
                                          lambda og, rng: sdr.Diffusivity(1, True, nu=_random_K(og, rng, 40.0), kappa=25.0)),
    "energy_isotropic_implicit_numbers": (dict(formulation="StaticEnergy", tracers=0), lambda og, rng: sdr.Diffusivity(0, True, nu=15.0, kappa=15.0)),
}


@pytest.mark.parametrize("case", list(STEP_CASES))
@pytest.mark.parametrize("stretched", [False, True])
def test_three_steps_match_restatement_on_every_tier(oracle, bz, monkeypatch, case, stretched):
    """(64, 8, 33), halo 3: the whole-step tier the model takes by itself (fused-RK for the theta model, fused for StaticEnergy) and the
    per-operator tier, each against the restatement to 1e-9 and against each other to 1e-12."""
    kw, diff_of = STEP_CASES[case]
    om, hm = _three_steps(oracle, bz, monkeypatch, SHAPES[1], stretched, 3, diff_of, **kw)
    _assert_steps(case + " whole-step tier", om, hm, 1e-9)
    om2, hm2 = _three_steps(oracle, bz, monkeypatch, SHAPES[1], stretched, 3, diff_of, operators=True, **kw)
    _assert_steps(case + " operators tier", om2, hm2, 1e-9)
    # the two runs took different tiers, and every stage ran one implicit launch
    whole, per_op = hm.profile(), hm2.profile()
    assert "make_pressure_correction" in per_op and "make_pressure_correction" not in whole, (sorted(whole), sorted(per_op))
    expected = 9 if diff_of(om.grid, np.random.default_rng(0)).implicit else 0
    assert whole.get("implicit_step", (0.0, 0))[1] == expected and per_op.get("implicit_step", (0.0, 0))[1] == expected
    a, b = _interiors(om, hm), _interiors(om2, hm2)
    mom = max(np.abs(a[n][1]).max() for n in ("ru", "rv", "rw"))
    for n in a:
        scale = mom if n in ("ru", "rv", "rw") else max(np.abs(a[n][1]).max(), 1e-12)
        assert np.abs(a[n][1] - b[n][1]).max() <= 1e-12 * scale, (n, np.abs(a[n][1] - b[n][1]).max() / scale)


@pytest.mark.parametrize("shape,stretched,halo", [(SHAPES[0], True, 3), (SHAPES[1], False, 5), (SHAPES[2], True, 5)])
def test_three_steps_on_ragged_flat_and_wide_halo_grids(oracle, bz, monkeypatch, shape, stretched, halo):
    kw, diff_of = STEP_CASES["theta_sa_tracer_isotropic_implicit_fields"]
    om, hm = _three_steps(oracle, bz, monkeypatch, shape, stretched, halo, diff_of, **kw)
    _assert_steps(f"{shape} halo {halo}", om, hm, 1e-9)


def test_three_steps_with_kessler(oracle, bz, monkeypatch):
    om, hm = _three_steps(oracle, bz, monkeypatch, SHAPES[0], False, 3, lambda og, rng: sdr.Diffusivity(0, True, nu=20.0, kappa=_random_K(og, rng, 30.0)),
                          microphysics="Kessler", tracers=0)
    _assert_steps("kessler", om, hm, 1e-9)


@pytest.mark.parametrize("operators", [False, True])
def test_field_diffusivity_rewritten_between_steps(oracle, bz, monkeypatch, operators):
    """The host rewrites nu and kappa between steps (interior only): the library refreshes their halos itself."""
    kw, diff_of = STEP_CASES["theta_sa_tracer_isotropic_implicit_fields"]
    om, hm = _three_steps(oracle, bz, monkeypatch, SHAPES[1], True, 3, diff_of, operators=operators, rewrite=True, **kw)
    _assert_steps("rewritten K", om, hm, 1e-9)


# ---- the reference's own tests on the device --------------------------------------------------------------------------------------------
def _device_decay(bz, closure, dt, nt, tracer=False, momentum=False):
    g = bz.RectilinearGrid((4, 4, 32), x=(0, 100.0), y=(0, 100.0), z=(0, 100.0))
    m = bz.AtmosphereModel(g, advection=bz.WENO(order=5), closure=closure, tracers=("c",) if tracer else ())
    cosine = np.cos(np.pi * g.zᶜ / 100.0)[:, None, None] + np.zeros((32, 4, 4))
    if tracer:
        m.tracers["c"].set_interior(cosine)
    if momentum:
        m.set(ρu=cosine)
    else:
        bz.update_state_(m)
    for _ in range(nt):
        m.time_step(dt)
    decay = lambda f: np.sqrt(np.sum(f.interior_cpu() ** 2) / np.sum(cosine ** 2))
    return (decay(m.tracers["c"]) if tracer else None), (decay(m.momentum["ρu"]) if momentum else None)


def test_reference_vertical_diffusion_known_answers_on_the_device(bz):
    """test/vertical_diffusion.jl:24-138 (from a rest state): rtol 0.05 of exp(-K (pi / Lz)^2 t), implicit against explicit rtol 0.01."""
    V, vitd, etd = bz.VerticalScalarDiffusivity, bz.VerticallyImplicitTimeDiscretization(), bz.ExplicitTimeDiscretization()
    exact = lambda K, t: np.exp(-K * (np.pi / 100.0) ** 2 * t)
    c, _ = _device_decay(bz, V(vitd, κ=10.0), 1.0, 10, tracer=True)
    assert abs(c - exact(10.0, 10.0)) <= 0.05 * exact(10.0, 10.0)
    ci, _ = _device_decay(bz, V(vitd, κ=1.0), 0.5, 10, tracer=True)
    ce, _ = _device_decay(bz, V(etd, κ=1.0), 0.5, 10, tracer=True)
    assert abs(ci - exact(1.0, 5.0)) <= 0.05 * exact(1.0, 5.0) and abs(ce - exact(1.0, 5.0)) <= 0.05 * exact(1.0, 5.0)
    assert abs(ci - ce) <= 0.01 * max(ci, ce)
    _, u = _device_decay(bz, V(vitd, ν=10.0), 1.0, 10, momentum=True)
    assert abs(u - exact(10.0, 10.0)) <= 0.05 * exact(10.0, 10.0)
    c, u = _device_decay(bz, V(vitd, ν=5.0, κ=10.0), 1.0, 10, tracer=True, momentum=True)
    assert abs(u - exact(5.0, 10.0)) <= 0.05 * exact(5.0, 10.0) and abs(c - exact(10.0, 10.0)) <= 0.05 * exact(10.0, 10.0)


def test_reference_closure_list_steps(bz):
    """test/turbulence_closures.jl:14-28: one time_step! with each of the two diffusivity entries, the constructor's defaults otherwise."""
    g = bz.RectilinearGrid((8, 8, 8), x=(0, 100.0), y=(0, 100.0), z=(0, 100.0))
    for closure in (bz.ScalarDiffusivity(ν=1, κ=2), bz.ScalarDiffusivity(bz.VerticallyImplicitTimeDiscretization(), ν=1)):
        m = bz.AtmosphereModel(g, closure=closure)
        m.time_step(1)
        m.synchronize()
        assert m.closure_fields == {}
        assert all(np.isfinite(f.interior_cpu()).all() for f in m.prognostic_fields().values())


@pytest.mark.parametrize("formulation", ["StaticEnergy", "LiquidIcePotentialTemperature"])
@pytest.mark.parametrize("implicit", [True, False])
def test_uniform_energy_is_not_diffused_on_the_device(bz, implicit, formulation):
    """test/turbulence_closures.jl:38-50: uniform e, ScalarDiffusivity(disc, nu = 1, kappa = 1), one step: the thermodynamic density
    within rtol 1e-5 (2-norms); explicit: bit-identical to the step with kappa = 0 (the fluxes of a uniform e are exact zeros)."""
    g = bz.RectilinearGrid((8, 8, 8), x=(0, 100.0), y=(0, 100.0), z=(0, 100.0))
    disc = bz.VerticallyImplicitTimeDiscretization() if implicit else bz.ExplicitTimeDiscretization()

    def run(kappa):
        m = bz.AtmosphereModel(g, advection=bz.WENO(order=5), formulation=formulation, closure=bz.ScalarDiffusivity(disc, ν=1, κ=kappa), tracers=("c",))
        if formulation == "StaticEnergy":
            m.set(e=m.thermodynamic_constants.dry_air_heat_capacity * m.dynamics.reference_state.potential_temperature)
        a = m.energy_density.interior_cpu().copy()
        m.time_step(1.0)
        return a, m.energy_density.interior_cpu().copy()
    a, b = run(1.0)
    assert np.linalg.norm(b - a) <= 1e-5 * max(np.linalg.norm(a), np.linalg.norm(b))
    if not implicit:
        assert np.array_equal(b, run(0.0)[1])


# ---- Float32 twin --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("halo", [3, 5])
@pytest.mark.parametrize("stretched", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_float32_implicit_step_within_four_times_the_restatements_float32_error(oracle, bz, shape, stretched, halo):
    """Every case of test_implicit_step_matches_restatement on Float32 grids (stiff rows, nu-only, kappa-only, K = 0, wall faces, NaN
    planting): the Float32 library against the Float64 restatement fed the Float32-rounded inputs; the bound is four times the error of
    the same restatement evaluated in numpy float32 on those inputs (measured here from the restatement, never from the device)."""
    og, _ = _grids(oracle, bz, shape, stretched, halo)
    worst = {}
    for name, (diff, r) in _implicit_cases(og, np.random.default_rng(7), 2.0).items():
        worst[name] = _check_implicit_step(oracle, bz, shape, stretched, halo, name, diff, r, float_type=np.float32)
    print(f"F32 RATIO {shape} stretched={stretched} halo={halo}: largest device error / numpy-float32 error "
          + " ".join(f"{k}={4 * v:.2f}" for k, v in worst.items()))


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_refused_combinations_name_the_option_and_leave_the_context_usable(bz):
    import ctypes as C
    from breeze_jl_amd import _lib
    V, vitd = bz.VerticalScalarDiffusivity, bz.VerticallyImplicitTimeDiscretization()
    g = bz.RectilinearGrid((16, 8, 8), x=(0, 100.0), y=(0, 100.0), z=(0, 100.0))
    for bad, word in ((lambda: bz.ScalarDiffusivity(κ={"c": 1.0}), "per-tracer"), (lambda: bz.ScalarDiffusivity(ν=lambda x, y, z, t: 1.0), "function"),
                      (lambda: bz.HorizontalScalarDiffusivity(ν=1.0), "HorizontalScalarDiffusivity"),
                      (lambda: bz.SmagorinskyLilly(vitd), "SmagorinskyLilly"),
                      (lambda: bz.AtmosphereModel(g, advection=bz.WENO(order=5), closure=(bz.ScalarDiffusivity(ν=1.0), bz.SmagorinskyLilly())), "tuple"),
                      (lambda: bz.AtmosphereModel(bz.RectilinearGrid((16, 8, 8), x=(0, 100.0), y=(0, 100.0), z=(0, 100.0), topology=(bz.Periodic, bz.Bounded, bz.Bounded)),
                                                  advection=bz.WENO(order=5), closure=V(vitd, ν=1.0)), "walls"),
                      (lambda: bz.AtmosphereModel(bz.RectilinearGrid((16, 8), x=(0, 100.0), z=(0, 100.0), topology=(bz.Bounded, bz.Flat, bz.Bounded)),
                                                  advection=bz.WENO(order=5), closure=V(vitd, ν=1.0)), "walls"),
                      (lambda: bz.AtmosphereModel(g, dynamics=bz.PrescribedDynamics(bz.ReferenceState(g)), advection=bz.WENO(order=5), closure=V(vitd, κ=1.0)),
                       "closure"),
                      (lambda: bz.CompressibleAtmosphereModel(g, bz.CompressibleDynamics(bz.SplitExplicitTimeDiscretization()), advection=bz.WENO(order=5),
                                                              closure=V(vitd, κ=1.0)), "closure")):
        with pytest.raises(NotImplementedError) as e:
            bad()
        assert word in str(e.value), (word, str(e.value))
    # C ABI: mutually exclusive with bz_set_closure, in both orders; the context steps afterwards
    m = bz.AtmosphereModel(g, advection=bz.WENO(order=5), closure=V(vitd, ν=2.0, κ=3.0))
    nu_e = bz.Field(g, (bz.Center, bz.Center, bz.Center), "cuda:0")
    sl = _lib.bz_smagorinsky_lilly(0.16, 1.0, 1.0)
    assert m._lib.bz_set_closure(m._ctx, C.byref(sl), C.c_void_p(nu_e.ptr())) == 2
    assert b"ScalarDiffusivity" in m._lib.bz_last_error(m._ctx)
    m.time_step(1.0)
    m2 = bz.AtmosphereModel(g, advection=bz.WENO(order=5), closure=bz.SmagorinskyLilly())
    sd = _lib.bz_scalar_diffusivity(1, 1, 1.0, 1.0)
    assert m2._lib.bz_set_scalar_diffusivity(m2._ctx, C.byref(sd), None, None) == 2
    assert b"SmagorinskyLilly" in m2._lib.bz_last_error(m2._ctx)
    m2.time_step(1.0)
    m2.synchronize()
    # compressible and kinematic contexts refuse the attachment by name
    cm = bz.CompressibleAtmosphereModel(g, bz.CompressibleDynamics(bz.SplitExplicitTimeDiscretization()), advection=bz.WENO(order=5))
    assert cm._lib.bz_set_scalar_diffusivity(cm._ctx, C.byref(sd), None, None) == 2
    assert b"compressible" in cm._lib.bz_last_error(cm._ctx)
    km = bz.AtmosphereModel(g, dynamics=bz.PrescribedDynamics(bz.ReferenceState(g)), advection=bz.WENO(order=5))
    assert km._lib.bz_set_scalar_diffusivity(km._ctx, C.byref(sd), None, None) == 2
    assert b"kinematic" in km._lib.bz_last_error(km._ctx)
    assert all(np.isfinite(f.interior_cpu()).all() for f in m.prognostic_fields().values())
    # negative and NaN coefficients
    for bad_sd in (_lib.bz_scalar_diffusivity(0, 1, -1.0, 1.0), _lib.bz_scalar_diffusivity(0, 0, 1.0, float("nan"))):
        m3 = bz.AtmosphereModel(g, advection=bz.WENO(order=5))
        assert m3._lib.bz_set_scalar_diffusivity(m3._ctx, C.byref(bad_sd), None, None) == 2
        assert b"negative" in m3._lib.bz_last_error(m3._ctx)
    m3.time_step(1.0)


def test_slab_and_walled_contexts_refuse_the_closure_by_name_and_still_step(bz):
    """y-slab models in Python and through the ABI, walls in y and in x through the ABI: each names the option, and the context steps."""
    import ctypes as C
    import uuid
    from breeze_jl_amd import _lib
    from breeze_jl_amd import distributed as bz_dist
    V, vitd = bz.VerticalScalarDiffusivity, bz.VerticallyImplicitTimeDiscretization()
    sd = _lib.bz_scalar_diffusivity(1, 1, 1.0, 1.0)
    G = bz.RectilinearGrid((32, 16, 12), x=(0, 3200.0), y=(0, 1600.0), z=(0, 1200.0))

    def slab(**kw):
        return bz_dist.LibrarySlabAtmosphereModel(G, 0, 1, transport="local:" + uuid.uuid4().hex, device="cuda:0", potential_temperature=300.0,
                                                  advection=bz.WENO(), **kw)
    with pytest.raises(NotImplementedError) as e:
        slab(closure=V(vitd, ν=1.0))
    assert "slab" in str(e.value)
    models = [(slab(), b"slab"),
              (bz.AtmosphereModel(bz.RectilinearGrid((16, 8, 8), x=(0, 100.0), y=(0, 100.0), z=(0, 100.0), topology=(bz.Periodic, bz.Bounded, bz.Bounded)),
                                  advection=bz.WENO(order=5)), b"walls"),
              (bz.AtmosphereModel(bz.RectilinearGrid((16, 8), x=(0, 100.0), z=(0, 100.0), topology=(bz.Bounded, bz.Flat, bz.Bounded)),
                                  advection=bz.WENO(order=5)), b"walls")]
    for m, word in models:
        assert m._lib.bz_set_scalar_diffusivity(m._ctx, C.byref(sd), None, None) == 2
        assert word in m._lib.bz_last_error(m._ctx), m._lib.bz_last_error(m._ctx)
        m.time_steps(1.0, 1)
        m.synchronize()
        assert all(np.isfinite(f.interior_cpu()).all() for f in m.prognostic_fields().values())


# ---- hipGraph ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field_K", [False, True])
def test_graph_replay_with_the_closure_is_bit_identical(oracle, bz, field_K):
    def run(graph):
        g = bz.RectilinearGrid((32, 16, 16), x=(-4e3, 4e3), y=(-2e3, 2e3), z=(0.0, 4e3))
        if field_K:
            K = bz.Field(g, (bz.Center, bz.Center, bz.Center), "cuda:0")
            K.set_interior(lambda x, y, z: 20.0 + 10.0 * np.sin(2 * np.pi * x / 8e3) * np.cos(np.pi * z / 4e3) + 0 * y)
        else:
            K = 25.0
        m = bz.AtmosphereModel(g, dynamics=bz.AnelasticDynamics(bz.ReferenceState(g, potential_temperature=300.0)), advection=bz.WENO(order=5),
                               closure=bz.ScalarDiffusivity(bz.VerticallyImplicitTimeDiscretization(), ν=K, κ=K), tracers=("c",))
        from helpers import bubble_theta
        m.tracers["c"].set_interior(lambda x, y, z: 1.0 + np.exp(-z / 1e3) + 0 * x + 0 * y)
        m.set(θ=bubble_theta(300.0, 9.81, r0=1.5e3, zc=1500.0), u=3.0)
        m.graph_enable(graph)
        for _ in range(6):
            m.time_step(2.0)
        m.synchronize()
        return {k: f.interior_cpu().copy() for k, f in m.prognostic_fields().items()}, m.graph_info()
    a, info = run(True)
    b, _ = run(False)
    assert info[0] and info[1] == 1 and info[2] >= 4, info
    for k in a:
        assert np.isfinite(a[k]).all() and np.array_equal(a[k], b[k]), k
