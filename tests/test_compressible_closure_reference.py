"""Pins of tests/compressible_closure_reference.py, the CPU restatement of the turbulence closures on the compressible split-explicit
model (Oceananigans' side is not vendored: parity unpinned): the anelastic restatements (oracle/closure.py,
tests/scalar_diffusivity_reference.py) on a state whose rho_d is the reference column and whose pressure is the reference pressure, closed
forms, conservation, and the reference's own known answers that need no Oceananigans (test/turbulence_closures.jl:52-67).  No GPU."""
import numpy as np
import pytest

import compressible_closure_reference as ccr
import scalar_diffusivity_reference as sdr
from oracle import oracle as orc
from oracle.closure import SmagorinskyLilly, add_closure_tendencies

SIZE = (10, 6, 12)      # Nx, Ny, Nz


def _z(Nz, Lz, stretched):
    if not stretched:
        return (0.0, Lz)
    s = np.linspace(0.0, 1.0, Nz + 1)
    return Lz * (0.35 * s + 0.65 * s ** 2)


def _grid(stretched=False, size=SIZE, L=(800.0, 500.0, 1200.0)):
    return orc.Grid(size, x=(0.0, L[0]), y=(0.0, L[1]), z=_z(size[2], L[2], stretched))


def _fill(m, **fields):
    """interior arrays into the model's parent arrays, halos filled the way update_state! fills them"""
    g = m.grid
    for name, a in fields.items():
        f, zf = getattr(m, name), name in ("w", "rw")
        g.interior(f, zf)[...] = a
        (m._halo_w if zf else m._halo_center)(f)


def _random_anelastic(g, seed, closure=None, diffusivity=None):
    """an anelastic restatement with a random dry state; returns the model after update_state"""
    kw = dict(surface_pressure=101325.0, potential_temperature=300.0)
    am = orc.OracleModel(g, closure=closure, **kw) if diffusivity is None else sdr.DiffusivityModel(g, diffusivity, **kw)
    rng = np.random.default_rng(seed)
    sh = (g.Nz, g.Ny, g.Nx)
    z = g.nodes("ccc")[2]
    am.set(theta=300.0 + 0.004 * z + 0.3 * rng.standard_normal(sh), ru=rng.standard_normal(sh), rv=rng.standard_normal(sh),
           rw=0.3 * rng.standard_normal((g.Nz + 1, g.Ny, g.Nx)), enforce_mass_conservation=False)
    am.update_state()
    return am


def _compressible_twin(am, **kw):
    """the compressible restatement on the anelastic model's u, v, w, T, theta with rho_d(x, y, z) = rho_r(z) and p = p_r(z), dry"""
    g = am.grid
    cm = ccr.ClosureCompressibleModel(g, **kw)
    Hz, Nz = g.Hz, g.Nz
    col = lambda a: np.broadcast_to(a[Hz:Hz + Nz][:, None, None], (Nz, g.Ny, g.Nx))
    I = g.interior
    _fill(cm, rho_d=col(am.ref.density), rho=col(am.ref.density), p=col(am.ref.pressure), u=I(am.u), v=I(am.v), w=I(am.w, True),
          T=I(am.T), theta=I(am.theta), q=0.0 * I(am.T))
    return cm


@pytest.mark.parametrize("stretched", [False, True])
def test_smagorinsky_reduces_to_the_anelastic_restatement(stretched):
    """nu_e to 1e-13 of its maximum on levels 1 .. Nz-2 (the outer two differ by design: the anelastic column extends p_r hydrostatically
    into its halo, the compressible pressure has a zero-gradient halo); the five tendencies to 1e-13 of their scale on levels 2 .. Nz-3."""
    g = _grid(stretched)
    am = _random_anelastic(g, 3, closure=SmagorinskyLilly())
    cm = _compressible_twin(am, closure=SmagorinskyLilly())
    cm.compute_closure_fields()
    assert am.nu_e.max() > 0
    assert np.abs(cm.nu_e - am.nu_e)[1:-1].max() <= 1e-13 * am.nu_e.max()
    assert np.abs(cm.nu_e - am.nu_e)[[0, -1]].max() > 1e-6 * am.nu_e.max()      # ... and they do differ there
    # a passive moisture field for the fifth tendency (nu_e above was formed dry)
    q = 0.01 * np.random.default_rng(4).random((g.Nz, g.Ny, g.Nx))
    _fill(am, q=q)
    _fill(cm, q=q)
    for n in am.G:
        am.G[n][...] = 0.0
    add_closure_tendencies(am)
    got = dict(cm.slow_closure_terms(), **cm.water_closure_terms())
    for n in ("ru", "rv", "rtheta", "rq"):
        want = -g.interior(am.G[n])
        assert np.abs(want).max() > 0, n
        assert np.abs(got[n] - want)[2:-2].max() <= 1e-13 * np.abs(want).max(), n
    want = -g.interior(am.G["rw"], True)[1:g.Nz]          # faces 1 .. Nz-1
    assert np.abs(got["rw"] - want)[2:-2].max() <= 1e-13 * np.abs(want).max()


@pytest.mark.parametrize("formulation", [0, 1])
def test_constant_diffusivity_reduces_to_the_anelastic_restatement(formulation):
    g = _grid(True)
    d = sdr.Diffusivity(formulation, False, nu=3.0, kappa=2.0)
    am = _random_anelastic(g, 5, diffusivity=d)
    cm = _compressible_twin(am, diffusivity=d)
    q = 0.01 * np.random.default_rng(6).random((g.Nz, g.Ny, g.Nx))
    _fill(am, q=q)
    _fill(cm, q=q)
    for n in am.G:
        am.G[n][...] = 0.0
    sdr.add_diffusivity_tendencies(am)
    got = dict(cm.slow_closure_terms(), **cm.water_closure_terms())
    for n in ("ru", "rv", "rtheta", "rq"):
        want = -g.interior(am.G[n])
        assert np.abs(want).max() > 0, n
        assert np.abs(got[n] - want)[2:-2].max() <= 1e-13 * np.abs(want).max(), n
    want = -g.interior(am.G["rw"], True)[1:g.Nz]
    assert np.abs(got["rw"] - want)[2:-2].max() <= 1e-13 * np.abs(want).max()


def test_pure_shear_gives_the_textbook_viscosity():
    """u = S z in neutral stratification: Sigma^2 = S^2 / 2, so nu_e = (C Delta)^2 S away from the walls (tests/test_closure.py:16-34 has the
    form).  theta_v is uniform to rounding, so the stability factor is 1 to ~1e-13 / Sigma^2."""
    g = orc.Grid((8, 8, 8), x=(0, 100.0), y=(0, 100.0), z=(0, 100.0))
    cm = ccr.ClosureCompressibleModel(g, closure=SmagorinskyLilly())
    S = 0.02
    cm.set(rho=1.0, theta=300.0, u=lambda x, y, z: S * z + 0 * x + 0 * y, v=0.0, w=0.0)
    want = (0.16 * 12.5) ** 2 * S
    assert np.abs(cm.nu_e[1:-1] - want).max() <= 1e-9 * want
    assert np.all(cm.nu_e[-1] < cm.nu_e[-2])      # the wall face carries no strain


def test_constant_viscosity_with_density_varying_in_x_is_the_hand_written_operator():
    """G_rho_theta loses -dx(Ix(rho_d) kappa dx theta) / dx^2, written out with rolls"""
    g = _grid(False)
    kappa = 7.0
    cm = ccr.ClosureCompressibleModel(g, diffusivity=sdr.Diffusivity(0, False, nu=0.0, kappa=kappa))
    rng = np.random.default_rng(8)
    rho = np.broadcast_to(1.0 + 0.2 * (2 * rng.random(g.Nx) - 1), (g.Nz, g.Ny, g.Nx))
    th = np.broadcast_to(300.0 + rng.standard_normal(g.Nx), (g.Nz, g.Ny, g.Nx))
    _fill(cm, rho_d=rho, theta=th)
    rho_f = (np.roll(rho, 1, axis=2) + rho) / 2                     # face i, between cells i-1 and i
    flux = rho_f * (-kappa * ((th - np.roll(th, 1, axis=2)) / g.dx))
    want = (np.roll(flux, -1, axis=2) - flux) / g.dx
    got = cm.slow_closure_terms()["rtheta"]
    assert "ru" not in cm.slow_closure_terms()                       # nu = 0: no momentum terms at all
    assert np.abs(want).max() > 0
    assert np.abs(got - want).max() <= 1e-14 * np.abs(want).max()


@pytest.mark.parametrize("which", ["smagorinsky", "isotropic", "vertical"])
def test_uniform_theta_has_an_exactly_zero_closure_tendency(which):
    g = _grid(True)
    rng = np.random.default_rng(9)
    sh = (g.Nz, g.Ny, g.Nx)
    kw = dict(closure=SmagorinskyLilly()) if which == "smagorinsky" else \
        dict(diffusivity=sdr.Diffusivity(which == "vertical", False, nu=1.0, kappa=5.0 * rng.random(sh)))
    cm = ccr.ClosureCompressibleModel(g, **kw)
    _fill(cm, rho_d=1.0 + 0.2 * (2 * rng.random(sh) - 1), theta=np.full(sh, 301.5), u=rng.standard_normal(sh), v=rng.standard_normal(sh))
    cm.nu_e = rng.random(sh)
    assert np.all(cm.slow_closure_terms()["rtheta"] == 0.0)


@pytest.mark.parametrize("which", ["smagorinsky", "isotropic", "vertical"])
def test_closure_terms_conserve(which):
    """Flux form, periodic sides, stress-free / no-flux walls: the volume sums of the closure terms of rho u, rho v, rho theta, rho q,
    rho q^cl, rho q^r vanish to 1e-12 of the sum of absolute values, with random rho_d and rho within 20 % of 1."""
    g = _grid(True)
    rng = np.random.default_rng(10)
    sh = (g.Nz, g.Ny, g.Nx)
    kw = dict(closure=SmagorinskyLilly()) if which == "smagorinsky" else \
        dict(diffusivity=sdr.Diffusivity(which == "vertical", False, nu=4.0 * rng.random(sh), kappa=5.0 * rng.random(sh)))
    cm = ccr.ClosureCompressibleModel(g, microphysics="Kessler", **kw)
    rnd = lambda: 1.0 + 0.2 * (2 * rng.random(sh) - 1)
    _fill(cm, rho_d=rnd(), rho=rnd(), theta=300.0 + rng.standard_normal(sh), q=0.01 * rng.random(sh), qcl=1e-3 * rng.random(sh),
          qr=1e-3 * rng.random(sh), u=rng.standard_normal(sh), v=rng.standard_normal(sh), w=rng.standard_normal((g.Nz + 1,) + sh[1:]))
    cm.nu_e = rng.random(sh)
    terms = dict(cm.slow_closure_terms(), **cm.water_closure_terms())
    dz = g.dzc[g.Hz:g.Hz + g.Nz][:, None, None]
    for n in ("ru", "rv", "rtheta", "rq", "rqcl", "rqr"):
        t = terms[n] * dz
        assert np.abs(t).sum() > 0, n
        assert abs(t.sum()) <= 1e-12 * np.abs(t).sum(), n
    assert np.abs(terms["rw"]).max() > 0


def test_reference_known_answers():
    """test/turbulence_closures.jl:52-59: nu = 1e4 moves G_rho_u of a Gaussian jet; :61-67: shear gives nu_e > 0"""
    g = orc.Grid((8, 8, 8), x=(0, 100.0), y=(0, 100.0), z=(0, 100.0))
    cm = ccr.ClosureCompressibleModel(g, diffusivity=sdr.Diffusivity(0, False, nu=1e4, kappa=0.0))
    cm.set(rho=1.0, theta=300.0, u=lambda x, y, z: np.exp(-(z - 50.0) ** 2 / (2 * 20.0 ** 2)) + 0 * x + 0 * y, v=0.0, w=0.0)
    base = ccr.ClosureCompressibleModel(g)
    base.set(rho=1.0, theta=300.0, u=lambda x, y, z: np.exp(-(z - 50.0) ** 2 / (2 * 20.0 ** 2)) + 0 * x + 0 * y, v=0.0, w=0.0)
    cm.compute_slow_tendencies()
    base.compute_slow_tendencies()
    assert np.abs(g.interior(cm.G["ru"]) - g.interior(base.G["ru"])).max() > 0
    assert np.array_equal(cm.G["rho_d"], base.G["rho_d"])          # G_rho_d gets nothing
    sm = ccr.ClosureCompressibleModel(g, closure=SmagorinskyLilly())
    sm.set(rho=1.0, theta=300.0, u=lambda x, y, z: z / 100 + 0 * x + 0 * y, v=0.0, w=0.0)
    assert sm.nu_e.max() > 0


def test_host_refuses_what_is_not_built_by_name(bz):
    """NotImplementedError before any device call, naming the option"""
    V, S, I = bz.VerticalScalarDiffusivity, bz.ScalarDiffusivity, bz.VerticallyImplicitTimeDiscretization
    ext = dict(x=(0, 1600.0), y=(0, 1600.0), z=(0, 800.0))
    grid = bz.RectilinearGrid((16, 16, 8), **ext)
    dyn = lambda: bz.CompressibleDynamics(bz.SplitExplicitTimeDiscretization(substeps=6), reference_potential_temperature=300.0)
    model = lambda g=grid, **kw: bz.CompressibleAtmosphereModel(g, dyn(), advection=bz.WENO(order=5), **kw)
    cases = [(lambda: model(closure=S(I(), ν=1.0)), "VerticallyImplicitTimeDiscretization"),
             (lambda: model(closure=V(I(), κ=1.0)), "VerticallyImplicitTimeDiscretization"),
             (lambda: model(closure=bz.HorizontalScalarDiffusivity(ν=1.0)), "HorizontalScalarDiffusivity"),
             (lambda: model(closure=bz.DynamicSmagorinsky()), "DynamicSmagorinsky"),
             (lambda: model(closure=bz.AnisotropicMinimumDissipation()), "AnisotropicMinimumDissipation"),
             (lambda: model(closure=(bz.SmagorinskyLilly(), S(ν=1.0))), "tuples"),
             (lambda: model(closure=S(κ={"ρθ": 1.0})), "per-tracer"),
             (lambda: model(closure=S(ν=lambda x, y, z, t: 1.0)), "function"),
             (lambda: model(bz.RectilinearGrid((16, 16, 8), topology=(bz.Periodic, bz.Bounded, bz.Bounded), **ext), closure=bz.SmagorinskyLilly()), "Bounded"),
             (lambda: model(bz.RectilinearGrid((16, 8), topology=(bz.Periodic, bz.Flat, bz.Bounded), x=ext["x"], z=ext["z"]), closure=S(ν=1.0)), "Flat"),
             (lambda: bz.compressible.SlabCompressibleModel(grid, 0, 2, dyn(), advection=bz.WENO(order=5), closure=bz.SmagorinskyLilly(), device="cpu",
                                               decomp=object()), "slab")]
    for make, word in cases:
        with pytest.raises(NotImplementedError) as e:
            make()
        assert word in str(e.value), (word, str(e.value))


@pytest.mark.parametrize("which", ["smagorinsky", "isotropic", "vertical"])
def test_float32_view_evaluates_in_float32_and_stays_close(which):
    """in_dtype(model, float32): every closure term comes back as float32 and within 1e-4 of the Float64 term's maximum (a few hundred
    float32 roundings of O(1) differences; a formula left in Float64 would return float64, one evaluated wrongly would miss by far more)"""
    g = _grid(True)
    rng = np.random.default_rng(12)
    sh = (g.Nz, g.Ny, g.Nx)
    kw = dict(closure=SmagorinskyLilly()) if which == "smagorinsky" else \
        dict(diffusivity=sdr.Diffusivity(which == "vertical", False, nu=4.0 * rng.random(sh), kappa=7.0))
    cm = ccr.ClosureCompressibleModel(g, **kw)
    rnd = lambda: 1.0 + 0.2 * (2 * rng.random(sh) - 1)
    _fill(cm, rho_d=rnd(), rho=rnd(), theta=300.0 + rng.standard_normal(sh), q=0.01 * rng.random(sh), u=rng.standard_normal(sh),
          v=rng.standard_normal(sh), w=rng.standard_normal((g.Nz + 1,) + sh[1:]), T=290.0 + rng.standard_normal(sh), p=9e4 * rnd())
    cm.compute_closure_fields()
    v = ccr.in_dtype(cm, np.float32)
    want = dict(cm.slow_closure_terms(), **cm.water_closure_terms())
    got = dict(v.slow_closure_terms(), **v.water_closure_terms())
    for n in want:
        assert got[n].dtype == np.float32, n
        assert np.abs(got[n] - want[n]).max() <= 1e-4 * np.abs(want[n]).max(), n
    if which == "smagorinsky":
        assert ccr.eddy_viscosity(v).dtype == np.float32
