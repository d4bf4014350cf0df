"""Pins of tests/scalar_diffusivity_reference.py, the CPU restatement of ScalarDiffusivity / VerticalScalarDiffusivity with explicit and
vertically implicit time discretisation (Oceananigans' side is not vendored: parity unpinned): numpy.linalg.solve, exact closed forms
and the reference's own known answers (test/vertical_diffusion.jl:24-138, test/turbulence_closures.jl:38-50).  No GPU."""
import numpy as np
import pytest

import scalar_diffusivity_reference as sdr

EPS = np.finfo(np.float64).eps


def _z_faces(Nz, Lz, stretched):
    if not stretched:
        return (0.0, Lz)
    s = np.linspace(0.0, 1.0, Nz + 1)
    return Lz * (0.35 * s + 0.65 * s ** 2)      # spacing grows about five-fold from the surface to the top


def _spacings(Nz, Lz, stretched):
    g = sdr.orc.Grid((4, 4, Nz), x=(0, 100.0), y=(0, 100.0), z=_z_faces(Nz, Lz, stretched))
    return g.dzc[g.Hz:g.Hz + Nz].copy(), g.dzf[g.Hz:g.Hz + Nz + 1].copy()


@pytest.mark.parametrize("stretched", [False, True])
@pytest.mark.parametrize("kind", ["constant", "random"])
@pytest.mark.parametrize("rows", ["centre", "face"])
def test_thomas_solve_matches_dense_solve(stretched, kind, rows):
    """Within 32 eps (1 + 4 r) max|phi|, r = max dtau K / min(dz)^2: the forward error of an unpivoted solve of a row-diagonally-dominant
    matrix (||A^-1||_inf <= 1, ||A||_inf <= 1 + 4 r).  r <= 1e3 in every case, so the bound never exceeds 1e-9 max|phi|."""
    Nz, ncol = 33, 12
    dzc, dzf = _spacings(Nz, 100.0, stretched)
    rng = np.random.default_rng(3 + 2 * stretched + (kind == "random"))
    dzmin = min(dzc.min(), dzf[1:Nz].min())
    for target_r in (0.3, 1e3):
        dtau = 2.0
        Kmax = target_r * dzmin ** 2 / dtau
        nK = Nz + 1 if rows == "centre" else Nz
        if kind == "constant":
            K = np.full((nK, ncol), Kmax)
        else:
            K = Kmax * rng.random((nK, ncol))
            K[rng.random((nK, ncol)) < 0.2] = 0.0          # zero cells: identity couplings inside the column
            K[nK // 2, 0] = Kmax
        r = dtau * K.max() / dzmin ** 2
        assert r <= 1e3 * (1 + 1e-12)
        lower, diag, upper = (sdr.centre_rows if rows == "centre" else sdr.face_rows)(dzc, dzf, K, dtau)
        phi = rng.standard_normal((diag.shape[0], ncol))
        x = sdr.thomas(lower, diag, upper, phi)
        bound = 32 * EPS * (1 + 4 * r) * np.abs(phi).max()
        assert bound <= 1e-9 * np.abs(phi).max()
        for c in range(ncol):
            A = sdr.dense_rows(lower[:, c], diag[:, c], upper[:, c])
            assert np.all(np.abs(A).sum(axis=1) <= (1 + 4 * r) * (1 + 1e-12))
            want = np.linalg.solve(A, phi[:, c])
            assert np.abs(x[:, c] - want).max() <= bound, (target_r, c, np.abs(x[:, c] - want).max(), bound)


def test_zero_diffusivity_rows_are_the_identity():
    dzc, dzf = _spacings(9, 100.0, True)
    phi = np.random.default_rng(0).standard_normal((9, 5))
    assert np.array_equal(sdr.thomas(*sdr.centre_rows(dzc, dzf, np.zeros((10, 5)), 3.0), phi), phi)
    assert np.array_equal(sdr.thomas(*sdr.face_rows(dzc, dzf, np.zeros((9, 5)), 3.0), phi[:8]), phi[:8])


@pytest.mark.parametrize("Nz", [8, 32])
def test_cosine_eigenmode_decays_by_the_closed_form(Nz):
    """cos(pi (k - 1/2) / Nz) on a uniform grid decays by exactly 1 / (1 + K lambda dtau) per solve, lambda = (2 - 2 cos(pi / Nz)) / dz^2."""
    Lz, K, dtau = 100.0, 10.0, 1.0
    dzc, dzf = _spacings(Nz, Lz, False)
    dz = Lz / Nz
    mode = np.cos(np.pi * (np.arange(Nz) + 0.5) / Nz)[:, None]
    x = sdr.thomas(*sdr.centre_rows(dzc, dzf, np.full((Nz + 1, 1), K), dtau), mode)
    lam = (2 - 2 * np.cos(np.pi / Nz)) / dz ** 2
    want = mode / (1 + K * lam * dtau)
    assert np.abs(x - want).max() <= 1e-14 * np.abs(want).max()


def _rest_model(size, Lz, diffusivity, tracers=0, **kw):
    g = sdr.orc.Grid(size, x=(0, 100.0), y=(0, 100.0), z=(0, Lz))
    return sdr.DiffusivityModel(g, diffusivity, tracers=tracers, **kw)


def test_implicit_vertical_viscosity_steps_match_the_stage_amplification():
    """Rest state, rho u = cos(pi z / Lz), VerticalScalarDiffusivity(vitd; nu): a1 = 1 / (1 + z), a2 = (3/4 + a1 / 4) / (1 + z / 4),
    a3 = (1/3 + 2 a2 / 3) / (1 + 2 z / 3), z = nu lambda dt; ten steps are a3^10 to 1e-12 (advection and projection contribute exact
    zeros for an x-, y-invariant u).  The scalars come back bit-identical: kappa = 0."""
    Nz, Lz, nu, dt = 16, 100.0, 10.0, 1.0
    m = _rest_model((4, 4, Nz), Lz, sdr.Diffusivity(1, True, nu=nu))
    g = m.grid
    mode = np.cos(np.pi * g.zc / Lz)[:, None, None] + np.zeros((Nz, 4, 4))
    m.set(ru=mode)
    rtheta0, rq0 = m.rtheta.copy(), m.rq.copy()
    for _ in range(10):
        m.time_step(dt)
    z = nu * (2 - 2 * np.cos(np.pi / Nz)) / (Lz / Nz) ** 2 * dt
    a1 = 1 / (1 + z)
    a2 = (0.75 + 0.25 * a1) / (1 + z / 4)
    a3 = (1 / 3 + 2 / 3 * a2) / (1 + 2 / 3 * z)
    assert np.abs(g.interior(m.ru) - a3 ** 10 * mode).max() <= 1e-12
    assert np.abs(g.interior(m.rv)).max() == 0
    assert np.array_equal(m.rtheta, rtheta0) and np.array_equal(m.rq, rq0)


def test_explicit_isotropic_viscosity_steps_match_the_rk3_polynomial():
    """rho u = rho_r(z) sin(k y): ten steps are P(-nu lambda_y dt)^10, P = 1 + z + z^2 / 2 + z^3 / 6, to 1e-12."""
    Ny, nu, dt = 8, 3.0, 0.5
    m = _rest_model((4, Ny, 6), 100.0, sdr.Diffusivity(0, False, nu=nu))
    g = m.grid
    ky = 2 * np.pi / 100.0
    rho = m.ref.density[g.Hz:g.Hz + g.Nz][:, None, None]
    ru0 = rho * np.sin(ky * g.yc)[None, :, None] + np.zeros((6, Ny, 4))
    m.set(ru=ru0)
    for _ in range(10):
        m.time_step(dt)
    z = -nu * (2 - 2 * np.cos(ky * g.dy)) / g.dy ** 2 * dt
    P = 1 + z + z ** 2 / 2 + z ** 3 / 6
    assert np.abs(g.interior(m.ru) - P ** 10 * ru0).max() <= 1e-12 * np.abs(ru0).max()


def _decay(field0, field1):
    return np.sqrt(np.sum(field1 ** 2) / np.sum(field0 ** 2))


def _run_reference_case(diffusivity, dt, nt, tracer=False, momentum=False):
    """test/vertical_diffusion.jl: grid 4 x 4 x 32, Lz = 100, cosine profiles, from a rest state (the advective terms are exact zeros)."""
    m = _rest_model((4, 4, 32), 100.0, diffusivity, tracers=1 if tracer else 0)
    g = m.grid
    cosine = np.cos(np.pi * g.zc / 100.0)[:, None, None] + np.zeros((32, 4, 4))
    kw = {}
    if tracer:
        kw["rc0"] = cosine
    if momentum:
        kw["ru"] = cosine
    m.set(**kw)
    for _ in range(nt):
        m.time_step(dt)
    out = {}
    if tracer:
        out["c"] = _decay(cosine, g.interior(m.rc0))
    if momentum:
        out["u"] = _decay(cosine, g.interior(m.ru))
    return out


def test_reference_vertical_diffusion_known_answers():
    """test/vertical_diffusion.jl:24-138: decay within rtol 0.05 of exp(-K (pi / Lz)^2 t); implicit and explicit within rtol 0.01."""
    exact = lambda K, t: np.exp(-K * (np.pi / 100.0) ** 2 * t)
    d = _run_reference_case(sdr.Diffusivity(1, True, kappa=10.0), 1.0, 10, tracer=True)["c"]
    assert abs(d - exact(10.0, 10.0)) <= 0.05 * exact(10.0, 10.0)
    di = _run_reference_case(sdr.Diffusivity(1, True, kappa=1.0), 0.5, 10, tracer=True)["c"]
    de = _run_reference_case(sdr.Diffusivity(1, False, kappa=1.0), 0.5, 10, tracer=True)["c"]
    assert abs(di - exact(1.0, 5.0)) <= 0.05 * exact(1.0, 5.0)
    assert abs(de - exact(1.0, 5.0)) <= 0.05 * exact(1.0, 5.0)
    assert abs(di - de) <= 0.01 * max(di, de)
    d = _run_reference_case(sdr.Diffusivity(1, True, nu=10.0), 1.0, 10, momentum=True)["u"]
    assert abs(d - exact(10.0, 10.0)) <= 0.05 * exact(10.0, 10.0)
    both = _run_reference_case(sdr.Diffusivity(1, True, nu=5.0, kappa=10.0), 1.0, 10, tracer=True, momentum=True)
    assert abs(both["u"] - exact(5.0, 10.0)) <= 0.05 * exact(5.0, 10.0)
    assert abs(both["c"] - exact(10.0, 10.0)) <= 0.05 * exact(10.0, 10.0)


@pytest.mark.parametrize("implicit", [True, False])
def test_uniform_energy_is_not_diffused(implicit):
    """test/turbulence_closures.jl:38-50: uniform e, ScalarDiffusivity(disc, nu = 1, kappa = 1), one step: rho e within rtol 1e-5
    (isapprox: 2-norms).  The explicit fluxes of a uniform e are exact zeros: the step is bit-identical to the one with kappa = 0."""
    def run(kappa):
        g = sdr.orc.Grid((8, 8, 8), x=(0, 100.0), y=(0, 100.0), z=(0, 100.0))
        m = sdr.DiffusivityModel(g, sdr.Diffusivity(0, implicit, nu=1.0, kappa=kappa), formulation="StaticEnergy", tracers=1)
        m.set(e=m.constants.cpd * m.ref.theta0)
        re0 = g.interior(m.rtheta).copy()
        m.time_step(1.0)
        return re0, g.interior(m.rtheta).copy()
    re0, re1 = run(1.0)
    assert np.linalg.norm(re1 - re0) <= 1e-5 * max(np.linalg.norm(re1), np.linalg.norm(re0))
    if not implicit:
        assert np.array_equal(re1, run(0.0)[1])


def test_isotropic_explicit_tendencies_agree_with_the_smagorinsky_flux_code(oracle):
    """nu_e held at the given nu and Pr = nu / kappa: oracle.closure's own divergences are the isotropic explicit ones."""
    from oracle.closure import SmagorinskyLilly, add_closure_tendencies
    size, rng = (6, 5, 7), np.random.default_rng(5)
    sh = (7, 5, 6)
    g = oracle.Grid(size, x=(0, 60.0), y=(0, 50.0), z=_z_faces(7, 70.0, True))
    nu = 0.5 + rng.random(sh)
    m = sdr.DiffusivityModel(g, sdr.Diffusivity(0, False, nu=nu, kappa=nu / 0.7), tracers=1)
    m.set(theta=288.0 + rng.standard_normal(sh), qt=1e-3 * rng.random(sh), ru=rng.standard_normal(sh), rv=rng.standard_normal(sh),
          rw=rng.standard_normal((8, 5, 6)), rc0=rng.random(sh))
    for n in m.G:
        m.G[n][...] = 0.0
    sdr.add_diffusivity_tendencies(m)
    mine = {n: m.G[n].copy() for n in m.G}
    for n in m.G:
        m.G[n][...] = 0.0
    m.closure, m.nu_e = SmagorinskyLilly(Pr=0.7), nu
    add_closure_tendencies(m)
    for n in m.G:
        assert np.abs(mine[n] - m.G[n]).max() <= 1e-13 * max(np.abs(m.G[n]).max(), 1e-300), n
