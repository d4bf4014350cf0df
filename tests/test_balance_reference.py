"""Pins tests/balance_reference.py, the numpy restatement behind tests/test_balance.py, and the host side of set_to_mean! and
HydrostaticallyBalancedDensity (breeze.jl_amd/compressible.py).  No GPU.

Bounds.  A level of the column integration is a handful of float64 operations around three to eight pow(), and level k depends on level
k - 1 with a factor of about one, so the relative error grows like a random walk of a few eps per level: 64 levels stay below 1e-14, and the
issue's 1e-13 against the longdouble evaluation leaves an order of margin (measured 1.5e-16 … 1.9e-15).  The discrete balance is limited by
the rounding of p itself: half an ulp of p[k-1] over Δzᶠ is 0.5 eps p/Δzᶠ, the scale of the bound; 8 of them are asserted (measured
0.8 … 1.3)."""
import numpy as np
import pytest

import balance_reference as br

EPS = float(np.finfo(np.float64).eps)
P0, PST = 101325.0, 1e5


def _faces(Nz, stretched):
    if not stretched:
        return np.linspace(0.0, 100.0 * Nz, Nz + 1)
    s = np.linspace(0.0, 1.0, Nz + 1)
    return np.round(100.0 * Nz * (0.5 * s + 0.5 * s ** 2))      # whole-number faces


def _profiles(Nz, stretched, moist, seed, columns=()):
    rng = np.random.default_rng(seed)
    zf = _faces(Nz, stretched)
    zc = 0.5 * (zf[:-1] + zf[1:]).reshape((-1,) + (1,) * len(columns))
    th = 300.0 + 0.004 * zc + rng.uniform(-0.5, 0.5, (Nz,) + tuple(columns))
    qv = (0.015 * np.exp(-zc / 2500.0) * rng.uniform(0.7, 1.3, (Nz,) + tuple(columns))) if moist else None
    return zf, th, qv


CASES = [(Nz, st, moist) for Nz in (2, 5, 12, 33, 64) for st in (False, True) for moist in (False, True)]


@pytest.fixture(scope="module")
def constants(bz):
    return br.constants_tuple(bz.ThermodynamicConstants())


@pytest.mark.parametrize("Nz,stretched,moist", CASES)
def test_column_is_in_discrete_balance_and_agrees_with_longdouble(constants, Nz, stretched, moist):
    zf, th, qv = _profiles(Nz, stretched, moist, seed=Nz, columns=(3,))
    dzc, dzf = br.z_metrics(zf)
    Pi, p, rho = br.exner_columns(th, qv, dzc, dzf, P0, PST, constants)
    ratio = br.balance_ratio(p, rho, dzf, constants[0], EPS)
    PiL, pL, rhoL = br.exner_columns(th, qv, dzc, dzf, P0, PST, constants, dtype=np.longdouble)
    worst = max(br.max_rel(Pi, PiL), br.max_rel(p, pL), br.max_rel(rho, rhoL))
    print(f"Nz={Nz} stretched={stretched} moist={moist}: balance {ratio:.2f} eps p/dz, vs longdouble {worst:.2e}")
    assert ratio <= 8.0
    assert worst <= 1e-13
    assert np.all(np.diff(p, axis=0) < 0) and np.all(rho > 0)


def test_dry_column_is_the_moist_one_at_zero_vapour(constants):
    zf, th, _ = _profiles(12, True, False, seed=3)
    dzc, dzf = br.z_metrics(zf)
    dry = br.exner_columns(th, None, dzc, dzf, P0, PST, constants)
    zero = br.exner_columns(th, np.zeros_like(th), dzc, dzf, P0, PST, constants)
    for a, b in zip(dry, zero):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("Nz,stretched", [(5, False), (16, True), (33, False), (64, True)])
def test_restatement_agrees_with_the_host_constructor(bz, constants, Nz, stretched):
    """ExnerReferenceState (breeze.jl_amd/compressible.py) on θ(z), qᵛ(z): the same operations in the same order, scalar by scalar there and
    level arrays here; each is within 1e-13 of the exact column (above), so they are within 2e-13 of each other."""
    zf = _faces(Nz, stretched)
    grid = bz.RectilinearGrid((8, 8, Nz), x=(0, 800), y=(0, 800), z=zf if stretched else (zf[0], zf[-1]))

    def theta(z):
        return 300.0 + 0.004 * z + 0.3 * np.sin(z / 700.0)

    def qv(z):
        return 0.015 * np.exp(-z / 2500.0)

    ref = bz.ExnerReferenceState(grid, surface_pressure=P0, potential_temperature=theta, vapor_mass_fraction=qv)
    dzc, dzf = br.z_metrics(zf)
    zc = 0.5 * (zf[:-1] + zf[1:])
    Pi, p, rho = br.exner_columns(theta(zc), qv(zc), dzc, dzf, P0, PST, constants)
    H = grid.Hz
    worst = max(br.max_rel(ref.exner_function[H:H + Nz], Pi), br.max_rel(ref.pressure[H:H + Nz], p), br.max_rel(ref.density[H:H + Nz], rho))
    print(f"Nz={Nz}: host constructor vs restatement {worst:.2e}")
    assert worst <= 2e-13
    # the constructor path from profile arrays is the same code: bit for bit, halo levels included
    again = bz.ExnerReferenceState.from_profiles(grid, theta(zc), qv(zc), surface_pressure=P0, surface_potential_temperature=theta(0.0))
    for name in ("exner_function", "pressure", "density", "potential_temperature"):
        assert np.array_equal(getattr(ref, name), getattr(again, name)), name


def test_set_profiles_recomputes_a_reference_in_place(bz):
    """reference_states.jl:532-550: a reference built at θ = 290, recomputed from the (uniform) mean 305, is a fresh ExnerReferenceState(θ = 305).
    The bottom halo of the density keeps the boundary value of construction, as the reference's field does."""
    grid = bz.RectilinearGrid((8, 8, 16), x=(0, 800), y=(0, 800), z=(0, 1600))
    ref = bz.ExnerReferenceState(grid, surface_pressure=P0, potential_temperature=290)
    fresh = bz.ExnerReferenceState(grid, surface_pressure=P0, potential_temperature=305)
    pressure_object = ref
    rho0_built = ref.surface_density
    mean_theta = np.full((16, 8, 8), 305.0).sum(axis=(1, 2)) / 64      # bz_horizontal_average: level sum over Nx Ny
    ref.set_profiles_(mean_theta, np.zeros(16))
    assert ref is pressure_object
    H = grid.Hz
    for name in ("exner_function", "pressure", "density"):
        assert br.max_rel(getattr(ref, name)[H:H + 16], getattr(fresh, name)[H:H + 16]) <= 1e-13, name
    assert ref.surface_density == rho0_built
    assert ref.density[H - 1] == 2 * rho0_built - ref.density[H] and ref.pressure[H - 1] == 2 * P0 - ref.pressure[H]
    assert ref.density[H + 16] == ref.density[H + 15] and ref.exner_function[H - 1] == ref.exner_function[H]


def _uniform_state(Nz, Ny, Nx, theta, q):
    ones = np.ones((Nz, Ny, Nx))
    return {"rho_d": ones.copy(), "ru": 0 * ones, "rv": 0 * ones, "rw": np.zeros((Nz + 1, Ny, Nx)), "rth": theta * ones, "rq": q * ones}


def test_balanced_set_known_answers(bz, constants):
    """reference_states.jl:727-746: uniform θ with qᵗ = 0 and HydrostaticallyBalancedDensity(p₀) gives the pressure and total density of the
    fresh reference; with qᵗ = 0.02 the specific humidity comes back as 0.02."""
    Nz = 16
    grid = bz.RectilinearGrid((8, 8, Nz), x=(0, 800), y=(0, 800), z=(0, 1600))
    fresh = bz.ExnerReferenceState(grid, surface_pressure=P0, potential_temperature=300)
    dzc, dzf = br.z_metrics(np.linspace(0.0, 1600.0, Nz + 1))
    th = np.full((Nz, 8, 8), 300.0)
    out = br.balanced_set(_uniform_state(Nz, 8, 8, 300.0, 0.0), th, dzc, dzf, P0, PST, constants)
    H = grid.Hz
    assert br.max_rel(out["p_column"], fresh.pressure[H:H + Nz].reshape(-1, 1, 1) * np.ones_like(th)) <= 1e-13
    assert br.max_rel(out["rho"], fresh.density[H:H + Nz].reshape(-1, 1, 1) * np.ones_like(th)) <= 1e-13
    assert np.array_equal(out["rho"], out["rho_d"]) and not out["rq"].any()
    moist = br.balanced_set(_uniform_state(Nz, 8, 8, 300.0, 0.02), th, dzc, dzf, P0, PST, constants)
    assert br.max_rel(moist["rq"] / moist["rho"], 0.02) <= 4 * EPS
    assert br.max_rel(moist["rth"] / moist["rho_d"], 300.0) <= 4 * EPS
    assert br.balance_ratio(out["p_column"], out["rho"], dzf, constants[0], EPS) <= 8.0


def test_balanced_set_preserves_specific_quantities(constants):
    """θ and q within 4 eps (a product and a quotient of rounded numbers, q through the residual density), velocities within 8 eps (a face
    mean more); the wall faces of ρw are not touched; Kessler species ride with the total density."""
    rng = np.random.default_rng(5)
    Nz, Ny, Nx = 12, 6, 10
    sh = (Nz, Ny, Nx)
    zf = _faces(Nz, True)
    dzc, dzf = br.z_metrics(zf)
    old = rng.uniform(0.8, 1.2, sh)
    th, q, qcl, qr = 300.0 + rng.uniform(0, 20, sh), rng.uniform(0, 0.02, sh), rng.uniform(0, 1e-3, sh), rng.uniform(0, 1e-3, sh)
    u, v = rng.normal(0, 5, sh), rng.normal(0, 5, sh)
    w = rng.normal(0, 1, (Nz + 1, Ny, Nx))

    def fx(a):
        return (a + np.roll(a, 1, 2)) / 2

    def fy(a):
        return (a + np.roll(a, 1, 1)) / 2

    state = {"rho_d": old, "ru": fx(old) * u, "rv": fy(old) * v, "rw": w.copy(), "rth": old * th, "rq": old * q, "rqcl": old * qcl, "rqr": old * qr}
    state["rw"][1:Nz] *= (old[1:] + old[:-1]) / 2
    out = br.balanced_set(state, state["rth"] / old, dzc, dzf, P0, PST, constants, kessler=True)
    new = out["rho_d"]
    assert br.max_rel(out["rth"] / new, state["rth"] / old) <= 4 * EPS
    for k in ("rq", "rqcl", "rqr"):
        assert br.max_rel(out[k] / out["rho_column"], state[k] / old) <= 4 * EPS, k
    assert br.max_rel(out["ru"] / fx(new), state["ru"] / fx(old)) <= 8 * EPS
    assert br.max_rel(out["rv"] / fy(new), state["rv"] / fy(old)) <= 8 * EPS
    assert br.max_rel(out["rw"][1:Nz] / ((new[1:] + new[:-1]) / 2), w[1:Nz]) <= 8 * EPS
    assert np.array_equal(out["rw"][0], w[0]) and np.array_equal(out["rw"][Nz], w[Nz])
    assert np.array_equal(out["rho"], new + (out["rq"] + (out["rqcl"] + (out["rqr"] + 0.0))))
    assert br.max_rel(out["rho"], out["rho_column"]) <= 2 * EPS


def test_host_api_names_and_refusals(bz):
    """the public names exist and validate their arguments without a GPU"""
    spec = bz.HydrostaticallyBalancedDensity()
    assert spec.surface_pressure is None and bz.HydrostaticallyBalancedDensity(surface_pressure=1e5).surface_pressure == 1e5
    with pytest.raises(ValueError, match="surface_pressure"):
        bz.HydrostaticallyBalancedDensity(surface_pressure=-1.0)
    assert callable(bz.set_to_mean_)
    grid = bz.RectilinearGrid((8, 8, 8), x=(0, 800), y=(0, 800), z=(0, 800))
    with pytest.raises(ValueError, match="Nz"):
        bz.ExnerReferenceState.from_profiles(grid, np.full(7, 300.0))
    ref = bz.ExnerReferenceState(grid, potential_temperature=300)
    dyn = bz.CompressibleDynamics(bz.SplitExplicitTimeDiscretization(), reference_state=ref)
    assert dyn._reference_given is ref
    with pytest.raises(ValueError, match="mutually exclusive"):
        bz.CompressibleDynamics(bz.SplitExplicitTimeDiscretization(), reference_state=ref, reference_potential_temperature=300.0)
    for name in ("bz_exner_columns", "bz_set_hydrostatically_balanced_density", "bz_set_exner_reference_state"):
        assert name in bz.SYMBOLS


def test_the_two_level_grid_is_refused_by_the_grid_itself(bz):
    """(16, 8, 2) of the device shapes: the kernels need halos of three levels and a halo cannot be wider than the domain, so the shortest
    column a model runs has Nz = 3 (tests/test_balance.py); the two-level recurrence is covered by the restatement cases above"""
    with pytest.raises(ValueError):
        bz.RectilinearGrid((16, 8, 2), x=(0, 1600), y=(0, 800), z=(0, 200))
    bz.RectilinearGrid((16, 8, 3), x=(0, 1600), y=(0, 800), z=(0, 300))
