"""Azimuthal means and polar winds on the device (csrc/bz_azimuthal.hip: bz_azimuthal_mean, bz_polar_winds; breeze.jl_amd/diagnostics.py)
against the numpy restatement tests/azimuthal_reference.py.

Counts.  A case is compared exactly in a precision only if the restatement shows every sample's r/Δr at least 16·eps·Nr away from a ring
edge in that precision (the chain to r/Δr has about four roundings on a value ≤ Nr: a 4× margin); the test asserts that condition.  Cases
whose Float32 margin is too small ("64_nr200": 1150 eps of 3200, "20_ext03": 58 of 176, "130x12_m8": 32 of 1120) are Float64 only.  The
rectangular case failed it about (0.13, −0.21) (46 eps of 144) and was moved to (0.125, −0.215) (1708 eps).
Means.  |device − longdouble mean| ≤ (n + 2)·eps·(Σ|f_s| / n) per ring with n samples: the first-order bound of any summation order.
Polar winds.  8 eps (|uᶜ| + |vᶜ|) in Float64; the Float32 twin within 4× the restatement's own Float32 error.

Measured on the MI355X: counts equal in all 27 (case, precision) pairs; worst mean error / bound 0.167 in Float64 and in
Float32 (Nr = 300), ≤ 0.073 for Nr ≤ 64; polar winds 1.2 / 1.6 eps of |uᶜ| + |vᶜ|, Float32 twin 0.85 / 1.00 of the restatement's own error."""
import ctypes as C

import numpy as np
import pytest

import azimuthal_reference as ar

pytestmark = pytest.mark.gpu

F64, F32 = np.float64, np.float32
KM = 1e3
# name: (size, x, y, radius, Nr, center, m, precisions compared)
CASES = {
    "64_nr8": ((64, 64, 4), (-1, 1), (-1, 1), 1.0, 8, (0.0, 0.0), 4, (F64, F32)),
    "64_nr64_m1": ((64, 64, 4), (-1, 1), (-1, 1), 1.0, 64, (0.0, 0.0), 1, (F64, F32)),          # 3 empty rings
    "64_nr64": ((64, 64, 4), (-1, 1), (-1, 1), 1.0, 64, (0.0, 0.0), 4, (F64, F32)),
    "64_nr200": ((64, 64, 4), (-1, 1), (-1, 1), 1.0, 200, (0.0, 0.0), 4, (F64,)),               # 1 empty ring; four accumulators per lane
    "64_r05_off": ((64, 64, 4), (-1, 1), (-1, 1), 0.5, 8, (0.3, -0.2), 4, (F64, F32)),
    "24_nr7_m3": ((24, 24, 3), (-1, 1), (-1, 1), 1.0, 7, (0.3, -0.2), 3, (F64, F32)),
    "20_ext03": ((20, 20, 3), (0, 3), (0, 3), 1.3, 11, (1.7, 1.1), 4, (F64,)),
    "12_nr5_m2": ((12, 12, 3), (-1, 1), (-1, 1), 0.9, 5, (0.05, 0.0), 2, (F64, F32)),
    "40_150km": ((40, 40, 4), (-150 * KM, 150 * KM), (-150 * KM, 150 * KM), 150 * KM, 30, (0.0, 0.0), 4, (F64, F32)),
    "rect_40x24": ((40, 24, 3), (-2, 2), (-1.5, 1.5), 1.4, 9, (0.125, -0.215), 4, (F64, F32)),   # Nx ≠ Ny, Δx = 0.1 ≠ Δy = 0.125
    "nr1": ((24, 24, 3), (-1, 1), (-1, 1), 0.77, 1, (0.1, 0.05), 4, (F64, F32)),
    "outside": ((24, 20, 3), (-1, 1), (-1, 1), 1.9, 12, (1.43, 0.31), 4, (F64, F32)),             # the centre lies outside the domain; 2 empty rings
    "130x12_m8": ((130, 12, 3), (0, 13), (0, 1.3), 3.1, 70, (6.37, 0.61), 8, (F64,)),             # rows cross lanes 64 and 128; slices without rows
    "nr300": ((24, 24, 3), (-1, 1), (-1, 1), 1.0, 300, (0.3, -0.2), 2, (F64, F32)),               # sixteen accumulators per lane, a cell spans 38 rings
    "nr1024": ((16, 12, 3), (-1, 1), (-1, 1), 1.1, 1024, (0.3, -0.2), 1, (F64, F32)),             # the largest Nr
}
PAIRS = [(n, p) for n, c in CASES.items() for p in c[7]]
IDS = [f"{n}-{p.__name__}" for n, p in PAIRS]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == F64 else np.uint32)


class Case:
    def __init__(self, bz, name, real):
        size, x, y, self.radius, self.Nr, self.center, self.m, _ = CASES[name]
        self.bz, self.real, self.name = bz, real, name
        self.grid = g = bz.RectilinearGrid(size, x=x, y=y, z=(0.0, 1.0), float_type=real)
        self.model = bz.AtmosphereModel(g, advection=bz.WENO(order=5))
        self.kw = dict(radius=self.radius, Nr=self.Nr, center=self.center, m=self.m)
        self._ref = {}
        rng = np.random.default_rng(len(name) * 1000 + self.Nr)
        sh = (g.Nz, g.Ny, g.Nx)
        self.random = (rng.standard_normal(sh) * 10.0 ** rng.uniform(-2, 2, sh)).astype(real)          # another pattern on every level
        X, Y = np.asarray(g.xᶜ)[None, None, :] - self.center[0], np.asarray(g.yᶜ)[None, :, None] - self.center[1]
        self.rfield = (np.sqrt(X ** 2 + Y ** 2) * np.ones(sh)).astype(real)

    def field(self, interior, zface=False, halo=float("nan")):
        """a Field whose halos are all `halo`"""
        import torch
        from breeze_jl_amd.grids import Center, Face
        f = self.bz.Field(self.grid, (Center, Center, Face if zface else Center), self.model.device)
        f.parent.fill_(halo)
        f.interior.copy_(torch.from_numpy(np.ascontiguousarray(interior)).to(f.dtype))
        return f

    def device(self, interior, zface=False, halo=float("nan")):
        return self.bz.azimuthal_mean(self.field(interior, zface, halo), model=self.model, **self.kw)

    def reference(self, key, interior):
        """the restatement in the case's precision on the values the device holds; computed once per field"""
        if key not in self._ref:
            g = self.grid
            self._ref[key] = ar.azimuthal_mean(interior, g.xᶜ, g.yᶜ, g.Δx, g.Δy, dtype=self.real, **self.kw)
        return self._ref[key]


@pytest.fixture(scope="module")
def cases(bz):
    made = {}

    def get(name, real):
        if (name, real) not in made:
            made[name, real] = Case(bz, name, real)
        return made[name, real]
    return get


# ---- 1. counts -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,real", PAIRS, ids=IDS)
def test_counts_are_the_reference_formulas_exactly(cases, name, real):
    c = cases(name, real)
    g = c.grid
    five = np.full((g.Nz, g.Ny, g.Nx), 5.0, real)
    want = c.reference("five", five)
    eps = np.finfo(real).eps
    print(f"AZ-MARGIN {name} {real.__name__}: {want.margin / eps:.3g} eps, need {16 * c.Nr}")
    assert want.margin >= 16 * eps * c.Nr, (want.margin / eps, 16 * c.Nr)          # the case is fit for an exact comparison
    got = c.device(five)
    assert got.data.shape == (c.Nr, g.Nz) and got.data.dtype == real and got.counts.dtype == np.int64
    assert np.array_equal(got.counts, want.counts), np.flatnonzero(got.counts != want.counts)
    assert got.counts.sum() + want.dropped == g.Nx * g.Ny * c.m ** 2
    empty = got.counts == 0
    assert np.array_equal(np.isnan(got.data), np.broadcast_to(empty[:, None], got.data.shape))      # NaN at every level of an empty ring, nowhere else
    assert np.all(got.data[~empty] == 5.0)                                                              # a constant is returned exactly
    np.testing.assert_allclose(got.r, (np.arange(c.Nr) + 0.5) * c.radius / c.Nr, rtol=1e-14)
    assert np.array_equal(got.z, g.zᶜ)


# ---- 2. means ------------------------------------------------------------------------------------------------------------------------
def _check_means(c, got, want, what):
    eps = np.finfo(c.real).eps
    n = want.counts.astype(ar.L)[None, :]
    live = want.counts > 0
    bound = ((n + 2) * eps * (want.abs_sum / np.maximum(n, 1)))[:, live]
    err = np.abs(got.data.T.astype(ar.L) - want.mean)[:, live]
    with np.errstate(all="ignore"):
        ratio = float(np.max(np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))))
    print(f"AZ-MEAN {c.name} {c.real.__name__} {what}: worst error / bound = {ratio:.3e}")
    assert np.array_equal(got.counts, want.counts)
    assert np.array_equal(np.isnan(got.data.T), np.isnan(want.mean))
    assert np.all(err <= bound), ratio


@pytest.mark.parametrize("name,real", PAIRS, ids=IDS)
def test_means_within_the_first_order_bound_of_any_summation_order(cases, name, real):
    c = cases(name, real)
    _check_means(c, c.device(c.random), c.reference("random", c.random), "random")
    _check_means(c, c.device(c.rfield), c.reference("radius", c.rfield), "radius")


# ---- 3. halos, 4. determinism ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,real", [("rect_40x24", F64), ("130x12_m8", F64), ("64_r05_off", F32)])
def test_halos_are_never_read(cases, name, real):
    c = cases(name, real)
    a, b = c.device(c.random, halo=float("nan")), c.device(c.random, halo=0.0)
    assert np.array_equal(_bits(a.data), _bits(b.data)) and np.isfinite(a.data[a.counts > 0]).all()


@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("name,real", [("64_nr8", F64), ("64_r05_off", F32), ("64_nr64", F64), ("nr300", F32)])      # packed and table-row counts
def test_a_non_finite_cell_reaches_only_the_rings_it_touches(cases, name, real, bad):
    """The reference adds ifelse(in_ring, f, 0): a NaN or Inf cell spoils the rings that hold one of its samples and no other, although the
    cell's count row is wider than the rings it touches (its tail is zero)."""
    c = cases(name, real)
    g = c.grid
    b, _ = ar.ring_index(g.xᶜ, g.yᶜ, g.Δx, g.Δy, c.radius, c.Nr, c.center, c.m, real)
    spread = int(np.sqrt(g.Δx ** 2 + g.Δy ** 2) / (c.radius / c.Nr)) + 3          # entries of a cell's count row
    inside = np.argwhere((b >= 0).all(axis=(2, 3)))          # cells with every sample inside the radius, in row order
    k, (j, i) = 1, inside[(2 * len(inside)) // 3]
    touched = np.unique(b[j, i])
    assert 1 <= touched.size < min(spread, c.Nr)          # the cell's row has a zero tail
    x, zeroed = c.random.copy(), c.random.copy()
    x[k, j, i], zeroed[k, j, i] = bad, 0.0
    got, clean = c.device(x), c.device(zeroed)
    hit = np.zeros((c.Nr, g.Nz), bool)
    hit[touched, k] = True
    assert not np.isfinite(got.data[hit]).any()
    assert np.array_equal(got.data[~hit], clean.data[~hit], equal_nan=True)          # every other ring and level: as if the cell held 0
    assert np.isfinite(got.data[~hit & (got.counts > 0)[:, None]]).all()
    # a non-finite cell with no sample inside the radius is not used at all
    far = np.argwhere((b < 0).all(axis=(2, 3)))
    if far.size:
        y = c.random.copy()
        y[:, far[0][0], far[0][1]] = bad
        assert np.array_equal(_bits(c.device(y).data), _bits(c.device(c.random).data))


@pytest.mark.parametrize("name,real", [("64_nr64", F64), ("nr300", F64), ("40_150km", F32)])
def test_two_calls_and_a_rebuilt_plan_give_the_same_bits(cases, name, real):
    c = cases(name, real)
    f = c.field(c.random)
    first = c.bz.azimuthal_mean(f, model=c.model, **c.kw)
    again = c.bz.azimuthal_mean(f, model=c.model, **c.kw)                          # the cached plan
    other = c.bz.azimuthal_mean(f, model=c.model, radius=0.61 * c.radius, Nr=c.Nr + 3, center=(c.center[0] + 0.1 * c.radius, c.center[1]), m=3)
    rebuilt = c.bz.azimuthal_mean(f, model=c.model, **c.kw)                        # another geometry in between: the plan is built again
    assert other.data.shape[0] == c.Nr + 3 and not np.array_equal(other.counts[:c.Nr], first.counts)
    for r in (again, rebuilt):
        assert np.array_equal(_bits(first.data), _bits(r.data)) and np.array_equal(first.counts, r.counts)


# ---- 5. z-face fields -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,real", [("24_nr7_m3", F64), ("rect_40x24", F32)])
def test_z_face_fields_have_one_more_level(cases, name, real):
    c = cases(name, real)
    g = c.grid
    rng = np.random.default_rng(5)
    x = rng.standard_normal((g.Nz + 1, g.Ny, g.Nx)).astype(real)
    got = c.device(x, zface=True)
    assert got.data.shape == (c.Nr, g.Nz + 1) and np.array_equal(got.z, g.zᶠ)
    _check_means(c, got, c.reference("zface", x), "z-face")


# ---- 6. operations, stale diagnostics -------------------------------------------------------------------------------------------------
def _anelastic(bz):
    grid = bz.RectilinearGrid((24, 20, 4), x=(-12e3, 12e3), y=(-10e3, 10e3), z=(0, 4e3))
    m = bz.AtmosphereModel(grid, dynamics=bz.AnelasticDynamics(bz.ReferenceState(grid, potential_temperature=300.0)), advection=bz.WENO(order=5))
    m.set(θ=lambda x, y, z: 300.0 + 1e-3 * z + 2.0 * np.exp(-(x ** 2 + y ** 2) / 2e7), u=3.0,
          qᵗ=lambda x, y, z: 0.01 * np.exp(-z / 2.5e3) * (1 + 0.2 * np.sin(2 * np.pi * x / 24e3)) + 0 * y)
    return m


def test_an_operation_is_computed_and_reduced(bz):
    m = _anelastic(bz)
    kw = dict(radius=9e3, Nr=6, center=(1e3, -500.0))
    a = bz.azimuthal_mean(bz.LiquidIcePotentialTemperature(m), **kw)
    b = bz.azimuthal_mean(bz.LiquidIcePotentialTemperature(m).compute(), model=m, **kw)
    assert np.array_equal(_bits(a.data), _bits(b.data)) and np.array_equal(a.counts, b.counts)
    assert a.data.shape == (6, 4) and np.isfinite(a.data).all() and 299 < a.data.min() < a.data.max() < 310
    c = bz.azimuthal_mean(m.potential_temperature, **kw)                          # a model field knows its model
    assert np.isfinite(c.data).all()


def test_stale_model_fields_are_rebuilt_first(bz):
    def stepped():
        m = _anelastic(bz)
        m.time_steps(4.0, 3, diagnose_last=False)
        return m
    kw = dict(radius=9e3, Nr=6)
    a = stepped()
    assert bz.diagnostics_stale(a)
    ma = bz.azimuthal_mean(a.potential_temperature, **kw)
    assert not bz.diagnostics_stale(a)
    b = stepped()
    bz.update_state_(b, compute_tendencies=False)
    mb = bz.azimuthal_mean(b.potential_temperature, **kw)
    assert np.array_equal(_bits(ma.data), _bits(mb.data))
    c = stepped()
    va = bz.TangentialVelocity(c).compute().interior_cpu()
    assert not bz.diagnostics_stale(c)
    assert np.array_equal(va, bz.TangentialVelocity(b).compute().interior_cpu())


# ---- 7. polar winds -------------------------------------------------------------------------------------------------------------------
def _wind_model(bz, real, u, v):
    """24 × 20 × 4 doubly periodic model whose velocity fields hold the given interiors, halos filled"""
    import torch
    grid = bz.RectilinearGrid((24, 20, 4), x=(-1.2, 1.2), y=(-1.0, 1.0), z=(0.0, 1.0), float_type=real)
    m = bz.AtmosphereModel(grid, advection=bz.WENO(order=5))
    for key, a in (("u", u), ("v", v)):
        f = m.velocities[key]
        f.parent.fill_(float("nan"))
        f.interior.copy_(torch.from_numpy(np.ascontiguousarray(a(grid) if callable(a) else a)).to(f.dtype))
        bz.fill_halo_regions_(m, f)
    return m


def _random_winds(real):
    rng = np.random.default_rng(24204)
    return rng.standard_normal((4, 20, 24)).astype(real), rng.standard_normal((4, 20, 24)).astype(real)


CENTER = (0.3, -0.2)


def test_polar_winds_of_random_velocities(bz):
    u, v = _random_winds(F64)
    m = _wind_model(bz, F64, u, v)
    g = m.grid
    vt, vr, scale = ar.polar_winds(u, v, g.xᶜ, g.yᶜ, CENTER)
    ft, fr = bz.TangentialVelocity(m, center=CENTER).compute(), bz.RadialVelocity(m, center=CENTER).compute()
    eps = np.finfo(F64).eps
    for what, f, want in (("tangential", ft, vt), ("radial", fr, vr)):
        err = np.abs(f.interior_cpu() - want) / scale
        print(f"POLAR {what}: worst error / (|uc| + |vc|) = {err.max() / eps:.2f} eps")
        assert np.all(err <= 8 * eps)
        P, H = f.cpu(), (g.Hz, g.Hy, g.Hx)
        assert np.array_equal(P[H[0]:-H[0], H[1]:-H[1], 0], P[H[0]:-H[0], H[1]:-H[1], g.Nx])          # halos filled
    # (the last column and row read the wrapped faces i = Nx, j = Ny: the restatement rolls them in)


def test_solid_body_rotation_is_tangential(bz):
    Ω = 0.7
    # u = −Ω y at the x faces does not vary along x and v = Ω x at the y faces does not vary along y, so the periodic wrap of the last
    # face is harmless: uᶜ = −Ω yᶜ and vᶜ = Ω xᶜ in every cell, and about the origin vθ = Ω r, vʳ = 0
    u = lambda g: np.broadcast_to((-Ω * g.yᶜ)[None, :, None], (4, 20, 24))
    v = lambda g: np.broadcast_to((Ω * g.xᶜ)[None, None, :], (4, 20, 24))
    m = _wind_model(bz, F64, u, v)
    g = m.grid
    X, Y = g.xᶜ[None, None, :], g.yᶜ[None, :, None]
    vt0 = bz.TangentialVelocity(m).compute().interior_cpu()
    vr0 = bz.RadialVelocity(m).compute().interior_cpu()
    r = np.sqrt(X ** 2 + Y ** 2)
    bound = 8 * np.finfo(F64).eps * (np.abs(Ω * Y) + np.abs(Ω * X)) + 0 * vt0
    print(f"ROTATION: worst error / bound: tangential {np.max(np.abs(vt0 - Ω * r) / bound):.3f}, radial {np.max(np.abs(vr0) / bound):.3f}")
    assert np.all(np.abs(vt0 - Ω * r) <= bound) and np.all(np.abs(vr0) <= bound)


def test_polar_winds_float32_twin(bz):
    u, v = _random_winds(F32)
    m = _wind_model(bz, F32, u, v)
    g = m.grid
    xc, yc = np.asarray(g.xᶜ).astype(F32), np.asarray(g.yᶜ).astype(F32)
    c32 = (float(F32(CENTER[0])), float(F32(CENTER[1])))
    want = ar.polar_winds(u, v, xc, yc, c32, F64)              # Float64 arithmetic on the Float32-rounded inputs
    own = ar.polar_winds(u, v, xc, yc, c32, F32)
    ft, fr = bz.TangentialVelocity(m, center=CENTER).compute(), bz.RadialVelocity(m, center=CENTER).compute()
    for what, f, w, o in (("tangential", ft, want[0], own[0]), ("radial", fr, want[1], own[1])):
        E32 = np.max(np.abs(o.astype(F64) - w))
        err = np.max(np.abs(f.interior_cpu().astype(F64) - w))
        print(f"F32POLAR {what}: E32 = {E32:.3e} device = {err:.3e} ratio = {err / E32:.2f}")
        assert f.interior_cpu().dtype == F32 and err <= 4 * E32


# ---- 8. the rainband example's analysis ----------------------------------------------------------------------------------------------
def test_rainband_example_analysis(bz):
    """examples/tropical_cyclone_with_rainband.jl: the model's keyword list at a small size, one step, then the example's two reductions"""
    N, Nz, L, Lz = 32, 25, 160e3, 25e3
    grid = bz.RectilinearGrid((N, N, Nz), halo=(5, 5, 5), x=(-L / 2, L / 2), y=(-L / 2, L / 2), z=(0.0, Lz))
    θb = lambda z: 300.0 + 0.004 * z
    dyn = bz.CompressibleDynamics(bz.SplitExplicitTimeDiscretization(), surface_pressure=101500.0, reference_potential_temperature=θb)
    ref = bz.ExnerReferenceState(grid, surface_pressure=101500.0, potential_temperature=θb)
    Hz = grid.Hz
    mask = lambda z: np.sin(np.pi * np.clip((z - 20e3) / 5e3, 0.0, None) / 2) ** 2 * (z > 20e3)
    sponge = lambda target=0.0: bz.Relaxation(rate=1.0 / 333.0, mask=mask, target=target)
    heating = lambda x, y, z: (4.24 / 3600.0) * np.exp(-((np.sqrt(x ** 2 + y ** 2) - 40e3) / 10e3) ** 2) * np.sin(np.pi * np.clip((z - 4e3) / 8e3, 0.0, 1.0)) ** 2
    model = bz.CompressibleAtmosphereModel(grid, dyn, coriolis=bz.FPlane(f=5e-5), advection=bz.WENO(order=5),
                                           forcing={"ρu": sponge(), "ρv": sponge(), "ρw": sponge(), "θ": bz.Forcing(heating),
                                                    "ρθ": sponge(np.asarray(ref.density)[Hz:Hz + Nz] * (300.0 + 0.004 * np.asarray(grid.zᶜ)))})
    col = np.asarray(ref.density)[Hz:Hz + Nz][:, None, None]
    vmax, rm = 20.0, 30e3
    vt = lambda r: vmax * (r / rm) * np.exp(0.5 * (1 - (r / rm) ** 2))
    r = lambda x, y: np.sqrt(x ** 2 + y ** 2) + 1e-9
    model.set(ρ=col, θ=lambda x, y, z: 300.0 + 0.004 * z + 0 * x + 0 * y, u=lambda x, y, z: -vt(r(x, y)) * y / r(x, y) * np.exp(-z / 8e3),
              v=lambda x, y, z: vt(r(x, y)) * x / r(x, y) * np.exp(-z / 8e3), w=0.0, qᵗ=0.0)
    model.time_step(10.0)
    radius = 75e3
    v̄ = bz.azimuthal_mean(bz.TangentialVelocity(model).compute(), radius, Nr=30, model=model)
    θ̄ = bz.azimuthal_mean(bz.LiquidIcePotentialTemperature(model), radius, Nr=30)
    live = v̄.counts > 0
    assert live.sum() >= 25 and np.array_equal(v̄.counts, θ̄.counts) and v̄.data.shape == (30, Nz)
    assert np.isfinite(v̄.data[live]).all() and np.isfinite(θ̄.data[live]).all()
    assert np.isnan(v̄.data[~live]).all()
    k = 0
    peak = v̄.r[live][np.argmax(v̄.data[live, k])]
    assert 20e3 < peak < 40e3 and 15.0 < v̄.data[live, k].max() < 20.5          # the vortex the example sets: 20 m/s at 30 km
    assert np.all(np.abs(θ̄.data[live] - (300.0 + 0.004 * np.asarray(grid.zᶜ))[None, :]) < 1.0)


# ---- 9. errors ------------------------------------------------------------------------------------------------------------------------
def _raw_call(m, field, radius=1.0, Nr=8, mm=4, lib=None, ctx=None):
    T = m._T
    prof = np.zeros((m.grid.Nz + 1) * max(Nr, 1), dtype=T.np_real)
    return (lib or m._lib).bz_azimuthal_mean(ctx or m._ctx, C.c_void_p(field.ptr()), 0, 0.0, 0.0, radius, Nr, mm,
                                             prof.ctypes.data_as(C.POINTER(T.real)), None)


def test_invalid_arguments_and_the_context_stays_usable(cases):
    c = cases("24_nr7_m3", F64)
    m, f = c.model, c.field(c.random)
    before = c.bz.azimuthal_mean(f, model=m, **c.kw)
    for kw, word in ((dict(Nr=0), b"Nr"), (dict(Nr=1025), b"Nr"), (dict(mm=0), b"m must"), (dict(mm=17), b"m must"), (dict(radius=0.0), b"radius"),
                     (dict(radius=-1.0), b"radius")):
        assert _raw_call(m, f, **kw) == 1          # BZ_ERR_INVALID
        assert word in m._lib.bz_last_error(m._ctx), (kw, m._lib.bz_last_error(m._ctx))
    after = c.bz.azimuthal_mean(f, model=m, **c.kw)
    assert np.array_equal(_bits(before.data), _bits(after.data)) and np.array_equal(before.counts, after.counts)


def test_flat_y_contexts_are_unsupported(bz):
    grid = bz.RectilinearGrid((24, 6), x=(0.0, 2.4e3), z=(0.0, 2400.0), topology=("Periodic", "Flat", "Bounded"))
    m = bz.AtmosphereModel(grid, advection=bz.WENO(order=5))
    assert _raw_call(m, m.temperature) == 2          # BZ_ERR_UNSUPPORTED
    assert b"Flat" in m._lib.bz_last_error(m._ctx)
    with pytest.raises(NotImplementedError):
        bz.azimuthal_mean(m.temperature, radius=1.0, Nr=8)
    assert np.isfinite(bz.horizontal_average(m, m.temperature)).all()          # the context is still usable


def test_slab_contexts_are_unsupported(bz):
    from breeze_jl_amd import _lib
    from breeze_jl_amd.thermodynamics import dry_air_gas_constant, vapor_gas_constant
    import torch
    lib = _lib.load()
    grid = bz.RectilinearGrid((16, 8, 8), x=(0, 1.6e3), y=(0, 800.0), z=(0, 800.0))
    c, ref = bz.ThermodynamicConstants(), bz.ReferenceState(grid)
    zf = np.ascontiguousarray(grid.zᶠ, dtype=F64)
    bg = _lib.bz_grid()
    bg.Nx, bg.Ny, bg.Nz, bg.Hx, bg.Hy, bg.Hz = grid.Nx, grid.Ny, grid.Nz, grid.Hx, grid.Hy, grid.Hz
    for d, t in enumerate(grid.topology_codes()):
        bg.topo[d] = t
    bg.ftype, bg.dx, bg.dy, bg.regular_z = 8, grid.Δx, grid.Δy, 1
    bg.zf = zf.ctypes.data_as(C.POINTER(C.c_double))
    bc = _lib.bz_constants(c.gravitational_acceleration, dry_air_gas_constant(c), vapor_gas_constant(c), c.dry_air_heat_capacity,
                           c.vapor_heat_capacity)
    arrays = [np.ascontiguousarray(a, dtype=F64) for a in (ref.density, ref.pressure, ref.temperature)]
    br = _lib.bz_reference_state(ref.surface_pressure, ref.potential_temperature, ref.standard_pressure,
                                 *[a.ctypes.data_as(C.POINTER(C.c_double)) for a in arrays])
    ctx = C.c_void_p()
    assert lib.bz_create_slab(C.byref(ctx), C.byref(bg), C.byref(bc), C.byref(br), 5, 1, 0) == 0
    try:
        field = torch.zeros(grid.parent_shape(), dtype=torch.float64, device="cuda:0")
        prof, counts = np.zeros(grid.Nz * 8), np.zeros(8, np.int64)
        rc = lib.bz_azimuthal_mean(ctx, C.c_void_p(field.data_ptr()), 0, 0.0, 0.0, 500.0, 8, 4, prof.ctypes.data_as(C.POINTER(C.c_double)),
                                   counts.ctypes.data_as(C.POINTER(C.c_int64)))
        assert rc == 2          # BZ_ERR_UNSUPPORTED
        assert b"slab" in lib.bz_last_error(ctx)
        avg = np.zeros(grid.Nz)
        assert lib.bz_horizontal_average(ctx, C.c_void_p(field.data_ptr()), 0, avg.ctypes.data_as(C.POINTER(C.c_double))) == 2
    finally:
        lib.bz_destroy(ctx)
