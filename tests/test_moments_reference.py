"""tests/moments_reference.py (the numpy restatement of bz_horizontal_moments) pinned by closed forms and by two identities of periodic
grids, and the host side of the feature: the expression builder behind `u ** 2 * w`, `partial_z(θ)`, `at((Center, Center, Center), ·)`,
the descriptors it produces for the profile lists of the reference's examples, its refusals, the dims rule and the exports.  No GPU."""
import ctypes as C
import re

import numpy as np
import pytest

import moments_reference as mr

F64, F32 = np.float64, np.float32
C_, FX, FY, FZ = (0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)


def _geo(Nx=12, Ny=6, Nz=5, H=3, flat=False, zf=None):
    zf = np.linspace(0.0, 2.0, Nz + 1) if zf is None else np.asarray(zf)
    dzc, dzf = mr.spacings(zf)
    return mr.Geometry(Nx, 1 if flat else Ny, Nz, H, 0 if flat else H, H, flat, dzc, dzf)


def _random_fields(geo, seed=0, dtype=F64):
    rng = np.random.default_rng(seed)
    out = []
    for loc in (FX, FY, FZ, C_, C_):
        nlev = geo.Nz + loc[2]
        interior = (1.5 + rng.standard_normal((nlev, geo.Ny, geo.Nx))).astype(dtype)
        out.append((mr.fill_parent(geo, loc, interior, z_halo=lambda s: rng.standard_normal(s) + 0.5), loc))
    return out


# ---- closed forms ----------------------------------------------------------------------------------------------------------------------
def test_spacings_of_a_regular_and_a_stretched_column():
    dzc, dzf = mr.spacings([0.0, 1.0, 2.0, 3.0])
    assert np.array_equal(dzc, [1, 1, 1]) and np.array_equal(dzf, [1, 1, 1, 1])
    dzc, dzf = mr.spacings([0.0, 1.0, 3.0, 7.0])
    assert np.array_equal(dzc, [1, 2, 4]) and np.array_equal(dzf, [1, 1.5, 3, 4])


@pytest.mark.parametrize("flat", [False, True])
def test_constant_fields_give_the_product_of_the_constants_at_every_level(flat):
    geo = _geo(flat=flat)
    a, b, c = 1.5, -2.0, 0.25          # every product and mean below is exact in binary
    fields = []
    for loc, val in ((FX, a), (FY, b), (FZ, c)):
        nlev = geo.Nz + loc[2]
        fields.append((mr.fill_parent(geo, loc, np.full((nlev, geo.Ny, geo.Nx), val), z_halo=val), loc))
    for m, want, nlev in ((mr.Moment(((0, 2), (2, 1)), False, True), a * a * c, geo.Nz),
                          (mr.Moment(((0, 1), (1, 1), (2, 1))), a * b * c, geo.Nz),
                          (mr.Moment(((2, 3),)), c ** 3, geo.Nz + 1),
                          (mr.Moment(((2, 3),), False, True), c ** 3, geo.Nz),
                          (mr.Moment(((2, 1), (0, 3))), c * a ** 3, geo.Nz + 1),
                          (mr.Moment(((0, 1),), True, True), 0.0, geo.Nz)):
        got = mr.profile(geo, fields, m)
        assert got.shape == (nlev,) and np.all(got == want), (m, got)
    assert np.all(mr.profile(geo, fields, mr.Moment(((0, 1), (1, 1), (2, 1))), majorant=True) == abs(a * b * c))


def test_dz_of_a_profile_linear_in_z_is_its_slope():
    zf = np.array([0.0, 0.5, 1.5, 2.0, 4.0, 5.0])
    geo = _geo(Nz=5, zf=zf)
    zc = (zf[:-1] + zf[1:]) / 2
    s = 3.0
    # centre field: the boundary faces take the mirrored centres z_c[-1], z_c[Nz]
    below, above = zc[0] - geo.dzf[0], zc[-1] + geo.dzf[-1]
    P = mr.fill_parent(geo, C_, np.broadcast_to((s * zc)[:, None, None], (5, geo.Ny, geo.Nx)).copy())
    P[geo.Hz - 1], P[geo.Hz + 5] = s * below, s * above
    got = mr.profile(geo, [(P, C_)], mr.Moment(((0, 1),), True))
    assert got.shape == (6,) and np.max(np.abs(got - s)) < 1e-14
    assert np.max(np.abs(mr.profile(geo, [(P, C_)], mr.Moment(((0, 1),), True, True)) - s)) < 1e-14
    # face field -> centres
    Pf = mr.fill_parent(geo, FZ, np.broadcast_to((s * zf)[:, None, None], (6, geo.Ny, geo.Nx)).copy())
    got = mr.profile(geo, [(Pf, FZ)], mr.Moment(((0, 1),), True))
    assert got.shape == (5,) and np.max(np.abs(got - s)) < 1e-14
    maj = mr.profile(geo, [(Pf, FZ)], mr.Moment(((0, 1),), True), majorant=True)
    assert np.allclose(maj, s * (zf[1:] + zf[:-1]) / geo.dzc)


@pytest.mark.parametrize("m", [1, 2, 5])
def test_discrete_sine_pair_has_the_closed_form_cos_over_two(m):
    """u = sin(2π m i / N) on x faces, w = sin(2π m (i + ½) / N) on centres: ℑx(w) at face i = cos(π m / N) sin(2π m i / N), so
    ⟨u ℑx(w)⟩ = cos(π m / N) / 2 for 0 < m < N / 2."""
    N = 16
    geo = _geo(Nx=N, Ny=4, Nz=3)
    i = np.arange(N)
    u = np.broadcast_to(np.sin(2 * np.pi * m * i / N), (geo.Nz, geo.Ny, N)).copy()
    w = np.broadcast_to(np.sin(2 * np.pi * m * (i + 0.5) / N), (geo.Nz + 1, geo.Ny, N)).copy()
    fields = [(mr.fill_parent(geo, FX, u), FX), (mr.fill_parent(geo, FZ, w, z_halo=lambda s: np.nan), FZ)]
    want = np.cos(np.pi * m / N) / 2
    for at_center in (False, True):
        got = mr.profile(geo, fields, mr.Moment(((0, 1), (1, 1)), False, at_center))
        assert got.shape == (geo.Nz,) and np.max(np.abs(got - want)) < 1e-15 * N, got - want


# ---- identities of periodic grids ---------------------------------------------------------------------------------------------------------
MOMENTS_AT_HORIZONTAL_FACES = [((0, 1),), ((0, 2), (2, 1)), ((1, 1), (2, 1)), ((1, 2), (3, 1)), ((0, 1), (1, 1), (4, 1))]
MOMENTS_AT_Z_FACES = [((2, 1),), ((2, 3),), ((2, 1), (3, 1)), ((2, 2), (0, 1))]


@pytest.mark.parametrize("factors", MOMENTS_AT_HORIZONTAL_FACES)
@pytest.mark.parametrize("dtype", [F64, F32])
def test_centring_a_horizontal_face_moment_keeps_its_average(factors, dtype):
    geo = _geo()
    fields = _random_fields(geo, 3, dtype)
    plain = mr.profile(geo, fields, mr.Moment(factors), precise=True)
    centred = mr.profile(geo, fields, mr.Moment(factors, False, True), precise=True)
    A = mr.profile(geo, fields, mr.Moment(factors), precise=True, majorant=True)
    eps = np.finfo(np.float64 if dtype == F32 else mr.L).eps
    assert np.all(np.abs(plain - centred) <= (geo.Nx * geo.Ny + 32) * eps * A)


@pytest.mark.parametrize("factors", MOMENTS_AT_Z_FACES)
def test_centring_a_z_face_moment_averages_adjacent_levels(factors):
    geo = _geo()
    fields = _random_fields(geo, 4)
    plain = mr.profile(geo, fields, mr.Moment(factors), precise=True)
    centred = mr.profile(geo, fields, mr.Moment(factors, False, True), precise=True)
    A = mr.profile(geo, fields, mr.Moment(factors), precise=True, majorant=True)
    assert plain.shape == (geo.Nz + 1,) and centred.shape == (geo.Nz,)
    eps = np.finfo(mr.L).eps
    assert np.all(np.abs((plain[:-1] + plain[1:]) / 2 - centred) <= (geo.Nx * geo.Ny + 32) * eps * (A[:-1] + A[1:]) / 2)


def test_cells_two_or_more_from_the_interior_are_never_read():
    geo = _geo()
    fields = _random_fields(geo, 5)          # far cells are NaN
    for factors in MOMENTS_AT_HORIZONTAL_FACES + MOMENTS_AT_Z_FACES:
        for at_center in (False, True):
            assert np.all(np.isfinite(mr.profile(geo, fields, mr.Moment(factors, False, at_center))))
    for f in range(5):
        for at_center in (False, True):
            assert np.all(np.isfinite(mr.profile(geo, fields, mr.Moment(((f, 1),), True, at_center))))


def test_the_evaluation_in_the_input_precision_is_within_the_bound_of_the_precise_one():
    geo = _geo()
    for dtype in (F64, F32):
        fields = _random_fields(geo, 6, dtype)
        for factors in MOMENTS_AT_HORIZONTAL_FACES + MOMENTS_AT_Z_FACES:
            m = mr.Moment(factors, False, True)
            own, ref = mr.profile(geo, fields, m), mr.profile(geo, fields, m, precise=True)
            A = mr.profile(geo, fields, m, precise=True, majorant=True)
            assert own.dtype == dtype
            assert np.all(np.abs(own.astype(ref.dtype) - ref) <= (geo.Nx * geo.Ny + 32) * np.finfo(dtype).eps * A)


# ---- the expression builder ---------------------------------------------------------------------------------------------------------------
class _Model:
    def __init__(self, grid):
        self.grid = grid


@pytest.fixture(scope="module")
def les(bz):
    from breeze_jl_amd.grids import Center, Face
    g = bz.RectilinearGrid((8, 8, 4), x=(0, 1), y=(0, 1), z=(0, 1))
    m = _Model(g)
    f = {n: bz.Field(g, loc, "cpu") for n, loc in (("u", (Face, Center, Center)), ("v", (Center, Face, Center)), ("w", (Center, Center, Face)),
                                                   ("θ", (Center, Center, Center)), ("νₑ", (Center, Center, Center)),
                                                   ("qᵛ", (Center, Center, Center)))}
    return bz, m, f, (Center, Center, Center)


def _keys(bz, model, outputs):
    return {name: bz.Average(expr, dims=(1, 2), model=model).moment.key() for name, expr in outputs.items()}


def test_the_abl_list_lowers_onto_eighteen_descriptors_over_five_fields(les):
    bz, m, f, CCC = les
    u, v, w, θ, νₑ = f["u"], f["v"], f["w"], f["θ"], f["νₑ"]
    at, dz = bz.at, bz.partial_z
    outputs = {          # examples/neutral_atmospheric_boundary_layer.jl:203-221 of the reference, in its order
        "uu": at(CCC, u ** 2), "vv": at(CCC, v ** 2), "ww": at(CCC, w ** 2),
        "uw": at(CCC, u * w), "vw": at(CCC, v * w), "θw": at(CCC, θ * w),
        "uuw": at(CCC, u ** 2 * w), "vvw": at(CCC, v ** 2 * w), "www": at(CCC, w ** 3), "ννν": at(CCC, νₑ ** 3),
        "∂z_u": at(CCC, dz(u)), "∂z_v": at(CCC, dz(v)), "∂z_θ": at(CCC, dz(θ)),
    }
    keys = _keys(bz, m, outputs)
    assert keys["uu"] == (((FX, 2),), False, True) and keys["ww"] == (((FZ, 2),), False, True)
    assert keys["uw"] == (((FX, 1), (FZ, 1)), False, True) and keys["θw"] == (((C_, 1), (FZ, 1)), False, True)
    assert keys["vvw"] == (((FY, 2), (FZ, 1)), False, True) and keys["www"] == (((FZ, 3),), False, True)
    assert keys["ννν"] == (((C_, 3),), False, True)
    assert keys["∂z_u"] == (((FX, 1),), True, True) and keys["∂z_θ"] == (((C_, 1),), True, True)
    # with the five plain fields the list is 18 moments over 5 distinct fields: one call
    from breeze_jl_amd import diagnostics as dg
    moments = [dg.Moment([(x, 1)]) for x in (u, v, w, θ, νₑ)] + [bz.Average(e, model=m).moment for e in outputs.values()]
    assert len(moments) == 18
    calls = dg._plan_calls(moments)
    assert len(calls) == 1 and len(calls[0][0]) == 5 and calls[0][1] == list(range(18))
    index = {id(x): n for n, x in enumerate(calls[0][0])}
    d = moments[5 + 6].descriptor(index)          # u² w
    assert (d.n_factors, list(d.field)[:2], list(d.power)[:2], d.dz, d.at_center) == (2, [0, 2], [2, 1], 0, 1)
    d = moments[5 + 10].descriptor(index)         # ∂z(u)
    assert (d.n_factors, d.field[0], d.power[0], d.dz, d.at_center) == (1, 0, 1, 1, 1)


def test_the_rico_and_tropical_cyclone_lists(les):
    bz, m, f, CCC = les
    u, v, w, θ, qᵛ = f["u"], f["v"], f["w"], f["θ"], f["qᵛ"]
    keys = _keys(bz, m, {"ww": w ** 2, "uw": u * w, "vw": v * w, "wθ": w * θ, "wq": w * qᵛ})      # rico.jl:281-282, tropical_cyclone_world.jl:244-249
    assert keys["ww"] == (((FZ, 2),), False, False)
    assert keys["uw"] == (((FX, 1), (FZ, 1)), False, False) and keys["vw"] == (((FY, 1), (FZ, 1)), False, False)
    assert keys["wθ"] == (((FZ, 1), (C_, 1)), False, False) and keys["wq"] == keys["wθ"]
    assert _keys(bz, m, {"uvw": u * v * w})["uvw"] == (((FX, 1), (FY, 1), (FZ, 1)), False, False)
    assert _keys(bz, m, {"x": (u ** 3 * v ** 2) * w ** 1})["x"] == (((FX, 3), (FY, 2), (FZ, 1)), False, False)


def test_planning_splits_on_the_limits_and_deduplicates_fields(les, bz):
    from breeze_jl_amd import _lib, diagnostics as dg
    _, m, f, _ = les
    u, w = f["u"], f["w"]
    many = [dg.Moment([(u, 1), (w, 1)]) for _ in range(_lib.BZ_MAX_MOMENTS + 3)]
    calls = dg._plan_calls(many)
    assert [len(c[1]) for c in calls] == [_lib.BZ_MAX_MOMENTS, 3] and all(len(c[0]) == 2 for c in calls)
    from breeze_jl_amd.grids import Center
    extra = [bz.Field(m.grid, (Center, Center, Center), "cpu") for _ in range(_lib.BZ_MAX_MOMENT_FIELDS + 1)]
    calls = dg._plan_calls([dg.Moment([(x, 1)]) for x in extra])
    assert [len(c[0]) for c in calls] == [_lib.BZ_MAX_MOMENT_FIELDS, 1]


def test_shapes_outside_the_accepted_ones_raise_not_implemented_naming_the_shape(les):
    bz, m, f, CCC = les
    u, v, w, θ = f["u"], f["v"], f["w"], f["θ"]
    from breeze_jl_amd.grids import Center, Face
    for expr, named in ((u * (v * w), "field * (field * field)"), (u + w, "field + field"), (u - w, "field + field"),
                        (bz.partial_z(u * w), "∂z(field * field)"), ((u * w) ** 2, "(field * field) ** 2"), (u ** 4, "field ** 4"),
                        (u ** 0, "field ** 0"), (u ** 2.0, "field ** 2.0"), (u * v * w * θ, "field * field * field * field"),
                        (bz.at((Face, Center, Center), θ), "at((Face, Center, Center), field)"), (u * bz.partial_z(θ), "field * ∂z(field)"),
                        (bz.at(CCC, u) * w, "at((Center, Center, Center), field) * field"), (u * 2.0, "field * float")):
        with pytest.raises(NotImplementedError) as e:
            bz.Average(expr, dims=(1, 2), model=m)
        assert named in str(e.value), (named, str(e.value))


def test_dims_one_is_the_same_average_on_a_flat_y_and_refused_elsewhere(les):
    bz, m, f, _ = les
    g2 = bz.RectilinearGrid((8, 4), x=(0, 1), z=(0, 1), topology=("Periodic", "Flat", "Bounded"))
    from breeze_jl_amd.grids import Center, Face
    u2, w2 = bz.Field(g2, (Face, Center, Center), "cpu"), bz.Field(g2, (Center, Center, Face), "cpu")
    flat = _Model(g2)
    assert bz.Average(u2 * w2, dims=1, model=flat).moment.key() == (((FX, 1), (FZ, 1)), False, False)
    assert bz.Average(w2, dims=1, model=flat).dims == (1,) and bz.Average(w2, dims=(1, 2), model=flat).dims == (1, 2)
    for dims in (1, (1,), 2, (1, 2, 3), (2, 3)):
        with pytest.raises(NotImplementedError):
            bz.Average(f["u"] * f["w"], dims=dims, model=m)
    with pytest.raises(NotImplementedError):
        bz.Average(u2, dims=2, model=flat)
    with pytest.raises(ValueError):
        bz.Average(f["u"] * f["w"])          # no leaf knows its model


def test_slab_models_are_refused_on_the_host(les):
    bz, m, f, _ = les
    from breeze_jl_amd.compressible import SlabCompressibleModel
    from breeze_jl_amd.distributed import LibrarySlabAtmosphereModel, SlabAtmosphereModel
    for cls in (LibrarySlabAtmosphereModel, SlabAtmosphereModel, SlabCompressibleModel):
        slab = object.__new__(cls)          # no context is made: the refusal comes first
        slab.grid = m.grid
        avg = bz.Average(f["u"] * f["w"], model=slab)
        with pytest.raises(NotImplementedError):
            bz.compute_averages(slab, {"uw": avg})
        with pytest.raises(NotImplementedError):
            avg.compute()
        slab.__dict__.clear()


def test_exports_bindings_and_limits_match_the_header(bz):
    from breeze_jl_amd import _lib
    for name in ("Average", "compute_averages", "at", "partial_z"):
        assert hasattr(bz, name)
    assert "bz_horizontal_moments" in _lib.SYMBOLS
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "breeze_hip.h"), encoding="utf-8") as fh:
        code = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    for name in ("BZ_MAX_MOMENT_FIELDS", "BZ_MAX_MOMENTS", "BZ_MAX_MOMENT_FACTORS"):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, getattr(_lib, name)), code), name
    # int32 n_factors, field[3], power[3], dz, at_center; pointer + three int32 (padded to the pointer's alignment)
    assert C.sizeof(_lib.bz_moment) == 4 * (1 + 3 + 3 + 1 + 1)
    assert C.sizeof(_lib.bz_moment_field) == 8 + 3 * 4 + 4
    assert _lib.types(4).bz_moment is _lib.bz_moment and _lib.types(4).bz_moment_field is _lib.bz_moment_field
