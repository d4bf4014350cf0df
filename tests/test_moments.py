"""bz_horizontal_moments on the device (csrc/bz_moments.hip; breeze.jl_amd/diagnostics.py: Average of expressions, compute_averages) against
the numpy restatement tests/moments_reference.py.

Inputs.  Random O(1) fields with O(1) variation and a non-zero mean, x / y halos periodic, the first z halo level on either side
overwritten with arbitrary finite values (as a boundary condition would), every halo cell two or more cells from the interior NaN: a
finite result at every level proves that no such cell is read.
Bound.  Every level of every profile within (Nx·Ny + 32)·eps·A_k of the restatement evaluated in np.longdouble (Float32 twin: in float64),
A_k the restatement's absolute majorant: Nx·Ny·eps is the first-order bound of any summation order, 32 exceeds the 29 roundings of the
longest admissible term (three cubed factors each under an eight-point mean, two products, an eight-point @at), eps that of the context's
type.
Shapes.  40 × 24 × 10 (Nx no multiple of a wave), 300 × 5 × 3 (Nx above one block's stride of 256, Ny below the 16 row slices),
48 × 1 × 8 on (Periodic, Flat, Bounded), 40 × 24 × 10 on the Float32 twin, a compressible model's u, w, ρ, a (Periodic, Bounded, Bounded)
context.

Measured on the MI355X: worst error / bound 0.0015 (40 × 24 × 10), 0.00067 (300 × 5 × 3), 0.013 (Flat y), 0.0017 (Float32
twin); through compute_averages on a set model state 0.0013 (Float64) and 0.0018 (Float32)."""
import ctypes as C

import numpy as np
import pytest

import moments_reference as mr

pytestmark = pytest.mark.gpu

F64, F32 = np.float64, np.float32
C_, FX, FY, FZ = (0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)
LOCS = (FX, FY, FZ, C_, C_)          # u, v, w, θ, νₑ
U, V, W, TH, NU = range(5)
M = mr.Moment
# examples/neutral_atmospheric_boundary_layer.jl:203-221 of the reference: 18 profiles of five fields, all under @at((Center, Center, Center), ·)
ABL = ([M(((f, 1),), False, True) for f in (U, V, W, TH, NU)] +
       [M(((f, 2),), False, True) for f in (U, V, W)] +
       [M(((U, 1), (W, 1)), False, True), M(((V, 1), (W, 1)), False, True), M(((TH, 1), (W, 1)), False, True),
        M(((U, 2), (W, 1)), False, True), M(((V, 2), (W, 1)), False, True), M(((W, 3),), False, True), M(((NU, 3),), False, True)] +
       [M(((f, 1),), True, True) for f in (U, V, TH)])
MOMENTS = ABL + [M(((U, 1), (V, 1), (W, 1))), M(((W, 1), (TH, 1))), M(((W, 1),), True)]          # u*v*w, w*θ without at, ∂z of a face field
assert len(ABL) == 18 and len(MOMENTS) == 21

CASES = {          # name: (size, topology, float type)
    "40x24x10": ((40, 24, 10), ("Periodic", "Periodic", "Bounded"), F64),
    "300x5x3": ((300, 5, 3), ("Periodic", "Periodic", "Bounded"), F64),
    "flat_48x8": ((48, 8), ("Periodic", "Flat", "Bounded"), F64),
    "f32_40x24x10": ((40, 24, 10), ("Periodic", "Periodic", "Bounded"), F32),
}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == F64 else np.uint32)


def _loc_classes(loc):
    from breeze_jl_amd.grids import Center, Face
    return tuple(Face if l else Center for l in loc)


def horizontal_moments(bz, model, fields, moments, sentinel=None):
    """One bz_horizontal_moments call on [(Field, loc), ...]: (rc, [profile of nlev values, ...], message)"""
    from breeze_jl_amd import _lib
    T = model._T
    fs = (_lib.bz_moment_field * max(len(fields), 1))()
    for n, (f, loc) in enumerate(fields):
        fs[n].data = f.ptr() if f is not None else None
        fs[n].face_x, fs[n].face_y, fs[n].face_z = loc
    ds = (_lib.bz_moment * max(len(moments), 1))()
    for n, m in enumerate(moments):
        m = M(*m)
        ds[n].n_factors = len(m.factors)
        for q, (f, p) in enumerate(m.factors[:3]):
            ds[n].field[q], ds[n].power[q] = f, p
        ds[n].dz, ds[n].at_center = int(m.dz), int(m.at_center)
    prof = np.full((max(len(moments), 1), model.grid.Nz + 1), np.nan if sentinel is None else sentinel, dtype=T.np_real)
    nlev = (C.c_int32 * max(len(moments), 1))()
    rc = model._lib.bz_horizontal_moments(model._ctx, len(fields), fs, len(moments), ds, prof.ctypes.data_as(C.POINTER(T.real)), nlev)
    msg = model._lib.bz_last_error(model._ctx).decode()
    if rc != 0:
        return rc, prof, msg
    return rc, [prof[n, :nlev[n]].copy() for n in range(len(moments))], msg


class Case:
    def __init__(self, bz, name):
        size, topology, self.real = CASES[name]
        ext = dict(x=(0.0, 4000.0), z=(0.0, 1000.0)) if topology[1] == "Flat" else dict(x=(0.0, 4000.0), y=(0.0, 2400.0), z=(0.0, 1000.0))
        self.bz, self.name = bz, name
        self.grid = g = bz.RectilinearGrid(size, topology=topology, float_type=self.real, **ext)
        self.model = bz.AtmosphereModel(g, advection=bz.WENO(order=5))
        self.geo = mr.geometry(g)
        self.rng = np.random.default_rng(sum(map(ord, name)))
        self.parents = [self.parent(loc, self.random_interior(loc)) for loc in LOCS]
        self.fields = [(self.upload(P, loc), loc) for P, loc in zip(self.parents, LOCS)]
        self._want = None

    def random_interior(self, loc):
        shape = (self.geo.Nz + loc[2], self.geo.Ny, self.geo.Nx)
        return (self.rng.uniform(0.5, 2.0) * (1.0 + self.rng.standard_normal(shape))).astype(self.real)          # O(1) mean and variation

    def parent(self, loc, interior):
        return mr.fill_parent(self.geo, loc, interior, z_halo=lambda s: self.rng.uniform(-2.0, 2.0, s).astype(self.real))

    def upload(self, P, loc):
        import torch
        f = self.bz.Field(self.grid, _loc_classes(loc), self.model.device)
        assert tuple(f.parent.shape) == P.shape and np.isnan(P).any()
        f.parent.copy_(torch.from_numpy(P))
        return f

    def device(self, moments=MOMENTS, fields=None):
        rc, profs, msg = horizontal_moments(self.bz, self.model, self.fields if fields is None else fields, moments)
        assert rc == 0, (rc, msg)
        return profs

    def want(self):
        """(restatement in higher precision, absolute majorant) per moment of MOMENTS: computed once"""
        if self._want is None:
            self._want = reference(self.geo, list(zip(self.parents, LOCS)), MOMENTS)
        return self._want


def reference(geo, fields, moments):
    return [(mr.profile(geo, fields, m, precise=True), mr.profile(geo, fields, m, precise=True, majorant=True)) for m in moments]


def check(geo, real, got, want, what):
    """every level of every profile within (Nx Ny + 32) eps A_k of the restatement; returns the worst error / bound"""
    eps = np.finfo(real).eps
    worst = 0.0
    assert len(got) == len(want)
    for n, (g, (ref, A)) in enumerate(zip(got, want)):
        assert g.shape == ref.shape and g.dtype == real, (what, n, g.shape, ref.shape)          # no level skipped
        assert np.all(np.isfinite(g)), (what, n, g)                                              # no NaN cell was read
        bound = (geo.Nx * geo.Ny + 32) * eps * A
        err = np.abs(g.astype(ref.dtype) - ref)
        assert np.all(err <= bound), (what, n, float(np.max(err - bound)), g, ref)
        ratio = (err[bound > 0] / bound[bound > 0]).max() if np.any(bound > 0) else 0.0
        worst = max(worst, float(ratio))
    return worst


@pytest.fixture(scope="module")
def cases(bz):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Case(bz, name)
        return made[name]
    return get


# ---- 1. the full list against the restatement --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_every_level_of_every_profile_is_within_the_bound_of_the_restatement(cases, name):
    c = cases(name)
    got = c.device()
    for m, g in zip(MOMENTS, got):
        Lz = mr.moment_location(c.geo, list(zip(c.parents, LOCS)), m)[2]
        assert len(g) == c.geo.Nz + (1 if (Lz and not m.at_center) else 0)
    worst = check(c.geo, c.real, got, c.want(), name)
    print(f"MOMENTS {name}: worst error / bound {worst:.3g}")


# ---- 2. wrap and edge indexing ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["40x24x10", "flat_48x8"])
def test_planted_single_cells_at_the_edges_reproduce_the_restatement(cases, name):
    c = cases(name)
    geo = c.geo
    for plant in ((0, 0, 0), (geo.Nx - 1, geo.Ny - 1, geo.Nz - 1), (0, geo.Ny - 1, geo.Nz - 1), (geo.Nx - 1, 0, 0)):
        i, j, k = plant
        parents = []
        for n, loc in enumerate(LOCS):
            interior = np.zeros((geo.Nz + loc[2], geo.Ny, geo.Nx), dtype=c.real)
            interior[k, j, i] = 1.25 + 0.5 * n
            parents.append(c.parent(loc, interior))
        fields = [(c.upload(P, loc), loc) for P, loc in zip(parents, LOCS)]
        got = c.device(fields=fields)
        check(geo, c.real, got, reference(geo, list(zip(parents, LOCS)), MOMENTS), (name, plant))
        assert any(np.any(g != 0) for g in got)


# ---- 3. determinism -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["40x24x10", "f32_40x24x10", "300x5x3"])
def test_fused_single_reversed_and_repeated_calls_give_the_same_bits(cases, name):
    c = cases(name)
    fused = c.device()
    again = c.device()
    backwards = c.device(MOMENTS[::-1])[::-1]
    for n, m in enumerate(MOMENTS):
        alone = c.device([m])[0]
        assert np.array_equal(_bits(fused[n]), _bits(alone)), (n, m)
        assert np.array_equal(_bits(fused[n]), _bits(again[n])) and np.array_equal(_bits(fused[n]), _bits(backwards[n])), (n, m)
    # ... and with the fields numbered the other way round
    order = [4, 3, 2, 1, 0]
    fields = [c.fields[o] for o in order]
    renumbered = [M(tuple((order.index(f), p) for f, p in m.factors), m.dz, m.at_center) for m in MOMENTS]
    for a, b in zip(fused, c.device(renumbered, fields)):
        assert np.array_equal(_bits(a), _bits(b))


# ---- 4. the Python interface ----------------------------------------------------------------------------------------------------------------
def _set_les_state(model, Lx, Ly):
    kx, ky = 2 * np.pi / Lx, 2 * np.pi / Ly
    model.set(θ=lambda x, y, z: 300.0 + 2e-3 * z + np.sin(kx * x) * np.cos(2 * ky * y),
              u=lambda x, y, z: 5.0 + np.sin(2 * kx * x + ky * y) + 1e-3 * z, v=lambda x, y, z: -2.0 + np.cos(kx * x) * np.sin(ky * y) + 0 * z,
              w=lambda x, y, z: np.sin(kx * x + 0.3) * np.cos(ky * y) * np.sin(np.pi * z / 1000.0))


def _model_fields(model):
    v = model.velocities
    return [v["u"], v["v"], v["w"], model.potential_temperature, model.temperature]


@pytest.mark.parametrize("real", [F64, F32])
def test_the_example_lists_evaluate_through_compute_averages(bz, real):
    from breeze_jl_amd.grids import Center
    CCC = (Center, Center, Center)
    grid = bz.RectilinearGrid((40, 24, 10), x=(0.0, 4000.0), y=(0.0, 2400.0), z=(0.0, 1000.0), float_type=real)
    model = bz.AtmosphereModel(grid, advection=bz.WENO(order=5))
    _set_les_state(model, 4000.0, 2400.0)
    u, v, w, θ, νₑ = _model_fields(model)          # (the temperature stands in for νₑ: any centre field)
    at, dz, Average = bz.at, bz.partial_z, bz.Average
    outputs = {          # neutral_atmospheric_boundary_layer.jl:203-221, then rico.jl:281-282 / tropical_cyclone_world.jl:244-249
        "u": u, "v": v, "w": w, "θ": θ, "νₑ": νₑ, "uu": u ** 2, "vv": v ** 2, "ww": w ** 2,
        "uw": u * w, "vw": v * w, "θw": θ * w, "uuw": u ** 2 * w, "vvw": v ** 2 * w, "www": w ** 3, "ννν": νₑ ** 3,
        "∂z_u": dz(u), "∂z_v": dz(v), "∂z_θ": dz(θ)}
    averages = {name: Average(at(CCC, e), dims=(1, 2), model=model) for name, e in outputs.items()}
    extra = {"uvw": Average(u * v * w), "wθ": Average(w * θ), "∂z_w": Average(dz(w)), "θ_plain": Average(θ), "w_plain": Average(w),
             "θᵛw": Average(bz.VirtualPotentialTemperature(model) * w)}
    got = bz.compute_averages(model, {**averages, **extra})          # 24 moments over 6 fields: one call
    assert list(got) == list(averages) + list(extra)
    geo = mr.geometry(grid)
    θᵛ = bz.VirtualPotentialTemperature(model).compute()
    parents = [(f.parent.cpu().numpy(), loc) for f, loc in zip((u, v, w, θ, νₑ, θᵛ), LOCS + (C_,))]
    moments = MOMENTS + [M(((TH, 1),)), M(((W, 1),)), M(((5, 1), (W, 1)))]
    worst = check(geo, real, list(got.values()), reference(geo, parents, moments), f"compute_averages {real.__name__}")
    print(f"MOMENTS compute_averages {real.__name__}: worst error / bound {worst:.3g}")
    # a single expression through Average(...).compute() is the same call
    assert np.array_equal(_bits(Average(at(CCC, u ** 2 * w)).compute()), _bits(got["uuw"]))
    # plain fields keep the bz_horizontal_average path and its bits; the fused call gives the same bits
    for f, name in ((θ, "θ_plain"), (w, "w_plain")):
        plain = bz.horizontal_average(model, f)
        assert np.array_equal(_bits(Average(f).compute()), _bits(plain))
        assert np.array_equal(_bits(got[name]), _bits(plain))


def test_dims_one_on_a_flat_y_is_the_horizontal_average(bz):
    grid = bz.RectilinearGrid((48, 8), x=(0.0, 4000.0), z=(0.0, 1000.0), topology=("Periodic", "Flat", "Bounded"))
    model = bz.AtmosphereModel(grid, advection=bz.WENO(order=5))
    model.set(θ=lambda x, z: 300.0 + 2e-3 * z + np.sin(2 * np.pi * x / 4000.0), u=lambda x, z: 5.0 + np.sin(4 * np.pi * x / 4000.0) + 1e-3 * z,
              w=lambda x, z: np.sin(2 * np.pi * x / 4000.0 + 0.3) * np.sin(np.pi * z / 1000.0))
    u, w, θ = model.velocities["u"], model.velocities["w"], model.potential_temperature
    got = bz.compute_averages(model, {"uw": bz.Average(u * w, dims=1), "wθ": bz.Average(w * θ, dims=(1, 2))})
    geo = mr.geometry(grid)
    parents = [(f.parent.cpu().numpy(), loc) for f, loc in ((u, FX), (w, FZ), (θ, C_))]
    check(geo, F64, list(got.values()), reference(geo, parents, [M(((0, 1), (1, 1))), M(((1, 1), (2, 1)))]), "flat dims=1")
    assert np.array_equal(_bits(bz.Average(θ, dims=1).compute()), _bits(bz.horizontal_average(model, θ)))


# ---- 5. other contexts ------------------------------------------------------------------------------------------------------------------------
def test_one_call_on_a_compressible_models_u_w_and_density(bz):
    grid = bz.RectilinearGrid((16, 16, 8), x=(0, 16e3), y=(0, 16e3), z=(0, 8e3))
    dyn = bz.CompressibleDynamics(bz.SplitExplicitTimeDiscretization(substeps=6), reference_potential_temperature=300.0)
    model = bz.CompressibleAtmosphereModel(grid, dyn, advection=bz.WENO(order=5))
    ref = dyn.reference_state
    sl = slice(grid.Hz, grid.Hz + grid.Nz)
    model.set(ρ=lambda x, y, z: np.interp(z, grid.zᶜ, ref.density[sl]) * (1 + 0.01 * np.sin(2 * np.pi * x / 16e3)) + 0 * y,
              θ=lambda x, y, z: 300.0 + 2.0 * np.cos(2 * np.pi * y / 16e3) + 1e-3 * z + 0 * x,
              u=lambda x, y, z: 3.0 + np.sin(2 * np.pi * (x + y) / 16e3) + 0 * z, v=0.0,
              w=lambda x, y, z: np.sin(2 * np.pi * (x + y) / 16e3) * np.sin(np.pi * z / 8e3))
    u, w, ρ = model.velocities["u"], model.velocities["w"], dyn.total_density
    from breeze_jl_amd.grids import Center
    CCC = (Center, Center, Center)
    got = bz.compute_averages(model, {"uw": bz.Average(bz.at(CCC, u * w), model=model), "ρw": bz.Average(ρ * w, model=model),
                                      "ρuw": bz.Average(ρ * u * w, model=model), "∂z_ρ": bz.Average(bz.partial_z(ρ), model=model),
                                      "w²": bz.Average(w ** 2, model=model)})
    geo = mr.geometry(grid)
    parents = [(f.parent.cpu().numpy(), loc) for f, loc in ((u, FX), (w, FZ), (ρ, C_))]
    moments = [M(((0, 1), (1, 1)), False, True), M(((2, 1), (1, 1))), M(((2, 1), (0, 1), (1, 1))), M(((2, 1),), True), M(((1, 2),))]
    check(geo, F64, list(got.values()), reference(geo, parents, moments), "compressible")
    assert np.abs(got["uw"]).max() > 0.1          # ⟨u w⟩ = sin(π z / H) / 2 up to the discrete means


def test_walls_run_centred_moments_and_refuse_horizontal_faces(bz):
    # (the walled pressure solve needs Nx a power of two and Ny a multiple of 8)
    grid = bz.RectilinearGrid((32, 16, 10), x=(0, 3200.0), y=(0, 1600.0), z=(0, 3000.0), topology=("Periodic", "Bounded", "Bounded"))
    model = bz.AtmosphereModel(grid, advection=bz.WENO(order=5))
    geo = mr.geometry(grid)
    rng = np.random.default_rng(7)
    import torch
    parents, fields = [], []
    for loc in (C_, FZ, FX):
        P = mr.fill_parent(geo, loc, 1.0 + rng.standard_normal((geo.Nz + loc[2], geo.Ny, geo.Nx)), z_halo=lambda s: rng.uniform(-2.0, 2.0, s))
        f = bz.Field(grid, _loc_classes(loc), model.device)
        f.parent.copy_(torch.from_numpy(P))
        parents.append((P, loc))
        fields.append((f, loc))
    moments = [M(((0, 1), (0, 1))), M(((0, 2), (1, 1)), False, True), M(((0, 1),), True), M(((1, 3),))]          # θ*θ, θ²*w at centres, ∂z(θ), w³
    rc, got, msg = horizontal_moments(bz, model, fields, moments)
    assert rc == 0, msg
    check(geo, F64, got, reference(geo, parents, moments), "walls")
    from breeze_jl_amd import _lib
    for bad in ([M(((2, 1), (1, 1)))], [M(((0, 1), (0, 1))), M(((0, 1), (2, 1)))], [M(((2, 1),), False, True)]):          # u*w, θ*u, at(CCC, u)
        rc, prof, msg = horizontal_moments(bz, model, fields, bad, sentinel=-7.0)
        assert rc == 2 and "bz_horizontal_moments" in msg and "walls" in msg, (rc, msg)
        assert np.all(prof == -7.0)


def test_bad_descriptors_return_invalid_with_a_message_and_launch_nothing(cases, bz):
    from breeze_jl_amd import _lib
    c = cases("40x24x10")
    good = M(((U, 1), (W, 1)))
    bad_lists = {
        "field index past n_fields": [good, M(((5, 1),))],
        "negative field index": [M(((-1, 1),))],
        "power 0": [M(((U, 0),))],
        "power 4": [good, M(((U, 1), (W, 4)))],
        "dz with two factors": [M(((U, 1), (W, 1)), True)],
        "dz with a power": [M(((U, 2),), True)],
        "no factor": [M((), False, False)],
        "dz = 2": [M(((U, 1),), 2)],
        "at_center = -1": [M(((U, 1),), False, -1)],
        "too many moments": [good] * (_lib.BZ_MAX_MOMENTS + 1),
        "no moments": [],
    }
    for what, moments in bad_lists.items():
        rc, prof, msg = horizontal_moments(bz, c.model, c.fields, moments, sentinel=-7.0)
        assert rc == 1 and msg.startswith("bz_horizontal_moments:"), (what, rc, msg)
        assert np.all(prof == -7.0), what
    for what, fields in (("too many fields", c.fields + c.fields[:4]), ("no fields", []), ("null data", [(None, C_)] + c.fields[1:]),
                         ("face flag 2", [(c.fields[0][0], (2, 0, 0))] + c.fields[1:])):
        rc, prof, msg = horizontal_moments(bz, c.model, fields, [M(((0, 1),))], sentinel=-7.0)
        assert rc == 1 and msg.startswith("bz_horizontal_moments:"), (what, rc, msg)
        assert np.all(prof == -7.0), what
    # four factors cannot be written into a descriptor; n_factors = 4 is refused as well
    T = c.model._T
    fs = (_lib.bz_moment_field * 1)()
    fs[0].data = c.fields[0][0].ptr()
    d = (_lib.bz_moment * 1)()
    d[0].n_factors = 4
    prof, nlev = np.zeros(c.geo.Nz + 1, dtype=T.np_real), (C.c_int32 * 1)()
    assert c.model._lib.bz_horizontal_moments(c.model._ctx, 1, fs, 1, d, prof.ctypes.data_as(C.POINTER(T.real)), nlev) == 1
    # the context still works
    assert len(c.device([good])[0]) == c.geo.Nz
