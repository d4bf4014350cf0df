"""Device diagnostics (csrc/bz_diagnostics.hip: bz_compute_diagnostics, bz_horizontal_average; breeze.jl_amd/diagnostics.py) against the
numpy restatement tests/diagnostics_reference.py and the reference-generated doctest numbers.

Bounds.  Float64 pointwise kinds: relative 1e-12 against the Float64 restatement (the bound tests/test_surface_layer.py holds one flux
evaluation to).  Dewpoint: the solver's own criterion |p^v+(T+) - p^v| <= 1e-4 p^v on every cell that enters the iteration and
|T+_dev - T+_ref| <= 2e-4 p^v / (dp^v+/dT at T+_ref); a cell with p^v+(T) - p^v <= 0 never enters it and returns T bit for bit
(vapor_saturation.jl:320) — random cold cells are of that kind too, not only the planted ones.  Averages: eps Nx Ny mean|x| per level,
the worst case of any summation order.  Float32 twin: 4 E32 per kind, E32 the restatement's own Float32 error on the test's inputs
(max-norm of Float32 arithmetic against Float64 arithmetic on the same Float32-rounded inputs); the dewpoint residual is evaluated in
Float32 as the device evaluates it, with 4 E32(p^v+) of slack for the device's own exp / log.

Measured on the MI355X (worst over the three grids; E32 and the device's Float32 error in the units of the kind): see DESIGN.md §10."""
import ctypes as C
import zlib

import numpy as np
import pytest

import diagnostics_reference as dr

pytestmark = pytest.mark.gpu

F64, F32 = np.float64, np.float32
SENTINEL = -777.25
PFB = ("Periodic", "Flat", "Bounded")
GRIDS = {
    "20x6x5": dict(size=(20, 6, 5), halo=(3, 4, 5), x=(0.0, 2e3), y=(0.0, 600.0), z=3000.0 * np.linspace(0, 1, 6) ** 1.3),
    "130x3x7": dict(size=(130, 3, 7), x=(0.0, 13e3), y=(0.0, 300.0), z=(0.0, 2800.0)),      # crosses lanes 64 and 128, no multiple of 64
    "flat_24x1x6": dict(size=(24, 6), x=(0.0, 2.4e3), z=(0.0, 2400.0), topology=PFB),
}
KINDS = dr.NAMES
DENSITY = tuple("DENSITY_" + n for n in dr.DENSITY_FLAVOURED)


def _code(bz, name):
    from breeze_jl_amd import _lib
    if name.startswith("DENSITY_"):
        return _lib.BZ_DIAG[name[8:]] | _lib.BZ_DIAG_DENSITY_WEIGHTED
    return _lib.BZ_DIAG[name]


def _relerr(got, want):
    """max |got - want| / |want|; a cell whose reference is an exact zero (the humidity of a cell without vapour) must be zero"""
    d = np.abs(np.asarray(got, F64) - want)
    with np.errstate(all="ignore"):
        return np.max(np.where(want != 0, d / np.abs(want), np.where(d == 0, 0.0, np.inf)))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == F64 else np.uint32)


class Case:
    """A model on one of GRIDS (its context, reference columns and library) and seeded thermodynamic inputs in tensors of their own:
    interiors random with planted cells, every halo NaN."""

    def __init__(self, bz, name, real, liquid):
        import torch
        kw = dict(GRIDS[name])
        self.bz, self.real, self.name = bz, real, name
        self.grid = g = bz.RectilinearGrid(kw.pop("size"), float_type=real, **kw)
        self.model = m = bz.AtmosphereModel(g, advection=bz.WENO(order=5))
        self.lib, self.T = m._lib, m._T
        rng = np.random.default_rng(zlib.crc32(name.encode()) + int(liquid))
        sh = (g.Nz, g.Ny, g.Nx)
        ref = m.dynamics.reference_state
        sl = slice(g.Hz, g.Hz + g.Nz)
        # the inputs as the library holds them: rounded to the model's type
        self.p = ref.pressure[sl].astype(real)[:, None, None] * np.ones(sh, real)
        self.rho = ref.density[sl].astype(real)[:, None, None] * np.ones(sh, real)
        self.z = self._zc()[:, None, None] * np.ones(sh, real)
        Tc = rng.uniform(230.0, 310.0, sh)
        qv = rng.uniform(1e-3, 0.02, sh)
        ql = rng.uniform(0.0, 2e-3, sh) if liquid else np.zeros(sh)
        c64 = dr.constants()
        flat = rng.choice(Tc.size, 8, replace=False)
        self.dry = np.unravel_index(flat[:4], sh)              # planted q^v = 0
        self.wet = np.unravel_index(flat[4:], sh)              # planted H = 1.2
        qv[self.wet] = 1.2 * dr.saturation_specific_humidity(Tc, qv, ql, self.p.astype(F64), c64)[self.wet]
        qv[self.dry] = 0.0
        self.Tc, self.qv, self.ql = Tc.astype(real), qv.astype(real), ql.astype(real)
        self.qe = (self.qv + self.ql).astype(real)
        self.n_dry = 4
        self.dev = {k: self._upload(a) for k, a in (("T", self.Tc), ("qv", self.qv), ("ql", self.ql), ("qe", self.qe),
                                                    ("p", self.p), ("rho", self.rho))}
        self.liquid = liquid
        self.torch = torch

    def _zc(self):
        g, f = self.grid, self.real
        zf = np.asarray(g.zᶠ).astype(f)
        if g.regular_z:
            dz = (zf[g.Nz] - zf[0]) / f(g.Nz)
            return (zf[0] + dz * (np.arange(g.Nz).astype(f) + f(0.5))).astype(f)
        return (f(0.5) * (zf[:-1] + zf[1:])).astype(f)

    def _upload(self, interior):
        import torch
        g = self.grid
        t = torch.full(g.parent_shape(), float("nan"), dtype=self.model.temperature.dtype, device=self.model.device)
        t[g.interior_slices()] = torch.from_numpy(np.ascontiguousarray(interior)).to(t.device)
        return t

    def run(self, names, fields3d=False, liquid_as_two=False):
        """One bz_compute_diagnostics call for `names`; returns the outputs' parent arrays (numpy)."""
        import torch
        g, m = self.grid, self.model
        I = self.T.bz_diagnostic_inputs()
        I.temperature, I.vapor, I.moisture = (self.dev[k].data_ptr() for k in ("T", "qv", "qe"))
        if self.liquid:
            I.liquid = self.dev["ql"].data_ptr()
        if fields3d:
            I.pressure, I.density = self.dev["p"].data_ptr(), self.dev["rho"].data_ptr()
        c = m.thermodynamic_constants
        I.liquid_latent_heat, I.liquid_heat_capacity = c.liquid_reference_latent_heat, c.liquid_heat_capacity
        I.energy_reference_temperature = c.energy_reference_temperature
        I.triple_point_temperature, I.triple_point_pressure = c.triple_point_temperature, c.triple_point_pressure
        outs = [torch.full(g.parent_shape(), SENTINEL, dtype=m.temperature.dtype, device=m.device) for _ in names]
        n = len(names)
        kinds = (C.c_int32 * n)(*[_code(self.bz, k) for k in names])
        ptrs = (C.c_void_p * n)(*[o.data_ptr() for o in outs])
        m._check(self.lib.bz_compute_diagnostics(m._ctx, C.byref(m._state), C.byref(I), n, kinds, ptrs), "bz_compute_diagnostics")
        m.synchronize()
        return [o.cpu().numpy() for o in outs]

    def interior(self, parent):
        return parent[self.grid.interior_slices()]

    def reference(self, name, dtype=F64):
        """the restatement in `dtype` arithmetic on the inputs as the library holds them"""
        a = lambda x: x.astype(dtype)
        with np.errstate(all="ignore"):
            return dr.evaluate(name, a(self.Tc), a(self.qv), a(self.ql), a(self.p), a(self.rho), a(self.z), a(self.qe), dr.constants(dtype))


@pytest.fixture(scope="module")
def cases(bz):
    made = {}

    def get(name, real=F64, liquid=True):
        if (name, real, liquid) not in made:
            made[name, real, liquid] = Case(bz, name, real, liquid)
        return made[name, real, liquid]
    return get


def _dpsat_dT(T, c):
    dc = c.cpv - c.cl
    L0 = c.Ll - dc * c.T_energy
    return dr.saturation_vapor_pressure(T, c) * (dc / c.Rv / T + L0 / (c.Rv * T * T))


def _check_dewpoint(case, got, residual_dtype=F64, slack=0.0):
    c = dr.constants()
    T, qv, ql, p = (a.astype(F64) for a in (case.Tc, case.qv, case.ql, case.p))
    pv = dr.vapor_pressure(T, qv, ql, p, c)
    H = pv / dr.saturation_vapor_pressure(T, c)
    margin = 1e-12 if case.real is F64 else 1e-5
    sat, unsat = H >= 1 + margin, (H <= 1 - margin) & (qv > 0)
    left_out = ~(sat | unsat)
    assert left_out.sum() <= case.n_dry and np.all(qv[left_out] == 0), left_out.sum()
    assert sat[case.wet].all() and sat.sum() >= 4
    assert np.array_equal(_bits(got[sat]), _bits(case.Tc[sat]))              # T+ == T bit for bit
    cr = dr.constants(residual_dtype)
    r = lambda x: x.astype(residual_dtype)
    res = np.abs(dr.saturation_vapor_pressure(r(got), cr) - dr.vapor_pressure(r(case.Tc), r(case.qv), r(case.ql), r(case.p), cr)).astype(F64)
    worst = (res[unsat] / pv[unsat]).max()
    print(f"DEWPOINT {case.name} {case.real.__name__}: worst residual / p^v = {worst:.3e} on {unsat.sum()} cells")
    assert np.all(res[unsat] <= 1e-4 * pv[unsat] + slack)
    return unsat, pv


# ---- 1. the reference's doctest models on the device -------------------------------------------------------------------------------
def _sig(x, digits=6):
    return 0.6 * 10.0 ** (np.floor(np.log10(abs(x))) - (digits - 1))


DOCTESTS = {      # golden entry -> (operation, SaturationAdjustment?)
    "static_energy": ("StaticEnergy", False), "virtual_potential_temperature": ("VirtualPotentialTemperature", False),
    "potential_temperature": ("PotentialTemperature", False), "liquid_ice_potential_temperature": ("LiquidIcePotentialTemperature", False),
    "equivalent_potential_temperature": ("EquivalentPotentialTemperature", False),
    "stability_equivalent_potential_temperature": ("StabilityEquivalentPotentialTemperature", False),
    "dewpoint_temperature": ("DewpointTemperature", True), "relative_humidity": ("RelativeHumidity", True),
}


@pytest.mark.parametrize("entry", sorted(DOCTESTS))
def test_doctest_models_on_the_device(bz, entry):
    import json
    import os
    with open(os.path.join(os.path.dirname(__file__), "golden", "reference_doctests.json"), encoding="utf-8") as f:
        gd = json.load(f)["model_diagnostics"][entry]
    op, adjustment = DOCTESTS[entry]
    Nz = gd["inputs"]["size"][2]
    # 1 x 1 x Nz is refused by the grid constructor (halo wider than the domain): 4 x 4 x Nz as tests/test_golden_reference.py
    grid = bz.RectilinearGrid((4, 4, Nz), x=(0, 1.0), y=(0, 1.0), z=(-1000.0, 0.0))
    model = bz.AtmosphereModel(grid, advection=bz.WENO(order=5), microphysics=bz.SaturationAdjustment(equilibrium=bz.WarmPhaseEquilibrium()) if adjustment else None)
    sets = {"θ": float(gd["inputs"]["set"]["theta"])}
    if "qt" in gd["inputs"]["set"]:
        sets["qᵗ"] = float(gd["inputs"]["set"]["qt"])
    model.set(**sets)
    field = getattr(bz, op)(model).compute()
    v = field.interior_cpu()
    assert np.array_equal(v, np.broadcast_to(v[:, :1, :1], v.shape))          # a column model: every column the same bits
    digits = 5 if entry == "virtual_potential_temperature" else 6
    for key, x in (("max", v.max()), ("min", v.min()), ("mean", v[:, 0, 0].mean())):
        assert abs(x - gd[key]) <= _sig(gd[key], digits), (entry, key, x, gd[key])
    # halos filled: periodic images in x, the no-flux row in z
    P, H = field.cpu(), (grid.Hz, grid.Hy, grid.Hx)
    assert np.array_equal(P[H[0]:-H[0], H[1]:-H[1], 0], P[H[0]:-H[0], H[1]:-H[1], grid.Nx])
    assert np.array_equal(P[H[0] - 1, H[1]:-H[1], H[2]:-H[2]], P[H[0], H[1]:-H[1], H[2]:-H[2]])


# ---- 2. random thermodynamic states through the C entry point -----------------------------------------------------------------------
@pytest.mark.parametrize("liquid", [False, True], ids=["ql0", "ql"])
@pytest.mark.parametrize("name", sorted(GRIDS))
def test_random_states_against_the_restatement(cases, name, liquid):
    case = cases(name, F64, liquid)
    names = KINDS + DENSITY
    outs = case.run(names)
    inside = np.zeros(case.grid.parent_shape(), bool)
    inside[case.grid.interior_slices()] = True
    for kind, P in zip(names, outs):
        assert np.all(P[~inside] == SENTINEL), kind                          # halos untouched
        got = case.interior(P)
        if kind == "DEWPOINT_TEMPERATURE":
            continue
        want = case.reference(kind)
        err = _relerr(got, want)
        print(f"DIAG {name} ql={int(liquid)} {kind}: max relative error {err:.3e}")
        assert np.isfinite(got).all() and err <= 1e-12, (kind, err)
    got = case.interior(outs[names.index("DEWPOINT_TEMPERATURE")])
    unsat, pv = _check_dewpoint(case, got)
    want = case.reference("DEWPOINT_TEMPERATURE")
    width = 2e-4 * pv / _dpsat_dT(want, dr.constants())
    assert np.all(np.abs(got - want)[unsat] <= width[unsat])


@pytest.mark.parametrize("name", sorted(GRIDS))
def test_fused_call_equals_single_calls_bitwise(cases, name):
    case = cases(name, F64, True)
    fused = case.run(KINDS)
    for kind, P in zip(KINDS, fused):
        single = case.run([kind])[0]
        assert np.array_equal(_bits(P), _bits(single)), kind


# ---- 3. 3-D pressure / density inputs ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(GRIDS))
def test_broadcast_columns_as_fields_equal_the_column_path(cases, name):
    case = cases(name, F64, True)
    names = KINDS + DENSITY
    cols, flds = case.run(names), case.run(names, fields3d=True)
    for kind, a, b in zip(names, cols, flds):
        a, b = case.interior(a), case.interior(b)
        ok = np.isfinite(a) | np.isfinite(b)                                  # the dewpoint of a q^v = 0 cell may be NaN in both
        assert (~ok).sum() <= case.n_dry
        err = _relerr(b[ok], a[ok])
        print(f"DIAG3D {name} {kind}: {err:.3e}")
        assert err <= 1e-14, (kind, err)


def _model_inputs(model, ql_fields=()):
    g = model.grid
    T = model.temperature.interior_cpu().astype(F64)
    ql = sum((f.interior_cpu().astype(F64) for f in ql_fields), np.zeros_like(T))
    return g, T, ql


def test_compressible_model_through_the_python_interface(bz):
    grid = bz.RectilinearGrid((16, 16, 8), x=(0, 16e3), y=(0, 16e3), z=(0, 8e3))
    dyn = bz.CompressibleDynamics(bz.SplitExplicitTimeDiscretization(substeps=6), reference_potential_temperature=300.0)
    model = bz.CompressibleAtmosphereModel(grid, dyn, advection=bz.WENO(order=5))
    ref = dyn.reference_state
    sl = slice(grid.Hz, grid.Hz + grid.Nz)
    rho = lambda x, y, z: np.interp(z, grid.zᶜ, ref.density[sl]) * (1 + 0.01 * np.sin(2 * np.pi * x / 16e3)) + 0 * y
    model.set(ρ=rho, θ=lambda x, y, z: 300.0 + 2.0 * np.cos(2 * np.pi * y / 16e3) + 1e-3 * z + 0 * x, u=0.0, v=0.0, w=0.0,
              qᵗ=lambda x, y, z: 0.012 * np.exp(-z / 3e3) + 0 * x + 0 * y)
    g, T, ql = _model_inputs(model)
    qv = model.specific_moisture.interior_cpu()
    p, r = dyn.pressure.interior_cpu(), dyn.total_density.interior_cpu()
    pr = ref.pressure[sl][:, None, None] * np.ones_like(T)
    rr = ref.density[sl][:, None, None] * np.ones_like(T)
    z = np.asarray(grid.zᶜ)[:, None, None] * np.ones_like(T)
    c = dr.constants()
    ops = [bz.PotentialTemperature(model), bz.PotentialTemperature(model, "density"), bz.VirtualPotentialTemperature(model),
           bz.LiquidIcePotentialTemperature(model), bz.EquivalentPotentialTemperature(model),
           bz.StabilityEquivalentPotentialTemperature(model, "density"), bz.StaticEnergy(model), bz.StaticEnergy(model, "density"),
           bz.RelativeHumidity(model), bz.SaturationSpecificHumidity(model), bz.SaturationSpecificHumidity(model, "equilibrium"),
           bz.SaturationSpecificHumidity(model, "total_moisture")]
    fields = bz.compute_diagnostics(model, ops)
    assert np.abs(p / pr - 1).max() > 1e-4          # the model's own pressure is not the reference column
    for op, f in zip(ops, fields):
        name = ("DENSITY_" if getattr(op, "flavor", "") == "density" else "") + op.kind
        own = op.uses_model_pressure
        want = dr.evaluate(name, T, qv, ql, p if own else pr, r if own else rr, z, qv, c)
        err = _relerr(f.interior_cpu(), want)
        print(f"COMPRESSIBLE {name}: {err:.3e}")
        assert err <= 1e-12, (name, err)
    # without a reference state only the potential temperatures are defined
    bare = bz.CompressibleAtmosphereModel(grid, bz.CompressibleDynamics(bz.SplitExplicitTimeDiscretization(substeps=6), reference_state=None),
                                          advection=bz.WENO(order=5))
    with pytest.raises(NotImplementedError):
        bz.RelativeHumidity(bare).compute()


# ---- 4. Kessler fractions ----------------------------------------------------------------------------------------------------------
def test_kessler_liquid_is_cloud_plus_rain(bz):
    grid = bz.RectilinearGrid((16, 16, 8), x=(0, 16e3), y=(0, 16e3), z=(0, 4e3))
    tc = bz.ThermodynamicConstants(saturation_vapor_pressure=bz.TetensFormula())
    model = bz.AtmosphereModel(grid, advection=bz.WENO(order=5), microphysics=bz.DCMIP2016KesslerMicrophysics(), thermodynamic_constants=tc)
    model.set(θ=lambda x, y, z: 300.0 + 1e-3 * z + np.sin(2 * np.pi * x / 16e3) + 0 * y, qᵗ=0.008,
              qᶜˡ=lambda x, y, z: 1e-3 * (1 + np.cos(2 * np.pi * y / 16e3)) + 0 * x + 0 * z,
              qʳ=lambda x, y, z: 5e-4 * (1 + np.sin(2 * np.pi * x / 16e3)) + 0 * y + 0 * z)
    μ = model.microphysical_fields
    g, T, ql = _model_inputs(model, (μ["qᶜˡ"], μ["qʳ"]))
    assert μ["qᶜˡ"].interior_cpu().min() > 0 and μ["qʳ"].interior_cpu().max() > 0
    qv = μ["qᵛ"].interior_cpu()
    ref = model.dynamics.reference_state
    sl = slice(grid.Hz, grid.Hz + grid.Nz)
    p = ref.pressure[sl][:, None, None] * np.ones_like(T)
    r = ref.density[sl][:, None, None] * np.ones_like(T)
    z = np.asarray(grid.zᶜ)[:, None, None] * np.ones_like(T)
    c = dr.constants()
    ops = [bz.LiquidIcePotentialTemperature(model), bz.VirtualPotentialTemperature(model), bz.StaticEnergy(model)]
    for op, f in zip(ops, bz.compute_diagnostics(model, ops)):
        want = dr.evaluate(op.kind, T, qv, ql, p, r, z, qv, c)
        cloud_only = dr.evaluate(op.kind, T, qv, μ["qᶜˡ"].interior_cpu().astype(F64), p, r, z, qv, c)
        err = _relerr(f.interior_cpu(), want)
        print(f"KESSLER {op.kind}: {err:.3e}")
        assert err <= 1e-12 and np.max(np.abs(cloud_only - want) / np.abs(want)) > 1e-6      # the rain matters at this bound
    with pytest.raises(NotImplementedError):          # p^v+ of these constants is Tetens' formula: not built
        bz.RelativeHumidity(model).compute()


# ---- 5. stale diagnostics ----------------------------------------------------------------------------------------------------------
def test_stale_diagnostics_are_rebuilt_by_the_call(bz):
    def stepped():
        grid = bz.RectilinearGrid((32, 32, 16), x=(-8e3, 8e3), y=(-8e3, 8e3), z=(0, 8e3))
        m = bz.AtmosphereModel(grid, dynamics=bz.AnelasticDynamics(bz.ReferenceState(grid, potential_temperature=300.0)),
                               advection=bz.WENO(order=5))
        m.set(θ=lambda x, y, z: 300.0 + 1e-3 * z + 3.0 * np.exp(-(x ** 2 + y ** 2 + (z - 2e3) ** 2) / 2e6), u=8.0,
              qᵗ=lambda x, y, z: 0.01 * np.exp(-z / 2.5e3) * (1 + 0.2 * np.sin(2 * np.pi * x / 16e3)) + 0 * y)
        before = bz.RelativeHumidity(m).compute().interior_cpu()
        m.time_steps(4.0, 3, diagnose_last=False)
        return m, before
    a, before = stepped()
    assert bz.diagnostics_stale(a)
    ha = bz.RelativeHumidity(a).compute()
    assert not bz.diagnostics_stale(a)
    b, _ = stepped()
    assert bz.diagnostics_stale(b)
    bz.update_state_(b, compute_tendencies=False)
    hb = bz.RelativeHumidity(b).compute()
    va, vb = ha.interior_cpu(), hb.interior_cpu()
    assert np.array_equal(va, vb)
    assert np.abs(va - before).max() > 1e-6          # the steps moved the humidity: a stale answer would have shown


# ---- 6. horizontal averages --------------------------------------------------------------------------------------------------------
def _nan_halo_field(bz, model, zface, interior):
    import torch
    from breeze_jl_amd.grids import Center, Face
    f = bz.Field(model.grid, (Center, Center, Face if zface else Center), model.device)
    f.parent.fill_(float("nan"))
    f.interior.copy_(torch.from_numpy(np.ascontiguousarray(interior)).to(f.dtype))
    return f


@pytest.mark.parametrize("zface", [False, True], ids=["centre", "zface"])
@pytest.mark.parametrize("name", ["130x3x7", "20x6x5"])
def test_horizontal_average(bz, cases, name, zface):
    case = cases(name, F64, True)
    g, m = case.grid, case.model
    sh = (g.Nz + (1 if zface else 0), g.Ny, g.Nx)
    rng = np.random.default_rng(17)
    x = rng.standard_normal(sh) * 10.0 ** rng.uniform(-3, 3, sh)
    f = _nan_halo_field(bz, m, zface, x)
    got = bz.horizontal_average(m, f)
    assert got.shape == (sh[0],)
    L = np.longdouble
    want = x.astype(L).mean(axis=(1, 2))
    bound = np.finfo(F64).eps * g.Nx * g.Ny * np.abs(x).mean(axis=(1, 2))
    print(f"HAVG {name} zface={zface}: worst error / bound {np.max(np.abs(got - want) / bound):.3e}")
    assert np.all(np.abs(got - want) <= bound)
    assert np.array_equal(_bits(got), _bits(bz.horizontal_average(m, f)))          # deterministic
    ints = rng.integers(-50, 50, sh).astype(F64)
    got = bz.Average(_nan_halo_field(bz, m, zface, ints), dims=(1, 2), model=m).compute()
    assert np.array_equal(got, ints.sum(axis=(1, 2)) / (g.Nx * g.Ny))             # exact sums, one correctly rounded division


def test_average_of_an_operation(bz, cases):
    m = cases("130x3x7", F64, True).model
    m.set(θ=lambda x, y, z: 295.0 + 2e-3 * z + np.sin(2 * np.pi * x / 13e3) + 0 * y, qᵗ=0.006)
    prof = bz.Average(bz.RelativeHumidity(m)).compute()
    field = bz.RelativeHumidity(m).compute()
    assert np.array_equal(prof, bz.horizontal_average(m, field))
    v = field.interior_cpu()
    np.testing.assert_allclose(prof, v.mean(axis=(1, 2)), rtol=1e-13)
    with pytest.raises(NotImplementedError):
        bz.Average(bz.RelativeHumidity(m), dims=(1, 2, 3))


def test_horizontal_average_is_unsupported_on_slab_contexts(bz):
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
        prof = np.zeros(grid.Nz)
        rc = lib.bz_horizontal_average(ctx, C.c_void_p(field.data_ptr()), 0, prof.ctypes.data_as(C.POINTER(C.c_double)))
        assert rc == 2          # BZ_ERR_UNSUPPORTED
        assert b"slab" in lib.bz_last_error(ctx)
    finally:
        lib.bz_destroy(ctx)


# ---- 7. Float32 twin ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("liquid", [False, True], ids=["ql0", "ql"])
@pytest.mark.parametrize("name", sorted(GRIDS))
def test_float32_twin_within_four_times_the_formulas_own_error(cases, name, liquid):
    case = cases(name, F32, liquid)
    names = KINDS + DENSITY
    outs = case.run(names)
    inside = np.zeros(case.grid.parent_shape(), bool)
    inside[case.grid.interior_slices()] = True
    bad = {}
    for kind, P in zip(names, outs):
        assert P.dtype == F32 and np.all(P[~inside] == F32(SENTINEL)), kind
        if kind == "DEWPOINT_TEMPERATURE":
            continue
        want = case.reference(kind, F64)
        E32 = np.max(np.abs(case.reference(kind, F32).astype(F64) - want))
        err = np.max(np.abs(case.interior(P).astype(F64) - want))
        print(f"F32DIAG {name} ql={int(liquid)} {kind}: E32 = {E32:.3e} device = {err:.3e} ratio = {err / E32:.2f}")
        if not err <= 4 * E32:
            bad[kind] = (err, E32)
    assert not bad, bad
    c64 = dr.constants()
    T64 = case.Tc.astype(F64)
    E_ps = np.max(np.abs(dr.saturation_vapor_pressure(case.Tc, dr.constants(F32)).astype(F64) - dr.saturation_vapor_pressure(T64, c64)))
    _check_dewpoint(case, case.interior(outs[names.index("DEWPOINT_TEMPERATURE")]), residual_dtype=F32, slack=4 * E_ps)
