"""Bulk surface fluxes on the compressible split-explicit model (csrc/bz_cmp_surface_flux.hip through the C ABI and
CompressibleAtmosphereModel(boundary_conditions = ...)) against the CPU restatement tests/compressible_surface_flux_reference.py (pinned by
tests/test_compressible_surface_flux_reference.py).

Kernel and shapes.  k_cmp_surface_flux is one lane per surface column, 256 lanes along x, j on blockIdx.y; a ragged Nx is a predicate on the
lane, the x / y neighbours of u, v are reached by periodic wrap offsets.
    (16, 8, 8)     one partly filled wavefront
    (66, 9, 9)     a ragged wavefront behind a full one, odd Ny
    (65, 8, 3)     Nx % 64 == 1 (one lane in the second wavefront), three levels
    (258, 4, 4)    two lanes into a second 256-lane block
Whole steps run on (16, 12, 12) and (66, 9, 9) with 100 m x 100 m x 50 m cells, dt = 0.5 s, six acoustic substeps: coefficients of 4e-3 to
6e-3 and a surface 1 - 4 K warmer than the air then move the first level of rho u, rho v and rho q by more than 1e4 times the tolerance in
three steps."""
import ctypes as C

import numpy as np
import pytest

import compressible_closure_reference as ccr
import compressible_surface_flux_reference as sfr
import instantaneous_precipitation_reference as ipr
import scalar_diffusivity_reference as sdr

pytestmark = pytest.mark.gpu

COEF = {"drag": (6e-3, 1.0), "heat": (4e-3, 1.0), "vapor": (4e-3, 0.5)}      # (coefficient, gustiness)
FIELDS = ("rho_d", "rtheta", "rq", "ru", "rv", "rw", "T", "p")
FLUXED = {"ru": "ρu", "rv": "ρv", "rtheta": "ρθ", "rq": "ρq"}
KINDS = ("vapour", "saturation_adjustment", "kessler", "instantaneous_precipitation")
# dt of the stepped cases: with 100 m cells and six substeps the model itself is unstable at dt = 1 s (a dry column at rest grows fifty-fold
# per step from the seventh step on, restatement and device alike); at 0.5 s it is not (tests/test_compressible_closure.py steps the same cells so)
DT = 0.5


def _T0(shape, k):
    """(Ny, Nx) surface temperature of condition k (0 drag, 1 heat, 2 vapour): 2 - 4 K above the 300 K air, varying in x and y"""
    Nx, Ny, _ = shape
    x, y = (np.arange(Nx) + 0.5) / Nx, (np.arange(Ny) + 0.5) / Ny
    return (301.0, 303.5, 302.5)[k] + 1.0 * np.sin(2 * np.pi * x)[None, :] * np.cos(2 * np.pi * y)[:, None]


def _restated_fluxes(shape, array=True):
    T0 = [_T0(shape, k) if array else float(_T0(shape, k)[0, 0]) for k in range(3)]
    return sfr.SurfaceFluxes(*[COEF[n] + (T0[k],) for k, n in enumerate(("drag", "heat", "vapor"))])


def _device_conditions(bz, shape, array=True, heat_key="ρe"):
    F = _restated_fluxes(shape, array)
    drag = bz.BulkDrag(coefficient=F.drag[0], gustiness=F.drag[1], surface_temperature=F.drag[2])
    return {"ρu": bz.FieldBoundaryConditions(bottom=drag), "ρv": bz.FieldBoundaryConditions(bottom=drag),
            heat_key: bz.BulkSensibleHeatFlux(coefficient=F.heat[0], gustiness=F.heat[1], surface_temperature=F.heat[2]),      # ρe: moved to ρθ
            "ρqᵗ": bz.FluxBoundaryCondition(bz.BulkVaporFlux(coefficient=F.vapor[0], gustiness=F.vapor[1], surface_temperature=F.vapor[2]))}


class _CycloneModel(sfr.SurfaceFluxMixin, ipr.InstantaneousPrecipitationModel, ccr.ClosureCompressibleModel):
    """InstantaneousPrecipitation + FPlane + field-valued VerticalScalarDiffusivity + the bulk surface fluxes: the list of
    validation/DCMIP2016_TC/dcmip2016_tc.jl:277-311"""


def _ext(shape):
    Nx, Ny, Nz = shape
    return dict(x=(0.0, 100.0 * Nx), y=(0.0, 100.0 * Ny), z=(0.0, 50.0 * Nz))


def _K(shape, seed, top):
    Nx, Ny, Nz = shape
    return top * np.random.default_rng(seed).random((Nz, Ny, Nx))


def _pair(oracle, oc, bz, shape, kind="vapour", fluxes=True, array=True, float_type=np.float64, substep_floattype=None, heat_key="ρe"):
    """-> (restatement, device model) with the three conditions attached to both (fluxes = False: to neither)"""
    ext = _ext(shape)
    og = oracle.Grid(shape, **ext)
    F = _restated_fluxes(shape, array) if fluxes else None
    kw = dict(time_discretization=oc.SplitExplicit(substeps=6), reference_potential_temperature=300.0)
    grid = bz.RectilinearGrid(shape, float_type=float_type, **ext)
    mk = {}
    if kind == "instantaneous_precipitation":
        nu, kappa = _K(shape, 20, 10.0), _K(shape, 30, 15.0)
        om = _CycloneModel(og, coriolis_f=1e-4, diffusivity=sdr.Diffusivity(1, False, nu=nu, kappa=kappa), **kw)
        hk = {}
        for name, value in (("ν", nu), ("κ", kappa)):
            hk[name] = bz.Field(grid, (bz.Center, bz.Center, bz.Center), "cuda:0")
            hk[name].set_interior(value)
        mk = dict(microphysics=bz.InstantaneousPrecipitation(equilibrium=bz.WarmPhaseEquilibrium()), coriolis=bz.FPlane(f=1e-4),
                  closure=bz.VerticalScalarDiffusivity(**hk))
    else:
        micro = {"vapour": None, "saturation_adjustment": "SaturationAdjustment", "kessler": "Kessler"}[kind]
        om = sfr.SurfaceFluxCompressibleModel(og, microphysics=micro, **kw)
        if kind == "kessler":
            mk = dict(thermodynamic_constants=bz.ThermodynamicConstants(saturation_vapor_pressure=bz.TetensFormula()),
                      microphysics=bz.DCMIP2016KesslerMicrophysics())
        elif kind == "saturation_adjustment":
            mk = dict(microphysics=bz.SaturationAdjustment(equilibrium=bz.WarmPhaseEquilibrium()))
    om.surface_fluxes = F
    dyn = bz.CompressibleDynamics(bz.SplitExplicitTimeDiscretization(substeps=6), reference_potential_temperature=300.0)
    hm = bz.CompressibleAtmosphereModel(grid, dyn, advection=bz.WENO(order=5), substep_floattype=substep_floattype,
                                        boundary_conditions=_device_conditions(bz, shape, array, heat_key) if fluxes else None, **mk)
    return om, hm


def _ic(om, kind, dry=False):
    """set! keywords of both models: sheared u and v over the reference column, moisture that condenses under the two adjustment schemes where
    its wave crests"""
    g = om.grid
    Lx, Ly, Lz = g.Nx * g.dx, g.Ny * g.dy, g.zf[-1] - g.zf[0]
    # Smooth fields only: at dt = 1 s the cone-shaped 0.5 K bubble of the adjustment tests (ipr.bubble_state) put the FLUX-FREE device /
    # restatement pair of these grids 1e-8 - 2e-7 apart in rho u after three steps, the same grids without it 1e-14 - 1e-11 (measured on
    # the MI355X): a state on which the step tolerance measures the fluxes and not the last bit of a WENO weight
    wave = lambda x, y, z: np.sin(2 * np.pi * x / Lx + 0.3) * np.cos(2 * np.pi * y / Ly - 0.2) * np.sin(np.pi * z / Lz)      # noqa: E731
    ic = dict(rho=om.ref.density[g.Hz:g.Hz + g.Nz][:, None, None], theta=300.0,
              u=lambda x, y, z: 3.0 + 1.0 * np.sin(2 * np.pi * y / Ly + 0.5) + 0 * x + 0 * z, v=lambda x, y, z: -1.5 + 0.5 * np.cos(2 * np.pi * x / Lx) + 0 * y + 0 * z,
              w=0.0)
    if dry:
        return ic
    if kind == "vapour":
        ic["qv"] = lambda x, y, z: 0.010 * np.exp(-z / 2e3) * (1 + 0.2 * np.sin(2 * np.pi * x / Lx)) + 0 * y
    elif kind == "kessler":
        ic["qv"] = lambda x, y, z: 0.012 + 0.004 * wave(x, y, z)
        ic.update(qcl=lambda x, y, z: 0.0015 * (1 + wave(x, y, z)), qr=lambda x, y, z: 0.0005 * (1 + wave(x, y, z)))
    else:      # the two adjustment schemes: saturated where the wave crests (q^v+ is 0.022 at the surface, 0.017 at the top of the 450 - 600 m column)
        ic["qv"] = lambda x, y, z: 0.017 + 0.006 * wave(x, y, z)
    return ic


def _set_device(hm, ic):
    names = {"rho": "ρ", "theta": "θ", "u": "u", "v": "v", "w": "w", "qv": "qᵗ", "qcl": "qcl", "qr": "qr"}
    hm.set(**{names[k]: v for k, v in ic.items()})


def _step(bz, hm, dt, whole_step=True):
    bz.compressible.time_step_(hm, dt, whole_step=whole_step)


def _got(hm):
    from test_gpu_compressible import O2H
    return {n: O2H[n](hm).interior_cpu().copy() for n in FIELDS}


def _distance(got, om):
    """per field: max-abs error relative to the field's max-abs, the momentum components on the vector's scale (test_gpu_compressible.cmp_interior)"""
    g = om.grid
    mom = max(np.abs(g.interior(getattr(om, n), n == "rw")).max() for n in ("ru", "rv", "rw"))
    out = {}
    for n in FIELDS:
        want = g.interior(getattr(om, n), n == "rw")
        out[n] = np.abs(got[n] - want).max() / max(mom if n in ("ru", "rv", "rw") else np.abs(want).max(), 1e-300)
    return out


def _push(om, hm):
    import torch
    from test_gpu_compressible import push
    push(om, hm)
    if om.microphysics == "SaturationAdjustment":
        hm.microphysical_fields["qᵛ"].parent.copy_(torch.from_numpy(om.qv))
        hm.microphysical_fields["qˡ"].parent.copy_(torch.from_numpy(om.ql))


# ---- 1. one evaluation ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,kind", [((16, 8, 8), "vapour"), ((66, 9, 9), "vapour"), ((65, 8, 3), "vapour"), ((258, 4, 4), "vapour"),
                                        ((16, 8, 8), "saturation_adjustment")],
                         ids=["16x8x8", "66x9x9", "65x8x3", "258x4x4", "16x8x8-saturation_adjustment"])
def test_one_evaluation_matches_the_restatement(oracle, oc, bz, shape, kind):
    """compute_flux_bc_tendencies_ on zeroed tendencies, from the restatement's bits: every first-level tendency within 1e-12 of max |J / dz|
    (the project's tolerance for the anelastic flux evaluation), every other entry an exact zero"""
    from test_gpu_compressible import seeded_state
    om, hm = _pair(oracle, oc, bz, shape, kind)
    seeded_state(om, 7)
    g = om.grid
    if kind == "saturation_adjustment":      # the vapour flux reads the diagnosed q^v, not the total moisture: a first level that is cloudy in part
        x = (np.arange(g.Nx) + 0.5) / g.Nx
        g.interior(om.rq)[0] = g.interior(om.rho_d)[0] * (0.026 + 0.008 * np.sin(2 * np.pi * x))[None, :]
        om.update_state(compute_tendencies=True)
        ql0 = g.interior(om.ql)[0]
        assert 0.02 < (ql0 > 0).mean() < 0.98, (ql0 > 0).mean()
    _push(om, hm)
    for k in hm.G:
        hm.G[k].parent.zero_()
    for n in om.G:
        om.G[n][...] = 0.0
    sfr.add_flux_bc_tendencies(om, om.surface_fluxes)
    bz.compressible.compute_flux_bc_tendencies_(hm)
    hm.synchronize()
    for n, k in FLUXED.items():
        want = g.interior(om.G[n])
        got = hm.G[k].cpu()
        scale = np.abs(want[0]).max()
        tol = 1e-12 * scale
        err = np.abs(hm.G[k].interior_cpu()[0] - want[0]).max()
        print(f"SFEVAL {shape} {kind} {n}: max|J/dz|={scale:.3e} err/max={err / scale:.2e}")
        assert scale >= 1e3 * tol and scale > 0, n
        assert (want[0] > 0).any() and (want[0] < 0).any() or n == "rq", n      # sign-changing momentum and heat fluxes
        assert err <= tol, (n, err / scale)
        got[g.Hz, g.Hy:g.Hy + g.Ny, g.Hx:g.Hx + g.Nx] = 0.0
        assert not got.any(), f"{n}: something beyond the first interior level was written"
    assert not hm.G["ρw"].cpu().any() and not hm.G["ρᵈ"].cpu().any()
    if kind == "saturation_adjustment":      # ... and the total moisture in its place would miss the bound by orders
        wrong = sfr.SurfaceFluxes(vapor=om.surface_fluxes.vapor)
        om.microphysics = None
        Jq = sfr.first_level_fluxes(om, wrong)["rq"] / g.dzc[g.Hz]
        om.microphysics = "SaturationAdjustment"
        assert np.abs(Jq - g.interior(om.G["rq"])[0]).max() > 1e6 * 1e-12 * np.abs(g.interior(om.G["rq"])[0]).max()


def test_a_number_is_the_constant_array(oracle, oc, bz):
    """surface_temperature as a number: the bits of the constant (Ny, Nx) array"""
    from test_gpu_compressible import seeded_state
    out = []
    for array in (False, True):
        om, hm = _pair(oracle, oc, bz, (66, 9, 9), array=False)
        if array:
            S = om.surface_fluxes
            conds = hm._surface_fluxes
            for slot, T0 in (("drag", S.drag[2]), ("heat", S.heat[2]), ("vapor", S.vapor[2])):
                conds[slot].surface_temperature = np.full((9, 66), T0)
            from breeze_jl_amd.forcings import materialize_compressible_surface_fluxes
            Sf, keep = materialize_compressible_surface_fluxes(hm.grid, conds, hm.dynamics, hm.thermodynamic_constants, hm._T)
            hm._check(hm._lib.bz_set_compressible_surface_fluxes(hm._ctx, C.byref(Sf)), "bz_set_compressible_surface_fluxes")
        seeded_state(om, 8)
        _push(om, hm)
        for k in hm.G:
            hm.G[k].parent.zero_()
        bz.compressible.compute_flux_bc_tendencies_(hm)
        out.append({k: hm.G[k].cpu().copy() for k in hm.G})
    for k in out[0]:
        assert np.array_equal(out[0][k], out[1][k]), k
    assert np.abs(out[0]["ρθ"]).max() > 0


# ---- 2. slow tendencies of a stage --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(16, 12, 12), (66, 9, 9)], ids=["16x12x12", "66x9x9"])
def test_slow_tendencies_of_a_stage_with_fluxes(oracle, oc, bz, shape):
    """compute_slow_tendencies! + compute_flux_bc_tendencies! of a stage against the restatement, 1e-12 of max-abs
    (tests/test_gpu_compressible.py: test_slow_tendencies_match_oracle); the moisture tendency is the one update_state! left, plus its flux"""
    from test_gpu_compressible import PROG, rel, seeded_state
    om, hm = _pair(oracle, oc, bz, shape, heat_key="ρθ")
    seeded_state(om, 3)
    _push(om, hm)                                   # (the moisture tendency of the closing update_state! travels with the state)
    base = {n: a.copy() for n, a in om.G.items()}
    om.compute_slow_tendencies()
    for k in hm.G:
        if k != "ρq":
            hm.G[k].parent.zero_()
    bz.compressible.compute_slow_tendencies_(hm)
    bz.compressible.compute_flux_bc_tendencies_(hm)
    g = om.grid
    for n, k in PROG.items():
        a, b = hm.G[k].interior_cpu(), g.interior(om.G[n], n == "rw")
        if n == "rw":
            a, b = a[1:-1], b[1:-1]
        print(f"SFSLOW {shape} {n}: {rel(a, b):.2e}")
        assert rel(a, b) <= 1e-12, (n, rel(a, b))
    assert np.abs(g.interior(om.G["rq"])[0] - g.interior(base["rq"])[0]).max() > 0      # the restatement added the vapour flux


# ---- 3. three whole steps ---------------------------------------------------------------------------------------------------------------
STEP_TOL = {"vapour": 5e-9, "saturation_adjustment": 1e-8, "kessler": 1e-8, "instantaneous_precipitation": 1e-8}
# (the tolerances the same models meet without fluxes: tests/test_gpu_compressible.py:306,714,790, tests/test_instantaneous_precipitation.py:246)


@pytest.mark.parametrize("shape", [(16, 12, 12), (66, 9, 9)], ids=["16x12x12", "66x9x9"])
@pytest.mark.parametrize("kind", KINDS)
def test_three_steps_match_the_restatement(oracle, oc, bz, kind, shape, monkeypatch):
    """time_step!, dt = 0.5 s: the whole-step seam (fused stage epilogue), the same seam with the unfused epilogue (BZ_NO_AC_END_FUSE=1) and the
    per-operator sequence (whole_step = False, bz_acoustic_rk3_substep) against the restatement; and the fluxes acted: the device run
    without them ends elsewhere at the first level — rho u and rho q by more than 1e4 tolerances, rho theta (0.05 C dtheta / dz of its
    350 kg K m^-3 in three seconds: 6e-6) by more than 1e2"""
    tol, dt = STEP_TOL[kind], DT
    om, a = _pair(oracle, oc, bz, shape, kind)
    _, b = _pair(oracle, oc, bz, shape, kind)
    monkeypatch.setenv("BZ_NO_AC_END_FUSE", "1")
    _, c = _pair(oracle, oc, bz, shape, kind)
    monkeypatch.delenv("BZ_NO_AC_END_FUSE")
    om0, free = _pair(oracle, oc, bz, shape, kind, fluxes=False)
    ic = _ic(om, kind)
    om.set(**ic)
    om0.set(**ic)
    for m in (a, b, c, free):
        _set_device(m, ic)
    a.profile_enable(True)
    for _ in range(3):
        om.time_step(dt)
        om0.time_step(dt)
        _step(bz, a, dt)
        _step(bz, b, dt, whole_step=False)
        _step(bz, c, dt)
        _step(bz, free, dt)
    for m in (a, b, c, free):
        m.synchronize()
    assert a.profile()["compressible_surface_fluxes"][1] == 9      # one launch per stage
    if kind in ("saturation_adjustment", "instantaneous_precipitation"):
        cloudy = (om.grid.interior(om.ql) > 0).mean() if kind == "saturation_adjustment" else om.condensed.mean()
        assert 0 < cloudy < 0.98, cloudy
    worst = {}
    for label, m in (("fused", a), ("operators", b), ("unfused epilogue", c)):
        worst[label] = _distance(_got(m), om)
        print(f"SFSTEPS {kind} {shape} {label}:", " ".join(f"{n}={e:.1e}" for n, e in worst[label].items()))
    # a field that needs more than the tolerance of the flux-free tests is held to twice the distance of the flux-free pair of this very
    # case (the device without fluxes against the restatement without fluxes): the fluxes may not add to what the model leaves anyway
    flux_free = _distance(_got(free), om0)
    print(f"SFSTEPS {kind} {shape} flux-free pair:", " ".join(f"{n}={e:.1e}" for n, e in flux_free.items()))
    bound = {n: max(tol, 2 * flux_free[n]) for n in FIELDS}
    for label, w in worst.items():
        bad = {n: (e, bound[n]) for n, e in w.items() if not e <= bound[n]}
        assert not bad, (label, bad)
    ga, gf = _got(a), _got(free)
    mom = max(np.abs(ga[n]).max() for n in ("ru", "rv", "rw"))
    moved = {n: np.abs(ga[n][0] - gf[n][0]).max() / (mom if n in ("ru", "rv") else np.abs(ga[n]).max()) for n in ("ru", "rv", "rtheta", "rq")}
    print(f"SFMOVED {kind} {shape}:", " ".join(f"{n}={e:.1e}" for n, e in moved.items()))
    assert moved["ru"] >= 1e4 * tol and moved["rv"] >= 1e4 * tol and moved["rq"] >= 1e4 * tol and moved["rtheta"] >= 1e2 * tol, moved


# ---- 4. evaporation into a dry model ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("whole_step", [True, False], ids=["whole_step", "operators"])
def test_evaporation_into_a_dry_model(oracle, oc, bz, whole_step):
    """q^t = 0 everywhere and a BulkVaporFlux: after one step the first level holds vapour, as much as the restatement's — the dry shortcut
    of the step (the moisture scan) must be off while the flux is attached"""
    shape = (66, 9, 9)
    om, hm = _pair(oracle, oc, bz, shape)
    ic = _ic(om, "vapour", dry=True)
    om.set(**ic)
    _set_device(hm, ic)
    assert not hm.moisture_density.parent.any()
    om.time_step(DT)
    _step(bz, hm, DT, whole_step=whole_step)
    hm.synchronize()
    g = om.grid
    want, got = g.interior(om.rq), hm.moisture_density.interior_cpu()
    assert (want[0] > 0).all() and (got[0] > 0).all()
    err = np.abs(got - want).max() / np.abs(want).max()
    print(f"SFDRY whole_step={whole_step}: max rq={want.max():.3e} err={err:.1e}")
    assert err <= 5e-9
    assert all(e <= 5e-9 for e in _distance(_got(hm), om).values())


# ---- 5. detach ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dry", [False, True], ids=["vapour", "dry"])
def test_detached_fluxes_leave_the_bits_of_a_model_built_without(oracle, oc, bz, dry):
    """bz_set_compressible_surface_fluxes(NULL): three steps carry the bits of a model built without boundary_conditions that starts from
    the same state (halos included).  vapour: detached after one step with the fluxes, whose state goes into both models; dry: detached
    before the first step of a model with q = 0 everywhere, where the moisture scan and its shortcut are back"""
    shape = (66, 9, 9)
    om, a = _pair(oracle, oc, bz, shape)
    _, b = _pair(oracle, oc, bz, shape, fluxes=False)
    ic = _ic(om, "vapour", dry=dry)
    for m in (a, b):
        _set_device(m, ic)
    if not dry:
        _step(bz, a, DT)                            # one step with the fluxes, then the same state into both
        for k, f in a.prognostic_fields().items():
            b.prognostic_fields()[k].parent.copy_(f.parent)
        sub_a, sub_b = a.timestepper.substepper, b.timestepper.substepper
        for n in ("time_averaged_u", "time_averaged_v", "time_averaged_w"):
            getattr(sub_b, n).parent.copy_(getattr(sub_a, n).parent)
    bz.compressible.detach_surface_fluxes_(a)
    for m in (a, b):
        if not dry:
            bz.compressible.update_state_(m, compute_tendencies=True)
            m.clock.iteration = 1
        for _ in range(3):
            _step(bz, m, DT)
        m.synchronize()
    for k, f in a.prognostic_fields().items():
        assert np.isfinite(f.interior_cpu()).all() and np.array_equal(f.cpu(), b.prognostic_fields()[k].cpu()), k
    Ta, Tb = a.temperature.interior_cpu(), b.temperature.interior_cpu()
    assert np.isfinite(Ta).all() and np.array_equal(Ta, Tb)
    assert (not a.moisture_density.parent.any()) if dry else np.abs(a.moisture_density.interior_cpu()).max() > 0


# ---- 6. Float32 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["float32_grid", "float32_substep_storage"])
def test_float32_by_increments(oracle, oc, bz, case):
    """eltype(grid) = Float32 (the _f32 twin) and substep_floattype = Float32 in a Float64 model, three steps with the fluxes against the
    Float64 restatement, judged by what the steps did to each field (helpers.assert_increments, as tests/test_surface_layer.py)"""
    import helpers
    from test_compressible_closure import _initial
    shape, dt = (40, 6, 12), 0.5
    f32 = case == "float32_grid"
    om, hm = _pair(oracle, oc, bz, shape, float_type=np.float32 if f32 else np.float64, substep_floattype=None if f32 else np.float32)
    ic = _initial(om, 5, rough=0.2)
    om.set(**ic)
    _set_device(hm, ic)
    g = om.grid
    table = "compressible" if f32 else "substep_storage"
    names = tuple(helpers.F32_INCREMENT_TOL[table])
    start = {n: g.interior(getattr(om, n), n == "rw").copy() for n in names}
    for _ in range(3):
        om.time_step(dt)
        hm.time_step(dt)
    hm.synchronize()
    from test_gpu_compressible import O2H
    got = {n: O2H[n](hm).interior_cpu() for n in names}
    want = {n: g.interior(getattr(om, n), n == "rw") for n in names}
    helpers.assert_increments(f"compressible surface fluxes {case}", got, want, start, table)


# ---- 7. the C entry points refuse what they do not run ----------------------------------------------------------------------------------------
def test_entry_points_refuse_anelastic_and_kinematic_contexts(bz):
    from breeze_jl_amd import _lib, forcings
    grid = bz.RectilinearGrid((16, 16, 8), x=(0, 1600.0), y=(0, 1600.0), z=(0, 800.0))
    ref = bz.ReferenceState(grid, potential_temperature=300.0)
    conds = forcings.compressible_surface_flux_conditions(_device_conditions(bz, (16, 16, 8)), grid, True, False)
    dyn = bz.CompressibleDynamics(bz.SplitExplicitTimeDiscretization(substeps=6), reference_potential_temperature=300.0)
    S, keep = forcings.materialize_compressible_surface_fluxes(grid, conds, dyn, bz.ThermodynamicConstants())
    anelastic = bz.AtmosphereModel(grid, dynamics=bz.AnelasticDynamics(ref), advection=bz.WENO(order=5))
    kinematic = bz.AtmosphereModel(grid, dynamics=bz.PrescribedDynamics(ref), advection=bz.WENO(order=5))
    s, G = _lib.bz_compressible_state(), _lib.bz_compressible_prognostic()
    for m, word in ((anelastic, "anelastic"), (kinematic, "PrescribedDynamics")):
        for fn, call in (("bz_set_compressible_surface_fluxes", lambda: m._lib.bz_set_compressible_surface_fluxes(m._ctx, C.byref(S))),
                         ("bz_compressible_compute_flux_bc_tendencies",
                          lambda: m._lib.bz_compressible_compute_flux_bc_tendencies(m._ctx, C.byref(s), C.byref(G)))):
            rc = call()
            msg = m._lib.bz_last_error(m._ctx).decode()
            assert rc == 2 and fn in msg and word in msg, (rc, msg)
    # a compressible context takes the set and lets it go; bz_set_surface_layer keeps its answer there
    cm = bz.CompressibleAtmosphereModel(grid, dyn, advection=bz.WENO(order=5))
    assert cm._lib.bz_set_compressible_surface_fluxes(cm._ctx, C.byref(S)) == 0
    assert cm._lib.bz_set_compressible_surface_fluxes(cm._ctx, None) == 0
    from test_surface_layer import _expect_unsupported, _layer
    _expect_unsupported(cm._lib, cm._ctx, _layer(bz, grid, ref), "Compressible")
    S.heat.surface_temperature_field = None
    S.heat.surface_temperature = -1.0
    assert cm._lib.bz_set_compressible_surface_fluxes(cm._ctx, C.byref(S)) == 1      # BZ_ERR_INVALID
    assert "surface temperature" in cm._lib.bz_last_error(cm._ctx).decode()
