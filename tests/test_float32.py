"""eltype(grid) = Float32: lib/libbreeze_hip_f32.so, the Float32 twin of the library generated from the same sources
(tools/gen_f32_sources.py).  Every GPU benchmark and example of the reference runs in Float32
(/root/reference/benchmarking/src/convective_boundary_layer.jl:59,70; examples/bomex.jl:40); SURVEY.md §8d asks for the Float32 run
to be reported separately and Appendix C states its tolerances: 1e-5 per kernel, 1e-4 after time steps, against the Float64 oracle."""
import ctypes as C
import glob
import os
import re

import numpy as np
import pytest

import f32_cases as fc
from helpers import PROG, assert_increments, bubble_theta, increment_error, randomize, relerr

EXT = ((-10e3, 10e3), (-10e3, 10e3), (0.0, 10e3))


def test_float32_library_exports_the_whole_abi(bz):
    """CPU: the Float32 twin loads and exports every symbol of the header; its struct mirrors replace every double by a float."""
    from breeze_jl_amd import _lib
    bz.build()
    lib = _lib.load_f32()
    for name in _lib.SYMBOLS:
        assert hasattr(lib, name), name
    T = _lib.types(4)
    assert C.sizeof(T.bz_constants) == 5 * 4 and C.sizeof(_lib.bz_constants) == 5 * 8
    assert T.bz_state is _lib.bz_state                      # pointer-only structs are shared
    assert dict(T.bz_grid._fields_)["dx"] is C.c_float and dict(T.bz_grid._fields_)["zf"] is C.POINTER(C.c_float)
    generated = os.path.join(os.path.dirname(_lib.CSRC), "csrc", "build", "f32", "bz_weno.h")
    text = open(generated).read()
    assert "1e-8f" in text and "float bz_weno5_fast(float a" in text
    # no double-precision type is left in the code of the generated twin (comments and string literals may speak of it)
    paths = sorted(glob.glob(os.path.join(os.path.dirname(generated), "*.hip")) + glob.glob(os.path.join(os.path.dirname(generated), "*.h")))
    assert len(paths) > 20 and any(p.endswith("bz_tendency5_kernels.h") for p in paths)
    left = {}
    for path in paths:
        with open(path, encoding="utf-8") as f:
            code = _code_only(f.read())
        found = set(re.findall(r"\b(?:double|double2|make_double2|hipfftDoubleComplex|HIPFFT_[DZ]2[DZ]|hipfftExec[DZ]2[DZ])\b", code))
        found -= F32_DOUBLE_EXCEPTIONS.get(os.path.basename(path), set())
        if found:
            left[os.path.basename(path)] = sorted(found)
    assert not left, left


# double-precision tokens the generated Float32 sources are meant to keep, by file (none)
F32_DOUBLE_EXCEPTIONS = {}


def _code_only(text):
    """The code of a source file without its comments and with every string literal emptied — the same scan as
    tools/gen_f32_sources.py: convert, which leaves comments and strings alone."""
    out, i, n = [], 0, len(text)
    while i < n:
        if text.startswith("//", i):
            j = text.find("\n", i)
            i = n if j < 0 else j
        elif text.startswith("/*", i):
            i = text.find("*/", i) + 2
        elif text[i] == '"':
            j = i + 1
            while text[j] != '"' or text[j - 1] == "\\":
                j += 1
            out.append('""')
            i = j + 1
        else:
            j = i
            while j < n and text[j] != '"' and not text.startswith("//", j) and not text.startswith("/*", j):
                j += 1
            out.append(text[i:j])
            i = j
    return "".join(out)


def _pair32(oracle, bz, size, z=EXT[2]):
    og = oracle.Grid(size, x=EXT[0], y=EXT[1], z=z)
    om = oracle.OracleModel(og, potential_temperature=300.0)
    grid = bz.RectilinearGrid(size, x=EXT[0], y=EXT[1], z=z, float_type=np.float32)
    hm = bz.AtmosphereModel(grid, dynamics=bz.AnelasticDynamics(bz.ReferenceState(grid, potential_temperature=300.0)), advection=bz.WENO())
    return om, hm


@pytest.mark.gpu
def test_float32_tendencies_match_the_float64_oracle(oracle, bz):
    _float32_tendencies(oracle, bz, (32, 20, 16), False)


@pytest.mark.gpu
@pytest.mark.parametrize("size,stretched", [((72, 12, 12), False), ((130, 16, 12), False), ((64, 24, 16), False),
                                            ((32, 24, 16), True)])      # the ragged shapes of tests/test_float32_increments.py and a stretched z
def test_float32_tendencies_at_ragged_shapes_match_the_float64_oracle(oracle, bz, size, stretched):
    _float32_tendencies(oracle, bz, size, stretched)


def _float32_tendencies(oracle, bz, size, stretched):
    import torch
    om, hm = _pair32(oracle, bz, size, z=fc.stretched_faces(size[2]) if stretched else EXT[2])
    assert hm.momentum["ρu"].parent.dtype == torch.float32
    randomize(om, seed=11)
    om.compute_tendencies()
    from helpers import ORACLE_TO_HIP
    for n in ("ru", "rv", "rw", "rtheta", "rq", "u", "v", "w", "theta", "q", "T"):
        ORACLE_TO_HIP[n](hm).parent.copy_(torch.from_numpy(getattr(om, n)).to(torch.float32))
    bz.compute_tendencies_(hm)
    hm.synchronize()
    for n, k in PROG.items():
        got, want = hm.G[k].interior_cpu().astype(np.float64), om.grid.interior(om.G[n], zface=(n == "rw"))
        # rho theta: the tendency is a small difference of fluxes of a 300 K field: 1e-5 of the FLUX scale
        scale = np.max(np.abs(want)) if n != "rtheta" else 300.0 * np.max(np.abs(om.grid.interior(om.G["rq"]))) / 5e-3
        # rho w: the buoyancy is g rho_r (T_r / T - 1) with T ~ 300 K rounded to 24 bits: 5e-5 of the tendency scale
        assert np.max(np.abs(got - want)) / scale < (5e-5 if n == "rw" else 2e-5), (n, np.max(np.abs(got - want)) / scale)


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(32, 20, 16), (64, 24, 16), (64, 16, 32)])      # the second shape takes the hand-written x transforms (Ny % 8 == 0)
@pytest.mark.parametrize("lean", [True, False])
def test_float32_time_steps_match_the_float64_oracle(oracle, oc, bz, lean, size, monkeypatch):
    _float32_time_steps(oracle, oc, bz, lean, size, False, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(32, 20, 16), (64, 24, 16), (64, 16, 32)])
@pytest.mark.parametrize("lean", [True, False])
def test_float32_moist_time_steps_match_the_float64_oracle(oracle, oc, bz, lean, size, monkeypatch):
    """The same steps with the vapour profile of the moist lean-seam cases: rho q is really compared (the dry model's is zero)."""
    _float32_time_steps(oracle, oc, bz, lean, size, True, monkeypatch)


def _float32_time_steps(oracle, oc, bz, lean, size, moist, monkeypatch):
    if not lean:
        monkeypatch.setenv("BZ_NO_LEAN", "1")
    if size == (64, 16, 32):      # round 6: the kx-major spectrum and the chunked middle of the solve (five chunks of 32 KB) in Float32
        monkeypatch.setenv("BZ_POISSON_KX_CHUNK_KB", "32")
    case = fc.STEP_CASES["time_steps_%dx%dx%d_%s" % (size + ("moist" if moist else "dry",))]
    om, hm = case.build(oracle, oc, bz)
    start = fc.oracle_fields(om, case.fields)
    for _ in range(case.steps):
        om.time_step(case.dt)
        hm.time_step(case.dt)
    hm.synchronize()
    assert_increments(case.name + (" lean" if lean else " nolean"), fc.device_fields(hm, case.fields), fc.oracle_fields(om, case.fields),
                      start, case.kind)
    for n, k in PROG.items():
        got = hm.prognostic_fields()[k].interior_cpu().astype(np.float64)
        want = om.grid.interior(getattr(om, n), zface=(n == "rw"))
        scale = max(np.max(np.abs(want)), 1e-3)
        assert np.max(np.abs(got - want)) / scale < 1e-4, (n, np.max(np.abs(got - want)) / scale)
    assert relerr(hm.temperature.interior_cpu().astype(np.float64), om.grid.interior(om.T)) < 1e-5
    # the projected momentum is divergence-free to Float32 round-off
    assert hm.max_abs_divergence() < 5e-4


@pytest.mark.gpu
def test_float32_bomex_physics_steps_match_the_float64_oracle(oracle, oc, bz):
    """The physics list of BASELINE configs[2] in the precision its example runs in (examples/bomex.jl:40, Float32): WENO5 + warm-phase
    saturation adjustment + SmagorinskyLilly + Coriolis / geostrophic / subsidence / profile forcings + bottom fluxes on a Float32
    grid, against the Float64 oracle.  Tolerances: 1e-4 of the field scale after three steps; the liquid water of
    cells sitting on the saturation threshold may switch branch under Float32 rounding, so q^l is compared in the mean."""
    case = fc.STEP_CASES["bomex"]
    om, hm = case.build(oracle, oc, bz)
    start = fc.oracle_fields(om, case.fields)
    g = om.grid
    # eddy viscosity of the initial state (after the steps the device's field is the one of the last stage's start: the whole-step
    # seam computes it where the tendencies need it).  The stability factor sqrt(1 - min(1, C_b N^2 / Sigma^2)) switches on a
    # threshold, so single cells may flip under Float32 rounding: compared in the mean
    om.update_state()
    bz.update_state_(hm, compute_tendencies=True)
    hm.synchronize()
    nu = hm.closure_fields["νₑ"].interior_cpu().astype(np.float64)
    assert np.abs(nu - om.nu_e).mean() < 1e-3 * om.nu_e.mean() and om.nu_e.max() > 0.01
    for _ in range(case.steps):
        om.time_step(case.dt)
        hm.time_step(case.dt)
    hm.synchronize()
    assert_increments(case.name, fc.device_fields(hm, case.fields), fc.oracle_fields(om, case.fields), start, case.kind)
    mom = max(np.abs(g.interior(getattr(om, n), zface=(n == "rw"))).max() for n in ("ru", "rv", "rw"))
    for n, k in PROG.items():
        want = g.interior(getattr(om, n), zface=(n == "rw"))
        got = hm.prognostic_fields()[k].interior_cpu().astype(np.float64)
        scale = mom if n in ("ru", "rv", "rw") else np.abs(want).max()
        assert np.abs(got - want).max() / scale < 1e-4, (n, np.abs(got - want).max() / scale)
    assert relerr(hm.temperature.interior_cpu().astype(np.float64), g.interior(om.T)) < 1e-5
    ql = hm.microphysical_fields["qˡ"].interior_cpu().astype(np.float64)
    assert abs(ql.mean() - g.interior(om.ql).mean()) < 1e-3 * max(g.interior(om.ql).mean(), 1e-8) + 1e-9


@pytest.mark.gpu
@pytest.mark.parametrize("kessler", [False, True])
def test_float32_compressible_steps_match_the_float64_oracle(oracle, oc, bz, kessler):
    """The precision of examples/splitting_supercell.jl:86 (Oceananigans.defaults.FloatType = Float32) on the split-explicit compressible
    model, dry and with the DCMIP2016 Kessler physics: two steps against the Float64 oracle at Appendix C's 1e-4 (density-like
    fields, whose perturbations are what Float32 resolves worst, relative to their own scale; momentum relative to the momentum scale)."""
    import torch
    case = fc.STEP_CASES["compressible_kessler" if kessler else "compressible_dry"]
    om, hm = case.build(oracle, oc, bz)
    og = om.grid
    assert hm.momentum["ρu"].parent.dtype == torch.float32
    start = fc.oracle_fields(om, case.fields)
    for _ in range(case.steps):
        om.time_step(case.dt)
        hm.time_step(case.dt)
    hm.synchronize()
    assert_increments(case.name, fc.device_fields(hm, case.fields, compressible=True), fc.oracle_fields(om, case.fields), start, case.kind)
    I = og.interior
    mom = max(np.abs(I(om.ru)).max(), np.abs(I(om.rw, True)).max())
    got = {"rho_d": hm.dynamics.dry_density, "rtheta": hm.potential_temperature_density, "rq": hm.moisture_density, "T": hm.temperature,
           "p": hm.dynamics.pressure, "ru": hm.momentum["ρu"], "rw": hm.momentum["ρw"]}
    worst = {}
    for n, f in got.items():
        want = I(getattr(om, n), n == "rw")
        scale = mom if n in ("ru", "rw") else np.abs(want).max()
        worst[n] = np.abs(f.interior_cpu().astype(np.float64) - want).max() / scale
    print("float32 compressible vs float64 oracle:", {k: f"{v:.1e}" for k, v in worst.items()})
    assert np.abs(I(om.rw, True)).max() > 1e-3
    assert max(worst.values()) < 1e-4, worst


def _steps_errors(om, hm, names):
    g = om.grid
    mom = max(np.abs(g.interior(getattr(om, n), n == "rw")).max() for n in ("ru", "rv", "rw"))
    out = {}
    for n, f in names:
        want = g.interior(getattr(om, n), n == "rw")
        scale = mom if n in ("ru", "rv", "rw") else max(np.abs(want).max(), 1e-6)
        out[n] = float(np.abs(f.interior_cpu().astype(np.float64) - want).max() / scale)
    return out


@pytest.mark.gpu
def test_float32_anelastic_kessler_tracers_and_static_energy(oracle, oc, bz):
    """The remaining model options on Float32 grids — DCMIP2016 Kessler species, user tracers, formulation = :StaticEnergy — two / three
    steps each against the Float64 oracle at Appendix C's 1e-4 of each field's scale."""
    # Kessler
    case = fc.STEP_CASES["kessler"]
    om, hm = case.build(oracle, oc, bz)
    start = fc.oracle_fields(om, case.fields)
    for _ in range(case.steps):
        om.time_step(case.dt)
        hm.time_step(case.dt)
    hm.synchronize()
    assert_increments(case.name, fc.device_fields(hm, case.fields), fc.oracle_fields(om, case.fields), start, case.kind)
    μ = hm.microphysical_fields
    e = _steps_errors(om, hm, (("ru", hm.momentum["ρu"]), ("rw", hm.momentum["ρw"]), ("rtheta", hm.potential_temperature_density),
                               ("rq", hm.moisture_density), ("rqcl", μ["ρqᶜˡ"]), ("rqr", μ["ρqʳ"]), ("T", hm.temperature)))
    print("float32 anelastic Kessler:", {k: f"{v:.1e}" for k, v in e.items()})
    assert max(e.values()) < 2e-4, e
    # tracers + StaticEnergy on the dry bubble
    for formulation in ("LiquidIcePotentialTemperature", "StaticEnergy"):
        tr = formulation == "LiquidIcePotentialTemperature"
        case = fc.STEP_CASES["tracer" if tr else "static_energy"]
        om, hm = case.build(oracle, oc, bz)
        start = fc.oracle_fields(om, case.fields)
        for _ in range(case.steps):
            om.time_step(case.dt)
            hm.time_step(case.dt)
        hm.synchronize()
        assert_increments(case.name, fc.device_fields(hm, case.fields), fc.oracle_fields(om, case.fields), start, case.kind)
        names = [(n, hm.prognostic_fields()[k]) for n, k in PROG.items() if n != "rq"]
        if tr:
            names.append(("rc0", hm.tracers["a"]))
        e = _steps_errors(om, hm, names)
        print("float32", formulation, {k: f"{v:.1e}" for k, v in e.items()})
        assert max(e.values()) < 1e-4, (formulation, e)


@pytest.mark.gpu
@pytest.mark.parametrize("order", [7, 9])
def test_float32_high_order_weno_matches_the_float64_oracle(oracle, oc, bz, order):
    """WENO(order = 7 / 9) on Float32 grids — the scheme AND the precision of examples/bomex.jl and splitting_supercell.jl.  The Float32
    build evaluates the smoothness indicators from first differences (tables BD / CD, tools/gen_weno_tables.py); with the expanded
    integer tables a 300 K field would lose every digit.  Tendencies 2e-5 of the flux scale, three steps 1e-4."""
    import torch
    from helpers import ORACLE_TO_HIP
    size = (24, 16, 14)
    og = oracle.Grid(size, x=EXT[0], y=EXT[1], z=EXT[2], halo=(5, 5, 5))
    om = oracle.OracleModel(og, potential_temperature=300.0, advection=f"WENO{order}")
    grid = bz.RectilinearGrid(size, x=EXT[0], y=EXT[1], z=EXT[2], halo=(5, 5, 5), float_type=np.float32)
    hm = bz.AtmosphereModel(grid, dynamics=bz.AnelasticDynamics(bz.ReferenceState(grid, potential_temperature=300.0)), advection=bz.WENO(order=order))
    randomize(om, seed=11)
    om.compute_tendencies()
    for n in ("ru", "rv", "rw", "rtheta", "rq", "u", "v", "w", "theta", "q", "T"):
        ORACLE_TO_HIP[n](hm).parent.copy_(torch.from_numpy(getattr(om, n)).to(torch.float32))
    bz.compute_tendencies_(hm)
    hm.synchronize()
    worst = {}
    for n, k in PROG.items():
        got, want = hm.G[k].interior_cpu().astype(np.float64), om.grid.interior(om.G[n], zface=(n == "rw"))
        scale = np.max(np.abs(want)) if n != "rtheta" else 300.0 * np.max(np.abs(om.grid.interior(om.G["rq"]))) / 5e-3
        worst[n] = np.max(np.abs(got - want)) / scale
    print(f"float32 WENO{order} tendencies:", {k: f"{v:.1e}" for k, v in worst.items()})
    assert all(v < (5e-5 if n == "rw" else 2e-5) for n, v in worst.items()), worst
    # three steps of the bubble
    case = fc.STEP_CASES[f"weno{order}"]
    om, hm = case.build(oracle, oc, bz)
    start = fc.oracle_fields(om, case.fields)
    for _ in range(case.steps):
        om.time_step(case.dt)
        hm.time_step(case.dt)
    hm.synchronize()
    assert_increments(case.name, fc.device_fields(hm, case.fields), fc.oracle_fields(om, case.fields), start, case.kind)
    e = _steps_errors(om, hm, [(n, hm.prognostic_fields()[k]) for n, k in PROG.items() if n != "rq"])
    print(f"float32 WENO{order} steps:", {k: f"{v:.1e}" for k, v in e.items()})
    assert max(e.values()) < 1e-4, e


@pytest.mark.gpu
def test_float32_order_nine_compressible_kessler_matches_the_float64_oracle(oracle, oc, bz):
    """examples/splitting_supercell.jl's scheme list in its own precision: CompressibleDynamics (split-explicit) + DCMIP2016 Kessler +
    WENO(order = 9) + Float32, two steps against the Float64 oracle."""
    case = fc.STEP_CASES["compressible_weno9_kessler"]
    om, hm = case.build(oracle, oc, bz)
    og = om.grid
    start = fc.oracle_fields(om, case.fields)
    for _ in range(case.steps):
        om.time_step(case.dt)
        hm.time_step(case.dt)
    hm.synchronize()
    assert_increments(case.name, fc.device_fields(hm, case.fields, compressible=True), fc.oracle_fields(om, case.fields), start, case.kind)
    I = og.interior
    mom = max(np.abs(I(om.ru)).max(), np.abs(I(om.rw, True)).max())
    worst = {}
    for n, f in (("rho_d", hm.dynamics.dry_density), ("rtheta", hm.potential_temperature_density), ("rq", hm.moisture_density),
                 ("T", hm.temperature), ("ru", hm.momentum["ρu"]), ("rw", hm.momentum["ρw"])):
        want = I(getattr(om, n), n == "rw")
        worst[n] = np.abs(f.interior_cpu().astype(np.float64) - want).max() / (mom if n in ("ru", "rw") else np.abs(want).max())
    print("float32 WENO9 compressible Kessler:", {k: f"{v:.1e}" for k, v in worst.items()})
    assert max(worst.values()) < 1e-4, worst


@pytest.mark.gpu
def test_float32_library_slabs_match_the_float64_oracle(oracle, oc, bz):
    """Float32 on y-slabs: the Float32 twin's own communicator (messages of 4-byte reals), two ranks sharing the GPU through the in-process
    transport, the dry bubble through the lean distributed step against the Float64 oracle at 1e-4."""
    import threading
    import uuid
    import torch
    from breeze_jl_amd import distributed as bz_dist
    size = (32, 24, 16)
    case = fc.STEP_CASES["slabs"]
    om, _ = case.build(oracle, oc)
    og = om.grid
    th = bubble_theta(300.0, om.constants.g)
    start = fc.oracle_fields(om, case.fields)
    for _ in range(case.steps):
        om.time_step(case.dt)
    G = bz.RectilinearGrid(size, x=EXT[0], y=EXT[1], z=EXT[2], float_type=np.float32)
    x, y, z = og.nodes("ccc")
    full = np.broadcast_to(th(x, y, z), (size[2], size[1], size[0])).copy()
    world, group = 2, "local:" + uuid.uuid4().hex
    models, errors = [None] * world, []

    def run(rank):
        try:
            torch.cuda.set_device(0)
            with torch.cuda.stream(torch.cuda.Stream()):
                m = bz_dist.LibrarySlabAtmosphereModel(G, rank, world, transport=group, device="cuda:0", potential_temperature=300.0, advection=bz.WENO())
                Ny = size[1] // world
                m.set(θ=full[:, rank * Ny:(rank + 1) * Ny, :], u=3.0, v=-2.0)
                for _ in range(case.steps):
                    m.time_step(case.dt)
                m.synchronize()
            models[rank] = m
        except Exception as e:      # noqa: BLE001
            import traceback
            errors.append((rank, repr(e), traceback.format_exc()))

    threads = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for m in models:      # the rank-local grids carry the global grid's eltype: the Float32 twin is what ran
        assert m.grid.ftype == 4 and m.momentum["ρu"].parent.dtype == torch.float32
        assert m._lib is bz._lib.load_f32()
    mom = max(np.abs(og.interior(getattr(om, n), n == "rw")).max() for n in ("ru", "rv", "rw"))
    got_all = {}
    for n, k in PROG.items():
        if n == "rq":
            continue
        got = np.concatenate([m.prognostic_fields()[k].interior_cpu().astype(np.float64) for m in models], axis=1)
        got_all[n] = got
        want = og.interior(getattr(om, n), n == "rw")
        scale = mom if n in ("ru", "rv", "rw") else np.abs(want).max()
        assert np.abs(got - want).max() / scale < 1e-4, (n, np.abs(got - want).max() / scale)
    want_all = fc.oracle_fields(om, got_all)
    assert_increments(case.name, got_all, want_all, {n: start[n] for n in got_all}, case.kind)


@pytest.mark.gpu
def test_float32_bounded_moisture_steps_match_the_float64_oracle(oracle, oc, bz):
    """examples/rico.jl:40,184-190: Float32 + bounds-preserving WENO for the moisture density; three steps of the sharp-edged blob against the
    Float64 oracle (1e-4 of each field's scale) and no overshoot beyond the limiter's own tolerance."""
    case = fc.STEP_CASES["bounded_moisture"]
    om, hm = case.build(oracle, oc, bz)
    start = fc.oracle_fields(om, case.fields)
    for _ in range(case.steps):
        om.time_step(case.dt)
        hm.time_step(case.dt)
    hm.synchronize()
    assert_increments(case.name, fc.device_fields(hm, case.fields), fc.oracle_fields(om, case.fields), start, case.kind)
    e = _steps_errors(om, hm, [(n, hm.prognostic_fields()[k]) for n, k in PROG.items()])
    print("float32 bounded:", {k: f"{v:.1e}" for k, v in e.items()})
    assert max(e.values()) < 1e-4, e


@pytest.mark.gpu
def test_float32_compressible_kessler_on_library_slabs_matches_the_single_gpu_model(bz):
    """configs[4] in the example's precision, decomposed: the Float32 twin's library-owned compressible step (per-substep halo exchanges)
    on two ranks against the single-GPU Float32 model (itself checked against the Float64 oracle above)."""
    import threading
    import uuid
    import torch
    case = fc.STEP_CASES["slab_compressible"]      # the oracle side of this set-up (tests/f32_cases.py) keeps its tolerance honest
    size, steps, dt = fc.SLAB_SIZE, case.steps, case.dt
    ext = fc.SLAB_EXT
    G = bz.RectilinearGrid(size, x=ext[0], y=ext[1], z=ext[2], float_type=np.float32)
    dynamics = lambda: bz.CompressibleDynamics(bz.SplitExplicitTimeDiscretization(substeps=6), reference_potential_temperature=300.0)
    mkw = dict(thermodynamic_constants=bz.ThermodynamicConstants(saturation_vapor_pressure=bz.TetensFormula()), microphysics=bz.DCMIP2016KesslerMicrophysics())
    ref = bz.CompressibleAtmosphereModel(G, dynamics(), advection=bz.WENO(), **mkw)
    rho = np.asarray(ref.dynamics.reference_state.density)[G.Hz:G.Hz + G.Nz][:, None, None]
    θ, qv = fc.slab_theta, fc.slab_qv
    ic = dict(ρ=rho, θ=θ, u=3.0, v=-2.0, w=0.0, qᵗ=qv)
    ref.set(**ic)
    ref.synchronize()
    inc_names = {"ρᵈ": "rho_d", "ρu": "ru", "ρw": "rw", "ρθ": "rtheta", "ρq": "rq"}
    start = {n: fc.COMPRESSIBLE_GET[n](ref).interior_cpu().astype(np.float64) for n in inc_names.values()}
    for _ in range(steps):
        ref.time_step(dt)
    ref.synchronize()
    world, group = 2, "local:" + uuid.uuid4().hex
    models, errors = [None] * world, []

    def run(rank):
        try:
            torch.cuda.set_device(0)
            with torch.cuda.stream(torch.cuda.Stream()):
                m = bz.compressible.SlabCompressibleModel(G, rank, world, dynamics(), advection=bz.WENO(), device="cuda:0", transport=group, **mkw)
                m.set(**ic)
                for _ in range(steps):
                    m.time_step(dt)
                m.synchronize()
            models[rank] = m
        except Exception as e:      # noqa: BLE001
            import traceback
            errors.append((rank, repr(e), traceback.format_exc()))

    threads = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for m in models:
        assert m.grid.ftype == 4 and m.momentum["ρu"].parent.dtype == torch.float32
        assert m._lib is bz._lib.load_f32()
    getters = {"ρᵈ": lambda m: m.dynamics.dry_density, "ρu": lambda m: m.momentum["ρu"], "ρw": lambda m: m.momentum["ρw"],
               "ρθ": lambda m: m.potential_temperature_density, "ρq": lambda m: m.moisture_density}
    mom = max(np.abs(getters[k](ref).interior_cpu()).max() for k in ("ρu", "ρw"))
    slabs, single = {}, {}
    for name, get in getters.items():
        got = np.concatenate([get(m).interior_cpu().astype(np.float64) for m in models], axis=1)
        want = get(ref).interior_cpu().astype(np.float64)
        scale = mom if name in ("ρu", "ρw") else np.abs(want).max()
        assert np.abs(got - want).max() / scale < 1e-4, (name, np.abs(got - want).max() / scale)      # Float32 round-off through different kernel sequences (App. C: 1e-4 after steps)
        slabs[inc_names[name]], single[inc_names[name]] = got, want
    # judged by the single-GPU run's own increments (device against device: the oracle side of the set-up is tests/f32_cases.py's)
    assert_increments("slab_compressible", slabs, single, start, "compressible")


@pytest.mark.gpu
def test_float32_two_dimensional_models_match_the_float64_oracle(oracle, oc, bz):
    """(Periodic, Flat, Bounded) on Float32 grids, both dynamical cores: the 2-D bubble through the anelastic per-operator kernels and the
    inertia-gravity-wave set-up through the compressible split-explicit model, three steps each against the Float64 oracle."""
    # anelastic
    case = fc.STEP_CASES["two_d_anelastic"]
    om, hm = case.build(oracle, oc, bz)
    start = fc.oracle_fields(om, case.fields)
    for _ in range(case.steps):
        om.time_step(case.dt)
        hm.time_step(case.dt)
    hm.synchronize()
    assert_increments(case.name, fc.device_fields(hm, case.fields), fc.oracle_fields(om, case.fields), start, case.kind)
    e = _steps_errors(om, hm, [(n, hm.prognostic_fields()[k]) for n, k in PROG.items() if n not in ("rq", "rv")])
    print("float32 2-D anelastic:", {k: f"{v:.1e}" for k, v in e.items()})
    assert max(e.values()) < 1e-4, e
    # compressible inertia-gravity wave
    case = fc.STEP_CASES["two_d_compressible"]
    om, hm = case.build(oracle, oc, bz)
    og = om.grid
    start = fc.oracle_fields(om, case.fields)
    for _ in range(case.steps):
        om.time_step(case.dt)
        hm.time_step(case.dt)
    hm.synchronize()
    assert_increments(case.name, fc.device_fields(hm, case.fields, compressible=True), fc.oracle_fields(om, case.fields), start, case.kind)
    I = og.interior
    for n, f in (("rho_d", hm.dynamics.dry_density), ("rtheta", hm.potential_temperature_density), ("ru", hm.momentum["ρu"])):
        want = I(getattr(om, n))
        assert np.abs(f.interior_cpu().astype(np.float64) - want).max() / np.abs(want).max() < 1e-5, n
    assert np.abs(hm.momentum["ρv"].interior_cpu()).max() == 0.0


@pytest.mark.gpu
def test_float32_mixed_orders_with_a_sponge_match_the_float64_oracle(oracle, oc, bz):
    """Float32 twin of the round-3 options: momentum WENO(order = 9) with WENO(order = 5) scalars (bounds-preserving moisture) and rico.jl's
    w sponge (examples/rico.jl:40,103-105,164,184-190 is a Float32 model), three steps against the Float64 oracle."""
    case = fc.STEP_CASES["mixed_orders"]
    om, hm = case.build(oracle, oc, bz)
    start = fc.oracle_fields(om, case.fields)
    for _ in range(case.steps):
        om.time_step(case.dt)
        hm.time_step(case.dt)
    hm.synchronize()
    assert_increments(case.name, fc.device_fields(hm, case.fields), fc.oracle_fields(om, case.fields), start, case.kind)
    e = _steps_errors(om, hm, [(n, hm.prognostic_fields()[k]) for n, k in PROG.items()])
    print("float32 mixed orders + sponge:", {k: f"{v:.1e}" for k, v in e.items()})
    assert max(e.values()) < 1e-4, e


@pytest.mark.gpu
def test_float32_marching_closure_kernels_carry_the_bits_of_the_cell_per_thread_kernels(oracle, bz, monkeypatch):
    """Round 5: on whole 64 x 8 tiles SmagorinskyLilly runs as z-marching LDS-tiled kernels (csrc/bz_closure.hip); the Float32 twin of
    those kernels against the Float32 cell-per-thread kernels (BZ_NO_CLOSURE_MARCH=1): nu_e and every tendency bit for bit, three steps
    of the BOMEX physics list bit for bit (same expressions, same order)."""
    import sys
    import os
    sys.path.insert(0, os.path.dirname(__file__))
    from test_closure import _turbulent_ic
    from test_forcings import EXTENT, _hip_forcing_kwargs
    size = (64, 16, 32)
    og = oracle.Grid(size, x=EXTENT[0], y=EXTENT[1], z=EXTENT[2])
    om = oracle.OracleModel(og, surface_pressure=101500.0, potential_temperature=299.1)
    ic = _turbulent_ic(om, 7)

    def run(no_march):
        if no_march:
            monkeypatch.setenv("BZ_NO_CLOSURE_MARCH", "1")
        else:
            monkeypatch.delenv("BZ_NO_CLOSURE_MARCH", raising=False)
        grid = bz.RectilinearGrid(size, x=EXTENT[0], y=EXTENT[1], z=EXTENT[2], float_type=np.float32)
        ref = bz.ReferenceState(grid, surface_pressure=101500.0, potential_temperature=299.1)
        hm = bz.AtmosphereModel(grid, dynamics=bz.AnelasticDynamics(ref), advection=bz.WENO(order=5), closure=bz.SmagorinskyLilly(),
                                microphysics=bz.SaturationAdjustment(equilibrium=bz.WarmPhaseEquilibrium()), **_hip_forcing_kwargs(bz))
        hm.set(θ=ic["theta"], qᵗ=ic["qt"], u=ic["u"], v=ic["v"])
        bz.update_state_(hm, compute_tendencies=True)
        hm.synchronize()
        first = {"nu": hm.closure_fields["νₑ"].interior_cpu().copy()}
        first.update({k: f.interior_cpu().copy() for k, f in hm.G.items()})
        for _ in range(3):
            hm.time_step(3.0)
        hm.synchronize()
        return first, {k: f.interior_cpu() for k, f in hm.prognostic_fields().items()}

    fa, sa = run(False)
    fb, sb = run(True)
    assert fa["nu"].max() > 0
    for k in fa:
        assert np.array_equal(fa[k], fb[k]), k
    for k in sa:
        assert np.array_equal(sa[k], sb[k]), k
        assert np.isfinite(sa[k]).all(), k
