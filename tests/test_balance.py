"""Discrete hydrostatic balance on the device (csrc/bz_balance.hip through the C ABI and the host API of breeze.jl_amd/compressible.py)
against the numpy restatement tests/balance_reference.py (pinned by tests/test_balance_reference.py).

Shapes: (40, 6, 5) ragged Nx (40 of a wave's 64 lanes, 40 of a block's 256); (64, 8, 33) one full wave per row, odd Nz; (128, 16, 12) two
waves per row; (24, 1, 16) Flat y (the y face mean is the identity); (16, 8, 3) the shortest recurrence a grid allows — the library needs
Nz >= Hz >= 3 (RectilinearGrid refuses (16, 8, 2): a halo cannot be wider than the domain, pinned in tests/test_balance_reference.py), the two-level recurrence runs in
tests/test_balance_reference.py.  Each on a uniform and a stretched z (whole-number faces: the metrics are exact in Float32 too) and with
halos 3 and 5 where the grid allows (the compressible model needs Ny >= 2 Hy: (128, 16, 12) and the Flat (24, 1, 16)); (16, 8, 64) joins the
column kernel as the long column of the Float32 bound.

Tolerances.  1e-12 relative, element by element, against the float64 restatement (the project's single-operator tolerance; the
restatement is within 3e-15 of its longdouble evaluation).  Balance: 8 eps p[k-1]/Δzᶠ[k] on the device's own output.  Float32 twin: the
device's error against the longdouble column on the same (Float32-rounded) inputs and constants within 4x the error of the restatement
run in numpy float32.  Specific quantities after the balanced set: θ, q within 4 eps, velocities within 8 eps (tests/test_balance_reference.py)."""
import copy
import ctypes as C

import numpy as np
import pytest

import balance_reference as br

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float64).eps)
P0, PST = 101325.0, 1e5
SHAPES = [(40, 6, 5), (64, 8, 33), (128, 16, 12), (24, 1, 16), (16, 8, 3)]
GRIDS = [(s, st, 3) for s in SHAPES for st in (False, True)] + [(s, st, 5) for s in ((128, 16, 12), (24, 1, 16)) for st in (False, True)]
COLUMN_GRIDS = GRIDS + [((16, 8, 64), False, 3), ((16, 8, 64), True, 3)]
F32_GRIDS = [((64, 8, 33), False, 3), ((64, 8, 33), True, 3), ((16, 8, 64), False, 3), ((16, 8, 64), True, 3), ((40, 6, 5), True, 3)]


def _faces(Nz, stretched):
    if not stretched:
        return np.linspace(0.0, 100.0 * Nz, Nz + 1)
    s = np.linspace(0.0, 1.0, Nz + 1)
    return np.round(100.0 * Nz * (0.5 * s + 0.5 * s ** 2))      # whole-number faces


def _grid(bz, shape, stretched, halo, float_type=np.float64, walls=False):
    Nx, Ny, Nz = shape
    zf = _faces(Nz, stretched)
    z = zf if stretched else (0.0, 100.0 * Nz)
    if Ny == 1:
        return bz.RectilinearGrid((Nx, Nz), x=(0.0, 100.0 * Nx), z=z, halo=(halo, halo), topology=(bz.Periodic, bz.Flat, bz.Bounded), float_type=float_type)
    topo = (bz.Periodic, bz.Bounded, bz.Bounded) if walls else (bz.Periodic, bz.Periodic, bz.Bounded)
    return bz.RectilinearGrid(shape, x=(0.0, 100.0 * Nx), y=(0.0, 100.0 * Ny), z=z, halo=halo, topology=topo, float_type=float_type)


def _model(bz, grid, micro=None, reference=300.0, substep_floattype=None, reference_state="auto"):
    td = bz.SplitExplicitTimeDiscretization(substeps=6)
    kw = dict(reference_state=reference_state) if reference_state != "auto" else dict(reference_potential_temperature=reference)
    dyn = bz.CompressibleDynamics(td, surface_pressure=P0, **kw)
    mk = {}
    if micro == "Kessler":
        mk = dict(thermodynamic_constants=bz.ThermodynamicConstants(saturation_vapor_pressure=bz.TetensFormula()),
                  microphysics=bz.DCMIP2016KesslerMicrophysics())
    elif micro == "SaturationAdjustment":
        mk = dict(microphysics=bz.SaturationAdjustment(equilibrium=bz.WarmPhaseEquilibrium()))
    return bz.CompressibleAtmosphereModel(grid, dyn, advection=bz.WENO(order=5), substep_floattype=substep_floattype, **mk)


_MODELS = {}


def _cached_model(bz, shape, stretched, halo, float_type=np.float64):
    key = (shape, stretched, halo, np.dtype(float_type).name)
    if key not in _MODELS:
        _MODELS[key] = _model(bz, _grid(bz, shape, stretched, halo, float_type))
    return _MODELS[key]


def _inputs(shape, stretched, seed, vapour=True):
    """θ, q, qᶜˡ, qʳ, u, v, w that vary in x, y and z: a stratified column with a wave and noise"""
    Nx, Ny, Nz = shape
    rng = np.random.default_rng(seed)
    sh = (Nz, Ny, Nx)
    zf = _faces(Nz, stretched)
    zc = (0.5 * (zf[:-1] + zf[1:])).reshape(-1, 1, 1)
    x = (np.arange(Nx) + 0.5).reshape(1, 1, -1) / Nx
    y = (np.arange(Ny) + 0.5).reshape(1, -1, 1) / Ny
    wave = np.sin(2 * np.pi * x + 0.3) * np.cos(2 * np.pi * y - 0.2)
    th = 300.0 + 0.004 * zc + 1.5 * wave + rng.uniform(-0.5, 0.5, sh)
    q = 0.015 * np.exp(-zc / 2500.0) * (1.0 + 0.2 * wave) * rng.uniform(0.8, 1.2, sh) if vapour else np.zeros(sh)
    w = rng.normal(0.0, 1.0, (Nz + 1, Ny, Nx))
    w[0] = w[Nz] = 0.0
    return dict(th=th, q=q, qcl=rng.uniform(0.0, 1e-3, sh), qr=rng.uniform(0.0, 1e-3, sh), u=5.0 * wave + rng.normal(0.0, 1.0, sh),
                v=rng.normal(0.0, 1.0, sh), w=w)


def _field(bz, model, values=None, fill=float("nan")):
    f = bz.Field(model.grid, (bz.Center, bz.Center, bz.Center), model.device)
    f.parent.fill_(fill)
    if values is not None:
        f.set_interior(values)
    return f


def _close(got, want, rtol, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    err = np.abs(got - want)
    worst = float(np.max(np.where(want != 0, err / np.where(want != 0, np.abs(want), 1.0), np.where(err == 0, 0.0, np.inf))))
    print(f"    {what}: {worst:.2e}")
    assert worst <= rtol, (what, worst)
    return worst


# ---- the column kernel ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("moist", [False, True])
@pytest.mark.parametrize("shape,stretched,halo", COLUMN_GRIDS)
def test_exner_columns(bz, shape, stretched, halo, moist):
    from breeze_jl_amd.compressible import exner_columns_
    m = _cached_model(bz, shape, stretched, halo)
    constants = br.constants_tuple(m.thermodynamic_constants)
    I = _inputs(shape, stretched, seed=7)
    th, qv = _field(bz, m, I["th"]), (_field(bz, m, I["q"]) if moist else None)      # NaN in every halo cell
    out = [_field(bz, m, fill=-7.0) for _ in range(3)]
    exner_columns_(m, th, qv, P0, *out)
    m.synchronize()
    dzc, dzf = br.z_metrics(_faces(shape[2], stretched))
    want = br.exner_columns(I["th"], I["q"] if moist else None, dzc, dzf, P0, PST, constants)
    print(f"exner columns {shape} stretched={stretched} halo={halo} moist={moist}")
    got = [f.interior_cpu() for f in out]
    for name, a, b in zip(("exner", "pressure", "density"), got, want):
        assert np.all(np.isfinite(a)), name
        _close(a, b, 1e-12, name)
    ratio = br.balance_ratio(got[1], got[2], dzf, constants[0], EPS)
    print(f"    balance: {ratio:.2f} eps p/dz")
    assert ratio <= 8.0
    for f in out:      # nothing but the interior is written
        parent = f.cpu().copy()
        parent[m.grid.interior_slices(False)] = -7.0
        assert np.all(parent == -7.0)


@pytest.mark.parametrize("moist", [False, True])
@pytest.mark.parametrize("shape,stretched,halo", F32_GRIDS)
def test_exner_columns_float32_twin(bz, shape, stretched, halo, moist):
    from breeze_jl_amd.compressible import exner_columns_
    m = _cached_model(bz, shape, stretched, halo, np.float32)
    f32 = np.float32
    constants = tuple(float(f32(c)) for c in br.constants_tuple(m.thermodynamic_constants))      # what the Float32 ABI carries
    I = _inputs(shape, stretched, seed=7)
    th32, q32 = I["th"].astype(f32), I["q"].astype(f32)
    th, qv = _field(bz, m, th32), (_field(bz, m, q32) if moist else None)
    out = [_field(bz, m, fill=-7.0) for _ in range(3)]
    exner_columns_(m, th, qv, P0, *out)
    m.synchronize()
    dzc, dzf = br.z_metrics(_faces(shape[2], stretched))      # whole numbers and halves: exact in Float32
    args = (th32, q32 if moist else None, dzc, dzf, P0, PST, constants)
    exact = br.exner_columns(*args, dtype=np.longdouble)
    numpy32 = br.exner_columns(*args, dtype=f32)
    print(f"exner columns Float32 {shape} stretched={stretched} moist={moist}")
    for name, f, n32, ex in zip(("exner", "pressure", "density"), out, numpy32, exact):
        got = f.interior_cpu()
        assert got.dtype == f32 and np.all(np.isfinite(got))
        e_dev, e_np = br.max_rel(got, ex), br.max_rel(n32, ex)
        print(f"    {name}: device {e_dev:.2e}, numpy float32 {e_np:.2e}")
        assert e_dev <= 4.0 * e_np, (name, e_dev, e_np)


# ---- the balanced set -----------------------------------------------------------------------------------------------------------------
_SET_NAMES = {"rho_d": "ρᵈ", "ru": "ρu", "rv": "ρv", "rw": "ρw", "rth": "ρθ", "rq": "ρq", "rqcl": "ρqᶜˡ", "rqr": "ρqʳ"}


def _device_state(m):
    return {k: m.prognostic_fields()[name].interior_cpu().copy() for k, name in _SET_NAMES.items() if name in m.prognostic_fields()}


def _check_balanced(bz, m, want, shape, stretched, kessler, dry, constants, dzf):
    got = _device_state(m)
    for k in got:
        _close(got[k], want[k], 1e-12, _SET_NAMES[k])
    Nz = shape[2]
    assert not got["rw"][0].any() and not got["rw"][Nz].any()      # the wall faces hold the zeros update_state! left there before the call
    rho = m.dynamics.total_density.interior_cpu()
    S = got["rq"] + ((got["rqcl"] + (got["rqr"] + 0.0)) if kessler else 0.0)
    assert np.array_equal(rho, got["rho_d"] + S)
    if dry:
        ratio = br.balance_ratio(m.dynamics.pressure.interior_cpu(), rho, dzf, constants[0], EPS)
        print(f"    model pressure and total density, balance: {ratio:.2f} eps p/dz")
        assert ratio <= 8.0


@pytest.mark.parametrize("micro", ["dry", "vapour", "SaturationAdjustment", "Kessler"])
@pytest.mark.parametrize("shape,stretched,halo", GRIDS)
def test_set_hydrostatically_balanced_density(bz, shape, stretched, halo, micro):
    kessler, dry = micro == "Kessler", micro == "dry"
    m = _model(bz, _grid(bz, shape, stretched, halo), micro=micro if micro in ("Kessler", "SaturationAdjustment") else None)
    constants = br.constants_tuple(m.thermodynamic_constants)
    I = _inputs(shape, stretched, seed=11, vapour=not dry)
    kw = dict(θ=I["th"], qᵗ=I["q"], u=I["u"], v=I["v"], w=I["w"])
    if kessler:
        kw.update(qᶜˡ=I["qcl"], qʳ=I["qr"])
    # surface_pressure=None takes the dynamics' (P0): half of the cases spell it out
    m.set(ρ=bz.HydrostaticallyBalancedDensity(None if stretched else P0), **kw)
    m.synchronize()
    # the deferred path: unit placeholder in ρᵈ, so phase 2 left ρθ = θ, ρq = q, ρu = u, ... and update_state! zeros on the wall faces of ρw
    Nx, Ny, Nz = shape
    one = np.ones((Nz, Ny, Nx))
    state = {"rho_d": one, "ru": I["u"], "rv": I["v"], "rw": I["w"], "rth": I["th"], "rq": I["q"]}
    if kessler:
        state.update(rqcl=I["qcl"], rqr=I["qr"])
    dzc, dzf = br.z_metrics(_faces(Nz, stretched))
    want = br.balanced_set(state, I["th"], dzc, dzf, P0, PST, constants, kessler=kessler, flat_y=Ny == 1)
    print(f"balanced set {shape} stretched={stretched} halo={halo} {micro}")
    _check_balanced(bz, m, want, shape, stretched, kessler, dry, constants, dzf)
    # specific quantities come back
    _close(m.potential_temperature.interior_cpu(), I["th"], 4 * EPS, "θ")
    _close(m.velocities["u"].interior_cpu(), I["u"], 8 * EPS, "u")
    _close(m.velocities["v"].interior_cpu(), I["v"], 8 * EPS, "v")
    _close(m.velocities["w"].interior_cpu(), I["w"], 8 * EPS, "w")
    if not dry:
        _close(m.specific_moisture.interior_cpu(), I["q"], 4 * EPS, "q")
    else:
        assert not m.specific_moisture.interior_cpu().any()
    if kessler:
        _close(m.microphysical_fields["qᶜˡ"].interior_cpu(), I["qcl"], 4 * EPS, "qᶜˡ")
        _close(m.microphysical_fields["qʳ"].interior_cpu(), I["qr"], 4 * EPS, "qʳ")


@pytest.mark.parametrize("micro", ["vapour", "Kessler"])
@pytest.mark.parametrize("shape,stretched,halo", [((40, 6, 5), True, 3), ((24, 1, 16), False, 3), ((128, 16, 12), True, 5)])
def test_balanced_density_from_a_state_with_its_own_density(bz, shape, stretched, halo, micro):
    """set_hydrostatically_balanced_density! on a state whose old dry density varies in space (the unit placeholder of the deferred path
    makes every old face mean a 1): every ratio of face means is exercised"""
    from breeze_jl_amd.compressible import set_hydrostatically_balanced_density_
    kessler = micro == "Kessler"
    m = _model(bz, _grid(bz, shape, stretched, halo), micro="Kessler" if kessler else None)
    constants = br.constants_tuple(m.thermodynamic_constants)
    I = _inputs(shape, stretched, seed=13)
    Nx, Ny, Nz = shape
    rng = np.random.default_rng(3)
    zc = 0.5 * (_faces(Nz, stretched)[:-1] + _faces(Nz, stretched)[1:]).reshape(-1, 1, 1)
    kw = dict(ρ=1.2 * np.exp(-zc / 8000.0) * rng.uniform(0.9, 1.1, (Nz, Ny, Nx)), θ=I["th"], qᵗ=I["q"], u=I["u"], v=I["v"], w=I["w"])
    if kessler:
        kw.update(qᶜˡ=I["qcl"], qʳ=I["qr"])
    m.set(**kw)
    m.synchronize()
    state = _device_state(m)
    theta = m.potential_temperature.interior_cpu().copy()
    set_hydrostatically_balanced_density_(m, bz.HydrostaticallyBalancedDensity(surface_pressure=1.0e5))
    m.synchronize()
    dzc, dzf = br.z_metrics(_faces(Nz, stretched))
    want = br.balanced_set(state, theta, dzc, dzf, 1.0e5, PST, constants, kessler=kessler, flat_y=Ny == 1)
    print(f"balanced density of a set state {shape} stretched={stretched} halo={halo} {micro}")
    _check_balanced(bz, m, want, shape, stretched, kessler, False, constants, dzf)
    _close(m.potential_temperature.interior_cpu(), theta, 4 * EPS, "θ")


@pytest.mark.parametrize("micro", ["vapour", "Kessler"])
@pytest.mark.parametrize("shape,stretched", [((40, 6, 5), True), ((64, 8, 33), False)])
def test_balanced_set_float32_twin(bz, shape, stretched, micro):
    """the Float32 library: every prognostic array's error against the longdouble restatement on the same (Float32-rounded) inputs and
    constants within 4x the error of the restatement run in numpy float32 (measured 0.87 … 1.13 of it)"""
    f32 = np.float32
    kessler = micro == "Kessler"
    m = _model(bz, _grid(bz, shape, stretched, 3, f32), micro="Kessler" if kessler else None)
    constants = tuple(float(f32(c)) for c in br.constants_tuple(m.thermodynamic_constants))
    I = {k: v.astype(f32) for k, v in _inputs(shape, stretched, seed=29).items()}
    kw = dict(θ=I["th"], qᵗ=I["q"], u=I["u"], v=I["v"], w=I["w"])
    if kessler:
        kw.update(qᶜˡ=I["qcl"], qʳ=I["qr"])
    m.set(ρ=bz.HydrostaticallyBalancedDensity(P0), **kw)
    m.synchronize()
    Nx, Ny, Nz = shape
    state = {"rho_d": np.ones((Nz, Ny, Nx), dtype=f32), "ru": I["u"], "rv": I["v"], "rw": I["w"], "rth": I["th"], "rq": I["q"]}
    if kessler:
        state.update(rqcl=I["qcl"], rqr=I["qr"])
    dzc, dzf = br.z_metrics(_faces(Nz, stretched))
    args = (state, I["th"], dzc, dzf, P0, PST, constants)
    exact = br.balanced_set(*args, kessler=kessler, dtype=np.longdouble)
    numpy32 = br.balanced_set(*args, kessler=kessler, dtype=f32)
    got = _device_state(m)
    print(f"balanced set Float32 {shape} stretched={stretched} {micro}")
    for k in got:
        assert got[k].dtype == f32 and np.all(np.isfinite(got[k]))
        sel = slice(1, Nz) if k == "rw" else slice(None)      # the wall faces of ρw are exact zeros
        e_dev, e_np = br.max_rel(got[k][sel], exact[k][sel]), br.max_rel(numpy32[k][sel], exact[k][sel])
        print(f"    {_SET_NAMES[k]}: device {e_dev:.2e}, numpy float32 {e_np:.2e}")
        assert e_dev <= 4.0 * e_np, (k, e_dev, e_np)
    assert not got["rw"][0].any() and not got["rw"][Nz].any()


# ---- replacing the reference state ----------------------------------------------------------------------------------------------------
def _perturbed_moist(shape, stretched):
    I = _inputs(shape, stretched, seed=17)
    Nx, Ny, Nz = shape
    zf = _faces(Nz, stretched)
    zc = (0.5 * (zf[:-1] + zf[1:])).reshape(-1, 1, 1)
    rng = np.random.default_rng(19)
    return dict(ρ=1.16 * np.exp(-zc / 8500.0) * rng.uniform(0.999, 1.001, (Nz, Ny, Nx)), θ=I["th"], qᵗ=I["q"], u=I["u"], v=I["v"], w=0.1 * I["w"])


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("substep_floattype", [None, np.float32])
@pytest.mark.parametrize("shape,stretched", [((40, 6, 5), False), ((64, 8, 33), True)])
def test_reference_replacement_is_bitwise_a_fresh_model(bz, shape, stretched, substep_floattype, graph):
    import torch
    from breeze_jl_amd.compressible import update_state_
    dt = 0.2
    ic = _perturbed_moist(shape, stretched)
    m1 = _model(bz, _grid(bz, shape, stretched, 3), reference=lambda z: 295.0 + 0.002 * z, substep_floattype=substep_floattype)
    replays0 = captures0 = 0
    if graph:      # a recording made with the old reference: ordinary step, recorded step, replayed step
        m1.set(**ic)
        m1.graph_enable(True)
        for _ in range(3):
            m1.time_step(dt)
        _, captures0, replays0 = m1.graph_info()
        assert captures0 == 1 and replays0 == 1
    before = [a.copy() for a in (m1.dynamics.reference_state.pressure, m1.dynamics.reference_state.density)]
    m1.set(compute_reference_state=True, **ic)
    m1.clock.iteration = 0      # both models prepare their first step (maybe_prepare_first_time_step!)
    ref = m1.dynamics.reference_state
    assert not np.array_equal(ref.pressure, before[0]) and not np.array_equal(ref.density, before[1])
    # a fresh model built from exactly the arrays the host object now holds, with the same prognostic state
    m2 = _model(bz, _grid(bz, shape, stretched, 3), substep_floattype=substep_floattype, reference_state=copy.deepcopy(ref))
    for k, f in m1.prognostic_fields().items():
        m2.prognostic_fields()[k].parent.copy_(f.parent)
    update_state_(m2, compute_tendencies=False)
    counts = []
    for _ in range(3):
        m1.time_step(dt)
        m2.time_step(dt)
        counts.append(m1.graph_info())
    m1.synchronize()
    m2.synchronize()
    for k, f in m1.prognostic_fields().items():
        assert torch.equal(f.parent, m2.prognostic_fields()[k].parent), k
    for a, b in ((m1.dynamics.pressure, m2.dynamics.pressure), (m1.temperature, m2.temperature), (m1.dynamics.total_density, m2.dynamics.total_density)):
        assert torch.equal(a.parent, b.parent)
    assert torch.isfinite(m1.dynamics.pressure.interior).all()
    if graph:
        # no recording survives the replacement: the first two steps after it are an ordinary and a newly recorded one, so the replay count
        # stands where it was; only the third step replays — the NEW recording (one more capture)
        assert counts[0][2] == replays0 and counts[1][2] == replays0
        assert counts[1][1] == captures0 + 1
        assert counts[2][2] == replays0 + 1


def test_set_to_mean_known_answer_and_keyword_order(bz):
    """reference_states.jl:532-611,628-634 on the device: built at 290, set uniformly to 305 with compute_reference_state, the columns are a
    fresh ExnerReferenceState(305); the reference survives a plain set!; a model without a reference ignores the keyword; with both
    keywords the reference is computed first, from the placeholder state (q of the field is q / (1 + q) there), then the density."""
    shape = (40, 6, 5)
    grid = _grid(bz, shape, False, 3)
    m = _model(bz, grid, reference=290.0)
    ref = m.dynamics.reference_state
    built = ref.pressure.copy()
    m.set(ρ=1.0, θ=305.0, qᵗ=0.0)
    assert np.array_equal(ref.pressure, built)
    m.set(ρ=1.0, θ=305.0, qᵗ=0.0, compute_reference_state=True)
    assert m.dynamics.reference_state is ref
    fresh = bz.ExnerReferenceState(grid, surface_pressure=P0, potential_temperature=305.0)
    H, Nz = grid.Hz, grid.Nz
    for name in ("exner_function", "pressure", "density"):
        assert br.max_rel(getattr(ref, name)[H:H + Nz], getattr(fresh, name)[H:H + Nz]) <= 1e-13, name
    # set_to_mean_ by itself
    m.set(ρ=1.0, θ=300.0, qᵗ=0.0)
    bz.set_to_mean_(ref, m)
    fresh = bz.ExnerReferenceState(grid, surface_pressure=P0, potential_temperature=300.0)
    assert br.max_rel(ref.pressure[H:H + Nz], fresh.pressure[H:H + Nz]) <= 1e-13
    # no reference: a no-op
    n = _model(bz, grid, reference_state=None)
    n.set(ρ=1.0, θ=305.0, qᵗ=0.0, compute_reference_state=True)
    assert n.dynamics.reference_state is None
    # both keywords
    I = _inputs(shape, False, seed=23)
    m.set(ρ=bz.HydrostaticallyBalancedDensity(), θ=I["th"], qᵗ=I["q"], compute_reference_state=True)
    N = shape[0] * shape[1]
    first = bz.ExnerReferenceState.from_profiles(grid, I["th"].sum(axis=(1, 2)) / N, (I["q"] / (1.0 + I["q"])).sum(axis=(1, 2)) / N, surface_pressure=P0)
    second = bz.ExnerReferenceState.from_profiles(grid, I["th"].sum(axis=(1, 2)) / N, I["q"].sum(axis=(1, 2)) / N, surface_pressure=P0)
    got = ref.density[H:H + Nz]
    assert br.max_rel(got, first.density[H:H + Nz]) <= 1e-12      # (the device's level sums associate differently: a few eps on the means)
    assert br.max_rel(got, second.density[H:H + Nz]) > 1e-6
    _close(m.specific_moisture.interior_cpu(), I["q"], 4 * EPS, "q after both keywords")


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
class _NoExchange:
    rows = 0

    def exchange_y_halos(self, tensors):
        pass


def _c_refusals(m, code, word):
    """every new entry point (word None: bz_set_exner_reference_state alone) returns `code` and bz_last_error names it, with `word`"""
    T = m._T
    lib, ctx = m._lib, m._ctx
    f = m.potential_temperature
    arrays = [np.ones(m.grid.Nz + 2 * m.grid.Hz, dtype=T.np_real) for _ in range(2)]
    ref = T.bz_exner_reference_state()
    ref.standard_pressure = m.dynamics.standard_pressure
    ref.pressure, ref.density = (a.ctypes.data_as(C.POINTER(T.real)) for a in arrays)
    calls = {"bz_set_exner_reference_state": lambda: lib.bz_set_exner_reference_state(ctx, C.byref(ref))}
    if word is not None:      # (the other two need no reference: a context without one runs them)
        out = [type(f)(m.grid, f.loc, m.device) for _ in range(3)]
        calls["bz_exner_columns"] = lambda: lib.bz_exner_columns(ctx, C.c_void_p(f.ptr()), None, P0, *(C.c_void_p(x.ptr()) for x in out))
        calls["bz_set_hydrostatically_balanced_density"] = lambda: lib.bz_set_hydrostatically_balanced_density(ctx, C.byref(m._state), P0)
    for name, call in calls.items():
        assert call() == code, name
        message = lib.bz_last_error(ctx).decode()
        assert name in message and (word is None or word in message), message


def test_refusals(bz):
    td = bz.SplitExplicitTimeDiscretization(substeps=6)
    balanced = bz.HydrostaticallyBalancedDensity(P0)
    # walls
    walled = _model(bz, _grid(bz, (16, 16, 8), False, 3, walls=True))
    # y-slab (one rank)
    G = _grid(bz, (16, 16, 8), False, 3)
    slab = bz.compressible.SlabCompressibleModel(G, 0, 1, bz.CompressibleDynamics(td, reference_potential_temperature=300.0), advection=bz.WENO(order=5),
                                                 device="cuda:0", decomp=_NoExchange())
    for m, word in ((walled, "Bounded"), (slab, "y-slab")):
        with pytest.raises(NotImplementedError, match="HydrostaticallyBalancedDensity.*" + word):
            m.set(ρ=balanced, θ=300.0)
        with pytest.raises(NotImplementedError, match="compute_reference_state.*" + word):
            m.set(ρ=1.0, θ=300.0, compute_reference_state=True)
        with pytest.raises(NotImplementedError, match="set_to_mean!.*" + word):
            bz.set_to_mean_(m.dynamics.reference_state, m)
        _c_refusals(m, 2, word)      # BZ_ERR_UNSUPPORTED, bz_last_error names the function
    # a context without a reference
    bare = _model(bz, G, reference_state=None)
    _c_refusals(bare, 1, None)       # BZ_ERR_INVALID
    assert "without a reference" in bare._lib.bz_last_error(bare._ctx).decode()
