"""Turbulence closures on the compressible split-explicit model (csrc/bz_closure.hip, csrc/bz_diffusivity.hip through the C ABI) against
the CPU restatement tests/compressible_closure_reference.py (pinned by tests/test_compressible_closure_reference.py).  Float64.

Kernels and shapes.  Whole 64 x 8 tiles (Nx % 64 == 0, Ny % 8 == 0, Nz >= 4) run the z-marching LDS-tiled kernels
k_smagorinsky_march<8, ExnerField> and k_closure_march<8, RhoField> (rho_d as a fifth rotating LDS plane; momentum and rho theta in one launch);
ragged grids, and every grid with BZ_NO_CLOSURE_MARCH=1, run the cell-per-thread k_smagorinsky_viscosity<ExnerField> (8 levels per workgroup)
and k_closure_tendencies<RhoField>.  The water scalars (k_water_closure, one launch) and the ScalarDiffusivity kernels
(k_diffusivity_momentum / k_diffusivity_scalar<.., RhoField>) are cell per thread on every grid.  The branch a shape reached is asserted from
the profile names (smagorinsky_march / closure_march against smagorinsky_viscosity / closure_tendencies):
    (40, 6, 5)     cell per thread: ragged row (40 of a block's 256 lanes), Nz below a halo of 5 and below the chunk of 8 levels
    (64, 8, 33)    march: one tile, odd number of levels, two chunks of levels (17 + 16)
    (128, 16, 12)  march: two tiles in x and two in y, every tile seam and the periodic wrap crossed; one chunk
The tiled and the cell-per-thread results of the two march shapes are compared at 1e-13 of the quantity's maximum (the expressions and
their order are the same; bitwise equality is not asserted).
each on a uniform and on a stretched z (whole-number faces) and with halos 3 and 5.  The compressible model needs Ny >= 2 Hy, so with a halo
of 5 the first two shapes are (40, 10, 5) and (64, 16, 33): the smallest with the same rows that the model accepts.

Inputs: random u, v, w of about 1 m/s on a stratified state with 100 m cells, 1 % vapour (rho_d and the total density differ: a kernel
that takes the wrong one fails the 1e-10 bound by eight orders), a block of fluid at rest (Sigma^2 = 0 exactly).  The restatement must show
all four classes of the stability factor and no sheared cell within 1e-3 of the switch C_b N^2+ / Sigma^2 = 1; both are asserted.
After the state is pushed, every halo cell of nu_e and of a field-valued K beyond the first is NaN, and the first halo cells of K hold
stale values: the library refills what it reads.  For nu_e alone (compute_closure_fields_) every model field is poisoned beyond its first
halo cell as well; the tendency entry points also advect, and WENO reads three cells, so the fields keep their halos there."""
import ctypes as C

import numpy as np
import pytest

import compressible_closure_reference as ccr
import scalar_diffusivity_reference as sdr

pytestmark = pytest.mark.gpu

SHAPES = [(40, 6, 5), (64, 8, 33), (128, 16, 12)]
SHAPES_HALO = [(s, 3) for s in SHAPES] + [((40, 10, 5), 5), ((64, 16, 33), 5), ((128, 16, 12), 5)]
PROG = {"rho_d": "ρᵈ", "ru": "ρu", "rv": "ρv", "rw": "ρw", "rtheta": "ρθ", "rq": "ρq"}
KES = {"rqcl": "ρqᶜˡ", "rqr": "ρqʳ"}
# seeds picked on the CPU so that the restatement shows the four classes of the stability factor and no sheared cell within 1e-3 of its switch


def _marches(shape):
    return shape[0] % 64 == 0 and shape[1] % 8 == 0 and shape[2] >= 4


SEEDS = {((40, 6, 5), False): 11, ((40, 6, 5), True): 11, ((64, 8, 33), False): 11, ((64, 8, 33), True): 12, ((128, 16, 12), False): 11,
         ((128, 16, 12), True): 14, ((40, 10, 5), False): 11, ((40, 10, 5), True): 11, ((64, 16, 33), False): 13, ((64, 16, 33), True): 11}


def _z_faces(Nz, stretched):
    if not stretched:
        return (0.0, 100.0 * Nz)
    s = np.linspace(0.0, 1.0, Nz + 1)
    return np.round(100.0 * Nz * (0.5 * s + 0.5 * s ** 2))      # whole-number faces (tests/test_scalar_diffusivity.py: _z_faces)


def _pair(oracle, oc, bz, shape, stretched=False, halo=3, closure=None, micro=None, order=5, coriolis=0.0, sponge=False, K=None, float_type=np.float64):
    """closure: None | "smagorinsky" | "isotropic" | "vertical"; K = (nu, kappa), numbers or (Nz, Ny, Nx) arrays (device: centre Fields,
    NaN beyond the interior until the library fills what it reads).  Returns (restatement, device model, {name: device K field})."""
    from oracle.closure import SmagorinskyLilly
    Nx, Ny, Nz = shape
    ext = dict(x=(0.0, 100.0 * Nx), y=(0.0, 100.0 * Ny), z=_z_faces(Nz, stretched))
    og = oracle.Grid(shape, halo=halo, **ext)
    kw = {}
    if closure == "smagorinsky":
        kw["closure"] = SmagorinskyLilly()
    elif closure is not None:
        kw["diffusivity"] = sdr.Diffusivity(int(closure == "vertical"), False, nu=K[0], kappa=K[1])
    td = dict(substeps=6, sponge=(0.2, 30.0 * Nz, "cubic")) if sponge else dict(substeps=6)
    om = ccr.ClosureCompressibleModel(og, time_discretization=oc.SplitExplicit(**td), reference_potential_temperature=300.0,
                                      microphysics=micro, advection=f"WENO{order}", coriolis_f=coriolis, **kw)
    grid = bz.RectilinearGrid(shape, halo=halo, float_type=float_type, **ext)
    fields = {}
    hc = None
    if closure == "smagorinsky":
        hc = bz.SmagorinskyLilly()
    elif closure is not None:
        hk = {}
        for name, value in zip(("ν", "κ"), K):
            if isinstance(value, np.ndarray):
                f = bz.Field(grid, (bz.Center, bz.Center, bz.Center), "cuda:0")
                f.parent.fill_(float("nan"))
                f.set_interior(value)
                hk[name] = fields[name] = f
            else:
                hk[name] = value
        hc = (bz.VerticalScalarDiffusivity if closure == "vertical" else bz.ScalarDiffusivity)(**hk)
    btd = bz.SplitExplicitTimeDiscretization(substeps=6, sponge=bz.UpperSponge(damping_rate=0.2, depth=30.0 * Nz, ramp=bz.CubicRamp()) if sponge else None)
    dyn = bz.CompressibleDynamics(btd, reference_potential_temperature=300.0)
    mk = {}
    if micro == "Kessler":
        mk = dict(thermodynamic_constants=bz.ThermodynamicConstants(saturation_vapor_pressure=bz.TetensFormula()),
                  microphysics=bz.DCMIP2016KesslerMicrophysics())
    elif micro == "SaturationAdjustment":
        mk = dict(microphysics=bz.SaturationAdjustment(equilibrium=bz.WarmPhaseEquilibrium()))
    hm = bz.CompressibleAtmosphereModel(grid, dyn, advection=bz.WENO(order=order), closure=hc,
                                        coriolis=bz.FPlane(f=coriolis) if coriolis else None, **mk)
    return om, hm, fields


def _initial(om, seed, vapour=0.01, rough=1.0):
    """keyword arrays of set!: a stratified column, 1 % density noise, u, v, w of about 1 m/s (rough = 1: white noise; below: a smooth wave plus
    that fraction of noise), a block of fluid at rest"""
    g = om.grid
    rng = np.random.default_rng(seed)
    sh = (g.Nz, g.Ny, g.Nx)
    x, y, z = g.nodes("ccc")
    Lx, Ly = g.Nx * g.dx, g.Ny * g.dy
    wave = np.broadcast_to(np.sin(2 * np.pi * x / Lx + 0.3) * np.cos(2 * np.pi * y / Ly - 0.2), sh)

    def field(shape=sh):
        n = rng.standard_normal(shape)
        return n if rough == 1.0 else (1 - rough) * wave[:1] * np.ones(shape) + rough * n

    # two layers, so that few cells sit near the switch of the stability factor: lively and almost neutral below (C_b N^2+ / Sigma^2 << 1, both
    # signs of N^2), a tenth of the wind and a stable 0.01 K/m above (>> 1)
    upper = np.arange(g.Nz) >= g.Nz // 2
    amp = np.where(upper, 0.1, 1.0)[:, None, None]
    ampf = np.where(np.arange(g.Nz + 1) > g.Nz // 2, 0.1, 1.0)[:, None, None]
    u, v, w = amp * field(), amp * field(), 0.5 * ampf * field((g.Nz + 1, g.Ny, g.Nx))
    w[0] = w[-1] = 0.0
    bi, bj, bk = slice(8, 16), slice(1, 5), slice(1, 4)
    u[bk, bj, bi] = 0.0
    v[bk, bj, bi] = 0.0
    w[1:5, bj, bi] = 0.0
    rho = om.ref.density[g.Hz:g.Hz + g.Nz][:, None, None] * (1.0 + (0.01 if rough == 1.0 else 0.001) * field())
    # 0.3 K of noise per cell for N^2, and a column-uniform 3 K pattern (0.7 wave + 0.3 noise, the mix and amplitude of
    # tests/test_gpu_compressible.py: seeded_state, whose 1e-12 bound on the full tendencies is used below) that leaves dz(log theta_v) alone:
    # WENO's smoothness indicators of theta = 300 K + perturbation are conditioned like 300 K / perturbation
    zmid = g.zf[g.Nz // 2]
    if rough == 1.0:
        theta = 300.0 + 0.0002 * np.minimum(z, zmid) + 0.01 * np.maximum(z - zmid, 0.0) + 0.3 * rng.standard_normal(sh) + \
            3.0 * (0.7 * wave[:1] + 0.3 * rng.standard_normal((1,) + sh[1:]))
    else:      # the stepped cases: close to the reference column (theta = 300 K), so that the acoustic adjustment of the first steps stays mild
        theta = 300.0 + 0.001 * z + 0.1 * field()
    ic = dict(rho=rho, theta=theta, u=u, v=v, w=w, qv=vapour * (1.0 + 0.3 * rng.random(sh)))
    if om.microphysics == "Kessler":
        ic.update(qcl=2e-4 * rng.random(sh), qr=1e-4 * rng.random(sh))
    return ic


def _push(om, hm):
    """the restatement's prognostic fields and time-averaged velocities into the device model, bit for bit; the device diagnoses the rest"""
    import torch
    from test_gpu_compressible import O2H
    names = ["rho_d", "ru", "rv", "rw", "rtheta", "rq"]
    for n in names:
        O2H[n](hm).parent.copy_(torch.from_numpy(getattr(om, n)))
    for n, k in KES.items():
        if om.microphysics == "Kessler":
            hm.microphysical_fields[k].parent.copy_(torch.from_numpy(getattr(om, n)))
    sub = hm.timestepper.substepper
    for n, k in (("au", "time_averaged_u"), ("av", "time_averaged_v"), ("aw", "time_averaged_w")):
        getattr(sub, k).parent.copy_(torch.from_numpy(getattr(om, n)))


def _poison_beyond_first_halo(f, zface=False):
    """NaN in every halo cell of a device field that is not adjacent to the interior"""
    import torch
    g = f.grid
    P = f.parent
    nz = g.Nz + (1 if zface else 0)
    keep = P[g.Hz - 1:g.Hz + nz + 1, g.Hy - 1:g.Hy + g.Ny + 1, g.Hx - 1:g.Hx + g.Nx + 1].clone()
    P.fill_(float("nan"))
    P[g.Hz - 1:g.Hz + nz + 1, g.Hy - 1:g.Hy + g.Ny + 1, g.Hx - 1:g.Hx + g.Nx + 1] = keep
    assert torch.isnan(P).any()


def _stale_K_halos(fields):
    import torch
    for f in fields.values():
        g = f.grid
        keep = f.interior.clone()
        f.parent.fill_(float("nan"))
        f.parent[g.Hz - 1:g.Hz + g.Nz + 1, g.Hy - 1:g.Hy + g.Ny + 1, g.Hx - 1:g.Hx + g.Nx + 1] = -777.0      # stale first halo cells
        f.interior.copy_(keep)
        assert torch.isnan(f.parent).any()


def _prepared(oracle, oc, bz, shape, seed=11, **kw):
    """a pair on the same pushed state, update_state!(compute_tendencies = true) done on both sides"""
    vapour = kw.pop("vapour", 0.01)
    om, hm, fields = _pair(oracle, oc, bz, shape, **kw)
    om.set(**_initial(om, seed, vapour=vapour))
    om.seed_time_averaged_velocities()
    om.update_state(compute_tendencies=True)
    _push(om, hm)
    _stale_K_halos(fields)
    if "νₑ" in hm.closure_fields:
        hm.closure_fields["νₑ"].parent.fill_(float("nan"))
    hm.profile_enable(True)
    bz.compressible.update_state_(hm, compute_tendencies=True)
    return om, hm, fields


def _assert_stability_classes(om):
    Sig2, arg = ccr.stability_argument(om)
    N2 = ccr.buoyancy_frequency(om)
    sheared = Sig2 > 0
    assert (Sig2 == 0).any(), "no cell at rest"
    assert (sheared & (N2 <= 0)).any() and (sheared & (arg > 0) & (arg < 1)).any() and (sheared & (arg >= 1)).any(), "a class of the stability factor is missing"
    assert not (sheared & (np.abs(1.0 - arg) < 1e-3)).any(), "a sheared cell sits on the switch of the stability factor: pick another seed"
    return Sig2


# ---- nu_e ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stretched", [False, True])
@pytest.mark.parametrize("shape,halo", SHAPES_HALO)
def test_eddy_viscosity_matches_the_restatement(oracle, oc, bz, shape, stretched, halo):
    """nu_e after update_state! within 1e-11 of its maximum (tests/test_closure.py:145); the cells at rest are exact zeros; recomputed by
    compute_closure_fields_ alone with every field NaN beyond its first halo cell: the same bits"""
    om, hm, _ = _prepared(oracle, oc, bz, shape, seed=SEEDS[shape, stretched], stretched=stretched, halo=halo, closure="smagorinsky")
    Sig2 = _assert_stability_classes(om)
    nu = hm.closure_fields["νₑ"].interior_cpu()
    err = np.abs(nu - om.nu_e).max() / om.nu_e.max()
    print(f"NUE {shape} stretched={stretched} halo={halo}: {err:.2e}")
    assert err <= 1e-11
    assert np.all(nu[Sig2 == 0] == 0.0)
    d = hm.dynamics
    for f in (d.dry_density, d.total_density, d.pressure, hm.velocities["u"], hm.velocities["v"], hm.potential_temperature,
              hm.specific_moisture, hm.temperature):
        _poison_beyond_first_halo(f)
    _poison_beyond_first_halo(hm.velocities["w"], zface=True)
    hm.closure_fields["νₑ"].parent.fill_(float("nan"))
    bz.compressible.compute_closure_fields_(hm)
    hm.synchronize()
    assert np.array_equal(hm.closure_fields["νₑ"].interior_cpu(), nu)
    # halos of nu_e: periodic in x / y, zero gradient in z
    g = om.grid
    P = hm.closure_fields["νₑ"].cpu()
    first = P[g.Hz - 1:g.Hz + g.Nz + 1, g.Hy - 1:g.Hy + g.Ny + 1, g.Hx - 1:g.Hx + g.Nx + 1]
    assert np.array_equal(first, ccr._pad_interior(g, nu))
    names = set(hm.profile())
    assert ("smagorinsky_march" in names) == _marches(shape) and ("smagorinsky_viscosity" in names) == (not _marches(shape)), names


@pytest.mark.parametrize("micro,vapour", [(None, 0.0), ("SaturationAdjustment", 0.02), ("Kessler", 0.01)])
def test_eddy_viscosity_takes_the_vapour_fraction(oracle, oc, bz, micro, vapour):
    """q^v = specific_humidity(model): zero in a dry model, the diagnosed vapour fraction with saturation adjustment (some cells cloudy), the
    moisture slot with Kessler"""
    om, hm, _ = _prepared(oracle, oc, bz, (40, 6, 5), stretched=True, closure="smagorinsky", micro=micro, vapour=vapour)
    if micro == "SaturationAdjustment":
        ql = om.grid.interior(om.ql)
        assert (ql > 0).any() and (ql == 0).any()
    nu = hm.closure_fields["νₑ"].interior_cpu()
    assert om.nu_e.max() > 0
    assert np.abs(nu - om.nu_e).max() <= 1e-11 * om.nu_e.max()


# ---- tendencies ---------------------------------------------------------------------------------------------------------------------
def _tendencies(bz, hm):
    bz.compressible.compute_slow_tendencies_(hm)
    hm.synchronize()
    out = {n: hm.G[k].interior_cpu().copy() for n, k in PROG.items()}
    if getattr(hm, "_kessler", False):
        out.update({n: hm.G[k].interior_cpu().copy() for n, k in KES.items()})
    return out


def _check_tendencies(oracle, oc, bz, shape, expect_part, **kw):
    """device tendencies with the closure minus the same calls with closure = None: within 1e-10 of the part's max-abs
    (tests/test_closure.py:160); the full tendencies within 1e-12 of the restatement (tests/test_gpu_compressible.py:187)"""
    om, hm, _ = _prepared(oracle, oc, bz, shape, **kw)
    om.compute_slow_tendencies()
    got = _tendencies(bz, hm)
    names = set(hm.profile())
    kw0 = dict(kw, closure=None)
    kw0.pop("K", None)
    om0, hm0, _ = _prepared(oracle, oc, bz, shape, **kw0)
    om0.compute_slow_tendencies()
    base = _tendencies(bz, hm0)
    g = om.grid
    for n in got:
        zf = n == "rw"
        want, want0 = g.interior(om.G[n], zf), g.interior(om0.G[n], zf)
        a, b = got[n], base[n]
        if zf:
            want, want0, a, b = want[1:-1], want0[1:-1], a[1:-1], b[1:-1]
        assert np.abs(a - want).max() <= 1e-12 * np.abs(want).max(), (n, np.abs(a - want).max() / np.abs(want).max())
        part = want - want0
        if n in expect_part:
            assert np.abs(part).max() > 0, n
            err = np.abs((a - b) - part).max() / np.abs(part).max()
            print(f"PART {shape} {kw.get('closure')} {n}: {err:.2e}")
            assert err <= 1e-10, (n, err)
        else:
            assert np.array_equal(part, np.zeros_like(part)), n
            assert np.array_equal(a, b), n          # the bits of the run without a closure
    return names


ALL = ("ru", "rv", "rw", "rtheta", "rq")


@pytest.mark.parametrize("stretched", [False, True])
@pytest.mark.parametrize("shape,halo", SHAPES_HALO)
def test_smagorinsky_tendencies(oracle, oc, bz, shape, stretched, halo):
    names = _check_tendencies(oracle, oc, bz, shape, ALL, seed=SEEDS[shape, stretched], stretched=stretched, halo=halo, closure="smagorinsky")
    mine = {"closure_march", "smagorinsky_march"} if _marches(shape) else {"closure_tendencies", "smagorinsky_viscosity"}
    other = {"closure_march", "smagorinsky_march", "closure_tendencies", "smagorinsky_viscosity"} - mine
    assert mine | {"water_closure_tendencies"} <= names and not (other & names), names


@pytest.mark.parametrize("stretched", [False, True])
@pytest.mark.parametrize("shape", [(64, 8, 33), (128, 16, 12)])
def test_tiled_kernels_match_the_cell_per_thread_kernels(oracle, oc, bz, shape, stretched, monkeypatch):
    """nu_e and every tendency of the LDS-tiled march against the cell-per-thread kernels (BZ_NO_CLOSURE_MARCH=1) on the same pushed state: 1e-13
    of the quantity's maximum (same expressions in the same order; bitwise equality is not asserted)"""
    out = []
    for no_march in (False, True):
        if no_march:
            monkeypatch.setenv("BZ_NO_CLOSURE_MARCH", "1")
        else:
            monkeypatch.delenv("BZ_NO_CLOSURE_MARCH", raising=False)
        om, hm, _ = _prepared(oracle, oc, bz, shape, seed=SEEDS[shape, stretched], stretched=stretched, closure="smagorinsky")
        got = _tendencies(bz, hm)
        got["nu"] = hm.closure_fields["νₑ"].interior_cpu().copy()
        names = set(hm.profile())
        assert ("closure_march" in names) == (not no_march) and ("closure_tendencies" in names) == no_march, names
        assert ("smagorinsky_march" in names) == (not no_march) and ("smagorinsky_viscosity" in names) == no_march, names
        out.append(got)
    for n in out[0]:
        scale = np.abs(out[1][n]).max()
        assert scale > 0, n
        err = np.abs(out[0][n] - out[1][n]).max() / scale
        print(f"TILED {shape} stretched={stretched} {n}: {err:.2e}")
        assert err <= 1e-13, (n, err)


def _Kfield(shape, seed, top):
    Nx, Ny, Nz = shape
    return top * np.random.default_rng(seed).random((Nz, Ny, Nx))


@pytest.mark.parametrize("stretched", [False, True])
@pytest.mark.parametrize("shape,halo", SHAPES_HALO)
@pytest.mark.parametrize("closure", ["isotropic", "vertical"])
@pytest.mark.parametrize("kind", ["numbers", "fields"])
def test_scalar_diffusivity_tendencies_on_every_shape(oracle, oc, bz, shape, halo, stretched, closure, kind):
    K = (15.0, 25.0) if kind == "numbers" else (_Kfield(shape, 1, 20.0), _Kfield(shape, 2, 30.0))
    names = _check_tendencies(oracle, oc, bz, shape, ALL, stretched=stretched, halo=halo, closure=closure, K=K)
    assert {"diffusivity_tendencies", "water_closure_tendencies"} <= names, names


@pytest.mark.parametrize("shape", [(40, 6, 5), (64, 8, 33)])
@pytest.mark.parametrize("closure", ["isotropic", "vertical"])
@pytest.mark.parametrize("kind", ["nu only", "kappa only", "zero"])
def test_scalar_diffusivity_tendencies(oracle, oc, bz, shape, closure, kind):
    K = {"numbers": (15.0, 25.0), "fields": (_Kfield(shape, 1, 20.0), _Kfield(shape, 2, 30.0)), "nu only": (15.0, 0.0),
         "kappa only": (0.0, 25.0), "zero": (0.0, 0.0)}[kind]
    expect = {"numbers": ALL, "fields": ALL, "nu only": ALL[:3], "kappa only": ALL[3:], "zero": ()}[kind]
    names = _check_tendencies(oracle, oc, bz, shape, expect, stretched=True, closure=closure, K=K)
    assert ("diffusivity_tendencies" in names) == (kind != "zero"), names
    assert ("water_closure_tendencies" in names) == (kind not in ("zero", "nu only")), names


@pytest.mark.parametrize("closure", ["smagorinsky", "vertical"])
def test_kessler_species_diffuse_in_the_same_launch(oracle, oc, bz, closure):
    K = (_Kfield((40, 6, 5), 3, 20.0), _Kfield((40, 6, 5), 4, 30.0)) if closure == "vertical" else None
    _check_tendencies(oracle, oc, bz, (40, 6, 5), ALL + ("rqcl", "rqr"), stretched=True, closure=closure, micro="Kessler", K=K)


# ---- steps --------------------------------------------------------------------------------------------------------------------------
def _step_fields(hm):
    out = {n: hm.prognostic_fields()[k].interior_cpu().copy() for n, k in PROG.items()}
    if getattr(hm, "_kessler", False):
        out.update({n: hm.microphysical_fields[k].interior_cpu().copy() for n, k in KES.items()})
    return out


STEP_CASES = {
    "smagorinsky dry": dict(closure="smagorinsky", vapour=0.0),
    "smagorinsky kessler": dict(closure="smagorinsky", micro="Kessler"),
    "vertical field K rewritten": dict(closure="vertical", K="fields"),
    "isotropic numbers fplane sponge": dict(closure="isotropic", K=(15.0, 25.0), coriolis=1e-4, sponge=True),
    "smagorinsky weno9 halo5": dict(closure="smagorinsky", order=9, halo=5),
}


@pytest.mark.parametrize("case", list(STEP_CASES), ids=list(STEP_CASES))
def test_three_steps_match_the_restatement(oracle, oc, bz, case):
    """Three WS-RK3 steps through the whole-step seam: 5e-9 of max-abs per field (tests/test_gpu_compressible.py:306), 1e-8 with Kessler
    (:714); the whole step equals the per-operator sequence to 1e-14 (:645-658).  The field-K case rewrites nu and kappa between the steps
    and leaves their halos stale, as validation/DCMIP2016_TC/dcmip2016_tc.jl:277-292 does."""
    kw = dict(STEP_CASES[case])
    shape, dt = (40, 10 if kw.get("halo") == 5 else 6, 12), 0.5
    vapour = kw.pop("vapour", 0.01)
    rewrite = kw.get("K") == "fields"
    if rewrite:
        kw["K"] = (_Kfield(shape, 20, 20.0), _Kfield(shape, 30, 30.0))
    om, a, fa = _pair(oracle, oc, bz, shape, stretched=True, **kw)
    _, b, fb = _pair(oracle, oc, bz, shape, stretched=True, **kw)
    ic = _initial(om, 5, vapour=vapour, rough=0.2)
    om.set(**ic)
    dev = {"ρ": ic["rho"], "θ": ic["theta"], "u": ic["u"], "v": ic["v"], "w": ic["w"], "qᵗ": ic["qv"]}
    dev.update({k: ic[k] for k in ("qcl", "qr") if k in ic})
    for m in (a, b):
        m.set(**dev)
    a.profile_enable(True)
    for s in range(3):
        if rewrite:
            Knew = (_Kfield(shape, 20 + s, 20.0), _Kfield(shape, 30 + s, 30.0))
            om.diffusivity.nu, om.diffusivity.kappa = Knew
            for fields in (fa, fb):
                fields["ν"].set_interior(Knew[0])
                fields["κ"].set_interior(Knew[1])
                _stale_K_halos(fields)
        om.time_step(dt)
        bz.compressible.time_step_(a, dt, whole_step=True)
        bz.compressible.time_step_(b, dt, whole_step=False)
        fa_, fb_ = _step_fields(a), _step_fields(b)
        mom_ = max(np.abs(fb_[n]).max() for n in ("ru", "rv", "rw"))
        seam = {n: np.abs(fa_[n] - fb_[n]).max() / (mom_ if n in ("ru", "rv", "rw") else max(np.abs(fb_[n]).max(), 1e-300)) for n in fa_}
        print(f"SEAM {case} step {s + 1}:", " ".join(f"{n}={e:.1e}" for n, e in seam.items()))
        # (with Kessler the seam and the sequence are not bitwise equal in the model as it stands — 1.0e-14 (rho v) and 1.4e-14 (rho w) after
        # three steps of this case with closure = None, 2.6e-14 / 3.4e-14 after two with SmagorinskyLilly, measured on the MI355X — so later
        # steps, which grow that difference by the model's own dynamics, are judged after the first step as :645-658 judges one step, later
        # ... against 1e-13, the bound tests/test_gpu_compressible.py:639 holds two runs of the same three Kessler steps to)
        bound = 1e-14 if (s == 0 or kw.get("micro") != "Kessler") else 1e-13
        assert all(e <= bound for e in seam.values()), (s + 1, seam)
    a.synchronize()
    b.synchronize()
    g = om.grid
    got = _step_fields(a)
    tol = 1e-8 if kw.get("micro") == "Kessler" else 5e-9
    mom = max(np.abs(g.interior(getattr(om, n), n == "rw")).max() for n in ("ru", "rv", "rw"))
    worst = {}
    for n in got:
        want = g.interior(getattr(om, n), n == "rw")
        scale = mom if n in ("ru", "rv", "rw") else np.abs(want).max()
        if scale == 0.0:
            assert not got[n].any(), n
            continue
        worst[n] = np.abs(got[n] - want).max() / scale
    print(f"STEPS {case}:", " ".join(f"{n}={e:.1e}" for n, e in worst.items()))
    assert all(e <= tol for e in worst.values()), worst
    if kw["closure"] == "smagorinsky":
        assert om.nu_e.max() > 0
        assert np.abs(a.closure_fields["νₑ"].interior_cpu() - om.nu_e).max() <= 1e-6 * om.nu_e.max()
    # the closure acted: the same steps without it end elsewhere
    kw0 = {k: v for k, v in kw.items() if k != "K"}
    kw0["closure"] = None
    om0, _, _ = _pair(oracle, oc, bz, shape, stretched=True, **kw0)
    om0.set(**ic)
    for _ in range(3):
        om0.time_step(dt)
    assert np.abs(g.interior(om0.rtheta) - g.interior(om.rtheta)).max() > tol * np.abs(g.interior(om.rtheta)).max()


def test_recorded_step_replays_the_same_bits(oracle, oc, bz):
    """hipGraph replay: recorded steps with a closure leave the bits of launched ones"""
    out = []
    for graph in (True, False):
        om, hm, _ = _pair(oracle, oc, bz, (40, 6, 12), stretched=True, closure="smagorinsky")
        ic = _initial(om, 6, rough=0.2)
        hm.set(ρ=ic["rho"], θ=ic["theta"], u=ic["u"], v=ic["v"], w=ic["w"], qᵗ=ic["qv"])
        if graph:
            hm.graph_enable(True)
        for _ in range(4):
            hm.time_step(0.5)
        hm.synchronize()
        if graph:
            en, cap, rep = hm.graph_info()
            assert en and cap >= 1 and rep >= 1, (en, cap, rep)
        out.append(dict(_step_fields(hm), nu=hm.closure_fields["νₑ"].interior_cpu().copy()))
    for n in out[0]:
        assert np.array_equal(out[0][n], out[1][n]), n


# ---- Float32 twin ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("closure", ["smagorinsky", "isotropic"])
def test_float32_steps_by_increments(oracle, oc, bz, closure):
    """eltype(grid) = Float32: three steps against the Float64 restatement, judged per field by helpers.increment_error.  The bound is the
    larger of F32_INCREMENT_TOL["compressible"] and 4 x the increment error of the same case with closure = None in the same test: the
    no-closure path is the yardstick.  Measured on the MI355X (F32INC lines):
        none         rho_d 1.34e-4  rtheta 1.06e-4  rq 2.02e-4  ru 1.35e-4  rw 1.04e-4     (both parametrisations)
        smagorinsky  rho_d 1.36e-4  rtheta 1.16e-4  rq 2.13e-4  ru 1.45e-4  rw 1.20e-4
        isotropic    rho_d 1.25e-4  rtheta 9.70e-5  rq 1.24e-4  ru 1.17e-4  rw 9.83e-5
    The closure part of the tendencies is judged by test_float32_closure_part_within_four_times_the_float32_restatement."""
    import torch
    from helpers import F32_INCREMENT_TOL, increment_error
    shape, dt = (40, 6, 12), 0.5
    errs = {}
    for which in (None, closure):
        kw = dict(closure=which, K=(15.0, 25.0)) if which == "isotropic" else dict(closure=which)
        om, hm, _ = _pair(oracle, oc, bz, shape, stretched=True, float_type=np.float32, **kw)
        assert hm.momentum["ρu"].parent.dtype == torch.float32
        ic = _initial(om, 5, rough=0.2)
        om.set(**ic)
        hm.set(ρ=ic["rho"], θ=ic["theta"], u=ic["u"], v=ic["v"], w=ic["w"], qᵗ=ic["qv"])
        g = om.grid
        names = ("rho_d", "rtheta", "rq", "ru", "rw")
        start = {n: g.interior(getattr(om, n), n == "rw").copy() for n in names}
        for _ in range(3):
            om.time_step(dt)
            hm.time_step(dt)
        hm.synchronize()
        got = _step_fields(hm)
        errs[which] = {n: increment_error(got[n], g.interior(getattr(om, n), n == "rw"), start[n]) for n in names}
        print(f"F32INC {which}:", " ".join(f"{n}={e:.2e}" for n, e in errs[which].items()))
    tol = F32_INCREMENT_TOL["compressible"]
    bad = {n: (e, max(tol[n], 4 * errs[None][n])) for n, e in errs[closure].items() if not e <= max(tol[n], 4 * errs[None][n])}
    assert not bad, bad


@pytest.mark.parametrize("closure", ["smagorinsky", "isotropic numbers", "isotropic fields", "vertical fields"])
def test_float32_closure_part_within_four_times_the_float32_restatement(oracle, oc, bz, closure):
    """eltype(grid) = Float32 at (64, 8, 33): the closure part of every slow and water tendency (device with the closure minus device
    without, same pushed state) against the Float64 restatement evaluated on the DEVICE's own diagnosed fields (u, v, w, theta, q, rho_d,
    rho, and nu_e / K as the device holds them, exact in Float64): the error is at most 4 x the error of the same formulas evaluated in
    numpy float32 on those inputs (compressible_closure_reference.in_dtype), subtracted in float32 from the device's closure-free tendency
    as the kernels subtract it — the rule of tests/test_diagnostics.py.  Both errors are computed here, every run."""
    import torch
    from test_gpu_compressible import O2H
    shape = (64, 8, 33)
    kind, _, what = closure.partition(" ")
    K = None if kind == "smagorinsky" else (15.0, 25.0) if what == "numbers" else (_Kfield(shape, 1, 20.0), _Kfield(shape, 2, 30.0))
    kw = dict(closure=kind, K=K) if K is not None else dict(closure=kind)
    om, hm, fields = _prepared(oracle, oc, bz, shape, seed=SEEDS[shape, True], stretched=True, float_type=np.float32, **kw)
    _, hm0, _ = _prepared(oracle, oc, bz, shape, seed=SEEDS[shape, True], stretched=True, float_type=np.float32)
    assert hm.momentum["ρu"].parent.dtype == torch.float32
    got, base = _tendencies(bz, hm), _tendencies(bz, hm0)
    for n in ("rho_d", "rho", "u", "v", "w", "theta", "q"):      # the device's inputs, exact in Float64
        getattr(om, n)[...] = O2H[n](hm).cpu().astype(np.float64)
    if kind == "smagorinsky":
        om.nu_e = hm.closure_fields["νₑ"].interior_cpu().astype(np.float64)
    elif fields:
        om.diffusivity.nu, om.diffusivity.kappa = (fields[k].interior_cpu().astype(np.float64) for k in ("ν", "κ"))
    truth = dict(om.slow_closure_terms(), **om.water_closure_terms())
    v32 = ccr.in_dtype(om, np.float32)
    yard = dict(v32.slow_closure_terms(), **v32.water_closure_terms())
    worst = {}
    for n in ALL:
        a, b = got[n], base[n]
        if n == "rw":
            a, b = a[1:-1], b[1:-1]
        assert a.dtype == np.float32 and yard[n].dtype == np.float32, n
        part_dev = a.astype(np.float64) - b.astype(np.float64)
        part_ref = ((b - yard[n]) - b).astype(np.float64)          # float32 arithmetic, as the kernel's read-modify-write
        err_dev, err_ref = np.abs(part_dev + truth[n]).max(), np.abs(part_ref + truth[n]).max()
        worst[n] = (err_dev, err_ref)
        assert np.abs(truth[n]).max() > 0 and err_ref > 0, n
    print(f"F32PART {closure}:", " ".join(f"{n}={d:.2e}/{r:.2e}" for n, (d, r) in worst.items()))
    bad = {n: v for n, v in worst.items() if not v[0] <= 4 * v[1]}
    assert not bad, bad


# ---- refusals of the C ABI ------------------------------------------------------------------------------------------------------------
def test_abi_refuses_what_is_not_built(bz):
    from breeze_jl_amd import _lib
    UNSUPPORTED = 2
    dyn = lambda: bz.CompressibleDynamics(bz.SplitExplicitTimeDiscretization(substeps=6), reference_potential_temperature=300.0)
    ext = dict(x=(0, 1600.0), y=(0, 1600.0), z=(0, 800.0))
    m = bz.CompressibleAtmosphereModel(bz.RectilinearGrid((16, 16, 8), **ext), dyn(), advection=bz.WENO(order=5))
    sd = _lib.bz_scalar_diffusivity(0, 1, 1.0, 1.0)      # vertically implicit
    assert m._lib.bz_set_scalar_diffusivity(m._ctx, C.byref(sd), None, None) == UNSUPPORTED
    assert b"VerticallyImplicitTimeDiscretization" in m._lib.bz_last_error(m._ctx)
    # the two closures stay mutually exclusive
    sd = _lib.bz_scalar_diffusivity(0, 0, 1.0, 1.0)
    assert m._lib.bz_set_scalar_diffusivity(m._ctx, C.byref(sd), None, None) == 0
    nu_e = bz.Field(m.grid, (bz.Center, bz.Center, bz.Center), "cuda:0")
    sl = _lib.bz_smagorinsky_lilly(0.16, 1.0, 1.0)
    assert m._lib.bz_set_closure(m._ctx, C.byref(sl), C.c_void_p(nu_e.ptr())) == UNSUPPORTED
    assert b"ScalarDiffusivity" in m._lib.bz_last_error(m._ctx)
    m.time_step(0.5)
    walled = bz.CompressibleAtmosphereModel(bz.RectilinearGrid((16, 16, 8), topology=(bz.Periodic, bz.Bounded, bz.Bounded), **ext), dyn(),
                                            advection=bz.WENO(order=5))
    nu_w = bz.Field(walled.grid, (bz.Center, bz.Center, bz.Center), "cuda:0")
    assert walled._lib.bz_set_closure(walled._ctx, C.byref(sl), C.c_void_p(nu_w.ptr())) == UNSUPPORTED
    assert b"Bounded" in walled._lib.bz_last_error(walled._ctx)
    assert walled._lib.bz_set_scalar_diffusivity(walled._ctx, C.byref(sd), None, None) == UNSUPPORTED
    assert b"Bounded" in walled._lib.bz_last_error(walled._ctx)
    # bz_compressible_kessler_update ends in update_state!, which a Bounded x does not run: refused by its own name
    wx = bz.CompressibleAtmosphereModel(bz.RectilinearGrid((16, 16, 8), topology=(bz.Bounded, bz.Periodic, bz.Bounded), **ext), dyn(),
                                        advection=bz.WENO(order=5))
    assert wx._lib.bz_compressible_kessler_update(wx._ctx, C.byref(wx._state), C.byref(wx._G), C.byref(wx._sub), 1.0) == UNSUPPORTED
    assert b"bz_compressible_kessler_update" in wx._lib.bz_last_error(wx._ctx)
