"""GPU parity: every entry point of the C ABI against the CPU oracle on the same seeded inputs.

Tolerances (Float64): the HIP kernels execute the oracle's operation order but hipcc contracts
mul+add into FMA and uses its own pow/sin, so single kernels agree to ~1e-13 of the field scale;
the Poisson solve differs by FFT algorithm (rocFFT real-to-complex vs pocketfft complex): 1e-11;
after full time steps: 1e-9 (last row)."""
import os

import numpy as np
import pytest

from helpers import PROG, bubble_theta, make_pair, push_state, randomize, relerr

pytestmark = pytest.mark.gpu

SIZES = [(32, 20, 16), (72, 16, 40), (16, 8, 8)]


def _interior(om, name):
    return om.grid.interior(getattr(om, name), zface=(name in ("rw", "w")))


@pytest.mark.parametrize("size", SIZES)
def test_halo_fill_matches_oracle(oracle, bz, size):
    import torch
    om, hm = make_pair(oracle, bz, size)
    rng = np.random.default_rng(1)
    for kind, name, ofill in ((0, "theta", om._halo_center), (1, "rw", om._halo_w), (2, "u", om._halo_velocity)):
        arr = getattr(om, name)
        arr[...] = rng.standard_normal(arr.shape)
        f = {"theta": hm.potential_temperature, "rw": hm.momentum["ρw"], "u": hm.velocities["u"]}[name]
        f.parent.copy_(torch.from_numpy(arr))
        ofill(arr)
        bz.fill_halo_regions_(hm, f, kind)
        hm.synchronize()
        assert np.array_equal(f.cpu(), arr)      # pure copies: bit-exact


@pytest.mark.parametrize("size", SIZES)
def test_update_state_matches_oracle(oracle, bz, size):
    om, hm = make_pair(oracle, bz, size)
    randomize(om, seed=7)
    push_state(om, hm, names=("ru", "rv", "rw", "rtheta", "rq"))
    bz.update_state_(hm, compute_tendencies=False)
    hm.synchronize()
    g = om.grid
    for n, f in (("u", hm.velocities["u"]), ("v", hm.velocities["v"]), ("w", hm.velocities["w"]),
                 ("theta", hm.potential_temperature), ("q", hm.specific_moisture), ("T", hm.temperature)):
        got, want = f.cpu(), getattr(om, n)
        # compare the whole parent array: halos must match too
        assert relerr(got, want) < 1e-14, n


@pytest.mark.parametrize("size", SIZES)
def test_tendencies_match_oracle(oracle, bz, size):
    om, hm = make_pair(oracle, bz, size)
    randomize(om, seed=11)
    om.compute_tendencies()
    push_state(om, hm, names=("ru", "rv", "rw", "rtheta", "rq", "u", "v", "w", "theta", "q", "T"))
    for k in hm.G.values():
        k.parent.zero_()
    bz.compute_tendencies_(hm)
    hm.synchronize()
    g = om.grid
    for n, k in PROG.items():
        zf = n == "rw"
        want = g.interior(om.G[n], zface=zf)
        got = hm.G[k].interior_cpu()
        if zf:      # wall faces are never updated
            want, got = want[1:-1], got[1:-1]
        assert relerr(got, want) < 1e-12, n


def test_tendencies_stretched_grid(oracle, bz):
    zf = 1e4 * (np.linspace(0, 1, 25) ** 1.3)
    om, hm = make_pair(oracle, bz, (32, 12, 24), z_faces=zf)
    randomize(om, seed=5)
    om.compute_tendencies()
    push_state(om, hm, names=("ru", "rv", "rw", "rtheta", "rq", "u", "v", "w", "theta", "q", "T"))
    bz.compute_tendencies_(hm)
    hm.synchronize()
    for n, k in PROG.items():
        zface = n == "rw"
        want, got = om.grid.interior(om.G[n], zface=zface), hm.G[k].interior_cpu()
        if zface:
            want, got = want[1:-1], got[1:-1]
        assert relerr(got, want) < 1e-12, n


@pytest.mark.parametrize("size", SIZES)
def test_pressure_correction_matches_oracle(oracle, bz, size):
    om, hm = make_pair(oracle, bz, size)
    randomize(om, seed=3)
    push_state(om, hm, names=("ru", "rv", "rw"))
    dt = 0.7
    om.compute_pressure_correction(dt)
    bz.compute_pressure_correction_(hm, dt)
    hm.synchronize()
    assert relerr(hm.dynamics.pressure_anomaly.cpu(), om.phi) < 1e-11
    om.make_pressure_correction(dt)
    bz.make_pressure_correction_(hm, dt)
    hm.synchronize()
    for n in ("ru", "rv", "rw"):
        f = {"ru": hm.momentum["ρu"], "rv": hm.momentum["ρv"], "rw": hm.momentum["ρw"]}[n]
        assert relerr(f.interior_cpu(), _interior(om, n)) < 1e-11, n
    # projection => discretely divergence-free (test/anelastic_pressure_solver_nonhydrostatic.jl:45-46)
    div = hm.max_abs_divergence()
    scale = np.max(np.abs(_interior(om, "ru"))) / om.grid.dx
    assert div < 1e-12 * scale


def test_rk3_substep_bit_exact_structure(oracle, bz):
    om, hm = make_pair(oracle, bz, (32, 20, 16))
    randomize(om, seed=13)
    om.compute_tendencies()
    for n in om.PROGNOSTIC:
        om.U0[n][...] = getattr(om, n) * 0.9
    push_state(om, hm)
    om.rk3_substep(1.3, 0.25)
    bz.ssp_rk3_substep_(hm, 1.3, 0.25)
    hm.synchronize()
    for n, k in PROG.items():
        assert relerr(hm.prognostic_fields()[k].cpu(), getattr(om, n)) < 1e-15, n


@pytest.mark.parametrize("size,dt", [((32, 20, 16), 2.0), ((64, 8, 32), 1.0)])
def test_time_steps_match_oracle(oracle, bz, size, dt):
    om, hm = make_pair(oracle, bz, size)
    th = bubble_theta(300.0, om.constants.g)
    om.set(theta=th, u=3.0, v=-2.0)
    hm.set(θ=th, u=3.0, v=-2.0)
    for step in range(3):
        om.time_step(dt)
        hm.time_step(dt)
    hm.synchronize()
    for n, k in PROG.items():
        got = hm.prognostic_fields()[k].interior_cpu()
        want = _interior(om, n)
        scale = max(np.max(np.abs(want)), 1e-3)
        assert np.max(np.abs(got - want)) / scale < 1e-9, n
    assert relerr(hm.temperature.interior_cpu(), om.grid.interior(om.T)) < 1e-9
    assert np.isfinite(hm.velocities["w"].cpu()).all()


@pytest.mark.parametrize("size", [(16, 8, 6), (32, 16, 5), (64, 8, 12), (128, 24, 9), (256, 8, 4), (512, 8, 3), (1024, 8, 3),
                                  (96, 8, 6), (192, 16, 5), (384, 8, 4), (768, 8, 3)])      # 3 * 2^m: the leading radix-3 stage
def test_fused_x_transform_pipeline_matches_oracle(oracle, bz, size):
    """Hand-written x transforms + transposed half spectrum (csrc/bz_xfft_kernels.h; taken when Nx is a power of two in [16, 1024]
    and Ny % 8 == 0): every radix mix (Nx/2 = 4^m and 2 * 4^m).  Per-operator solve (rows of the rhs buffer in, phi out) and whole
    steps (source term evaluated inside the forward pass, stage 1-2 projection inside the inverse pass) against the oracle, whose
    transforms are pocketfft's complex ones — same tolerances as the library-transform path."""
    om, hm = make_pair(oracle, bz, size)
    randomize(om, seed=5)
    push_state(om, hm, names=("ru", "rv", "rw"))
    dt = 0.7
    om.compute_pressure_correction(dt)
    bz.compute_pressure_correction_(hm, dt)
    hm.synchronize()
    assert relerr(hm.dynamics.pressure_anomaly.cpu(), om.phi) < 1e-11
    om.make_pressure_correction(dt)
    bz.make_pressure_correction_(hm, dt)
    hm.synchronize()
    scale = np.max(np.abs(_interior(om, "ru"))) / om.grid.dx
    assert hm.max_abs_divergence() < 1e-12 * scale
    # whole steps
    om, hm = make_pair(oracle, bz, size)
    th = bubble_theta(300.0, om.constants.g)
    om.set(theta=th, u=3.0, v=-2.0)
    hm.set(θ=th, u=3.0, v=-2.0)
    for step in range(2):
        om.time_step(1.0)
        hm.time_step(1.0)
    hm.synchronize()
    mom = max(np.max(np.abs(_interior(om, n))) for n in ("ru", "rv", "rw"))      # the components of a vector share its scale
    for n, k in PROG.items():
        got = hm.prognostic_fields()[k].interior_cpu()
        want = _interior(om, n)
        scale = mom if n in ("ru", "rv", "rw") else max(np.max(np.abs(want)), 1e-3)
        assert np.max(np.abs(got - want)) / scale < 1e-9, n
    for n, f in (("u", hm.velocities["u"]), ("theta", hm.potential_temperature), ("T", hm.temperature), ("rv", hm.momentum["ρv"])):
        assert relerr(f.cpu(), getattr(om, n)) < 1e-9, n        # whole parent arrays: the fused projection stores the halo images


@pytest.mark.parametrize("size,chunk_kb,pad", [((64, 16, 32), 64, 1), ((128, 24, 16), 48, 0), ((32, 64, 128), 200, 3), ((256, 8, 64), 300, 1)])
def test_kx_major_spectrum_and_chunked_solve_match_oracle(oracle, bz, size, chunk_kb, pad, monkeypatch):
    """Round 6: on a single GPU the half spectrum is kx-major (a range of wavenumbers contiguous, `pad` phantom lines per wavenumber) and the y
    transform / vertical solves / inverse y transform run chunk by chunk of wavenumbers (csrc/bz_poisson.hip: bzi_xf_middle; at 512^3 a chunk
    is ~220 MB and stays in the Infinity Cache between its three passes).  BZ_POISSON_KX_CHUNK_KB brings small grids onto the same path: five
    to seven chunks with a shorter last one, 16 / 64 vertical segments, both Stockham radix mixes.  Per-operator solve against the oracle
    (1e-11), projected momentum discretely divergence-free, two whole steps (1e-9), and bit for bit against the level-major whole-spectrum
    passes (BZ_POISSON_KXMAJOR=0): the same kernels on the same numbers, only the addresses differ."""
    def solve(kxmajor):
        monkeypatch.setenv("BZ_POISSON_KXMAJOR", "1" if kxmajor else "0")
        monkeypatch.setenv("BZ_POISSON_KX_CHUNK_KB", str(chunk_kb))
        monkeypatch.setenv("BZ_POISSON_KX_PAD", str(pad))
        om, hm = make_pair(oracle, bz, size)
        randomize(om, seed=11)
        push_state(om, hm, names=("ru", "rv", "rw"))
        dt = 0.7
        om.compute_pressure_correction(dt)
        bz.compute_pressure_correction_(hm, dt)
        hm.synchronize()
        phi = hm.dynamics.pressure_anomaly.cpu().copy()
        assert relerr(phi, om.phi) < 1e-11
        om.make_pressure_correction(dt)
        bz.make_pressure_correction_(hm, dt)
        hm.synchronize()
        scale = np.max(np.abs(_interior(om, "ru"))) / om.grid.dx
        assert hm.max_abs_divergence() < 1e-12 * scale
        om, hm = make_pair(oracle, bz, size)
        th = bubble_theta(300.0, om.constants.g)
        om.set(theta=th, u=3.0, v=-2.0)
        hm.set(θ=th, u=3.0, v=-2.0)
        for step in range(2):
            om.time_step(1.0)
            hm.time_step(1.0)
        hm.synchronize()
        mom = max(np.max(np.abs(_interior(om, n))) for n in ("ru", "rv", "rw"))
        out = {}
        for n, k in PROG.items():
            got = hm.prognostic_fields()[k].interior_cpu()
            want = _interior(om, n)
            scale = mom if n in ("ru", "rv", "rw") else max(np.max(np.abs(want)), 1e-3)
            assert np.max(np.abs(got - want)) / scale < 1e-9, n
            out[n] = got.copy()
        return phi, out

    phi_a, a = solve(True)
    phi_b, b = solve(False)
    assert np.array_equal(phi_a, phi_b)
    for n in a:
        assert np.array_equal(a[n], b[n]), n


def test_whole_step_equals_operator_sequence(bz):
    """bz_time_step_anelastic == the reference's call sequence through the per-operator entry points."""
    models = []
    for whole in (True, False):
        grid = bz.RectilinearGrid((32, 16, 16), x=(-10e3, 10e3), y=(-10e3, 10e3), z=(0, 10e3))
        m = bz.AtmosphereModel(grid, dynamics=bz.AnelasticDynamics(bz.ReferenceState(grid, potential_temperature=300)),
                               advection=bz.WENO())
        m.set(θ=bubble_theta(300.0, 9.81), u=1.0)
        for _ in range(2):
            bz.time_step_(m, 2.0, whole_step=whole)
        m.synchronize()
        models.append(m)
    a, b = models
    # same arithmetic, but the fused kernels are separate compilations (FMA contraction may differ)
    for k in a.prognostic_fields():
        assert relerr(a.prognostic_fields()[k].cpu(), b.prognostic_fields()[k].cpu()) < 1e-13, k
    for fa, fb in ((a.temperature, b.temperature), (a.velocities["u"], b.velocities["u"]),
                   (a.velocities["w"], b.velocities["w"]), (a.dynamics.pressure_anomaly, b.dynamics.pressure_anomaly),
                   (a.potential_temperature, b.potential_temperature)):
        assert relerr(fa.cpu(), fb.cpu()) < 1e-12      # whole parent arrays: halos included


def test_momentum_conservation_on_device(bz):
    """test/dynamics.jl:45-116 restated on the HIP path: 16^3 WENO bubble, 10 steps of 1e-3 s."""
    grid = bz.RectilinearGrid((16, 16, 16), x=(-10e3, 10e3), y=(-10e3, 10e3), z=(-3e3, 7e3), halo=(5, 5, 5))
    m = bz.AtmosphereModel(grid, advection=bz.WENO())
    th0, g = m.dynamics.reference_state.potential_temperature, 9.81

    def thi(x, y, z):
        r = np.sqrt(x ** 2 + y ** 2 + z ** 2)
        return th0 * np.exp(1e-6 * z / g) + 10 * np.maximum(0, 1 - r / 2e3)

    m.set(θ=thi, u=5.0, v=3.0)
    Px0 = m.momentum["ρu"].interior.sum().item()
    Py0 = m.momentum["ρv"].interior.sum().item()
    for _ in range(10):
        m.time_step(1e-3)
        Px, Py = m.momentum["ρu"].interior.sum().item(), m.momentum["ρv"].interior.sum().item()
        assert abs(Px - Px0) <= 1e-12 * abs(Px0)
        assert abs(Py - Py0) <= 1e-12 * abs(Py0)


def test_full_size_properties_512(bz):
    """BASELINE.json configs[1] at full size (512^3): size-independent properties of the step instead of an oracle
    comparison — after two steps the momentum is discretely divergence-free, horizontal momentum stays zero by
    symmetry of the flux form, the pressure anomaly has zero mean and everything is finite."""
    import torch
    N = 512
    grid = bz.RectilinearGrid((N, N, N), x=(-10e3, 10e3), y=(-10e3, 10e3), z=(0, 10e3))
    m = bz.AtmosphereModel(grid, dynamics=bz.AnelasticDynamics(bz.ReferenceState(grid, potential_temperature=300)),
                           advection=bz.WENO())
    m.set(θ=bubble_theta(300.0, 9.81))
    for _ in range(2):
        m.time_step(1.0)
    m.synchronize()
    ru, rv, rw = (m.momentum[k].interior for k in ("ρu", "ρv", "ρw"))
    scale = float(rw.abs().max())
    assert scale > 1e-3                                   # the bubble has started to rise
    assert float(m.max_abs_divergence()) < 1e-12 * scale / grid.Δz * 100
    assert abs(float(ru.sum())) < 1e-9 * scale * N ** 3 and abs(float(rv.sum())) < 1e-9 * scale * N ** 3
    phi = m.dynamics.pressure_anomaly.interior
    assert abs(float(phi.mean())) < 1e-10 * float(phi.abs().max())
    for f in (m.temperature, m.potential_temperature, m.velocities["w"]):
        assert bool(torch.isfinite(f.interior).all())
    # walls stay closed
    assert float(m.momentum["ρw"].interior[0].abs().max()) == 0.0 and float(m.momentum["ρw"].interior[-1].abs().max()) == 0.0


def test_missing_library_fails_loudly(bz, monkeypatch, tmp_path):
    from breeze_jl_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(RuntimeError):
        _lib.load()


# ---- formulation = :StaticEnergy (src/StaticEnergyFormulations/) ----------------------------------
def _energy_state(om, seed):
    randomize(om, seed=seed)
    g, c = om.grid, om.constants
    rng = np.random.default_rng(seed + 100)
    rho_c = om.ref.density[g.Hz:g.Hz + g.Nz][:, None, None]
    T = 290.0 - 0.006 * g.zc[:, None, None] + 2.0 * rng.standard_normal((g.Nz, g.Ny, g.Nx))
    g.interior(om.rtheta)[...] = rho_c * (c.cpd * T + c.g * g.zc[:, None, None])
    om.update_state(compute_tendencies=False)


def test_static_energy_diagnosis_and_tendencies_match_oracle(oracle, bz):
    """T = (e - g z)/c_pm and G_rho_e = -div_rhoUc(e) - Iz(w Iz(buoyancy)) against the oracle: 1e-14 / 1e-12."""
    om, hm = make_pair(oracle, bz, (32, 20, 16), formulation="StaticEnergy")
    _energy_state(om, 21)
    om.compute_tendencies()
    push_state(om, hm, names=("ru", "rv", "rw", "rtheta", "rq"))
    bz.update_state_(hm, compute_tendencies=True)
    hm.synchronize()
    g = om.grid
    for n, f in (("theta", hm.specific_energy), ("q", hm.specific_moisture), ("T", hm.temperature)):
        assert relerr(f.cpu(), getattr(om, n)) < 1e-14, n
    for n, k in PROG.items():
        zf = n == "rw"
        want, got = g.interior(om.G[n], zface=zf), hm.G[k].interior_cpu()
        if zf:
            want, got = want[1:-1], got[1:-1]
        assert relerr(got, want) < 1e-12, n


def test_static_energy_time_steps_match_oracle(oracle, bz):
    om, hm = make_pair(oracle, bz, (32, 20, 16), formulation="StaticEnergy")
    th = bubble_theta(300.0, om.constants.g)
    om.set(theta=th, u=3.0, v=-2.0)
    hm.set(θ=th, u=3.0, v=-2.0)
    assert relerr(hm.energy_density.interior_cpu(), om.grid.interior(om.rtheta)) < 1e-14
    for _ in range(3):
        om.time_step(2.0)
        hm.time_step(2.0)
    hm.synchronize()
    errs = {}
    mom_scale = max(np.max(np.abs(_interior(om, n))) for n in ("ru", "rv", "rw"))     # momentum components share a scale
    for n, k in PROG.items():
        got, want = hm.prognostic_fields()[k].interior_cpu(), _interior(om, n)
        scale = mom_scale if n in ("ru", "rv", "rw") else max(np.max(np.abs(want)), 1e-3)
        errs[n] = float(np.max(np.abs(got - want)) / scale)
    errs["T"] = float(relerr(hm.temperature.interior_cpu(), om.grid.interior(om.T)))
    assert all(v < 1e-9 for v in errs.values()), {k: f"{v:.1e}" for k, v in errs.items()}


# ---- microphysics = SaturationAdjustment(equilibrium = WarmPhaseEquilibrium()) -------------------
def _moist_pair(oracle, bz, size=(32, 20, 16)):
    extent = ((-4e3, 4e3), (-3e3, 3e3), (0.0, 4e3))
    og = oracle.Grid(size, x=extent[0], y=extent[1], z=extent[2])
    om = oracle.OracleModel(og, potential_temperature=295.0, microphysics="SaturationAdjustment")
    grid = bz.RectilinearGrid(size, x=extent[0], y=extent[1], z=extent[2])
    ref = bz.ReferenceState(grid, potential_temperature=295.0)
    hm = bz.AtmosphereModel(grid, dynamics=bz.AnelasticDynamics(ref), advection=bz.WENO(order=5),
                            microphysics=bz.SaturationAdjustment(equilibrium=bz.WarmPhaseEquilibrium()))
    return om, hm


def _moist_ic():
    qt = lambda x, y, z: 0.018 * np.exp(-z / 2500.0) * (1 + 0.1 * np.sin(2 * np.pi * x / 8e3)) + 0 * y
    th = lambda x, y, z: 295.0 + 0.003 * z + 1.5 * np.maximum(0.0, 1.0 - np.sqrt(x ** 2 + y ** 2 + (z - 1500.0) ** 2) / 1000.0)
    return qt, th


def test_saturation_adjustment_diagnosis_and_buoyancy_match_oracle(oracle, bz):
    """T from the secant iteration, q^v / q^l diagnosis (cloudy and clear cells) and the moist-buoyancy w tendency."""
    om, hm = _moist_pair(oracle, bz)
    qt, th = _moist_ic()
    om.set(qt=qt, theta=th, u=2.0)
    om.compute_tendencies()
    push_state(om, hm, names=("ru", "rv", "rw", "rtheta", "rq"))
    bz.update_state_(hm, compute_tendencies=True)
    hm.synchronize()
    g = om.grid
    ql = g.interior(om.ql)
    assert 0.05 < (ql > 0).mean() < 0.95          # both branches of the adjustment are exercised
    assert relerr(hm.temperature.cpu(), om.T) < 1e-13
    assert np.abs(hm.microphysical_fields["qᵛ"].cpu() - om.qv).max() < 1e-15
    assert np.abs(hm.microphysical_fields["qˡ"].cpu() - om.ql).max() < 1e-15
    # theta carries a kinked bubble here: the expanded smoothness-indicator polynomials of WENO-5 are ill-conditioned and
    # hipcc's FMA contraction alone moves such a flux by ~1e-9 of max|G| (lib/libbreeze_hip_refdiv.so, built with the
    # reference operation order and -ffp-contract=off, passes this very test at 1e-12: BREEZE_HIP_LIB=... pytest -k saturation)
    strict = "refdiv" in bz.LIB_PATH
    for n, k in PROG.items():
        zf = n == "rw"
        want, got = g.interior(om.G[n], zface=zf), hm.G[k].interior_cpu()
        if zf:
            want, got = want[1:-1], got[1:-1]
        assert relerr(got, want) < (1e-12 if strict or n not in ("rtheta", "rq") else 5e-9), n


def test_saturation_adjustment_time_steps_match_oracle(oracle, bz):
    om, hm = _moist_pair(oracle, bz)
    qt, th = _moist_ic()
    om.set(qt=qt, theta=th, u=2.0)
    hm.set(qᵗ=qt, θ=th, u=2.0)
    for _ in range(3):
        om.time_step(2.0)
        hm.time_step(2.0)
    hm.synchronize()
    errs = {}
    mom_scale = max(np.max(np.abs(_interior(om, n))) for n in ("ru", "rv", "rw"))
    for n, k in PROG.items():
        got, want = hm.prognostic_fields()[k].interior_cpu(), _interior(om, n)
        scale = mom_scale if n in ("ru", "rv", "rw") else max(np.max(np.abs(want)), 1e-3)
        errs[n] = float(np.max(np.abs(got - want)) / scale)
    errs["T"] = float(relerr(hm.temperature.interior_cpu(), om.grid.interior(om.T)))
    errs["ql"] = float(np.abs(hm.microphysical_fields["qˡ"].interior_cpu() - om.grid.interior(om.ql)).max())
    assert all(v < 1e-9 for v in errs.values()), {k: f"{v:.1e}" for k, v in errs.items()}
    assert (om.grid.interior(om.ql) > 0).any()


def test_config0_two_dimensional_bubble_as_y_invariant_run(oracle, bz):
    """BASELINE.json configs[0] (examples/dry_thermal_bubble.jl: 2-D (Periodic, Flat, Bounded) anelastic WENO5 bubble, the
    reference's CPU plumbing case, README.md:67-75) at reduced size: the oracle runs it on the Flat-y grid, the device runs
    the same problem as a y-invariant 3-D one (y fluxes cancel identically, only the k_y = 0 Poisson modes are excited)."""
    Nx, Nz, Ny = 64, 64, 8
    th = lambda x, y, z: 300.0 + 2.0 * np.cos(np.pi / 2 * np.minimum(1.0, np.sqrt(x ** 2 + (z - 2000.0) ** 2) / 2000.0)) ** 2 + 0 * y
    og = oracle.Grid((Nx, Nz), x=(-10e3, 10e3), z=(0, 10e3), topology=("Periodic", "Flat", "Bounded"))
    om = oracle.OracleModel(og, surface_pressure=101325, potential_temperature=300.0)
    om.set(theta=th)
    grid = bz.RectilinearGrid((Nx, Ny, Nz), x=(-10e3, 10e3), y=(0, 2500.0), z=(0, 10e3))
    hm = bz.AtmosphereModel(grid, dynamics=bz.AnelasticDynamics(bz.ReferenceState(grid, surface_pressure=101325, potential_temperature=300)),
                            advection=bz.WENO(order=5))
    hm.set(θ=th)
    for _ in range(5):
        om.time_step(2.0)
        hm.time_step(2.0)
    hm.synchronize()
    w3, w2 = hm.velocities["w"].interior_cpu(), og.interior(om.w, True)
    assert np.abs(w3 - w3[:, :1, :]).max() <= 1e-12 * np.abs(w3).max()          # stays y-invariant
    assert np.abs(hm.velocities["v"].interior_cpu()).max() <= 1e-12 * np.abs(w3).max()
    assert np.abs(w3[:, 0, :] - w2[:, 0, :]).max() / np.abs(w2).max() < 1e-9
    th3, th2 = hm.potential_temperature.interior_cpu(), og.interior(om.theta)
    assert np.abs(th3[:, 0, :] - th2[:, 0, :]).max() / 300.0 < 1e-12
    assert np.abs(w2).max() > 1e-3


def test_cell_advection_timescale_and_nan_checker(oracle, bz):
    """The run!-loop reductions: min 1/(|u|/dx + |v|/dy + |w|/dz) against numpy on the oracle's
    velocities, +Inf at rest, the horizontal formulation, and the NaN check of the first prognostic field."""
    om, hm = make_pair(oracle, bz, (32, 20, 16))
    assert bz.cell_advection_timescale(hm) == np.inf
    randomize(om, seed=5)
    push_state(om, hm, names=("ru", "rv", "rw", "rtheta", "rq"))
    bz.update_state_(hm, compute_tendencies=False)
    g = om.grid
    u, v, w = g.interior(om.u), g.interior(om.v), g.interior(om.w, True)[:-1]
    dz = g.dzf[g.Hz:g.Hz + g.Nz][:, None, None]
    want = 1.0 / (np.abs(u) / g.dx + np.abs(v) / g.dy + np.abs(w) / dz).max()
    want_h = 1.0 / (np.abs(u) / g.dx + np.abs(v) / g.dy).max()
    assert bz.cell_advection_timescale(hm) == pytest.approx(want, rel=1e-14)
    assert bz.cell_advection_timescale(hm, "Horizontal") == pytest.approx(want_h, rel=1e-14)
    assert bz.nan_checker(hm) is False
    hm.momentum["ρu"].interior[3, 4, 5] = float("nan")
    assert bz.nan_checker(hm) is True


# ---- DCMIP2016 Kessler column microphysics ---------------------------------------------------------
def test_kessler_column_update_matches_oracle(oracle, bz):
    """bz_kessler_microphysics_update against the oracle's restatement of `_microphysical_update!` (itself pinned to the
    reference test's independent Fortran translation at 1e-12), column by column: (a) the reference test's lapse-rate
    profile through 3-D density / pressure arrays, with moisture varied across columns; (b) the anelastic reference
    columns of the context.  This is the single-pass case: dt = 10 s is below every column's max_dt (about 13 s), so each
    column takes one sedimentation pass and no rain reaches the surface.  Subcycling, surface precipitation, the
    top-level rain flux and the clamps are driven by tests/test_kessler_columns.py."""
    import torch
    from oracle import kessler as ks
    Nx, Ny, Nz = 16, 8, 40
    grid = bz.RectilinearGrid((Nx, Ny, Nz), x=(0, 1600), y=(0, 800), z=(0, 4000))
    R, cpd = 8.314462618, 1003.0
    Md = R / 287.0
    tc = bz.ThermodynamicConstants(dry_air_molar_mass=Md, vapor_molar_mass=Md, dry_air_heat_capacity=cpd, vapor_heat_capacity=cpd,
                                   liquid_reference_latent_heat=2500000.0, liquid_heat_capacity=cpd)
    hm = bz.AtmosphereModel(grid, dynamics=bz.AnelasticDynamics(bz.ReferenceState(grid, tc, surface_pressure=1e5, potential_temperature=300)),
                            advection=bz.WENO(order=5), thermodynamic_constants=tc)
    c = ks.TetensConstants(molar_gas_constant=R, dry_air_molar_mass=Md, vapor_molar_mass=Md, dry_air_heat_capacity=cpd,
                           vapor_heat_capacity=cpd, liquid_latent_heat=2500000.0, liquid_heat_capacity=cpd, liquid_temperature_offset=36.0)
    tf = bz.TetensFormula(liquid_temperature_offset=36)
    mp, kp = bz.DCMIP2016KesslerMicrophysics(), ks.KesslerParameters()
    zc = grid.zᶜ
    rng = np.random.default_rng(11)
    p0 = 1e5
    ref = hm.dynamics.reference_state
    Hz = grid.Hz
    for case in ("arrays", "reference columns"):
        if case == "arrays":
            T = 288.0 - 0.0065 * zc
            p = 101325.0 * (T / 288.0) ** (9.81 / (287.0 * 0.0065))
            rho = p / (287.0 * T)
        else:
            rho, p = ref.density[Hz:Hz + Nz].copy(), ref.pressure[Hz:Hz + Nz].copy()
            T = p / (287.0 * rho)
        amp = 0.3 + 1.7 * rng.random((1, Ny, Nx))                       # per-column moisture amplitude
        rv = 0.015 * np.exp(-((zc - 1000) / 1000) ** 2)[:, None, None] * amp
        rcl = np.where((zc > 1500) & (zc < 2500), 0.002, 0.0)[:, None, None] * amp
        rr = np.where((zc > 1000) & (zc < 2000), 0.0005, 0.0)[:, None, None] * amp * 4
        rt = rv + rcl + rr
        qv, qcl, qr = rv / (1 + rt), rcl / (1 + rt), rr / (1 + rt)
        ql = qcl + qr
        cpm = (1 - (qv + ql)) * c.cpd + qv * c.cpv + ql * c.cl
        Rm = (1 - (qv + ql)) * c.Rd + qv * c.Rv
        theta = (T[:, None, None] - c.Ll * ql / cpm) / (p[:, None, None] / p0) ** (Rm / cpm)
        R3, P3 = np.broadcast_to(rho[:, None, None], theta.shape), np.broadcast_to(p[:, None, None], theta.shape)
        kf = bz.KesslerMicrophysicalFields(hm)
        hm.potential_temperature.set_interior(theta)
        hm.potential_temperature_density.set_interior(R3 * theta)
        hm.moisture_density.set_interior(R3 * qv)
        kf.rho_qcl.set_interior(R3 * qcl)
        kf.rho_qr.set_interior(R3 * qr)
        dens = pres = None
        if case == "arrays":
            dens, pres = bz.Field(grid, hm.potential_temperature.loc, hm.device), bz.Field(grid, hm.potential_temperature.loc, hm.device)
            dens.set_interior(R3)
            pres.set_interior(P3)
        dt = 10.0
        bz.microphysics_model_update_(mp, hm, kf, dt, tetens=tf, density=dens, pressure=pres, standard_pressure=p0)
        hm.synchronize()
        got = {"theta": hm.potential_temperature.interior_cpu(), "rtheta": hm.potential_temperature_density.interior_cpu(),
               "rqv": hm.moisture_density.interior_cpu(), "rqcl": kf.rho_qcl.interior_cpu(), "rqr": kf.rho_qr.interior_cpu(),
               "qv": kf.qv.interior_cpu(), "qcl": kf.qcl.interior_cpu(), "qr": kf.qr.interior_cpu(), "W": kf.W.interior_cpu()}
        precip = kf.precipitation_rate.cpu().numpy()[grid.Hy:grid.Hy + Ny, grid.Hx:grid.Hx + Nx]
        counts = set()
        for j in range(Ny):
            for i in range(Nx):
                th, rth = theta[:, j, i].copy(), (R3 * theta)[:, j, i].copy()
                a, b, d = (R3 * qv)[:, j, i].copy(), (R3 * qcl)[:, j, i].copy(), (R3 * qr)[:, j, i].copy()
                oqv, oqcl, oqr, oW, oP, Ns = ks.kessler_column_update(dt, rho, p, p0, zc, th, rth, a, b, d, kp, c)
                counts.add(Ns)
                for name, want in (("theta", th), ("rtheta", rth), ("rqv", a), ("rqcl", b), ("rqr", d), ("qv", oqv),
                                   ("qcl", oqcl), ("qr", oqr), ("W", oW)):
                    np.testing.assert_allclose(got[name][:, j, i], want, rtol=1e-11, atol=1e-18, err_msg=f"{case} {name} ({i},{j})")
                assert precip[j, i] == pytest.approx(oP, rel=1e-11, abs=1e-18)
        assert counts == {1}


def _kessler_pair(oracle, bz, size=(16, 12, 20), z=(0.0, 5e3), bubble_height=1500.0):
    extent = ((0.0, 4e3), (0.0, 3e3), z)
    og = oracle.Grid(size, x=extent[0], y=extent[1], z=extent[2])
    om = oracle.OracleModel(og, surface_pressure=1e5, potential_temperature=300.0, microphysics="Kessler")
    grid = bz.RectilinearGrid(size, x=extent[0], y=extent[1], z=extent[2])
    tc = bz.ThermodynamicConstants(saturation_vapor_pressure=bz.TetensFormula())
    ref = bz.ReferenceState(grid, tc, surface_pressure=1e5, potential_temperature=300.0)
    hm = bz.AtmosphereModel(grid, dynamics=bz.AnelasticDynamics(ref), advection=bz.WENO(order=5), thermodynamic_constants=tc,
                            microphysics=bz.DCMIP2016KesslerMicrophysics())
    from kessler_cases import anelastic_initial_conditions
    ic = anelastic_initial_conditions(bubble_height)
    return om, hm, ic


def test_kessler_model_requires_tetens_constants(bz):
    grid = bz.RectilinearGrid((16, 12, 20), x=(0, 4e3), y=(0, 3e3), z=(0, 5e3))
    with pytest.raises(ValueError):
        bz.AtmosphereModel(grid, dynamics=bz.AnelasticDynamics(bz.ReferenceState(grid)), advection=bz.WENO(order=5),
                           microphysics=bz.DCMIP2016KesslerMicrophysics())


def test_anelastic_kessler_model_matches_oracle(oracle, bz):
    """AtmosphereModel(...; microphysics = DCMIP2016KesslerMicrophysics()): diagnosis with (q^v, q^cl + q^r), species
    tendencies, moist buoyancy, and two full steps ending with the column update, against the oracle."""
    om, hm, ic = _kessler_pair(oracle, bz)
    om.set(**ic)
    hm.set(qᵗ=ic["qt"], θ=ic["theta"], qcl=ic["qcl"], qr=ic["qr"], u=ic["u"])
    g = om.grid
    μ = hm.microphysical_fields
    assert relerr(hm.temperature.cpu(), om.T) < 1e-14
    assert relerr(μ["qᶜˡ"].cpu(), om.qcl) < 1e-15 and relerr(μ["qʳ"].cpu(), om.qr) < 1e-15
    om.compute_tendencies()
    bz.compute_tendencies_(hm)
    for n, k in list(PROG.items()) + [("rqcl", "ρqᶜˡ"), ("rqr", "ρqʳ")]:
        zf = n == "rw"
        want, got = g.interior(om.G[n], zface=zf), hm.G[k].interior_cpu()
        if zf:
            want, got = want[1:-1], got[1:-1]
        assert relerr(got, want) < (5e-9 if n in ("rtheta", "rq", "rqcl", "rqr") else 1e-12), n
    for _ in range(2):
        om.time_step(5.0)
        hm.time_step(5.0)
    hm.synchronize()
    errs = {}
    mom = max(np.abs(_interior(om, n)).max() for n in ("ru", "rv", "rw"))
    for n, f in (("ru", hm.momentum["ρu"]), ("rw", hm.momentum["ρw"]), ("rtheta", hm.potential_temperature_density),
                 ("rq", hm.moisture_density), ("rqcl", μ["ρqᶜˡ"]), ("rqr", μ["ρqʳ"]), ("T", hm.temperature), ("W", μ["𝕎ʳ"])):
        want = g.interior(getattr(om, n), n == "rw")
        scale = mom if n in ("ru", "rw") else max(np.abs(want).max(), 1e-6)
        errs[n] = float(np.abs(f.interior_cpu() - want).max() / scale)
    assert all(v < 1e-8 for v in errs.values()), {k: f"{v:.1e}" for k, v in errs.items()}
    P = μ["precipitation_rate"].cpu().numpy()[g.Hy:g.Hy + g.Ny, g.Hx:g.Hx + g.Nx]
    assert np.abs(P - om.precipitation_rate).max() <= 1e-9 * max(np.abs(om.precipitation_rate).max(), 1e-12)
    assert g.interior(om.W).max() > 0.5


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(4, 4, 4), (6, 6, 4), (5, 7, 3), (64, 6, 5), (8, 8, 6), (3, 3, 3), (7, 4, 4)])
def test_minimal_and_ragged_grids_step_like_the_oracle(oracle, bz, size):
    """Edge sizes: the reference's own smoke tests run on 4 x 4 x 4 boxes (halo 3: fewer interior cells than 2 H, so the halo
    images overlap and the device leaves its fused tiers), 6 x 6 is the smallest grid of the fused tiers, odd / prime extents
    exercise every partial tile, and Nz = 3 has only reduced-order vertical stencils."""
    om, hm = make_pair(oracle, bz, size, extent=((0.0, 400.0), (0.0, 400.0), (0.0, 400.0)), theta0=300.0)
    th = lambda x, y, z: 300.0 + 0.01 * z + 0.5 * np.sin(2 * np.pi * x / 400.0) * np.cos(2 * np.pi * y / 400.0)
    om.set(theta=th, u=1.0, v=-0.5)
    hm.set(θ=th, u=1.0, v=-0.5)
    for _ in range(2):
        om.time_step(0.5)
        hm.time_step(0.5)
    hm.synchronize()
    mom = max(np.abs(_interior(om, n)).max() for n in ("ru", "rv", "rw"))
    for n, k in PROG.items():
        want, got = _interior(om, n), hm.prognostic_fields()[k].interior_cpu()
        scale = mom if n in ("ru", "rv", "rw") else max(np.abs(want).max(), 1e-3)
        assert np.abs(got - want).max() / scale < 1e-10, (n, size)
    assert np.isfinite(hm.temperature.interior_cpu()).all()


@pytest.mark.gpu
def test_reference_set_temperature_and_relative_humidity(bz):
    """test/set_atmosphere_model.jl:100-155 and :157-215 restated on the device model: set!(model; T) reproduces the lapse-rate
    profile (rtol 1e-4) with theta increasing upward and a T -> theta -> T round trip; set!(model; θ, ℋ) yields the requested
    relative humidity (rtol 5e-2), a function ℋ(z) is followed level by level, and ℋ = 1.5 condenses everywhere with the
    adjusted state capped at saturation."""
    grid = bz.RectilinearGrid((4, 4, 10), x=(0, 1000.0), y=(0, 1000.0), z=(0, 5000.0))
    ref = bz.ReferenceState(grid, surface_pressure=101500.0, potential_temperature=300.0)
    m = bz.AtmosphereModel(grid, dynamics=bz.AnelasticDynamics(ref), advection=bz.WENO(order=5))
    T_profile = lambda x, y, z: 300.0 - 0.0065 * z + 0 * x + 0 * y
    m.set(T=T_profile, qᵗ=0.0)
    zc = np.asarray(grid.zᶜ)
    T = m.temperature.interior_cpu()
    np.testing.assert_allclose(T[:, 0, 0], 300.0 - 0.0065 * zc, rtol=1e-4)
    th = m.potential_temperature.interior_cpu()[:, 0, 0]
    assert np.all(np.diff(th) > 0)
    m.set(T=280.0, qᵗ=0.0)
    assert m.temperature.interior_cpu()[4, 1, 1] == pytest.approx(280.0, rel=1e-4)

    # relative humidity with warm-phase saturation adjustment
    grid1 = bz.RectilinearGrid((8, 8, 8), x=(0, 1e3), y=(0, 1e3), z=(0, 1e3))
    ref1 = bz.ReferenceState(grid1, surface_pressure=101325.0, potential_temperature=300.0)
    c = bz.ThermodynamicConstants()
    from breeze_jl_amd.thermodynamics import dry_air_gas_constant, vapor_gas_constant
    Rd, Rv = dry_air_gas_constant(c), vapor_gas_constant(c)

    def relative_humidity(model):      # p^v / p^v+ with p^v = q^v rho R^v T, rho = p_r / (R^m T)
        T = model.temperature.interior_cpu()
        qv, ql = model.microphysical_fields["qᵛ"].interior_cpu(), model.microphysical_fields["qˡ"].interior_cpu()
        Hz, Nz = grid1.Hz, grid1.Nz
        pr = ref1.pressure[Hz:Hz + Nz][:, None, None]
        Rm = (1 - qv - ql) * Rd + qv * Rv
        rho = pr / (Rm * T)
        dc = c.vapor_heat_capacity - c.liquid_heat_capacity
        L0 = c.liquid_reference_latent_heat - dc * c.energy_reference_temperature
        ps = c.triple_point_pressure * (T / c.triple_point_temperature) ** (dc / Rv) * np.exp((1 / c.triple_point_temperature - 1 / T) * L0 / Rv)
        return qv * rho * Rv * T / ps

    def moist_model():
        return bz.AtmosphereModel(grid1, dynamics=bz.AnelasticDynamics(ref1), advection=bz.WENO(order=5), thermodynamic_constants=c,
                                  microphysics=bz.SaturationAdjustment(equilibrium=bz.WarmPhaseEquilibrium()))

    m1 = moist_model()
    m1.set(θ=300.0, ℋ=0.5)
    np.testing.assert_allclose(relative_humidity(m1), 0.5, rtol=5e-2)
    assert (m1.microphysical_fields["qᵛ"].interior_cpu() > 0).all()
    m2 = moist_model()
    H = lambda x, y, z: 0.8 * np.exp(-z / 500.0) + 0 * x + 0 * y
    m2.set(θ=300.0, ℋ=H)
    zc1 = np.asarray(grid1.zᶜ)
    np.testing.assert_allclose(relative_humidity(m2)[:, 0, 0], 0.8 * np.exp(-zc1 / 500.0), rtol=5e-2)
    m3 = moist_model()
    m3.set(θ=300.0, ℋ=1.5)
    assert (m3.microphysical_fields["qˡ"].interior_cpu() > 0).all()
    assert (relative_humidity(m3) <= 1.01).all()


@pytest.mark.gpu
def test_device_reproduces_reference_doctest_numbers(bz):
    """The reference-generated Field summaries of the StaticEnergy and RelativeHumidity doctests (tests/golden/reference_doctests.json,
    six printed digits), recomputed from the DEVICE model's temperature / moisture fields on the doctests' default models."""
    import json
    import os
    gd = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "reference_doctests.json"), encoding="utf-8"))["model_diagnostics"]
    sig = lambda x: 0.6 * 10.0 ** (np.floor(np.log10(abs(x))) - 5)
    c = bz.ThermodynamicConstants()
    from breeze_jl_amd.thermodynamics import dry_air_gas_constant, vapor_gas_constant
    Rd, Rv = dry_air_gas_constant(c), vapor_gas_constant(c)
    grid = bz.RectilinearGrid((8, 8, 8), x=(0, 1.0), y=(0, 1.0), z=(-1000.0, 0.0))
    m = bz.AtmosphereModel(grid)                    # every default, as in the doctest (advection Centered(2), ReferenceState defaults)
    m.set(θ=300.0)
    T = m.temperature.interior_cpu()[:, 0, 0]
    e = c.dry_air_heat_capacity * T + c.gravitational_acceleration * np.asarray(grid.zᶜ)
    for key, val in (("max", e.max()), ("min", e.min()), ("mean", e.mean())):
        assert abs(val - gd["static_energy"][key]) <= sig(gd["static_energy"][key]), (key, val)
    grid2 = bz.RectilinearGrid((8, 8, 128), x=(0, 1e3), y=(0, 1e3), z=(-1000.0, 0.0))
    m2 = bz.AtmosphereModel(grid2, microphysics=bz.SaturationAdjustment(equilibrium=bz.WarmPhaseEquilibrium()))
    m2.set(θ=300.0, qᵗ=0.005)
    T = m2.temperature.interior_cpu()[:, 0, 0]
    qv = m2.microphysical_fields["qᵛ"].interior_cpu()[:, 0, 0]
    ref = m2.dynamics.reference_state
    p = ref.pressure[grid2.Hz:grid2.Hz + grid2.Nz]
    rho = p / (((1 - qv) * Rd + qv * Rv) * T)
    dc = c.vapor_heat_capacity - c.liquid_heat_capacity
    L0 = c.liquid_reference_latent_heat - dc * c.energy_reference_temperature
    ps = c.triple_point_pressure * (T / c.triple_point_temperature) ** (dc / Rv) * np.exp((1 / c.triple_point_temperature - 1 / T) * L0 / Rv)
    rh = rho * qv * Rv * T / ps
    for key, val in (("max", rh.max()), ("min", rh.min()), ("mean", rh.mean())):
        assert abs(val - gd["relative_humidity"][key]) <= sig(gd["relative_humidity"][key]), (key, val)


def _moist_q(x, y, z):
    r = np.sqrt(x ** 2 + (y - 1000.0) ** 2 + (z - 2500.0) ** 2)
    return 8e-3 * np.exp(-z / 2500.0) * (1.0 + 0.3 * np.maximum(0.0, 1.0 - r / 3e3))


@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("size,moist", [((32, 20, 16), False), ((32, 20, 16), True), ((72, 24, 40), True), ((130, 16, 12), False),
                                        ((64, 64, 12), True)])      # Ny >= 64: the 64 x 16 tiles of the y-momentum kernel
def test_lean_seam_matches_the_diagnostic_seam(oracle, bz, size, moist, strict, monkeypatch):
    """The lean whole-step seam (bz_tendency5_kernels.h: tendency kernels on prognostic fields only, u, v, w, theta, q^v, T derived
    on the fly with the correctly rounded column division, momentum-only projection in stages 1-2) against the generation-4 seam
    that reads stored diagnostics (BZ_NO_LEAN=1), three steps, dry (table-driven Exner factor) and with vapour (pow() behind the
    noinline call), full and ragged tiles.
      strict: the -ffp-contract=off build (lib/libbreeze_hip_refdiv.so): every field, halos included, carries the SAME BITS —
              the derived quantities are exactly the stored ones (tools/check_cdiv_gpu.hip: 0 mismatches in 4e9 divisions);
      default build: hipcc contracts mul+add into FMA differently in the two kernel generations, so the last bit of a few
              per cent of the momentum values differs after the third step: 1e-13 of the field scale (the tolerance of the
              whole-step-versus-operator-sequence test)."""
    from breeze_jl_amd import _lib
    if strict:
        monkeypatch.setattr(_lib, "LIB_PATH", os.path.join(os.path.dirname(_lib.LIB_PATH), "libbreeze_hip_refdiv.so"))
    th = bubble_theta(300.0, 9.81)
    runs = []
    for lean in (True, False):
        if lean:
            monkeypatch.delenv("BZ_NO_LEAN", raising=False)
        else:
            monkeypatch.setenv("BZ_NO_LEAN", "1")
        om, hm = make_pair(oracle, bz, size)
        kw = dict(θ=th, u=3.0, v=-2.0)
        if moist:
            kw["qᵗ"] = _moist_q
        hm.set(**kw)
        for _ in range(3):
            hm.time_step(1.5)
        hm.synchronize()
        runs.append(hm)
    a, b = runs
    fields = {"ρu": lambda m: m.momentum["ρu"], "ρv": lambda m: m.momentum["ρv"], "ρw": lambda m: m.momentum["ρw"],
              "ρθ": lambda m: m.potential_temperature_density, "ρq": lambda m: m.moisture_density,
              "u": lambda m: m.velocities["u"], "w": lambda m: m.velocities["w"], "θ": lambda m: m.potential_temperature,
              "q": lambda m: m.specific_moisture, "T": lambda m: m.temperature, "ϕ": lambda m: m.dynamics.pressure_anomaly}
    for name, get in fields.items():
        fa, fb = get(a), get(b)
        if strict:
            assert np.array_equal(fa.interior_cpu(), fb.interior_cpu()), name
            if name not in ("u", "w"):          # velocity z-halos are `nothing` boundary conditions: never filled
                assert np.array_equal(fa.cpu(), fb.cpu()), name + " (halos)"
        else:
            assert relerr(fa.interior_cpu(), fb.interior_cpu()) < 1e-13, name
    if moist and not strict:               # and the moist lean seam against the oracle
        om, _ = make_pair(oracle, bz, size)
        om.set(theta=th, u=3.0, v=-2.0, qt=_moist_q)
        for _ in range(3):
            om.time_step(1.5)
        for n, k in PROG.items():
            got = a.prognostic_fields()[k].interior_cpu()
            want = _interior(om, n)
            assert np.max(np.abs(got - want)) / max(np.max(np.abs(want)), 1e-3) < 1e-9, n
