"""k_kessler_column where its lanes diverge: sedimentation subcycle counts from 1 to 7 inside one wavefront, surface precipitation,
rain on the top level, clamped negative inputs, 3-D density and pressure, a partly filled block, a stretched z grid; the memory
the kernel must not touch; the time steps on which it must do nothing; and whole model steps whose columns subcycle.

The inputs, the oracle runs and the column-scaled measure are in tests/kessler_cases.py; tests/test_oracle_kessler.py asserts on
the CPU that the case really has these properties."""
import numpy as np
import pytest

import kessler_cases as kc
from test_gpu_parity import _interior, _kessler_pair

pytestmark = pytest.mark.gpu

SENTINEL = -1.2345e300          # halo filler: finite, and nothing the kernel could compute


@pytest.fixture(scope="module")
def ks(oracle):
    from oracle import kessler
    return kessler


class _Columns:
    """The device side of one variant of the column case: an anelastic model on the stretched grid whose θ, ρθ, ρqᵛ and a set of
    KesslerMicrophysicalFields carry the inputs; every halo (and the precipitation rate's ring) holds SENTINEL."""

    def __init__(self, bz, variant):
        import torch
        self.bz, self.variant = bz, variant
        grid = bz.RectilinearGrid((kc.NX, kc.NY, kc.NZ), x=kc.X_EXTENT, y=kc.Y_EXTENT, z=kc.Z_FACES)
        tc = bz.ThermodynamicConstants(dry_air_molar_mass=kc.MD, vapor_molar_mass=kc.MD, dry_air_heat_capacity=kc.CPD,
                                       vapor_heat_capacity=kc.CPD, liquid_reference_latent_heat=kc.LATENT, liquid_heat_capacity=kc.CPD)
        hm = bz.AtmosphereModel(grid, dynamics=bz.AnelasticDynamics(bz.ReferenceState(grid, tc, surface_pressure=kc.P0, potential_temperature=300)),
                                advection=bz.WENO(order=5), thermodynamic_constants=tc)
        self.grid, self.hm = grid, hm
        assert np.array_equal(grid.zᶜ, kc.z_centers())
        ref = hm.dynamics.reference_state
        Hz = grid.Hz
        self.reference = (ref.density[Hz:Hz + kc.NZ].copy(), ref.pressure[Hz:Hz + kc.NZ].copy())
        self.kf = kf = bz.KesslerMicrophysicalFields(hm)
        self.written = {"theta": hm.potential_temperature, "rtheta": hm.potential_temperature_density, "rqv": hm.moisture_density,
                        "rqcl": kf.rho_qcl, "rqr": kf.rho_qr, "qv": kf.qv, "qcl": kf.qcl, "qr": kf.qr, "W": kf.W}
        self.dens = self.pres = None
        if variant == "arrays":
            self.dens, self.pres = (bz.Field(grid, hm.potential_temperature.loc, hm.device) for _ in range(2))
        self.torch = torch

    def load(self, case):
        for f in self.written.values():
            f.parent.fill_(SENTINEL)
        self.kf.precipitation_rate.fill_(SENTINEL)
        for n in ("theta", "rtheta", "rqv", "rqcl", "rqr"):
            self.written[n].set_interior(case[n])
        for n in ("qv", "qcl", "qr", "W"):                  # outputs only: the kernel overwrites every interior element
            self.written[n].set_interior(0.0)
        if self.dens is not None:
            self.dens.set_interior(case["rho"])
            self.pres.set_interior(case["p"])
        self.torch.cuda.synchronize()

    def update(self, dt):
        self.bz.microphysics_model_update_(self.bz.DCMIP2016KesslerMicrophysics(), self.hm, self.kf, dt,
                                           tetens=self.bz.TetensFormula(liquid_temperature_offset=kc.TETENS_OFFSET),
                                           density=self.dens, pressure=self.pres, standard_pressure=kc.P0)
        self.hm.synchronize()
        self.torch.cuda.synchronize()

    def parents(self):
        """Host copies of every array the kernel may write, halos included (read straight from the device arrays)."""
        out = {n: f.parent.cpu().numpy() for n, f in self.written.items()}
        out["precip"] = self.kf.precipitation_rate.cpu().numpy()
        return out

    def interiors(self, parents):
        g = self.grid
        out = {n: parents[n][g.Hz:g.Hz + kc.NZ, g.Hy:g.Hy + kc.NY, g.Hx:g.Hx + kc.NX] for n in kc.FIELDS}
        out["precip"] = parents["precip"][g.Hy:g.Hy + kc.NY, g.Hx:g.Hx + kc.NX]
        return out

    def halos_untouched(self, parents):
        g = self.grid
        bits = np.float64(SENTINEL).view(np.int64)
        bad = []
        for n, a in parents.items():
            inside = np.zeros(a.shape, dtype=bool)
            if a.ndim == 3:
                inside[g.Hz:g.Hz + kc.NZ, g.Hy:g.Hy + kc.NY, g.Hx:g.Hx + kc.NX] = True
            else:
                inside[g.Hy:g.Hy + kc.NY, g.Hx:g.Hx + kc.NX] = True
            assert (~inside).sum() > 0
            touched = (np.ascontiguousarray(a).view(np.int64) != bits) & ~inside
            if touched.any():
                bad.append((n, int(touched.sum()), tuple(int(v) for v in np.argwhere(touched)[0])))
        return bad


@pytest.fixture(scope="module")
def columns(bz):
    cache = {}

    def get(variant):
        if variant not in cache:
            cache[variant] = _Columns(bz, variant)
        return cache[variant]
    return get


@pytest.mark.parametrize("variant", kc.VARIANTS)
def test_subcycling_columns_match_oracle(ks, columns, variant):
    """All 216 columns of the case against the oracle, per column and per field at kc.TOL = max(1e-11, 100 c1) of the column's
    own scale, the precipitation rate relatively; reference columns that are identically zero (W without rain, q^cl after complete
    evaporation, the precipitation of rainless columns) must be identically zero on the device.  Every halo element and the ring
    around the precipitation rate keep the bits they had before the launch.

    Worst column-scaled errors measured on the MI355X: see DESIGN.md, "Kessler column tests"."""
    dev = columns(variant)
    case, want, ratios = kc.oracle_case(ks, variant)
    if variant == "reference columns":
        # the device reads the context's reference columns: the oracle gets the same numbers
        rho, p = dev.reference
        assert np.array_equal(rho, case["rho"][:, 0, 0]) and np.array_equal(p, case["p"][:, 0, 0])
    assert set(want["Ns"][0, :64].tolist()) >= {1, 3, 5, 6, 7} and kc.integer_distance(ratios) >= 1e-3
    dev.load(case)
    dev.update(kc.DT)
    parents = dev.parents()
    got = dev.interiors(parents)
    kc.assert_columns_match(variant, got, want)
    assert got["precip"].max() > 0.01
    assert dev.halos_untouched(parents) == []


@pytest.mark.parametrize("dt", [0.0, -1.0, float("nan"), float("inf")])
def test_noop_time_steps_leave_every_bit(ks, columns, dt):
    """dt <= 0, NaN and Inf return success before any launch: every field, halos included, and the precipitation rate (pre-filled
    with a sentinel) are bitwise what they were."""
    dev = columns("arrays")
    case, _, _ = kc.oracle_case(ks, "arrays")
    dev.load(case)
    before = dev.parents()
    dev.update(dt)                      # raises on any status other than success
    after = dev.parents()
    for n in before:
        assert np.array_equal(before[n].view(np.int64), after[n].view(np.int64)), n
    assert (after["precip"] == SENTINEL).all()


def test_anelastic_model_steps_with_subcycling_columns(oracle, bz, ks):
    """bzi_kessler_update -> bz_update_state with columns at Ns = 1 .. 3: the set-up of test_anelastic_kessler_model_matches_oracle
    on (16, 12, 40) levels of 50 m with the bubble low enough for its rain to reach the ground, two steps of 16 s
    (kc.ANELASTIC_STEPS); tolerances of that test (1e-8 of the field scale, 1e-9 on the precipitation rate)."""
    case = kc.ANELASTIC_STEPS
    dt, steps = case["dt"], case["steps"]
    om, hm, ic = _kessler_pair(oracle, bz, size=case["size"], z=case["z"], bubble_height=case["bubble_height"])
    om.set(**ic)
    hm.set(qᵗ=ic["qt"], θ=ic["theta"], qcl=ic["qcl"], qr=ic["qr"], u=ic["u"])
    g = om.grid
    μ = hm.microphysical_fields
    rho = np.ascontiguousarray(om.ref.density[g.Hz:g.Hz + g.Nz])
    record = kc.record_subcycling(ks, om, dt, lambda: rho)
    for _ in range(steps):
        record["measure"]()
        om.time_step(dt)
        hm.time_step(dt)
    hm.synchronize()
    kc.assert_subcycling("anelastic", record, steps)
    errs = {}
    mom = max(np.abs(_interior(om, n)).max() for n in ("ru", "rv", "rw"))
    for n, f in (("ru", hm.momentum["ρu"]), ("rw", hm.momentum["ρw"]), ("rtheta", hm.potential_temperature_density),
                 ("rq", hm.moisture_density), ("rqcl", μ["ρqᶜˡ"]), ("rqr", μ["ρqʳ"]), ("T", hm.temperature), ("W", μ["𝕎ʳ"])):
        want = g.interior(getattr(om, n), n == "rw")
        scale = mom if n in ("ru", "rw") else max(np.abs(want).max(), 1e-6)
        errs[n] = float(np.abs(f.interior_cpu() - want).max() / scale)
    P = μ["precipitation_rate"].cpu().numpy()[g.Hy:g.Hy + g.Ny, g.Hx:g.Hx + g.Nx]
    Pmax = np.abs(om.precipitation_rate).max()
    errs["precip"] = float(np.abs(P - om.precipitation_rate).max() / max(Pmax, 1e-12))
    print("anelastic kessler, subcycling columns:", {k: f"{v:.1e}" for k, v in errs.items()}, f"precipitation max {Pmax:.3g}")
    assert Pmax > 0
    assert all(v < kc.STEPS_TOL for k, v in errs.items() if k != "precip"), {k: f"{v:.1e}" for k, v in errs.items()}
    assert errs["precip"] <= 1e-9


def test_compressible_model_steps_with_subcycling_columns(oracle, oc, bz, ks):
    """The compressible path, where the columns read a genuinely 3-D density and pressure: the set-up of
    test_compressible_kessler_model_matches_oracle on (16, 12, 40) levels of 10 m with the bubble on the ground and no mean wind, two steps of 4 s
    with 12 acoustic substeps (kc.COMPRESSIBLE_STEPS), columns at Ns = 1 .. 3; tolerances of that test (1e-8 of the field scale)."""
    from test_gpu_compressible import cmp_interior
    case = kc.COMPRESSIBLE_STEPS
    dt, steps = case["dt"], case["steps"]
    om = kc.compressible_oracle(oracle, oc, **case)
    grid = bz.RectilinearGrid(case["size"], x=kc.STEPS_X, y=kc.STEPS_Y, z=case["z"])
    tc = bz.ThermodynamicConstants(saturation_vapor_pressure=bz.TetensFormula())
    dyn = bz.CompressibleDynamics(bz.SplitExplicitTimeDiscretization(substeps=case["substeps"]), surface_pressure=1e5,
                                  reference_potential_temperature=300.0)
    hm = bz.CompressibleAtmosphereModel(grid, dyn, advection=bz.WENO(order=5), thermodynamic_constants=tc,
                                        microphysics=bz.DCMIP2016KesslerMicrophysics())
    rho = kc.set_compressible_oracle(om, **case)
    ic = kc.compressible_initial_conditions(case["bubble_height"], case["u"])
    hm.set(ρ=rho, θ=ic["theta"], u=ic["u"], v=ic["v"], w=ic["w"], qᵗ=ic["qv"], qcl=ic["qcl"], qr=ic["qr"])
    μ = hm.microphysical_fields
    g = om.grid
    record = kc.record_subcycling(ks, om, dt, lambda: g.interior(om.rho_d))
    for _ in range(steps):
        record["measure"]()
        om.time_step(dt)
        hm.time_step(dt)
    kc.assert_subcycling("compressible", record, steps)
    assert np.ptp(g.interior(om.rho_d), axis=2).max() > 1e-3                    # density varies along x inside a wavefront
    worst = cmp_interior(om, hm, ("rho_d", "rtheta", "rq", "ru", "rw", "T", "p"), np.inf)
    for n, k in (("rqcl", "ρqᶜˡ"), ("rqr", "ρqʳ"), ("W", "𝕎ʳ"), ("qcl", "qᶜˡ")):
        want = g.interior(getattr(om, n))
        worst[n] = float(np.abs(μ[k].interior_cpu() - want).max() / max(np.abs(want).max(), 1e-9))
    P = μ["precipitation_rate"].cpu().numpy()[g.Hy:g.Hy + g.Ny, g.Hx:g.Hx + g.Nx]
    Pmax = np.abs(om.precipitation_rate).max()
    worst["precip"] = float(np.abs(P - om.precipitation_rate).max() / max(Pmax, 1e-12))
    print("compressible kessler, subcycling columns:", {k: f"{v:.1e}" for k, v in worst.items()}, f"precipitation max {Pmax:.3g}")
    assert Pmax > 0
    assert all(v <= kc.STEPS_TOL for v in worst.values()), {k: f"{v:.1e}" for k, v in worst.items()}
