"""The three clients of the bounds-preserving WENO kernel (csrc/bz_bounded.hip: bzi_bounded_tendencies) on the device against the oracle:
moisture (bounded_mask & 1), the two Kessler condensate species (& 2) and user tracers (& 4), alone and all at once, on the grids and
rough two-plateau states of tests/bounded_weno_cases.py — ragged tiles, stretched z, z-chunk seams at 11 + 10 and 8 + 8 + 8, a column of
7 levels where all but two faces take reduced stencils, and the Flat-y branch.  tests/test_bounded_weno_reference.py pins the oracle's
operator on the same states to a long-double reference and shows that the limiter is active on them.

Every run goes through bz.compute_tendencies_ after bit-for-bit copies of the oracle's state.  The scalar tendency arrays start as NaN,
halos included: afterwards the interior holds none and every halo entry of a limited array still does (the kernel writes the interior
only, above and below the z-chunk seams too).  A limited tendency must differ from the plain WENO-5 one by more than 1e-4, so a launch
that did not happen (a mask bit lost between the host and bzi_bounded_tendencies) fails; a scalar whose class is not limited must
keep the plain tendency.

TOLERANCE 1e-12 of max|want|, the project's bound for a device tendency against the oracle: the oracle itself is within 5.7e-14 of
the long-double reference on these states (measured, tests/test_bounded_weno_reference.py), below the 1e-13 at which the bound would
have to follow the oracle's own error."""
import functools

import numpy as np
import pytest

import bounded_weno_cases as cases
from helpers import bubble_theta, push_state, randomize

TOLERANCE = 1e-12
# oracle name of a limited scalar -> (its specific field, its key among the device model's prognostic fields)
SCALARS = {"rq": ("q", "ρq"), "rqcl": ("qcl", "ρqᶜˡ"), "rqr": ("qr", "ρqʳ"), "rc0": ("c0", "a"), "rc1": ("c1", "b")}
CONFIGURATIONS = {"moisture": ("rq",), "species": ("rqcl", "rqr"), "tracers": ("rc0", "rc1"), "all": ("rq", "rqcl", "rqr", "rc0", "rc1")}


def _oracle_options(config):
    kw = dict(surface_pressure=1e5, microphysics="Kessler") if config in ("species", "all") else {}
    if config in ("tracers", "all"):
        kw["tracers"] = 2
    return kw


@functools.lru_cache(maxsize=None)
def _oracle_case(config, name, bounds):
    """(oracle model holding the state and the tendencies with `config`'s scalars limited, its plain WENO-5 tendencies): computed once,
    shared, never changed"""
    from oracle import oracle
    oracle.build()
    om = cases.oracle_model(oracle, name, **_oracle_options(config))
    randomize(om, seed=cases.SEED)
    for s, key in enumerate(CONFIGURATIONS[config]):          # a state of its own for every limited scalar
        cases.plant(om, SCALARS[key][0], key, *bounds, seed=cases.SEED + 1 + s)
    om.compute_tendencies()
    plain = {n: om.G[n].copy() for n in om.PROGNOSTIC}
    om.bounded = {key: bounds for key in CONFIGURATIONS[config]}
    om.compute_tendencies()
    return om, plain


def _device_model(bz, config, name, bounds, size=None):
    if size is None:
        size, kw = cases.grid_arguments(name)
        if name == "flat":
            kw["topology"] = (bz.Periodic, bz.Flat, bz.Bounded)
    else:
        kw = dict(x=cases.EXT[0], y=cases.EXT[1], z=cases.EXT[2])
    grid = bz.RectilinearGrid(size, **kw)
    W, B = bz.WENO(), bz.WENO(bounds=bounds)
    device_keys = {"rq": "ρqᵛ", "rqcl": "ρqᶜˡ", "rqr": "ρqʳ", "rc0": "a", "rc1": "b"}
    advection = {"momentum": W, "ρθ": W, **{device_keys[k]: B for k in CONFIGURATIONS[config]}}
    mkw = {}
    if config in ("species", "all"):
        tc = bz.ThermodynamicConstants(saturation_vapor_pressure=bz.TetensFormula())
        ref = bz.ReferenceState(grid, tc, surface_pressure=1e5, potential_temperature=300.0)
        mkw.update(thermodynamic_constants=tc, microphysics=bz.DCMIP2016KesslerMicrophysics())
    else:
        ref = bz.ReferenceState(grid, potential_temperature=300.0)
    if config in ("tracers", "all"):
        mkw["tracers"] = ("a", "b")
    return bz.AtmosphereModel(grid, dynamics=bz.AnelasticDynamics(ref), advection=advection, **mkw)


def _push(om, hm):
    """the oracle's arrays, halos included, into the device model's fields, bit for bit"""
    import torch
    push_state(om, hm, names=("ru", "rv", "rw", "rtheta", "rq", "u", "v", "w", "theta", "q", "T"))
    copy = lambda field, name: field.parent.copy_(torch.from_numpy(getattr(om, name)))
    if om.microphysics == "Kessler":
        μ = hm.microphysical_fields
        for k, n in (("ρqᶜˡ", "rqcl"), ("ρqʳ", "rqr"), ("qᵛ", "qv"), ("qᶜˡ", "qcl"), ("qʳ", "qr")):
            copy(μ[k], n)
    for t, n in enumerate(hm.tracers):
        copy(hm.tracers[n], f"rc{t}")
        copy(hm.specific_tracers[n], f"c{t}")


def _relative(got, want):
    return float(np.max(np.abs(got - want)) / max(np.max(np.abs(want)), 1e-30))


def _check_tendencies(bz, config, name, bounds):
    import torch
    om, plain = _oracle_case(config, name, bounds)
    hm = _device_model(bz, config, name, bounds)
    _push(om, hm)
    g = om.grid
    scalars = [n for n in om.PROGNOSTIC if n not in ("ru", "rv", "rw")]
    key = lambda n: SCALARS[n][1] if n in SCALARS else "ρθ"
    for n in scalars:
        hm.G[key(n)].parent.fill_(float("nan"))
    torch.cuda.synchronize()
    bz.compute_tendencies_(hm)
    hm.synchronize()
    errs, off_plain = {}, {}
    for n in scalars:
        G = hm.G[key(n)].parent.cpu().numpy()
        interior = np.zeros(G.shape, dtype=bool)
        g.interior(interior)[...] = True
        assert not np.isnan(G[interior]).any(), (n, "interior cells the kernel did not write")
        if n in om.bounded:
            assert np.isnan(G[~interior]).all(), (n, "the bounded kernel wrote outside the interior", int((~np.isnan(G[~interior])).sum()))
            off_plain[n] = _relative(g.interior(G), g.interior(plain[n]))
        errs[n] = _relative(g.interior(G), g.interior(om.G[n]))      # om.G: limited where om.bounded says so, plain elsewhere
    print(f"BOUNDED-DEVICE {config} {name} {bounds}:", " ".join(f"{n}={e:.2e}" for n, e in errs.items()), "| off plain:",
          " ".join(f"{n}={e:.2e}" for n, e in off_plain.items()))
    assert set(off_plain) == set(CONFIGURATIONS[config])
    assert all(e < TOLERANCE for e in errs.values()), errs
    assert all(e > 1e-4 for e in off_plain.values()), off_plain
    return om


@pytest.mark.gpu
@pytest.mark.parametrize("bounds", cases.BOUNDS)
@pytest.mark.parametrize("name", list(cases.GRIDS))
def test_bounded_moisture_tendency_on_hard_columns(oracle, bz, name, bounds):
    om = _check_tendencies(bz, "moisture", name, bounds)
    if name == "flat":
        assert np.abs(om.v).max() > 0          # the flat_y branch has a v to ignore


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ragged", "thin"])
def test_bounded_kessler_species_tendencies(oracle, bz, name):
    """mask 2 alone: G(rho q^cl) and G(rho q^r) limited, G(rho q) and G(rho theta) plain"""
    _check_tendencies(bz, "species", name, cases.BOUNDS[1])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ragged", "thin"])
def test_bounded_tracer_tendencies(oracle, bz, name):
    """mask 4 alone: both tracers limited, G(rho q) and G(rho theta) plain"""
    _check_tendencies(bz, "tracers", name, cases.BOUNDS[0])


@pytest.mark.gpu
def test_all_three_bounded_masks_at_once(oracle, bz):
    """Kessler + two tracers + moisture under one pair of bounds: five limited tendencies, rho theta untouched"""
    _check_tendencies(bz, "all", "ragged", cases.BOUNDS[1])


@pytest.mark.gpu
@pytest.mark.parametrize("config", ["species", "tracers"])
def test_three_steps_with_bounded_species_or_tracers_alone(oracle, bz, config):
    """bz_time_step with mask 2 or mask 4 alone (the whole-step tiers decide by the mask): the sharp blob of
    tests/test_bounded_weno.py in q^cl (in tracer a), three steps against the oracle at that test's 1e-8 with its scale floor"""
    from test_bounded_weno import QMAX, _blob
    size, bounds = (24, 24, 20), (0.0, QMAX)
    om = oracle.OracleModel(oracle.Grid(size, x=cases.EXT[0], y=cases.EXT[1], z=cases.EXT[2]), potential_temperature=300.0, **_oracle_options(config))
    om.bounded = {key: bounds for key in CONFIGURATIONS[config]}
    hm = _device_model(bz, config, None, bounds, size=size)
    th = bubble_theta(300.0, 9.81)
    if config == "species":
        om.set(theta=th, u=12.0, v=-7.0, qcl=_blob)
        hm.set(θ=th, u=12.0, v=-7.0, qcl=_blob)
    else:
        g = om.grid
        x, y, z = g.nodes("ccc")
        rho = om.ref.density[g.Hz:g.Hz + g.Nz][:, None, None]
        a = rho * np.broadcast_to(_blob(x, y, z), (g.Nz, g.Ny, g.Nx))
        b = rho * 0.5 * QMAX * (1.0 + 0.5 * np.sin(2 * np.pi * x / 20e3) * np.cos(2 * np.pi * y / 20e3) + 0 * z)
        om.set(theta=th, u=12.0, v=-7.0, rc0=a, rc1=b)
        hm.tracers["a"].set_interior(a)
        hm.tracers["b"].set_interior(b)
        hm.set(θ=th, u=12.0, v=-7.0)
    for _ in range(3):
        om.time_step(5.0)
        hm.time_step(5.0)
    hm.synchronize()
    fields = hm.prognostic_fields()
    names = {"ru": "ρu", "rv": "ρv", "rw": "ρw", "rtheta": "ρθ", "rq": "ρq", **{k: SCALARS[k][1] for k in CONFIGURATIONS[config]}}
    errs = {}
    for n, k in names.items():
        got, want = fields[k].interior_cpu(), om.grid.interior(getattr(om, n), zface=(n == "rw"))
        errs[n] = float(np.max(np.abs(got - want)) / max(np.max(np.abs(want)), 1e-3))
    print(f"BOUNDED-STEPS {config}:", " ".join(f"{n}={e:.2e}" for n, e in errs.items()))
    assert all(e < 1e-8 for e in errs.values()), errs
    first = CONFIGURATIONS[config][0]
    assert np.max(np.abs(om.grid.interior(getattr(om, first)))) > 1e-3          # above the scale floor: the comparison is relative
