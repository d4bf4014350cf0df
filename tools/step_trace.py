#!/usr/bin/env python
"""tools/step_trace.py [--compressible] [--out FILE] [--only NAME ...] — which kernels a whole anelastic step launches, and the bits it
leaves, for every tier of bz_time_step_anelastic (csrc/bz_step.hip: bzi_anelastic_tier) and of the slab drivers (csrc/bz_comm.hip).

One process.  Each configuration below creates its model with profiling on and runs one time_step ("first"), then
time_steps(dt, 2, diagnose_last=False) followed by one time_step ("then").  After each of the two phases the output holds the profile
(record name -> launches, in first-appearance order) and a SHA-256 of the interior of every prognostic and diagnostic field.  Two builds
whose outputs are equal launch the same records in the same order and compute the same bits; DESIGN §4 "which tier runs where" is
checked against the record names (profiles/step_trace_*.json).  Small grids only: 32x16x16, 64x32x16 for the CBL stack.

--compressible runs the other group instead (a process of its own): the components of the compressible split-explicit model at 32x16x16,
three time_steps each, with the profile and the digests after the first and after the third (profiles/step_trace_compressible*.json)."""
import argparse
import hashlib
import json
import os
import sys
import threading
import uuid

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

EXT = dict(x=(-10e3, 10e3), y=(-10e3, 10e3), z=(0.0, 10e3))
BOMEX_EXT = dict(x=(-3.2e3, 3.2e3), y=(-2e3, 2e3), z=(0.0, 3e3))
F0, RHO0, USTAR = 3.76e-5, 1.15, 0.28


def bubble(x, y, z):
    r = np.sqrt(x ** 2 + (y - 1500.0) ** 2 + (z - 3000.0) ** 2)
    return 300.0 * np.exp(1e-6 * z / 9.81) + 10.0 * np.maximum(0.0, 1.0 - r / 2.5e3)


def vapour(x, y, z):
    return 6e-3 * np.exp(-z / 2500.0) * (1.0 + 0.3 * np.sin(2 * np.pi * y / 20e3)) + 0 * x


def anelastic(bz, size=(32, 16, 16), order=5, halo=None, topology=None, theta0=300.0, surface_pressure=101325, ext=EXT, **kw):
    gkw = dict(ext)
    if topology is not None:
        gkw["topology"] = topology
        if topology[1] == bz.Flat:
            gkw.pop("y")
    if halo is not None:
        gkw["halo"] = halo
    grid = bz.RectilinearGrid(size, **gkw)
    ref = bz.ReferenceState(grid, surface_pressure=surface_pressure, potential_temperature=theta0)
    return bz.AtmosphereModel(grid, dynamics=bz.AnelasticDynamics(ref), advection=bz.WENO(order=order), **kw)


def dry_bubble(bz, **kw):
    m = anelastic(bz, **kw)
    m.set(θ=bubble, u=3.0, v=-2.0)
    return m


def moist_bubble(bz, **kw):
    m = anelastic(bz, **kw)
    m.set(θ=bubble, u=3.0, v=-2.0, qᵗ=vapour)
    return m


def saturated_bubble(bz, **kw):
    m = anelastic(bz, **kw)
    m.set(θ=bubble, u=1.0, qᵗ=0.012)
    return m


def kessler_bubble(bz, **kw):
    tc = bz.ThermodynamicConstants(saturation_vapor_pressure=bz.TetensFormula())
    m = anelastic(bz, thermodynamic_constants=tc, microphysics=bz.DCMIP2016KesslerMicrophysics(), **kw)
    m.set(θ=bubble, u=1.0, qᵗ=0.012)
    return m


def flat_bubble(bz, topology):
    m = anelastic(bz, size=(32, 16), topology=topology)
    m.set(θ=lambda x, z: bubble(x, 1500.0 + 0 * x, z))
    return m


def cbl(bz, **kw):
    from breeze_jl_amd import benchmarks
    return benchmarks.convective_boundary_layer(size=(64, 32, 16), float_type=np.float64, advection=bz.WENO(order=5), **kw)


def bomex_kwargs(bz):
    """the forcing / Coriolis / bottom-flux stack of examples/bomex.jl (Siebesma et al. 2003, appendix B)"""
    ws = lambda z: -6.5e-3 * z / 1500.0 if z <= 1500.0 else (-6.5e-3 * (1 - (z - 1500.0) / 600.0) if z <= 2100.0 else 0.0)
    drying = lambda z: -1.2e-8 if z <= 300.0 else (-1.2e-8 * (1 - (z - 300.0) / 200.0) if z <= 500.0 else 0.0)
    cooling = lambda z: 1005.0 * (-2.0 / 86400.0 if z <= 1500.0 else (-2.0 / 86400.0 * (1 - (z - 1500.0) / 1500.0) if z <= 3000.0 else 0.0))
    subsidence = bz.SubsidenceForcing(ws)
    geo = bz.geostrophic_forcings(lambda z: -10.0 + 1.8e-3 * z, lambda z: 0.0)
    drag = bz.FieldBoundaryConditions(bottom=bz.FluxBoundaryCondition(bz.FrictionVelocityDrag(RHO0, USTAR)))
    return dict(coriolis=bz.FPlane(f=F0),
                forcing={"u": (subsidence, geo.u), "v": (subsidence, geo.v), "θ": subsidence, "qᵉ": (subsidence, bz.Forcing(drying)),
                         "e": bz.Forcing(cooling)},
                boundary_conditions={"ρθ": bz.FieldBoundaryConditions(bottom=bz.FluxBoundaryCondition(RHO0 * 8e-3)),
                                     "ρqᵉ": bz.FieldBoundaryConditions(bottom=bz.FluxBoundaryCondition(RHO0 * 5.2e-5)), "ρu": drag, "ρv": drag})


def bomex(bz):
    m = anelastic(bz, size=(32, 16, 16), theta0=299.1, surface_pressure=101500.0, ext=BOMEX_EXT, closure=bz.SmagorinskyLilly(),
                  microphysics=bz.SaturationAdjustment(equilibrium=bz.WarmPhaseEquilibrium()), **bomex_kwargs(bz))
    rng = np.random.default_rng(2)
    m.set(θ=299.1 + 0.3 * rng.standard_normal((16, 16, 32)), qᵗ=0.016 + 1e-3 * rng.standard_normal((16, 16, 32)), u=-6.0)
    return m


def with_tracers(bz):
    m = anelastic(bz, tracers=("a", "b"))
    rng = np.random.default_rng(5)
    for t in m.tracers.values():
        t.set_interior(1.0 + 0.1 * rng.standard_normal((16, 16, 32)))
    m.set(θ=bubble, u=3.0, v=-2.0)
    return m


def sponge(bz):
    m = anelastic(bz, forcing={"ρw": bz.Relaxation(rate=0.01, mask=bz.GaussianMask(9e3, 1e3), target=0.0)})
    m.set(θ=bubble, u=3.0, v=-2.0)
    return m


def sat(bz):
    return bz.SaturationAdjustment(equilibrium=bz.WarmPhaseEquilibrium())


# name -> (environment of the context, model factory, dt)
def single_device_cases(bz):
    PBB, PFB, BFB = (bz.Periodic, bz.Bounded, bz.Bounded), (bz.Periodic, bz.Flat, bz.Bounded), (bz.Bounded, bz.Flat, bz.Bounded)
    return {
        # lean tier
        "lean/dry_bubble": ({}, lambda: dry_bubble(bz), 2.0),
        "lean/vapour": ({}, lambda: moist_bubble(bz), 2.0),
        "lean/no_xfft": ({"BZ_NO_XFFT": "1"}, lambda: dry_bubble(bz), 2.0),
        "lean/cbl_forcing_stack": ({}, lambda: cbl(bz), 0.05),
        "lean/walls_in_y": ({}, lambda: dry_bubble(bz, topology=PBB), 2.0),
        "lean/cbl_walls_in_y": ({}, lambda: cbl(bz, topology=PBB), 0.05),
        # fused-RK tier
        "fused_rk/no_lean": ({"BZ_NO_LEAN": "1"}, lambda: dry_bubble(bz), 2.0),
        "fused_rk/saturation_adjustment": ({}, lambda: saturated_bubble(bz, microphysics=sat(bz)), 2.0),
        "fused_rk/bomex_stack": ({}, lambda: bomex(bz), 3.0),
        "fused_rk/bomex_stack_no_fold_forcing": ({"BZ_NO_FOLD_FORCING": "1"}, lambda: bomex(bz), 3.0),
        "fused_rk/tracers": ({}, lambda: with_tracers(bz), 2.0),
        "fused_rk/weno9": ({}, lambda: dry_bubble(bz, order=9, halo=(5, 5, 5)), 2.0),
        "fused_rk/weno9_walls_in_y": ({}, lambda: dry_bubble(bz, order=9, halo=(5, 5, 5), topology=PBB), 2.0),
        # fused tier
        "fused/no_fuse_rk": ({"BZ_NO_FUSE_RK": "1"}, lambda: dry_bubble(bz), 2.0),
        "fused/kessler": ({}, lambda: kessler_bubble(bz), 2.0),
        "fused/static_energy": ({}, lambda: dry_bubble(bz, formulation="StaticEnergy"), 2.0),
        "fused/sponge": ({}, lambda: sponge(bz), 2.0),
        "fused/bomex_stack_no_fuse_forcing": ({"BZ_NO_FUSE_FORCING": "1"}, lambda: bomex(bz), 3.0),
        # operators tier
        "operators/no_fused": ({"BZ_NO_FUSED": "1"}, lambda: dry_bubble(bz), 2.0),
        "operators/flat_y": ({}, lambda: flat_bubble(bz, PFB), 2.0),
        "operators/walls_in_x": ({}, lambda: flat_bubble(bz, BFB), 2.0),
        "operators/walls_in_y_no_lean": ({"BZ_NO_LEAN": "1"}, lambda: dry_bubble(bz, topology=PBB), 2.0),
    }


# two thread ranks on one GPU through the local transport: name -> (environment, model keywords, set keywords)
def slab_cases(bz):
    tc = bz.ThermodynamicConstants(saturation_vapor_pressure=bz.TetensFormula())
    return {
        "slab/lean": ({}, {}, dict(θ=bubble, u=3.0, v=-2.0, qᵗ=vapour)),
        "slab/lean_with_no_lean_set": ({"BZ_NO_LEAN": "1"}, {}, dict(θ=bubble, u=3.0, v=-2.0, qᵗ=vapour)),      # the switch is not consulted on slabs
        "slab/saturation_adjustment": ({}, dict(microphysics=sat(bz)), dict(θ=bubble, u=1.0, qᵗ=0.012)),
        "slab/kessler": ({}, dict(microphysics=bz.DCMIP2016KesslerMicrophysics(), thermodynamic_constants=tc), dict(θ=bubble, u=1.0, qᵗ=0.012)),
    }


# ---- the compressible group: name -> (environment, model factory, dt) ----
CEXT = dict(x=(0.0, 8e3), y=(0.0, 4e3), z=(0.0, 4e3))


def cbubble(x, y, z):
    return np.maximum(0.0, 1.0 - np.sqrt((x - 4e3) ** 2 + (y - 2e3) ** 2 + (z - 1500.0) ** 2) / 1200.0)


def ctheta(x, y, z):
    return 300.0 + 0.004 * z + cbubble(x, y, z)


def cvapour(x, y, z):
    return 0.014 * np.exp(-z / 3000.0) + 0.004 * cbubble(x, y, z)


def compressible(bz, topology=None, moist=False, slab=False, make_kw=None, sets=None, **kw):
    gkw = dict(CEXT)
    if topology is not None:
        gkw["topology"] = topology
    flat = topology is not None and topology[1] == bz.Flat
    if flat:
        gkw.pop("y")
    grid = bz.RectilinearGrid((32, 16) if flat else (32, 16, 16), **gkw)
    dyn = bz.CompressibleDynamics(bz.SplitExplicitTimeDiscretization(substeps=6), surface_pressure=1e5, reference_potential_temperature=300.0)
    if make_kw is not None:
        kw.update(make_kw(grid))
    if slab:
        m = bz.compressible.SlabCompressibleModel(grid, 0, 1, dyn, advection=bz.WENO(order=5), transport="local:" + uuid.uuid4().hex,
                                                  device="cuda:0", **kw)
    else:
        m = bz.CompressibleAtmosphereModel(grid, dyn, advection=bz.WENO(order=5), **kw)
    ref = m.dynamics.reference_state
    ρ = ref.density[grid.Hz:grid.Hz + grid.Nz][:, None, None]
    two = (lambda f: (lambda x, z: f(x, 2e3 + 0 * x, z))) if flat else (lambda f: f)
    state = dict(ρ=ρ, θ=two(ctheta), u=3.0, v=0.0 if topology is not None else -2.0, w=0.0)
    if moist:
        state["qᵗ"] = two(cvapour)
    state.update(sets or {})
    m.set(**state)
    return m


def nu_field(bz):
    def make(grid):
        ν = bz.Field(grid, (bz.Center, bz.Center, bz.Center), "cuda:0")
        ν.set_interior(lambda x, y, z: 5.0 + 3.0 * np.sin(2 * np.pi * x / 8e3) * np.cos(2 * np.pi * y / 4e3) + 1e-3 * z)
        return dict(closure=bz.ScalarDiffusivity(ν=ν, κ=8.0))
    return make


def compressible_cases(bz):
    tc = bz.ThermodynamicConstants(saturation_vapor_pressure=bz.TetensFormula())
    PBB, PFB = (bz.Periodic, bz.Bounded, bz.Bounded), (bz.Periodic, bz.Flat, bz.Bounded)
    forced = dict(coriolis=bz.FPlane(f=1e-4),
                  forcing={"ρw": bz.Relaxation(rate=0.01, mask=bz.GaussianMask(3.5e3, 5e2), target=0.0),
                           "θ": bz.Forcing(lambda x, y, z: 1e-3 * cbubble(x, y, z))})
    return {
        "compressible/dry": ({}, lambda: compressible(bz), 2.0),
        "compressible/saturation_adjustment": ({}, lambda: compressible(bz, moist=True, microphysics=sat(bz)), 2.0),
        "compressible/kessler": ({}, lambda: compressible(bz, moist=True, thermodynamic_constants=tc, microphysics=bz.DCMIP2016KesslerMicrophysics(),
                                                          sets=dict(qcl=lambda x, y, z: 0.003 * cbubble(x, y, z),
                                                                    qr=lambda x, y, z: 0.001 * cbubble(x, y, z))), 2.0),
        "compressible/smagorinsky_lilly": ({}, lambda: compressible(bz, closure=bz.SmagorinskyLilly()), 2.0),
        "compressible/scalar_diffusivity_nu_field": ({}, lambda: compressible(bz, make_kw=nu_field(bz)), 2.0),
        "compressible/fplane_sponge_field_forcing": ({}, lambda: compressible(bz, **forced), 2.0),
        "compressible/walls_in_y": ({}, lambda: compressible(bz, topology=PBB), 2.0),
        "compressible/flat_y": ({}, lambda: compressible(bz, topology=PFB), 2.0),
        "compressible/substep_float32": ({}, lambda: compressible(bz, substep_floattype=np.float32), 2.0),
        "compressible/slab_local_world1": ({}, lambda: compressible(bz, slab=True), 2.0),
    }


def compressible_fields_of(m):
    f = dict(m.prognostic_fields())
    f.update({"u": m.velocities["u"], "v": m.velocities["v"], "w": m.velocities["w"], "θ": m.potential_temperature, "q": m.specific_moisture,
              "T": m.temperature, "ρ": m.dynamics.total_density, "p": m.dynamics.pressure})
    f.update({k: v for k, v in m.microphysical_fields.items() if hasattr(v, "interior_cpu") and k not in f})
    f.update(m.closure_fields)
    return f


def trace_compressible(m, dt):
    m.profile_enable(True)
    m.time_step(dt)
    first = snapshot(m, compressible_fields_of)
    m.time_step(dt)
    m.time_step(dt)
    return {"first": first, "then": snapshot(m, compressible_fields_of)}


def fields_of(m):
    f = dict(m.prognostic_fields())
    f.update({"u": m.velocities["u"], "v": m.velocities["v"], "w": m.velocities["w"], "θ": m.potential_temperature, "q": m.specific_moisture,
              "T": m.temperature, "ϕ": m.dynamics.pressure_anomaly})
    return f


def snapshot(m, fields=None):
    m.synchronize()
    digests = {k: hashlib.sha256(np.ascontiguousarray(f.interior_cpu()).tobytes()).hexdigest() for k, f in (fields or fields_of)(m).items()}
    return {"profile": [[name, n] for name, (_, n) in m.profile().items()], "sha256": digests}


def trace(m, dt):
    m.profile_enable(True)
    m.time_step(dt)
    first = snapshot(m)
    m.time_steps(dt, 2, diagnose_last=False)
    m.time_step(dt)
    return {"first": first, "then": snapshot(m)}


class environment:
    def __init__(self, env):
        self.env = env

    def __enter__(self):
        self.saved = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def run_slabs(bz, model_kw, set_kw, dt, world=2):
    import torch
    from breeze_jl_amd import distributed
    G = bz.RectilinearGrid((32, 32, 16), **EXT)
    group = "local:" + uuid.uuid4().hex
    out, errors = [None] * world, []

    def rank_main(rank):
        try:
            torch.cuda.set_device(0)
            with torch.cuda.stream(torch.cuda.Stream()):
                m = distributed.LibrarySlabAtmosphereModel(G, rank, world, transport=group, potential_temperature=300.0, advection=bz.WENO(order=5),
                                                           device="cuda:0", **model_kw)
                m.set(**set_kw)
                out[rank] = trace(m, dt)
        except Exception as e:      # noqa: BLE001
            errors.append(f"rank {rank}: {e!r}")

    threads = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    if errors:
        raise RuntimeError("; ".join(errors))
    return {f"rank{r}": o for r, o in enumerate(out)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None, help="write the JSON here (default: standard output)")
    ap.add_argument("--only", nargs="*", default=None, help="configuration names (default: all)")
    ap.add_argument("--compressible", action="store_true", help="the compressible group instead of the anelastic and slab configurations")
    a = ap.parse_args()
    import breeze_jl_amd as bz
    result = {}
    if a.compressible:
        todo = [(name, env, lambda make=make, dt=dt: trace_compressible(make(), dt)) for name, (env, make, dt) in compressible_cases(bz).items()]
    else:
        todo = [(name, env, lambda make=make, dt=dt: trace(make(), dt)) for name, (env, make, dt) in single_device_cases(bz).items()]
        todo += [(name, env, lambda mkw=mkw, skw=skw: run_slabs(bz, mkw, skw, 2.0)) for name, (env, mkw, skw) in slab_cases(bz).items()]
    try:
        for name, env, run in todo:
            if a.only and name not in a.only:
                continue
            with environment(env):
                try:
                    result[name] = run()
                except (TypeError, ValueError, KeyError, AttributeError, NotImplementedError) as e:      # the host API refused the configuration
                    result[name] = {"refused": repr(e)}
            print(name, "refused" if "refused" in result[name] else "ok", file=sys.stderr, flush=True)
    finally:      # a library error ends the run there (nothing more is started on the device); what ran is still written
        write(result, a.out)


def write(result, out):
    text = json.dumps(result, indent=1, ensure_ascii=False, sort_keys=False)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w", encoding="utf-8") as f:
            f.write(text + "\n")
    else:
        print(text)


if __name__ == "__main__":
    main()
