#!/usr/bin/env python
"""tools/bench_surface_layer.py — what the wind- and stability-dependent bulk surface fluxes on a filtered surface state cost.

Two shapes: the configuration of examples/prescribed_sea_surface_temperature.jl (128 x 128 (Periodic, Flat, Bounded), halo 5,
momentum WENO9 / scalars WENO5, warm-phase saturation adjustment) and a 3-D 256 x 256 x 128 variant (WENO5).  Each runs with
(a) constant coefficients and scalar surface temperatures through bz_set_bulk_surface_fluxes, and (b) PolynomialCoefficient +
T0(x) + FilteredSurfaceVelocities through bz_set_surface_layer.  Every step runs under a time limit; one JSON line per (shape, variant)
with the whole-step time (unprofiled) and the profile table of a second pass.

    python tools/bench_surface_layer.py [--shapes example 3d] [--steps 20] [--warmup 3] [--step-limit 20]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np


def build(bz, shape, variant):
    sa = bz.SaturationAdjustment(equilibrium=bz.WarmPhaseEquilibrium())
    if shape == "example":
        grid = bz.RectilinearGrid(size=(128, 128), halo=(5, 5), x=(-10e3, 10e3), z=(0, 10e3), topology=(bz.Periodic, bz.Flat, bz.Bounded))
        adv = dict(momentum_advection=bz.WENO(order=9), scalar_advection=bz.WENO(order=5))
    else:
        grid = bz.RectilinearGrid((256, 256, 128), x=(-10e3, 10e3), y=(-10e3, 10e3), z=(0, 10e3))
        adv = dict(advection=bz.WENO(order=5))
    θ0 = 285
    ref = bz.ReferenceState(grid, surface_pressure=101325, potential_temperature=θ0)
    if variant == "constant":
        c, T0, fv = 1.2e-3, float(θ0 + 2), None
    else:
        c, fv = bz.PolynomialCoefficient(roughness_length=1.5e-4), bz.FilteredSurfaceVelocities(grid, filter_timescale=3600.0)
        T0 = lambda x: θ0 + 2 * np.sign(np.cos(2 * np.pi * x / grid.Lx))
    kw = {} if fv is None else {"filtered_velocities": fv}
    d = bz.BulkDrag(coefficient=c, gustiness=1e-2, surface_temperature=T0, **kw)
    bcs = {"ρu": bz.FieldBoundaryConditions(bottom=d), "ρv": bz.FieldBoundaryConditions(bottom=d),
           "ρe": bz.FieldBoundaryConditions(bottom=bz.BulkSensibleHeatFlux(coefficient=c, gustiness=1e-2, surface_temperature=T0, **kw)),
           "ρqᵉ": bz.FieldBoundaryConditions(bottom=bz.BulkVaporFlux(coefficient=c, gustiness=1e-2, surface_temperature=T0, **kw))}
    m = bz.AtmosphereModel(grid, dynamics=bz.AnelasticDynamics(ref), microphysics=sa, boundary_conditions=bcs, **adv)
    m.set(θ=ref.potential_temperature, u=1)
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["example", "3d"], choices=("example", "3d"))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dt", type=float, default=10.0)
    ap.add_argument("--step-limit", type=float, default=20.0, help="seconds one step may take before the run is abandoned")
    a = ap.parse_args()
    import torch
    import breeze_jl_amd as bz

    def steps(m, n):
        for _ in range(n):
            t0 = time.perf_counter()
            m.time_step(a.dt)
            m.synchronize()
            if time.perf_counter() - t0 > a.step_limit:
                raise SystemExit(f"a step took longer than {a.step_limit} s: abandoned")

    for shape in a.shapes:
        for variant in ("constant", "polynomial+filter"):
            m = build(bz, shape, variant)
            steps(m, a.warmup)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            steps(m, a.steps)
            t1 = time.perf_counter()
            m.profile_enable(True)
            m.profile_reset()
            steps(m, a.steps)
            m.profile_enable(False)
            prof = m.profile()
            g = m.grid
            finite = bool(torch.isfinite(m.velocities["w"].interior).all().item())
            print(json.dumps({"tool": "bench_surface_layer", "shape": shape, "grid": [g.Nx, g.Ny, g.Nz], "variant": variant, "dtype": "f64",
                              "ms_per_step": (t1 - t0) / a.steps * 1e3, "steps": a.steps, "dt": a.dt, "stepping": "one call per step, synchronised",
                              "kernels_ms_per_step": {k: v[0] / a.steps for k, v in sorted(prof.items()) if v[1]},
                              "kernel_launches_per_step": {k: v[1] / a.steps for k, v in sorted(prof.items()) if v[1]}, "finite": finite}), flush=True)
            del m
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
