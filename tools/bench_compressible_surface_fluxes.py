#!/usr/bin/env python
"""tools/bench_compressible_surface_fluxes.py — what the bulk surface fluxes cost on the compressible split-explicit model
(csrc/bz_cmp_surface_flux.hip: k_cmp_surface_flux, one launch over the Nx x Ny surface per stage, three per step).

At 256 x 256 x 128 and 512 x 512 x 256, Float64 and Float32, WENO(order = 5), a vapour-carrying model with sheared surface winds:
  kernel   ms per `compressible_surface_fluxes` record of the library's own profile table (HIP-event times around the launch)
  step     ms per time_step with BulkDrag + BulkSensibleHeatFlux + BulkVaporFlux attached and of the same model without boundary
           conditions: the median, the minimum and the spread (max - min) of `--reps` windows of `--steps` steps
The fluxed model is built second in the process, and a model built later in a process steps slower whatever it carries (0.7 ms at
512 x 512 x 256 Float64): read the cost of the fluxes from the kernel line, not from the difference of the two step lines.
`--no-fluxes` measures the flux-free model alone: run on another build of the library (BREEZE_HIP_LIB / BREEZE_HIP_F32_LIB) it gives that
build's flux-free step for comparison.  One JSON line per measurement; no number is fixed in advance.

    python tools/bench_compressible_surface_fluxes.py [--sizes 256x256x128 512x512x256] [--dtypes f64 f32] [--steps 5] [--reps 5]
                                                      [--warmup 1] [--no-fluxes] [--label NAME] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="+", default=["256x256x128", "512x512x256"])
    ap.add_argument("--dtypes", nargs="+", default=["f64", "f32"], choices=["f64", "f32"])
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-fluxes", action="store_true", help="the flux-free model only")
    ap.add_argument("--label", default="this build")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    import torch
    import breeze_jl_amd as bz

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))

    for size in a.sizes:
        Nx, Ny, Nz = (int(n) for n in size.split("x"))
        Lx, Ly, Lz = 100.0 * Nx, 100.0 * Ny, 50.0 * Nz
        dt = 0.25
        theta = lambda x, y, z: 300.0 + 0.002 * z + 0 * x + 0 * y
        qt = lambda x, y, z: 0.010 * np.exp(-z / 2e3) * (1 + 0.2 * np.sin(2 * np.pi * x / Lx)) + 0 * y
        u = lambda x, y, z: 1.5 + 4.0 * np.sin(2 * np.pi * y / Ly + 0.5) + 0 * x + 0 * z
        v = lambda x, y, z: -0.5 + 3.0 * np.cos(2 * np.pi * x / Lx) + 0 * y + 0 * z
        xs, ys = (np.arange(Nx) + 0.5) / Nx, (np.arange(Ny) + 0.5) / Ny
        T0 = 302.5 + np.sin(2 * np.pi * xs)[None, :] * np.cos(2 * np.pi * ys)[:, None]
        for dtype in a.dtypes:
            ft = np.float64 if dtype == "f64" else np.float32

            def emit(**kw):
                line = json.dumps({"tool": "bench_compressible_surface_fluxes", "build": a.label, "grid": [Nx, Ny, Nz], "dtype": dtype, **kw})
                print(line, flush=True)
                if a.out:
                    with open(a.out, "a", encoding="utf-8") as f:
                        f.write(line + "\n")

            for fluxes in ((False,) if a.no_fluxes else (False, True)):
                g = bz.RectilinearGrid((Nx, Ny, Nz), x=(0, Lx), y=(0, Ly), z=(0, Lz), float_type=ft)
                dyn = bz.CompressibleDynamics(bz.SplitExplicitTimeDiscretization(), reference_potential_temperature=300.0)
                bcs = None
                if fluxes:
                    drag = bz.BulkDrag(coefficient=2e-3, gustiness=1.0, surface_temperature=T0)
                    bcs = {"ρu": drag, "ρv": drag, "ρθ": bz.BulkSensibleHeatFlux(coefficient=2e-3, gustiness=1.0, surface_temperature=T0),
                           "ρqᵗ": bz.BulkVaporFlux(coefficient=2e-3, gustiness=1.0, surface_temperature=T0)}
                kw = dict(boundary_conditions=bcs) if fluxes else {}
                m = bz.CompressibleAtmosphereModel(g, dyn, advection=bz.WENO(order=5), **kw)
                rho = m.dynamics.reference_state.density[g.Hz:g.Hz + g.Nz][:, None, None]
                m.set(ρ=rho, θ=theta, qᵗ=qt, u=u, v=v, w=0.0)

                def steps():
                    for _ in range(a.steps):
                        m.time_step(dt)

                med, best, worst = timed(steps)
                emit(what="step", fluxes=fluxes, ms_per_step_median=med / a.steps, ms_per_step_min=best / a.steps,
                     ms_per_step_spread=(worst - best) / a.steps, steps=a.steps, reps=a.reps)
                if fluxes:
                    m.profile_enable(True)
                    m.profile_reset()
                    steps()
                    m.synchronize()
                    prof = m.profile()
                    m.profile_enable(False)
                    ms, calls = prof["compressible_surface_fluxes"]
                    emit(what="kernel", record="compressible_surface_fluxes", ms_per_call=ms / calls, calls=calls, surface_cells=Nx * Ny)
                assert np.isfinite(m.potential_temperature_density.interior_cpu()).all()
                del m
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
