#!/usr/bin/env python
"""tools/bench_compressible_closure.py — what a turbulence closure costs on the compressible split-explicit model
(csrc/bz_closure.hip, csrc/bz_diffusivity.hip: the carrier-templated kernels; the z-marching LDS-tiled pair on these whole-tile grids,
the cell-per-thread pair with BZ_NO_CLOSURE_MARCH=1).

At 256 x 256 x 128 and 512 x 512 x 256, Float64 and Float32, WENO(order = 5) with 1 % vapour, for closure = None, SmagorinskyLilly(),
ScalarDiffusivity(ν, κ) numbers and VerticalScalarDiffusivity(ν, κ) centre fields:
  step     ms per time_step (a window of `--steps` steps between two events, median over `--reps` windows)
  kernel   for every closure record of the library's own profile table (HIP-event times): ms per call, the compulsory words per cell of
           the call — each array read or written once — and those as a fraction of the 8 TB/s HBM roofline:
             smagorinsky_march | _viscosity   u, v, w, T, q^v, p read, nu_e written                                   7   (anelastic: 6, no p)
             closure_march | _tendencies      u, v, w, nu_e, theta, rho_d read, four tendencies read and written     14   (anelastic: 16, with q)
             water_closure_tendencies   rho, nu_e | kappa, q read, one tendency read and written                5   (kappa a number: 4)
             diffusivity_tendencies     u, v, w, rho_d [, nu] + three tendencies; theta, rho_d [, kappa] + one  16 numbers, 18 fields
One JSON line per measurement; no number is fixed in advance.

    python tools/bench_compressible_closure.py [--sizes 256x256x128 512x512x256] [--dtypes f64 f32] [--steps 3] [--reps 3] [--warmup 1] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np

ROOFLINE = 8e12      # bytes / s
WORDS = {"smagorinsky_viscosity": {"smagorinsky": 7}, "closure_tendencies": {"smagorinsky": 14},      # ragged grids, BZ_NO_CLOSURE_MARCH=1
         "smagorinsky_march": {"smagorinsky": 7}, "closure_march": {"smagorinsky": 14},                   # whole 64 x 8 tiles
         "water_closure_tendencies": {"smagorinsky": 5, "numbers": 4, "vertical fields": 5},
         "diffusivity_tendencies": {"numbers": 16, "vertical fields": 18}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="+", default=["256x256x128", "512x512x256"])
    ap.add_argument("--dtypes", nargs="+", default=["f64", "f32"], choices=["f64", "f32"])
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
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
        return float(np.median(ms)), float(np.min(ms))

    for size in a.sizes:
        Nx, Ny, Nz = (int(n) for n in size.split("x"))
        Lx, Ly, Lz = 100.0 * Nx, 100.0 * Ny, 12e3
        cells = Nx * Ny * Nz
        dt = 0.5
        theta = lambda x, y, z: 300.0 + 4e-3 * z + np.sin(2 * np.pi * x / Lx) + 0 * y
        qv = lambda x, y, z: 0.01 * np.exp(-z / 2.5e3) * (1.0 + 0.2 * np.cos(2 * np.pi * y / Ly)) + 0 * x
        u = lambda x, y, z: 3.0 + np.sin(2 * np.pi * y / Ly) * np.cos(2 * np.pi * z / Lz) + 0 * x
        Kfun = lambda x, y, z: 20.0 * np.exp(-z / 1.5e3) * (1.0 + 0.5 * np.sin(2 * np.pi * x / Lx) * np.cos(2 * np.pi * y / Ly))
        for dtype in a.dtypes:
            word = 8 if dtype == "f64" else 4
            ft = np.float64 if dtype == "f64" else np.float32

            def emit(**kw):
                line = json.dumps({"tool": "bench_compressible_closure", "grid": [Nx, Ny, Nz], "dtype": dtype, **kw})
                print(line, flush=True)
                if a.out:
                    with open(a.out, "a", encoding="utf-8") as f:
                        f.write(line + "\n")

            for kind in ("none", "smagorinsky", "numbers", "vertical fields"):
                g = bz.RectilinearGrid((Nx, Ny, Nz), x=(0, Lx), y=(0, Ly), z=(0, Lz), float_type=ft)
                closure = None
                if kind == "smagorinsky":
                    closure = bz.SmagorinskyLilly()
                elif kind == "numbers":
                    closure = bz.ScalarDiffusivity(ν=10.0, κ=15.0)
                elif kind == "vertical fields":
                    Ks = [bz.Field(g, (bz.Center, bz.Center, bz.Center), "cuda:0") for _ in range(2)]
                    for K in Ks:
                        K.set_interior(Kfun)
                    closure = bz.VerticalScalarDiffusivity(ν=Ks[0], κ=Ks[1])
                dyn = bz.CompressibleDynamics(bz.SplitExplicitTimeDiscretization(), reference_potential_temperature=300.0)
                m = bz.CompressibleAtmosphereModel(g, dyn, advection=bz.WENO(order=5), closure=closure)
                rho = m.dynamics.reference_state.density[g.Hz:g.Hz + g.Nz][:, None, None]
                m.set(ρ=rho, θ=theta, qᵗ=qv, u=u, v=0.0, w=0.0)

                def steps():
                    for _ in range(a.steps):
                        m.time_step(dt)

                med, best = timed(steps)
                emit(what="step", closure=kind, ms_per_step_median=med / a.steps, ms_per_step_min=best / a.steps, steps=a.steps, reps=a.reps)
                if closure is not None:
                    m.profile_enable(True)
                    m.profile_reset()
                    steps()
                    m.synchronize()
                    prof = m.profile()
                    m.profile_enable(False)
                    for name, words in WORDS.items():
                        if name in prof and kind in words:
                            ms, calls = prof[name]
                            nbytes = word * words[kind] * cells
                            emit(what="kernel", closure=kind, record=name, ms_per_call=ms / calls, calls=calls, words_per_cell=words[kind],
                                 bytes=nbytes, roofline_fraction=nbytes / (ms / calls * 1e-3) / ROOFLINE)
                assert np.isfinite(m.potential_temperature_density.interior_cpu()).all()
                del m
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
