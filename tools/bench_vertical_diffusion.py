#!/usr/bin/env python
"""tools/bench_vertical_diffusion.py — what closure = ScalarDiffusivity(VerticallyImplicitTimeDiscretization(), ν, κ) costs
(csrc/bz_diffusivity.hip).

At 256 x 256 x 128 and 512 x 512 x 256, Float64 and Float32, with ν and κ numbers ("constant") and centre fields ("field"); the model is
the WENO(order = 5) θ model with moisture and one tracer, so the stage's implicit launch solves F = 6 fields (ρu, ρv, ρw, ρθ, ρq, ρc):
  implicit   ms per implicit launch of a stage (the library's own profile record `implicit_step`, three launches per step; the constant
             form includes its one-block table prologue), the compulsory bytes of a launch — 2 words per cell and field (the field read
             and written once) plus one read of each K field per launch when field-valued — and that as a fraction of the 8 TB/s HBM
             roofline.  (The kernel moves more: the modified right-hand side goes through the field in place, 4 words per cell and
             field, and the field form reads its K once per field class.)
  step       ms per time_step with the closure and without it (time_steps(Δt, n) between two events, median over `--reps` windows)
One JSON line per measurement; no number is fixed in advance.

    python tools/bench_vertical_diffusion.py [--sizes 256x256x128 512x512x256] [--dtypes f64 f32] [--steps 5] [--reps 5] [--warmup 2]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np

ROOFLINE = 8e12      # bytes / s
FIELDS = 6           # ρu, ρv, ρw, ρθ, ρq, one tracer


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="+", default=["256x256x128", "512x512x256"])
    ap.add_argument("--dtypes", nargs="+", default=["f64", "f32"], choices=["f64", "f32"])
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
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
        dt = 2.0
        theta = lambda x, y, z: 300.0 + 4e-3 * z + np.sin(2 * np.pi * x / Lx) + 0 * y
        qv = lambda x, y, z: 0.01 * np.exp(-z / 2.5e3) * (1.0 + 0.2 * np.cos(2 * np.pi * y / Ly)) + 0 * x
        tracer = lambda x, y, z: 1.0 + 0.5 * np.sin(2 * np.pi * x / Lx) * np.cos(2 * np.pi * y / Ly) * np.exp(-z / 4e3)
        Kfun = lambda x, y, z: 20.0 * np.exp(-z / 1.5e3) * (1.0 + 0.5 * np.sin(2 * np.pi * x / Lx) * np.cos(2 * np.pi * y / Ly))
        for dtype in a.dtypes:
            word = 8 if dtype == "f64" else 4
            ft = np.float64 if dtype == "f64" else np.float32

            def emit(**kw):
                print(json.dumps({"tool": "bench_vertical_diffusion", "grid": [Nx, Ny, Nz], "dtype": dtype, "fields": FIELDS, **kw}), flush=True)

            for kind in ("none", "constant", "field"):
                g = bz.RectilinearGrid((Nx, Ny, Nz), x=(0, Lx), y=(0, Ly), z=(0, Lz), float_type=ft)
                closure, nK = None, 0
                if kind == "constant":
                    closure = bz.ScalarDiffusivity(bz.VerticallyImplicitTimeDiscretization(), ν=10.0, κ=15.0)
                elif kind == "field":
                    Ks = [bz.Field(g, (bz.Center, bz.Center, bz.Center), "cuda:0") for _ in range(2)]
                    for K in Ks:
                        K.set_interior(Kfun)
                    closure, nK = bz.ScalarDiffusivity(bz.VerticallyImplicitTimeDiscretization(), ν=Ks[0], κ=Ks[1]), 2
                try:
                    m = bz.AtmosphereModel(g, dynamics=bz.AnelasticDynamics(bz.ReferenceState(g, potential_temperature=300.0)),
                                           advection=bz.WENO(order=5), closure=closure, tracers=("c",))
                except bz.BreezeHIPError as e:
                    emit(what="refused", closure=kind, message=str(e))
                    continue
                m.tracers["c"].set_interior(tracer)
                m.set(θ=theta, qᵗ=qv, u=3.0)
                med, best = timed(lambda: m.time_steps(dt, a.steps))
                emit(what="step", closure=kind, ms_per_step_median=med / a.steps, ms_per_step_min=best / a.steps, steps=a.steps, reps=a.reps)
                if closure is not None:
                    m.profile_enable(True)
                    m.profile_reset()
                    m.time_steps(dt, a.steps)
                    m.synchronize()
                    prof = m.profile()
                    m.profile_enable(False)
                    ms, launches = prof["implicit_step"]
                    nbytes = word * (2 * FIELDS + nK) * cells
                    emit(what="implicit", closure=kind, ms_per_launch=ms / launches, launches=launches, words_per_cell=2 * FIELDS + nK, bytes=nbytes,
                         roofline_fraction=nbytes / (ms / launches * 1e-3) / ROOFLINE,
                         explicit_remainder_ms_per_stage=prof.get("diffusivity_tendencies", (0.0, 1))[0] / max(prof.get("diffusivity_tendencies", (0.0, 1))[1], 1))
                assert np.isfinite(m.potential_temperature_density.interior_cpu()).all()
                del m
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
