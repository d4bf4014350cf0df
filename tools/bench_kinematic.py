#!/usr/bin/env python
"""tools/bench_kinematic.py — what a step of AtmosphereModel(dynamics = PrescribedDynamics(...)) costs (csrc/bz_kinematic.hip).

At 256 x 256 x 128 (default), Float64, θ, qᵛ and two tracers (S = 4 scalars), with the divergence correction off and on:
  step             ms per time_step (time_steps(Δt, n) between two events, median over `--reps` windows)
  stage            ms per launch of k_kin_scalar_stage (the library's own profile records, three launches per step), the compulsory bytes of
                   a launch — (4 + 4 S) words per cell with the correction (u, v, w, D read once; per scalar c read, ρc read and written,
                   U0 read or, in stage 1, written), (3 + 4 S) without — and that as a fraction of the 8 TB/s HBM roofline
and, for comparison at the same grid and scalar count,
  anelastic        ms per step of the anelastic model (momentum, pressure solve and the same scalars)
  scalar_tendency  S separate bz_compute_scalar_tendency launches (one tendency evaluation per scalar, no RK update)
One JSON line per measurement.

    python tools/bench_kinematic.py [--size 256 256 128] [--steps 10] [--reps 5] [--warmup 2]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np

ROOFLINE = 8e12      # bytes / s
TRACERS = ("a", "b")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, nargs=3, default=[256, 256, 128])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    import torch
    import breeze_jl_amd as bz

    Nx, Ny, Nz = a.size
    Lx, Ly, Lz = 100.0 * Nx, 100.0 * Ny, 12e3
    cells, S = Nx * Ny * Nz, 2 + len(TRACERS)
    dt = 2.0
    u = lambda x, y, z: 3.0 + 4.0 * np.sin(2 * np.pi * x / Lx) * np.cos(2 * np.pi * y / Ly) + 0 * z
    v = lambda x, y, z: -2.0 + 3.0 * np.cos(2 * np.pi * x / Lx) * np.sin(2 * np.pi * y / Ly) + 0 * z
    w = lambda x, y, z: 2.0 * np.sin(np.pi * z / Lz) * (1.0 + 0.5 * np.cos(2 * np.pi * x / Lx)) + 0 * y
    theta = lambda x, y, z: 300.0 + 4e-3 * z + np.sin(2 * np.pi * x / Lx) + 0 * y
    qv = lambda x, y, z: 0.01 * np.exp(-z / 2.5e3) * (1.0 + 0.2 * np.cos(2 * np.pi * y / Ly)) + 0 * x
    tracer = lambda x, y, z: 1.0 + 0.5 * np.sin(2 * np.pi * x / Lx) * np.cos(2 * np.pi * y / Ly) * np.exp(-z / 4e3)

    def grid():
        return bz.RectilinearGrid((Nx, Ny, Nz), x=(0, Lx), y=(0, Ly), z=(0, Lz))

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

    def emit(**kw):
        print(json.dumps({"tool": "bench_kinematic", "grid": [Nx, Ny, Nz], "dtype": "f64", "scalars": S, **kw}), flush=True)

    for correction in (False, True):
        g = grid()
        m = bz.AtmosphereModel(g, dynamics=bz.PrescribedDynamics(bz.ReferenceState(g, potential_temperature=300.0), divergence_correction=correction),
                               advection=bz.WENO(order=5), tracers=TRACERS)
        m.set(θ=theta, qᵗ=qv, u=u, v=v, w=w, **{n: tracer for n in TRACERS})      # (a tracer keyword sets its density field)
        med, best = timed(lambda: m.time_steps(dt, a.steps))
        emit(what="step", correction=correction, ms_per_step_median=med / a.steps, ms_per_step_min=best / a.steps, steps=a.steps, reps=a.reps)
        m.profile_enable(True)
        m.profile_reset()
        m.time_steps(dt, a.steps)
        m.synchronize()
        prof = m.profile()
        m.profile_enable(False)
        ms, launches = prof["kinematic_scalar_stage"]
        words = (4 if correction else 3) + 4 * S
        nbytes = 8 * words * cells
        emit(what="stage", correction=correction, ms_per_launch=ms / launches, launches=launches, words_per_cell=words, bytes=nbytes,
             roofline_fraction=nbytes / (ms / launches * 1e-3) / ROOFLINE,
             profile={k: [t, n] for k, (t, n) in prof.items()})
        assert np.isfinite(m.potential_temperature_density.interior_cpu()).all()
        del m
        torch.cuda.empty_cache()

    # the anelastic model at the same grid and scalar count
    g = grid()
    m = bz.AtmosphereModel(g, dynamics=bz.AnelasticDynamics(bz.ReferenceState(g, potential_temperature=300.0)), advection=bz.WENO(order=5),
                           tracers=TRACERS)
    for n in TRACERS:
        m.tracers[n].set_interior(tracer)
    m.set(θ=theta, qᵗ=qv, u=u, v=v, w=w)
    med, best = timed(lambda: m.time_steps(dt, a.steps))
    emit(what="anelastic", ms_per_step_median=med / a.steps, ms_per_step_min=best / a.steps, steps=a.steps, reps=a.reps)
    # S separate scalar_tendency launches (per stage the fused kernel replaces them and the RK updates)
    fields = [m.potential_temperature, m.specific_moisture] + [m.specific_tracers[n] for n in TRACERS]
    outs = [m.G["ρθ"], m.G["ρq"]] + [m.G[n] for n in TRACERS]
    m.refresh_diagnostics()
    med, best = timed(lambda: [bz.compute_scalar_tendency_(m, c, G) for c, G in zip(fields, outs)])
    emit(what="scalar_tendency", launches=S, ms_median=med, ms_min=best, reps=a.reps)


if __name__ == "__main__":
    main()
