#!/usr/bin/env python
"""tools/bench_balanced_set.py — what set!(model; ρ = HydrostaticallyBalancedDensity(p₀)) costs on the device (csrc/bz_balance.hip).

At 256 x 256 x 128 and 512 x 512 x 256, Float64 and Float32 (the twin library), a vapour-carrying compressible model, WENO(order = 5):
  balanced_set   ms per bz_set_hydrostatically_balanced_density call (median over `--reps` calls between two events; the call re-balances
                 the state it left, which is the same work)
  kernels        ms per launch of k_exner_columns, k_rescale_density_weighted (two launches per call), k_dry_from_total and of the halo fill
                 and update_state! that close the call (the library's own profile records); for k_exner_columns the pow() evaluations per
                 second (8 per level and column above the first) — the kernel is pow-bound — and for the two streaming kernels the
                 compulsory bytes against the 8 TB/s HBM roofline
  step           ms per time_step of the same model, for scale
One JSON line per measurement.  Reporting, not a gate.

    python tools/bench_balanced_set.py [--sizes 256x256x128 512x512x256] [--reps 5] [--warmup 2]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np

ROOFLINE = 8e12      # bytes / s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="+", default=["256x256x128", "512x512x256"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    import torch
    import breeze_jl_amd as bz
    from breeze_jl_amd.compressible import set_hydrostatically_balanced_density_

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
        theta = lambda x, y, z: 300.0 + 4e-3 * z + np.sin(2 * np.pi * x / Lx) * np.cos(2 * np.pi * y / Ly)
        qv = lambda x, y, z: 0.012 * np.exp(-z / 2.5e3) * (1.0 + 0.2 * np.cos(2 * np.pi * y / Ly)) + 0 * x
        u = lambda x, y, z: 5.0 + 2.0 * np.sin(2 * np.pi * y / Ly) + 0 * x + 0 * z
        for float_type, name in ((np.float64, "f64"), (np.float32, "f32")):
            word = np.dtype(float_type).itemsize

            def emit(**kw):
                print(json.dumps({"tool": "bench_balanced_set", "grid": [Nx, Ny, Nz], "dtype": name, **kw}), flush=True)

            grid = bz.RectilinearGrid((Nx, Ny, Nz), x=(0, Lx), y=(0, Ly), z=(0, Lz), float_type=float_type)
            dyn = bz.CompressibleDynamics(bz.SplitExplicitTimeDiscretization(), reference_potential_temperature=lambda z: 300.0 + 4e-3 * z)
            m = bz.CompressibleAtmosphereModel(grid, dyn, advection=bz.WENO(order=5))
            spec = bz.HydrostaticallyBalancedDensity()
            m.set(ρ=spec, θ=theta, qᵗ=qv, u=u, compute_reference_state=True)
            med, best = timed(lambda: set_hydrostatically_balanced_density_(m, spec))
            emit(what="balanced_set", ms_median=med, ms_min=best, reps=a.reps)
            m.profile_enable(True)
            m.profile_reset()
            for _ in range(a.reps):
                set_hydrostatically_balanced_density_(m, spec)
            m.synchronize()
            prof = m.profile()
            m.profile_enable(False)
            per = {k: t / n for k, (t, n) in prof.items() if n}
            pows = 8 * (Nz - 1) * Nx * Ny + 2 * Nx * Ny
            # compulsory words per cell: rescale (momentum launch) reads both densities and reads + writes four fields; residual reads ρ, ρq, writes ρᵈ
            emit(what="kernels", ms_per_launch=per, launches={k: n for k, (t, n) in prof.items()},
                 exner_columns_gpow_per_s=pows / (per["exner_columns"] * 1e-3) / 1e9,
                 exner_columns_bytes=4 * word * cells,
                 rescale_roofline_fraction=(10 + 4) / 2 * word * cells / (per["rescale_density_weighted"] * 1e-3) / ROOFLINE,
                 dry_from_total_roofline_fraction=3 * word * cells / (per["dry_from_total"] * 1e-3) / ROOFLINE)
            dt = 0.5
            m.time_step(dt)
            med, best = timed(lambda: m.time_step(dt))
            emit(what="step", ms_per_step_median=med, ms_per_step_min=best, dt=dt)
            assert np.isfinite(m.dynamics.pressure.interior_cpu()).all()
            del m
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
