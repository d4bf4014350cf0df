#!/usr/bin/env python
"""tools/bench_azimuthal.py — what the device's azimuthal mean and polar winds (csrc/bz_azimuthal.hip) cost.

At 512 x 512 x 64 (default), Nr = 30, m = 4, rings of radius 0.3 Lx about the domain centre, in Float64 and Float32:
  first        bz_azimuthal_mean with the ring plan built (the geometry alternates between two radii, so every call rebuilds it)
  repeat       bz_azimuthal_mean with the plan cached (both include the read-back of the profile and the synchronisation)
  polar_winds  one bz_polar_winds call writing both components
Each is timed with events after `--warmup` calls, `--reps` repetitions, and reported as the median with the bytes it must move and that as
a fraction of the 8 TB/s HBM roofline (mean: the field once; winds: u, v in, two fields out).  `host` is the route without the kernels:
the field copied to the host and the numpy restatement of tests/azimuthal_reference.py there (Float64 sums, one repetition).
One JSON line per (dtype, measurement).

    python tools/bench_azimuthal.py [--size 512 512 64] [--Nr 30] [--m 4] [--reps 10] [--warmup 3] [--no-host]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np

ROOFLINE = 8e12      # bytes / s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, nargs=3, default=[512, 512, 64])
    ap.add_argument("--Nr", type=int, default=30)
    ap.add_argument("--m", type=int, default=4)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-host", action="store_true")
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

    for real in (np.float64, np.float32):
        Nx, Ny, Nz = a.size
        Lx, Ly = 1000.0 * Nx, 1000.0 * Ny
        grid = bz.RectilinearGrid((Nx, Ny, Nz), x=(-Lx / 2, Lx / 2), y=(-Ly / 2, Ly / 2), z=(0, 16e3), float_type=real)
        m = bz.AtmosphereModel(grid, dynamics=bz.AnelasticDynamics(bz.ReferenceState(grid, potential_temperature=300.0)), advection=bz.WENO(order=5))
        m.set(θ=lambda x, y, z: 300.0 + 4e-3 * z + np.sin(2 * np.pi * x / Lx) * np.cos(2 * np.pi * y / Ly),
              u=lambda x, y, z: -1e-4 * y + 0 * x + 0 * z, v=lambda x, y, z: 1e-4 * x + 0 * y + 0 * z, enforce_mass_conservation=False)
        word, cells = np.dtype(real).itemsize, Nx * Ny * Nz
        f = m.potential_temperature
        vt, vr = (bz.Field(grid, (bz.Center,) * 3, m.device) for _ in range(2))
        radius = 0.3 * Lx
        flip = [0]

        def first():
            flip[0] ^= 1
            bz.azimuthal_mean(f, radius * (1.0 - 0.01 * flip[0]), a.Nr, m=a.m, model=m)

        import ctypes as C
        from breeze_jl_amd.diagnostics import _set_nodes
        _set_nodes(m)
        u, v = m.velocities["u"], m.velocities["v"]

        def winds():
            m._check(m._lib.bz_polar_winds(m._ctx, C.c_void_p(u.ptr()), C.c_void_p(v.ptr()), 0.0, 0.0, C.c_void_p(vt.ptr()), C.c_void_p(vr.ptr())),
                     "bz_polar_winds")

        measurements = {
            "first": (first, word * cells),
            "repeat": (lambda: bz.azimuthal_mean(f, radius, a.Nr, m=a.m, model=m), word * cells),
            "polar_winds": (winds, 4 * word * cells),
        }
        for name, (fn, nbytes) in measurements.items():
            med, best = timed(fn)
            print(json.dumps({"tool": "bench_azimuthal", "grid": [Nx, Ny, Nz], "Nr": a.Nr, "m": a.m, "dtype": "f64" if word == 8 else "f32",
                              "what": name, "ms_median": med, "ms_min": best, "reps": a.reps, "bytes": nbytes,
                              "roofline_fraction": nbytes / (med * 1e-3) / ROOFLINE}), flush=True)
        if not a.no_host:
            import azimuthal_reference as ar
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host = f.interior.cpu().numpy()
            t1 = time.perf_counter()
            ref = ar.azimuthal_mean(host, grid.xᶜ, grid.yᶜ, grid.Δx, grid.Δy, radius, a.Nr, m=a.m, dtype=real, accumulate=np.float64)
            t2 = time.perf_counter()
            dev = bz.azimuthal_mean(f, radius, a.Nr, m=a.m, model=m)
            print(json.dumps({"tool": "bench_azimuthal", "grid": [Nx, Ny, Nz], "Nr": a.Nr, "m": a.m, "dtype": "f64" if word == 8 else "f32",
                              "what": "host", "ms_copy": (t1 - t0) * 1e3, "ms_numpy": (t2 - t1) * 1e3, "ms_total": (t2 - t0) * 1e3,
                              "bytes_copied": word * cells, "counts_equal": bool(np.array_equal(dev.counts, ref.counts)),
                              "max_abs_difference": float(np.nanmax(np.abs(dev.data.T - ref.mean.astype(np.float64))))}), flush=True)
        del m, f, vt, vr, measurements
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
