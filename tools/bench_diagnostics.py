#!/usr/bin/env python
"""tools/bench_diagnostics.py — what the device diagnostics (csrc/bz_diagnostics.hip) cost.

At 512 x 512 x 256 (default), in Float64 and Float32, on a warm-phase saturation-adjustment model (T, q^v, q^l in, reference columns):
  fused        one bz_compute_diagnostics call for {theta_v, theta_e, H, q^v+}
  singles      the sum of the four single calls
  dewpoint     the dewpoint alone
  average      one bz_horizontal_average of a centre field (includes its read-back and synchronisation)
Each is timed with events after a warm-up, `--reps` repetitions, and reported as the median with the bytes it must move (inputs once +
outputs) and that as a fraction of the 8 TB/s HBM roofline.  `host` is what the same four fields cost without the kernel: T, q^v, q^l
copied to the host and the numpy restatement of tests/diagnostics_reference.py evaluated there (Float64, one repetition).
One JSON line per (dtype, measurement).

    python tools/bench_diagnostics.py [--size 512 512 256] [--reps 20] [--warmup 3] [--no-host]
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
    ap.add_argument("--size", type=int, nargs=3, default=[512, 512, 256])
    ap.add_argument("--reps", type=int, default=20)
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
        grid = bz.RectilinearGrid((Nx, Ny, Nz), x=(0, 100.0 * Nx), y=(0, 100.0 * Ny), z=(0, 12e3), float_type=real)
        m = bz.AtmosphereModel(grid, dynamics=bz.AnelasticDynamics(bz.ReferenceState(grid, potential_temperature=300.0)),
                               advection=bz.WENO(order=5), microphysics=bz.SaturationAdjustment(equilibrium=bz.WarmPhaseEquilibrium()))
        m.set(θ=lambda x, y, z: 300.0 + 4e-3 * z + np.sin(2 * np.pi * x / (100.0 * Nx)) + 0 * y,
              qᵗ=lambda x, y, z: 0.018 * np.exp(-z / 2.5e3) + 0 * x + 0 * y, enforce_mass_conservation=False)
        word, cells = np.dtype(real).itemsize, Nx * Ny * Nz
        four = [bz.VirtualPotentialTemperature(m), bz.EquivalentPotentialTemperature(m), bz.RelativeHumidity(m),
                bz.SaturationSpecificHumidity(m)]
        out4 = [bz.Field(grid, (bz.Center,) * 3, m.device) for _ in four]
        from breeze_jl_amd.diagnostics import _launch
        measurements = {
            "fused": (lambda: _launch(m, four, out4, False), (3 + 4) * word * cells),
            "singles": (lambda: [_launch(m, [op], [f], False) for op, f in zip(four, out4)], 4 * (3 + 1) * word * cells),
            "dewpoint": (lambda: _launch(m, [bz.DewpointTemperature(m)], out4[:1], False), (3 + 1) * word * cells),
            "average": (lambda: bz.horizontal_average(m, out4[2]), word * cells),
        }
        for name, (fn, nbytes) in measurements.items():
            med, best = timed(fn)
            print(json.dumps({"tool": "bench_diagnostics", "grid": [Nx, Ny, Nz], "dtype": "f64" if word == 8 else "f32", "what": name,
                              "ms_median": med, "ms_min": best, "reps": a.reps, "bytes": nbytes,
                              "roofline_fraction": nbytes / (med * 1e-3) / ROOFLINE}), flush=True)
        if word == 8 and not a.no_host:
            import diagnostics_reference as dr
            c = dr.constants()
            μ = m.microphysical_fields
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            T, qv, ql = (f.interior.cpu().numpy() for f in (m.temperature, μ["qᵛ"], μ["qˡ"]))
            t1 = time.perf_counter()
            sl = slice(grid.Hz, grid.Hz + Nz)
            p = m.dynamics.reference_state.pressure[sl][:, None, None]
            for kind in ("VIRTUAL_POTENTIAL_TEMPERATURE", "EQUIVALENT_POTENTIAL_TEMPERATURE", "RELATIVE_HUMIDITY", "SATURATION_SPECIFIC_HUMIDITY"):
                dr.evaluate(kind, T, qv, ql, p, None, None, None, c)
            t2 = time.perf_counter()
            print(json.dumps({"tool": "bench_diagnostics", "grid": [Nx, Ny, Nz], "dtype": "f64", "what": "host",
                              "ms_copy": (t1 - t0) * 1e3, "ms_numpy": (t2 - t1) * 1e3, "ms_total": (t2 - t0) * 1e3,
                              "bytes_copied": 3 * word * cells}), flush=True)
        del m, out4, four, measurements
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
