#!/usr/bin/env python
"""tools/bench_instantaneous_precipitation.py — what microphysics = InstantaneousPrecipitation(...) costs on the compressible
split-explicit model (csrc/bz_instant_precip.hip: k_instantaneous_precipitation, one launch per step, followed by one update_state!).

At 256 x 256 x 128 and 512 x 512 x 256, Float64 and Float32, WENO(order = 5), on the mixed bubble of the tests (a saturated upper part and a
clear surface layer around a moist bubble: saturated and clear wavefronts both occur):
  kernel   ms per `instantaneous_precipitation` record of the library's own profile table (HIP-event times), the 7 compulsory words per
           cell of the launch (rho, rho_d, rho theta, rho q^v read; rho theta, rho q^v, precipitation_rate written) as a fraction of the
           8 TB/s HBM roofline, and the fraction of cells that condensed in the last step (precipitation_rate > 0 in a model that started
           from zeros is an upper bound: a cell keeps its rate once it has condensed)
  step     ms per time_step with the scheme and of the same model with microphysics = None: the median of `--reps` windows of `--steps` steps
One JSON line per measurement; no number is fixed in advance.

    python tools/bench_instantaneous_precipitation.py [--sizes 256x256x128 512x512x256] [--dtypes f64 f32] [--steps 5] [--reps 5] [--warmup 1] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np

ROOFLINE = 8e12      # bytes / s
WORDS = 7


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="+", default=["256x256x128", "512x512x256"])
    ap.add_argument("--dtypes", nargs="+", default=["f64", "f32"], choices=["f64", "f32"])
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
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

    theta_ref = lambda z: 300.0 * np.exp(9.80616 * z / (1005 * 300.0))
    for size in a.sizes:
        Nx, Ny, Nz = (int(n) for n in size.split("x"))
        Lx, Ly, Lz = 100.0 * Nx, 100.0 * Ny, 3e3
        cells = Nx * Ny * Nz
        dt = 0.25
        bub = lambda x, y, z: np.maximum(0.0, 1.0 - np.sqrt(((x - 0.5 * Lx) / (0.225 * Lx)) ** 2 + ((y - 0.5 * Ly) / (0.3 * Ly)) ** 2
                                                            + ((z - 0.4 * Lz) / (0.3 * Lz)) ** 2))
        theta = lambda x, y, z: 300.0 + 0.5 * bub(x, y, z)
        qt = lambda x, y, z: 0.012 + 0.014 * bub(x, y, z) + 0.004 * (z / Lz)
        for dtype in a.dtypes:
            word = 8 if dtype == "f64" else 4
            ft = np.float64 if dtype == "f64" else np.float32

            def emit(**kw):
                line = json.dumps({"tool": "bench_instantaneous_precipitation", "grid": [Nx, Ny, Nz], "dtype": dtype, **kw})
                print(line, flush=True)
                if a.out:
                    with open(a.out, "a", encoding="utf-8") as f:
                        f.write(line + "\n")

            for scheme in (False, True):
                g = bz.RectilinearGrid((Nx, Ny, Nz), x=(0, Lx), y=(0, Ly), z=(0, Lz), float_type=ft)
                dyn = bz.CompressibleDynamics(bz.SplitExplicitTimeDiscretization(), surface_pressure=1e5, reference_potential_temperature=theta_ref)
                mp = bz.InstantaneousPrecipitation(equilibrium=bz.WarmPhaseEquilibrium()) if scheme else None
                m = bz.CompressibleAtmosphereModel(g, dyn, advection=bz.WENO(order=5), microphysics=mp)
                rho = m.dynamics.reference_state.density[g.Hz:g.Hz + g.Nz][:, None, None]
                m.set(ρ=rho, θ=theta, qᵗ=qt, u=2.0, v=0.0, w=0.0)

                def steps():
                    for _ in range(a.steps):
                        m.time_step(dt)

                med, best = timed(steps)
                emit(what="step", scheme=scheme, ms_per_step_median=med / a.steps, ms_per_step_min=best / a.steps, steps=a.steps, reps=a.reps)
                if scheme:
                    m.profile_enable(True)
                    m.profile_reset()
                    steps()
                    m.synchronize()
                    prof = m.profile()
                    m.profile_enable(False)
                    ms, calls = prof["instantaneous_precipitation"]
                    nbytes = word * WORDS * cells
                    P = m.microphysical_fields["precipitation_rate"].interior
                    emit(what="kernel", record="instantaneous_precipitation", ms_per_call=ms / calls, calls=calls, words_per_cell=WORDS, bytes=nbytes,
                         roofline_fraction=nbytes / (ms / calls * 1e-3) / ROOFLINE, cells_that_have_condensed=float((P > 0).double().mean().item()))
                assert np.isfinite(m.potential_temperature_density.interior_cpu()).all()
                del m
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
