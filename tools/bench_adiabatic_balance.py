#!/usr/bin/env python
"""tools/bench_adiabatic_balance.py — what one cycle of balance_adiabatically! costs on the device (csrc/bz_adiabatic_balance.hip).

At 256 x 256 x 128, Float64, WENO(order = 5), a moist warm bubble on a stripped model, for the compressible and the anelastic model:
  single_call   ms per balance_adiabatically_(model, Δt=dt, cycles=1): snapshot, four steps (+dt, -dt, -dt, +dt), two nudges with their halo
                fills and two update_state! behind ONE library call (the snapshot block is allocated and released by the call)
  composition   ms for the same cycle composed from the public calls every earlier version has: four time_step_, torch nudges over the
                parent arrays (add_ / div_) and two update_state_, with torch clones as the snapshot
The two are timed alternately, `--reps` times each after `--warmup` untimed rounds, by a host clock around work that ends in a device
synchronise (the single call waits for its own work before it releases the snapshot).  One JSON line per measurement.  Reporting, not a gate.

    python tools/bench_adiabatic_balance.py [--size 256x256x128] [--reps 5] [--warmup 2] [--out profiles/bench_adiabatic_balance.jsonl]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="256x256x128")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--weight", type=float, default=2.0)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    a = ap.parse_args()
    import torch
    import breeze_jl_amd as bz

    Nx, Ny, Nz = (int(n) for n in a.size.split("x"))
    Lx, Ly, Lz = 100.0 * Nx, 100.0 * Ny, 12e3
    dt = 0.5

    def theta(x, y, z):
        r = np.sqrt((x - Lx / 2) ** 2 + (y - Ly / 2) ** 2 + (z - 3000.0) ** 2)
        return 300.0 + 4e-3 * z + 2.0 * np.maximum(0.0, 1.0 - r / 2000.0)

    def qv(x, y, z):
        return 0.012 * np.exp(-z / 2.5e3) * (1.0 + 0.2 * np.cos(2 * np.pi * y / Ly)) + 0 * x

    def u(x, y, z):
        return 5.0 + 2.0 * np.sin(2 * np.pi * y / Ly) + 0 * x + 0 * z

    def emit(**kw):
        line = json.dumps({"tool": "bench_adiabatic_balance", "grid": [Nx, Ny, Nz], "dtype": "f64", "dt": dt, "weight": a.weight, **kw})
        print(line, flush=True)
        if a.out:
            with open(a.out, "a", encoding="utf-8") as fh:
                fh.write(line + "\n")

    def build(kind):
        grid = bz.RectilinearGrid((Nx, Ny, Nz), x=(0, Lx), y=(0, Ly), z=(0, Lz))
        if kind == "compressible":
            dyn = bz.CompressibleDynamics(bz.SplitExplicitTimeDiscretization(), reference_potential_temperature=lambda z: 300.0 + 4e-3 * z)
            m = bz.CompressibleAtmosphereModel(grid, dyn, advection=bz.WENO(order=5))
            m.set(ρ=bz.HydrostaticallyBalancedDensity(), θ=theta, qᵗ=qv, u=u)
            return m, bz.compressible.time_step_, bz.compressible.update_state_
        m = bz.AtmosphereModel(grid, dynamics=bz.AnelasticDynamics(bz.ReferenceState(grid, potential_temperature=300.0)), advection=bz.WENO(order=5))
        m.set(θ=theta, qᵗ=qv, u=u)
        return m, bz.time_step_, bz.update_state_

    for kind in ("compressible", "anelastic"):
        m, time_step, update_state = build(kind)
        fields = bz.initial_fields(m)

        def single_call():
            bz.balance_adiabatically_(m, Δt=dt, cycles=1, weight=a.weight)

        def composition():
            snap = [f.parent.clone() for f in fields]
            for s in (1.0, -1.0):
                time_step(m, s * dt)
                time_step(m, -s * dt)
                for f, x0 in zip(fields, snap):
                    f.parent.add_(x0, alpha=a.weight).div_(1.0 + a.weight)
                update_state(m)          # (its halo fills cover the nudged fields)
            m.clock.time, m.clock.iteration, m.clock.last_Δt = 0.0, 0, float("inf")

        def timed(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            return 1e3 * (time.perf_counter() - t0)

        for _ in range(a.warmup):
            single_call()
            composition()
        ms = {"single_call": [], "composition": []}
        for _ in range(a.reps):
            ms["single_call"].append(timed(single_call))
            ms["composition"].append(timed(composition))
        for what, v in ms.items():
            emit(model=kind, what=what, ms_median=float(np.median(v)), ms_min=float(np.min(v)), ms_all=[round(x, 3) for x in v], reps=a.reps)
        emit(model=kind, what="ratio", single_over_composition=float(np.median(ms["single_call"]) / np.median(ms["composition"])))
        assert np.isfinite(m.temperature.interior_cpu()).all()
        del m, fields
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
