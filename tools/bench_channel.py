#!/usr/bin/env python
"""tools/bench_channel.py — what the y walls cost a step of the compressible split-explicit model.

Two grids, each stepped as (Periodic, Bounded, Bounded) — impenetrable south and north walls, the topology of the reference's
validation/cartesian_baroclinic_wave — and as (Periodic, Periodic, Bounded) from the same build, Float64 and Float32:
  channel   400 x 60 x 30 at halo (5, 5, 5): the validation case's grid (100 km cells, dt = 600 s, the default SplitExplicitTimeDiscretization:
            2, 3 and 5 substeps, FPlane); rows of 400 cells: the ragged scalar kernel
  box       512 x 512 x 64 at halo (3, 3, 3): 100 m cells, dt = 1 s, six substeps; rows of 512 cells: the LDS-tiled scalar kernel
ms per time_step between two events after `--warmup` steps and a device synchronisation, median over `--reps` windows of `--steps` steps.
One JSON line: {"tool": "bench_channel", "results": [{grid, dtype, walled_ms, periodic_ms, ratio}, ...]}; with --profile each result also
carries the library's kernel table (ms, launches) of a walled and of a periodic step.

    python tools/bench_channel.py [--steps 5] [--reps 5] [--warmup 3] [--only channel|box] [--profile]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np

WALLS, PERIODIC = ("Periodic", "Bounded", "Bounded"), ("Periodic", "Periodic", "Bounded")
CASES = {
    "channel": dict(size=(400, 60, 30), halo=(5, 5, 5), cell=(1e5, 1e5, 1e3), dt=600.0, substeps=None, f=1.03e-4, jet=20.0),
    "box": dict(size=(512, 512, 64), halo=(3, 3, 3), cell=(100.0, 100.0, 125.0), dt=1.0, substeps=6, f=None, jet=5.0),
}


def theta_ref(z):
    return 250.0 * np.exp(9.80665 * z / (1005.0 * 250.0))


def build(bz, case, topology, float_type):
    Nx, Ny, Nz = case["size"]
    Lx, Ly, Lz = (n * d for n, d in zip(case["size"], case["cell"]))
    grid = bz.RectilinearGrid(case["size"], halo=case["halo"], topology=topology, x=(0.0, Lx), y=(0.0, Ly), z=(0.0, Lz), float_type=float_type)
    td = bz.SplitExplicitTimeDiscretization() if case["substeps"] is None else bz.SplitExplicitTimeDiscretization(substeps=case["substeps"])
    dyn = bz.CompressibleDynamics(td, surface_pressure=1e5, reference_potential_temperature=theta_ref)
    kw = {} if case["f"] is None else dict(coriolis=bz.FPlane(f=case["f"]))
    m = bz.CompressibleAtmosphereModel(grid, dyn, advection=bz.WENO(order=5), **kw)
    ref = dyn.reference_state
    rho = ref.density[grid.Hz:grid.Hz + grid.Nz][:, None, None]
    jet = lambda x, y, z: case["jet"] * np.sin(np.pi * y / Ly) ** 2 * np.exp(-((z - Lz / 3) / (Lz / 4)) ** 2) + 0 * x          # noqa: E731
    theta = lambda x, y, z: (theta_ref(z) * (1 - 0.01 * np.cos(2 * np.pi * y / Ly))                                        # noqa: E731
                             + np.exp(-((x - 0.4 * Lx) / (0.1 * Lx)) ** 2 - ((y - 0.5 * Ly) / (0.2 * Ly)) ** 2))
    qv = lambda x, y, z: 5e-3 * np.exp(-z / 2e3) * (1 + 0.2 * np.sin(2 * np.pi * x / Lx)) + 0 * y                            # noqa: E731
    m.set(ρ=rho, θ=theta, u=jet, v=0.0, w=0.0, qᵗ=qv)
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=sorted(CASES), default=None)
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    import torch
    import breeze_jl_amd as bz

    def timed(m, dt):
        for _ in range(a.warmup):
            m.time_step(dt)
        m.synchronize()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.steps):
                m.time_step(dt)
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1) / a.steps)
        return float(np.median(ms)), float(np.min(ms))

    def table(m, dt):
        m.profile_enable(True)
        m.profile_reset()
        m.time_step(dt)
        m.synchronize()
        prof = m.profile()
        m.profile_enable(False)
        return {k: [round(t, 4), n] for k, (t, n) in prof.items()}

    results = []
    for name, case in CASES.items():
        if a.only and name != a.only:
            continue
        for ft, label in ((np.float64, "f64"), (np.float32, "f32")):
            r = {"case": name, "grid": list(case["size"]), "halo": list(case["halo"]), "dtype": label}
            for key, topo in (("walled", WALLS), ("periodic", PERIODIC)):
                m = build(bz, case, topo, ft)
                med, best = timed(m, case["dt"])
                r[key + "_ms"], r[key + "_ms_min"] = round(med, 4), round(best, 4)
                assert np.isfinite(m.potential_temperature_density.interior_cpu()).all(), (name, label, key)
                if a.profile:
                    r[key + "_profile"] = table(m, case["dt"])
                del m
                torch.cuda.empty_cache()
            r["ratio"] = round(r["walled_ms"] / r["periodic_ms"], 4)
            results.append(r)
    print(json.dumps({"tool": "bench_channel", "steps": a.steps, "reps": a.reps, "warmup": a.warmup, "results": results}), flush=True)


if __name__ == "__main__":
    main()
