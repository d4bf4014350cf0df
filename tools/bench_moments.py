#!/usr/bin/env python
"""tools/bench_moments.py — what the turbulence statistics of an LES output list cost per evaluation (csrc/bz_moments.hip).

At 512 x 512 x 256 (default), in Float64 and Float32, on the convective-boundary-layer model of bench.py after a few steps, the 18
profiles of the reference's examples/neutral_atmospheric_boundary_layer.jl:203-221 (u, v, w, θ, νₑ, their squares, u w, v w, θ w, u² w,
v² w, w³, νₑ³, ∂z u, ∂z v, ∂z θ, all under @at((Center, Center, Center), ·); the temperature stands in for νₑ):
  fused          one bz_horizontal_moments call for the whole list (one read-back, one synchronisation)
  torch+average  the route without it: every expression formed with torch on the device parent arrays (the same two-point means, written
                 with shifted views, the result stored into a parent-shaped scratch field), then one bz_horizontal_average per profile
Both are timed with events after a warm-up and reported as the median, with the compulsory bytes (the five field interiors read once),
that as a fraction of the 8 TB/s HBM roofline, and the time as a fraction of one CBL step of the same size and precision (the median of
`--steps` single steps).  The two routes' profiles are compared (`max_rel_diff`, relative to the largest magnitude of a profile).
One JSON line per (dtype, route).

    python tools/bench_moments.py [--size 512 512 256] [--reps 20] [--torch-reps 5] [--warmup 3] [--steps 5]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np

ROOFLINE = 8e12      # bytes / s
U, V, W, TH, NU = range(5)
# (factors ((field, power), ...), dz): the ABL list, every entry under @at(CCC, ·)
ABL = ([(((f, 1),), False) for f in (U, V, W, TH, NU)] + [(((f, 2),), False) for f in (U, V, W)] +
       [(((U, 1), (W, 1)), False), (((V, 1), (W, 1)), False), (((TH, 1), (W, 1)), False), (((U, 2), (W, 1)), False), (((V, 2), (W, 1)), False),
        (((W, 3),), False), (((NU, 3),), False)] + [(((f, 1),), True) for f in (U, V, TH)])


def torch_profile(bz, model, fields, factors, dz, scratch):
    """at(CCC, expression) formed with torch on the parent arrays, then bz_horizontal_average of the result"""
    g = model.grid
    face = [tuple(int(l is bz.Face) for l in f.loc) for f in fields]
    L = list(face[factors[0][0]])
    if dz:
        L[2] = 1 - L[2]
    ext = L      # the values at L are needed on Nx + 1 (Ny + 1, Nz + 1) points where L is a face

    def view(P, s):
        return P[g.Hz + s[2]:g.Hz + s[2] + g.Nz + ext[2], g.Hy + s[1]:g.Hy + s[1] + g.Ny + ext[1], g.Hx + s[0]:g.Hx + s[0] + g.Nx + ext[0]]

    def mean(parts):
        return parts[0] if len(parts) == 1 else (parts[0] + parts[1]) / 2

    if dz:
        P = fields[factors[0][0]].parent
        if L[2]:
            value = (view(P, (0, 0, 0)) - view(P, (0, 0, -1))) / g.Δz
        else:
            value = (view(P, (0, 0, 1)) - view(P, (0, 0, 0))) / g.Δz
    else:
        value = None
        for f, p in factors:
            P = fields[f].parent
            offs = [(0,) if a == b else ((-1, 0) if b else (0, 1)) for a, b in zip(face[f], L)]
            t = mean([mean([mean([view(P, (ax, ay, az)) ** p for az in offs[2]]) for ay in offs[1]]) for ax in offs[0]])
            value = t if value is None else value * t
    centred = mean([mean([mean([value[az:az + g.Nz, ay:ay + g.Ny, ax:ax + g.Nx] for az in range(L[2] + 1)]) for ay in range(L[1] + 1)])
                    for ax in range(L[0] + 1)])
    scratch.interior.copy_(centred)
    return bz.horizontal_average(model, scratch)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, nargs=3, default=[512, 512, 256])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--torch-reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=5)
    a = ap.parse_args()
    import torch
    import breeze_jl_amd as bz

    def timed(fn, reps, warmup):
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return float(np.median(ms)), float(np.min(ms))

    CCC = (bz.Center, bz.Center, bz.Center)
    for real in (np.float64, np.float32):
        Nx, Ny, Nz = a.size
        m = bz.benchmarks.convective_boundary_layer((Nx, Ny, Nz), float_type=real)
        step_ms, _ = timed(lambda: m.time_step(1.0), a.steps, 2)
        fields = [m.velocities["u"], m.velocities["v"], m.velocities["w"], m.potential_temperature, m.temperature]
        averages = {}
        for n, (factors, dz) in enumerate(ABL):
            if dz:
                e = bz.partial_z(fields[factors[0][0]])
            else:
                e = None
                for f, p in factors:
                    t = fields[f] if p == 1 else fields[f] ** p
                    e = t if e is None else e * t
            averages[n] = bz.Average(bz.at(CCC, e), model=m)
        scratch = bz.Field(m.grid, CCC, m.device)
        word, cells = np.dtype(real).itemsize, Nx * Ny * Nz
        nbytes = 5 * word * cells
        fused = bz.compute_averages(m, averages)
        plain = {n: torch_profile(bz, m, fields, factors, dz, scratch) for n, (factors, dz) in enumerate(ABL)}
        diff = max(float(np.max(np.abs(fused[n].astype(np.float64) - plain[n].astype(np.float64))) /
                         max(float(np.max(np.abs(plain[n]))), 1e-300)) for n in fused)
        routes = {"fused": (lambda: bz.compute_averages(m, averages), a.reps),
                  "torch+average": (lambda: [torch_profile(bz, m, fields, factors, dz, scratch) for factors, dz in ABL], a.torch_reps)}
        for name, (fn, reps) in routes.items():
            med, best = timed(fn, reps, a.warmup if name == "fused" else 1)
            print(json.dumps({"tool": "bench_moments", "grid": [Nx, Ny, Nz], "dtype": "f64" if word == 8 else "f32", "what": name,
                              "profiles": len(ABL), "ms_median": med, "ms_min": best, "reps": reps, "compulsory_bytes": nbytes,
                              "roofline_fraction": nbytes / (med * 1e-3) / ROOFLINE, "cbl_step_ms": step_ms,
                              "fraction_of_cbl_step": med / step_ms, "max_rel_diff": diff}), flush=True)
        del m, fields, averages, scratch, routes
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
