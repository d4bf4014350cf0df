#!/usr/bin/env python
"""tools/bench_negative_moisture.py — what BulkMicrophysics(negative_moisture_correction = VerticalBorrowing()) costs on the anelastic
model, and that the uncorrected step did not pay for it.

Grids 256 x 256 x 128 and 512 x 512 x 256 over 25.6 km x 25.6 km x 10 km, Float64 and Float32, WENO(order = 5), warm-phase saturation
adjustment under theta_0 = 300 K.
  kernel   ms per launch of k_fix_negative_moisture (profile slot fix_negative_moisture) on a field without negative cells and on one with
           about a tenth of its cells negative (scattered cells and whole upper layers, so deficits travel), against its compulsory bytes
           (one word read per cell, one written per cell that changes) and the 8 TB/s roofline.  The kernel stores a cell where its bits
           changed; the store-always policy it was measured against is in the recorded lines (policy = "store_always") and in DESIGN §7.
           The field is restored from a copy before every launch (not timed: the slot's events bracket the kernel alone); windows of
           `--launches` launches alternate between the two cases.
  step     ms per time_step of the corrected model and of the model built with the bare SaturationAdjustment, same build, same state (a
           saturated column, a warm bubble, about a tenth of the cells of the upper levels negative), alternating windows
  parent   (--parent-lib DIR: libbreeze_hip.so / libbreeze_hip_f32.so built from the parent commit) the uncorrected step on this build and on
           the parent's build in the same call, alternating A B B', B B' A, ...; the parent runs as two models, and the spread between those
           two runs of the same library is the yardstick: this build's median must not exceed the parent's by more than it
One JSON line per measurement, appended to profiles/bench_negative_moisture.jsonl (--out).  No number is fixed in advance.

    python tools/bench_negative_moisture.py [--sizes 256x256x128 512x512x256] [--dtypes f64 f32] [--steps 10] [--rounds 5] [--parent-lib DIR]
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np

ROOFLINE = 8e12      # bytes / s
SLOT = "fix_negative_moisture"


def bind_parent(path):
    """a library of the parent commit under the current binding: every symbol it exports"""
    from breeze_jl_amd import _lib
    import torch  # noqa: F401
    lib = C.CDLL(path)
    f32 = path.endswith("_f32.so")
    for name, (res, args) in _lib.SYMBOLS.items():
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = res, ([_lib._f32_type(a) for a in args] if f32 else args)
    _lib._libs[path] = lib
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="+", default=["256x256x128", "512x512x256"])
    ap.add_argument("--dtypes", nargs="+", default=["f64", "f32"], choices=["f64", "f32"])
    ap.add_argument("--steps", type=int, default=10, help="steps per timed window")
    ap.add_argument("--rounds", type=int, default=5, help="alternating windows per model / case")
    ap.add_argument("--launches", type=int, default=20, help="kernel launches per window")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dt", type=float, default=1.0)
    ap.add_argument("--parent-lib", default=None, help="directory with the parent commit's libbreeze_hip.so and libbreeze_hip_f32.so")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_negative_moisture.jsonl"))
    a = ap.parse_args()
    assert a.steps * a.rounds >= 50, "at least 50 steps per model"
    import torch
    import breeze_jl_amd as bz
    from breeze_jl_amd import _lib

    def build(size, ft, corrected, lib_dir=None):
        own = (_lib.LIB_PATH, _lib.F32_LIB_PATH)
        if lib_dir:          # the model binds the library its constructor finds under these names
            _lib.LIB_PATH, _lib.F32_LIB_PATH = os.path.join(lib_dir, "libbreeze_hip.so"), os.path.join(lib_dir, "libbreeze_hip_f32.so")
            for p in (_lib.LIB_PATH, _lib.F32_LIB_PATH):
                if p not in _lib._libs:
                    bind_parent(p)
        try:
            g = bz.RectilinearGrid(size, x=(0.0, 25.6e3), y=(0.0, 25.6e3), z=(0.0, 10e3), float_type=ft)
            ref = bz.ReferenceState(g, potential_temperature=300.0)
            sa = bz.SaturationAdjustment(equilibrium=bz.WarmPhaseEquilibrium())
            micro = bz.BulkMicrophysics(cloud_formation=sa, negative_moisture_correction=bz.VerticalBorrowing()) if corrected else sa
            m = bz.AtmosphereModel(g, dynamics=bz.AnelasticDynamics(ref), advection=bz.WENO(order=5), microphysics=micro)
        finally:
            _lib.LIB_PATH, _lib.F32_LIB_PATH = own
        return m, ref

    def state(size, m, ref, negatives):
        """a column saturated throughout, a warm bubble, a sheared wind; negatives: q^t < 0 in a third of the columns of the top three tenths
        of the levels (a tenth of the cells)"""
        Nx, Ny, Nz = size
        g, c = m.grid, m.thermodynamic_constants
        from breeze_jl_amd.thermodynamics import dry_air_gas_constant, vapor_gas_constant
        Rd, Rv = dry_air_gas_constant(c), vapor_gas_constant(c)
        T = ref.temperature[g.Hz:g.Hz + g.Nz]
        p = ref.pressure[g.Hz:g.Hz + g.Nz]
        dc = c.vapor_heat_capacity - c.liquid_heat_capacity
        L0 = c.liquid_reference_latent_heat - dc * c.energy_reference_temperature
        ps = c.triple_point_pressure * (T / c.triple_point_temperature) ** (dc / Rv) * np.exp((1 / c.triple_point_temperature - 1 / T) * L0 / Rv)
        qs = (Rd / Rv) * ps / (p - ps)
        x = (np.arange(Nx) + 0.5) * 25.6e3 / Nx
        y = (np.arange(Ny) + 0.5) * 25.6e3 / Ny
        z = (np.arange(Nz) + 0.5) * 10e3 / Nz
        r2 = ((x[None, None, :] - 12.8e3) / 4e3) ** 2 + ((y[None, :, None] - 12.8e3) / 4e3) ** 2 + ((z[:, None, None] - 4e3) / 2e3) ** 2
        qt = np.minimum(1.3 * qs, 0.03)[:, None, None] * np.ones((Nz, Ny, Nx))
        if negatives:
            cols = (np.arange(Nx)[None, :] + np.arange(Ny)[:, None]) % 3 == 0
            k0 = Nz - (3 * Nz) // 10
            qt[k0:, cols] *= -0.5
        m.set(qᵗ=qt, θ=300.0 + 2.0 * np.exp(-r2),
              u=5.0 + 2.0 * np.sin(2 * np.pi * x / 25.6e3)[None, None, :] * np.cos(np.pi * z / 10e3)[:, None, None] * np.ones((Nz, Ny, Nx)))

    def window(m):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.steps):
            m.time_step(a.dt)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.steps

    def stats(v):
        return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)), windows=[round(t, 5) for t in v])

    def alternate(models):
        for m in models.values():
            for _ in range(a.warmup):
                m.time_step(a.dt)
            m.synchronize()
        ms = {k: [] for k in models}
        keys = list(models)
        for r in range(a.rounds):          # the order rotates from round to round
            for k in keys[r % len(keys):] + keys[:r % len(keys)]:
                ms[k].append(window(models[k]))
        return {k: stats(v) for k, v in ms.items()}

    def kernel_window(m, saved):
        rq = m.moisture_density
        m.profile_reset()
        for _ in range(a.launches):
            rq.parent.copy_(saved)
            bz.fix_negative_moisture_(m)
        m.synchronize()
        ms, n = m.profile()[SLOT]
        assert n == a.launches
        return ms / n

    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    for size_s in a.sizes:
        size = tuple(int(n) for n in size_s.split("x"))
        cells = size[0] * size[1] * size[2]
        for dtype in a.dtypes:
            word, ft = (8, np.float64) if dtype == "f64" else (4, np.float32)

            def emit(**kw):
                line = json.dumps({"tool": "bench_negative_moisture", "grid": list(size), "dtype": dtype, "dt": a.dt, **kw})
                print(line, flush=True)
                with open(a.out, "a", encoding="utf-8") as f:
                    f.write(line + "\n")

            # ---- the kernel per launch ----
            cases = {}
            m, ref = build(size, ft, True)
            m.profile_enable(True)
            rng = np.random.default_rng(1)
            rho = np.asarray(ref.density)[m.grid.Hz:m.grid.Hz + m.grid.Nz][:, None, None]
            clean = (rho * (1e-3 + 1e-2 * rng.random((size[2], size[1], size[0])))).astype(ft)
            neg = clean.copy()
            neg[rng.random(neg.shape) < 0.07] *= -0.3                               # scattered cells
            neg[size[2] - max(1, (3 * size[2]) // 100):] *= -0.05                   # whole upper layers: deficits travel
            for name, arr in (("no_negatives", clean), ("tenth_negative", neg)):
                m.moisture_density.set_interior(arr)
                saved = m.moisture_density.parent.clone()
                bz.fix_negative_moisture_(m)
                m.synchronize()
                after = m.moisture_density.interior.cpu().numpy()
                changed = int((after.view(np.uint64 if word == 8 else np.uint32) != arr.view(np.uint64 if word == 8 else np.uint32)).sum())
                cases[name] = dict(saved=saved, negative_fraction=float((arr < 0).mean()), changed=changed)
            for case in cases.values():
                kernel_window(m, case["saved"])          # warm-up
            times = {k: [] for k in cases}
            keys = list(cases)
            for r in range(a.rounds):
                for k in keys[r % len(keys):] + keys[:r % len(keys)]:
                    times[k].append(kernel_window(m, cases[k]["saved"]))
            for name, case in cases.items():
                t = stats(times[name])
                nbytes = (cells + case["changed"]) * word
                emit(what="kernel", policy="store_if_changed", field=name, negative_fraction=case["negative_fraction"], cells_changed=case["changed"],
                     launches_per_window=a.launches, windows=a.rounds, ms_per_launch=t, compulsory_bytes=nbytes,
                     share_of_8TBs=nbytes / (t["median"] * 1e-3) / ROOFLINE)
            del cases, case, m, saved
            torch.cuda.empty_cache()

            # ---- the step with and without the correction, same build ----
            models = {}
            for name, corrected in (("corrected", True), ("uncorrected", False)):
                models[name], ref = build(size, ft, corrected)
                state(size, models[name], ref, negatives=True)
            t = alternate(models)
            emit(what="step", steps_per_window=a.steps, windows=a.rounds, ms_per_step=t,
                 corrected_over_uncorrected=t["corrected"]["median"] / t["uncorrected"]["median"])
            for m in models.values():
                assert np.isfinite(m.potential_temperature_density.interior_cpu()).all()
            del models, m
            torch.cuda.empty_cache()

            # ---- the uncorrected step against the parent's build ----
            if a.parent_lib:
                trio = {}
                for name, lib_dir in (("this_build", None), ("parent_a", a.parent_lib), ("parent_b", a.parent_lib)):
                    trio[name], ref = build(size, ft, False, lib_dir)
                    state(size, trio[name], ref, negatives=False)
                t = alternate(trio)
                spread = abs(t["parent_a"]["median"] - t["parent_b"]["median"])
                parent = min(t["parent_a"]["median"], t["parent_b"]["median"])
                emit(what="uncorrected_step_vs_parent", steps_per_window=a.steps, windows=a.rounds, ms_per_step=t, parent_repeat_spread_ms=spread,
                     this_minus_parent_ms=t["this_build"]["median"] - parent, not_slower_than_parent=bool(t["this_build"]["median"] <= parent + spread))
                del trio
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
