#!/usr/bin/env python
"""tools/bench_mixed_phase.py — what SaturationAdjustment(equilibrium = MixedPhaseEquilibrium()) costs on the anelastic model, and that the
warm-phase step did not pay for it.

Grids 256 x 256 x 128 and 512 x 512 x 256 over 25.6 km x 25.6 km x 10 km, Float64 and Float32, WENO(order = 5), theta_0 = 300 K: the
reference column crosses T^f near 2.7 km and T^h near 6.8 km.  The state is saturated through the whole column (q^t = 1.3 q^v+ over liquid
of the reference column, a warm bubble and a sheared wind on top), so every cell runs the secant iteration: liquid below, mixed between,
all ice above.
  step     ms per time_step of the mixed-phase model and of the warm-phase model in the same process, alternating windows of `--steps`
           steps after warm-up, `--rounds` windows each (at least 50 steps each in all); median and min-max spread of the windows;
           the mixed-to-warm ratio is reported, not bounded
  parent   (--parent-lib DIR: libbreeze_hip.so / libbreeze_hip_f32.so built from the parent commit) the warm-phase step on this build and
           on the parent's build in the same call, alternating A B B', B B' A, ... (the order rotates); the parent runs as two models (B, B'), and the spread between
           those two repeated runs of the same library is the yardstick: this build's median must not exceed the parent's by more than it
  kernel   ms per launch of the diagnosis-carrying kernel (project_and_diagnose) and of the z-momentum kernel (z_momentum_tendency+rk3)
           from the library's kernel table, their compulsory words per cell (warm 18 and 9: tools/accounting.py with q^v, q^l; mixed 19 and
           10: one more stored field in the diagnosis, one more loaded field in the w kernel), the share of the 8 TB/s roofline, and the
           bound that applies (hbm where the share is above one half; else the kernel is not limited by its compulsory traffic: the
           diagnosis by the pow / exp of its secant iterations, the w kernel by its WENO arithmetic)
One JSON line per measurement, appended to profiles/bench_mixed_phase.jsonl (--out).  No number is fixed in advance.

    python tools/bench_mixed_phase.py [--sizes 256x256x128 512x512x256] [--dtypes f64 f32] [--steps 10] [--rounds 5] [--warmup 3] [--parent-lib DIR]
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
WORDS = {"project_and_diagnose": {"warm": 18, "mixed": 19}, "z_momentum_tendency+rk3": {"warm": 9, "mixed": 10}}


def bind_parent(path):
    """a library of the parent commit under the current binding: every symbol it exports (it has no bz_set_mixed_phase_equilibrium)"""
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
    ap.add_argument("--rounds", type=int, default=5, help="alternating windows per model")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dt", type=float, default=1.0)
    ap.add_argument("--parent-lib", default=None, help="directory with the parent commit's libbreeze_hip.so and libbreeze_hip_f32.so")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_mixed_phase.jsonl"))
    a = ap.parse_args()
    assert a.steps * a.rounds >= 50, "at least 50 steps per model"
    import torch
    import breeze_jl_amd as bz
    from breeze_jl_amd import _lib

    def build(size, ft, mixed, lib_dir=None):
        Nx, Ny, Nz = size
        own = (_lib.LIB_PATH, _lib.F32_LIB_PATH)
        if lib_dir:          # the model binds the library its constructor finds under these names
            _lib.LIB_PATH, _lib.F32_LIB_PATH = os.path.join(lib_dir, "libbreeze_hip.so"), os.path.join(lib_dir, "libbreeze_hip_f32.so")
            for p in (_lib.LIB_PATH, _lib.F32_LIB_PATH):
                if p not in _lib._libs:
                    bind_parent(p)
        try:
            g = bz.RectilinearGrid(size, x=(0.0, 25.6e3), y=(0.0, 25.6e3), z=(0.0, 10e3), float_type=ft)
            ref = bz.ReferenceState(g, potential_temperature=300.0)
            eq = bz.MixedPhaseEquilibrium() if mixed else bz.WarmPhaseEquilibrium()
            m = bz.AtmosphereModel(g, dynamics=bz.AnelasticDynamics(ref), advection=bz.WENO(order=5), microphysics=bz.SaturationAdjustment(equilibrium=eq))
        finally:
            _lib.LIB_PATH, _lib.F32_LIB_PATH = own
        c = m.thermodynamic_constants
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
        m.set(qᵗ=np.minimum(1.3 * qs, 0.03)[:, None, None] * np.ones((Nz, Ny, Nx)), θ=300.0 + 2.0 * np.exp(-r2),
              u=5.0 + 2.0 * np.sin(2 * np.pi * x / 25.6e3)[None, None, :] * np.cos(np.pi * z / 10e3)[:, None, None] * np.ones((Nz, Ny, Nx)))
        return m

    def window(m):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.steps):
            m.time_step(a.dt)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.steps

    def alternate(models):
        for m in models.values():
            for _ in range(a.warmup):
                m.time_step(a.dt)
            m.synchronize()
        ms = {k: [] for k in models}
        keys = list(models)
        for r in range(a.rounds):          # the order rotates from round to round: no model always runs first after the others' last window
            for k in keys[r % len(keys):] + keys[:r % len(keys)]:
                ms[k].append(window(models[k]))
        return {k: dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)), windows=[round(t, 4) for t in v]) for k, v in ms.items()}

    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    for size_s in a.sizes:
        size = tuple(int(n) for n in size_s.split("x"))
        cells = size[0] * size[1] * size[2]
        for dtype in a.dtypes:
            word, ft = (8, np.float64) if dtype == "f64" else (4, np.float32)

            def emit(**kw):
                line = json.dumps({"tool": "bench_mixed_phase", "grid": list(size), "dtype": dtype, "dt": a.dt, **kw})
                print(line, flush=True)
                with open(a.out, "a", encoding="utf-8") as f:
                    f.write(line + "\n")

            models = {"mixed": build(size, ft, True), "warm": build(size, ft, False)}
            t = alternate(models)
            emit(what="step", steps_per_window=a.steps, windows=a.rounds, ms_per_step=t, mixed_over_warm=t["mixed"]["median"] / t["warm"]["median"])
            for phase, m in models.items():
                m.profile_enable(True)
                m.profile_reset()
                for _ in range(a.steps):
                    m.time_step(a.dt)
                m.synchronize()
                prof = m.profile()
                m.profile_enable(False)
                mu = m.microphysical_fields
                ice = float((mu["qⁱ"].interior > 0).double().mean().item()) if phase == "mixed" else 0.0
                liquid = float((mu["qˡ"].interior > 0).double().mean().item())
                for record, words in WORDS.items():
                    ms, calls = prof[record]
                    nbytes = words[phase] * word * cells
                    share = nbytes / (ms / calls * 1e-3) / ROOFLINE
                    emit(what="kernel", phase=phase, record=record, ms_per_launch=ms / calls, launches=calls, compulsory_words_per_cell=words[phase],
                         compulsory_bytes=nbytes, share_of_8TBs=share, bound="hbm" if share > 0.5 else "not its compulsory traffic",
                         cells_with_liquid=liquid, cells_with_ice=ice)
                assert np.isfinite(m.potential_temperature_density.interior_cpu()).all()
            del models
            torch.cuda.empty_cache()
            if a.parent_lib:          # three fresh warm-phase models from the same state: this build, and the parent's build twice
                trio = {"this_build": build(size, ft, False), "parent_a": build(size, ft, False, a.parent_lib), "parent_b": build(size, ft, False, a.parent_lib)}
                t = alternate(trio)
                spread = abs(t["parent_a"]["median"] - t["parent_b"]["median"])
                parent = min(t["parent_a"]["median"], t["parent_b"]["median"])
                emit(what="warm_step_vs_parent", steps_per_window=a.steps, windows=a.rounds, ms_per_step=t, parent_repeat_spread_ms=spread,
                     this_minus_parent_ms=t["this_build"]["median"] - parent, not_slower_than_parent=bool(t["this_build"]["median"] <= parent + spread))
                del trio
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
