#!/usr/bin/env python
"""tools/bench_compressible_mixed_phase.py — what SaturationAdjustment(equilibrium = MixedPhaseEquilibrium()) costs on the compressible
split-explicit model, and that the warm-phase step did not pay for it.

Grids 256 x 256 x 128 and 512 x 512 x 256 over 25.6 km x 25.6 km x 10 km, Float64 and Float32, WENO(order = 5), 6 substeps, reference
theta = 300 K: the column crosses T^f near 2.7 km and T^h near 6.8 km.  The state is saturated through the whole column (q^t = 1.3 q^v+ over
liquid at the reference column's own density, a warm bubble and a sheared wind on top), so every cell runs the secant iteration: liquid
below, liquid + ice between, all ice above.
  step     ms per time_step of the mixed-phase model and of the warm-phase model in the same process, alternating windows of `--steps`
           steps after warm-up, `--rounds` windows each (at least 50 steps each in all); median and min-max spread of the windows;
           the mixed-to-warm ratio is reported, not bounded
  parent   (--parent-lib DIR: libbreeze_hip.so / libbreeze_hip_f32.so built from the parent commit) the warm-phase step on this build and
           on the parent's build in the same call, the order rotating; the parent runs as two models, and the spread between those two
           repeated runs of the same library is the yardstick: this build's median must lie within it of the faster parent run.  Two trios
           are timed, with this build constructed second and constructed last (the position of a model among the three moves its step);
           the library's own records of one window, this build beside the parent's, follow each (a kernel that changed would show there)
  kernel   ms per launch of the fused stage epilogue (acoustic_stage_end+update_state[+linearization]: k_ac_stage_end) during the steps,
           and of the diagnosis kernel (update_state: k_cmp_diagnose<true, false, MP>) over `--steps` calls of update_state!(compute_tendencies
           = false); their compulsory words per cell — stage epilogue 38 with the linearisation and 34 without it (the count in
           csrc/bz_acoustic_kernels.h) plus the stored fractions, q^v and q^l (warm: + 2) and q^i (mixed: + 3); diagnosis 6 prognostic
           fields read and u, v, w, rho, theta, q, T, p stored (14) plus the same fractions; working fields counted as the grid's real —
           the share of the 8 TB/s roofline, and the bound that applies (hbm where the share is above one half; else the pow / exp of
           the secant and Newton iterations)
One JSON line per measurement, appended to profiles/bench_compressible_mixed_phase.jsonl (--out).  No number is fixed in advance.

    python tools/bench_compressible_mixed_phase.py [--sizes 256x256x128 512x512x256] [--dtypes f64 f32] [--steps 10] [--rounds 5] [--warmup 3]
                                                   [--parent-lib DIR]
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
WORDS = {"acoustic_stage_end+update_state+linearization": {"warm": 40, "mixed": 41}, "acoustic_stage_end+update_state": {"warm": 36, "mixed": 37},
         "update_state": {"warm": 16, "mixed": 17}}


def bind_parent(path):
    """a library of the parent commit under the current binding: every symbol it exports (it has no bz_set_compressible_mixed_phase_equilibrium)"""
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
    ap.add_argument("--dt", type=float, default=None, help="default: 0.005 s per metre of dx (0.5 s at 256 x 256, 0.25 s at 512 x 512: the same acoustic Courant number)")
    ap.add_argument("--parent-lib", default=None, help="directory with the parent commit's libbreeze_hip.so and libbreeze_hip_f32.so")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_compressible_mixed_phase.jsonl"))
    a = ap.parse_args()
    assert a.steps * a.rounds >= 50, "at least 50 steps per model"
    import torch
    import breeze_jl_amd as bz
    from breeze_jl_amd import _lib
    from breeze_jl_amd.thermodynamics import dry_air_gas_constant, vapor_gas_constant

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
            dyn = bz.CompressibleDynamics(bz.SplitExplicitTimeDiscretization(substeps=6), surface_pressure=1e5, reference_potential_temperature=300.0)
            m = bz.CompressibleAtmosphereModel(g, dyn, advection=bz.WENO(order=5), microphysics=bz.SaturationAdjustment(equilibrium=bz.WarmPhaseEquilibrium()))
            if mixed:
                bz.compressible.set_mixed_phase_equilibrium_(m, bz.MixedPhaseEquilibrium())
        finally:
            _lib.LIB_PATH, _lib.F32_LIB_PATH = own
        c, ref = m.thermodynamic_constants, m.dynamics.reference_state
        Rd, Rv = dry_air_gas_constant(c), vapor_gas_constant(c)
        rho = np.asarray(ref.density[g.Hz:g.Hz + g.Nz], dtype=np.float64)
        T = np.asarray(ref.pressure[g.Hz:g.Hz + g.Nz], dtype=np.float64) / (rho * Rd)
        dc = c.vapor_heat_capacity - c.liquid_heat_capacity
        L0 = c.liquid_reference_latent_heat - dc * c.energy_reference_temperature
        ps = c.triple_point_pressure * (T / c.triple_point_temperature) ** (dc / Rv) * np.exp((1 / c.triple_point_temperature - 1 / T) * L0 / Rv)
        qs = ps / (rho * Rv * T)
        x = (np.arange(Nx) + 0.5) * 25.6e3 / Nx
        y = (np.arange(Ny) + 0.5) * 25.6e3 / Ny
        z = (np.arange(Nz) + 0.5) * 10e3 / Nz
        r2 = ((x[None, None, :] - 12.8e3) / 4e3) ** 2 + ((y[None, :, None] - 12.8e3) / 4e3) ** 2 + ((z[:, None, None] - 4e3) / 2e3) ** 2
        m.set(ρ=rho[:, None, None], qᵗ=np.minimum(1.3 * qs, 0.03)[:, None, None] * np.ones((Nz, Ny, Nx)), θ=300.0 + 2.0 * np.exp(-r2), v=0.0, w=0.0,
              u=5.0 + 2.0 * np.sin(2 * np.pi * x / 25.6e3)[None, None, :] * np.cos(np.pi * z / 10e3)[:, None, None] * np.ones((Nz, Ny, Nx)))
        return m

    def window(m, dt):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.steps):
            m.time_step(dt)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.steps

    def alternate(models, dt):
        for m in models.values():
            for _ in range(a.warmup):
                m.time_step(dt)
            m.synchronize()
        ms = {k: [] for k in models}
        keys = list(models)
        for r in range(a.rounds):          # the order rotates from round to round: no model always runs first after the others' last window
            for k in keys[r % len(keys):] + keys[:r % len(keys)]:
                ms[k].append(window(models[k], dt))
        return {k: dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)), windows=[round(t, 4) for t in v]) for k, v in ms.items()}

    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    for size_s in a.sizes:
        size = tuple(int(n) for n in size_s.split("x"))
        cells = size[0] * size[1] * size[2]
        dt = a.dt if a.dt is not None else 0.005 * 25.6e3 / size[0]
        for dtype in a.dtypes:
            word, ft = (8, np.float64) if dtype == "f64" else (4, np.float32)

            def emit(**kw):
                line = json.dumps({"tool": "bench_compressible_mixed_phase", "grid": list(size), "dtype": dtype, "dt": dt, **kw})
                print(line, flush=True)
                with open(a.out, "a", encoding="utf-8") as f:
                    f.write(line + "\n")

            models = {"mixed": build(size, ft, True), "warm": build(size, ft, False)}
            t = alternate(models, dt)
            emit(what="step", steps_per_window=a.steps, windows=a.rounds, ms_per_step=t, mixed_over_warm=t["mixed"]["median"] / t["warm"]["median"])
            for phase, m in models.items():
                m.profile_enable(True)
                m.profile_reset()
                for _ in range(a.steps):
                    m.time_step(dt)
                for _ in range(a.steps):
                    bz.compressible.update_state_(m, compute_tendencies=False)
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
                # (where a model is built among the three moves its step by more than the libraries differ, so this build is timed in the
                # middle and, in a second trio, last: the position the faster parent run had in the first)
                for order in (("parent_a", "this_build", "parent_b"), ("parent_a", "parent_b", "this_build")):
                    trio = {k: build(size, ft, False, None if k == "this_build" else a.parent_lib) for k in order}
                    t = alternate(trio, dt)
                    spread = abs(t["parent_a"]["median"] - t["parent_b"]["median"])
                    parent = min(t["parent_a"]["median"], t["parent_b"]["median"])
                    emit(what="warm_step_vs_parent", build_order=list(order), steps_per_window=a.steps, windows=a.rounds, ms_per_step=t, parent_repeat_spread_ms=spread,
                         this_minus_parent_ms=t["this_build"]["median"] - parent, not_slower_than_parent=bool(t["this_build"]["median"] <= parent + spread))
                    table = {}          # every record of the step, this build against the parent's: a kernel that changed shows here
                    for k in ("this_build", "parent_a"):
                        m = trio[k]
                        m.profile_enable(True)
                        m.profile_reset()
                        for _ in range(a.steps):
                            m.time_step(dt)
                        m.synchronize()
                        for record, (ms, calls) in m.profile().items():
                            table.setdefault(record, {})[k] = round(ms / a.steps, 4)
                        m.profile_enable(False)
                    emit(what="warm_records_vs_parent", build_order=list(order), ms_per_step_by_record=table)
                    del trio, m
                    torch.cuda.empty_cache()
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
