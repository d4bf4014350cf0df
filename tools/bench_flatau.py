#!/usr/bin/env python
"""tools/bench_flatau.py — what ThermodynamicConstants(saturation_vapor_pressure = FlatauPolynomial()) changes in the cost of the saturation
adjustments, and that the Clausius-Clapeyron step did not pay for it.

Grids 256 x 256 x 128 and 512 x 512 x 256, Float64 and Float32, WENO(order = 5).  Four cases, each as a polynomial model and a
Clausius-Clapeyron model of the same build, from the same state, in the same process:
  anelastic_warm, anelastic_mixed   the set-up of tools/bench_mixed_phase.py (25.6 km x 25.6 km x 10 km under theta_0 = 300 K, saturated through
                                    the whole column: every cell runs the secant iteration); diagnosing kernel: project_and_diagnose
  compressible_sa                   the mixed bubble of tools/bench_instantaneous_precipitation.py with SaturationAdjustment(WarmPhaseEquilibrium);
                                    diagnosing kernel: the stage epilogue (acoustic_stage_end+update_state[+linearization])
  instantaneous_precipitation       the same bubble with InstantaneousPrecipitation; kernel: instantaneous_precipitation
  step     ms per time_step, alternating windows of `--steps` steps after warm-up, `--rounds` windows per model, the order rotating from round
           to round; median and min-max of the windows; the polynomial-to-Clausius-Clapeyron ratio is reported, not bounded
  kernel   ms per launch of the diagnosing kernel from the library's kernel table (HIP events), its compulsory words per cell and the share of
           the 8 TB/s roofline those bytes make at that time
  parent   (--parent-lib DIR with libbreeze_hip.so / libbreeze_hip_f32.so of the parent commit) the Clausius-Clapeyron step of this build and
           of the parent's build twice (B, B'), rotating; --build-order rotates which model is built (allocated) first, --parent-only skips the rest; the spread between the parent's two repeats is the yardstick: this build's median
           must not exceed the parent's by more than it
One JSON line per measurement, appended to profiles/bench_flatau.jsonl (--out).  No number is fixed in advance.

    python tools/bench_flatau.py [--sizes ...] [--dtypes f64 f32] [--cases ...] [--steps 10] [--rounds 5] [--warmup 3] [--parent-lib DIR]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np

from bench_mixed_phase import bind_parent

ROOFLINE = 8e12      # bytes / s
CASES = ("anelastic_warm", "anelastic_mixed", "compressible_sa", "instantaneous_precipitation")
# compulsory words per cell of the diagnosing kernel: tools/bench_mixed_phase.py (18 / 19), the stage epilogue's single pass
# (csrc/bz_acoustic_kernels.h: 38) and the rain-out kernel (tools/bench_instantaneous_precipitation.py: 7)
RECORDS = {"anelastic_warm": (("project_and_diagnose",), 18), "anelastic_mixed": (("project_and_diagnose",), 19),
           "compressible_sa": (("acoustic_stage_end+update_state", "acoustic_stage_end+update_state+linearization"), 38),
           "instantaneous_precipitation": (("instantaneous_precipitation",), 7)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="+", default=["256x256x128", "512x512x256"])
    ap.add_argument("--dtypes", nargs="+", default=["f64", "f32"], choices=["f64", "f32"])
    ap.add_argument("--cases", nargs="+", default=list(CASES), choices=CASES)
    ap.add_argument("--steps", type=int, default=10, help="steps per timed window")
    ap.add_argument("--rounds", type=int, default=5, help="alternating windows per model")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parent-lib", default=None, help="directory with the parent commit's libbreeze_hip.so and libbreeze_hip_f32.so")
    ap.add_argument("--build-order", type=int, default=0, help="rotate which of the three models of the parent comparison is built first (0: this build)")
    ap.add_argument("--parent-only", action="store_true", help="skip the polynomial measurements: the parent comparison alone")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_flatau.jsonl"))
    a = ap.parse_args()
    import torch
    import breeze_jl_amd as bz
    from breeze_jl_amd import _lib
    from breeze_jl_amd.thermodynamics import dry_air_gas_constant, vapor_gas_constant

    def constants(polynomial):
        return bz.ThermodynamicConstants(saturation_vapor_pressure=bz.FlatauPolynomial()) if polynomial else bz.ThermodynamicConstants()

    def build(case, size, ft, polynomial, lib_dir=None):
        Nx, Ny, Nz = size
        own = (_lib.LIB_PATH, _lib.F32_LIB_PATH)
        if lib_dir:          # the model binds the library its constructor finds under these names
            _lib.LIB_PATH, _lib.F32_LIB_PATH = os.path.join(lib_dir, "libbreeze_hip.so"), os.path.join(lib_dir, "libbreeze_hip_f32.so")
            for p in (_lib.LIB_PATH, _lib.F32_LIB_PATH):
                if p not in _lib._libs:
                    bind_parent(p)
        try:
            if case.startswith("anelastic"):
                g = bz.RectilinearGrid(size, x=(0.0, 25.6e3), y=(0.0, 25.6e3), z=(0.0, 10e3), float_type=ft)
                ref = bz.ReferenceState(g, potential_temperature=300.0)
                eq = bz.MixedPhaseEquilibrium() if case == "anelastic_mixed" else bz.WarmPhaseEquilibrium()
                m = bz.AtmosphereModel(g, dynamics=bz.AnelasticDynamics(ref), advection=bz.WENO(order=5),
                                       microphysics=bz.SaturationAdjustment(equilibrium=eq), thermodynamic_constants=constants(polynomial))
            else:
                Lx, Ly, Lz = 100.0 * Nx, 100.0 * Ny, 3e3
                g = bz.RectilinearGrid(size, x=(0, Lx), y=(0, Ly), z=(0, Lz), float_type=ft)
                dyn = bz.CompressibleDynamics(bz.SplitExplicitTimeDiscretization(), surface_pressure=1e5,
                                              reference_potential_temperature=lambda z: 300.0 * np.exp(9.80616 * z / (1005 * 300.0)))
                mp = (bz.SaturationAdjustment(equilibrium=bz.WarmPhaseEquilibrium()) if case == "compressible_sa"
                      else bz.InstantaneousPrecipitation(equilibrium=bz.WarmPhaseEquilibrium()))
                m = bz.CompressibleAtmosphereModel(g, dyn, advection=bz.WENO(order=5), microphysics=mp, thermodynamic_constants=constants(polynomial))
        finally:
            _lib.LIB_PATH, _lib.F32_LIB_PATH = own
        if case.startswith("anelastic"):
            c = m.thermodynamic_constants
            Rd, Rv = dry_air_gas_constant(c), vapor_gas_constant(c)
            T, p = ref.temperature[g.Hz:g.Hz + g.Nz], ref.pressure[g.Hz:g.Hz + g.Nz]
            dc = c.vapor_heat_capacity - c.liquid_heat_capacity
            L0 = c.liquid_reference_latent_heat - dc * c.energy_reference_temperature
            ps = c.triple_point_pressure * (T / c.triple_point_temperature) ** (dc / Rv) * np.exp((1 / c.triple_point_temperature - 1 / T) * L0 / Rv)
            qs = (Rd / Rv) * ps / (p - ps)
            x, y, z = (np.arange(Nx) + 0.5) * 25.6e3 / Nx, (np.arange(Ny) + 0.5) * 25.6e3 / Ny, (np.arange(Nz) + 0.5) * 10e3 / Nz
            r2 = ((x[None, None, :] - 12.8e3) / 4e3) ** 2 + ((y[None, :, None] - 12.8e3) / 4e3) ** 2 + ((z[:, None, None] - 4e3) / 2e3) ** 2
            m.set(qᵗ=np.minimum(1.3 * qs, 0.03)[:, None, None] * np.ones((Nz, Ny, Nx)), θ=300.0 + 2.0 * np.exp(-r2),
                  u=5.0 + 2.0 * np.sin(2 * np.pi * x / 25.6e3)[None, None, :] * np.cos(np.pi * z / 10e3)[:, None, None] * np.ones((Nz, Ny, Nx)))
            m._bench_dt = 1.0
        else:
            bub = lambda x, y, z: np.maximum(0.0, 1.0 - np.sqrt(((x - 0.5 * Lx) / (0.225 * Lx)) ** 2 + ((y - 0.5 * Ly) / (0.3 * Ly)) ** 2
                                                                + ((z - 0.4 * Lz) / (0.3 * Lz)) ** 2))
            rho = m.dynamics.reference_state.density[g.Hz:g.Hz + g.Nz][:, None, None]
            m.set(ρ=rho, θ=lambda x, y, z: 300.0 + 0.5 * bub(x, y, z), qᵗ=lambda x, y, z: 0.012 + 0.014 * bub(x, y, z) + 0.004 * (z / Lz),
                  u=2.0, v=0.0, w=0.0)
            m._bench_dt = 0.25
        return m

    def window(m):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.steps):
            m.time_step(m._bench_dt)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.steps

    def alternate(models):
        for m in models.values():
            for _ in range(a.warmup):
                m.time_step(m._bench_dt)
            m.synchronize()
        ms = {k: [] for k in models}
        keys = list(models)
        for r in range(a.rounds):          # the order rotates from round to round
            for k in keys[r % len(keys):] + keys[:r % len(keys)]:
                ms[k].append(window(models[k]))
        return {k: dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)), windows=[round(t, 4) for t in v]) for k, v in ms.items()}

    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    for size_s in a.sizes:
        size = tuple(int(n) for n in size_s.split("x"))
        cells = size[0] * size[1] * size[2]
        for dtype in a.dtypes:
            word, ft = (8, np.float64) if dtype == "f64" else (4, np.float32)
            for case in a.cases:
                def emit(**kw):
                    line = json.dumps({"tool": "bench_flatau", "case": case, "grid": list(size), "dtype": dtype, **kw})
                    print(line, flush=True)
                    with open(a.out, "a", encoding="utf-8") as f:
                        f.write(line + "\n")

                if a.parent_only:
                    models = {}
                else:
                    models = {"polynomial": build(case, size, ft, True), "clausius_clapeyron": build(case, size, ft, False)}
                t = alternate(models) if models else None
                if models:
                    emit(what="step", steps_per_window=a.steps, windows=a.rounds, ms_per_step=t,
                         polynomial_over_clausius_clapeyron=t["polynomial"]["median"] / t["clausius_clapeyron"]["median"])
                records, words = RECORDS[case]
                for name, m in models.items():
                    m.profile_enable(True)
                    m.profile_reset()
                    for _ in range(a.steps):
                        m.time_step(m._bench_dt)
                    m.synchronize()
                    prof = m.profile()
                    m.profile_enable(False)
                    ms = sum(prof[r][0] for r in records if r in prof)
                    calls = sum(prof[r][1] for r in records if r in prof)
                    nbytes = words * word * cells
                    emit(what="kernel", formulation=name, records=[r for r in records if r in prof], ms_per_launch=ms / calls, launches=calls,
                         compulsory_words_per_cell=words, compulsory_bytes=nbytes, share_of_8TBs=nbytes / (ms / calls * 1e-3) / ROOFLINE)
                    assert np.isfinite(m.potential_temperature_density.interior_cpu()).all()
                del models
                torch.cuda.empty_cache()
                if a.parent_lib:
                    order = [("this_build", None), ("parent_a", a.parent_lib), ("parent_b", a.parent_lib)]
                    order = order[a.build_order % 3:] + order[:a.build_order % 3]          # the allocation order of the three models rotates with it
                    trio = {k: build(case, size, ft, False, lib) for k, lib in order}
                    t = alternate(trio)
                    spread = abs(t["parent_a"]["median"] - t["parent_b"]["median"])
                    parent = min(t["parent_a"]["median"], t["parent_b"]["median"])
                    emit(what="clausius_clapeyron_step_vs_parent", build_order=[k for k, _ in order], steps_per_window=a.steps, windows=a.rounds, ms_per_step=t, parent_repeat_spread_ms=spread,
                         this_minus_parent_ms=t["this_build"]["median"] - parent, not_slower_than_parent=bool(t["this_build"]["median"] <= parent + spread))
                    del trio
                    torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
