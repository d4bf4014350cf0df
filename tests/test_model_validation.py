"""Configuration errors of the five model constructors, and the struct builders they share.

Every constructor raises its configuration errors before it asks for a GPU, so the table below runs anywhere.  Each row is an invalid
configuration with the exception type and the full message it raises; rows marked "(two checks)" trip two checks at once and so pin the
order of the checks as well.  The messages are literals recorded from the constructors as they stood before the shared host module
(breeze.jl_amd/_context.py) existed; the one message that changed with it, and only by becoming longer, is the compressible model's Kessler
`TetensFormula` error, which now carries the anelastic model's full text."""
import ctypes as C

import numpy as np
import pytest

EXT = dict(x=(0.0, 16e3), y=(0.0, 8e3), z=(0.0, 8e3))


def grid(bz, topology=None, size=None, **kw):
    ext = dict(EXT)
    if topology is not None:
        kw["topology"] = topology
        for d, name in enumerate("xyz"):
            if topology[d] == bz.Flat:
                ext.pop(name)
    return bz.RectilinearGrid(size or (16, 8, 8)[:len(ext)], **ext, **kw)


def anelastic(bz, topology=None, size=None, **kw):
    kw.setdefault("advection", bz.WENO(order=5))
    return bz.AtmosphereModel(grid(bz, topology, size), **kw)


def compressible(bz, topology=None, size=None, model=None, **kw):
    kw.setdefault("advection", bz.WENO(order=5))
    dyn = bz.CompressibleDynamics(bz.SplitExplicitTimeDiscretization())
    return (model or bz.CompressibleAtmosphereModel)(grid(bz, topology, size), dyn, **kw)


def kinematic(bz, topology=None, **kw):
    g = grid(bz, topology)
    return bz.AtmosphereModel(g, dynamics=bz.PrescribedDynamics(bz.ReferenceState(g)), advection=bz.WENO(order=5), **kw)


def slab(bz, cls, topology=None, world=1, **kw):
    from breeze_jl_amd import distributed
    kw.setdefault("advection", bz.WENO(order=5))
    kw.setdefault("device", "cuda:0")      # named, so that no constructor asks torch for the current device before it validates
    g = grid(bz, topology)
    if cls == "SlabCompressibleModel":
        return bz.compressible.SlabCompressibleModel(g, 0, world, bz.CompressibleDynamics(bz.SplitExplicitTimeDiscretization()), **kw)
    return getattr(distributed, cls)(g, 0, world, **kw)


class Unknown:
    pass


def cases(bz):
    P, B, F = bz.Periodic, bz.Bounded, bz.Flat
    PBB, PFB, BFB, BPB, BBB, PPP, FPB = (P, B, B), (P, F, B), (B, F, B), (B, P, B), (B, B, B), (P, P, P), (F, P, B)
    smag, kessler = bz.SmagorinskyLilly(), bz.DCMIP2016KesslerMicrophysics()
    implicit = bz.ScalarDiffusivity(bz.VerticallyImplicitTimeDiscretization(), ν=1.0, κ=1.0)
    diffusivity = bz.ScalarDiffusivity(ν=1.0, κ=1.0)
    sponge = bz.Relaxation(rate=0.01, mask=bz.GaussianMask(7e3, 5e2))
    plain_constants = bz.ThermodynamicConstants()
    sat = bz.SaturationAdjustment(equilibrium=bz.WarmPhaseEquilibrium())
    walls = {"ρv": bz.FieldBoundaryConditions(south=bz.NormalFlowBoundaryCondition(1.0))}
    return {
        # ---- AtmosphereModel ----
        "anelastic/grid_type": lambda: bz.AtmosphereModel("grid"),
        "anelastic/advection_and_momentum_advection": lambda: anelastic(bz, momentum_advection=bz.WENO()),
        "anelastic/velocities_without_prescribed_dynamics": lambda: anelastic(bz, velocities=bz.PrescribedVelocityFields()),
        "anelastic/velocities_and_topology (two checks)": lambda: anelastic(bz, BPB, velocities=bz.PrescribedVelocityFields()),
        "anelastic/topology": lambda: anelastic(bz, BPB),
        "anelastic/topology_and_closure_tuple (two checks)": lambda: anelastic(bz, BBB, closure=(smag,)),
        "anelastic/flat_y_default_advection": lambda: bz.AtmosphereModel(grid(bz, PFB)),
        "anelastic/flat_y_centered": lambda: anelastic(bz, PFB, advection=bz.Centered()),
        "anelastic/bounded_x_odd_Nx": lambda: anelastic(bz, BFB, size=(15, 8)),
        "anelastic/bounded_x_bounds_preserving": lambda: anelastic(bz, BFB, advection={"momentum": bz.WENO(), "ρqᵉ": bz.WENO(bounds=(0, 1))}),
        "anelastic/bounded_y_centered": lambda: anelastic(bz, PBB, advection=bz.Centered()),
        "anelastic/formulation": lambda: anelastic(bz, formulation="Entropy"),
        "anelastic/flat_y_centered_and_formulation (two checks)": lambda: anelastic(bz, PFB, advection=bz.Centered(), formulation="Entropy"),
        "anelastic/timestepper": lambda: anelastic(bz, timestepper="RungeKutta3"),
        "anelastic/closure_tuple": lambda: anelastic(bz, closure=(smag, smag)),
        "anelastic/closure_list": lambda: anelastic(bz, closure=[smag]),
        "anelastic/closure_type": lambda: anelastic(bz, closure=Unknown()),
        "anelastic/closure_tuple_and_microphysics_type (two checks)": lambda: anelastic(bz, closure=(smag,), microphysics=Unknown()),
        "anelastic/timestepper_and_closure_type (two checks)": lambda: anelastic(bz, timestepper="RungeKutta3", closure=Unknown()),
        "anelastic/scalar_diffusivity_between_walls": lambda: anelastic(bz, PBB, closure=diffusivity),
        "anelastic/scalar_diffusivity_bounded_x": lambda: anelastic(bz, BFB, closure=diffusivity),
        "anelastic/microphysics_type": lambda: anelastic(bz, microphysics=Unknown()),
        "anelastic/microphysics_static_energy": lambda: anelastic(bz, microphysics=sat, formulation="StaticEnergy"),
        "anelastic/kessler_without_constants": lambda: anelastic(bz, microphysics=kessler),
        "anelastic/kessler_without_tetens": lambda: anelastic(bz, microphysics=kessler, thermodynamic_constants=plain_constants),
        "anelastic/kessler_without_tetens_static_energy (two checks)": lambda: anelastic(bz, microphysics=kessler, formulation="StaticEnergy"),
        "anelastic/closure_type_and_kessler_without_tetens (two checks)": lambda: anelastic(bz, closure=Unknown(), microphysics=kessler),
        "anelastic/scalar_advection_partially_named": lambda: bz.AtmosphereModel(grid(bz), momentum_advection=bz.WENO(),
                                                                                 scalar_advection={"ρθ": bz.WENO()}),
        "anelastic/scalar_advection_partially_named_with_tracer": lambda: bz.AtmosphereModel(
            grid(bz), momentum_advection=bz.WENO(), scalar_advection={"ρθ": bz.WENO(), "ρqᵉ": bz.WENO()}, tracers=("a",)),
        "anelastic/kessler_without_tetens_and_partial_scalar_advection (two checks)": lambda: bz.AtmosphereModel(
            grid(bz), momentum_advection=bz.WENO(), scalar_advection={"ρθ": bz.WENO()}, microphysics=kessler),
        "anelastic/advection_key": lambda: anelastic(bz, advection={"momentum": bz.WENO(), "ρx": bz.WENO(bounds=(0, 1))}),
        # ---- the kinematic driver ----
        "kinematic/topology": lambda: kinematic(bz, PBB),
        "kinematic/closure": lambda: kinematic(bz, closure=smag),
        "kinematic/velocities": lambda: kinematic(bz, velocities=bz.PrescribedVelocityFields()),
        "kinematic/formulation_and_closure (two checks)": lambda: kinematic(bz, formulation="StaticEnergy", closure=smag),
        # ---- CompressibleAtmosphereModel ----
        "compressible/bare_dynamics": lambda: bz.CompressibleDynamics(),
        "compressible/grid_type": lambda: bz.CompressibleAtmosphereModel("grid", None),
        "compressible/dynamics_type": lambda: bz.CompressibleAtmosphereModel(grid(bz), bz.AnelasticDynamics(None), advection=bz.WENO()),
        "compressible/walls_and_flat": lambda: compressible(bz, BFB),
        "compressible/topology_periodic_z": lambda: compressible(bz, PPP),
        "compressible/topology_flat_x": lambda: compressible(bz, FPB),
        "compressible/topology_and_boundary_conditions (two checks)": lambda: compressible(bz, PPP, boundary_conditions=walls),
        "compressible/topology_and_closure_tuple (two checks)": lambda: compressible(bz, FPB, closure=(smag,)),
        "compressible/boundary_conditions_on_periodic_grid": lambda: compressible(bz, boundary_conditions=walls),
        "compressible/boundary_conditions_and_closure_tuple (two checks)": lambda: compressible(bz, boundary_conditions=walls, closure=(smag,)),
        "compressible/flat_y_default_advection": lambda: bz.CompressibleAtmosphereModel(
            grid(bz, PFB), bz.CompressibleDynamics(bz.SplitExplicitTimeDiscretization())),
        "compressible/flat_y_centered": lambda: compressible(bz, PFB, advection=bz.Centered()),
        "compressible/weno9_halo": lambda: compressible(bz, advection=bz.WENO(order=9)),
        "compressible/weno9_halo_and_closure_type (two checks)": lambda: compressible(bz, advection=bz.WENO(order=9), closure=Unknown()),
        "compressible/closure_tuple": lambda: compressible(bz, closure=(smag, smag)),
        "compressible/closure_type": lambda: compressible(bz, closure=Unknown()),
        "compressible/closure_vertically_implicit": lambda: compressible(bz, closure=implicit),
        "compressible/closure_vertically_implicit_between_walls (two checks)": lambda: compressible(bz, PBB, closure=implicit),
        "compressible/closure_between_walls": lambda: compressible(bz, PBB, closure=smag),
        "compressible/closure_flat_y": lambda: compressible(bz, PFB, closure=diffusivity),
        "compressible/closure_tuple_and_coriolis (two checks)": lambda: compressible(bz, closure=(smag,), coriolis=Unknown()),
        "compressible/coriolis_type": lambda: compressible(bz, coriolis=Unknown()),
        "compressible/column_forcing": lambda: compressible(bz, forcing={"θ": bz.Forcing(lambda z: 0.0)}),
        "compressible/sponge_on_moisture": lambda: compressible(bz, forcing={"ρqᵗ": sponge}),
        "compressible/sponge_on_velocity": lambda: compressible(bz, forcing={"u": sponge}),
        "compressible/coriolis_and_sponge_on_moisture (two checks)": lambda: compressible(bz, coriolis=Unknown(), forcing={"ρqᵗ": sponge}),
        "compressible/microphysics_type": lambda: compressible(bz, microphysics=Unknown()),
        "compressible/sponge_on_moisture_and_microphysics_type (two checks)": lambda: compressible(bz, forcing={"ρqᵗ": sponge}, microphysics=Unknown()),
        "compressible/kessler_without_constants": lambda: compressible(bz, microphysics=kessler),
        "compressible/kessler_without_tetens": lambda: compressible(bz, microphysics=kessler, thermodynamic_constants=plain_constants),
        "compressible/coriolis_and_kessler_without_tetens (two checks)": lambda: compressible(bz, coriolis=Unknown(), microphysics=kessler),
        # ---- the three slab constructors ----
        "SlabAtmosphereModel/topology": lambda: slab(bz, "SlabAtmosphereModel", PBB),
        "SlabAtmosphereModel/advection": lambda: slab(bz, "SlabAtmosphereModel", advection=bz.WENO(order=9)),
        "SlabAtmosphereModel/divisibility": lambda: slab(bz, "SlabAtmosphereModel", world=3),
        "SlabAtmosphereModel/topology_and_divisibility (two checks)": lambda: slab(bz, "SlabAtmosphereModel", PBB, world=3),
        "SlabAtmosphereModel/advection_and_divisibility (two checks)": lambda: slab(bz, "SlabAtmosphereModel", advection=None, world=3),
        "LibrarySlabAtmosphereModel/prescribed_dynamics": lambda: slab(bz, "LibrarySlabAtmosphereModel", dynamics=bz.PrescribedDynamics(None)),
        "LibrarySlabAtmosphereModel/topology": lambda: slab(bz, "LibrarySlabAtmosphereModel", PFB),
        "LibrarySlabAtmosphereModel/divisibility": lambda: slab(bz, "LibrarySlabAtmosphereModel", world=3),
        "LibrarySlabAtmosphereModel/topology_and_divisibility (two checks)": lambda: slab(bz, "LibrarySlabAtmosphereModel", PBB, world=3),
        "LibrarySlabAtmosphereModel/torch_transport": lambda: slab(bz, "LibrarySlabAtmosphereModel", transport="torch"),
        "LibrarySlabAtmosphereModel/divisibility_and_torch_transport (two checks)": lambda: slab(bz, "LibrarySlabAtmosphereModel", world=3,
                                                                                                 transport="torch"),
        "LibrarySlabAtmosphereModel/scalar_diffusivity": lambda: slab(bz, "LibrarySlabAtmosphereModel", closure=diffusivity),
        "SlabCompressibleModel/topology": lambda: slab(bz, "SlabCompressibleModel", PBB),
        "SlabCompressibleModel/divisibility": lambda: slab(bz, "SlabCompressibleModel", world=3),
        "SlabCompressibleModel/topology_and_divisibility (two checks)": lambda: slab(bz, "SlabCompressibleModel", PFB, world=3),
        "SlabCompressibleModel/substep_float32_torch_transport": lambda: slab(bz, "SlabCompressibleModel", substep_floattype=np.float32),
        "SlabCompressibleModel/closure": lambda: slab(bz, "SlabCompressibleModel", closure=smag),
        "SlabCompressibleModel/coriolis": lambda: slab(bz, "SlabCompressibleModel", coriolis=bz.FPlane(f=1e-4)),
        "SlabCompressibleModel/divisibility_and_closure (two checks)": lambda: slab(bz, "SlabCompressibleModel", world=3, closure=smag),
    }


EXPECTED = {
    "anelastic/grid_type": (TypeError,
        "grid must be a RectilinearGrid"),
    "anelastic/advection_and_momentum_advection": (ValueError,
        "pass either `advection` or `momentum_advection` / `scalar_advection`"),
    "anelastic/velocities_without_prescribed_dynamics": (ValueError,
        "`velocities` belongs to AtmosphereModel(dynamics = PrescribedDynamics(...))"),
    "anelastic/velocities_and_topology (two checks)": (ValueError,
        "`velocities` belongs to AtmosphereModel(dynamics = PrescribedDynamics(...))"),
    "anelastic/topology": (NotImplementedError,
        "the HIP path implements topology (Periodic, Periodic, Bounded), (Periodic, Flat, Bounded), (Bounded, "
        "Flat, Bounded) and (Periodic, Bounded, Bounded)"),
    "anelastic/topology_and_closure_tuple (two checks)": (NotImplementedError,
        "the HIP path implements topology (Periodic, Periodic, Bounded), (Periodic, Flat, Bounded), (Bounded, "
        "Flat, Bounded) and (Periodic, Bounded, Bounded)"),
    "anelastic/flat_y_default_advection": (NotImplementedError,
        "(Periodic, Flat, Bounded): WENO(order = 5 | 7 | 9) models are implemented"),
    "anelastic/flat_y_centered": (NotImplementedError,
        "(Periodic, Flat, Bounded): WENO(order = 5 | 7 | 9) models are implemented"),
    "anelastic/bounded_x_odd_Nx": (NotImplementedError,
        "(Bounded, Flat, Bounded): WENO(order = 5 | 7 | 9) models without bounds-preserving advection on an even "
        "number of columns are implemented"),
    "anelastic/bounded_x_bounds_preserving": (NotImplementedError,
        "(Bounded, Flat, Bounded): WENO(order = 5 | 7 | 9) models without bounds-preserving advection on an even "
        "number of columns are implemented"),
    "anelastic/bounded_y_centered": (NotImplementedError,
        "(Periodic, Bounded, Bounded): WENO(order = 5 | 7 | 9) models without bounds-preserving advection are "
        "implemented"),
    "anelastic/formulation": (NotImplementedError,
        "formulation 'Entropy' is not implemented"),
    "anelastic/flat_y_centered_and_formulation (two checks)": (NotImplementedError,
        "(Periodic, Flat, Bounded): WENO(order = 5 | 7 | 9) models are implemented"),
    "anelastic/timestepper": (NotImplementedError,
        "only SSPRungeKutta3 is implemented"),
    "anelastic/closure_tuple": (NotImplementedError,
        "closure: one closure is implemented (no closure tuples)"),
    "anelastic/closure_list": (NotImplementedError,
        "closure: one closure is implemented (no closure tuples)"),
    "anelastic/closure_type": (NotImplementedError,
        "closure: SmagorinskyLilly(), ScalarDiffusivity(...) and VerticalScalarDiffusivity(...) are implemented"),
    "anelastic/closure_tuple_and_microphysics_type (two checks)": (NotImplementedError,
        "closure: one closure is implemented (no closure tuples)"),
    "anelastic/timestepper_and_closure_type (two checks)": (NotImplementedError,
        "only SSPRungeKutta3 is implemented"),
    "anelastic/scalar_diffusivity_between_walls": (NotImplementedError,
        "closure = ScalarDiffusivity / VerticalScalarDiffusivity: not implemented between walls in x or y (Bounded "
        "x / Bounded y)"),
    "anelastic/scalar_diffusivity_bounded_x": (NotImplementedError,
        "closure = ScalarDiffusivity / VerticalScalarDiffusivity: not implemented between walls in x or y (Bounded "
        "x / Bounded y)"),
    "anelastic/microphysics_type": (NotImplementedError,
        "microphysics: SaturationAdjustment(equilibrium = WarmPhaseEquilibrium()) and "
        "DCMIP2016KesslerMicrophysics() are implemented"),
    "anelastic/microphysics_static_energy": (NotImplementedError,
        "microphysics is implemented for the potential-temperature formulation"),
    "anelastic/kessler_without_constants": (ValueError,
        "DCMIP2016KesslerMicrophysics requires `thermodynamic_constants` with a `TetensFormula` saturation vapor "
        "pressure formulation. Construct the model with, e.g., `thermodynamic_constants = "
        "ThermodynamicConstants(saturation_vapor_pressure = TetensFormula())`."),
    "anelastic/kessler_without_tetens": (ValueError,
        "DCMIP2016KesslerMicrophysics requires `thermodynamic_constants` with a `TetensFormula` saturation vapor "
        "pressure formulation. Construct the model with, e.g., `thermodynamic_constants = "
        "ThermodynamicConstants(saturation_vapor_pressure = TetensFormula())`."),
    "anelastic/kessler_without_tetens_static_energy (two checks)": (NotImplementedError,
        "microphysics is implemented for the potential-temperature formulation"),
    "anelastic/closure_type_and_kessler_without_tetens (two checks)": (NotImplementedError,
        "closure: SmagorinskyLilly(), ScalarDiffusivity(...) and VerticalScalarDiffusivity(...) are implemented"),
    "anelastic/scalar_advection_partially_named": (NotImplementedError,
        'scalar_advection names only some scalars: the others would take Centered(order = 2), and one order for '
        "all scalars is implemented (unnamed: ['moisture'])"),
    "anelastic/scalar_advection_partially_named_with_tracer": (NotImplementedError,
        'scalar_advection names only some scalars: the others would take Centered(order = 2), and one order for '
        "all scalars is implemented (unnamed: ['a'])"),
    "anelastic/kessler_without_tetens_and_partial_scalar_advection (two checks)": (ValueError,
        "DCMIP2016KesslerMicrophysics requires `thermodynamic_constants` with a `TetensFormula` saturation vapor "
        "pressure formulation. Construct the model with, e.g., `thermodynamic_constants = "
        "ThermodynamicConstants(saturation_vapor_pressure = TetensFormula())`."),
    "anelastic/advection_key": (ValueError,
        "advection key 'ρx' names no prognostic scalar of this model"),
    "kinematic/topology": (NotImplementedError,
        "AtmosphereModel(dynamics = PrescribedDynamics(...)): topology ('Periodic', 'Bounded', 'Bounded') is not "
        'implemented'),
    "kinematic/closure": (NotImplementedError,
        "AtmosphereModel(dynamics = PrescribedDynamics(...)): a closure is not implemented"),
    "kinematic/velocities": (NotImplementedError,
        "AtmosphereModel(dynamics = PrescribedDynamics(...)): PrescribedVelocityFields (velocities as functions of "
        "time) is not implemented"),
    "kinematic/formulation_and_closure (two checks)": (NotImplementedError,
        "AtmosphereModel(dynamics = PrescribedDynamics(...)): the StaticEnergy formulation is not implemented"),
    "compressible/bare_dynamics": (NotImplementedError,
        "the HIP path implements CompressibleDynamics(SplitExplicitTimeDiscretization(...)); ExplicitTimeStepping "
        "is outside the hot-path scope"),
    "compressible/grid_type": (TypeError,
        "grid must be a RectilinearGrid"),
    "compressible/dynamics_type": (TypeError,
        "dynamics must be CompressibleDynamics"),
    "compressible/walls_and_flat": (NotImplementedError,
        "Bounded x / y of the compressible model: 3-D grids on one device"),
    "compressible/topology_periodic_z": (NotImplementedError,
        "the HIP path implements topology (Periodic, Periodic, Bounded) and (Periodic, Flat, Bounded)"),
    "compressible/topology_flat_x": (NotImplementedError,
        "the HIP path implements topology (Periodic, Periodic, Bounded) and (Periodic, Flat, Bounded)"),
    "compressible/topology_and_boundary_conditions (two checks)": (NotImplementedError,
        "the HIP path implements topology (Periodic, Periodic, Bounded) and (Periodic, Flat, Bounded)"),
    "compressible/topology_and_closure_tuple (two checks)": (NotImplementedError,
        "the HIP path implements topology (Periodic, Periodic, Bounded) and (Periodic, Flat, Bounded)"),
    "compressible/boundary_conditions_on_periodic_grid": (NotImplementedError,
        "boundary_conditions: the open lateral boundaries of the acoustic substep loop on a Bounded x / y"),
    "compressible/boundary_conditions_and_closure_tuple (two checks)": (NotImplementedError,
        "boundary_conditions: the open lateral boundaries of the acoustic substep loop on a Bounded x / y"),
    "compressible/flat_y_default_advection": (NotImplementedError,
        "(Periodic, Flat, Bounded): the WENO(order = 5 | 7 | 9) model is implemented"),
    "compressible/flat_y_centered": (NotImplementedError,
        "(Periodic, Flat, Bounded): the WENO(order = 5 | 7 | 9) model is implemented"),
    "compressible/weno9_halo": (ValueError,
        "WENO(order=9) needs halos of at least 5 cells in every direction"),
    "compressible/weno9_halo_and_closure_type (two checks)": (ValueError,
        "WENO(order=9) needs halos of at least 5 cells in every direction"),
    "compressible/closure_tuple": (NotImplementedError,
        "closure: one closure is implemented (no closure tuples)"),
    "compressible/closure_type": (NotImplementedError,
        "closure = Unknown: SmagorinskyLilly(), ScalarDiffusivity(...) and VerticalScalarDiffusivity(...) are "
        "implemented"),
    "compressible/closure_vertically_implicit": (NotImplementedError,
        "closure with VerticallyImplicitTimeDiscretization: CompressibleDynamics runs the closures with "
        "ExplicitTimeDiscretization (the implicit substep of the reference is not built)"),
    "compressible/closure_vertically_implicit_between_walls (two checks)": (NotImplementedError,
        "closure with VerticallyImplicitTimeDiscretization: CompressibleDynamics runs the closures with "
        "ExplicitTimeDiscretization (the implicit substep of the reference is not built)"),
    "compressible/closure_between_walls": (NotImplementedError,
        "closure: not implemented on a compressible model between walls (Bounded x / Bounded y)"),
    "compressible/closure_flat_y": (NotImplementedError,
        "closure: not implemented on a compressible model with a Flat y"),
    "compressible/closure_tuple_and_coriolis (two checks)": (NotImplementedError,
        "closure: one closure is implemented (no closure tuples)"),
    "compressible/coriolis_type": (NotImplementedError,
        "coriolis: FPlane is implemented"),
    "compressible/column_forcing": (NotImplementedError,
        "CompressibleDynamics: Relaxation sponges keyed ρu, ρv, ρw, ρθ and a 3-D Forcing on θ / ρθ are the "
        "forcings implemented"),
    "compressible/sponge_on_moisture": (NotImplementedError,
        "CompressibleDynamics: Relaxation sponges keyed ρu, ρv, ρw, ρθ"),
    "compressible/sponge_on_velocity": (NotImplementedError,
        "CompressibleDynamics: Relaxation sponges keyed ρu, ρv, ρw, ρθ"),
    "compressible/coriolis_and_sponge_on_moisture (two checks)": (NotImplementedError,
        "coriolis: FPlane is implemented"),
    "compressible/microphysics_type": (NotImplementedError,
        "compressible microphysics: DCMIP2016KesslerMicrophysics() and SaturationAdjustment(equilibrium = "
        "WarmPhaseEquilibrium()) are implemented"),
    "compressible/sponge_on_moisture_and_microphysics_type (two checks)": (NotImplementedError,
        "CompressibleDynamics: Relaxation sponges keyed ρu, ρv, ρw, ρθ"),
    "compressible/kessler_without_constants": (ValueError,
        "DCMIP2016KesslerMicrophysics requires `thermodynamic_constants` with a `TetensFormula` saturation vapor "
        "pressure formulation. Construct the model with, e.g., `thermodynamic_constants = "
        "ThermodynamicConstants(saturation_vapor_pressure = TetensFormula())`."),      # (the anelastic model's full text)
    "compressible/kessler_without_tetens": (ValueError,
        "DCMIP2016KesslerMicrophysics requires `thermodynamic_constants` with a `TetensFormula` saturation vapor "
        "pressure formulation. Construct the model with, e.g., `thermodynamic_constants = "
        "ThermodynamicConstants(saturation_vapor_pressure = TetensFormula())`."),      # (the anelastic model's full text)
    "compressible/coriolis_and_kessler_without_tetens (two checks)": (NotImplementedError,
        "coriolis: FPlane is implemented"),
    "SlabAtmosphereModel/topology": (NotImplementedError,
        "slab decomposition implements topology (Periodic, Periodic, Bounded)"),
    "SlabAtmosphereModel/advection": (NotImplementedError,
        "the HIP path requires advection=WENO(order=5)"),
    "SlabAtmosphereModel/divisibility": (ValueError,
        "Ny=8 is not divisible by 3 ranks"),
    "SlabAtmosphereModel/topology_and_divisibility (two checks)": (NotImplementedError,
        "slab decomposition implements topology (Periodic, Periodic, Bounded)"),
    "SlabAtmosphereModel/advection_and_divisibility (two checks)": (NotImplementedError,
        "the HIP path requires advection=WENO(order=5)"),
    "LibrarySlabAtmosphereModel/prescribed_dynamics": (NotImplementedError,
        "AtmosphereModel(dynamics = PrescribedDynamics(...)): y-slab (distributed) models are not implemented"),
    "LibrarySlabAtmosphereModel/topology": (NotImplementedError,
        "slab decomposition implements topology (Periodic, Periodic, Bounded)"),
    "LibrarySlabAtmosphereModel/divisibility": (ValueError,
        "Ny=8 is not divisible by 3 ranks"),
    "LibrarySlabAtmosphereModel/topology_and_divisibility (two checks)": (NotImplementedError,
        "slab decomposition implements topology (Periodic, Periodic, Bounded)"),
    "LibrarySlabAtmosphereModel/torch_transport": (ValueError,
        'LibrarySlabAtmosphereModel runs on the library-owned communicator: transport "rccl" or "local:<name>"'),
    "LibrarySlabAtmosphereModel/divisibility_and_torch_transport (two checks)": (ValueError,
        "Ny=8 is not divisible by 3 ranks"),
    "LibrarySlabAtmosphereModel/scalar_diffusivity": (NotImplementedError,
        "closure = ScalarDiffusivity / VerticalScalarDiffusivity: not implemented on y-slab (distributed) models"),
    "SlabCompressibleModel/topology": (NotImplementedError,
        "slab decomposition implements topology (Periodic, Periodic, Bounded)"),
    "SlabCompressibleModel/divisibility": (ValueError,
        "Ny=8 is not divisible by 3 ranks"),
    "SlabCompressibleModel/topology_and_divisibility (two checks)": (NotImplementedError,
        "slab decomposition implements topology (Periodic, Periodic, Bounded)"),
    "SlabCompressibleModel/substep_float32_torch_transport": (NotImplementedError,
        'substep_floattype = Float32 on y-slabs: transport "rccl" or "local:<name>"'),
    "SlabCompressibleModel/closure": (NotImplementedError,
        "closure: not implemented on y-slab (distributed) compressible models"),
    "SlabCompressibleModel/coriolis": (NotImplementedError,
        "Coriolis and sponges of the compressible model: single-GPU contexts"),
    "SlabCompressibleModel/divisibility_and_closure (two checks)": (ValueError,
        "Ny=8 is not divisible by 3 ranks"),
}


def test_every_case_has_a_recorded_message(bz):
    assert sorted(cases(bz)) == sorted(EXPECTED)


@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_invalid_configuration_raises_its_message(bz, name):
    kind, message = EXPECTED[name]
    with pytest.raises(Exception) as info:
        cases(bz)[name]()
    assert (type(info.value), str(info.value)) == (kind, message)


# ---- the struct builders the constructors share (breeze.jl_amd/_context.py) ----
STRETCHED = np.array([0.0, 300.0, 700.0, 1300.0, 2100.0, 3200.0, 4600.0, 6300.0, 8000.0])


@pytest.mark.parametrize("float_type", [np.float64, np.float32])
@pytest.mark.parametrize("z", [(0.0, 8e3), STRETCHED], ids=["regular_z", "stretched_z"])
def test_grid_struct_mirrors_the_grid(bz, float_type, z):
    import gc
    from breeze_jl_amd import _context, _lib
    g = bz.RectilinearGrid((16, 8, 8), x=(0.0, 16e3), y=(-1e3, 7e3), z=z, halo=(3, 4, 5), topology=(bz.Periodic, bz.Bounded, bz.Bounded),
                           float_type=float_type)
    T = _lib.types(g.ftype)
    real = C.c_double if float_type is np.float64 else C.c_float
    assert T.real is real and np.dtype(T.np_real) == np.dtype(float_type)
    bg, zf = _context.grid_struct(T, g)
    assert type(bg) is T.bz_grid and dict(type(bg)._fields_)["dx"] is real and dict(type(bg)._fields_)["zf"] is C.POINTER(real)
    assert (type(bg) is _lib.bz_grid) == (float_type is np.float64)      # Float32 grids get the _lib.types(4) mirror, not the Float64 struct
    assert (bg.Nx, bg.Ny, bg.Nz, bg.Hx, bg.Hy, bg.Hz) == (16, 8, 8, 3, 4, 5)
    assert tuple(bg.topo) == g.topology_codes() == (0, 1, 1)
    assert bg.ftype == g.ftype == np.dtype(float_type).itemsize
    assert (bg.dx, bg.dy) == (real(g.Δx).value, real(g.Δy).value) == (1000.0, 1000.0)
    assert bg.regular_z == (1 if isinstance(z, tuple) else 0) and bg.reserved == 0
    assert zf.dtype == np.dtype(float_type) and zf.flags["C_CONTIGUOUS"] and zf.shape == (9,)
    assert np.array_equal(zf, np.asarray(g.zᶠ, dtype=float_type))
    assert C.addressof(bg.zf.contents) == zf.ctypes.data      # the struct points INTO the keep-alive ...
    expected = zf.copy()
    del g
    gc.collect()
    junk = [np.full(9, -1.0, dtype=float_type) for _ in range(64)]      # ... which is what keeps those bytes: nothing else holds them
    assert np.array_equal(np.ctypeslib.as_array(bg.zf, shape=(9,)), expected) and junk


@pytest.mark.parametrize("ftype", [8, 4])
def test_constants_struct_holds_the_five_constants(bz, ftype):
    from breeze_jl_amd import _context, _lib
    from breeze_jl_amd.thermodynamics import dry_air_gas_constant, vapor_gas_constant
    c = bz.ThermodynamicConstants()
    T = _lib.types(ftype)
    bc = _context.constants_struct(T, c)
    assert type(bc) is T.bz_constants and (type(bc) is _lib.bz_constants) == (ftype == 8)
    want = (c.gravitational_acceleration, dry_air_gas_constant(c), vapor_gas_constant(c), c.dry_air_heat_capacity, c.vapor_heat_capacity)
    got = tuple(getattr(bc, name) for name, _ in type(bc)._fields_)
    assert len(got) == 5 and got == tuple(T.real(w).value for w in want)
    if ftype == 8:
        assert got == want
