"""ctypes binding of libbreeze_hip.so (C ABI declared in include/breeze_hip.h).

The product path has no CPU fallback: if the HIP library is missing or fails to load, importing
this module's `load()` raises.  Nothing here imports the test oracle.
"""
import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
# BREEZE_HIP_LIB selects another build of the same ABI (e.g. lib/libbreeze_hip_refdiv.so, the variant that
# keeps the reference's three-quotient WENO weight formula, used for A/B timing and tight parity checks).
LIB_PATH = os.environ.get("BREEZE_HIP_LIB") or os.path.join(_HERE, "lib", "libbreeze_hip.so")
CSRC = os.path.join(_HERE, "csrc")

_dp = C.POINTER(C.c_double)
BZ_UNIQUE_ID_BYTES = 128


class bz_grid(C.Structure):
    _fields_ = [("Nx", C.c_int32), ("Ny", C.c_int32), ("Nz", C.c_int32),
                ("Hx", C.c_int32), ("Hy", C.c_int32), ("Hz", C.c_int32),
                ("topo", C.c_int32 * 3), ("ftype", C.c_int32),
                ("dx", C.c_double), ("dy", C.c_double),
                ("zf", _dp), ("regular_z", C.c_int32), ("reserved", C.c_int32)]


class bz_constants(C.Structure):
    _fields_ = [("gravitational_acceleration", C.c_double),
                ("dry_air_gas_constant", C.c_double),
                ("vapor_gas_constant", C.c_double),
                ("dry_air_heat_capacity", C.c_double),
                ("vapor_heat_capacity", C.c_double)]


class bz_reference_state(C.Structure):
    _fields_ = [("surface_pressure", C.c_double), ("potential_temperature", C.c_double),
                ("standard_pressure", C.c_double),
                ("density", _dp), ("pressure", _dp), ("temperature", _dp)]


_STATE_FIELDS = ("rho_u", "rho_v", "rho_w", "rho_theta", "rho_q", "u", "v", "w", "theta", "q", "T", "phi")
_PROG_FIELDS = ("rho_u", "rho_v", "rho_w", "rho_theta", "rho_q")


class bz_state(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in _STATE_FIELDS]


class bz_prognostic(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in _PROG_FIELDS]


class bz_saturation_adjustment(C.Structure):
    _fields_ = [("liquid_latent_heat", C.c_double), ("liquid_heat_capacity", C.c_double),
                ("energy_reference_temperature", C.c_double), ("triple_point_temperature", C.c_double),
                ("triple_point_pressure", C.c_double), ("abstol", C.c_double), ("maxiter", C.c_int32),
                ("reserved", C.c_int32)]


class bz_mixed_phase_equilibrium(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("freezing_temperature", "homogeneous_ice_nucleation_temperature", "ice_latent_heat",
                                          "ice_heat_capacity")]


class bz_flatau_polynomial(C.Structure):
    _fields_ = [("liquid_coefficients", C.c_double * 9), ("ice_coefficients", C.c_double * 9),
                ("reference_temperature", C.c_double), ("minimum_temperature_offset", C.c_double)]


class bz_negative_moisture_correction(C.Structure):
    """Descriptor of bz_set_negative_moisture_correction: the two phases, the species chain (heaviest first), the (number, mass) pairs and the
    clamped number fields, every array a device parent array.  Pointers and counts only: one struct for both precisions."""
    _fields_ = [("species_borrowing", C.c_int32), ("vertical_borrowing", C.c_int32),
                ("n_mass", C.c_int32), ("n_pairs", C.c_int32), ("n_clamp", C.c_int32), ("reserved", C.c_int32),
                ("mass", C.c_void_p * 4), ("number", C.c_void_p * 4), ("pair_mass", C.c_void_p * 4), ("clamp", C.c_void_p * 4)]


class bz_bulk_surface_fluxes(C.Structure):
    _fields_ = [(n, C.c_double) for n in (
        "drag_coefficient", "drag_gustiness", "drag_surface_temperature",
        "heat_coefficient", "heat_gustiness", "heat_surface_temperature",
        "vapor_coefficient", "vapor_gustiness", "vapor_surface_temperature",
        "surface_pressure", "standard_pressure",
        "liquid_latent_heat", "liquid_heat_capacity", "energy_reference_temperature", "triple_point_temperature",
        "triple_point_pressure")]


_MAPPING_FIELDS = ("stable_unstable_transition", "strongly_stable_transition", "au11", "bu11", "bu12", "au21", "au22", "bu31", "bu32", "bu33",
                   "aw11", "aw12", "aw21", "aw22", "bw11", "bw12", "bw21", "bw22", "as11", "as21", "bs11", "bs21", "bs22")
_PSI_FIELDS = ("gamma_d", "gamma_t", "psi_a", "psi_b", "psi_c", "psi_d")


class bz_polynomial_coefficient(C.Structure):
    _fields_ = ([(n, C.c_double) for n in ("a0", "a1", "a2", "roughness_length", "minimum_wind_speed")] +
                [("stability", C.c_int32), ("reserved", C.c_int32), ("scalar_roughness_length", C.c_double)] +
                [(n, C.c_double) for n in _MAPPING_FIELDS + _PSI_FIELDS])


class bz_surface_flux(C.Structure):
    _fields_ = [("enabled", C.c_int32), ("polynomial", C.c_int32), ("coefficient", C.c_double), ("gustiness", C.c_double),
                ("surface_temperature", C.c_double), ("surface_temperature_field", _dp), ("poly", bz_polynomial_coefficient)]


class bz_surface_layer(C.Structure):
    _fields_ = ([("drag", bz_surface_flux), ("heat", bz_surface_flux), ("vapor", bz_surface_flux)] +
                [(n, C.c_double) for n in ("surface_pressure", "standard_pressure", "liquid_latent_heat", "liquid_heat_capacity",
                                           "energy_reference_temperature", "triple_point_temperature", "triple_point_pressure")] +
                [("filtered", C.c_int32), ("filter_height_set", C.c_int32), ("filter_height", C.c_double), ("filter_timescale", C.c_double),
                 ("filter_stage_mask", C.c_int32), ("reserved", C.c_int32)])


class bz_compressible_surface_flux(C.Structure):
    _fields_ = [("enabled", C.c_int32), ("reserved", C.c_int32), ("coefficient", C.c_double), ("gustiness", C.c_double),
                ("surface_temperature", C.c_double), ("surface_temperature_field", _dp)]


class bz_compressible_surface_fluxes(C.Structure):
    _fields_ = ([("drag", bz_compressible_surface_flux), ("heat", bz_compressible_surface_flux), ("vapor", bz_compressible_surface_flux)] +
                [(n, C.c_double) for n in ("surface_pressure", "standard_pressure", "liquid_latent_heat", "liquid_heat_capacity",
                                           "energy_reference_temperature", "triple_point_temperature", "triple_point_pressure")])


class bz_tracer_fields(C.Structure):
    _fields_ = [("density", C.c_void_p), ("specific", C.c_void_p), ("U0", C.c_void_p), ("G", C.c_void_p)]


class bz_bounds_preserving_advection(C.Structure):
    _fields_ = [("lower", C.c_double), ("upper", C.c_double), ("moisture", C.c_int32), ("microphysical_species", C.c_int32),
                ("tracers", C.c_int32), ("reserved", C.c_int32)]


class bz_smagorinsky_lilly(C.Structure):
    _fields_ = [("smagorinsky_coefficient", C.c_double), ("reduction_factor", C.c_double), ("prandtl_number", C.c_double)]


class bz_scalar_diffusivity(C.Structure):
    _fields_ = [("formulation", C.c_int32), ("time_discretization", C.c_int32), ("nu", C.c_double), ("kappa", C.c_double)]


class bz_column_forcings(C.Structure):
    _fields_ = [("u_forcing", _dp), ("v_forcing", _dp), ("theta_forcing", _dp), ("moisture_forcing", _dp),
                ("energy_forcing", _dp), ("subsidence_vertical_velocity", _dp),
                ("subsidence_u", C.c_int32), ("subsidence_v", C.c_int32), ("subsidence_theta", C.c_int32),
                ("subsidence_moisture", C.c_int32), ("coriolis_f", C.c_double),
                ("bottom_theta_flux", C.c_double), ("bottom_moisture_flux", C.c_double),
                ("bottom_drag_rho0_ustar2", C.c_double), ("bottom_drag_epsilon", C.c_double),
                ("bottom_energy_flux", C.c_double)]


class bz_column_relaxation(C.Structure):
    _fields_ = [(f"{a}_{b}", _dp) for b in ("u", "v", "w", "theta", "moisture") for a in ("rate", "target")] + [("specific_mask", C.c_int32)]


_KESSLER_PARAMS = ("dcmip_temperature_scale", "terminal_velocity_coefficient", "density_scale", "terminal_velocity_exponent",
                   "autoconversion_rate", "autoconversion_threshold", "accretion_rate", "accretion_exponent",
                   "evaporation_ventilation_coefficient_1", "evaporation_ventilation_coefficient_2",
                   "evaporation_ventilation_exponent_1", "evaporation_ventilation_exponent_2", "diffusivity_coefficient",
                   "thermal_conductivity_coefficient", "substep_cfl", "tetens_reference_saturation_vapor_pressure",
                   "tetens_reference_temperature", "tetens_liquid_coefficient", "tetens_liquid_temperature_offset",
                   "liquid_latent_heat", "liquid_heat_capacity")
_KESSLER_FIELDS = ("density", "pressure", "potential_temperature", "potential_temperature_density", "moisture_density",
                   "cloud_liquid_density", "rain_density", "vapor_mass_fraction", "cloud_liquid_mass_fraction",
                   "rain_mass_fraction", "rain_terminal_velocity", "precipitation_rate")


class bz_kessler_microphysics(C.Structure):
    _fields_ = [(n, C.c_double) for n in _KESSLER_PARAMS]


class bz_kessler_fields(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in _KESSLER_FIELDS]


_KESSLER_MODEL_FIELDS = ("cloud_liquid_density", "rain_density", "U0_cloud_liquid_density", "U0_rain_density",
                         "G_cloud_liquid_density", "G_rain_density", "vapor_mass_fraction", "cloud_liquid_mass_fraction",
                         "rain_mass_fraction", "rain_terminal_velocity", "precipitation_rate")


class bz_kessler_model_fields(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in _KESSLER_MODEL_FIELDS]


_CSTATE_FIELDS = ("rho_d", "rho", "rho_u", "rho_v", "rho_w", "rho_theta", "rho_q", "u", "v", "w", "theta", "q", "T", "p")
_CPROG_FIELDS = ("rho_d", "rho_u", "rho_v", "rho_w", "rho_theta", "rho_q")
_SUBSTEPPER_FIELDS = ("exner", "potential_temperature", "gamma_R_mixture", "density_perturbation",
                      "density_potential_temperature_perturbation", "momentum_perturbation_u", "momentum_perturbation_v",
                      "momentum_perturbation_w", "density_predictor", "density_potential_temperature_predictor",
                      "previous_density_potential_temperature_perturbation", "time_averaged_u", "time_averaged_v",
                      "time_averaged_w", "slow_vertical_momentum_tendency", "vertical_solver_source_term")


class bz_compressible_state(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in _CSTATE_FIELDS]


class bz_compressible_prognostic(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in _CPROG_FIELDS]


class bz_acoustic_substepper(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in _SUBSTEPPER_FIELDS]


class bz_split_explicit(C.Structure):
    _fields_ = [("substeps", C.c_int32), ("damp_vertical", C.c_int32),
                ("apply_first_substep_pressure_gradient", C.c_int32), ("newton_maxiter", C.c_int32),
                ("acoustic_cfl", C.c_double), ("forward_weight", C.c_double), ("damping_coefficient", C.c_double),
                ("thermodynamic_tendency_factor", C.c_double), ("vertical_momentum_tendency_factor", C.c_double),
                ("newton_abstol", C.c_double), ("direct_divergence_damping", C.c_int32), ("sponge_ramp", C.c_int32),
                ("sponge_damping_rate", C.c_double), ("sponge_depth", C.c_double),
                ("substep_distribution", C.c_int32), ("substep_float_bytes", C.c_int32), ("damping_length_scale", C.c_double)]


class bz_diagnostic_inputs(C.Structure):
    _fields_ = ([(n, C.c_void_p) for n in ("temperature", "vapor", "liquid", "liquid_2", "moisture", "pressure", "density")] +
                [(n, C.c_double) for n in ("liquid_latent_heat", "liquid_heat_capacity", "energy_reference_temperature",
                                           "triple_point_temperature", "triple_point_pressure")])


# bz_diagnostic_kind of include/breeze_hip.h
DIAGNOSTIC_KINDS = ("POTENTIAL_TEMPERATURE", "LIQUID_ICE_POTENTIAL_TEMPERATURE", "VIRTUAL_POTENTIAL_TEMPERATURE",
                    "EQUIVALENT_POTENTIAL_TEMPERATURE", "STABILITY_EQUIVALENT_POTENTIAL_TEMPERATURE", "STATIC_ENERGY",
                    "RELATIVE_HUMIDITY", "SATURATION_SPECIFIC_HUMIDITY", "SATURATION_SPECIFIC_HUMIDITY_EQUILIBRIUM",
                    "SATURATION_SPECIFIC_HUMIDITY_TOTAL_MOISTURE", "DEWPOINT_TEMPERATURE")
BZ_DIAG = {name: code for code, name in enumerate(DIAGNOSTIC_KINDS)}
BZ_DIAG_DENSITY_WEIGHTED = 0x100
BZ_MAX_DIAGNOSTICS = 24


# bz_horizontal_moments of include/breeze_hip.h
BZ_MAX_MOMENT_FIELDS, BZ_MAX_MOMENTS, BZ_MAX_MOMENT_FACTORS = 8, 24, 3


class bz_moment_field(C.Structure):
    _fields_ = [("data", C.c_void_p), ("face_x", C.c_int32), ("face_y", C.c_int32), ("face_z", C.c_int32)]


class bz_moment(C.Structure):
    _fields_ = [("n_factors", C.c_int32), ("field", C.c_int32 * BZ_MAX_MOMENT_FACTORS), ("power", C.c_int32 * BZ_MAX_MOMENT_FACTORS),
                ("dz", C.c_int32), ("at_center", C.c_int32)]


class bz_exner_reference_state(C.Structure):
    _fields_ = [("standard_pressure", C.c_double), ("pressure", _dp), ("density", _dp)]


# every symbol include/breeze_hip.h declares: name -> (restype, argtypes)
_ctx = C.c_void_p
_sp, _pp = C.POINTER(bz_state), C.POINTER(bz_prognostic)
_csp, _cpp, _asp = C.POINTER(bz_compressible_state), C.POINTER(bz_compressible_prognostic), C.POINTER(bz_acoustic_substepper)
SYMBOLS = {
    "bz_create": (C.c_int, [C.POINTER(_ctx), C.POINTER(bz_grid), C.POINTER(bz_constants),
                            C.POINTER(bz_reference_state), C.c_int]),
    "bz_destroy": (None, [_ctx]),
    "bz_set_formulation": (C.c_int, [_ctx, C.c_int]),
    "bz_set_saturation_adjustment": (C.c_int, [_ctx, C.POINTER(bz_saturation_adjustment), C.c_void_p, C.c_void_p]),
    "bz_set_mixed_phase_equilibrium": (C.c_int, [_ctx, C.POINTER(bz_mixed_phase_equilibrium), C.c_void_p]),
    "bz_set_compressible_mixed_phase_equilibrium": (C.c_int, [_ctx, C.POINTER(bz_mixed_phase_equilibrium), C.c_void_p]),
    "bz_set_saturation_vapor_pressure_polynomial": (C.c_int, [_ctx, C.POINTER(bz_flatau_polynomial)]),
    "bz_set_negative_moisture_correction": (C.c_int, [_ctx, C.POINTER(bz_negative_moisture_correction)]),
    "bz_fix_negative_moisture": (C.c_int, [_ctx, C.POINTER(bz_state)]),
    "bz_set_stream": (C.c_int, [_ctx, C.c_void_p]),
    "bz_graph_enable": (C.c_int, [_ctx, C.c_int]),
    "bz_graph_info": (C.c_int, [_ctx, C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "bz_closure_march_info": (C.c_int, [_ctx, C.POINTER(C.c_int32)]),
    "bz_sync": (C.c_int, [_ctx]),
    "bz_last_error": (C.c_char_p, [_ctx]),
    "bz_fill_halo_regions": (C.c_int, [_ctx, C.c_void_p, C.c_int]),
    "bz_compute_velocities": (C.c_int, [_ctx, _sp]),
    "bz_compute_auxiliary_thermodynamic_variables": (C.c_int, [_ctx, _sp]),
    "bz_compute_tendencies": (C.c_int, [_ctx, _sp, _pp]),
    "bz_compute_scalar_tendency": (C.c_int, [_ctx, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bz_set_scalar_advection_order": (C.c_int, [_ctx, C.c_int]),
    "bz_update_state": (C.c_int, [_ctx, _sp, _pp, C.c_int]),
    "bz_store_initial_state": (C.c_int, [_ctx, _sp, _pp]),
    "bz_ssp_rk3_substep": (C.c_int, [_ctx, _sp, _pp, _pp, C.c_double, C.c_double]),
    "bz_compute_pressure_correction": (C.c_int, [_ctx, _sp, C.c_double]),
    "bz_make_pressure_correction": (C.c_int, [_ctx, _sp, C.c_double]),
    "bz_time_step_anelastic": (C.c_int, [_ctx, _sp, _pp, _pp, C.c_double]),
    "bz_time_steps_anelastic": (C.c_int, [_ctx, _sp, _pp, _pp, C.c_double, C.c_int, C.c_int]),
    "bz_diagnostics_stale": (C.c_int, [_ctx]),
    "bz_set_prescribed_dynamics": (C.c_int, [_ctx, C.c_int]),
    "bz_compute_kinematic_tendencies": (C.c_int, [_ctx, _sp, _pp]),
    "bz_time_steps_kinematic": (C.c_int, [_ctx, _sp, _pp, _pp, C.c_double, C.c_int, C.c_int]),
    "bz_create_slab": (C.c_int, [C.POINTER(_ctx), C.POINTER(bz_grid), C.POINTER(bz_constants),
                                 C.POINTER(bz_reference_state), C.c_int, C.c_int, C.c_int]),
    "bz_slab_info": (C.c_int, [_ctx] + [C.POINTER(C.c_int32)] * 5),
    "bz_ssp_rk3_substep_fused": (C.c_int, [_ctx, _sp, _pp, _pp, C.c_double, C.c_double, C.c_int]),
    "bz_poisson_source_term": (C.c_int, [_ctx, _sp, C.c_double, C.c_void_p]),
    "bz_spectral_tridiagonal_solve": (C.c_int, [_ctx, C.c_void_p, C.c_double]),
    "bz_project_and_diagnose": (C.c_int, [_ctx, _sp, C.c_void_p, C.c_void_p, C.c_double]),
    "bz_tendencies_fused_rk": (C.c_int, [_ctx, _sp, _pp, _pp, C.c_double, C.c_double, C.c_int]),
    "bz_poisson_source_term_from": (C.c_int, [_ctx, _sp, _pp, C.c_double, C.c_void_p]),
    "bz_project_and_diagnose_from": (C.c_int, [_ctx, _sp, _pp, C.c_void_p, C.c_void_p, C.c_double]),
    "bz_create_compressible": (C.c_int, [C.POINTER(_ctx), C.POINTER(bz_grid), C.POINTER(bz_constants),
                                         C.POINTER(bz_exner_reference_state), C.POINTER(bz_split_explicit), C.c_int]),
    "bz_compressible_update_state": (C.c_int, [_ctx, _csp, _cpp, _asp, C.c_int]),
    "bz_refresh_linearization": (C.c_int, [_ctx, _csp, _asp]),
    "bz_seed_time_averaged_velocities": (C.c_int, [_ctx, _csp, _asp]),
    "bz_compute_slow_tendencies": (C.c_int, [_ctx, _csp, _cpp]),
    "bz_stage_substeps": (C.c_int, [_ctx, C.c_double, C.c_double, C.POINTER(C.c_int32), C.POINTER(C.c_double)]),
    "bz_acoustic_substep_loop": (C.c_int, [_ctx, _csp, _cpp, _cpp, _asp, C.c_double, C.c_double]),
    "bz_acoustic_rk3_substep": (C.c_int, [_ctx, _csp, _cpp, _cpp, _asp, C.c_double, C.c_double]),
    "bz_time_step_compressible": (C.c_int, [_ctx, _csp, _cpp, _cpp, _asp, C.c_double]),
    "bz_exner_columns": (C.c_int, [_ctx, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bz_set_hydrostatically_balanced_density": (C.c_int, [_ctx, _csp, C.c_double]),
    "bz_set_exner_reference_state": (C.c_int, [_ctx, C.POINTER(bz_exner_reference_state)]),
    "bz_create_compressible_slab": (C.c_int, [C.POINTER(_ctx), C.POINTER(bz_grid), C.POINTER(bz_constants),
                                              C.POINTER(bz_exner_reference_state), C.POINTER(bz_split_explicit), C.c_int,
                                              C.c_int, C.c_int]),
    "bz_acoustic_stage_begin": (C.c_int, [_ctx, _csp, _cpp, _cpp, _asp, C.c_double, C.c_double, C.POINTER(C.c_int32),
                                          C.POINTER(C.c_int32)]),
    "bz_acoustic_substep": (C.c_int, [_ctx, _csp, _cpp, _cpp, _asp, C.c_int32, C.POINTER(C.c_int32)]),
    "bz_acoustic_direct_damping": (C.c_int, [_ctx, _csp, _cpp, _cpp, _asp]),
    "bz_acoustic_stage_end": (C.c_int, [_ctx, _csp, _cpp, _cpp, _asp, C.c_double, C.c_double, C.c_int]),
    "bz_set_acoustic_scratch": (C.c_int, [_ctx, C.c_void_p, C.c_void_p]),
    "bz_set_acoustic_lateral_boundaries": (C.c_int, [_ctx, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double]),
    "bz_compute_moisture_tendency": (C.c_int, [_ctx, _csp, _cpp, _asp]),
    "bz_kessler_microphysics_update": (C.c_int, [_ctx, C.POINTER(bz_kessler_microphysics), C.POINTER(bz_kessler_fields),
                                                 C.c_double, C.c_double]),
    "bz_set_kessler_microphysics": (C.c_int, [_ctx, C.POINTER(bz_kessler_microphysics), C.POINTER(bz_kessler_model_fields),
                                              C.c_double]),
    "bz_kessler_model_update": (C.c_int, [_ctx, _sp, _pp, C.c_double]),
    "bz_compressible_kessler_update": (C.c_int, [_ctx, _csp, _cpp, _asp, C.c_double]),
    "bz_set_instantaneous_precipitation": (C.c_int, [_ctx, C.POINTER(bz_saturation_adjustment), C.c_void_p]),
    "bz_instantaneous_precipitation_update": (C.c_int, [_ctx, _csp, _cpp, _asp, C.c_double]),
    "bz_column_integral": (C.c_int, [_ctx, C.c_void_p, C.c_void_p]),
    "bz_pack_transpose": (C.c_int, [_ctx, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "bz_pack_rows": (C.c_int, [_ctx, C.POINTER(C.c_void_p), C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32]),
    "bz_slab_transform": (C.c_int, [_ctx, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32]),
    "bz_comm_unique_id": (C.c_int, [C.c_void_p]),
    "bz_comm_init_rccl": (C.c_int, [_ctx, C.c_void_p]),
    "bz_comm_init_local": (C.c_int, [_ctx, C.c_char_p]),
    "bz_comm_destroy": (C.c_int, [_ctx]),
    "bz_comm_exchange_y_halos": (C.c_int, [_ctx, C.POINTER(C.c_void_p), C.POINTER(C.c_int32), C.c_int32]),
    "bz_comm_update_state_and_project": (C.c_int, [_ctx, _sp, _pp, C.c_double, C.c_int]),
    "bz_comm_info": (C.c_int, [_ctx, C.POINTER(C.c_char_p), C.POINTER(C.c_int64), C.POINTER(C.c_int32)]),
    "bz_comm_compressible_update_state": (C.c_int, [_ctx, _csp, _cpp, _asp, C.c_int]),
    "bz_set_tracers": (C.c_int, [_ctx, C.c_int32, C.POINTER(bz_tracer_fields)]),
    "bz_set_closure": (C.c_int, [_ctx, C.POINTER(bz_smagorinsky_lilly), C.c_void_p]),
    "bz_set_scalar_diffusivity": (C.c_int, [_ctx, C.POINTER(bz_scalar_diffusivity), C.c_void_p, C.c_void_p]),
    "bz_implicit_step": (C.c_int, [_ctx, _sp, C.c_double]),
    "bz_set_bounds_preserving_advection": (C.c_int, [_ctx, C.POINTER(bz_bounds_preserving_advection)]),
    "bz_compute_closure_fields": (C.c_int, [_ctx, _sp]),
    "bz_compressible_compute_closure_fields": (C.c_int, [_ctx, _csp]),
    "bz_set_bulk_surface_fluxes": (C.c_int, [_ctx, C.POINTER(bz_bulk_surface_fluxes)]),
    "bz_set_surface_layer": (C.c_int, [_ctx, C.POINTER(bz_surface_layer)]),
    "bz_surface_layer_initialize": (C.c_int, [_ctx, _sp]),
    "bz_surface_layer_update": (C.c_int, [_ctx, _sp, C.c_double]),
    "bz_surface_layer_get_filtered": (C.c_int, [_ctx, C.c_int, _dp]),
    "bz_surface_layer_set_filtered": (C.c_int, [_ctx, C.c_int, _dp]),
    "bz_set_compressible_surface_fluxes": (C.c_int, [_ctx, C.POINTER(bz_compressible_surface_fluxes)]),
    "bz_compressible_compute_flux_bc_tendencies": (C.c_int, [_ctx, _csp, _cpp]),
    "bz_set_forcings": (C.c_int, [_ctx, C.POINTER(bz_column_forcings)]),
    "bz_set_relaxation": (C.c_int, [_ctx, C.POINTER(bz_column_relaxation)]),
    "bz_set_field_forcing": (C.c_int, [_ctx, C.c_void_p, C.c_int]),
    "bz_compute_forcings": (C.c_int, [_ctx, _sp]),
    "bz_compute_flux_bc_tendencies": (C.c_int, [_ctx, _sp, _pp]),
    "bz_cell_advection_timescale": (C.c_int, [_ctx, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_double)]),
    "bz_any_nan": (C.c_int, [_ctx, C.c_void_p, C.c_int, C.POINTER(C.c_int32)]),
    "bz_profile_enable": (C.c_int, [_ctx, C.c_int]),
    "bz_profile_reset": (C.c_int, [_ctx]),
    "bz_profile_count": (C.c_int, [_ctx]),
    "bz_profile_get": (C.c_int, [_ctx, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_double),
                                 C.POINTER(C.c_int64)]),
    "bz_max_abs_divergence": (C.c_int, [_ctx, _sp, C.POINTER(C.c_double)]),
    "bz_compute_diagnostics": (C.c_int, [_ctx, _sp, C.POINTER(bz_diagnostic_inputs), C.c_int32, C.POINTER(C.c_int32),
                                         C.POINTER(C.c_void_p)]),
    "bz_horizontal_average": (C.c_int, [_ctx, C.c_void_p, C.c_int, _dp]),
    "bz_horizontal_moments": (C.c_int, [_ctx, C.c_int32, C.POINTER(bz_moment_field), C.c_int32, C.POINTER(bz_moment), _dp,
                                        C.POINTER(C.c_int32)]),
    "bz_set_horizontal_nodes": (C.c_int, [_ctx, _dp, _dp]),
    "bz_azimuthal_mean": (C.c_int, [_ctx, C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_double, C.c_int32, C.c_int32, _dp,
                                    C.POINTER(C.c_int64)]),
    "bz_polar_winds": (C.c_int, [_ctx, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_void_p, C.c_void_p]),
    "bz_nudge_fields": (C.c_int, [_ctx, C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.c_double]),
    "bz_balance_adiabatically_compressible": (C.c_int, [_ctx, _csp, _cpp, _cpp, _asp, C.c_double, C.c_int32, C.c_double, C.c_int32]),
    "bz_balance_adiabatically_anelastic": (C.c_int, [_ctx, _sp, _pp, _pp, C.c_double, C.c_int32, C.c_double, C.c_int32]),
}


def build(verbose=False):
    """Compile every HIP source for gfx950 into lib/libbreeze_hip.so (hipcc cross-compiles without a GPU)."""
    cmd = ["make", "-C", CSRC, "-j8"]
    out = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if out.returncode != 0:
        raise RuntimeError("building libbreeze_hip.so failed:\n" + out.stdout)
    if verbose:
        print(out.stdout)
    return LIB_PATH


_lib = None


CENTERED2_LIB_PATH = os.path.join(_HERE, "lib", "libbreeze_hip_centered2.so")
_libs = {}


def load(advection_order=5, ft2_hypothesis=0):
    """Load libbreeze_hip.so (advection = WENO(order = 5)) or, for advection_order = 2, libbreeze_hip_centered2.so — the same
    sources built with the reconstructions collapsed to Centered(order = 2) — and bind every declared symbol.  ft2_hypothesis = 1 | 2:
    lib/libbreeze_hip_ft2_<level>.so, the WENO kernels built with BZ_WENO_FT2 (csrc/bz_weno.h).  Raises if the library is absent."""
    global _lib
    path = CENTERED2_LIB_PATH if advection_order == 2 else LIB_PATH      # WENO orders 5, 7, 9 live in the same library
    if ft2_hypothesis and advection_order != 2:
        path = os.path.join(_HERE, "lib", f"libbreeze_hip_ft2_{int(ft2_hypothesis)}.so")
    if path in _libs:
        return _libs[path]
    if not os.path.exists(path):
        raise RuntimeError(
            f"{path} not found: the HIP extension is required (no CPU fallback). "
            "Run `python -c 'import __graft_entry__ as g; g.build()'` or `make -C breeze.jl_amd/csrc`.")
    # torch bundles its own HIP runtime; load it first so that libbreeze_hip.so binds to the same
    # libamdhip64 instance (two runtimes in one process cannot both see the device).
    import torch  # noqa: F401
    lib = C.CDLL(path)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)          # AttributeError if a declared symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _libs[path] = lib
    if advection_order != 2 and not ft2_hypothesis:
        _lib = lib
    return lib


# ---- Float32 twin (lib/libbreeze_hip_f32.so, generated by tools/gen_f32_sources.py: every double of the ABI is a float) --------
F32_LIB_PATH = os.environ.get("BREEZE_HIP_F32_LIB") or os.path.join(_HERE, "lib", "libbreeze_hip_f32.so")      # (BREEZE_HIP_F32_LIB: A/B builds of the Float32 twin)
_f32_structs = {}


def _f32_type(t):
    """The Float32 ABI's counterpart of a ctypes type of the Float64 ABI."""
    if t is C.c_double:
        return C.c_float
    if t is _dp:
        return C.POINTER(C.c_float)
    if isinstance(t, type) and issubclass(t, C.Structure):
        if t not in _f32_structs:
            fields = [(n, _f32_type(ft)) for n, ft in t._fields_]
            same = all(a[1] is b[1] for a, b in zip(fields, t._fields_))          # pointer-only structs are shared by both ABIs
            _f32_structs[t] = t if same else type(t.__name__, (C.Structure,), {"_fields_": fields})
        return _f32_structs[t]
    if isinstance(t, type) and issubclass(t, C._Pointer):
        inner = _f32_type(t._type_)
        return t if inner is t._type_ else C.POINTER(inner)
    if isinstance(t, type) and issubclass(t, C.Array):
        return C.c_float * t._length_ if t._type_ is C.c_double else t      # (arrays of pointers are shared by both ABIs)
    return t


class _Types:
    """Struct classes and the scalar type of one precision: types(8).bz_grid is bz_grid, types(4).bz_grid its Float32 mirror."""

    def __init__(self, ftype):
        self.ftype = ftype
        self.real = C.c_double if ftype == 8 else C.c_float
        self.np_real = "float64" if ftype == 8 else "float32"

    def __getattr__(self, name):
        cls = globals()[name]
        return cls if self.ftype == 8 else _f32_type(cls)


def types(ftype=8):
    if ftype not in (4, 8):
        raise ValueError("float type must be 4 (Float32) or 8 (Float64) bytes")
    return _Types(ftype)


def load_f32():
    """libbreeze_hip_f32.so with the Float32 signatures (WENO(order = 5) build)."""
    if F32_LIB_PATH in _libs:
        return _libs[F32_LIB_PATH]
    if not os.path.exists(F32_LIB_PATH):
        raise RuntimeError(f"{F32_LIB_PATH} not found: run `make -C breeze.jl_amd/csrc` (no CPU fallback)")
    import torch  # noqa: F401
    lib = C.CDLL(F32_LIB_PATH)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = [_f32_type(a) for a in args]
    _libs[F32_LIB_PATH] = lib
    return lib


class BreezeHIPError(RuntimeError):
    pass


def check(lib, ctx, rc, what):
    if rc != 0:
        msg = lib.bz_last_error(ctx).decode() if ctx else ""
        raise BreezeHIPError(f"{what} failed with code {rc}: {msg}")
