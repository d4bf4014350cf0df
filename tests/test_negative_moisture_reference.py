"""CPU pins of tests/negative_moisture_reference.py and of the host side of BulkMicrophysics(negative_moisture_correction = ...):
hand-computed columns in dyadic numbers (exact in floating point), the species chain, conservation of the column mass, the host classes,
their refusals and bindings, and the teeth of the device step tests (the oracle run with the correction differs from the run without by
far more than the step tolerance, and every update_state of it finds negative cells).  Nothing here needs a GPU."""
import numpy as np
import pytest

import negative_moisture_reference as nmr

F64, F32 = np.float64, np.float32
DTYPES = pytest.mark.parametrize("dtype", [F64, F32], ids=["Float64", "Float32"])


def _vertical(rq, dz, rho=None, dtype=F64):
    rq = np.array(rq, dtype=dtype)
    rho = np.ones(len(rq)) if rho is None else rho
    return nmr.fix_negative_moisture(rq, np.asarray(rho, dtype=dtype), np.asarray(dz, dtype=dtype), vertical=True)


# ---- vertical borrowing by hand -----------------------------------------------------------------------------------------------------------------
@DTYPES
def test_cascade_reaches_the_bottom_and_level_two_is_not_positive(dtype):
    """dz = (1, 2, 4), rho = 1: top -2 -> deficit 8, level 2: -1 - 8 / 2 = -5 -> deficit 10, bottom 3 - 10 = -7; level 2 ends at 0: no upward borrow"""
    got = _vertical([3.0, -1.0, -2.0], [1.0, 2.0, 4.0], dtype=dtype)
    assert nmr.same_bits(got, np.array([-7.0, 0.0, 0.0], dtype=dtype))


@DTYPES
def test_bottom_borrows_from_level_two(dtype):
    """dz = (1, 2, 4): needed 1, available 4 * 2 = 8: the bottom takes min(1, 8) = 1, level 2 gives 1 / 2"""
    got = _vertical([-1.0, 4.0, 0.5], [1.0, 2.0, 4.0], dtype=dtype)
    assert nmr.same_bits(got, np.array([0.0, 3.5, 0.5], dtype=dtype))


@DTYPES
def test_bottom_takes_what_there_is_when_the_supply_is_short(dtype):
    """needed 8, available 0.5 * 2 = 1: the bottom ends at -8 + 1 = -7, level 2 at 0"""
    got = _vertical([-8.0, 0.5, 2.0], [1.0, 2.0, 4.0], dtype=dtype)
    assert nmr.same_bits(got, np.array([-7.0, 0.0, 2.0], dtype=dtype))


@DTYPES
def test_density_scales_nothing_but_the_sign_test(dtype):
    """rho = (2, 4, 8) on the first example: the deficits are masses rho q dz, the same numbers"""
    got = _vertical([3.0, -1.0, -2.0], [1.0, 2.0, 4.0], rho=[2.0, 4.0, 8.0], dtype=dtype)
    assert nmr.same_bits(got, np.array([-7.0, 0.0, 0.0], dtype=dtype))


@DTYPES
def test_a_single_level_is_left_alone(dtype):
    """Nz = 1: the sweep is empty, k_top = k_bot, dq = 0"""
    for v in (-3.0, 2.0):
        assert nmr.same_bits(_vertical([v], [2.0], dtype=dtype), np.array([v], dtype=dtype))


@DTYPES
def test_a_nan_cell_passes_through(dtype):
    """every comparison with a NaN is false: no deficit is formed from it, and the cells above and below it are treated as without it"""
    got = _vertical([1.0, np.nan, -2.0, 1.0], [1.0, 1.0, 1.0, 1.0], dtype=dtype)
    assert np.isnan(got[1]) and np.isnan(got[0:1]).sum() == 0
    assert got[3] == 1.0 and got[2] == 0.0 and np.isnan(got[1]) and got[0] == 1.0
    got = _vertical([np.nan, 2.0, 1.0], [1.0, 1.0, 1.0], dtype=dtype)          # a NaN at the bottom borrows nothing
    assert np.isnan(got[0]) and got[1] == 2.0 and got[2] == 1.0


@DTYPES
def test_minus_zero_is_not_negative(dtype):
    """-0 < 0 is false: no deficit; rho q += 0 / dz makes it +0 at the levels the sweep and the bottom step add to, rho q -= 0 keeps the sign"""
    got = _vertical([-0.0, -0.0, -0.0], [1.0, 2.0, 4.0], dtype=dtype)
    assert np.all(got == 0) and not np.signbit(got).any()
    got = _vertical([1.0, 2.0, -0.0, 3.0], [1.0, 1.0, 1.0, 1.0], dtype=dtype)
    assert nmr.same_bits(got, np.array([1.0, 2.0, 0.0, 3.0], dtype=dtype))


@DTYPES
def test_a_quotient_that_underflows_is_not_negative(dtype):
    """rho q = -tiny (the smallest subnormal) over rho = 4 rounds to -0: 'not negative', the cell keeps its value; over rho = 1 it is a deficit"""
    tiny = np.finfo(dtype).smallest_subnormal
    got = _vertical([1.0, -tiny], [1.0, 1.0], rho=[1.0, 4.0], dtype=dtype)
    assert nmr.same_bits(got, np.array([1.0, -tiny], dtype=dtype))
    got = _vertical([1.0, -tiny], [1.0, 1.0], rho=[1.0, 1.0], dtype=dtype)
    assert got[1] == 0.0 and got[0] == dtype(1.0) - tiny


def test_the_residue_of_a_removed_deficit_is_the_references():
    """rho q + (-rho q dz) / dz is not an exact zero in general: the restatement keeps the reference's operations, not their algebra"""
    rng = np.random.default_rng(3)
    v, dz = -rng.random(4000), 1.0 + rng.random(4000)
    rq = np.stack([np.ones(4000), v])
    got = nmr.fix_negative_moisture(rq.copy(), np.ones(2), np.ones(2), vertical=True)          # dz = 1: exact
    assert np.all(got[1] == 0)
    res = v + (-v * dz) / dz
    assert (res != 0).any() and np.abs(res).max() <= np.finfo(F64).eps


# ---- species borrowing by hand -------------------------------------------------------------------------------------------------------------------
def _col(*v, dtype=F64):
    return np.array(v, dtype=dtype)


@DTYPES
def test_an_empty_chain_does_nothing(dtype):
    rq = _col(-1.0, 2.0, dtype=dtype)
    got = nmr.fix_negative_moisture(rq.copy(), np.ones(2), np.ones(2), species=True)
    assert nmr.same_bits(got, rq)


@DTYPES
def test_a_chain_of_one_borrows_from_the_moisture_prognostic(dtype):
    """rho = 2, levels: cloud -1 with vapour 3 (all of the deficit), cloud -4 with vapour 1 (what there is), cloud -1 with vapour -2 (nothing),
    cloud +1 (no sink)"""
    rho = np.full(4, 2.0)
    cloud, rq = _col(-1.0, -4.0, -1.0, 1.0, dtype=dtype), _col(3.0, 1.0, -2.0, 5.0, dtype=dtype)
    total = cloud + rq
    nmr.fix_negative_moisture(rq, rho, np.ones(4), species=True, mass=(cloud,))
    assert nmr.same_bits(cloud, _col(0.0, -3.0, -1.0, 1.0, dtype=dtype)) and nmr.same_bits(rq, _col(2.0, 0.0, -2.0, 5.0, dtype=dtype))
    assert np.array_equal(cloud + rq, total)


@DTYPES
def test_a_chain_of_two_with_pairs_and_a_clamp(dtype):
    """rain <- cloud <- vapour at one level of rho = 1: rain -2 takes 1.5 from cloud (all it has), cloud 0 then takes nothing it needs;
    second level: rain -1 from cloud 4.  Numbers: rain's number dies where rain's mass stays <= 0, and negative numbers are clamped."""
    rho = np.ones(2)
    rain, cloud, rq = _col(-2.0, -1.0, dtype=dtype), _col(1.5, 4.0, dtype=dtype), _col(8.0, 8.0, dtype=dtype)
    n_rain, n_cloud = _col(7.0, 7.0, dtype=dtype), _col(-3.0, 9.0, dtype=dtype)
    total = rain + cloud + rq
    nmr.fix_negative_moisture(rq, rho, np.ones(2), species=True, mass=(rain, cloud), pairs=((n_rain, rain), (n_cloud, cloud)),
                              numbers=(n_rain, n_cloud))
    assert nmr.same_bits(rain, _col(-0.5, 0.0, dtype=dtype)) and nmr.same_bits(cloud, _col(0.0, 3.0, dtype=dtype))
    assert nmr.same_bits(rq, _col(8.0, 8.0, dtype=dtype))
    assert np.array_equal(rain + cloud + rq, total)
    assert nmr.same_bits(n_rain, _col(0.0, 0.0, dtype=dtype))          # rain mass -0.5 and 0: both orphaned
    assert nmr.same_bits(n_cloud, _col(0.0, 9.0, dtype=dtype))         # cloud mass 0 orphans the first (and the clamp has nothing left to do)


def test_the_clamp_alone_and_vertical_borrowing_alone():
    n = _col(-1.0, 2.0, -0.0)
    nmr.fix_negative_moisture(_col(1.0, 1.0, 1.0), np.ones(3), np.ones(3), species=True, numbers=(n,))
    assert nmr.same_bits(n, _col(0.0, 2.0, 0.0))
    # VerticalBorrowing() alone skips the species phase: the lists are not looked at
    cloud, rq = _col(-1.0, -1.0), _col(3.0, 3.0)
    nmr.fix_negative_moisture(rq, np.ones(2), np.ones(2), species=False, vertical=True, mass=(cloud,))
    assert nmr.same_bits(cloud, _col(-1.0, -1.0)) and nmr.same_bits(rq, _col(3.0, 3.0))


@DTYPES
def test_species_then_vertical(dtype):
    """the species phase of every level comes before the sweep: cloud -1 takes 1 of vapour 0.5 -> vapour 0, cloud -0.5; the level above's
    deficit then lands on that 0"""
    cloud, rq = _col(0.0, -1.0, 0.0, dtype=dtype), _col(4.0, 0.5, -1.0, dtype=dtype)
    nmr.fix_negative_moisture(rq, np.ones(3), np.ones(3), species=True, vertical=True, mass=(cloud,))
    assert nmr.same_bits(cloud, _col(0.0, -0.5, 0.0, dtype=dtype)) and nmr.same_bits(rq, _col(3.0, 0.0, 0.0, dtype=dtype))


# ---- conservation ----------------------------------------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("Nz", [3, 9, 40])
def test_column_mass_is_conserved_on_random_stretched_columns(dtype, Nz):
    """sum_k rho q dz changes by at most (Nz + 2) eps sum_k |rho q| dz"""
    rng = np.random.default_rng(Nz)
    dz = np.diff(nmr.stretched_faces(Nz)).astype(dtype)
    rho = (1.2 * np.exp(-np.cumsum(dz.astype(F64)) / 8000.0)).astype(dtype)
    rq = ((rng.random((Nz, 500)) - 0.45) * 1e-2).astype(dtype)
    before = rq.copy()
    nmr.fix_negative_moisture(rq, rho, dz, vertical=True)
    m0, m1 = nmr.column_mass(before, dz)[0], nmr.column_mass(rq, dz)[0]
    bound = nmr.conservation_bound(before, dz)
    assert np.all(np.abs(m1 - m0) <= bound), float((np.abs(m1 - m0) / bound).max())
    assert not nmr.same_bits(rq, before) and np.all(rq[2:] / rho[2:, None] > -np.finfo(dtype).eps)


def test_populations_hold_what_their_names_say():
    shape = (9, 3, 65)
    rho = 1.2 * np.exp(-np.arange(9) / 6.0)
    f, tag = nmr.populations(shape, rho, F64)
    assert sorted(np.unique(tag)) == list(range(len(nmr.POPULATIONS)))
    dz = np.diff(nmr.stretched_faces(9))
    out = nmr.fix_negative_moisture(f.copy(), rho, dz, vertical=True)
    sel = lambda a, name: a[:, tag == nmr.POPULATIONS.index(name)]
    assert nmr.same_bits(sel(out, "positive"), sel(f, "positive"))
    assert np.all(sel(out, "top")[1:] > -1e-17) and np.all(sel(out, "top")[0] > 0)
    assert np.all(sel(out, "cascade")[0] < 0) and np.all(sel(out, "all-negative")[0] < 0)
    assert np.all(np.abs(sel(out, "bottom-enough")[0]) < 1e-17) and np.all(sel(out, "bottom-too-little")[0] < -1e-2)
    assert nmr.same_bits(sel(out, "bottom-nothing")[0], sel(f, "bottom-nothing")[0])
    assert np.isnan(sel(out, "nan")).sum(axis=0).min() == 1 and not np.signbit(sel(out, "minus-zero")[0]).any()


# ---- the host mirror -------------------------------------------------------------------------------------------------------------------------------
def _grid(bz):
    return bz.RectilinearGrid((16, 8, 8), x=(0, 1600.0), y=(0, 800.0), z=(0, 8e3))


def test_constructors_and_their_refusals(bz):
    b = bz.BulkMicrophysics()
    assert isinstance(b.cloud_formation, bz.SaturationAdjustment) and b.cloud_formation.mixed_phase
    assert b.categories is None and b.precipitation_boundary_condition is None and b.negative_moisture_correction is None
    s = bz.SpeciesBorrowing()
    assert s.vertical_borrowing is None
    v = bz.VerticalBorrowing()
    assert bz.SpeciesBorrowing(vertical_borrowing=v).vertical_borrowing is v
    warm = bz.SaturationAdjustment(equilibrium=bz.WarmPhaseEquilibrium())
    b = bz.BulkMicrophysics(cloud_formation=warm, negative_moisture_correction=v)
    assert b.cloud_formation is warm and b.negative_moisture_correction is v
    with pytest.raises(NotImplementedError, match="categories"):
        bz.BulkMicrophysics(categories=object())
    with pytest.raises(NotImplementedError, match="NonEquilibriumCloudFormation"):
        bz.BulkMicrophysics(cloud_formation=bz.NonEquilibriumCloudFormation(None))
    with pytest.raises(NotImplementedError, match="precipitation_boundary_condition"):
        bz.BulkMicrophysics(precipitation_boundary_condition=object())
    with pytest.raises(TypeError, match="negative_moisture_correction"):
        bz.BulkMicrophysics(negative_moisture_correction="VerticalBorrowing")
    with pytest.raises(TypeError, match="vertical_borrowing"):
        bz.SpeciesBorrowing(vertical_borrowing=True)


def test_the_wrapper_is_looked_through(bz):
    from breeze_jl_amd import _context
    from breeze_jl_amd.microphysics import cloud_formation, vertical_borrowing
    warm, mixed = bz.SaturationAdjustment(equilibrium=bz.WarmPhaseEquilibrium()), bz.SaturationAdjustment()
    assert _context.is_mixed_phase(bz.BulkMicrophysics(cloud_formation=mixed)) and _context.is_mixed_phase(mixed)
    assert not _context.is_mixed_phase(bz.BulkMicrophysics(cloud_formation=warm)) and not _context.is_mixed_phase(None)
    assert cloud_formation(bz.BulkMicrophysics(cloud_formation=warm)) is warm and cloud_formation(warm) is warm and cloud_formation(None) is None
    assert vertical_borrowing(bz.VerticalBorrowing()) and vertical_borrowing(bz.SpeciesBorrowing(bz.VerticalBorrowing()))
    assert not vertical_borrowing(bz.SpeciesBorrowing()) and not vertical_borrowing(None)
    # the mixed-phase refusals of the anelastic model reach a wrapped mixed-phase adjustment
    grid = _grid(bz)
    ref = bz.ReferenceState(grid, potential_temperature=300.0)
    heat = bz.BulkSensibleHeatFlux(coefficient=1e-3, surface_temperature=300.0)
    with pytest.raises(NotImplementedError, match="MixedPhaseEquilibrium"):
        bz.AtmosphereModel(grid, dynamics=bz.AnelasticDynamics(ref), advection=bz.WENO(order=5), microphysics=bz.BulkMicrophysics(cloud_formation=mixed),
                           boundary_conditions={"ρθ": bz.FieldBoundaryConditions(bottom=heat)})


def test_the_other_models_refuse_by_name_before_asking_for_a_gpu(bz):
    """CompressibleAtmosphereModel, the slab models and the kinematic driver name BulkMicrophysics, before their generic type check (whose
    pinned messages stay as they are) and before the device check"""
    from breeze_jl_amd import distributed
    grid = _grid(bz)
    ref = bz.ReferenceState(grid, potential_temperature=300.0)
    bulk = bz.BulkMicrophysics(cloud_formation=bz.SaturationAdjustment(equilibrium=bz.WarmPhaseEquilibrium()),
                               negative_moisture_correction=bz.VerticalBorrowing())
    dyn = lambda: bz.CompressibleDynamics(bz.SplitExplicitTimeDiscretization(substeps=6))
    cases = {
        "compressible": lambda: bz.CompressibleAtmosphereModel(grid, dyn(), advection=bz.WENO(order=5), microphysics=bulk),
        "compressible slab": lambda: bz.compressible.SlabCompressibleModel(grid, 0, 1, dyn(), advection=bz.WENO(order=5), microphysics=bulk,
                                                                           device="cuda:0"),
        "kinematic": lambda: bz.AtmosphereModel(grid, dynamics=bz.PrescribedDynamics(ref), advection=bz.WENO(order=5), microphysics=bulk),
        "library slab": lambda: distributed.LibrarySlabAtmosphereModel(grid, 0, 1, advection=bz.WENO(order=5), microphysics=bulk, device="cuda:0"),
    }
    for name, make in cases.items():
        with pytest.raises(NotImplementedError, match="BulkMicrophysics is not implemented"):
            make()
    with pytest.raises(NotImplementedError) as e:          # an unknown type keeps the pinned message
        bz.CompressibleAtmosphereModel(grid, dyn(), advection=bz.WENO(order=5), microphysics=object())
    assert "BulkMicrophysics" not in str(e.value)


def test_symbols_struct_and_headers(bz):
    import ctypes
    import os
    from breeze_jl_amd import _lib
    for name, nargs in (("bz_set_negative_moisture_correction", 2), ("bz_fix_negative_moisture", 2)):
        res, args = bz.SYMBOLS[name]
        assert res is ctypes.c_int and len(args) == nargs
    S = _lib.bz_negative_moisture_correction
    assert [n for n, _ in S._fields_] == ["species_borrowing", "vertical_borrowing", "n_mass", "n_pairs", "n_clamp", "reserved", "mass", "number",
                                          "pair_mass", "clamp"]
    assert ctypes.sizeof(S) == 6 * 4 + 16 * 8 and _lib.types(4).bz_negative_moisture_correction is S          # pointers and counts only
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for header, real in (("breeze_hip.h", "double"), ("breeze_hip_f32.h", "float")):
        text = open(os.path.join(root, "include", header), encoding="utf-8").read()
        assert "int bz_set_negative_moisture_correction(bz_ctx *ctx, const bz_negative_moisture_correction *c);" in text, header
        assert "int bz_fix_negative_moisture(bz_ctx *ctx, const bz_state *s);" in text, header
        assert f"{real} *mass[4];" in text and f"{real} *number[4], *pair_mass[4];" in text and f"{real} *clamp[4];" in text, header
    assert all(hasattr(bz, n) for n in ("BulkMicrophysics", "VerticalBorrowing", "SpeciesBorrowing", "fix_negative_moisture_"))


# ---- teeth of the device step tests ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("phase", ["warm", "mixed"])
def test_the_oracle_pair_of_the_step_tests_has_teeth(oracle, phase):
    """the state and the oracle the GPU step tests use (test_negative_moisture.py), with and without the correction: after three steps rho q
    differs by at least 1e3 times the step tolerance (1e-9 of the field's scale), and every update_state of the corrected run finds
    negative cells"""
    size = (64, 16, 12)
    fields = {}
    for corrected in (True, False):
        om = nmr.oracle_model(oracle, size, phase, corrected_run=corrected)
        built = len(getattr(om, "negative_cells", ()))          # (the constructor's own update_states, on an empty state)
        nmr.set_oracle(om)
        for _ in range(nmr.STEPS):
            om.time_step(nmr.DT)
        fields[corrected] = np.array(om.grid.interior(om.rq))
        if corrected:
            # set: two update_states; the first step: maybe_prepare_first_time_step and three stages; then three per step
            found = om.negative_cells[built:]
            assert len(found) == 2 + 1 + 3 * nmr.STEPS and min(found) >= 1, om.negative_cells
    scale = np.abs(fields[True]).max()
    assert np.abs(fields[True] - fields[False]).max() >= 1e3 * nmr.STEP_TOL * scale
    assert np.isfinite(fields[True]).all() and np.isfinite(fields[False]).all()
