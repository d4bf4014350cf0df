"""Pins tests/compressible_surface_flux_reference.py (no GPU): the restated fluxes against the anelastic oracle's bulk-flux code
(oracle/forcings.py: _add_bulk_fluxes) on the same first-level fields, closed forms, a constant (Ny, Nx) surface temperature against the
number; and the host side of CompressibleAtmosphereModel(boundary_conditions = ...): every refusal by name before anything needs a GPU,
the pinned lateral message, the ABI symbols and the struct layout in both headers."""
import ctypes
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import compressible_surface_flux_reference as sfr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps
EXT = dict(x=(0.0, 1600.0), y=(0.0, 900.0), z=(0.0, 800.0))


def _model(oracle, oc, size=(16, 9, 8), p0=101325.0, pst=1e5, micro=None, fluxes=None):
    og = oracle.Grid(size, **EXT)
    return sfr.SurfaceFluxCompressibleModel(og, surface_fluxes=fluxes, time_discretization=oc.SplitExplicit(substeps=6), surface_pressure=p0,
                                            standard_pressure=pst, reference_potential_temperature=300.0, microphysics=micro)


def _fill(m, u, v, theta, q):
    """first-level (and every other level's) u, v, theta, q from functions of x (y-invariant), periodic halos filled"""
    g = m.grid
    x = (np.arange(g.Nx) + 0.5) / g.Nx
    for f, fun in ((m.u, u), (m.v, v), (m.theta, theta), (m.q, q)):
        g.interior(f)[...] = np.broadcast_to(fun(x)[None, None, :], (g.Nz, g.Ny, g.Nx))
        m._halo_center(f)


SHEAR = dict(u=lambda x: 6.0 * np.sin(2 * np.pi * x) + 1.0, v=lambda x: 4.0 * np.cos(4 * np.pi * x) - 0.5,
             theta=lambda x: 299.0 + 2.0 * np.sin(2 * np.pi * x + 0.4), q=lambda x: 0.012 + 0.004 * np.cos(2 * np.pi * x))


@pytest.mark.parametrize("micro", [None, "SaturationAdjustment"])
def test_restated_fluxes_equal_the_anelastic_oracle_code(oracle, oc, micro):
    """the same first-level fields through both: equal to the last bit or within 4 eps of the flux"""
    from oracle import forcings as of
    drag, heat, vapor = (1.3e-3, 0.5, 298.0), (1.1e-3, 1.0, 301.5), (1.2e-3, 0.25, 300.5)
    m = _model(oracle, oc, micro=micro, fluxes=sfr.SurfaceFluxes(drag, heat, vapor))
    _fill(m, **SHEAR)
    g = m.grid
    if micro:
        g.interior(m.qv)[...] = 0.9 * g.interior(m.q)
        g.interior(m.ql)[...] = 0.1 * g.interior(m.q)
    J = sfr.first_level_fluxes(m, m.surface_fluxes)
    a = SimpleNamespace(grid=g, constants=m.constants, u=m.u, v=m.v, theta=m.theta, q=m.q, qv=getattr(m, "qv", None), microphysics=micro,
                        G={n: np.zeros_like(m.G[n]) for n in ("ru", "rv", "rtheta", "rq")})
    of._add_bulk_fluxes(a, of.BulkFluxes(m.p0, m.pst, drag=drag, heat=heat, vapor=vapor), 1.0)
    for n in ("ru", "rv", "rtheta", "rq"):
        want = g.interior(a.G[n])[0]
        assert np.abs(want).max() > 0, n
        assert np.all(np.abs(J[n] - want) <= 4 * EPS * np.abs(want)), (n, np.abs(J[n] - want).max())
        assert not g.interior(a.G[n])[1:].any()
    # through compute_flux_bc_tendencies!: J / dz_1 at k = 0, nothing above
    for n in m.G:
        m.G[n][...] = 0.0
    sfr.add_flux_bc_tendencies(m, m.surface_fluxes)
    dz = g.dzc[g.Hz]
    for n in ("ru", "rv", "rtheta", "rq"):
        assert np.array_equal(g.interior(m.G[n])[0], J[n] * 1.0 / dz), n
        assert not g.interior(m.G[n])[1:].any()
    assert not m.G["rw"].any() and not m.G["rho_d"].any()


def test_closed_forms(oracle, oc):
    """u = (3, 0) with gustiness 4: U~ = 5 exactly; p0 = p_st makes theta0 = T0, so theta - theta0 = 1 exactly"""
    T0, C = 299.0, 2e-3
    m = _model(oracle, oc, p0=1e5, pst=1e5, fluxes=sfr.SurfaceFluxes(drag=(C, 4.0, T0), heat=(C, 4.0, T0), vapor=(C, 4.0, T0)))
    one = lambda x: np.ones_like(x)      # noqa: E731
    _fill(m, u=lambda x: 3.0 * one(x), v=lambda x: 0.0 * x, theta=lambda x: (T0 + 1.0) * one(x), q=lambda x: 0.0 * x)
    J = sfr.first_level_fluxes(m, m.surface_fluxes)
    rho0 = 1e5 / (m.constants.Rd * T0)
    assert np.all(J["ru"] == -rho0 * C * 5.0 * 3.0)
    assert np.all(J["rv"] == 0.0)
    assert np.all(J["rtheta"] == -rho0 * C * 5.0 * 1.0)
    from oracle.thermo import ThermoConstants, saturation_specific_humidity
    q0 = saturation_specific_humidity(T0, rho0, ThermoConstants(), "liquid")
    assert 0.005 < q0 < 0.03
    want = rho0 * C * 5.0 * q0                       # evaporation into dry air: upward (positive) flux
    assert np.all(np.abs(J["rq"] - want) <= 4 * EPS * want) and np.all(J["rq"] > 0)


def test_constant_array_reproduces_the_number(oracle, oc):
    scal = sfr.SurfaceFluxes((1.3e-3, 0.5, 298.0), (1.1e-3, 1.0, 301.5), (1.2e-3, 0.25, 300.5))
    m = _model(oracle, oc, fluxes=scal)
    _fill(m, **SHEAR)
    g = m.grid
    arr = sfr.SurfaceFluxes(*[(c, gu, np.full((g.Ny, g.Nx), T0)) for c, gu, T0 in (scal.drag, scal.heat, scal.vapor)])
    Ja, Jb = sfr.first_level_fluxes(m, scal), sfr.first_level_fluxes(m, arr)
    for n in Ja:
        assert np.array_equal(Ja[n], Jb[n]), n
    # and a varying array changes every flux
    rng = np.random.default_rng(0)
    var = sfr.SurfaceFluxes(*[(c, gu, T0 + rng.random((g.Ny, g.Nx))) for c, gu, T0 in (scal.drag, scal.heat, scal.vapor)])
    Jc = sfr.first_level_fluxes(m, var)
    assert all(np.abs(Jc[n] - Ja[n]).max() > 1e-6 * np.abs(Ja[n]).max() for n in Ja)


def test_stage_adds_the_fluxes_after_the_slow_tendencies(oracle, oc):
    """compute_slow_tendencies of the restatement = the parent's + J / dz_1 at k = 0 of G_ru, G_rv, G_rtheta and of the moisture tendency"""
    m = _model(oracle, oc, size=(16, 12, 8), fluxes=None)
    g = m.grid
    rho = m.ref.density[g.Hz:g.Hz + g.Nz][:, None, None]
    m.set(rho=rho, theta=lambda x, y, z: 300.0 + 0.003 * z + np.sin(2 * np.pi * x / 1600.0), u=lambda x, y, z: 3.0 * np.cos(2 * np.pi * y / 900.0) + 0 * x + 0 * z,
          v=1.0, w=0.0, qv=0.01)
    m.seed_time_averaged_velocities()
    m.update_state(compute_tendencies=True)
    m.compute_slow_tendencies()
    base = {n: a.copy() for n, a in m.G.items()}
    m.surface_fluxes = sfr.SurfaceFluxes((1e-3, 1.0, 300.0), (1e-3, 1.0, 302.0), (1e-3, 1.0, 302.0))
    m.update_state(compute_tendencies=True)
    m.compute_slow_tendencies()
    J = sfr.first_level_fluxes(m, m.surface_fluxes)
    dz = g.dzc[g.Hz]
    for n in ("ru", "rv", "rtheta", "rq"):
        d = g.interior(m.G[n]) - g.interior(base[n])
        assert np.array_equal(g.interior(m.G[n])[0], g.interior(base[n])[0] + J[n] * 1.0 / dz), n
        assert not d[1:].any() and np.abs(d[0]).max() > 0, n
    assert np.array_equal(m.G["rw"], base["rw"]) and np.array_equal(m.G["rho_d"], base["rho_d"])


# ---- host side --------------------------------------------------------------------------------------------------------------------------
LATERAL = "boundary_conditions: the open lateral boundaries of the acoustic substep loop on a Bounded x / y"


def _grid(bz, topology=None, size=(16, 8, 8)):
    ext = dict(x=(0.0, 1600.0), y=(0.0, 800.0), z=(0.0, 800.0))
    kw = {}
    if topology is not None:
        kw["topology"] = topology
        for d, name in enumerate("xyz"):
            if topology[d] == bz.Flat:
                ext.pop(name)
    return bz.RectilinearGrid(size[:len(ext)], **ext, **kw)


def _build(bz, bcs, topology=None, size=(16, 8, 8), **kw):
    dyn = bz.CompressibleDynamics(bz.SplitExplicitTimeDiscretization())
    return bz.CompressibleAtmosphereModel(_grid(bz, topology, size), dyn, advection=bz.WENO(order=5), boundary_conditions=bcs, **kw)


def _refusals(bz):
    P, B, F = bz.Periodic, bz.Bounded, bz.Flat
    FBC, drag = bz.FieldBoundaryConditions, bz.BulkDrag(coefficient=1e-3, surface_temperature=300.0)
    heat = bz.BulkSensibleHeatFlux(coefficient=1e-3, surface_temperature=300.0)
    ok = {"ρu": FBC(bottom=drag), "ρv": FBC(bottom=drag)}

    def slab():
        dyn = bz.CompressibleDynamics(bz.SplitExplicitTimeDiscretization())
        return bz.compressible.SlabCompressibleModel(_grid(bz), 0, 1, dyn, advection=bz.WENO(order=5), device="cuda:0", boundary_conditions=ok)

    return {
        "PolynomialCoefficient": lambda: _build(bz, {"ρu": FBC(bottom=bz.BulkDrag(coefficient=bz.PolynomialCoefficient(), surface_temperature=300.0))}),
        "FilteredSurfaceVelocities": lambda: _build(bz, {"ρθ": FBC(bottom=bz.BulkSensibleHeatFlux(
            coefficient=1e-3, surface_temperature=300.0, filtered_velocities=bz.FilteredSurfaceVelocities(filter_timescale=600.0)))}),
        "function-valued coefficient": lambda: _build(bz, {"ρu": FBC(bottom=bz.BulkDrag(coefficient=lambda U: 1e-3 * U, surface_temperature=300.0))}),
        "plain flux number": lambda: _build(bz, {"ρθ": FBC(bottom=bz.FluxBoundaryCondition(0.01))}),
        "bare number": lambda: _build(bz, {"ρqᵗ": 5e-5}),
        "top": lambda: _build(bz, {"ρθ": FBC(top=heat)}),
        "lateral flux": lambda: _build(bz, {"ρθ": FBC(west=heat)}),
        "Flat y": lambda: _build(bz, ok, (P, F, B)),
        "walls in y": lambda: _build(bz, ok, (P, B, B)),
        "walls in x": lambda: _build(bz, ok, (B, P, B)),
        "SlabCompressibleModel": slab,
    }


@pytest.mark.parametrize("case", ["PolynomialCoefficient", "FilteredSurfaceVelocities", "function-valued coefficient", "plain flux number",
                                  "bare number", "top", "lateral flux", "Flat y", "walls in y", "walls in x", "SlabCompressibleModel"])
def test_refused_by_name_before_anything_needs_a_gpu(bz, case):
    with pytest.raises(NotImplementedError, match="bulk surface fluxes"):
        _refusals(bz)[case]()


def test_pinned_lateral_message_and_key_checks(bz):
    walls = {"ρv": bz.FieldBoundaryConditions(south=bz.NormalFlowBoundaryCondition(1.0))}
    for kw in ({}, dict(closure=(bz.SmagorinskyLilly(),))):
        with pytest.raises(NotImplementedError) as e:
            _build(bz, walls, **kw)
        assert str(e.value) == LATERAL
    drag = bz.BulkDrag(coefficient=1e-3, surface_temperature=300.0)
    with pytest.raises(NotImplementedError) as e:      # a lateral open condition beside bottom fluxes: still the lateral message
        _build(bz, dict(walls, **{"ρu": bz.FieldBoundaryConditions(bottom=drag)}))
    assert str(e.value) == LATERAL
    with pytest.raises(ValueError, match="surface_temperature"):      # default_drag_surface_temperature(::CompressibleDynamics) throws
        _build(bz, {"ρu": bz.BulkDrag(coefficient=1e-3)})
    heat = bz.BulkSensibleHeatFlux(coefficient=1e-3, surface_temperature=300.0)
    with pytest.raises(ValueError, match="both ρθ and ρe|BulkSensibleHeatFlux belongs"):
        _build(bz, {"ρu": heat})
    with pytest.raises((ValueError, NotImplementedError), match="both ρθ and ρe"):
        _build(bz, {"ρθ": heat, "ρe": heat})
    with pytest.raises(ValueError, match="shape"):
        _build(bz, {"ρθ": bz.BulkSensibleHeatFlux(coefficient=1e-3, surface_temperature=np.full((3, 3), 300.0))})


def test_conditions_are_sorted_into_slots_and_materialized(bz):
    from breeze_jl_amd import _lib, forcings
    g = _grid(bz)
    drag = bz.BulkDrag(coefficient=1.5e-3, gustiness=0.5, surface_temperature=299.0)
    T0 = np.linspace(298.0, 302.0, g.Ny * g.Nx).reshape(g.Ny, g.Nx)
    heat = bz.BulkSensibleHeatFlux(coefficient=1.1e-3, surface_temperature=T0, gustiness=1.0)
    vap = bz.BulkVaporFlux(coefficient=1.2e-3, surface_temperature=lambda x, y: 300.0 + 1e-3 * x)
    for moisture_key in ("ρqᵛ", "ρqᵉ", "ρqᵗ"):
        bcs = {"ρu": bz.FieldBoundaryConditions(bottom=drag), "ρv": bz.FieldBoundaryConditions(bottom=drag), "ρe": heat, moisture_key: vap}
        slots = forcings.compressible_surface_flux_conditions(bcs, g, True, False)
        assert slots == {"drag": drag, "heat": heat, "vapor": vap}      # keyed rho e: moved to rho theta, the same condition
    dyn = bz.CompressibleDynamics(bz.SplitExplicitTimeDiscretization(), surface_pressure=1.01e5, standard_pressure=1e5)
    for ftype, real in ((8, np.float64), (4, np.float32)):
        S, keep = forcings.materialize_compressible_surface_fluxes(g, slots, dyn, bz.ThermodynamicConstants(), _lib.types(ftype))
        assert (S.drag.enabled, S.heat.enabled, S.vapor.enabled) == (1, 1, 1)
        assert S.drag.coefficient == real(1.5e-3) and S.drag.gustiness == 0.5 and S.drag.surface_temperature == 299.0
        assert not S.drag.surface_temperature_field and bool(S.heat.surface_temperature_field) and bool(S.vapor.surface_temperature_field)
        assert S.surface_pressure == real(1.01e5) and S.standard_pressure == 1e5 and S.triple_point_temperature == real(273.16)
        assert keep[0].dtype == real and np.array_equal(keep[0], T0.astype(real)) and keep[1].shape == (g.Ny, g.Nx)
    assert forcings.compressible_surface_flux_conditions({}, g, True, False) == {}


def _header_struct(text, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), re.sub(r"/\*.*?\*/", "", text, flags=re.S), flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype, names = re.match(r"((?:const\s+)?\w+)\s+(.*)", decl, flags=re.S).groups()
        for n in names.split(","):
            n = n.strip()
            fields.append((n.lstrip("*"), ctype + (" *" if n.startswith("*") else "")))
    return fields


@pytest.mark.parametrize("header,real", [("breeze_hip.h", "double"), ("breeze_hip_f32.h", "float")])
def test_abi_symbols_and_struct_layout_match_the_headers(bz, header, real):
    from breeze_jl_amd import _lib
    with open(os.path.join(ROOT, "include", header), encoding="utf-8") as f:
        text = f.read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"int bz_set_compressible_surface_fluxes\(bz_ctx \*ctx, const bz_compressible_surface_fluxes \*fluxes\);", code)
    assert re.search(r"int bz_compressible_compute_flux_bc_tendencies\(bz_ctx \*ctx, const bz_compressible_state \*s, "
                     r"const bz_compressible_prognostic \*G\);", code)
    assert _lib.SYMBOLS["bz_set_compressible_surface_fluxes"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(_lib.bz_compressible_surface_fluxes)])
    assert _lib.SYMBOLS["bz_compressible_compute_flux_bc_tendencies"][1][1:] == [ctypes.POINTER(_lib.bz_compressible_state),
                                                                                 ctypes.POINTER(_lib.bz_compressible_prognostic)]
    T = _lib.types(8 if real == "double" else 4)
    creal = ctypes.c_double if real == "double" else ctypes.c_float
    kinds = {"int32_t": ctypes.c_int32, real: creal, f"const {real} *": ctypes.POINTER(creal), "bz_compressible_surface_flux": T.bz_compressible_surface_flux}
    for name in ("bz_compressible_surface_flux", "bz_compressible_surface_fluxes"):
        want = [(n, kinds[t]) for n, t in _header_struct(text, name)]
        assert [(n, t) for n, t in getattr(T, name)._fields_] == want, name
    w = ctypes.sizeof(creal)
    one = 8 + 3 * w
    one += (-one) % 8 + 8                            # the pointer is 8-byte aligned
    assert ctypes.sizeof(T.bz_compressible_surface_flux) == one
    whole = 3 * one + 7 * w
    assert ctypes.sizeof(T.bz_compressible_surface_fluxes) == whole + (-whole) % 8
    lib = _lib.load() if real == "double" else _lib.load_f32()
    for sym in ("bz_set_compressible_surface_fluxes", "bz_compressible_compute_flux_bc_tendencies"):
        assert hasattr(lib, sym)
