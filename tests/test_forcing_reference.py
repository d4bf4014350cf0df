"""oracle/forcings.py (compute_forcings, add_forcing_tendencies, add_relaxation_tendencies, add_field_forcing, add_flux_bc_tendencies, each
applied to zeroed G) against the independent long-double reference of tests/forcing_reference.py, TERM BY TERM, on every grid, stack and
state of tests/forcing_cases.py (the oracle model is built on all of them), over the cells the operator writes.

BOUND: 1e-13 of max|term|, the project's figure for one Float64 operator against a long-double one.  One term takes an addition that is
derived, not measured: the subsidence column.  Its profile takes DIFFERENCES of horizontal means that sit on a 300 K background, so the
Float64 rounding of the oracle's np.mean — c 2^-53 mean|field| with c the longest chain of additions of numpy's row-wise pairwise sum
(forcing_cases.sum_chain) — enters amplified by mean / difference of means; that part (forcing_cases.subsidence_bound, the construction the
device test uses for the kernels' sums) is added for the fields that carry subsidence and printed beside the measured error.  What the
rounding of the means cannot excuse is held at 1e-13 on its own: test_oracle_subsidence_profile_from_given_averages feeds the oracle's
subsidence_profile the reference's averages (rounded to Float64) and compares the profile alone.

The oracle adds Coriolis and column terms on the u face i = 0 between x walls and the v face j = 0 between y walls, where the device
tendency kernels — and therefore the reference — write nothing (the walls are closed; nothing reads G there).  The test prints
"oracle writes wall faces" for those fields and compares the written cells only.

MEASURED (x86-64, 80-bit long double): worst max|oracle - reference| / max|term| over all FORCING-CPU lines
  coriolis 2.4e-16 (waves, bomex moist, rv), column without subsidence 1.1e-16, energy 4.8e-16 (ragged, bomex moist), relaxation 2.4e-16
  (short, sponge_specific, rw), field forcing 8.9e-17, bottom fluxes 1.4e-14 (xwalls, bulk moist, rq: q^v - q^v+ loses a digit; every
  other flux is at 1e-15 or better);
  column with subsidence: 4.0e-12 of the term (waves, bomex dry, rtheta: means near 300 K, differences of a few hundredths of a kelvin)
  against a derived part of 1.3e-10; the profile from given averages 7.0e-16.
  No disagreement between the oracle and the reference was found on the written cells.  The smallest FORCING-SWITCH figure is 4.3e9 device
  tolerances (subsidence_dzf_shift on ragged, sub_theta).

SENSITIVITY: every keyword switch of the reference moves the term it belongs to by more than 1e3 x the device tolerance of
tests/test_forcing_device.py on a named grid and stack (FORCING-SWITCH lines); subsidence_dzf_shift, relaxation_w_centre_density and
bottom_dz_regular on stretched grids.  CLOSED FORMS are held by the reference alone.  AVERAGING: the points of every horizontal average
differ at the first level and in the interior; every term is within two orders of magnitude of the tendency it is added to on some grid."""
import functools

import numpy as np
import pytest

import forcing_cases as cases
import forcing_reference as ref

LD = ref.LD
TOLERANCE = 1e-13
CPU_CASES = [(n, s, False) for n in cases.GRIDS for s in cases.STACKS] + [(n, s, True) for n in cases.GRIDS for s in cases.MOIST_STACKS]
IDS = [f"{n}-{s}-{'moist' if m else 'dry'}" for n, s, m in CPU_CASES]


def _zero(m):
    for n in m.G:
        m.G[n][...] = 0.0


def _interior(m):
    return {n: m.grid.interior(m.G[n]).copy() for n in cases.FIELDS}          # rho w: faces 0 .. Nz - 1


def oracle_terms(name, stack_id, moist):
    """the oracle's terms, one sub-stack at a time on zeroed G: {term: {field: interior array}}"""
    from oracle.forcings import add_field_forcing, add_flux_bc_tendencies, add_forcing_tendencies, add_relaxation_tendencies, compute_forcings
    out = {}
    for part in ("coriolis", "column", "energy"):
        m = cases.oracle_model(name, stack_id, moist, only=part)
        compute_forcings(m)
        _zero(m)
        add_forcing_tendencies(m)
        out[part] = _interior(m)
        if part == "column":
            out["sub"] = dict(m.forcings.sub)
    m = cases.oracle_model(name, stack_id, moist, only="flux")
    _zero(m)
    add_flux_bc_tendencies(m)
    out["flux"] = _interior(m)
    _zero(m)
    if m.relaxation:
        add_relaxation_tendencies(m)
    out["relaxation"] = _interior(m)
    _zero(m)
    if m.field_forcing is not None:
        add_field_forcing(m)
    out["field"] = _interior(m)
    return out


@functools.lru_cache(maxsize=None)
def forced_scale(name, stack_id, moist):
    """max|G| per field of the oracle's whole forced tendency on the shared state: the scale the terms are added to"""
    from oracle.forcings import compute_forcings
    m = cases.oracle_model(name, stack_id, moist)
    compute_forcings(m)
    m.compute_tendencies()
    return {n: float(np.max(np.abs(m.grid.interior(m.G[n])))) for n in cases.FIELDS}


@functools.lru_cache(maxsize=None)
def reference_terms(name, stack_id, moist):
    return cases.reference_terms(name, stack_id, moist)


@pytest.mark.parametrize("name,stack_id,moist", CPU_CASES, ids=IDS)
def test_oracle_matches_long_double_reference(name, stack_id, moist):
    T, O = reference_terms(name, stack_id, moist), oracle_terms(name, stack_id, moist)
    S = cases.STACKS[stack_id]
    report, walls, bad = [], [], []
    for term in cases.VOLUME_TERMS + ("flux",):
        for field in cases.FIELDS:
            got = O[term][field]
            if field not in T[term]:
                assert np.all(got == 0), (term, field, "the oracle adds a term the reference does not have")
                continue
            want = T[term][field]
            if term == "flux":
                assert np.all(got[1:] == 0), (field, "a bottom flux above the first level")
                got = got[0]
            mask = ~np.isnan(want)
            if np.any(got[~mask] != 0):
                walls.append(field)
            scale = float(np.max(np.abs(want[mask])))
            assert scale > 0, (term, field)
            err = float(np.max(np.abs(got[mask] - want[mask])))
            bound = TOLERANCE * scale
            spec = {"ru": "u", "rv": "v", "rtheta": "theta", "rq": "q"}.get(field)
            extra = cases.subsidence_bound(name, stack_id, moist, spec, "numpy") if term == "column" and spec in S["subsidence"] else 0.0
            report.append(f"{term}/{field}={err / scale:.1e}" + (f"(sub bound {extra / scale:.1e})" if extra else ""))
            if not err < bound + extra:
                bad.append((term, field, err, bound, extra))
    print(f"FORCING-CPU {name} {stack_id} {'moist' if moist else 'dry'}:", " ".join(report),
          ("| oracle writes wall faces: " + ",".join(sorted(set(walls)))) if walls else "")
    assert not bad, bad


@pytest.mark.parametrize("name", list(cases.GRIDS))
def test_oracle_subsidence_profile_from_given_averages(name):
    """the profile formula alone — metric level, end cells, sign — at 1e-13, with the rounding of the means taken out: both sides start from
    the reference's averages rounded to Float64"""
    from oracle.forcings import subsidence_profile
    om = cases.dry_state(name)
    g, geo, C = om.grid, cases.geometry(om), cases.columns(name, "bomex")
    worst = 0.0
    for spec in ("u", "v", "theta", "q"):
        avg = np.asarray(ref.horizontal_average(geo, getattr(om, spec)), dtype=np.float64)
        want = ref.subsidence_profile(geo, C["ws"], avg)
        got = subsidence_profile(C["ws"], avg, g.dzf[g.Hz:g.Hz + g.Nz + 1])
        # differences of Float64 means: each profile entry is judged against the products that enter it, not against their cancelled difference
        scale = float(np.max(np.abs(np.asarray(C["ws"][1:-1], dtype=LD)) * np.max(np.abs(avg)) / np.min(geo.dzf_[1:-1])))
        worst = max(worst, float(np.max(np.abs(got - want))) / scale)
    print(f"FORCING-CPU {name} subsidence profile from given averages: {worst:.1e}")
    assert worst < TOLERANCE


# ---- closed forms, held by the reference alone -------------------------------------------------------------------------------------------------
def test_linear_mean_on_stretched_z_gives_minus_w_gamma_in_every_cell():
    om = cases.dry_state("ragged")
    geo = cases.geometry(om)
    zf = np.asarray(cases.z_faces("ragged"), dtype=LD)
    zc = (zf[1:] + zf[:-1]) / 2
    Gamma, w = LD("0.004"), LD("-1e-3")
    F = ref.subsidence_profile(geo, np.full(geo.Nz + 1, w), 300 + Gamma * zc)
    assert np.max(np.abs(F + w * Gamma)) < 1e-15 * abs(w * Gamma) * 300 / float(Gamma * zc[1])          # ends included: one-sided, same slope
    ws = np.array([cases.w_subsidence(float(z)) for z in zf], dtype=LD)
    F = ref.subsidence_profile(geo, ws, 300 + Gamma * zc)
    tol = 1e-15 * float(np.max(np.abs(ws)) * Gamma) * 300 / float(Gamma * zc[1])
    assert abs(F[3] + Gamma * (ws[3] + ws[4]) / 2) < tol and abs(F[0] + Gamma * ws[1]) < tol and abs(F[-1] + Gamma * ws[geo.Nz - 1]) < tol


def test_geostrophic_wind_gives_zero_momentum_forcing():
    """u = u_g, v = v_g: Coriolis and the geostrophic columns cancel in both components, to the Float64 rounding of the inputs"""
    name = "thin"
    om = cases.dry_state(name)
    g, geo, C = om.grid, cases.geometry(om), cases.columns(name, "momentum_only")
    f = cases.STACKS["momentum_only"]["f"]
    ug, vg = C["Fv"] / f, -C["Fu"] / f
    rho = np.zeros(g.Szc)
    rho[g.Hz:g.Hz + g.Nz] = C["rho"]
    ru = np.zeros_like(om.ru)
    rv = np.zeros_like(om.rv)
    ru[g.Hz:g.Hz + g.Nz] = (C["rho"] * ug)[:, None, None]
    rv[g.Hz:g.Hz + g.Nz] = (C["rho"] * vg)[:, None, None]
    cu, cv = ref.coriolis(geo, f, ru, rv)
    shape = (g.Nz, g.Ny, g.Nx)
    tu = cu + ref.column_term(geo, "u", C["rho"], C["Fu"], shape)
    tv = cv + ref.column_term(geo, "v", C["rho"], C["Fv"], shape)
    scale = f * float(np.max(C["rho"])) * 10.0
    assert np.max(np.abs(tu)) < 1e-15 * scale and np.max(np.abs(tv)) < 1e-15 * scale and np.max(np.abs(cu)) > 1e-2 * scale


def test_bulk_heat_flux_vanishes_at_the_surface_equivalent_theta():
    name = "thin"
    om = cases.dry_state(name)
    geo, c = cases.geometry(om), ref.CONSTANTS
    T0 = LD(cases.BULK["heat"][2])
    theta0 = T0 / (LD(cases.P0) / LD(cases.PST)) ** ((LD(c.R) / LD(c.Md)) / LD(c.cpd))
    assert abs(theta0 - T0) > 0.5
    theta = np.full_like(om.theta, float(theta0))
    dz = ref.bottom_dz(geo, cases.LZ)
    J = ref.bulk_fluxes(geo, c, cases.P0, cases.PST, om.u, om.v, theta, om.q, dz, heat=cases.BULK["heat"])["theta"]
    one_kelvin = ref.bulk_fluxes(geo, c, cases.P0, cases.PST, om.u, om.v, theta + 1.0, om.q, dz, heat=cases.BULK["heat"])["theta"]
    assert np.max(np.abs(J)) < 1e-13 * np.max(np.abs(one_kelvin)) and np.max(np.abs(one_kelvin)) > 0


# ---- the cases can see the mistakes the switches stand for ---------------------------------------------------------------------------------
SENSITIVITY = {      # switch: [(grid, stack, moist, term, field)]; volume terms are judged as the sum the device comparison sees
    "subsidence_dzf_shift": [("ragged", "sub_theta", False, "column", "rtheta"), ("short", "sub_q", False, "column", "rq"),
                             ("march", "bomex", True, "column", "ru")],
    "subsidence_ends_halved": [("short", "sub_u", False, "column", "ru"), ("thin", "sub_theta", False, "column", "rtheta")],
    "coriolis_two_point": [("ragged", "momentum_only", False, "coriolis", "ru"), ("ywalls", "momentum_only", False, "coriolis", "rv")],
    "coriolis_same_sign": [("ragged", "momentum_only", False, "coriolis", "rv")],
    "energy_dry_constants": [("thin", "bomex", True, "energy", "rtheta"), ("ragged", "bomex", False, "energy", "rtheta")],
    "drag_unaveraged_speed": [("ragged", "momentum_only", False, "flux", "ru"), ("xwalls", "bomex", False, "flux", "rv")],
    "bulk_square_of_mean": [("thin", "bulk", False, "flux", "ru"), ("ragged", "bulk", True, "flux", "rtheta")],
    "relaxation_w_centre_density": [("ragged", "sponge_specific", False, "relaxation", "rw"), ("thin", "sponge_specific", False, "relaxation", "rw")],
    "bottom_dz_regular": [("thin", "energy_flux", False, "flux", "rtheta"), ("ragged", "bomex", True, "flux", "rq"),
                          ("waves", "bulk", False, "flux", "rv")],
}


@pytest.mark.parametrize("switch", list(cases.SWITCHES))
def test_switched_reference_differs_by_a_thousand_device_tolerances(switch):
    assert SENSITIVITY[switch]
    for name, stack_id, moist, term, field in SENSITIVITY[switch]:
        base = reference_terms(name, stack_id, moist)
        broken = cases.reference_terms(name, stack_id, moist, **{switch: True})
        if term == "flux":
            a, b = base["flux"][field], broken["flux"][field]
            tolerance = 1e-13 * float(np.nanmax(np.abs(a)))
        else:
            (a, _), (b, _) = cases.tendency_sum(base, field), cases.tendency_sum(broken, field)
            tolerance, _ = cases.tendency_bound(name, stack_id, moist, field, base, forced_scale(name, stack_id, moist)[field],
                                                cases.device_sum_path(name, no_fuse_level_sums=True))
            tolerance = max(tolerance, cases.tendency_bound(name, stack_id, moist, field, base, forced_scale(name, stack_id, moist)[field],
                                                            cases.device_sum_path(name))[0])
        d = float(np.nanmax(np.abs(a - b)))
        print(f"FORCING-SWITCH {switch} ({name}, {stack_id}, {'moist' if moist else 'dry'}, {term}, {field}): {d / tolerance:.2e} device tolerances")
        assert d > 1e3 * tolerance, (switch, name, stack_id, d, tolerance)


# ---- conditions on the states ------------------------------------------------------------------------------------------------------------------
def _distinct_share(points):
    """share of cells in which the points of an average are pairwise different (coinciding points of a Flat direction count once)"""
    ok = np.ones(points[0].shape, dtype=bool)
    for a in range(len(points)):
        for b in range(a + 1, len(points)):
            ok &= points[a] != points[b]
    return float(ok.mean())


@pytest.mark.parametrize("moist", [False, True])
@pytest.mark.parametrize("name", list(cases.GRIDS))
def test_points_of_every_horizontal_average_differ(name, moist):
    """the four points (two on a Flat y) of the averages of rho v, v to the u point and of rho u, u to the v point, and the pairs of the
    centre averages of u and v, are pairwise different at the first level and in the interior: a wrong neighbour changes the result.  The
    planted runs of equal cells of the dry state are the exception (under 10 % of the cells)."""
    om = cases.state(name, moist)
    geo = cases.geometry(om)
    flat = geo.flat_y
    shares = {}
    for a, to in (("rv", "u"), ("v", "u"), ("ru", "v"), ("u", "v")):
        f = getattr(om, a)
        if to == "u":
            pts = [ref._at(geo, f, 0, -1), ref._at(geo, f, 0, 0)] + ([] if flat else [ref._at(geo, f, 1, -1), ref._at(geo, f, 1, 0)])
        else:
            pts = [ref._at(geo, f, 0, 0), ref._at(geo, f, 0, 1)] + ([] if flat else [ref._at(geo, f, -1, 0), ref._at(geo, f, -1, 1)])
        mask = np.zeros(pts[0].shape, dtype=bool)
        mask[ref.written(geo, to, pts[0].shape)] = True
        if geo.bounded[1 if a in ("rv", "v") else 2]:
            continue          # between walls the average takes the closed wall face (zero) in its first / last row: covered by the periodic grids
        for label, sl in (("first", slice(0, 1)), ("interior", slice(1, geo.Nz - 1))):
            shares[(a, to, label)] = _distinct_share([p[sl][mask[sl]] for p in pts])
    print(f"FORCING-AVERAGES {name} {'moist' if moist else 'dry'}: smallest share of distinct points {min(shares.values()):.3f}")
    assert min(shares.values()) >= 0.9, shares
    if moist:
        g = om.grid
        ql = g.interior(om.ql)
        cloudy = (ql > 0).mean(axis=(1, 2))
        print(f"FORCING-AVERAGES {name} cloud fraction per level:", " ".join(f"{c:.2f}" for c in cloudy))
        assert 0.05 < cloudy[0] < 0.95 and np.any((cloudy[1:] > 0.05) & (cloudy[1:] < 0.95)), cloudy


def test_every_term_is_visible_beside_the_tendency_it_is_added_to():
    """max|term| >= 1e-2 max|G_forced| on at least one grid per term and field: otherwise the first part of the device bound would hide it"""
    best = {}
    for name in cases.GRIDS:
        for stack_id, moist in (("bomex", False), ("bomex", True), ("momentum_only", False), ("sponge_density", False), ("sponge_specific", False),
                                ("sub_u", False), ("sub_v", False), ("sub_theta", False), ("sub_q", False)):
            T, G = reference_terms(name, stack_id, moist), forced_scale(name, stack_id, moist)
            for term in cases.VOLUME_TERMS:
                for field, t in T[term].items():
                    label = (term + ("+subsidence" if term == "column" and cases.STACKS[stack_id]["subsidence"] else ""), field,
                             "specific" if stack_id == "sponge_specific" else "")
                    r = float(np.nanmax(np.abs(t))) / G[field]
                    if r > best.get(label, (0.0,))[0]:
                        best[label] = (r, name, stack_id, moist)
    for label, (r, name, stack_id, moist) in sorted(best.items()):
        print(f"FORCING-RATIO {'/'.join(x for x in label if x)}: max|t| / max|G_forced| = {r:.2e} on {name}, {stack_id}{', moist' if moist else ''}")
    assert all(r >= 1e-2 for r, *_ in best.values()), {k: v for k, v in best.items() if v[0] < 1e-2}
