"""The forcing, sponge and bottom-flux kernels of csrc/bz_forcing.hip (k_level_sums, k_level_wave_sums, k_level_reduce, k_subsidence_profiles,
k_apply_forcings, k_apply_relaxation, k_bottom_flux, k_bulk_bottom_flux) and their copies in the RK epilogues of k6_u / k6_v against THE
LONG-DOUBLE REFERENCE of tests/forcing_reference.py, on the grids, stacks and states of tests/forcing_cases.py.  States go into the device
model bit for bit (helpers.push_state); a saturation-adjustment model then runs update_state_ and every diagnosed field, q^v and q^l
included, is read back as the reference's input.  Switches are read when the context is created: monkeypatch.setenv before the model is built.

(a) BOTTOM FLUXES ALONE.  Every G is zeroed, bz.compute_flux_bc_tendencies_ leaves the flux term itself: |G - reference| < 1e-13
    max|reference| per field on the first level, exactly 0 above it, on G(rho w), in the halos and on the unwritten wall faces; a second call
    doubles every value (the operator adds).

(b) THE FORCING PASS INSIDE bz_compute_tendencies.  Two contexts on the same pushed state, with and without the stack: D = G_forced -
    G_unforced over the written cells is the sum t of the terms the stack adds to that field, each by one read-modify-write of G, so
        |D - t| <= m 2^-53 max|G_forced| + 1e-13 max|t| (+ the subsidence part)
    with m the number of separate additions (Coriolis 1, subsidence + static column 1, energy 1, relaxation 1, field forcing 1).  The
    subsidence part is the rounding of the kernels' horizontal sums, derived from the code (forcing_cases.sum_chain: k_level_sums where
    Nx % 64 != 0 or under BZ_NO_FUSE_LEVEL_SUMS=1, k_level_wave_sums + k_level_reduce otherwise) and carried through the profile
    (forcing_cases.subsidence_bound).  Outside the written cells — wall faces, halos — G_forced and G_unforced are bit-identical, and a second
    call of compute_tendencies_ leaves the same bits.  A host call sums in its own pass, so its record is "subsidence_averages" on both
    paths ("subsidence_averages_from_wave_sums" is the record of sums that rode on the projection kernel inside a step: section (c)); which
    of the two kernels ran is decided by Nx % 64 and the switch, not visible in the record name.

(c) ONE SET OF TERMS, EVERY TIER.  Two whole steps through the tier the model picks and through BZ_NO_FOLD_FORCING, BZ_NO_FUSE_FORCING,
    BZ_NO_FUSE_RK, BZ_NO_FUSED (and BZ_NO_FUSE_LEVEL_SUMS for bomex on "march"; BZ_NO_LEAN for the momentum-only stack, which is what sends it
    to the fused-RK fold) against the operator sequence bz.time_step_(m, dt, whole_step=False): every prognostic field and u, w, theta, T
    over whole parent arrays at 1e-12 of the field scale (momentum components share one scale, as do u and w).  dt = 3 s of
    tests/test_forcings.py (dz = 187.5 m) scaled by the smallest dz of the grid.  Records (of the second step: the first opens with
    update_state_ and its per-operator tendencies on every tier): the lean seam never enters the forcing pass
    ("forcing_tendencies" absent for the momentum-only stack it carries, present on the operator tier); the fold and BZ_NO_FOLD_FORCING
    both record "forcing_tendencies" (the folded pass still opens its record for the scalar terms), so there the switch decides; sums that
    ride on the projection kernel record "subsidence_averages_from_wave_sums" on "march" and never on "ragged" or under
    BZ_NO_FUSE_LEVEL_SUMS.

MEASURED on the MI355X: NOT YET.  No device was available while these tests were written, so the table of the worst error per group and
stack against its bound is still to be filled in from the FORCING-DEVICE lines of the first device run, and the record-name
assertions of (b) and (c) are read from the code (csrc/bz_forcing.hip, csrc/bz_step.hip), not observed.  What is measured is the CPU side
(tests/test_forcing_reference.py): the oracle agrees with the reference to 4.8e-16 per term (1.4e-14 for the vapour flux) and every switch
of the reference moves its term by more than 4e9 device tolerances.  The bounds above are derived and are not to be tightened to the
numbers a device run gives.
"""
import numpy as np
import pytest

import forcing_cases as cases
from helpers import PROG, push_state

pytestmark = pytest.mark.gpu

LD = cases.LD
SWITCHES = ("BZ_NO_FOLD_FORCING", "BZ_NO_FUSE_FORCING", "BZ_NO_FUSE_RK", "BZ_NO_FUSED", "BZ_NO_FUSE_LEVEL_SUMS", "BZ_NO_LEAN", "BZ_NO_K6_STORED")
PUSHED = ("ru", "rv", "rw", "rtheta", "rq", "u", "v", "w", "theta", "q", "T")
SENTINEL = 1.5


def _environment(monkeypatch, switch=None):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    if switch:
        monkeypatch.setenv(switch, "1")


def _pushed_model(bz, name, stack_id, moist):
    """the device model holding the shared state, and the state arrays as the kernels see them (None: the pushed oracle arrays)"""
    from helpers import ORACLE_TO_HIP
    om = cases.state(name, moist)
    hm = cases.device_model(bz, name, stack_id, moist)
    push_state(om, hm, names=PUSHED)
    fields = None
    if moist:
        bz.update_state_(hm, compute_tendencies=False)
        hm.synchronize()
        fields = {n: ORACLE_TO_HIP[n](hm).parent.cpu().numpy() for n in PUSHED}
        fields["qv"], fields["ql"] = (hm.microphysical_fields[k].parent.cpu().numpy() for k in ("qᵛ", "qˡ"))
        assert (om.grid.interior(fields["ql"])[0] > 0).any() and (om.grid.interior(fields["ql"])[1:] > 0).any()
    hm.synchronize()
    return om, hm, fields


def _G(hm):
    hm.synchronize()
    return {n: hm.G[k].parent.cpu().numpy() for n, k in PROG.items()}


def _label(name, stack_id, moist, switch=None):
    return f"{name} {stack_id}{' moist' if moist else ''}{' ' + switch if switch else ''}"


# ---- (a) bottom fluxes alone ---------------------------------------------------------------------------------------------------------------
FLUX_GRIDS = ("ragged", "thin", "flat", "ywalls", "xwalls", "waves")
FLUX_STACKS = [("bomex", False), ("bomex_eps0", False), ("momentum_only", False), ("bulk", False), ("energy_flux", False),
               ("bomex", True), ("bomex_eps0", True), ("bulk", True), ("energy_flux", True)]
FLUX_RUNS = [(n, s, m) for s, m in FLUX_STACKS for n in FLUX_GRIDS]


@pytest.mark.parametrize("name,stack_id,moist", FLUX_RUNS, ids=[_label(*r).replace(" ", "-") for r in FLUX_RUNS])
def test_bottom_fluxes_alone(bz, name, stack_id, moist, monkeypatch):
    _environment(monkeypatch)
    om, hm, fields = _pushed_model(bz, name, stack_id, moist)
    g = om.grid
    T = cases.reference_terms(name, stack_id, moist, fields=fields)["flux"]
    assert T, "the stack has no bottom flux"
    for k in PROG.values():
        hm.G[k].parent.zero_()
    bz.compute_flux_bc_tendencies_(hm)
    once = _G(hm)
    bz.compute_flux_bc_tendencies_(hm)
    twice = _G(hm)
    errs = {}
    for field in cases.FIELDS:
        parent = once[field].copy()
        first = parent[g.Hz, g.Hy:g.Hy + g.Ny, g.Hx:g.Hx + g.Nx].copy()
        parent[g.Hz, g.Hy:g.Hy + g.Ny, g.Hx:g.Hx + g.Nx] = 0.0
        assert not parent.any(), (field, "a bottom flux outside the first level of the interior")
        assert np.array_equal(twice[field], 2.0 * once[field]), (field, "the second call does not double the values")
        if field not in T:
            assert not first.any(), (field, "a flux the stack does not hold")
            continue
        want = T[field]
        mask = ~np.isnan(want)
        assert not first[~mask].any(), (field, "a flux on an unwritten wall face")
        scale = float(np.max(np.abs(want[mask])))
        errs[field] = float(np.max(np.abs(first[mask] - want[mask]))) / scale
    print(f"FORCING-DEVICE (a) {_label(name, stack_id, moist)}:", " ".join(f"{n}={e:.2e}" for n, e in errs.items()), "| bound 1e-13")
    assert set(errs) == set(T) and all(e < 1e-13 for e in errs.values()), errs


# ---- (b) the forcing pass inside bz_compute_tendencies --------------------------------------------------------------------------------------
ALL_GRIDS = tuple(cases.GRIDS)
PASS_RUNS = [(n, s, m, None) for s, m in (("bomex", False), ("bomex", True), ("momentum_only", False), ("sponge_density", False),
                                          ("sponge_specific", False)) for n in ALL_GRIDS]
PASS_RUNS += [(n, s, False, None) for s in cases.SUBSIDENCE_ONE for n in ("ragged", "march", "waves", "thin", "flat", "short")]
PASS_RUNS += [(n, s, m, "BZ_NO_FUSE_LEVEL_SUMS") for n in ("march", "waves")
              for s, m in (("bomex", False), ("bomex", True)) + tuple((s, False) for s in cases.SUBSIDENCE_ONE)]
_unforced = {}


def _tendencies(bz, hm):
    """G of every field after compute_tendencies_ on a sentinel, the profile records of the launch; the second call must leave the same bits"""
    for k in PROG.values():
        hm.G[k].parent.fill_(SENTINEL)
    hm.profile_enable()
    hm.profile_reset()
    bz.compute_tendencies_(hm)
    G = _G(hm)
    records = set(hm.profile())
    bz.compute_tendencies_(hm)
    again = _G(hm)
    for n in G:
        assert np.array_equal(G[n], again[n], equal_nan=True), (n, "a second compute_tendencies_ changes bits")
    return G, records


def _unforced_tendencies(bz, name, moist):
    """the tendencies of the context without a stack on the same pushed state: computed once per grid and state, never changed"""
    if (name, moist) not in _unforced:
        _, hm, _ = _pushed_model(bz, name, None, moist)
        G, _ = _tendencies(bz, hm)
        for a in G.values():
            a.setflags(write=False)
        _unforced[(name, moist)] = G
    return _unforced[(name, moist)]


@pytest.mark.parametrize("name,stack_id,moist,switch", PASS_RUNS, ids=[_label(*r).replace(" ", "-") for r in PASS_RUNS])
def test_forcing_pass_adds_the_reference_terms(bz, name, stack_id, moist, switch, monkeypatch):
    _environment(monkeypatch, switch)
    om, hm, fields = _pushed_model(bz, name, stack_id, moist)
    g, S = om.grid, cases.STACKS[stack_id]
    T = cases.reference_terms(name, stack_id, moist, fields=fields)
    forced, records = _tendencies(bz, hm)
    plain = _unforced_tendencies(bz, name, moist)
    path = cases.device_sum_path(name, no_fuse_level_sums=switch == "BZ_NO_FUSE_LEVEL_SUMS")
    report, bad = [], []
    for field in cases.FIELDS:
        t, m = cases.tendency_sum(T, field)
        differs = forced[field] != plain[field]
        if t is None:
            assert not differs.any(), (field, "the stack holds no term of this field")
            continue
        mask = ~np.isnan(t)
        inner = g.interior(differs)
        assert not inner[~mask].any(), (field, "G_forced and G_unforced differ on an unwritten wall face")
        inner[...] = False
        assert not differs.any(), (field, "G_forced and G_unforced differ outside the interior")
        Gf = g.interior(forced[field])
        D = np.asarray(Gf, dtype=LD) - np.asarray(g.interior(plain[field]), dtype=LD)
        G_max = float(np.max(np.abs(Gf[mask])))
        bound, parts = cases.tendency_bound(name, stack_id, moist, field, T, G_max, path, fields)
        err = float(np.max(np.abs(D[mask] - t[mask])))
        t_max = float(np.max(np.abs(t[mask])))
        report.append(f"{field}: err={err:.2e} bound={bound:.2e} (m={m}: {parts[0]:.1e} + {parts[1]:.1e} + sums {parts[2]:.1e}) t/G={t_max / G_max:.1e}")
        if not err <= bound:
            bad.append((field, err, bound))
    print(f"FORCING-DEVICE (b) {_label(name, stack_id, moist, switch)} [{path if S['subsidence'] else 'no sums'}]:", " | ".join(report),
          "| records", ",".join(sorted(r for r in records if "forcing" in r or "subsidence" in r)))
    if S["f"] or S["geostrophic"] or S["subsidence"] or S["drying"] or S["cooling"]:
        assert "forcing_tendencies" in records, sorted(records)
    if S["subsidence"]:
        assert "subsidence_averages" in records and "subsidence_averages_from_wave_sums" not in records, sorted(records)
    if S["relax"] or S["field_forcing"]:
        assert "relaxation_forcings" in records, sorted(records)
    assert not bad, bad


# ---- (c) one set of terms, every tier ----------------------------------------------------------------------------------------------------------
STEP_CASES = [("bomex", False, "ragged"), ("bomex", False, "march"), ("bomex", True, "ragged"), ("bomex", True, "march"),
              ("momentum_only", False, "ragged"), ("momentum_only", False, "ywalls")]
TIERS = (None, "BZ_NO_FOLD_FORCING", "BZ_NO_FUSE_FORCING", "BZ_NO_FUSE_RK", "BZ_NO_FUSED")
STEP_RUNS = [(s, m, n, t) for s, m, n in STEP_CASES for t in TIERS]
STEP_RUNS += [("bomex", m, "march", "BZ_NO_FUSE_LEVEL_SUMS") for m in (False, True)]
STEP_RUNS += [("momentum_only", False, n, "BZ_NO_LEAN") for n in ("ragged", "ywalls")]
_sequence = {}


def _time_step(name):
    return 3.0 * float(np.min(np.diff(cases.z_faces(name)))) / 187.5


def _two_steps(bz, name, stack_id, moist, whole_step):
    om, hm, _ = _pushed_model(bz, name, stack_id, moist)
    bz.time_step_(hm, _time_step(name), whole_step=whole_step)
    hm.profile_enable()          # the records of the second step: the first one opens with update_state_ and its per-operator tendencies
    hm.profile_reset()
    bz.time_step_(hm, _time_step(name), whole_step=whole_step)
    hm.synchronize()
    out = {k: f.cpu() for k, f in hm.prognostic_fields().items()}
    out.update(u=hm.velocities["u"].cpu(), w=hm.velocities["w"].cpu(), theta=hm.potential_temperature.cpu(), T=hm.temperature.cpu())
    return out, set(hm.profile())


@pytest.mark.parametrize("stack_id,moist,name,switch", STEP_RUNS, ids=[_label(n, s, m, t).replace(" ", "-") for s, m, n, t in STEP_RUNS])
def test_every_tier_equals_the_operator_sequence(bz, stack_id, moist, name, switch, monkeypatch):
    _environment(monkeypatch)
    key = (stack_id, moist, name)
    if key not in _sequence:          # the operator sequence, once per case
        _sequence[key] = _two_steps(bz, name, stack_id, moist, whole_step=False)[0]
    want = _sequence[key]
    _environment(monkeypatch, switch)
    got, records = _two_steps(bz, name, stack_id, moist, whole_step=True)
    momentum = max(float(np.abs(want[k]).max()) for k in ("ρu", "ρv", "ρw"))
    velocity = max(float(np.abs(want[k]).max()) for k in ("u", "w"))
    errs = {}
    for k in want:
        scale = momentum if k in ("ρu", "ρv", "ρw") else velocity if k in ("u", "w") else max(float(np.abs(want[k]).max()), 1e-3)
        errs[k] = float(np.abs(got[k] - want[k]).max()) / scale
    print(f"FORCING-DEVICE (c) {_label(name, stack_id, moist, switch)} dt={_time_step(name):.2f}:", " ".join(f"{k}={e:.2e}" for k, e in errs.items()),
          "| records", ",".join(sorted(r for r in records if "forcing" in r or "subsidence" in r or "flux_bc" in r)))
    moved = float(np.abs(want["ρθ"] - cases.state(name, moist).rtheta).max())
    assert moved > 0
    if stack_id == "momentum_only":
        assert "flux_bc_tendencies" in records, sorted(records)
        if switch in (None, "BZ_NO_FOLD_FORCING"):          # the lean seam: the terms ride the RK epilogues of k6_u / k6_v, no forcing pass
            assert "forcing_tendencies" not in records, sorted(records)
        if switch == "BZ_NO_FUSED":
            assert "forcing_tendencies" in records, sorted(records)
    else:
        assert "forcing_tendencies" in records, sorted(records)
        rides = name == "march" and switch in (None, "BZ_NO_FOLD_FORCING")
        assert ("subsidence_averages_from_wave_sums" in records) == rides, sorted(records)
    assert all(e < 1e-12 for e in errs.values()), errs
