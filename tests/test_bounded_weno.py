"""Bounds-preserving WENO for moisture (second half): advection = (; rho_q = WENO(order = 5, bounds = (0, 1))),
/root/reference/src/Advection.jl:42-47, used by /root/reference/examples/rico.jl:184-190 and tropical_cyclone_world.jl:169.

PARITY UNPINNED: Breeze only adds the three `bounded_tracer_flux_divergence_{x,y,z}` of Oceananigans (not vendored) and divides by
the cell volume; the reference has no test that asserts a value of this operator.  The oracle restates the published limiter
(oracle/breeze_oracle.c: og_scalar_tendency_bounded); what can be pinned here are its defining properties:
  * where the limiter is inactive (theta = 1) the operator IS the plain WENO-5 flux divergence;
  * an independent numpy restatement of the 1-D formula agrees with the C oracle;
  * under a stirring bubble the overshoot of a sharp blob above its upper bound shrinks by more than 10x against plain WENO-5
    (the operator limits only a cell's own reconstructions, so it is not strictly bounds-preserving — see that test);
and the device kernel (gpu) matches the oracle: tendencies 1e-12, three steps 1e-9, same overshoot suppression on the device.

Pinned elsewhere, to an independent long-double statement of the formulas (tests/bounded_weno_reference.py,
tests/test_bounded_weno_reference.py): the oracle's y and z directions, the wall stencils of z (order 5 / 3 / upwind), the face densities
and stretched z, on rough states where both bounds bind.  tests/test_bounded_weno_clients.py runs the device kernel on those states for
moisture, the Kessler species and user tracers.  What remains unpinned is the reference package itself: Oceananigans is not vendored, no
value of this operator exists in the reference, and both statements could share one misreading of the published limiter."""
import ctypes as C

import numpy as np
import pytest

from helpers import PROG, bubble_theta, make_pair, push_state, randomize, relerr

EXT = ((-10e3, 10e3), (-10e3, 10e3), (0.0, 10e3))


def _p(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _tend(om, bounded, lo=0.0, hi=1.0):
    G = np.zeros_like(om.q)
    if bounded:
        om.lib.og_scalar_tendency_bounded(C.byref(om.cg), _p(G), _p(om.u), _p(om.v), _p(om.w), _p(om.q), C.c_double(lo), C.c_double(hi))
    else:
        om.lib.og_scalar_tendency(C.byref(om.cg), _p(G), _p(om.u), _p(om.v), _p(om.w), _p(om.q))
    return om.grid.interior(G)


def test_inactive_limiter_reduces_to_plain_weno(oracle):
    g = oracle.Grid((24, 16, 12), x=EXT[0], y=EXT[1], z=EXT[2])
    om = oracle.OracleModel(g, potential_temperature=300.0)
    randomize(om, seed=3, amp_q=1e-3)
    g.interior(om.q)[...] = 0.4 + g.interior(om.q)           # smooth, far from both bounds
    g.interior(om.rq)[...] = om.ref.density[g.Hz:g.Hz + g.Nz][:, None, None] * g.interior(om.q)
    om.update_state(compute_tendencies=False)
    plain, bounded = _tend(om, False), _tend(om, True)
    assert np.max(np.abs(plain)) > 0
    assert relerr(bounded, plain) < 1e-13
    # bounds that bite change the answer
    assert relerr(_tend(om, True, 0.3995, 0.4005), plain) > 1e-6


def _numpy_bounded_div_x(c, flux, lo, hi):
    """Independent restatement for a periodic row: c cell values, flux = rho A u at the faces (face i left of cell i)."""
    def weno5(a, b, cc, d, e):
        # 3 x Jiang-Shu, the scaling of Oceananigans' coefficient tables that the oracle restates (it matters through eps = 1e-8)
        b0 = 3 * (13 / 12 * (cc - 2 * d + e) ** 2 + 0.25 * (3 * cc - 4 * d + e) ** 2)
        b1 = 3 * (13 / 12 * (b - 2 * cc + d) ** 2 + 0.25 * (b - d) ** 2)
        b2 = 3 * (13 / 12 * (a - 2 * b + cc) ** 2 + 0.25 * (a - 4 * b + 3 * cc) ** 2)
        tau = abs(b0 - b2)
        a0, a1, a2 = 0.3 * (1 + (tau / (b0 + 1e-8)) ** 2), 0.6 * (1 + (tau / (b1 + 1e-8)) ** 2), 0.1 * (1 + (tau / (b2 + 1e-8)) ** 2)
        p0, p1, p2 = cc / 3 + 5 * d / 6 - e / 6, -b / 6 + 5 * cc / 6 + d / 3, a / 3 - 7 * b / 6 + 11 * cc / 6
        return (a0 * p0 + a1 * p1 + a2 * p2) / (a0 + a1 + a2)
    N = len(c)
    cc = lambda i: c[i % N]
    left = lambda f: weno5(cc(f - 3), cc(f - 2), cc(f - 1), cc(f), cc(f + 1))       # value at face f from the left
    right = lambda f: weno5(cc(f + 2), cc(f + 1), cc(f), cc(f - 1), cc(f - 2))
    ubp = lambda u, l, r: ((u + abs(u)) * l + (u - abs(u)) * r) / 2
    out = np.zeros(N)
    for i in range(N):
        cpL, cpR, cmL, cmR = left(i + 1), right(i + 1), left(i), right(i)
        pt = (c[i] - 5 / 18 * cmR - 5 / 18 * cpL) / (1 - 10 / 18)
        M, m = max(pt, cpL, cmR), min(pt, cpL, cmR)
        th = min(abs((hi - c[i]) / (M - c[i] + 1e-20)), abs((lo - c[i]) / (m - c[i] + 1e-20)), 1.0)
        cpL, cmR = th * (cpL - c[i]) + c[i], th * (cmR - c[i]) + c[i]
        out[i] = ubp(flux[(i + 1) % N], cpL, cpR) - ubp(flux[i], cmL, cmR)
    return out


def test_c_oracle_matches_independent_numpy_restatement(oracle):
    """x-only flow over a row with a sharp-edged blob touching both bounds: the C oracle against the numpy formula."""
    g = oracle.Grid((32, 8, 6), x=EXT[0], y=EXT[1], z=EXT[2])
    om = oracle.OracleModel(g, potential_temperature=300.0)
    rng = np.random.default_rng(5)
    row = np.clip(np.where((np.arange(32) > 8) & (np.arange(32) < 20), 1.0, 0.0) + 0.02 * rng.standard_normal(32), 0.0, 1.0)
    urow = 4.0 * np.sin(2 * np.pi * np.arange(32) / 32 + 0.4) + 1.0          # changes sign: both upwind branches
    g.interior(om.q)[...] = row[None, None, :]
    g.interior(om.u)[...] = urow[None, None, :]
    om.v[...] = 0.0
    om.w[...] = 0.0
    for f in (om.q, om.u):
        om.lib.og_fill_halo_periodic_xy(C.byref(om.cg), _p(f), C.c_int(f.shape[0]))
    got = _tend(om, True)
    k = 2
    rho = om.ref.density[g.Hz + k]
    dzc = (EXT[2][1] - EXT[2][0]) / g.Nz
    Ax = g.dy * dzc
    want = -_numpy_bounded_div_x(row, rho * Ax * urow, 0.0, 1.0) / (g.dx * g.dy * dzc)
    assert relerr(got[k, 3, :], want) < 1e-10          # expanded (oracle) vs squared-difference (here) smoothness indicators


QMAX = 0.01       # the blob's vapour mass fraction and the upper bound of the scheme in the stirring tests


def _blob(x, y, z):
    return QMAX * ((np.abs(x) < 3e3) & (np.abs(y - 500.0) < 3e3) & (np.abs(z - 3000.0) < 1.5e3)).astype(float)


def test_bounded_scheme_suppresses_the_overshoots_of_plain_weno(oracle):
    """What the scheme is for (examples/rico.jl: q^e, q^cl, q^r should not leave their bounds): a sharp-edged blob of q = QMAX in
    q = 0 stirred by the rising bubble + a mean wind, 48 steps, bounds = (0, QMAX).
    The operator as Oceananigans writes it (and as restated here) limits only the two reconstructions that START in a cell; the
    inflow value of a face is the neighbour's UNLIMITED reconstruction, so the scheme is neither strictly conservative nor strictly
    bounds-preserving (measured on a passive tracer in uniform 1-D flow: undershoot -9.7e-7 against -1.45e-6 for plain WENO-5).
    The assertion is therefore the honest one: the overshoot above the upper bound shrinks by more than an order of magnitude,
    the undershoot does not grow, and the mass drift stays small."""
    th = bubble_theta(300.0, 9.81)
    res = {}
    for bounded in (True, False):
        g = oracle.Grid((24, 24, 20), x=EXT[0], y=EXT[1], z=EXT[2])
        om = oracle.OracleModel(g, potential_temperature=300.0)
        if bounded:
            om.bounded = {"rq": (0.0, QMAX)}
        om.set(theta=th, u=12.0, v=-7.0, qt=_blob)
        for _ in range(48):
            om.time_step(5.0)
        q = g.interior(om.rq) / om.ref.density[g.Hz:g.Hz + g.Nz][:, None, None]
        res[bounded] = (q.min() / QMAX, q.max() / QMAX - 1.0, float(np.sum(g.interior(om.rq))))
    assert res[False][1] > 1e-2, res[False]                      # plain WENO-5 overshoots by more than 1 % here
    assert res[True][1] < 0.1 * res[False][1], (res[True], res[False])
    assert res[True][0] > 1.0001 * res[False][0] - 1e-15, (res[True], res[False])      # undershoot not worse
    assert abs(res[True][2] - res[False][2]) / res[False][2] < 5e-3


# ---- device ------------------------------------------------------------------------------------------------------------------
def _pair(oracle, bz, size, bounds=(0.0, 1.0)):
    z = EXT[2]
    og = oracle.Grid(size, x=EXT[0], y=EXT[1], z=z)
    om = oracle.OracleModel(og, potential_temperature=300.0)
    om.bounded = {"rq": bounds}
    grid = bz.RectilinearGrid(size, x=EXT[0], y=EXT[1], z=z)
    hm = bz.AtmosphereModel(grid, dynamics=bz.AnelasticDynamics(bz.ReferenceState(grid, potential_temperature=300.0)),
                            advection={"momentum": bz.WENO(), "ρθ": bz.WENO(), "ρqᵛ": bz.WENO(bounds=bounds)})
    return om, hm


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(32, 20, 16), (70, 9, 12)])
def test_device_bounded_tendency_matches_oracle(oracle, bz, size):
    om, hm = _pair(oracle, bz, size)
    randomize(om, seed=13, amp_q=0.3)                         # |q| up to ~0.5: the upper bound is far, the lower bound bites
    om.compute_tendencies()
    push_state(om, hm, names=("ru", "rv", "rw", "rtheta", "rq", "u", "v", "w", "theta", "q", "T"))
    bz.compute_tendencies_(hm)
    hm.synchronize()
    for n, k in PROG.items():
        got, want = hm.G[k].interior_cpu(), om.grid.interior(om.G[n], zface=(n == "rw"))
        assert np.max(np.abs(got - want)) / max(np.max(np.abs(want)), 1e-30) < 1e-12, n
    # and it is not the plain tendency
    plain = _tend(om, False)
    assert relerr(hm.G["ρq"].interior_cpu(), plain) > 1e-4


@pytest.mark.gpu
def test_device_bounded_steps_match_oracle_and_suppress_overshoots(oracle, bz):
    om, hm = _pair(oracle, bz, (24, 24, 20), bounds=(0.0, QMAX))
    th = bubble_theta(300.0, 9.81)
    om.set(theta=th, u=12.0, v=-7.0, qt=_blob)
    hm.set(θ=th, u=12.0, v=-7.0, qᵗ=_blob)
    for _ in range(3):
        om.time_step(5.0)
        hm.time_step(5.0)
    hm.synchronize()
    for n, k in PROG.items():
        got, want = hm.prognostic_fields()[k].interior_cpu(), om.grid.interior(getattr(om, n), zface=(n == "rw"))
        # sharp-edged blob on a coarse grid: the WENO weights of kinked data amplify FMA-contraction differences (DESIGN.md §6
        # "Strict-parity library"): 1e-8 here instead of the 1e-9 of the smooth-bubble step tests
        assert np.max(np.abs(got - want)) / max(np.max(np.abs(want)), 1e-3) < 1e-8, n
    for _ in range(45):
        hm.time_step(5.0)
    hm.synchronize()
    q = hm.specific_moisture.interior_cpu()
    assert q.max() / QMAX - 1.0 < 3e-3 and q.min() / QMAX > -1.1e-3, (q.min(), q.max())      # plain WENO-5: +3.2e-2 (CPU test above)


def test_host_rejects_unsupported_bounded_requests(bz):
    import torch
    from breeze_jl_amd.model import _split_advection
    base, req, *_ = _split_advection({"momentum": bz.WENO(), "ρqᵉ": bz.WENO(bounds=(0, 1)), "ρqʳ": bz.WENO(bounds=(0, 1))}, ())
    assert base.order == 5 and req == {"moisture": 1, "microphysical_species": 1, "tracers": 0, "lower": 0.0, "upper": 1.0}
    assert _split_advection(bz.WENO(), ())[1] is None
    with pytest.raises(NotImplementedError):
        _split_advection({"momentum": bz.WENO(bounds=(0, 1))}, ())
    with pytest.raises(NotImplementedError):
        _split_advection(bz.WENO(bounds=(0, 1)), ())
    with pytest.raises(ValueError):
        bz.WENO(bounds=(1, 0))


def test_host_rejects_bounds_on_a_part_of_a_class(bz):
    """one mask bit per class in the library: bounds on one tracer of two, or on one Kessler species, would limit the other as well"""
    from breeze_jl_amd.model import _SPECIES_KEYS, _check_bounded_clients
    W, B = bz.WENO(), bz.WENO(bounds=(0, 1))
    _check_bounded_clients(W, ("a", "b"), _SPECIES_KEYS)
    _check_bounded_clients({"momentum": W, "ρθ": W, "ρqᵉ": B}, ("a", "b"), _SPECIES_KEYS)          # moisture alone: no class is split
    _check_bounded_clients({"momentum": W, "a": B, "ρb": B, "ρqᶜˡ": B, "ρqʳ": B}, ("a", "b"), _SPECIES_KEYS)
    for advection, tracers, unnamed in (({"momentum": W, "a": B}, ("a", "b"), "b"), ({"momentum": W, "a": W, "ρb": B}, ("a", "b"), "a"),
                                        ({"momentum": W, "ρqʳ": B}, (), "ρqᶜˡ"), ({"momentum": W, "ρqᶜˡ": B, "ρqʳ": W}, ("a",), "ρqʳ")):
        with pytest.raises(NotImplementedError) as e:
            _check_bounded_clients(advection, tracers, _SPECIES_KEYS)
        assert repr(unnamed) in str(e.value), (unnamed, str(e.value))
    grid = bz.RectilinearGrid((8, 8, 8), x=EXT[0], y=EXT[1], z=EXT[2])
    with pytest.raises(NotImplementedError, match="'b'"):          # the constructor asks, before it needs a GPU
        bz.AtmosphereModel(grid, advection={"momentum": W, "ρθ": W, "a": B}, tracers=("a", "b"))


def test_host_rejects_bounds_on_species_the_model_does_not_carry(bz):
    """the library limits the species of a Kessler model only: on any other model the request would be a silent plain WENO-5 run"""
    from breeze_jl_amd.model import _check_bounded_clients
    W, B = bz.WENO(), bz.WENO(bounds=(0, 1))
    for key in ("ρqᶜˡ", "ρqʳ"):
        with pytest.raises(ValueError, match=key):
            _check_bounded_clients({"momentum": W, "ρqᵉ": B, key: B}, (), ())
    _check_bounded_clients({"momentum": W, "ρqᶜˡ": W, "ρqʳ": W}, (), ())          # without bounds the key asks for nothing the library gates
    grid = bz.RectilinearGrid((8, 8, 8), x=EXT[0], y=EXT[1], z=EXT[2])
    for microphysics in (None, bz.SaturationAdjustment(equilibrium=bz.WarmPhaseEquilibrium())):
        with pytest.raises(ValueError, match="ρqᶜˡ"):
            bz.AtmosphereModel(grid, advection={"momentum": W, "ρθ": W, "ρqᶜˡ": B, "ρqʳ": B}, microphysics=microphysics)


@pytest.mark.gpu
def test_bounded_moisture_on_library_slabs_matches_oracle(oracle, bz):
    """examples/rico.jl:184-190's bounds-preserving moisture advection on y-slabs (operator-by-operator distributed step): two ranks sharing
    the GPU through the in-process transport against the single-process oracle."""
    import threading
    import uuid
    import torch
    from breeze_jl_amd import distributed as bz_dist
    size = (24, 24, 20)
    og = oracle.Grid(size, x=EXT[0], y=EXT[1], z=EXT[2])
    om = oracle.OracleModel(og, potential_temperature=300.0)
    om.bounded = {"rq": (0.0, QMAX)}
    th = bubble_theta(300.0, 9.81)
    om.set(theta=th, u=12.0, v=-7.0, qt=_blob)
    for _ in range(3):
        om.time_step(5.0)
    G = bz.RectilinearGrid(size, x=EXT[0], y=EXT[1], z=EXT[2])
    x, y, z = og.nodes("ccc")
    full = {"θ": np.broadcast_to(th(x, y, z), (size[2], size[1], size[0])).copy(), "q": np.broadcast_to(_blob(x, y, z), (size[2], size[1], size[0])).copy()}
    world, group = 2, "local:" + uuid.uuid4().hex
    models, errors = [None] * world, []

    def run(rank):
        try:
            torch.cuda.set_device(0)
            with torch.cuda.stream(torch.cuda.Stream()):
                m = bz_dist.LibrarySlabAtmosphereModel(G, rank, world, transport=group, device="cuda:0", potential_temperature=300.0,
                                                       advection={"momentum": bz.WENO(), "ρθ": bz.WENO(), "ρqᵛ": bz.WENO(bounds=(0.0, QMAX))})
                Ny = size[1] // world
                sl = slice(rank * Ny, (rank + 1) * Ny)
                m.set(θ=full["θ"][:, sl, :], u=12.0, v=-7.0, qᵗ=full["q"][:, sl, :])
                for _ in range(3):
                    m.time_step(5.0)
                m.synchronize()
            models[rank] = m
        except Exception as e:      # noqa: BLE001
            import traceback
            errors.append((rank, repr(e), traceback.format_exc()))

    threads = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for n, k in PROG.items():
        got = np.concatenate([m.prognostic_fields()[k].interior_cpu() for m in models], axis=1)
        want = og.interior(getattr(om, n), zface=(n == "rw"))
        assert np.max(np.abs(got - want)) / max(np.max(np.abs(want)), 1e-3) < 1e-8, n
