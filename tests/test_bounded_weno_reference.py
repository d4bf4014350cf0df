"""The C oracle's bounds-preserving WENO operator (oracle/breeze_oracle.c: og_scalar_tendency_bounded) against the independent
long-double reference of tests/bounded_weno_reference.py, on the grids and states of tests/bounded_weno_cases.py: x, y and z alone (the
other two velocities zero) and all three together, bounds (0, 1) and (0, 0.01).  This pins, beside the periodic x row of
tests/test_bounded_weno.py, the y direction, z with the wall order reduction (buffers 3 / 2 / 1 by distance to the wall), the face
densities and stretched z.

MEASURED  max|oracle - reference| / max|reference|, per grid over both pairs of bounds (x86-64, 80-bit long double):
                x         y         z         all
  ragged    2.0e-14   1.6e-14   5.7e-14   2.1e-14
  fit       1.7e-14   2.8e-16   2.4e-14   1.7e-14
  thin      2.4e-14   2.9e-15   3.4e-15   2.2e-14
  flat      1.5e-14      -      1.5e-14   1.5e-14
TOLERANCE = 6e-13, 10 x the worst of them (5.7e-14: z alone on the stretched ragged grid); no direction needs the 1e-10 of the x-row test.
The expanded smoothness indicators of the oracle against the squared differences here cost these 1e-14 and no more because the rough
state has a cell-to-cell variation of the order of its mean: there is no large mean for the expanded form to cancel.

The activity condition keeps the limiter awake: per direction at least 10 % of the cells have 0 < theta < 1, and each bound is the
binding one in at least 1 % of them.  The defect checks break the reference on purpose (Gauss-Lobatto weight 1/4 for 5/18, theta applied
to all four reconstructions, order 5 at the faces whose buffer is 2) and see the same comparison fail by orders of magnitude."""
import ctypes as C
import functools

import numpy as np
import pytest

import bounded_weno_cases as cases
from bounded_weno_reference import buffer_face, bounded_weno_tendency
from helpers import randomize

TOLERANCE = 6e-13      # 10 x 5.7e-14, the worst measured (module docstring)


def _p(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


@functools.lru_cache(maxsize=None)
def _case(name, bounds, field=0):
    """the oracle model with the planted moisture state, built once per grid and pair of bounds and left unchanged; field = 1, 2, ...:
    the states the device tests give their second, third, ... limited scalar (seed + field)"""
    from oracle import oracle
    oracle.build()
    om = cases.oracle_model(oracle, name)
    randomize(om, seed=cases.SEED)
    cases.plant(om, "q", "rq", *bounds, seed=cases.SEED + 1 + field)
    return om


def _directions(om):
    return ("x", "z", "all") if om.grid.Ny == 1 else ("x", "y", "z", "all")


def _velocities(om, direction):
    keep = {"x": "u", "y": "v", "z": "w", "all": "uvw"}[direction]
    return tuple(getattr(om, n) if n in keep else np.zeros_like(getattr(om, n)) for n in "uvw")


def _oracle(om, uvw, bounds):
    G = np.zeros_like(om.q)
    om.lib.og_scalar_tendency_bounded(C.byref(om.cg), _p(G), *(_p(a) for a in uvw), _p(om.q), C.c_double(bounds[0]), C.c_double(bounds[1]))
    return om.grid.interior(G)


def _reference(om, uvw, bounds, **defect):
    g = om.grid
    return bounded_weno_tendency(om.q, *uvw, om.ref.density, g.zf, g.dx, g.dy, *bounds, halo=(g.Hx, g.Hy, g.Hz), flat_y=(g.Ny == 1), **defect)


def _distance(got, want):
    return float(np.max(np.abs(got - want)) / np.max(np.abs(want)))


@pytest.mark.parametrize("bounds", cases.BOUNDS)
@pytest.mark.parametrize("name", list(cases.GRIDS))
def test_oracle_matches_long_double_reference(name, bounds):
    om = _case(name, bounds)
    errs = {}
    for d in _directions(om):
        uvw = _velocities(om, d)
        want, _ = _reference(om, uvw, bounds)
        assert np.max(np.abs(want)) > 0
        errs[d] = _distance(_oracle(om, uvw, bounds), want)
    print(f"BOUNDED-REF {name} {bounds}:", " ".join(f"{d}={e:.2e}" for d, e in errs.items()))
    assert all(e < TOLERANCE for e in errs.values()), errs
    if om.grid.Ny == 1:      # a Flat y has no faces: v alone moves nothing
        assert not _oracle(om, _velocities(om, "y"), bounds).any() and np.abs(om.v).max() > 0


# moisture on every grid; then the further states of tests/test_bounded_weno_clients.py: species and tracers take fields 0 and 1 on
# "ragged" and "thin", all three masks at once fields 0 .. 4 on "ragged" under the second pair of bounds
ACTIVE = [(n, b, 0) for n in cases.GRIDS for b in cases.BOUNDS] + [(n, b, 1) for n in ("ragged", "thin") for b in cases.BOUNDS] + \
    [("ragged", cases.BOUNDS[1], f) for f in (2, 3, 4)]


@pytest.mark.parametrize("name,bounds,field", ACTIVE)
def test_limiter_is_active_in_every_direction(name, bounds, field):
    om = _case(name, bounds, field)
    _, info = _reference(om, _velocities(om, "all"), bounds)
    assert set(info) == ({"x", "z"} if om.grid.Ny == 1 else {"x", "y", "z"})
    shares = {}
    for d, t in info.items():
        th, up, low = t["theta"], t["upper"], t["lower"]
        shares[d] = (np.mean((th > 0) & (th < 1)), np.mean((up < 1) & (up < low)), np.mean((low < 1) & (low < up)), float(th[th > 0].min()),
                     np.mean(th == 0))
    print(f"BOUNDED-ACTIVITY {name} {bounds}:", " ".join(f"{d}=" + "/".join(f"{s:.3g}" for s in v) for d, v in shares.items()))
    for d, (partial, upper, lower, _, zero) in shares.items():
        assert partial >= 0.10 and upper >= 0.01 and lower >= 0.01, (d, shares[d])
        assert zero > 0, d      # the cells planted at a bound


def test_planted_cells_reach_the_limiter():
    """the run of equal cells makes M - c = 0 somewhere (theta = 1 through the 1e-20), and the two cells outside the bounds are there"""
    om = _case("ragged", cases.BOUNDS[0])
    g = om.grid
    q = g.interior(om.q)
    assert q.min() < 0.0 and q.max() > 1.0
    for axis in (0, 1, 2):
        d = np.diff(q, axis=axis) == 0.0
        run = d.copy()
        for s in range(1, 6):      # six consecutive zero differences = seven equal cells
            run = run[tuple(slice(None, -1) if a == axis else slice(None) for a in range(3))] & \
                d[tuple(slice(s, None) if a == axis else slice(None) for a in range(3))]
        assert run.any(), axis


@pytest.mark.parametrize("defect", ["gauss_lobatto_weight", "theta_on_all_four", "order_5_where_buffer_is_2"])
def test_comparison_fails_against_a_broken_reference(defect):
    name, bounds = "thin", cases.BOUNDS[0]
    om = _case(name, bounds)
    uvw = _velocities(om, "all")
    kw = {"gauss_lobatto_weight": dict(gl_weight=0.25), "theta_on_all_four": dict(limit_all_four=True),
          "order_5_where_buffer_is_2": dict(z_buffer=lambda k, Nz: 3 if buffer_face(k, Nz) == 2 else buffer_face(k, Nz))}[defect]
    broken, _ = _reference(om, uvw, bounds, **kw)
    d = _distance(_oracle(om, uvw, bounds), broken)
    print(f"BOUNDED-DEFECT {defect}: {d:.2e}")
    assert d > 1e4 * TOLERANCE, (defect, d)
