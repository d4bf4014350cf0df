"""Device tendencies G(rho u), G(rho v), G(rho w), G(rho theta), G(rho q) of bz.compute_tendencies_ against THE LONG-DOUBLE REFERENCE of
tests/advection_reference.py (and, as a second printed number, against the C oracle), on the grids and planted states of
tests/advection_cases.py, through every kernel family that computes plain WENO 5 / 7 / 9 tendencies:

  family             kernels                                                               grids                      switch
  k6_stored          k6_u / k6_v / k6_w<stored velocity> + k5_scalar_pair (bz_tendency5)   ragged, cascade, thin      default
  gen4_tiles         k_u / k_v / k_w_tend_lds + k_scalar_pair_lds (bz_tendency4_kernels)    ragged                     BZ_NO_K6_STORED=1
  gen1               k_u / k_v / k_w_tendency + k_scalar_tendency (bz_tendency.hip)         flat, ywalls, xwalls       default (no tiles there)
  generic            orders 7, 9 (bz_tendency_generic.hip): the marching kernel where the  cascade, march, ywalls,    default
                     grid allows it ("march" alone), else flux pass + divergence pass       xwalls
  generic_two_pass   orders 7, 9: flux pass + divergence pass everywhere                    the same four              BZ_NO_GENERIC_MARCH=1
  mixed              momentum of order 9 (generic), scalars of order 5 (k5_scalar_pair),    cascade                    default
                     through compute_tendencies_by_operator of bz_tendency.hip

A context between x walls has a Flat y and therefore no tiled kernels: bz_compute_tendencies takes the generation-1 kernels on "xwalls"
(the generation-4 tiles run there in whole steps only), so "xwalls" stands with "gen1" here.  The switches are read when the context
is created: they are set with monkeypatch.setenv before the model is built.  hm.profile() record names show what they can: the tiled
families record "scalar_tendencies" (theta and moisture in one launch), the generation-1 and generic kernels record
"potential_temperature_tendency" and "moisture_tendency"; the stored-velocity kernels and the generation-4 tiles share their record
names, as do the marching kernel and the two passes: there the environment switch, and the launch conditions spelled out in
tests/advection_cases.py, decide.

States go into the device model bit for bit (helpers.push_state: prognostic fields, velocities, theta, q, T, halos included; the models
are dry without tracers, so there is nothing further to copy).  Every G starts as NaN; afterwards no NaN remains in the cells the
operator writes.  G(rho w) is compared on faces 1 .. Nz - 1, G(rho u) and G(rho v) without the first wall face between x / y walls (the
cells advection_reference.written names).

TOLERANCE against the reference: 1e-12 of max|reference| for order 5, 1e-11 for orders 7 and 9, the project's bounds for a device tendency.
No entry of the CPU table of tests/test_advection_reference.py exceeds 1e-13 / 1e-12 (worst 4.2e-14), so no field takes an exception.

The lean whole-step seam runs the same k6 bodies with derived instead of stored velocities; it is held bit for bit to this operator
sequence by tests/test_multi_step.py and tests/test_dry_shortcut.py and is not tested again here.  Out of scope: the saturation-adjustment
and mixed-phase buoyancy modes, the compressible slow tendencies, Float32, production-length z chunks.

MEASURED on the MI355X, worst max|device - reference| / max|reference| per family (the ADV-DEVICE lines):
                     against the reference                  without G(rho w)                 against the oracle
  k6_stored          3.5e-14  (rw, thin)                    3.4e-16  (rv, cascade)           1.3e-14  (rw, ragged)
  gen4_tiles         2.5e-14  (rw, ragged)                  3.3e-16  (rv, ragged)            1.3e-14  (rw, ragged)
  gen1               3.6e-14  (rw, ywalls)                  4.3e-16  (ru, ywalls)            1.3e-14  (rw, ywalls)
  generic            3.4e-14  (rw, ywalls, order 7)         5.5e-16  (ru, ywalls, order 9)   2.0e-14  (rv, march, order 9)
  generic_two_pass   3.4e-14  (rw, ywalls, order 7)         5.5e-16  (ru, ywalls, order 9)   2.0e-14  (rv, march, order 9)
  mixed              3.1e-14  (rw, cascade)                 3.9e-16  (rv, cascade)           1.3e-14  (rw, cascade)
G(rho w) carries the Float64 rounding of R_d T_r / (R_m T) - 1 in the buoyancy (the oracle's 3e-14 .. 4e-14 of
tests/test_advection_reference.py is the same term); everything else is within a few ulp of the reference, closer to it than the oracle
is at orders 7 and 9.  On "ragged" the stored-velocity kernels and the generation-4 tiles gave the same figures to every printed digit,
and so did the marching kernel and the two passes on "march".  The bounds above are not tightened on the basis of these numbers.
"""
import numpy as np
import pytest

import advection_cases as cases
from helpers import PROG, push_state
from test_advection_reference import FIELDS, KIND, oracle_tendency, reference

pytestmark = pytest.mark.gpu

TOLERANCE = {5: 1e-12, 7: 1e-11, 9: 1e-11}
MOMENTUM_RECORDS = {"x_momentum_tendency", "y_momentum_tendency", "z_momentum_tendency"}
TILED = MOMENTUM_RECORDS | {"scalar_tendencies"}
PER_OPERATOR = MOMENTUM_RECORDS | {"potential_temperature_tendency", "moisture_tendency"}
# family: (environment, orders, grids, the profile records of the launch, records that must be absent)
FAMILIES = {
    "k6_stored": ({}, (5,), ("ragged", "cascade", "thin"), TILED, PER_OPERATOR - MOMENTUM_RECORDS),
    "gen4_tiles": ({"BZ_NO_K6_STORED": "1"}, (5,), ("ragged",), TILED, PER_OPERATOR - MOMENTUM_RECORDS),
    "gen1": ({}, (5,), ("flat", "ywalls", "xwalls"), PER_OPERATOR, {"scalar_tendencies"}),
    "generic": ({}, (7, 9), ("cascade", "march", "ywalls", "xwalls"), PER_OPERATOR, {"scalar_tendencies"}),
    "generic_two_pass": ({"BZ_NO_GENERIC_MARCH": "1"}, (7, 9), ("cascade", "march", "ywalls", "xwalls"), PER_OPERATOR, {"scalar_tendencies"}),
}
RUNS = [(f, n, o) for f, (_, orders, grids, _, _) in FAMILIES.items() for n in grids for o in orders]


def _device_model(bz, name, order, scalar_order=None):
    size, kw = cases.grid_arguments(name, max(order, scalar_order or order))
    kw["topology"] = tuple(getattr(bz, t) for t in kw["topology"])
    grid = bz.RectilinearGrid(size, **kw)
    dynamics = bz.AnelasticDynamics(bz.ReferenceState(grid, potential_temperature=300.0))
    if scalar_order:
        return bz.AtmosphereModel(grid, dynamics=dynamics, momentum_advection=bz.WENO(order=order), scalar_advection=bz.WENO(order=scalar_order))
    return bz.AtmosphereModel(grid, dynamics=dynamics, advection=bz.WENO(order=order))


def _run(bz, label, name, order, scalar_order, present, absent):
    import torch
    om = cases.oracle_case(name, order, scalar_order)
    hm = _device_model(bz, name, order, scalar_order)
    push_state(om, hm, names=("ru", "rv", "rw", "rtheta", "rq", "u", "v", "w", "theta", "q", "T"))
    for k in PROG.values():
        hm.G[k].parent.fill_(float("nan"))
    torch.cuda.synchronize()
    hm.profile_enable()
    hm.profile_reset()
    bz.compute_tendencies_(hm)
    hm.synchronize()
    records = set(hm.profile())
    g = om.grid
    errs, against_oracle = {}, {}
    for field in FIELDS:
        o = scalar_order if (scalar_order and KIND[field] == "c") else order
        want, _ = reference(name, order, field, "all", scalar_order)
        got = g.interior(hm.G[PROG[field]].parent.cpu().numpy())          # rho w: faces 0 .. Nz - 1
        mask = ~np.isnan(want)
        assert not np.isnan(got[mask]).any(), (field, "cells the operator writes still hold NaN", int(np.isnan(got[mask]).sum()))
        scale = np.max(np.abs(want[mask]))
        errs[field] = float(np.max(np.abs(got[mask] - want[mask])) / scale)
        orc = oracle_tendency(om, field, "all", o)
        against_oracle[field] = float(np.max(np.abs(got[mask] - orc[mask])) / scale)
    print(f"ADV-DEVICE {label} {name} order {order}{'/' + str(scalar_order) if scalar_order else ''}: reference",
          " ".join(f"{n}={e:.2e}" for n, e in errs.items()), "| oracle", " ".join(f"{n}={e:.2e}" for n, e in against_oracle.items()),
          "| records", ",".join(sorted(records)))
    assert present <= records and not (absent & records), (sorted(records), sorted(present), sorted(absent))
    tol = {f: TOLERANCE[scalar_order if (scalar_order and KIND[f] == "c") else order] for f in FIELDS}
    assert all(errs[f] < tol[f] for f in FIELDS), (errs, tol)


@pytest.mark.parametrize("family,name,order", RUNS, ids=[f"{f}-{n}-order{o}" for f, n, o in RUNS])
def test_device_tendencies_match_long_double_reference(oracle, bz, family, name, order, monkeypatch):
    env, _, _, present, absent = FAMILIES[family]
    for k in ("BZ_NO_K6_STORED", "BZ_NO_GENERIC_MARCH"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    _run(bz, family, name, order, None, present, absent)


def test_momentum_of_order_nine_with_scalars_of_order_five(oracle, bz, monkeypatch):
    """compute_tendencies_by_operator: the generic momentum kernels of order 9 (1e-11), then theta and moisture of order 5 through the
    tiled pair kernel (1e-12), on "cascade" with the halos of order 9"""
    for k in ("BZ_NO_K6_STORED", "BZ_NO_GENERIC_MARCH"):
        monkeypatch.delenv(k, raising=False)
    _run(bz, "mixed", "cascade", 9, 5, TILED, PER_OPERATOR - MOMENTUM_RECORDS)
