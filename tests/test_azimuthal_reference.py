"""tests/azimuthal_reference.py (the numpy restatement of the reference's azimuthal_mean) against the reference's own test
(test/diagnostics.jl:269-319: 64 × 64 × 4 grid, x, y ∈ (−1, 1)) and its doctest value (tests/golden/azimuthal_mean.json), and the
host-side argument checks of bz.azimuthal_mean / bz.TangentialVelocity / bz.RadialVelocity, which run before any device call."""
import json
import os

import numpy as np
import pytest

import azimuthal_reference as ar

F64, F32 = np.float64, np.float32
N, NZ = 64, 4


def _nodes(n, lo, hi):
    d = (hi - lo) / n
    return lo + d * (np.arange(n) + 0.5), d


XC, DX = _nodes(N, -1.0, 1.0)
YC, DY = _nodes(N, -1.0, 1.0)


def _field(fn):
    return np.broadcast_to(fn(XC[None, None, :], YC[None, :, None]), (NZ, N, N)).astype(F64)


def _mean(field, dtype=F64, **kw):
    return ar.azimuthal_mean(field.astype(dtype), XC, YC, DX, DY, dtype=dtype, **kw)


FIVE = _field(lambda x, y: 5.0 + 0 * x + 0 * y)


@pytest.mark.parametrize("dtype", [F64, F32])
def test_constant_field_gives_the_constant_the_doctest_value(dtype):
    with open(os.path.join(os.path.dirname(__file__), "golden", "azimuthal_mean.json"), encoding="utf-8") as f:
        gd = json.load(f)["doctest"]
    assert gd["grid"]["size"] == [N, N, NZ] and gd["field"] == 5
    r = _mean(FIVE, dtype, radius=gd["radius"], Nr=gd["Nr"])
    assert r.mean.shape == (NZ, 8)
    assert np.nanmax(r.mean) == gd["maximum"]
    assert np.all(r.counts > 0) and np.all(r.mean == 5)


@pytest.mark.parametrize("dtype", [F64, F32])
def test_radius_field_gives_a_sorted_profile(dtype):
    r = _mean(_field(lambda x, y: np.sqrt(x ** 2 + y ** 2)), dtype, radius=1, Nr=8)
    p = r.mean[0].astype(F64)
    assert np.all(np.diff(p) > 0) and np.all((0 < p) & (p < 1))
    assert np.array_equal(r.mean, np.broadcast_to(r.mean[:1], r.mean.shape))
    xc, yc = 0.3, -0.2
    r = _mean(_field(lambda x, y: np.sqrt((x - xc) ** 2 + (y - yc) ** 2)), dtype, radius=0.5, Nr=8, center=(xc, yc))
    p = r.mean[0].astype(F64)
    assert np.all(np.diff(p) > 0) and np.all((0 < p) & (p < 1))


def test_subcell_sampling_fills_the_rings_centres_alone_leave_empty():
    coarse = _mean(FIVE, radius=1, Nr=64, m=1)
    filled = _mean(FIVE, radius=1, Nr=64)
    assert np.isnan(coarse.mean).any() and not np.isnan(filled.mean).any()
    assert np.array_equal(np.isnan(coarse.mean), np.broadcast_to(coarse.counts == 0, coarse.mean.shape))
    assert np.all(np.isnan(coarse.mean) | (coarse.mean == 5)) and np.all(filled.mean == 5)
    assert (coarse.counts == 0).sum() == 3          # the figure of the issue's case table


def test_rings_finer_than_the_subcells_stay_nan():
    fine = _mean(FIVE, radius=1, Nr=200)
    assert np.isnan(fine.mean).any() and np.all(np.isnan(fine.mean) | (fine.mean == 5))
    assert (fine.counts == 0).sum() == 1


@pytest.mark.parametrize("kw", [dict(radius=1, Nr=8), dict(radius=1, Nr=64, m=1), dict(radius=0.5, Nr=8, center=(0.3, -0.2)),
                                dict(radius=1, Nr=200), dict(radius=0.9, Nr=5, m=3, center=(2.0, 0.1))])
def test_every_sample_is_in_one_ring_or_dropped(kw):
    r = _mean(FIVE, **kw)
    m = kw.get("m", 4)
    assert r.counts.sum() + r.dropped == N * N * m * m
    assert r.dropped > 0          # the corners of the square lie past every radius used here


def test_margin_is_the_distance_from_a_ring_edge():
    q = np.array([0.0, 0.25, 2.9, 3.0625, 8.5, 11.0])
    assert ar.edge_margin(q, 8) == 0.0625          # 0 is no edge; past the radius only the edge Nr counts
    assert ar.edge_margin(np.array([0.0, 0.5]), 8) == 0.5


def test_polar_restatement_on_a_solid_body_rotation():
    xf, yf = XC - DX / 2, YC - DY / 2
    Ω = 0.7
    u = np.broadcast_to((-Ω * YC)[None, :, None] + 0 * xf[None, None, :], (1, N, N))
    v = np.broadcast_to((Ω * XC)[None, None, :] + 0 * yf[None, :, None], (1, N, N))
    vt, vr, scale = ar.polar_winds(u, v, XC, YC, center=(0.0, 0.0))
    r = np.sqrt(XC[None, None, :] ** 2 + YC[None, :, None] ** 2)
    assert np.max(np.abs(vt - Ω * r)) <= 8 * np.finfo(F64).eps * scale.max() and np.max(np.abs(vr)) <= 8 * np.finfo(F64).eps * scale.max()


# ---- host-side argument errors: no device call is reached, so no GPU is needed -----------------------------------------------------
class _Grid:
    def __init__(self, topology):
        self.topology = topology


class _Model:
    def __init__(self, topology=("Periodic", "Periodic", "Bounded")):
        self.grid = _Grid(topology)


@pytest.mark.parametrize("kw", [dict(radius=1.0, Nr=0), dict(radius=1.0, Nr=-3), dict(radius=1.0, Nr=8, m=0), dict(radius=1.0, Nr=1025), dict(radius=1.0, Nr=8, m=17),
                                dict(radius=0.0, Nr=8),
                                dict(radius=-2.0, Nr=8), dict(radius=float("nan"), Nr=8)])
def test_bad_arguments_raise_value_errors_on_the_host(bz, kw):
    with pytest.raises(ValueError):
        bz.azimuthal_mean(object(), model=_Model(), **kw)


def test_a_field_without_a_model_is_refused(bz):
    with pytest.raises(ValueError):
        bz.azimuthal_mean(object(), radius=1.0, Nr=8)


def test_flat_y_grids_are_refused_on_the_host(bz):
    flat = _Model(("Periodic", "Flat", "Bounded"))
    with pytest.raises(NotImplementedError):
        bz.azimuthal_mean(object(), radius=1.0, Nr=8, model=flat)
    for op in (bz.TangentialVelocity, bz.RadialVelocity):
        with pytest.raises(NotImplementedError):
            op(flat)


def test_slab_models_are_refused_on_the_host(bz):
    from breeze_jl_amd.compressible import SlabCompressibleModel
    from breeze_jl_amd.distributed import LibrarySlabAtmosphereModel, SlabAtmosphereModel
    for cls in (LibrarySlabAtmosphereModel, SlabAtmosphereModel, SlabCompressibleModel):
        slab = object.__new__(cls)          # no context is made: the refusal comes first
        slab.grid = _Grid(("Periodic", "Periodic", "Bounded"))
        with pytest.raises(NotImplementedError):
            bz.azimuthal_mean(object(), radius=1.0, Nr=8, model=slab)
        with pytest.raises(NotImplementedError):
            bz.TangentialVelocity(slab, center=(0.3, -0.2))
        slab.__dict__.clear()


def test_exports(bz):
    for name in ("azimuthal_mean", "AzimuthalMean", "TangentialVelocity", "RadialVelocity"):
        assert hasattr(bz, name)
    assert {"bz_azimuthal_mean", "bz_polar_winds", "bz_set_horizontal_nodes"} <= set(bz.SYMBOLS)
