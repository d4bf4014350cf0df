"""CPU: the numpy reference of the whole-field reductions (tests/reductions_reference.py) says what the oracle's C code says about the
divergence, without sharing a line with it, and tells the metric columns of a stretched grid apart.  tests/test_reductions.py holds the
device kernels to this reference."""
import numpy as np
import pytest

import reductions_reference as rr

EPS = np.finfo(np.float64).eps
EXT = dict(x=(-10e3, 10e3), y=(-10e3, 10e3))
STRETCHED = 1e4 * np.linspace(0, 1, 25) ** 1.3          # the faces of test_tendencies_stretched_grid


def _grid(oracle, kind):
    if kind == "uniform":
        return oracle.Grid((20, 9, 12), z=(0.0, 10e3), **EXT)
    if kind == "stretched":
        return oracle.Grid((32, 12, 24), z=STRETCHED, **EXT)
    return oracle.Grid((40, 12), x=EXT["x"], z=(0.0, 10e3), topology=("Periodic", "Flat", "Bounded"))


@pytest.mark.parametrize("kind", ["uniform", "stretched", "flat_y"])
def test_divergence_reference_agrees_with_the_oracle(oracle, kind):
    """random parent arrays, halos included: every cell of the reference within 16 eps S of og_divergence (six products and five sums
    of terms bounded by S, each rounded once in the C code; the longdouble reference adds nothing at this scale)"""
    g = _grid(oracle, kind)
    om = oracle.OracleModel(g, potential_temperature=300.0)
    rng = np.random.default_rng(3)
    for f in (om.ru, om.rv, om.rw):
        f[...] = 5.0 * rng.standard_normal(f.shape)
    want = om.divergence()
    got, S = rr.divergence_field(g, om.ru, om.rv, om.rw)
    top, S2 = rr.max_abs_divergence(g, om.ru, om.rv, om.rw)
    assert S2 == S and top == np.abs(got).max()
    ratio = float(np.abs(got - want).max() / (EPS * S))
    print(f"REDREF divergence {kind}: max |ref - oracle| / (eps S) = {ratio:.3f}, max |div| / S = {float(top / S):.3f}")
    assert top > 0.1 * S                  # the field is not nearly solenoidal: the comparison is of numbers of order S
    assert ratio <= 16.0
    if kind == "flat_y":                  # the y term is dropped, whatever rho v holds
        om.rv[...] = 1e6
        assert rr.max_abs_divergence(g, om.ru, om.rv, om.rw)[0] == top


def test_timescale_reference_tells_the_metric_columns_apart(oracle):
    """the stretched grid of the device test: with the extremum planted in w at k = 1 and at k = Nz - 1, reading dzc[k], dzf[k - 1] or
    dzf[k + 1] for dzf[k] moves the answer by more than 1e-3 relative — a bound of 8 eps in tests/test_reductions.py tells them apart"""
    g = _grid(oracle, "stretched")
    Hz, Nz = g.Hz, g.Nz
    rng = np.random.default_rng(4)
    u, v, w = (rng.standard_normal(s) for s in ((g.Szc, g.Sy, g.Sx), (g.Szc, g.Sy, g.Sx), (g.Szf, g.Sy, g.Sx)))
    wrong = {"dzc[k]": g.dzc[Hz:Hz + Nz], "dzf[k-1]": g.dzf[Hz - 1:Hz + Nz - 1], "dzf[k+1]": g.dzf[Hz + 1:Hz + Nz + 1]}
    margin = np.inf
    for k in (1, Nz - 1):
        w2 = w.copy()
        w2[Hz + k, g.Hy + 5, g.Hx + 7] = 1e3
        right = rr.advection_timescale(g, u, v, w2)
        assert abs(right * 1e3 / g.dzf[Hz + k] - 1) < 0.1           # the planted face sets the answer
        for name, dz in wrong.items():
            d = float(abs(rr.advection_timescale(g, u, v, w2, dz=dz) - right) / right)
            print(f"REDREF timescale plant at k={k}: {name} for dzf[k] moves the answer by {d:.3e}")
            margin = min(margin, d)
    print(f"REDREF timescale: smallest dzf / dzc distinguishability margin {margin:.3e}")
    assert margin > 1e-3


def test_timescale_reference_basics(oracle):
    g = _grid(oracle, "uniform")
    z = np.zeros((g.Szc, g.Sy, g.Sx))
    zw = np.zeros((g.Szf, g.Sy, g.Sx))
    assert rr.advection_timescale(g, z, z, zw) == np.inf
    u = z.copy()
    u[g.Hz + 2, g.Hy + 3, g.Hx + 4] = -4.0
    zw[g.Hz + g.Nz, g.Hy, g.Hx] = 1e9          # the top face is not a cell's: k = 0 .. Nz - 1
    u[0, 0, 0] = 1e9                           # nor is a halo
    assert float(rr.advection_timescale(g, u, z, zw)) == pytest.approx(g.dx / 4.0, rel=1e-15)
    zw[g.Hz + 1, g.Hy, g.Hx] = 2.0
    assert float(rr.advection_timescale(g, u, z, zw)) == pytest.approx(g.dx / 4.0, rel=1e-15)      # another cell: the maximum is per cell
    assert float(rr.advection_timescale(g, u, z, zw, horizontal=True)) == pytest.approx(g.dx / 4.0, rel=1e-15)
    zw[g.Hz + 2, g.Hy + 3, g.Hx + 4] = 2.0
    assert float(rr.advection_timescale(g, u, z, zw)) == pytest.approx(1 / (4.0 / g.dx + 2.0 / g.dzf[g.Hz + 2]), rel=1e-15)
