"""numpy restatement of the reference's azimuthal_mean (src/AtmosphereModels/Diagnostics/azimuthal_mean.jl:54-92) and of the polar wind
components of examples/tropical_cyclone_with_rainband.jl.  Not a test: tests/test_azimuthal_reference.py pins it to the reference's own
test, tests/test_azimuthal.py holds the device kernels (csrc/bz_azimuthal.hip) to it.

For Nr uniform rings on [0, radius], Δr = radius / Nr, every cell (ii, jj) is split into m × m sub-cell centres
    x = (xᶜ[ii] − xc) + (2si − m − 1)·Δx / (2m),  y likewise        (product, then quotient, then sum)
and a sample is in ring ir iff trunc(sqrt(x·x + y·y) / Δr) + 1 == ir.  Coordinates and the ring index are computed in `dtype`, every
operation rounded once, in that order (numpy never contracts); the sums are taken in np.longdouble.
"""
from types import SimpleNamespace

import numpy as np

L = np.longdouble


def ring_index(xc, yc, dx, dy, radius, Nr, center=(0, 0), m=4, dtype=np.float64):
    """(b, q): ring (0-based, −1 past the radius) and r/Δr of every sample, arrays of shape (Ny, Nx, m, m) indexed [jj, ii, sj, si]."""
    T = np.dtype(dtype).type
    xc, yc = np.asarray(xc).astype(T), np.asarray(yc).astype(T)
    dr = T(radius) / T(Nr)
    s = np.arange(1, m + 1)
    off = (2 * s - m - 1).astype(T)
    X = (xc - T(center[0]))[:, None] + off[None, :] * T(dx) / T(2 * m)          # (Nx, m)
    Y = (yc - T(center[1]))[:, None] + off[None, :] * T(dy) / T(2 * m)          # (Ny, m)
    X, Y = X[None, :, None, :], Y[:, None, :, None]
    q = np.sqrt(X * X + Y * Y) / dr
    assert q.dtype == np.dtype(dtype)
    inside = q < T(Nr)
    b = np.where(inside, np.trunc(np.where(inside, q, 0)).astype(np.int64), -1)
    return b, q


def edge_margin(q, Nr):
    """smallest distance of any sample's r/Δr from a ring edge 1 .. Nr (0 is no edge: nothing lies below it)"""
    q = q.astype(np.float64)
    return float(np.min(np.abs(q - np.clip(np.rint(q), 1, Nr))))


def azimuthal_mean(field, xc, yc, dx, dy, radius, Nr, center=(0, 0), m=4, dtype=np.float64, accumulate=L):
    """field: (nlev, Ny, Nx) interior values.  Returns .mean (nlev, Nr; NaN in empty rings), .counts (Nr), .dropped (samples past the
    radius), .margin (edge_margin), .abs_sum (nlev, Nr: Σ|f_s| over the ring's samples, for error bounds)."""
    field = np.asarray(field)
    nlev, Ny, Nx = field.shape
    b, q = ring_index(xc, yc, dx, dy, radius, Nr, center, m, dtype)
    counts = np.bincount(b[b >= 0], minlength=Nr).astype(np.int64)
    # n(cell, ring) through a flat (cell, ring) histogram, then Σ f·n per ring
    cell = np.broadcast_to(np.arange(Ny * Nx).reshape(Ny, Nx, 1, 1), b.shape)
    ok = b >= 0
    pair, n = np.unique(cell[ok] * Nr + b[ok], return_counts=True)
    pc, pr = pair // Nr, pair % Nr
    sums = np.zeros((nlev, Nr), accumulate)
    abs_sum = np.zeros((nlev, Nr), accumulate)
    for k in range(nlev):
        v = field[k].reshape(-1)[pc].astype(accumulate) * n
        np.add.at(sums[k], pr, v)
        np.add.at(abs_sum[k], pr, np.abs(v))
    with np.errstate(all="ignore"):
        mean = np.where(counts > 0, sums / np.maximum(counts, 1), np.nan)
    return SimpleNamespace(mean=mean, counts=counts, dropped=int((~ok).sum()), margin=edge_margin(q, Nr), abs_sum=abs_sum)


def polar_winds(u, v, xc, yc, center=(0, 0), dtype=np.float64):
    """u, v: interiors (Nz, Ny, Nx) of the face velocities on a doubly periodic grid (face Nx + 1 is face 1).  Returns (vθ, vʳ, |uᶜ| + |vᶜ|)
    at cell centres: uᶜ = (u[i] + u[i+1])/2, vθ = (−y·uᶜ + x·vᶜ)/r, vʳ = (x·uᶜ + y·vᶜ)/r."""
    T = np.dtype(dtype).type
    u, v = np.asarray(u).astype(T), np.asarray(v).astype(T)
    uc = (u + np.roll(u, -1, axis=2)) / T(2)
    vc = (v + np.roll(v, -1, axis=1)) / T(2)
    x = (np.asarray(xc).astype(T) - T(center[0]))[None, None, :]
    y = (np.asarray(yc).astype(T) - T(center[1]))[None, :, None]
    r = np.sqrt(x * x + y * y)
    with np.errstate(all="ignore"):
        return (-y * uc + x * vc) / r, (x * uc + y * vc) / r, np.abs(uc) + np.abs(vc)
