"""A literal numpy restatement of bz_horizontal_moments (include/breeze_hip.h): Average(expression, dims=(1, 2)) of products, powers and
∂z of staggered fields, on halo-inclusive parent arrays shaped (z, y, x).

    location   L of a moment = location of its first factor; with dz the z location is flipped; a Flat y has no y location
    value      f0^p0 · ℑ_L(f1^p1) · ℑ_L(f2^p2), left to right; power (repeated multiplication) before interpolation; ℑ_L the two-point
               mean (a + b) / 2 per differing direction, x outermost, z innermost; centre -> face i: centres i − 1, i; face -> centre i:
               faces i, i + 1
    dz         centre -> face k: (f[k] − f[k−1]) / Δzᵃᵃᶠ[k]; face -> centre k: (f[k+1] − f[k]) / Δzᵃᵃᶜ[k]
    at_center  the values at L interpolated to (Center, Center, Center) with the same ℑ
    profile    Σ over the Nx × Ny interior points of a level / (Nx Ny)

Two additions for the tests: `precise=True` evaluates in np.longdouble (float64 for Float32 inputs), and `majorant=True` returns the
absolute majorant A_k — every factor replaced by its absolute value, ∂z's difference by (|a| + |b|) / Δz — which bounds, times eps, what
one rounding can move.  Only the cells the semantics name are indexed: a NaN anywhere else in the parent arrays cannot reach a result."""
from collections import namedtuple

import numpy as np

L = np.longdouble
Geometry = namedtuple("Geometry", "Nx Ny Nz Hx Hy Hz flat_y dzc dzf")          # dzc: Nz spacings at centres; dzf: Nz + 1 at faces
Moment = namedtuple("Moment", "factors dz at_center", defaults=(False, False))  # factors: ((field index, power), ...)


def spacings(zf):
    """Δzᵃᵃᶜ (Nz) and Δzᵃᵃᶠ (Nz + 1) of the faces zf, the first and last cell mirrored outward for the boundary faces"""
    zf = np.asarray(zf, dtype=np.float64)
    dzc = np.diff(zf)
    zc = np.concatenate([[zf[0] - dzc[0] / 2], (zf[:-1] + zf[1:]) / 2, [zf[-1] + dzc[-1] / 2]])
    return dzc, np.diff(zc)


def geometry(grid):
    """Geometry of a RectilinearGrid of the package (regular z: the one Δz everywhere)"""
    if grid.regular_z:
        dzc, dzf = np.full(grid.Nz, grid.Δz), np.full(grid.Nz + 1, grid.Δz)
    else:
        dzc, dzf = spacings(grid.zᶠ)
    return Geometry(grid.Nx, grid.Ny, grid.Nz, grid.Hx, grid.Hy, grid.Hz, grid.topology[1] == "Flat", dzc, dzf)


def parent_shape(geo, loc):
    return (geo.Nz + 2 * geo.Hz + (1 if loc[2] else 0), geo.Ny + 2 * geo.Hy, geo.Nx + 2 * geo.Hx)


def fill_parent(geo, loc, interior, z_halo=0.0, far=np.nan):
    """Parent array of a field at `loc` ((face_x, face_y, face_z) as 0 / 1) from its interior (nlev, Ny, Nx): periodic images in x and y,
    `z_halo` (a number or a function of the shape) in the first z halo level on either side, `far` in every cell two or more cells from
    the interior."""
    interior = np.asarray(interior)
    nlev = geo.Nz + (1 if loc[2] else 0)
    assert interior.shape == (nlev, geo.Ny, geo.Nx), (interior.shape, (nlev, geo.Ny, geo.Nx))
    P = np.full(parent_shape(geo, loc), far, dtype=interior.dtype)
    Hx, Hy, Hz = geo.Hx, geo.Hy, geo.Hz
    ring = np.pad(interior, ((0, 0), (0 if geo.flat_y else 1,) * 2, (1, 1)), mode="wrap")          # one periodic cell around every level
    ey = 0 if geo.flat_y else 1
    P[Hz:Hz + nlev, Hy - ey:Hy + geo.Ny + ey, Hx - 1:Hx + geo.Nx + 1] = ring
    for k in (Hz - 1, Hz + nlev):
        shape = (geo.Ny + 2 * ey, geo.Nx + 2)
        P[k, Hy - ey:Hy + geo.Ny + ey, Hx - 1:Hx + geo.Nx + 1] = z_halo(shape) if callable(z_halo) else z_halo
    return P


def _location(geo, loc):
    return (int(loc[0]), 0 if geo.flat_y else int(loc[1]), int(loc[2]))


def _offsets(G, Lc):
    """cells a value at location Lc takes from a field at G, per direction"""
    return [(0,) if g == l else ((-1, 0) if l else (0, 1)) for g, l in zip(G, Lc)]


def _mean(parts):
    return parts[0] if len(parts) == 1 else (parts[0] + parts[1]) / 2


def _box(geo, P, box, shift):
    """P at the points (i + sx, j + sy, k + sz) for (i, j, k) in box = ((i0, i1), (j0, j1), (k0, k1))"""
    (i0, i1), (j0, j1), (k0, k1) = box
    sx, sy, sz = shift
    return P[geo.Hz + k0 + sz:geo.Hz + k1 + sz, geo.Hy + j0 + sy:geo.Hy + j1 + sy, geo.Hx + i0 + sx:geo.Hx + i1 + sx]


def _power(v, p):
    r = v
    for _ in range(p - 1):
        r = r * v
    return r


def _factor(geo, P, p, G, Lc, box, majorant):
    ox, oy, oz = _offsets(G, Lc)

    def cell(s):
        v = _box(geo, P, box, s)
        return _power(np.abs(v) if majorant else v, p)
    return _mean([_mean([_mean([cell((ax, ay, az)) for az in oz]) for ay in oy]) for ax in ox])


def _values(geo, fields, m, Lc, box, majorant):
    """the moment at the points of L in `box`"""
    P0, loc0 = fields[m.factors[0][0]]
    if m.dz:
        assert len(m.factors) == 1 and m.factors[0][1] == 1
        (k0, k1) = box[2]
        if Lc[2]:      # centre -> face
            a, b, dz = _box(geo, P0, box, (0, 0, 0)), _box(geo, P0, box, (0, 0, -1)), geo.dzf[k0:k1]
        else:          # face -> centre
            a, b, dz = _box(geo, P0, box, (0, 0, 1)), _box(geo, P0, box, (0, 0, 0)), geo.dzc[k0:k1]
        dz = np.asarray(dz).astype(a.dtype)[:, None, None]
        return (np.abs(a) + np.abs(b)) / dz if majorant else (a - b) / dz
    v = None
    for f, p in m.factors:
        P, loc = fields[f]
        t = _factor(geo, P, p, _location(geo, loc), Lc, box, majorant)
        v = t if v is None else v * t
    return v


def moment_location(geo, fields, m):
    Lc = list(_location(geo, fields[m.factors[0][0]][1]))
    if m.dz:
        Lc[2] = 1 - Lc[2]
    return tuple(Lc)


def profile(geo, fields, m, precise=False, majorant=False):
    """The profile of Moment m over `fields` [(parent array, (face_x, face_y, face_z)), ...]: nlev values."""
    m = Moment(*m)
    real = fields[m.factors[0][0]][0].dtype
    work = np.dtype((np.float64 if real == np.float32 else L) if precise else real).type
    fields = [(P.astype(work), loc) for P, loc in fields]
    Lc = moment_location(geo, fields, m)
    c = Lc if m.at_center else (0, 0, 0)          # directions in which the values at L are brought to the centre
    nlev = geo.Nz + (1 if (Lc[2] and not m.at_center) else 0)
    box = ((0, geo.Nx + c[0]), (0, geo.Ny + c[1]), (0, nlev + c[2]))
    V = _values(geo, fields, m, Lc, box, majorant)

    def part(sx, sy, sz):
        return V[sz:sz + nlev, sy:sy + geo.Ny, sx:sx + geo.Nx]
    X = _mean([_mean([_mean([part(ax, ay, az) for az in range(c[2] + 1)]) for ay in range(c[1] + 1)]) for ax in range(c[0] + 1)])
    assert X.shape == (nlev, geo.Ny, geo.Nx) and X.dtype == work
    return X.sum(axis=(1, 2)) / work(geo.Nx * geo.Ny)
