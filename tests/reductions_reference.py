"""Plain numpy restatement, in np.longdouble, of the whole-field reductions behind the C ABI (csrc/bz_state.hip):
bz_max_abs_divergence and bz_cell_advection_timescale.  The functions take parent arrays (halos included, (z, y, x)-shaped, as read
back from the device) and the oracle's `Grid`; they share no code with the oracle's C library nor with the kernels, and the module
imports neither torch nor the oracle."""
import numpy as np

L = np.longdouble
FLAT = 2          # oracle.Grid.topo code of a Flat direction


def _box(g):
    return (g.Hz, g.Hz + g.Nz), (g.Hy, g.Hy + g.Ny), (g.Hx, g.Hx + g.Nx)


def divergence_field(g, ru, rv, rw):
    """(div, S): Vinv_c[k] (Ax[k] (ru[i+1] - ru[i]) + Ay[k] (rv[j+1] - rv[j]) + Az (rw[k+1] - rw[k])) on the interior cells, with the
    metrics of csrc/bz_internal.h (Ax = dy dzc, Ay = dx dzc, Az = dx dy, Vinv_c = 1 / (dx dy dzc)); the y term is dropped on Flat y.
    S = max over cells of |ru|/dx + |rv|/dy + |rw|/dzc, each momentum taken at the larger of the two faces the cell reads: every one of
    the six products Vinv_c A rho u is bounded by S."""
    (k0, k1), (j0, j1), (i0, i1) = _box(g)
    ru, rv, rw = (np.asarray(a).astype(L) for a in (ru, rv, rw))
    dx, dy = L(g.dx), L(g.dy)
    dzc = np.asarray(g.dzc[k0:k1]).astype(L)[:, None, None]
    Ax, Ay, Az, Vinv = dy * dzc, dx * dzc, dx * dy, 1 / (dx * dy * dzc)
    uw, ue = ru[k0:k1, j0:j1, i0:i1], ru[k0:k1, j0:j1, i0 + 1:i1 + 1]
    wb, wt = rw[k0:k1, j0:j1, i0:i1], rw[k0 + 1:k1 + 1, j0:j1, i0:i1]
    div = Ax * (ue - uw) + Az * (wt - wb)
    S = np.maximum(np.abs(uw), np.abs(ue)) / dx + np.maximum(np.abs(wb), np.abs(wt)) / dzc
    if g.topo[1] != FLAT:
        vs, vn = rv[k0:k1, j0:j1, i0:i1], rv[k0:k1, j0 + 1:j1 + 1, i0:i1]
        div = div + Ay * (vn - vs)
        S = S + np.maximum(np.abs(vs), np.abs(vn)) / dy
    return Vinv * div, S.max()


def max_abs_divergence(g, ru, rv, rw):
    """(max |div| over the interior cells, S) of `divergence_field`."""
    div, S = divergence_field(g, ru, rv, rw)
    return np.abs(div).max(), S


def advection_timescale(g, u, v, w, horizontal=False, dz=None):
    """1 / max(|u|/dx + |v|/dy + |w|/dzf[k]) over the interior cells k = 0 .. Nz-1, with dzf[k] the centre spacing at face k (the
    spacing at w's own location); the y term is dropped on Flat y and the z term where `horizontal`.  `dz` (Nz values) stands in for
    dzf[0 .. Nz-1]: the tests use it to show that another metric column would have given another answer."""
    (k0, k1), (j0, j1), (i0, i1) = _box(g)
    box = (slice(k0, k1), slice(j0, j1), slice(i0, i1))
    inv = np.abs(np.asarray(u)[box].astype(L)) / L(g.dx)
    if g.topo[1] != FLAT:
        inv = inv + np.abs(np.asarray(v)[box].astype(L)) / L(g.dy)
    if not horizontal:
        dz = g.dzf[k0:k1] if dz is None else dz
        inv = inv + np.abs(np.asarray(w)[box].astype(L)) / np.asarray(dz).astype(L)[:, None, None]
    m = inv.max()
    return L(np.inf) if m == 0 else 1 / m
