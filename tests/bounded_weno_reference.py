"""Independent reference of the bounds-preserving WENO-5 scalar tendency, plain numpy in np.longdouble.

    G = -V^-1 (delta_x + delta_y + delta_z)        on (Periodic, Periodic, Bounded) and (Periodic, Flat, Bounded)

Written from the header comment of csrc/bz_bounded.hip and from csrc/bz_weno.h (bz_upB, bz_buffer_face); it shares no code with oracle/ or
with tests/test_bounded_weno.py::_numpy_bounded_div_x.  Every array is halo-inclusive and already halo-filled, laid out (z, y, x); the
result covers the interior.  Per direction and cell, in this order:

  1. four reconstructions: the left- and right-biased values at the cell's upper face (c+L, c+R) and at its lower face (c-L, c-R);
  2. the Gauss-Lobatto interior point  p = (c - w1 c-R - w1 c+L) / (1 - 2 w1),  w1 = 5/18;
  3. theta = min(|(hi - c) / (M - c + 1e-20)|, |(lo - c) / (m - c + 1e-20)|, 1),  M, m = max, min(p, c+L, c-R);
  4. only the two reconstructions that start in the cell move:  c+L <- theta (c+L - c) + c,  c-R likewise;
  5. divergence = ubp(F_hi, c+L, c+R) - ubp(F_lo, c-L, c-R),  ubp(F, l, r) = ((F + |F|) l + (F - |F|) r) / 2   (upwind_biased_product).

Reconstructions: WENO-Z, eps = 1e-8.  Order 5 carries the x3 scaling of the smoothness indicators, in squared-difference form over the
first differences D1..D4 of the five cells (bz_weno.h):  beta_2 = 13/4 (D2-D1)^2 + 3/4 (3 D2 - D1)^2,  beta_1 = 13/4 (D3-D2)^2 +
3/4 (D2+D3)^2,  beta_0 = 13/4 (D4-D3)^2 + 3/4 (D4 - 3 D3)^2,  tau = |beta_0 - beta_2|,  alpha_s = C_s (1 + (tau / (beta_s + eps))^2),
C = (3/10, 3/5, 1/10), candidates c + delta_s with delta_0 = 2/3 D3 - 1/6 D4, delta_1 = 1/3 D3 + 1/6 D2, delta_2 = 5/6 D2 - 1/3 D1.
Order 3 (buffer 2): beta_0 = (c-b)^2, beta_1 = (b-a)^2 (unscaled), C = (2/3, 1/3), candidates (b+c)/2 and (3b-a)/2.  Buffer 1: the
upwind cell.  x and y are periodic and always order 5; in z face k takes the buffer bz_buffer_face(k, Nz): 3 where 3 <= k <= Nz-3, 2
where 2 <= k <= Nz-2, else 1.

Face mass fluxes: rho_k Ax_k u, rho_k Ay_k v, 1/2 (rho_{k-1} + rho_k) Az w with Ax = dy dz_k, Ay = dx dz_k, Az = dx dy, V = dx dy dz_k,
dz_k = zf[k+1] - zf[k].

The keyword arguments gl_weight, limit_all_four and z_buffer exist so that a test can break this reference on purpose and see its
comparison fail (tests/test_bounded_weno_reference.py)."""
import numpy as np

LD = np.longdouble
EPS = LD("1e-8")
EPS_THETA = LD("1e-20")


def buffer_face(k, Nz):
    if 3 <= k <= Nz - 3:
        return 3
    if 2 <= k <= Nz - 2:
        return 2
    return 1


def weno5(a, b, c, d, e):
    """cells a..e, upwind cell c: the value at the face between c and d"""
    D1, D2, D3, D4 = b - a, c - b, d - c, e - d
    q134, q34 = LD(13) / 4, LD(3) / 4
    beta2 = q134 * (D2 - D1) ** 2 + q34 * (3 * D2 - D1) ** 2
    beta1 = q134 * (D3 - D2) ** 2 + q34 * (D2 + D3) ** 2
    beta0 = q134 * (D4 - D3) ** 2 + q34 * (D4 - 3 * D3) ** 2
    tau = np.abs(beta0 - beta2)
    alpha0 = LD(3) / 10 * (1 + (tau / (beta0 + EPS)) ** 2)
    alpha1 = LD(3) / 5 * (1 + (tau / (beta1 + EPS)) ** 2)
    alpha2 = LD(1) / 10 * (1 + (tau / (beta2 + EPS)) ** 2)
    delta0 = LD(2) / 3 * D3 - D4 / 6
    delta1 = D3 / 3 + D2 / 6
    delta2 = LD(5) / 6 * D2 - D1 / 3
    return c + (alpha0 * delta0 + alpha1 * delta1 + alpha2 * delta2) / (alpha0 + alpha1 + alpha2)


def weno3(a, b, c):
    """cells a, b, c, upwind cell b: the value at the face between b and c"""
    beta0, beta1 = (c - b) ** 2, (b - a) ** 2
    tau = np.abs(beta0 - beta1)
    alpha0 = LD(2) / 3 * (1 + (tau / (beta0 + EPS)) ** 2)
    alpha1 = LD(1) / 3 * (1 + (tau / (beta1 + EPS)) ** 2)
    return (alpha0 * (b + c) / 2 + alpha1 * (3 * b - a) / 2) / (alpha0 + alpha1)


def _face_pair(at, f, B):
    """(left-biased, right-biased) value at the face between the cells at offsets f - 1 and f of the cell, with buffer B"""
    if B == 3:
        return weno5(at(f - 3), at(f - 2), at(f - 1), at(f), at(f + 1)), weno5(at(f + 2), at(f + 1), at(f), at(f - 1), at(f - 2))
    if B == 2:
        return weno3(at(f - 2), at(f - 1), at(f)), weno3(at(f + 1), at(f), at(f - 1))
    return at(f - 1), at(f)


def _direction(at, F_lo, F_hi, lo, hi, B_lo, B_hi, gl_weight, limit_all_four):
    """The divergence of one direction.  at(s): the cell values at offset s along it (interior shape); F_lo, F_hi: the mass fluxes through
    the cell's lower and upper face; B_lo, B_hi: None (order 5 everywhere) or integer arrays, broadcastable, of the two faces' buffers."""
    c = at(0)

    def faces(f, B):
        if B is None:
            return _face_pair(at, f, 3)
        pairs = {b: _face_pair(at, f, b) for b in (1, 2, 3)}
        return tuple(np.where(B == 3, pairs[3][s], np.where(B == 2, pairs[2][s], pairs[1][s])) for s in (0, 1))

    cpL, cpR = faces(1, B_hi)
    cmL, cmR = faces(0, B_lo)
    w1 = gl_weight
    p = (c - w1 * cmR - w1 * cpL) / (1 - 2 * w1)
    M = np.maximum(p, np.maximum(cpL, cmR))
    m = np.minimum(p, np.minimum(cpL, cmR))
    upper = np.abs((hi - c) / (M - c + EPS_THETA))
    lower = np.abs((lo - c) / (m - c + EPS_THETA))
    theta = np.minimum(np.minimum(upper, lower), 1)
    cpL = theta * (cpL - c) + c
    cmR = theta * (cmR - c) + c
    if limit_all_four:
        cpR = theta * (cpR - c) + c
        cmL = theta * (cmL - c) + c
    ubp = lambda F, left, right: ((F + np.abs(F)) * left + (F - np.abs(F)) * right) / 2
    return ubp(F_hi, cpL, cpR) - ubp(F_lo, cmL, cmR), {"theta": theta, "upper": upper, "lower": lower}


def bounded_weno_tendency(c, u, v, w, rho, zf, dx, dy, lo, hi, halo, flat_y=False, gl_weight=LD(5) / 18, limit_all_four=False,
                          z_buffer=buffer_face):
    """c, u, v: (Nz + 2 Hz, Ny + 2 Hy, Nx + 2 Hx) cell values and x- / y-face velocities (face i is the left face of cell i); w: one more
    level, z-face velocity (face k below cell k); rho: the reference density at the Nz + 2 Hz centres; zf: the Nz + 1 z faces;
    halo = (Hx, Hy, Hz), Hy = 0 with flat_y (Ny = 1, dy = 1, no y term).
    Returns (G over the interior, {"x" | "y" | "z": {"theta", "upper", "lower"}}); "upper" and "lower" are the two ratios theta is the
    minimum of, so upper < min(lower, 1) marks the cells whose upper bound binds."""
    c, u, v, w, rho, zf = (np.asarray(a, dtype=LD) for a in (c, u, v, w, rho, zf))
    dx, dy, lo, hi, w1 = LD(dx), LD(1 if flat_y else dy), LD(lo), LD(hi), LD(gl_weight)
    Hx, Hy, Hz = halo
    Nz, Ny, Nx = c.shape[0] - 2 * Hz, c.shape[1] - 2 * Hy, c.shape[2] - 2 * Hx
    assert zf.shape == (Nz + 1,) and rho.shape == (Nz + 2 * Hz,) and w.shape[0] == Nz + 1 + 2 * Hz

    def view(a, sz=0, sy=0, sx=0):
        return a[Hz + sz:Hz + sz + Nz, Hy + sy:Hy + sy + Ny, Hx + sx:Hx + sx + Nx]

    dz = (zf[1:] - zf[:-1])[:, None, None]
    rho_c = rho[Hz:Hz + Nz][:, None, None]
    rho_below = rho[Hz - 1:Hz - 1 + Nz][:, None, None]
    rho_above = rho[Hz + 1:Hz + 1 + Nz][:, None, None]
    Ax, Ay, Az, V = dy * dz, dx * dz, dx * dy, dx * dy * dz
    info = {}
    div, info["x"] = _direction(lambda s: view(c, sx=s), rho_c * (Ax * view(u)), rho_c * (Ax * view(u, sx=1)), lo, hi, None, None,
                                w1, limit_all_four)
    if not flat_y:
        dy_div, info["y"] = _direction(lambda s: view(c, sy=s), rho_c * (Ay * view(v)), rho_c * (Ay * view(v, sy=1)), lo, hi, None, None,
                                       w1, limit_all_four)
        div = div + dy_div
    B = np.array([z_buffer(k, Nz) for k in range(Nz + 1)])
    dz_div, info["z"] = _direction(lambda s: view(c, sz=s), (rho_below + rho_c) / 2 * (Az * view(w)),
                                   (rho_c + rho_above) / 2 * (Az * view(w, sz=1)), lo, hi, B[:-1, None, None], B[1:, None, None],
                                   w1, limit_all_four)
    return -(div + dz_div) / V, info
