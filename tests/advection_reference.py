"""Independent reference of the plain WENO 5 / 7 / 9 advective tendencies of the anelastic model, numpy in np.longdouble:

    G(rho u), G(rho v), G(rho w) (+ buoyancy), G(rho c)       u_tendency, v_tendency, w_tendency, scalar_tendency

on (Periodic, Periodic, Bounded), (Periodic, Flat, Bounded), (Periodic, Bounded, Bounded) and (Bounded, Flat, Bounded).  Written from the
operator definitions of Breeze (div_rhoUc of src/Advection.jl; x_, y_, z_momentum_tendency and scalar_tendency of
AtmosphereModels/dynamics_kernel_functions.jl; buoyancy_force of AnelasticEquations/anelastic_buoyancy.jl) and of the flux-form momentum
advection of Oceananigans they call (div_Uu, div_Uv, div_Uw with the momentum as the advecting field).  It shares no code with oracle/,
with tests/bounded_weno_reference.py or with any kernel header; the only imports are the exact-rational tables of
tools/gen_weno_tables.py for r = 4, 5 (tables(r), centered(n)).  Orders 5, 3 and 1 and Centered(4) are written out by hand.

CONVENTIONS.  Arrays are halo-inclusive and halo-filled, laid out (z, y, x); index 0 below is the first interior entry.  Face i of a
direction is the low-side face of cell i; a Bounded direction with N cells has faces 0 .. N, faces 0 and N are the walls.  u lives on x
faces, v on y faces, w (and rho w) on z faces (one more level).  Metrics: dz_c(k) = zf[k+1] - zf[k] (a regular z, given as (a, b),
carries the single number (b - a) / Nz), dz_f(k) = zc[k] - zc[k-1], Ax = dy dz_c, Ay = dx dz_c, Az = dx dy, V_c = dx dy dz_c,
V_f = dx dy dz_f.  A Flat y has Ny = 1, dy = 1, no halo, no y term, and every y interpolation is the identity.

RULES, in the order a tendency is built:

 1. Buffer.  A scheme of order 2R - 1 (R = 3, 4, 5) uses buffer B = R in a Periodic direction.  In a Bounded direction the target at
    index idx takes the largest B <= R with
        face target   (value at face idx from centre data):    B     <= idx <= N - B
        centre target (value at centre idx from face data):    B - 1 <= idx <= N - B
    and B = 1 where none fits: the cascade 9 -> 7 -> 5 -> 3 -> 1.  The two rules differ on the low side: a centre target is admitted one
    index closer to the low wall than a face target.  (keyword centre_rule_as_face breaks this.)

 2. Upwind-biased reconstruction with buffer B from the 2B - 1 values v[0 .. 2B-2] whose upwind value is v[B-1], at the point between
    v[B-1] and v[B].  Face target idx, left bias: centres idx-B .. idx+B-2; right bias: centres idx+B-1 down to idx-B+1.  A centre target
    idx is the face rule of idx + 1 applied to face data (left: faces idx-B+1 .. idx+B-1, right: faces idx+B down to idx-B+2).
      B = 1: v[0].
      B = 2: candidates (v1 + v2) / 2 and (3 v1 - v0) / 2, linear weights 2/3, 1/3, beta_0 = (v2 - v1)^2, beta_1 = (v1 - v0)^2.
      B = 3: candidates (2 c + 5 d - e) / 6, (-b + 5 c + 2 d) / 6, (2 a - 7 b + 11 c) / 6 of cells a .. e (c upwind), linear weights 3/10,
             3/5, 1/10; the Jiang-Shu indicators times 3 in squared-difference form:
             beta_0 = 13/4 (c - 2d + e)^2 + 3/4 (3c - 4d + e)^2, beta_1 = 13/4 (b - 2c + d)^2 + 3/4 (b - d)^2,
             beta_2 = 13/4 (a - 2b + c)^2 + 3/4 (a - 4b + 3c)^2.
      B = 4, 5: stencil s = 0 .. B-1 holds v[B-1-s .. 2B-2-s]; candidates, linear weights D_s and the quadratic forms beta_s from the
             exact tables (beta scaled x240, x5040), evaluated after subtracting the upwind value from the stencil (beta and
             candidate - upwind value do not change under a constant shift), so no large mean enters a product.
      WENO-Z weights for every B >= 2: alpha_s = D_s (1 + (tau / (beta_s + eps))^2), eps = 1e-8, value = sum alpha_s p_s / sum alpha_s, with
             the global indicators tau = |beta_0 - beta_1| (B = 2), |beta_0 - beta_2| (3), |beta_0 + 3 beta_1 - 3 beta_2 - beta_3| (4),
             |beta_0 + 2 beta_1 - 6 beta_2 + 2 beta_3 + beta_4| (5).  (keyword tau7_without_factor_3: |beta_0 + beta_1 - beta_2 - beta_3|.)

 3. Symmetric interpolation of the advecting mass flux: Centered(order 2 (B - 1)) with the buffer B of rule 1 at the same target (its own
    reduction near walls; order 2 for B <= 2): sum_d c_d (q[-1-d] + q[d]) over the pairs straddling the target, c = (1/2);
    (7/12, -1/12); centered(6); centered(8).  (keyword centered4_weights replaces (7/12, -1/12).)  What is interpolated is area x momentum:
    Ax rho u, Ay rho v, Az rho w.  Ax and Ay carry dz_c of the level of each value, so in the z interpolation of rho u, rho v to a w
    face dz_c rides inside.  (keyword dzf_outside: dz_f(k) times the interpolated rho u, rho v instead.)

 4. Bias: left where the interpolated advecting flux is > 0, right otherwise (zero: right).  For scalars the advecting quantity is the
    face velocity itself.  (keyword bias_from_advected: the sign of the two-point mean of the advected velocity at the target.)

 5. Fluxes and tendencies.  Momentum flux = interpolated advecting flux x reconstructed velocity:
      G(rho u)(i) = -[ (Uu(i) - Uu(i-1)) + (Vu(j+1) - Vu(j)) + (Wu(k+1) - Wu(k)) ] / V_c(k)
          Uu at centre i: rho u -> x centre, u -> x centre;  Vu at (x face i, y face j): rho v -> x face, u -> y face;
          Wu at (x face i, z face k): rho w -> x face, u -> z face
      G(rho v)(j) likewise with x and y exchanged
      G(rho w)(k) = -[ (Uw(i+1) - Uw(i)) + (Vw(j+1) - Vw(j)) + (Ww(k) - Ww(k-1)) ] / V_f(k) + (b(k-1) + b(k)) / 2
          Uw at (x face i, z face k): rho u -> z face, w -> x face;  Ww at centre k: rho w -> z centre, w -> z centre
          b = -g rho_r (R_d T_r / (R_m T) - 1),  R_m = (1 - q) R_d + q R_v   (dry reference, vapour only)
          (keyword buoyancy_levels_above averages b(k), b(k+1).)
      G(rho c) = -[ dX + dY + dZ ] / V_c,  X(i) = rho_k Ax u(i) c_face,  Y likewise,  Z(k) = (rho_{k-1} + rho_k) / 2 Az w(k) c_face
    A direction whose advecting field is identically zero contributes exactly nothing and is skipped.

 6. Written cells: the interior, without the first u face between x walls (i = 0), the first v face between y walls (j = 0) and both
    w wall faces (k = 0, Nz).  `written(geometry, field)` gives the slices of the interior the operator writes; entries outside hold NaN.

Every function returns (G over the interior [w: faces 0 .. Nz-1], info); info[direction] = {"flux": the advecting quantity whose sign
picks the bias, at the low-side targets of that direction, "face_buffers", "centre_buffers": the buffers used}."""
import importlib.util
import os
from dataclasses import dataclass

import numpy as np

LD = np.longdouble
EPS = LD("1e-8")
Z, Y, X = 0, 1, 2


def _tables():
    spec = importlib.util.spec_from_file_location("gen_weno_tables", os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools",
                                                                                  "gen_weno_tables.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    ld = lambda f: LD(f.numerator) / LD(f.denominator)
    wide = {}
    for r in (4, 5):
        C, D, B = gen.tables(r)
        wide[r] = ([[ld(x) for x in row] for row in C], [ld(x) for x in D], [[[ld(x) for x in row] for row in Bs] for Bs in B])
    return wide, {6: [ld(x) for x in gen.centered(6)], 8: [ld(x) for x in gen.centered(8)]}


WIDE, CENTERED = _tables()
TAU = {4: (1, 3, -3, -1), 5: (1, 2, -6, 2, 1)}


@dataclass
class Geometry:
    """z: the Nz + 1 faces, or (a, b) with Nz for a regular z; halo = (Hx, Hy, Hz), Hy = 0 on a Flat y; topology: three of "Periodic",
    "Bounded", "Flat" for x, y, z"""
    z: object
    dx: float
    dy: float
    halo: tuple
    topology: tuple = ("Periodic", "Periodic", "Bounded")
    Nz: int = None

    def __post_init__(self):
        if isinstance(self.z, tuple) and len(self.z) == 2:
            a, b = self.z
            self.dzc = np.full(self.Nz, LD((b - a) / self.Nz))
            self.dzf_ = np.full(self.Nz + 1, LD((b - a) / self.Nz))
        else:
            zf = np.asarray(self.z, dtype=LD)
            self.Nz = zf.size - 1
            self.dzc = zf[1:] - zf[:-1]
            zc = (zf[1:] + zf[:-1]) / 2
            self.dzf_ = np.full(self.Nz + 1, LD("nan"))
            self.dzf_[1:-1] = zc[1:] - zc[:-1]
        self.flat_y = self.topology[1] == "Flat"
        self.dx, self.dy = LD(self.dx), LD(1 if self.flat_y else self.dy)
        assert self.topology[2] == "Bounded" and self.topology[0] in ("Periodic", "Bounded")
        # (z, y, x) order
        self.bounded = (True, self.topology[1] == "Bounded", self.topology[0] == "Bounded")
        self.H = (self.halo[2], self.halo[1], self.halo[0])


def buffer_of(idx, N, R, face, centre_rule_as_face=False):
    """rule 1 in a Bounded direction"""
    for B in range(R, 1, -1):
        lo = B if (face or centre_rule_as_face) else B - 1
        if lo <= idx <= N - B:
            return B
    return 1


def written(geo, field, shape):
    """slices (z, y, x) of the interior array of `field` in "u", "v", "w", "c" that the operator writes"""
    Nz, Ny, Nx = shape
    sl = [slice(0, Nz), slice(0, Ny), slice(0, Nx)]
    if field == "w":
        sl[Z] = slice(1, Nz)
    if field == "u" and geo.bounded[X]:
        sl[X] = slice(1, Nx)
    if field == "v" and geo.bounded[Y]:
        sl[Y] = slice(1, Ny)
    return tuple(sl)


# ---- rule 2 -----------------------------------------------------------------------------------------------------------------------------
def _weno_z(D, betas, candidates, tau):
    num = den = 0
    for d, b, p in zip(D, betas, candidates):
        alpha = d * (1 + (tau / (b + EPS)) ** 2)
        num, den = num + alpha * p, den + alpha
    return num / den


def upwind3(v):
    v0, v1, v2 = v
    b0, b1 = (v2 - v1) ** 2, (v1 - v0) ** 2
    return _weno_z((LD(2) / 3, LD(1) / 3), (b0, b1), ((v1 + v2) / 2, (3 * v1 - v0) / 2), np.abs(b0 - b1))


def upwind5(v):
    a, b, c, d, e = v
    q134, q34 = LD(13) / 4, LD(3) / 4
    b0 = q134 * (c - 2 * d + e) ** 2 + q34 * (3 * c - 4 * d + e) ** 2
    b1 = q134 * (b - 2 * c + d) ** 2 + q34 * (b - d) ** 2
    b2 = q134 * (a - 2 * b + c) ** 2 + q34 * (a - 4 * b + 3 * c) ** 2
    # candidates as upwind value + differences
    p0 = c + (5 * (d - c) - (e - c)) / 6
    p1 = c + (2 * (d - c) - (b - c)) / 6
    p2 = c + (2 * (a - c) - 7 * (b - c)) / 6
    return _weno_z((LD(3) / 10, LD(3) / 5, LD(1) / 10), (b0, b1, b2), (p0, p1, p2), np.abs(b0 - b2))


def upwind_wide(v, r, tau7_without_factor_3=False):
    C, D, Bt = WIDE[r]
    up = v[r - 1]
    d = [x - up for x in v]
    betas, cands = [], []
    for s in range(r):
        w = d[r - 1 - s:2 * r - 1 - s]
        betas.append(sum(Bt[s][j][l] * w[j] * w[l] for j in range(r) for l in range(j, r)))
        cands.append(up + sum(C[s][j] * w[j] for j in range(r)))
    t = (1, 1, -1, -1) if (r == 4 and tau7_without_factor_3) else TAU[r]
    tau = np.abs(sum(c * b for c, b in zip(t, betas)))
    return _weno_z(D, betas, cands, tau)


def upwind(v, B, **kw):
    """v: the 2B - 1 values, far upwind side first"""
    if B == 1:
        return v[0]
    if B == 2:
        return upwind3(v)
    if B == 3:
        return upwind5(v)
    return upwind_wide(v, B, **kw)


class _Operator:
    def __init__(self, geo, order, shape, centre_rule_as_face=False, centered4_weights=(LD(7) / 12, -LD(1) / 12), dzf_outside=False,
                 bias_from_advected=False, buoyancy_levels_above=False, tau7_without_factor_3=False):
        assert order in (5, 7, 9)
        self.geo, self.R = geo, (order + 1) // 2
        self.N = shape                      # (Nz, Ny, Nx) of the centre interior
        self.crf, self.c4 = centre_rule_as_face, tuple(LD(x) for x in centered4_weights)
        self.dzf_outside, self.bias_from_advected, self.b_above = dzf_outside, bias_from_advected, buoyancy_levels_above
        self.wide_kw = dict(tau7_without_factor_3=tau7_without_factor_3)
        assert all(h >= self.R for h, n in zip(geo.H, shape) if n > 1 or h > 0), "halo narrower than the scheme"
        self.info = {}

    # -- windows --------------------------------------------------------------------------------------------------------------------------
    def cut(self, a, o):
        """the interior box of `a` shifted by o = (oz, oy, ox)"""
        return a[tuple(slice(h + s, h + s + n) for h, s, n in zip(self.geo.H, o, self.N))]

    @staticmethod
    def move(o, axis, s):
        o = list(o)
        o[axis] += s
        return tuple(o)

    def column(self, col, o):
        """a column over levels -Hz .. (halo-inclusive), as (Nz, 1, 1) at the levels of the box shifted by o"""
        h = self.geo.H[Z]
        return col[h + o[Z]:h + o[Z] + self.N[Z]][:, None, None]

    def dzc(self, o):
        """dz_c at the levels of the box; outside 0 .. Nz-1 the value is never used by a target that is written (rule 1): NaN there"""
        k = np.arange(self.N[Z]) + o[Z]
        out = np.full(self.N[Z], LD("nan"))
        ok = (k >= 0) & (k < self.N[Z])
        out[ok] = self.geo.dzc[k[ok]]
        return out[:, None, None]

    def buffers(self, axis, o, face):
        """None in a Periodic direction (B = R), else the integer array of rule 1 at the targets of the box, broadcastable"""
        if not self.geo.bounded[axis]:
            return None
        n = self.N[axis]
        B = np.array([buffer_of(i + o[axis], n, self.R, face, self.crf) for i in range(n)])
        return B.reshape([-1 if a == axis else 1 for a in range(3)])

    def select(self, B, per_buffer):
        """per_buffer(b) evaluated for the buffers that occur, picked by B"""
        if B is None:
            return per_buffer(self.R)
        out = None
        for b in sorted(set(B.ravel().tolist())):
            val = per_buffer(b)
            out = val if out is None else np.where(B == b, val, out)
        return out

    # -- rules 2, 3 -----------------------------------------------------------------------------------------------------------------------
    def biased(self, a, o, axis, left, face):
        """upwind-biased value of `a` along `axis` at the face / centre targets of the box shifted by o"""
        B = self.buffers(axis, o, face)
        e = 0 if face else 1        # a centre target idx is the face rule of idx + 1 on face data
        at = lambda s: self.cut(a, self.move(o, axis, s))
        lft = self.select(B, lambda b: upwind([at(e - b + j) for j in range(2 * b - 1)], b, **self.wide_kw))
        rgt = self.select(B, lambda b: upwind([at(e + b - 1 - j) for j in range(2 * b - 1)], b, **self.wide_kw))
        return np.where(left, lft, rgt), B

    def symmetric(self, q, o, axis, face):
        """Centered(2 (B - 1)) of q(s) [the area-weighted momentum at offset s along axis from the box shifted by o] at the targets"""
        if self.N[axis] == 1 and self.geo.H[axis] == 0:      # Flat: identity
            return q(0)
        B = self.buffers(axis, o, face)
        e = 0 if face else 1

        def centred(b):
            h = max(b - 1, 1)
            c = {1: (LD(1) / 2,), 2: self.c4, 3: CENTERED[6], 4: CENTERED[8]}[h]
            return sum(c[d] * (q(e - 1 - d) + q(e + d)) for d in range(h))
        return self.select(B, centred)

    def bias(self, flux, advected, o, axis, face):
        if not self.bias_from_advected:
            return flux > 0
        e = 0 if face else 1
        return (self.cut(advected, self.move(o, axis, e - 1)) + self.cut(advected, self.move(o, axis, e))) / 2 > 0

    def record(self, name, flux, Bf=None, Bc=None):
        d = self.info.setdefault(name, {"face_buffers": set(), "centre_buffers": set()})
        if flux is not None:
            d["flux"] = flux
        for key, B in (("face_buffers", Bf), ("centre_buffers", Bc)):
            if B is not None:
                d[key] |= set(B.ravel().tolist())

    # -- rule 5: one momentum flux.  M: advecting momentum, area(o): its area at the box shifted by o, sym_axis / sym_face: where it is
    #    interpolated to, c: advected velocity, rec_axis / rec_face: where that is reconstructed ------------------------------------------
    def momentum_flux(self, M, area, sym_axis, sym_face, c, rec_axis, rec_face, o, outside=None):
        q = lambda s: area(self.move(o, sym_axis, s)) * self.cut(M, self.move(o, sym_axis, s))
        adv = self.symmetric(q, o, sym_axis, sym_face)
        if outside is not None:
            adv = outside * adv
        rec, B = self.biased(c, o, rec_axis, self.bias(adv, c, o, rec_axis, rec_face), rec_face)
        name = "zyx"[rec_axis]
        if o == (0, 0, 0):
            self.record(name, adv, **({"Bf": B} if rec_face else {"Bc": B}))
        Bs = self.buffers(sym_axis, o, sym_face)
        if o == (0, 0, 0) and Bs is not None:
            self.record("zyx"[sym_axis], None, **({"Bf": Bs} if sym_face else {"Bc": Bs}))
        return adv * rec


def _prepare(geo, order, arrays, defects):
    arrays = [np.asarray(a, dtype=LD) for a in arrays]
    shape = tuple(n - 2 * h for n, h in zip(arrays[0].shape, geo.H))
    return _Operator(geo, order, shape, **defects), arrays


def _active(op, axis, M):
    return (op.N[axis] > 1 or op.geo.H[axis] > 0) and bool(np.any(M != 0))


def u_tendency(geo, order, ru, rv, rw, u, **defects):
    op, (ru, rv, rw, u) = _prepare(geo, order, (ru, rv, rw, u), defects)
    g, O = geo, (0, 0, 0)
    Ax = lambda o: g.dy * op.dzc(o)
    Ay = lambda o: g.dx * op.dzc(o)
    Az = lambda o: g.dx * g.dy
    div = 0
    if _active(op, X, ru):
        F = lambda o: op.momentum_flux(ru, Ax, X, False, u, X, False, o)
        div = div + (F(O) - F((0, 0, -1)))
    if _active(op, Y, rv):
        F = lambda o: op.momentum_flux(rv, Ay, X, True, u, Y, True, o)
        div = div + (F((0, 1, 0)) - F(O))
    if _active(op, Z, rw):
        F = lambda o: op.momentum_flux(rw, Az, X, True, u, Z, True, o)
        div = div + (F((1, 0, 0)) - F(O))
    return _finish(op, "u", -(div / (g.dx * g.dy * op.dzc(O))))


def v_tendency(geo, order, ru, rv, rw, v, **defects):
    op, (ru, rv, rw, v) = _prepare(geo, order, (ru, rv, rw, v), defects)
    g, O = geo, (0, 0, 0)
    Ax = lambda o: g.dy * op.dzc(o)
    Ay = lambda o: g.dx * op.dzc(o)
    Az = lambda o: g.dx * g.dy
    div = 0
    if _active(op, X, ru):
        F = lambda o: op.momentum_flux(ru, Ax, Y, True, v, X, True, o)
        div = div + (F((0, 0, 1)) - F(O))
    if _active(op, Y, rv):
        F = lambda o: op.momentum_flux(rv, Ay, Y, False, v, Y, False, o)
        div = div + (F(O) - F((0, -1, 0)))
    if _active(op, Z, rw):
        F = lambda o: op.momentum_flux(rw, Az, Y, True, v, Z, True, o)
        div = div + (F((1, 0, 0)) - F(O))
    return _finish(op, "v", -(div / (g.dx * g.dy * op.dzc(O))))


def buoyancy(T, q, rho_r, T_r, g, Rd, Rv):
    """rule 5: b at centres; T, q (Nz, Ny, Nx) windows, rho_r, T_r (Nz, 1, 1)"""
    Rm = (1 - q) * Rd + q * Rv
    return -g * (rho_r * (Rd * T_r / (Rm * T) - 1))


def w_tendency(geo, order, ru, rv, rw, w, T=None, q=None, rho_r=None, T_r=None, constants=None, **defects):
    """constants = (g, R_d, R_v); rho_r, T_r: the reference columns at the Nz + 2 Hz centres.  T = None: advection alone.
    The result covers faces 0 .. Nz - 1; face 0 is not written (NaN)."""
    op, (ru, rv, rw, w) = _prepare(geo, order, (ru, rv, rw, w), defects)
    g, O = geo, (0, 0, 0)
    dzf = g.dzf_[:-1][:, None, None]
    if op.dzf_outside:
        Ax, Ay, out_x, out_y = (lambda o: 1), (lambda o: 1), g.dy * dzf, g.dx * dzf
    else:
        Ax, Ay, out_x, out_y = (lambda o: g.dy * op.dzc(o)), (lambda o: g.dx * op.dzc(o)), None, None
    Az = lambda o: g.dx * g.dy
    div = 0
    if _active(op, X, ru):
        F = lambda o: op.momentum_flux(ru, Ax, Z, True, w, X, True, o, outside=out_x)
        div = div + (F((0, 0, 1)) - F(O))
    if _active(op, Y, rv):
        F = lambda o: op.momentum_flux(rv, Ay, Z, True, w, Y, True, o, outside=out_y)
        div = div + (F((0, 1, 0)) - F(O))
    if _active(op, Z, rw):
        F = lambda o: op.momentum_flux(rw, Az, Z, False, w, Z, False, o)
        div = div + (F(O) - F((-1, 0, 0)))
    G = -(div / (g.dx * g.dy * dzf))
    if T is not None:
        T, q, rho_r, T_r = (np.asarray(a, dtype=LD) for a in (T, q, rho_r, T_r))
        gr, Rd, Rv = (LD(c) for c in constants)
        b = lambda o: buoyancy(op.cut(T, o), op.cut(q, o), op.column(rho_r, o), op.column(T_r, o), gr, Rd, Rv)
        G = G + ((b((0, 0, 0)) + b((1, 0, 0))) / 2 if op.b_above else (b((-1, 0, 0)) + b((0, 0, 0))) / 2)
    return _finish(op, "w", G + np.zeros(op.N, dtype=LD))


def scalar_tendency(geo, order, u, v, w, c, rho_r, **defects):
    op, (u, v, w, c) = _prepare(geo, order, (u, v, w, c), defects)
    rho_r = np.asarray(rho_r, dtype=LD)
    g, O = geo, (0, 0, 0)
    div = 0

    def flux(vel, axis, o):
        adv = op.cut(vel, o)
        rec, B = op.biased(c, o, axis, adv > 0, True)
        if o == O:
            op.record("zyx"[axis], adv, Bf=B)
        if axis == Z:
            return (op.column(rho_r, op.move(o, Z, -1)) + op.column(rho_r, o)) / 2 * ((g.dx * g.dy * adv) * rec)
        area = (g.dy if axis == X else g.dx) * op.dzc(o)
        return op.column(rho_r, o) * ((area * adv) * rec)

    for axis, vel in ((X, u), (Y, v), (Z, w)):
        if _active(op, axis, vel):
            div = div + (flux(vel, axis, op.move(O, axis, 1)) - flux(vel, axis, O))
    return _finish(op, "c", -(div / (g.dx * g.dy * op.dzc(O))) + np.zeros(op.N, dtype=LD))


def _finish(op, field, G):
    G = np.array(G + np.zeros(op.N, dtype=LD), dtype=LD)
    mask = np.zeros(op.N, dtype=bool)
    mask[written(op.geo, field, op.N)] = True
    G[~mask] = LD("nan")
    return G, op.info
