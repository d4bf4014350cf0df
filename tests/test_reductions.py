"""The whole-field reductions behind the C ABI against numpy (tests/reductions_reference.py, np.longdouble):
bz_max_abs_divergence (k_max_abs_div — the judge of every "the projection closes the step" assertion of the suite),
bz_cell_advection_timescale (k_max_inverse_advection_timescale), bz_any_nan (k_any_nan) and the moisture scan of the lean seam
(k_scan_moisture).  The momentum is NOT projected: the divergence is of order S = max(|ru|/dx + |rv|/dy + |rw|/dzc), so a tile, a row, a
level or a wave's maximum that the kernel dropped shows.  Every reference is computed from the arrays read back from the device after
the call (halos and wall faces as the library left them); for the Float32 twin it is the longdouble result on the float32 values, with
the metrics the library derives in float32 from the faces it is handed.

Bounds: divergence |got - want| <= 16 eps S (six products and five sums of terms bounded by S, each rounded once, FMA contraction
allowed, plus the rounding of Ax, Ay, Vinv_c themselves); timescale relative error <= 8 eps (three quotients, two sums, one reciprocal,
the rounded metrics).  Worst ratios measured on the MI355X over every case of this module, planted extrema included:
  divergence  |got - want| / (eps S):     Float64 2.04 (16x8x8, rho u planted at (15, 4, 0)), Float32 1.47 (70x9x12, rho u planted at (64, 8, 11))
  timescale   |got - want| / (eps want):  Float64 1.08 (70x9x12, u planted at (69, 4, 11)), Float32 1.03 (stretched, v planted at (31, 11, 23))

Two shapes are the nearest the library builds to the ones one would wish for (both refusals are asserted below): (Bounded, Flat, Bounded)
runs at (34, 10), not (33, 10) — an odd number of columns between walls in x is refused; (Periodic, Bounded, Bounded) runs at (32, 16, 8),
not (24, 9, 8) — the cosine-transform solve between walls in y needs Nx a power of two and Ny a multiple of 8."""
import ctypes as C

import numpy as np
import pytest

import reductions_reference as rr
from helpers import make_pair, push_state, randomize

pytestmark = pytest.mark.gpu

L = np.longdouble
PPB, PFB, BFB, PBB = (("Periodic", "Periodic", "Bounded"), ("Periodic", "Flat", "Bounded"), ("Bounded", "Flat", "Bounded"),
                      ("Periodic", "Bounded", "Bounded"))
STRETCHED = 1e4 * np.linspace(0, 1, 25) ** 1.3          # the faces of test_tendencies_stretched_grid
H = 1e4 / 37          # dx = H, dy = 1.25 H, dz = 0.8 H: three different spacings (a swapped metric shows), none a float32 number, and close
#                       enough to one another that 1e3 planted in ANY component of a field of amplitude 1 stands 100 x above the rest


def _ext(size, z=None):
    Nx, Nz = size[0], size[-1]
    y = (0.0, 1.25 * H * size[1]) if len(size) == 3 else None
    return ((0.0, H * Nx), y, (0.0, 0.8 * H * Nz)) if z is None else ((0.0, 300.0 * Nx), (0.0, 375.0 * size[1]), z)


# name: (size, topology, (x, y, z)); tiles are TX x TY = 64 x 4 threads, one wave per row of a tile
SHAPES = {
    "16x8x8": ((16, 8, 8), PPB, _ext((16, 8, 8))),                        # less than one x tile
    "70x9x12": ((70, 9, 12), PPB, _ext((70, 9, 12))),                     # ragged in x and y, one tile seam at i = 64
    "130x6x5": ((130, 6, 5), PPB, _ext((130, 6, 5))),                     # two seams, ragged, Ny no multiple of 4
    "stretched": ((32, 12, 24), PPB, _ext((32, 12, 24), STRETCHED)),      # the metric columns
    "flat_y": ((40, 12), PFB, _ext((40, 12))),
    "walls_x": ((34, 10), BFB, _ext((34, 10))),
    "walls_y": ((32, 16, 8), PBB, _ext((32, 16, 8))),
}
F64, F32 = np.float64, np.float32
MODELS = [(n, F64) for n in SHAPES] + [("70x9x12", F32), ("stretched", F32)]
IDS = ["%s-%s" % (n, "f32" if r is F32 else "f64") for n, r in MODELS]
MOMENTUM, VELOCITIES = ("ρu", "ρv", "ρw"), ("u", "v", "w")


# ---- models --------------------------------------------------------------------------------------------------------------------------
def _metrics_as_the_library_holds_them(g, real):
    """the Float32 twin derives every metric in float32 from float32 faces (csrc/bz_context.hip); the Float64 one as the oracle does"""
    if real is F64:
        return g
    Nz, Hz, f = g.Nz, g.Hz, np.float32
    zf = g.zf.astype(f)
    ext = np.empty(Nz + 1 + 2 * Hz, f)
    ext[Hz:Hz + Nz + 1] = zf
    for h in range(1, Hz + 1):
        ext[Hz - h] = ext[Hz - h + 1] - (zf[1] - zf[0])
        ext[Hz + Nz + h] = ext[Hz + Nz + h - 1] + (zf[Nz] - zf[Nz - 1])
    zc = f(0.5) * (ext[:-1] + ext[1:])
    dzc, dzf = ext[1:] - ext[:-1], np.zeros(Nz + 1 + 2 * Hz, f)
    dzf[1:-1] = zc[1:] - zc[:-1]
    dzf[0], dzf[-1] = dzf[1], dzf[-2]
    if g.regular_z:
        dzc[:] = dzf[:] = (zf[Nz] - zf[0]) / f(Nz)
    assert dzc.dtype == f and dzf.dtype == f and zc.dtype == f
    g.dx, g.dy, g.dzc, g.dzf = float(f(g.dx)), float(f(g.dy)), dzc.astype(F64), dzf.astype(F64)
    return g


class Model:
    def __init__(self, oracle, bz, name, real):
        size, topo, (x, y, z) = SHAPES[name]
        self.name, self.real, self.eps = name, real, L(np.finfo(real).eps)
        self.om = None
        if topo == PPB and real is F64:
            self.om, self.hm = make_pair(oracle, bz, size, extent=(x, y, z), z_faces=None if isinstance(z, tuple) else z)
            self.og = self.om.grid
        else:
            ext = dict(x=x, z=z) if "Flat" in topo else dict(x=x, y=y, z=z)
            self.og = _metrics_as_the_library_holds_them(oracle.Grid(size, topology=topo, **ext), real)
            grid = bz.RectilinearGrid(size, topology=topo, float_type=real, **ext)
            self.hm = bz.AtmosphereModel(grid, dynamics=bz.AnelasticDynamics(bz.ReferenceState(grid, potential_temperature=300.0)),
                                         advection=bz.WENO(order=5))
            self.hm.set(θ=300.0)
        g = self.og
        self.N = (g.Nx, g.Ny, g.Nz)
        self.walls_x, self.walls_y = topo[0] == "Bounded", topo[1] == "Bounded"

    def momentum(self, seed, unit=False):
        """seeded random momentum, not projected: through the oracle where make_pair applies, else straight into the interiors;
        `unit`: every component scaled to max |.| = 1"""
        import torch
        hm = self.hm
        if self.om is not None:
            randomize(self.om, seed)
            push_state(self.om, hm, names=("ru", "rv", "rw", "rtheta", "rq"))
        else:
            rng = np.random.default_rng(seed)
            for k in MOMENTUM:
                f = hm.momentum[k]
                f.interior.copy_(torch.from_numpy(5.0 * rng.standard_normal(tuple(f.interior.shape))).to(f.dtype))
        if unit:
            for k in MOMENTUM:
                hm.momentum[k].parent.div_(hm.momentum[k].interior.abs().max())

    def velocities(self, bz, seed):
        """update_state! of the random momentum, then every component scaled to max |.| = 1"""
        self.momentum(seed)
        bz.update_state_(self.hm, compute_tendencies=False)
        for k in VELOCITIES:
            f = self.hm.velocities[k]
            f.parent.div_(f.interior.abs().max())


@pytest.fixture(scope="module")
def zoo(oracle, bz):
    models = {}

    def get(name, real):
        if (name, real) not in models:
            models[name, real] = Model(oracle, bz, name, real)
        return models[name, real]
    return get


def positions(Nx, Ny, Nz):
    """(i, j, k): the eight corners, and the tile seams / last threads crossed with the rows around a tile edge and both end levels"""
    corners = {(i, j, k) for i in (0, Nx - 1) for j in (0, Ny - 1) for k in (0, Nz - 1)}
    I = {min(i, Nx - 1) for i in (62, 63, 64, 65, 127, 128, Nx - 1)}
    J = {min(j, Ny - 1) for j in (3, 4, Ny - 1)}
    return sorted(corners | {(i, j, k) for i in I for j in J for k in (0, Nz - 1)})


def test_positions_reach_every_seam():
    p = positions(130, 6, 5)
    assert {i for i, _, _ in p} == {0, 62, 63, 64, 65, 127, 128, 129} and {j for _, j, _ in p} == {0, 3, 4, 5} and {k for _, _, k in p} == {0, 4}
    assert positions(16, 8, 8) == sorted({(i, j, k) for i in (0, 15) for j in (0, 7) for k in (0, 7)} | {(15, j, k) for j in (3, 4) for k in (0, 7)})
    assert {j for _, j, _ in positions(40, 1, 12)} == {0}


def test_the_wall_shapes_one_would_wish_for_are_refused(bz):
    """(33, 10) between walls in x and (24, 9, 8) between walls in y: the day the library builds them, SHAPES should move to them"""
    from breeze_jl_amd import _lib

    def build(size, topo):
        x, y, z = _ext(size)
        ext = dict(x=x, z=z) if "Flat" in topo else dict(x=x, y=y, z=z)
        grid = bz.RectilinearGrid(size, topology=topo, **ext)
        bz.AtmosphereModel(grid, dynamics=bz.AnelasticDynamics(bz.ReferenceState(grid, potential_temperature=300.0)), advection=bz.WENO(order=5))

    with pytest.raises(NotImplementedError):
        build((33, 10), BFB)
    with pytest.raises(_lib.BreezeHIPError):
        build((24, 9, 8), PBB)


def _np(field):
    return field.parent.cpu().numpy()


def _poison_halos(fields, value):
    for f in fields:
        keep = f.interior.clone()
        f.parent.fill_(value)
        f.interior.copy_(keep)


class _planted:
    """field.interior[k, j, i] += add (or = value) for the length of the block; the old value comes back bit for bit"""

    def __init__(self, field, ijk, add=None, value=None):
        i, j, k = ijk
        self.cell, self.add, self.value = field.interior[k:k + 1, j:j + 1, i:i + 1], add, value

    def __enter__(self):
        self.old = self.cell.clone()
        if self.add is not None:
            self.cell.add_(self.add)
        else:
            self.cell.fill_(self.value)

    def __exit__(self, *exc):
        self.cell.copy_(self.old)


# ---- divergence ----------------------------------------------------------------------------------------------------------------------
def _divergence(M, label):
    """(got, want, S): the device's answer and the reference on what the device holds after the call; asserts the 16 eps S bound"""
    got = M.hm.max_abs_divergence()
    want, S = rr.max_abs_divergence(M.og, *(_np(M.hm.momentum[k]) for k in MOMENTUM))
    ratio = float(abs(L(got) - want) / (M.eps * S))
    print(f"REDUCTION divergence {M.name} {M.real.__name__} {label}: got {got:.17g} want {float(want):.17g} S {float(S):.6g} ratio {ratio:.3f}")
    assert ratio <= 16.0, (label, got, float(want), float(S), ratio)
    return got, want, S


@pytest.mark.parametrize("name,real", MODELS, ids=IDS)
def test_divergence_of_a_random_field(zoo, name, real):
    M = zoo(name, real)
    M.momentum(seed=21)
    got, want, S = _divergence(M, "random")
    assert want > 0.1 * S          # of order S, not a projected field's zero


@pytest.mark.parametrize("name,real", MODELS, ids=IDS)
def test_divergence_finds_a_planted_extremum(zoo, name, real):
    """1e3 added to one face of a field of amplitude 1: the answer follows the reference and stands above 100 x the answer without the
    plant, wherever the face is — a cell the kernel skipped cannot pass.  The wall faces themselves (rho u at i = 0 between walls in x)
    are left out: the halo fill that opens bz_max_abs_divergence sets them to zero."""
    M = zoo(name, real)
    Nx, Ny, Nz = M.N
    M.momentum(seed=22, unit=True)
    base, _, _ = _divergence(M, "amplitude 1")
    plants = [("ρu", p) for p in positions(*M.N) if not (M.walls_x and p[0] == 0)]
    plants += [("ρw", (Nx // 2, Ny // 2, Nz - 1)), ("ρw", (Nx - 1, Ny - 1, Nz - 1))]      # the faces whose neighbour is a wall or a wrap
    if Ny > 1:
        plants += [("ρv", (Nx // 2, Ny - 1, Nz // 2)), ("ρv", (Nx - 1, Ny - 1, 0))]
    for key, p in plants:
        with _planted(M.hm.momentum[key], p, add=1e3):
            got, _, _ = _divergence(M, f"{key} + 1e3 at {p}")
            assert got > 100.0 * base, (key, p, got, base)
    assert M.hm.max_abs_divergence() == base          # every plant is gone


@pytest.mark.parametrize("name,real", MODELS, ids=IDS)
def test_divergence_fills_the_momentum_halos_itself(zoo, name, real):
    M = zoo(name, real)
    M.momentum(seed=23)
    before, _, _ = _divergence(M, "before the halos are poisoned")
    _poison_halos([M.hm.momentum[k] for k in MOMENTUM], 1e30)
    assert M.hm.max_abs_divergence() == before
    _divergence(M, "after")


@pytest.mark.parametrize("real", [F64, F32], ids=["f64", "f32"])
def test_divergence_of_non_finite_momentum_is_never_finite(zoo, real):
    """the judge of `assert div < tol` must not pass a blown-up state: non-finite momentum reports +Inf (NaN is tolerated for an
    infinite momentum, whose divergence is Inf - Inf in one cell's neighbour), never a finite value.  (5, 2, 1) puts the NaN in
    lanes 4 and 5 of a wave whose lane 0 holds a finite value."""
    M = zoo("70x9x12", real)
    ru = M.hm.momentum["ρu"]
    M.momentum(seed=24)
    assert np.isfinite(M.hm.max_abs_divergence())
    for p in ((5, 2, 1), (0, 0, 0)):
        with _planted(ru, p, value=float("nan")):
            got = M.hm.max_abs_divergence()
            print(f"REDUCTION divergence non-finite {real.__name__}: NaN at {p} -> {got}")
            assert got == np.inf, (p, got)
    with _planted(ru, (37, 5, 7), value=float("inf")):
        got = M.hm.max_abs_divergence()
        print(f"REDUCTION divergence non-finite {real.__name__}: +Inf at (37, 5, 7) -> {got}")
        assert not np.isfinite(got), got
    keep = ru.interior.clone()
    ru.interior.fill_(float("nan"))
    got = M.hm.max_abs_divergence()
    print(f"REDUCTION divergence non-finite {real.__name__}: all NaN -> {got}")
    ru.interior.copy_(keep)
    assert got == np.inf, got
    assert np.isfinite(M.hm.max_abs_divergence())


# ---- advection timescale -------------------------------------------------------------------------------------------------------------
def _timescale(bz, M, formulation, label):
    """(got, want): asserts the 8 eps bound against the reference on the velocities the device holds"""
    got = bz.cell_advection_timescale(M.hm, formulation)
    want = rr.advection_timescale(M.og, *(_np(M.hm.velocities[k]) for k in VELOCITIES), horizontal=formulation == "Horizontal")
    ratio = float(abs(L(got) - want) / (M.eps * want))
    print(f"REDUCTION timescale {M.name} {M.real.__name__} {formulation} {label}: got {got:.17g} want {float(want):.17g} ratio {ratio:.3f}")
    assert ratio <= 8.0, (label, got, float(want), ratio)
    return got, want


FORMULATIONS = ["ThreeDimensional", "Horizontal"]


@pytest.mark.parametrize("formulation", FORMULATIONS)
@pytest.mark.parametrize("name,real", MODELS, ids=IDS)
def test_timescale_of_a_random_state(bz, zoo, name, real, formulation):
    M = zoo(name, real)
    M.momentum(seed=31)
    bz.update_state_(M.hm, compute_tendencies=False)
    got, _ = _timescale(bz, M, formulation, "random")
    assert 0.0 < got < np.inf


@pytest.mark.parametrize("formulation", FORMULATIONS)
@pytest.mark.parametrize("name,real", MODELS, ids=IDS)
def test_timescale_finds_a_planted_extremum(bz, zoo, name, real, formulation):
    """1e3 added to one velocity of a state of amplitude 1, written straight into the field (the entry point takes bare pointers).  On
    the stretched grid the plants in w at k = 1 and k = Nz - 1 are the ones tests/test_reductions_reference.py shows to move by more
    than 6e-3 if dzc[k] or a shifted dzf were read for dzf[k]."""
    M = zoo(name, real)
    Nx, Ny, Nz = M.N
    M.velocities(bz, seed=32)
    base, _ = _timescale(bz, M, formulation, "amplitude 1")
    plants = [("u", p) for p in positions(*M.N)]
    if Ny > 1:
        plants += [("v", (Nx // 2, Ny - 1, Nz // 2)), ("v", (Nx - 1, Ny - 1, Nz - 1))]
    if formulation == "ThreeDimensional":
        plants += [("w", (Nx // 2, Ny // 2, k)) for k in (1, Nz - 1)] + [("w", (Nx - 1, Ny - 1, Nz - 1)), ("w", (0, 0, 1))]
    for key, p in plants:
        with _planted(M.hm.velocities[key], p, add=1e3):
            got, _ = _timescale(bz, M, formulation, f"{key} + 1e3 at {p}")
            spacing = {"u": M.og.dx, "v": M.og.dy, "w": M.og.dzf[M.og.Hz + p[2]]}[key]
            assert got <= spacing / 999.0 * (1 + 1e-6) < base, (key, p, got, base)          # |planted value| >= 999 sets the answer
    assert bz.cell_advection_timescale(M.hm, formulation) == base
    if formulation == "Horizontal":          # w is not read at all
        with _planted(M.hm.velocities["w"], (Nx // 2, Ny // 2, 1), value=float("nan")):
            assert bz.cell_advection_timescale(M.hm, formulation) == base


@pytest.mark.parametrize("formulation", FORMULATIONS)
@pytest.mark.parametrize("name,real", MODELS, ids=IDS)
def test_timescale_reads_no_halo_and_no_top_face(bz, zoo, name, real, formulation):
    M = zoo(name, real)
    M.velocities(bz, seed=33)
    base, _ = _timescale(bz, M, formulation, "before the halos are poisoned")
    for value in (1e30, float("nan")):
        _poison_halos([M.hm.velocities[k] for k in VELOCITIES], value)
        assert bz.cell_advection_timescale(M.hm, formulation) == base, value
    w = M.hm.velocities["w"]
    keep = w.interior[-1].clone()
    w.interior[-1] = float("nan")            # face Nz belongs to no cell k = 0 .. Nz - 1
    assert bz.cell_advection_timescale(M.hm, formulation) == base
    w.interior[-1] = keep


@pytest.mark.parametrize("name,real", MODELS, ids=IDS)
def test_timescale_special_values(bz, zoo, name, real):
    M = zoo(name, real)
    Nx, Ny, Nz = M.N
    for k in VELOCITIES:
        M.hm.velocities[k].parent.zero_()
    for formulation in FORMULATIONS:
        assert bz.cell_advection_timescale(M.hm, formulation) == np.inf          # at rest
    M.velocities(bz, seed=34)
    for key, p in (("u", (min(5, Nx - 1), min(2, Ny - 1), 1)), ("u", (0, 0, 0)), ("v", (Nx - 1, Ny - 1, Nz - 1)), ("w", (Nx - 1, Ny - 1, Nz - 1))):
        if key == "v" and Ny == 1:
            continue
        with _planted(M.hm.velocities[key], p, value=float("nan")):
            got = bz.cell_advection_timescale(M.hm)
            assert got == 0.0 and not np.signbit(got), (key, p, got)          # a NaN velocity: timescale exactly 0
            if key != "w":
                assert bz.cell_advection_timescale(M.hm, "Horizontal") == 0.0


# ---- NaN check -----------------------------------------------------------------------------------------------------------------------
def _any_nan(hm, field, z_face):
    out = C.c_int32(-1)
    hm._check(hm._lib.bz_any_nan(hm._ctx, C.c_void_p(field.ptr()), z_face, C.byref(out)), "bz_any_nan")
    assert out.value in (0, 1)
    return bool(out.value)


def _nan_checks(bz, M):
    """(label, field, levels of its interior that the check covers, the check)"""
    hm, Nz = M.hm, M.N[2]
    return [("nan_checker ρu", hm.momentum["ρu"], Nz, lambda: bz.nan_checker(hm)),
            ("bz_any_nan ρw z_face=1", hm.momentum["ρw"], Nz + 1, lambda: _any_nan(hm, hm.momentum["ρw"], 1)),
            ("bz_any_nan ρθ z_face=0", hm.potential_temperature_density, Nz, lambda: _any_nan(hm, hm.potential_temperature_density, 0))]


@pytest.mark.parametrize("name,real", MODELS, ids=IDS)
def test_nan_check_sees_every_interior_cell_and_nothing_else(bz, zoo, name, real):
    import torch
    M = zoo(name, real)
    hm, g = M.hm, M.og
    Nx, Ny, Nz = M.N
    rng = np.random.default_rng(41)
    assert list(hm.prognostic_fields())[0] == "ρu"
    for label, f, nlev, check in _nan_checks(bz, M):
        f.parent.copy_(torch.from_numpy(rng.standard_normal(tuple(f.parent.shape))).to(f.dtype))          # halos hold numbers too
        assert check() is False, label
        where = positions(Nx, Ny, Nz) + ([(i, j, Nz) for i in (0, Nx - 1) for j in (0, Ny - 1)] if nlev == Nz + 1 else [])
        for p in where:
            with _planted(f, p, value=float("nan")):
                assert check() is True, (label, p)
        assert check() is False, label
        for value in (float("inf"), float("-inf")):
            with _planted(f, (Nx - 1, Ny - 1, Nz - 1), value=value):
                assert check() is False, (label, value)
        # NaN outside the interior: every x-halo column of the interior rows, every y-halo row, every z-halo level
        keep = f.parent.clone()
        k0, k1, j0, j1, i0, i1 = g.Hz, g.Hz + nlev, g.Hy, g.Hy + Ny, g.Hx, g.Hx + Nx
        f.parent[k0:k1, j0:j1, :i0] = float("nan")
        f.parent[k0:k1, j0:j1, i1:] = float("nan")
        assert check() is False, (label, "x halos")
        f.parent.copy_(keep)
        f.parent[:, :j0, :] = float("nan")
        f.parent[:, j1:, :] = float("nan")
        assert check() is False, (label, "y halos")
        f.parent.copy_(keep)
        f.parent[:k0] = float("nan")
        f.parent[k1:] = float("nan")
        assert check() is False, (label, "z halos")
        f.parent.copy_(keep)
        assert int(torch.isnan(f.parent).sum()) == 0
    # the top face of a z-face field is the check's only with z_face = 1
    rw = hm.momentum["ρw"]
    with _planted(rw, (Nx // 2, Ny // 2, Nz), value=float("nan")):
        assert _any_nan(hm, rw, 1) is True
        assert _any_nan(hm, rw, 0) is False


def test_reductions_share_their_scratch_without_mixing_answers(bz, zoo):
    """timescale, NaN check and divergence all answer through ctx->d_scalar: in any order each says what it says alone"""
    M = zoo("70x9x12", F64)
    hm = M.hm
    M.momentum(seed=51)
    bz.update_state_(hm, compute_tendencies=False)
    rt = hm.potential_temperature_density
    with _planted(rt, (64, 8, 11), value=float("nan")):
        div, _, _ = _divergence(M, "alone")
        tau, _ = _timescale(bz, M, "ThreeDimensional", "alone")
        tau_h, _ = _timescale(bz, M, "Horizontal", "alone")
        assert _any_nan(hm, rt, 0) is True
        assert bz.nan_checker(hm) is False
        for _ in range(2):
            assert bz.cell_advection_timescale(hm) == tau
            assert _any_nan(hm, rt, 0) is True
            assert hm.max_abs_divergence() == div
            assert bz.nan_checker(hm) is False
            assert bz.cell_advection_timescale(hm, "Horizontal") == tau_h
            assert bz.nan_checker(hm) is False
            assert hm.max_abs_divergence() == div
            assert _any_nan(hm, rt, 0) is True
            assert bz.cell_advection_timescale(hm) == tau


# ---- compressible models -------------------------------------------------------------------------------------------------------------
def test_reductions_of_a_compressible_model(oracle, bz):
    """cell_advection_timescale and nan_checker take a CompressibleDynamics model as they stand: the velocities are fields of the same
    layout, and the first prognostic field is the dry density"""
    import torch
    size = (40, 12, 9)
    x, y, z = _ext(size)
    og = oracle.Grid(size, x=x, y=y, z=z)
    grid = bz.RectilinearGrid(size, x=x, y=y, z=z)
    dyn = bz.CompressibleDynamics(bz.SplitExplicitTimeDiscretization(), reference_potential_temperature=300.0)
    hm = bz.CompressibleAtmosphereModel(grid, dyn, advection=bz.WENO(order=5))
    rng = np.random.default_rng(61)
    for k in VELOCITIES:
        f = hm.velocities[k]
        f.parent.copy_(torch.from_numpy(rng.standard_normal(tuple(f.parent.shape))))
    eps = L(np.finfo(F64).eps)
    for formulation in FORMULATIONS:
        got = bz.cell_advection_timescale(hm, formulation)
        want = rr.advection_timescale(og, *(_np(hm.velocities[k]) for k in VELOCITIES), horizontal=formulation == "Horizontal")
        ratio = float(abs(L(got) - want) / (eps * want))
        print(f"REDUCTION timescale compressible 40x12x9 float64 {formulation} random: got {got:.17g} want {float(want):.17g} ratio {ratio:.3f}")
        assert ratio <= 8.0
    name, rho_d = next(iter(hm.prognostic_fields().items()))
    assert name == "ρᵈ"
    rho_d.parent.fill_(1.0)
    assert bz.nan_checker(hm) is False
    for p in ((0, 0, 0), (39, 11, 8), (17, 4, 3)):
        with _planted(rho_d, p, value=float("nan")):
            assert bz.nan_checker(hm) is True, p
    rho_d.parent[:, :, :grid.Hx] = float("nan")
    assert bz.nan_checker(hm) is False


# ---- moisture scan -------------------------------------------------------------------------------------------------------------------
def _one_moist_cell(bz, size, cell, before, after):
    """the backdoor procedure of test_dry_shortcut.py::test_moisture_that_appears_later_is_seen with the moisture in ONE cell"""
    from test_dry_shortcut import _model
    m = _model(bz, size=size)
    m.time_steps(2.0, before)
    i, j, k = cell
    rq = m.moisture_density
    rq.interior[k, j, i] = 1e-3 * float(m.dynamics.reference_state.density[m.grid.Hz + k])
    bz.fill_halo_regions_(m, rq)
    m.synchronize()
    first = int(np.flatnonzero(rq.parent.cpu().numpy().ravel())[0])          # the first element of the parent array the scan can find
    m.time_steps(2.0, after)
    m.synchronize()
    return m, first


def _scan_sees_one_cell(bz, monkeypatch, size, cell, before, after):
    from test_dry_shortcut import _equal
    monkeypatch.delenv("BZ_NO_DRY_SHORTCUT", raising=False)
    a, first = _one_moist_cell(bz, size, cell, before, after)
    monkeypatch.setenv("BZ_NO_DRY_SHORTCUT", "1")
    b, _ = _one_moist_cell(bz, size, cell, before, after)
    _equal(a, b)
    assert int(np.count_nonzero(a.moisture_density.interior_cpu())) > 1          # the cell's moisture has been advected
    return first


@pytest.mark.parametrize("corner", ["first", "last"])
def test_moisture_scan_sees_a_single_moist_cell(bz, monkeypatch, corner):
    size = (64, 16, 24)
    cell = (0, 0, 0) if corner == "first" else tuple(n - 1 for n in size)
    _scan_sees_one_cell(bz, monkeypatch, size, cell, 2, 2)


def test_moisture_scan_sees_a_cell_of_its_second_pass(bz, monkeypatch):
    """k_scan_moisture runs 8 blocks of 256 threads per compute unit and strides over the parent array: at 128 x 64 x 64 (134 x 70 x 70 =
    656 600 elements with halos) the last interior cell and every halo copy of it lie beyond the first pass of a 256-unit device"""
    import torch
    size = (128, 64, 64)
    first_pass = torch.cuda.get_device_properties(0).multi_processor_count * 2048
    if not 134 * 70 * 70 > first_pass:
        pytest.skip(f"the scan covers {first_pass} elements in one pass on this device: 656 600 elements take no second pass")
    first = _scan_sees_one_cell(bz, monkeypatch, size, tuple(n - 1 for n in size), 1, 1)
    assert first >= first_pass, (first, first_pass)
