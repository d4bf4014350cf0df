"""Restatement of the reference's negative moisture correction (src/AtmosphereModels/negative_moisture_correction.jl:199-347) in typed
numpy, Float64 and Float32: a literal transcription of the column kernel's loops, one numpy operation per reference operation, with the
read-modify-write through memory and k_top = min(2, Nz).  Columns are the trailing axes: every array is (Nz, ...), level 0 the bottom.

    phase 1, every level (SpeciesBorrowing only): along heaviest -> ... -> lightest -> moisture prognostic, each neighbouring pair
        q_h = rho q_h / rho, q_l = rho q_l / rho, sink = q_h < 0 ? min(-q_h, max(0, q_l)) : 0, rho q_h += rho sink, rho q_l -= rho sink
    orphaned numbers: number = 0 where its mass <= 0;   clamp: number = max(0, number)
    phase 2 (VerticalBorrowing): for k = Nz .. 2: deficit = rho q[k] / rho[k] < 0 ? -rho q[k] dz[k] : 0, rho q[k] += deficit / dz[k],
        rho q[k - 1] -= deficit / dz[k - 1]; then the bottom borrows min(-rho q[1] dz[1], rho q[2] dz[2]) from level 2 if q[1] < 0 < q[2]

min and max are Julia's (a NaN operand gives a NaN, max(0, -0) = +0); every comparison with a NaN is false, so a NaN cell passes through.
The device kernel (csrc/bz_negative_moisture.hip) fuses the phases into one downward pass with the same operations per cell in the
same order, uncontracted: its results are these bits.

Also here: the columns a device model holds (device_columns), the populations of the kernel tests (populations), the moist bubble with
planted negative cells of the step tests (planted_bubble) and a mixin that makes the oracle models apply the correction to the interior
of rho q at the head of update_state (corrected)."""
import numpy as np


def jl_max(a, b):
    """Base.max on floats: diff = a - b; a NaN operand -> diff (a NaN); else signbit(diff) ? b : a"""
    diff = a - b
    return np.where(np.isnan(a) | np.isnan(b), diff, np.where(np.signbit(diff), b, a))


def jl_min(a, b):
    diff = a - b
    return np.where(np.isnan(a) | np.isnan(b), diff, np.where(np.signbit(diff), a, b))


def fix_negative_moisture(rq, rho, dz, species=False, vertical=False, mass=(), pairs=(), numbers=()):
    """_fix_negative_moisture_column! on every column of rq (Nz, ...), IN PLACE, in rq's own dtype.  rho, dz: (Nz,) columns.
    species: SpeciesBorrowing (mass: the species chain heaviest first, pairs: (number, mass) arrays, numbers: the clamped number fields;
    all modified in place); vertical: the scheme's vertical borrowing.  VerticalBorrowing alone: species = False, the lists are not looked at."""
    T = rq.dtype.type
    Nz = rq.shape[0]
    assert all(a.dtype == rq.dtype and a.shape == rq.shape for a in (*mass, *numbers, *(x for p in pairs for x in p)))
    rho, dz = np.asarray(rho, dtype=rq.dtype), np.asarray(dz, dtype=rq.dtype)
    assert rho.shape == (Nz,) and dz.shape == (Nz,)
    zero = T(0)
    with np.errstate(all="ignore"):
        if species:
            chain = (*mass, rq)
            for k in range(Nz):                                      # Phase 1: species borrowing at each level
                r = rho[k]
                for heavy, light in zip(chain[:-1], chain[1:]):
                    q_heavy = heavy[k] / r
                    q_light = light[k] / r
                    sink = np.where(q_heavy < 0, jl_min(-q_heavy, jl_max(np.full_like(q_light, zero), q_light)), zero).astype(rq.dtype)
                    heavy[k] = heavy[k] + r * sink
                    light[k] = light[k] - r * sink
            for k in range(Nz):                                      # zero orphaned numbers
                for n, m in pairs:
                    n[k] = np.where(m[k] <= 0, zero, n[k])
            for k in range(Nz):                                      # clamp negative numbers
                for f in numbers:
                    f[k] = jl_max(np.full_like(f[k], zero), f[k])
        if vertical:
            for k in range(Nz - 1, 0, -1):                           # k = Nz : -1 : 2 of the reference
                v = rq[k].copy()
                q = v / rho[k]
                deficit = np.where(q < 0, -v * dz[k], zero).astype(rq.dtype)
                rq[k] = rq[k] + deficit / dz[k]
                rq[k - 1] = rq[k - 1] - deficit / dz[k - 1]
            k_bot, k_top = 0, min(2, Nz) - 1
            v_bot, v_top = rq[k_bot].copy(), rq[k_top].copy()
            q_bot, q_top = v_bot / rho[k_bot], v_top / rho[k_top]
            can_borrow = (Nz >= 2) & (q_bot < 0) & (q_top > 0)
            needed = -v_bot * dz[k_bot]
            available = v_top * dz[k_top]
            dq = np.where(can_borrow, jl_min(needed, available), zero).astype(rq.dtype)
            rq[k_bot] = rq[k_bot] + dq / dz[k_bot]
            rq[k_top] = rq[k_top] - dq / dz[k_top]
    return rq


def column_mass(rq, dz):
    """sum_k rho q dz and sum_k |rho q| dz per column, in float64 (NaN columns give NaN)"""
    w = np.asarray(dz, dtype=np.float64).reshape((-1,) + (1,) * (rq.ndim - 1))
    a = rq.astype(np.float64)
    return (a * w).sum(axis=0), (np.abs(a) * w).sum(axis=0)


def conservation_bound(rq_before, dz):
    """(Nz + 2) eps sum_k |rho q| dz of the field BEFORE the correction: every cell is written at most three times (its own deficit, the
    deficit it receives, the bottom step), each write one rounding of a value no larger than the column's absolute mass"""
    eps = np.finfo(rq_before.dtype).eps
    return (rq_before.shape[0] + 2) * eps * column_mass(rq_before, dz)[1]


# ---- what a device model holds ---------------------------------------------------------------------------------------------------------------
def device_columns(hm):
    """(rho_r, dz) of the interior levels as the context of a device model holds them, in the grid's precision: the reference density the
    model handed over, and dz from the face heights the way bz_create forms it (a regular grid carries the one number Lz / Nz)"""
    g = hm.grid
    T = g.float_type
    rho = np.asarray(hm._ref_arrays[0], dtype=T)[g.Hz:g.Hz + g.Nz].copy()
    zf = np.ascontiguousarray(g.zᶠ, dtype=T)
    if g.regular_z:
        dz = np.full(g.Nz, (zf[g.Nz] - zf[0]) / T(g.Nz), dtype=T)
    else:
        dz = (zf[1:] - zf[:-1]).astype(T)
    return rho, dz


def stretched_faces(Nz, Lz=4096.0):
    """Nz + 1 face heights with growing, dyadic spacings (exact in Float32 too): dz[k] proportional to 1 + k"""
    w = np.arange(1, Nz + 1, dtype=np.float64)
    unit = 2.0 ** np.floor(np.log2(Lz / w.sum()))
    return np.concatenate(([0.0], np.cumsum(w * unit)))


POPULATIONS = ("positive", "top", "middle", "bottom", "cascade", "bottom-enough", "bottom-too-little", "bottom-nothing", "all-negative",
               "nan", "minus-zero", "random")


def populations(shape, rho, dtype, seed=5):
    """rho q of shape (Nz, Ny, Nx) with one population per column, cycling through POPULATIONS along x + 3 y -> (field, tag (Ny, Nx))"""
    Nz, Ny, Nx = shape
    rng = np.random.default_rng(seed)
    base = (2e-3 + 1.5e-2 * rng.random(shape)) * np.asarray(rho, dtype=np.float64)[:, None, None]
    tag = (np.arange(Nx)[None, :] + 3 * np.arange(Ny)[:, None]) % len(POPULATIONS)
    f = base.copy()
    mid = Nz // 2
    for j in range(Ny):
        for i in range(Nx):
            c = f[:, j, i]
            name = POPULATIONS[tag[j, i]]
            if name == "top":
                c[Nz - 1] = -3e-3
            elif name == "middle":
                c[mid] = -4e-3
            elif name == "bottom":
                c[0] = -2e-3
            elif name == "cascade":
                c[1:] = -np.abs(c[1:]) * 0.25
                c[0] = 1e-3
            elif name == "bottom-enough":
                c[0], c[1] = -1e-3, 5e-2
            elif name == "bottom-too-little":
                c[0], c[1] = -5e-2, 1e-3
            elif name == "bottom-nothing":
                c[0], c[1] = -5e-3, 0.0
            elif name == "all-negative":
                c[:] = -np.abs(c)
            elif name == "nan":
                c[mid] = np.nan
                c[Nz - 1] = -1e-3
            elif name == "minus-zero":
                c[Nz - 1], c[mid], c[0] = -0.0, -0.0, -0.0
            elif name == "random":
                c[:] = (rng.random(Nz) - 0.4) * 1e-2
    return f.astype(dtype), tag


def same_bits(a, b):
    """equal bit for bit where neither is a NaN, and NaN in the same places"""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    u = np.uint64 if a.dtype == np.float64 else np.uint32
    nan = np.isnan(a)
    return bool(np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(u)[~nan], b.view(u)[~nan]))


# ---- the step tests' state and oracle ----------------------------------------------------------------------------------------------------------
def plant_negatives(qt):
    """cells of q^t < 0 in a (Nz, Ny, Nx) field: at the top and below it, two stacked at the top (a cascade through the dry upper levels),
    next to the bottom, and at the bottom with enough and with too little above (the last stays negative through every step)"""
    Nz, Ny, Nx = qt.shape
    q = qt.copy()
    q[Nz - 1, 0, 1] = -2e-3
    q[Nz - 2, Ny // 2, 5] = -1e-3
    q[Nz - 1, Ny - 1, Nx - 1] = q[Nz - 2, Ny - 1, Nx - 1] = -3e-3
    q[1, 0, 3] = -4e-3
    q[0, Ny // 2, 7] = -5e-2
    q[0, 0, Nx - 2] = -1e-3
    return q


def corrected(base, species=False, vertical=True):
    """A subclass of an oracle model class (OracleModel, MixedPhaseOracleModel) whose update_state opens with fix_negative_moisture! on the
    interior of rho q, as the reference's update_state! does; `negative_cells` records how many cells each call found with q < 0."""

    class Corrected(base):
        def __init__(self, *a, **kw):
            self.negative_cells = []
            super().__init__(*a, **kw)

        def update_state(self, compute_tendencies=True):
            g = self.grid
            rho, dz = self.ref.density[g.Hz:g.Hz + g.Nz], g.dzc[g.Hz:g.Hz + g.Nz]
            interior = g.interior(self.rq)
            self.negative_cells.append(int((interior / rho[:, None, None] < 0).sum()))
            fix_negative_moisture(interior, rho, dz, species=species, vertical=vertical)
            super().update_state(compute_tendencies)

    Corrected.__name__ = "Corrected" + base.__name__
    return Corrected


# the oracle pair of the step tests: a 10 km deep domain under theta_0 = 300 K (clear near the ground, liquid, mixed and ice above), a
# moist bubble in sheared wind, negative cells planted into q^t
PBP, FLAT, PBB = ("Periodic", "Periodic", "Bounded"), ("Periodic", "Flat", "Bounded"), ("Periodic", "Bounded", "Bounded")
DT, STEPS = 2.0, 3
STEP_TOL = 1e-9          # of each field's scale: the project's tolerance for anelastic whole steps against the oracle
TIER_TOL = 1e-12         # between the tier a model picks and each other tier


def extent(topology):
    return dict(x=(-4e3, 4e3), z=(0.0, 10e3)) if topology == FLAT else dict(x=(-4e3, 4e3), y=(-3e3, 3e3), z=(0.0, 10e3))


def oracle_model(oracle, size, phase="warm", corrected_run=True, topology=PBP, tracers=0):
    """OracleModel (warm phase) or MixedPhaseOracleModel with, if corrected_run, VerticalBorrowing at the head of update_state"""
    import mixed_phase_reference as mpr
    halo = (3, 3) if topology == FLAT else (3, 3, 3)
    og = oracle.Grid(size, topology=topology, halo=halo, **extent(topology))
    base = mpr.MixedPhaseOracleModel if phase == "mixed" else oracle.OracleModel
    cls = corrected(base) if corrected_run else base
    return cls(og, potential_temperature=300.0, advection="WENO5", tracers=tracers, microphysics="SaturationAdjustment")


def planted_bubble(og, amplitude=1.5, wind=1.0):
    """the moist bubble's (theta, q^t with planted negative cells, u) on the oracle grid's nodes"""
    x, y, z = og.nodes("ccc")
    Lx = 8e3
    r2 = (x / 2500.0) ** 2 + ((y / 2500.0) ** 2 if og.Ny > 1 else 0.0) + ((z - 4500.0) / 2500.0) ** 2
    shape = (og.Nz, og.Ny, og.Nx)
    qt = np.broadcast_to(0.019 * np.exp(-z / 2600.0) * (1.0 + 0.15 * np.exp(-r2) + 0.05 * np.sin(2 * np.pi * x / Lx)), shape).copy()
    th = np.broadcast_to(300.0 + 1.0e-4 * z + amplitude * np.exp(-r2), shape).copy()
    u = np.broadcast_to(wind * (3.0 + 1.0 * np.sin(2 * np.pi * x / Lx) * np.cos(np.pi * z / 10e3)), shape).copy()
    return dict(theta=th, qt=plant_negatives(qt), u=u)


def tracer_density(om, ic):
    g = om.grid
    return om.ref.density[g.Hz:g.Hz + g.Nz][:, None, None] * (1.0 + 0.5 * np.tanh(ic["theta"] - 300.5))


def set_oracle(om, tracer=False, plant=True, **kw):
    ic = planted_bubble(om.grid, **kw)
    if not plant:
        ic["qt"] = np.abs(ic["qt"])
    om.set(qt=ic["qt"], theta=ic["theta"], u=ic["u"], **({"rc0": tracer_density(om, ic)} if tracer else {}))
    return ic
